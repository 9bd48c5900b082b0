"""tests/loop_shape_workloads.py on the host: every family reaches the branch of ndt_sessions_find_loops its row names, on
replay.PointCloudMap's bookkeeping with the odometry's prediction as the poses, the pre-filter's host model and, where clouds
or exact poses are needed, session_helpers.OracleSessions.  These are conditions on the workloads, not measurements; the
device run (tests/test_gpu_loop_shapes.py) must show the same candidates on the composed chain.  No GPU."""
import itertools

import numpy as np
import pytest

import loop_shape_workloads as L
import session_schedules as SS
import session_workloads as W
from loops_helpers import robot_frame
from session_helpers import OracleSessions, lockstep

_RUNS = {}


def host(name):
    if name not in _RUNS:
        _RUNS[name] = L.host_run(L.family(name))
    return _RUNS[name]


def oracle_run(oracle, fam, upto=None):
    """The family's classes on OracleSessions (the reference's prediction arithmetic, real clouds) -> the model."""
    from ndt_slam_amd import capi
    model = OracleSessions(oracle, capi, len(fam["logs"]), fam["p"], allow_item_failures=fam["tolerant"])
    for k, scans, odo, act in lockstep(fam["logs"], fam["starts"]):
        model.step(scans, odo, act)
        if k == upto:
            break
    return model


@pytest.mark.parametrize("name", sorted(L.FAMILIES))
def test_every_call_of_every_family_has_the_candidates_it_names(name):
    fam = L.family(name)
    cands, _ = host(name)
    assert len(cands) == len(fam["calls"]) >= 1 and len(fam["logs"]) <= 6
    assert max(s + len(log[0]) for s, log in zip(fam["starts"], fam["logs"])) <= 16
    assert fam["p"]["score_thre"] == -1.0 and 1.0 <= fam["p"]["sepThre"] <= 1.5
    for call, got in zip(fam["calls"], cands):
        assert len(call["which"]) == len(fam["cls"]) and any(call["which"]), call["tag"]
        assert call["lp"]["min_path"] in (0.0, 1.0) and call["lp"]["radius"] >= 10.0
        assert all(c is not None for c in got.values()), (name, call["tag"], got)        # every named session has a candidate
        assert all(c["submap"] == (call["k"] - fam["starts"][i]) // 2 - 2 or name in ("later_submap", "many", "zero_pose")
                   for i, c in got.items()), (name, call["tag"])


def test_ragged_filtered_lengths_are_pairwise_different_across_the_wave_boundaries():
    fam = L.family("ragged")
    assert len(fam["logs"]) >= 6 and [len(log[0][-1]) for log in fam["logs"]] == list(L.RAGGED) and fam["calls"][0]["lp"]["top_k"] == 8
    _, pms = host("ragged")
    sizes = [L.stored_and_filtered(fam, c, SS.host_poses(pms[c])[-1]) for c in range(len(fam["logs"]))]
    stored, filtered = [s for s, _ in sizes], [f for _, f in sizes]
    print("ragged: stored %s, filtered %s" % (stored, filtered))
    assert len(set(filtered)) == len(filtered) and filtered[0] == 1
    assert all(a != b for a, b in itertools.combinations(filtered, 2))
    # the prefixes K * o0 of the candidates cross a wave (64) and a workgroup (256) inside the call
    off = np.cumsum([0] + filtered)
    assert any(0 < o < 64 for o in off) and any(o % 64 for o in off[1:]) and any(f > 256 for f in filtered) and any(f < 64 for f in filtered)


def test_dead_slots_lattices_are_smaller_than_top_k():
    fam = L.family("dead_slots")
    nine, one = fam["calls"]
    for call, poses in ((nine, 9), (one, 1)):
        hx, hy, hk = call["lp"]["half"]
        assert (2 * hx + 1) * (2 * hy + 1) * (2 * hk + 1) == poses and call["lp"]["top_k"] == 8 and call["lp"]["local_max"] == 1
    # (n_cand itself is the device certificate: 0 < n_cand < 8 and n_cand <= 1, on the composed reference)


def test_nothing_picked_passes_the_gate_with_a_scan_far_from_every_map():
    fam = L.family("nothing_picked")
    far = fam["far"]
    (both, neighbours), pms = host("nothing_picked")
    assert sorted(both) == [0, 1, 2] and sorted(neighbours) == [0, 2] and both[far]["submap"] == 0
    clean = L._logs(((34, 6),))[0][0][5]
    moved = fam["logs"][far][0][5]
    assert moved.shape == clean.shape
    assert np.allclose(moved - clean, [L.FAR, 0.0]) and len(moved) > 100
    # robot frame: every point is more than 400 m from the drive, whose maps end within 30 m of it (the lidar's range)
    assert np.all(np.hypot(moved[:, 0], moved[:, 1]) > 400.0)
    assert all(np.hypot(*SS.host_poses(pm)[-1][:2]) < 20.0 for pm in pms)


def test_empty_newest_names_candidates_whose_last_scan_is_empty():
    fam = L.family("empty_newest")
    (mixed, only), _ = host("empty_newest")
    assert sorted(mixed) == [0, 1, 2, 3] and sorted(only) == sorted(fam["empty"]) == [1, 2]
    assert all(len(fam["logs"][i][0][-1]) == (0 if i in fam["empty"] else L.BEAMS) for i in range(4))
    assert fam["calls"][1]["which"] == [0, 1, 1, 0]
    # the step with the empty scan is no split step: the candidate is the one its neighbours have
    assert {c["submap"] for c in mixed.values()} == {0}


def test_later_submap_picks_four_different_submaps_in_one_call():
    fam = L.family("later_submap")
    (got,), pms = host("later_submap")
    assert [got[c]["submap"] for c in range(4)] == fam["submaps"] == [0, 1, 2, 3]
    assert [len(pm.submaps) - 1 for pm in pms] == [2, 3, 4, 5]                   # closed submaps: two drives have four and more


@pytest.mark.parametrize("name,bad", [("refused_first", 0), ("refused_middle", 1)])
def test_refused_families_carry_the_outlier_in_the_first_closed_cloud_of_one_candidate(name, bad):
    fam = L.family(name)
    (got,), pms = host(name)
    assert fam["bad"] == bad and sorted(got) == [0, 1, 2] and all(c["submap"] == 0 for c in got.values())
    for i in range(3):
        has = any(tuple(pt) == W.GRID_OUTLIER for pt in fam["logs"][i][0][0])
        assert has == (i == bad)
        assert not any((np.abs(s) > 100).any() for s in fam["logs"][i][0][1:])
    # submap 0 owns the scans 0 and 1; its cloud's box at the match resolution is beyond 2^28 cells
    assert SS.layout(pms[bad])[0][:2] == [0, 2]
    assert (W.GRID_OUTLIER[0] / fam["p"]["Resolution"]) ** 2 > 2 ** 28


def test_map_reuse_meets_three_clouds_of_different_sizes_the_second_smaller(oracle):
    fam = L.family("map_reuse")
    cands, _ = host("map_reuse")
    assert [c[0]["submap"] for c in cands] == fam["submaps"] == [0, 2, 4] and [c["k"] for c in fam["calls"]] == [5, 9, 13]
    assert len(fam["logs"][0][0]) > 14                                          # steps are left behind the last search
    model = oracle_run(oracle, fam)
    sizes = [len(model.pcmaps[0].submaps[m].p_cloud) for m in fam["submaps"]]
    print("map_reuse: candidate clouds of %s points" % sizes)
    assert len(set(sizes)) == 3 and sizes[1] < sizes[0] and sizes[2] > sizes[1]
    assert abs(sizes[1] - sizes[0]) > 50 and abs(sizes[2] - sizes[0]) > 50      # (not a matter of a last bit of a pose)


def test_picks_and_costs_is_the_whole_product():
    calls = L.family("picks_and_costs")["calls"]
    got = sorted((c["lp"]["top_k"], c["lp"]["local_max"], c["lp"]["max_cost"]) for c in calls)
    assert got == sorted(itertools.product((1, 8), (0, 1), (-L.INF, L.INF)))


def test_many_is_more_than_a_wave_of_candidates_from_five_logs():
    fam = L.family("many")
    (got,), _ = host("many")
    assert len(fam["cls"]) == 65 and len(fam["logs"]) == 5 and sorted(set(fam["cls"])) == [0, 1, 2, 3, 4]
    assert [got[c]["submap"] for c in range(5)] == fam["submaps"] and len(set(fam["submaps"])) == 3
    assert fam["calls"][0]["lp"]["top_k"] == 8 and all(fam["calls"][0]["which"])
    assert len({fam["cls"][i] for i in (0, 63, 64)}) >= 2                        # the wave's last and the next candidate differ


def test_zero_pose_reaches_the_bit_pattern_of_zero_in_the_references_arithmetic(oracle):
    fam = L.family("zero_pose")
    z = fam["zero"]
    model = oracle_run(oracle, fam)
    pm = model.pcmaps[z]
    poses = np.array([(q.tx, q.ty, q.th) for q in pm.poses], np.float64)
    assert poses[:, 0].tolist() == list(L.ZERO_X) and not poses[:, 1:].any()
    assert poses[-1].tobytes() == np.zeros(3).tobytes()                         # +0.0 three times, not -0.0
    (got,), pms = host("zero_pose")
    assert got[z]["submap"] == 0 and got[z]["dist"] == 0.0 and len(pms[z].submaps) - 1 == 4
    # with that pose the robot frame is the stored scan's bytes (ndt_repose_points' rule, M.same in loop_scan_kernel)
    stored = np.ascontiguousarray(pm.submaps[-1].scans[-1], np.float32).reshape(-1, 2)
    assert len(stored) and robot_frame(stored, poses[-1]).tobytes() == stored.tobytes()
    assert robot_frame(stored, (0.0, -0.0, 0.0)).shape == stored.shape          # (a -0.0 would take the arithmetic path)
