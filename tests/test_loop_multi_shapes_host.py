"""tests/loop_multi_shape_workloads.py on the host: every family reaches the branch of ndt_sessions_find_loops_multi /
ndt_sessions_find_cross_loops its row names, on replay.PointCloudMap's bookkeeping with the odometry's prediction as the poses
(session_schedules.host_map / host_add), the numpy gates (loops_multi_helpers.gate_multi_ref, cross_loops_helpers.cross_gate_ref),
the pre-filter's host model and, where clouds or exact poses are needed, session_helpers.OracleSessions.  These are conditions
on the workloads, not measurements; the device run (tests/test_gpu_loop_multi_shapes.py) must show the same candidates on the
composed chain, and checks the certificates that are statements about picks and decisions.  No GPU."""
import itertools

import numpy as np
import pytest

import loop_multi_shape_workloads as M
import loop_shape_workloads as L
import session_schedules as SS
import session_workloads as W
from loops_helpers import robot_frame
from session_helpers import to_map_frame
from test_loop_shapes_host import oracle_run

_RUNS = {}


def host(name):
    if name not in _RUNS:
        from ndt_slam_amd import capi
        _RUNS[name] = M.host_run(capi, M.family(name))
    return _RUNS[name]


def per_searcher(cands, S):
    return [[c for c in cands if c[0] == i] for i in range(S)]


@pytest.mark.parametrize("name", sorted(M.FAMILIES))
def test_every_call_of_every_family_has_candidates_in_rank_order(name):
    fam = M.family(name)
    cands, _ = host(name)
    assert len(cands) == len(fam["calls"]) >= 1 and len(fam["logs"]) <= 6
    assert max(s + len(log[0]) for s, log in zip(fam["starts"], fam["logs"])) <= 16
    assert fam["p"]["score_thre"] == -1.0 and fam["p"]["sepThre"] == 1.0
    assert [c["k"] for c in fam["calls"]] == sorted(c["k"] for c in fam["calls"])
    for call, got in zip(fam["calls"], cands):
        kind = M.kind_of(call)
        assert len(call["which"]) == len(fam["cls"]) and any(call["which"]) and got, call["tag"]
        assert call["lp"]["min_path"] == 0.0 and call["lp"]["radius"] == 10.0 and call["lp"]["half"] == (2, 2, 1)
        assert kind == "single" or 1 <= call["mp"]["max_submaps"] <= 4
        assert (kind == "cross") == ("against" in call)
        # a searcher's candidates lie in a row, rank 0, 1, ...; only a cross candidate has another owner
        assert [c[0] for c in got] == sorted(c[0] for c in got)
        for mine in per_searcher(got, len(fam["cls"])):
            assert [c[1] for c in mine] == list(range(len(mine))) and len(mine) <= (1 if kind == "single" else call["mp"]["max_submaps"])
        assert all((c[0] != c[2]) == (kind == "cross") for c in got)


def test_ragged_ranks_has_one_to_four_candidates_per_session_and_four_filtered_lengths():
    fam = M.family("ragged_ranks")
    (got,), pms = host("ragged_ranks")
    mine = per_searcher(got, 4)
    assert [len(m) for m in mine] == fam["per_session"] == [1, 2, 3, 4]
    assert [[c[3] for c in m] for m in mine] == fam["submaps"] == [[0], [1, 0], [2, 1, 0], [3, 2, 1, 0]]
    assert [len(log[0][-1]) for log in fam["logs"]] == list(M.RANK_CUTS) == [1, 63, 65, 257]
    sizes = [L.stored_and_filtered(fam, c, SS.host_poses(pms[c])[-1]) for c in range(4)]
    filtered = [f for _, f in sizes]
    print("ragged_ranks: stored %s, filtered %s" % ([s for s, _ in sizes], filtered))
    assert len(set(filtered)) == 4 and filtered[0] == 1
    # before[0] of a candidate, summed over candidates and summed over scans: different for every candidate behind session 1's
    # second, and no candidate's K-fold prefix is another's
    per_cand = np.concatenate([[0], np.cumsum([filtered[c[0]] for c in got])])[:-1]
    scan_first = np.concatenate([[0], np.cumsum(filtered)])[:-1]
    per_scan = np.array([scan_first[c[0]] for c in got])
    assert (per_cand[2:] != per_scan[2:]).all() and len(set(per_cand[1:].tolist())) == len(got) - 1


def test_many_ranks_is_more_than_a_workgroup_of_candidates():
    fam = M.family("many_ranks")
    (got,), _ = host("many_ranks")
    cls = fam["cls"]
    assert len(cls) == 65 and cls == [(7 * i + 3) % 5 for i in range(65)] and sorted(set(cls)) == [0, 1, 2, 3, 4]
    assert len(got) == 260 > 256 and all(len(m) == fam["per_class"] == 4 for m in per_searcher(got, 65))
    assert len({(cls[c[0]], c[3]) for c in got}) == 20
    assert all(len(log[0]) == 12 for log in fam["logs"]) and fam["calls"][0]["mp"]["max_submaps"] == 4
    # the candidates 256 .. 259 are session 64's: the second trip of loop_guess_kernel's sum is theirs
    assert [c[0] for c in got[256:]] == [64] * 4


@pytest.mark.parametrize("name,bad,rank", [("refused_rank3", 1, 3), ("refused_rank0_first", 0, 0)])
def test_refused_ranks_carry_the_outlier_in_the_cloud_of_one_rank(name, bad, rank):
    fam = M.family(name)
    cands, pms = host(name)
    every, without = cands[:2]
    assert (fam["bad"], fam["bad_rank"]) == (bad, rank) and fam["tolerant"]
    for i in range(3):
        holds = [k for k, s in enumerate(fam["logs"][i][0]) if any(tuple(pt) == fam["outlier"] for pt in s)]
        assert holds == ([fam["bad_scan"]] if i == bad else []) and not any((np.abs(s) > 100).any() for k, s in enumerate(fam["logs"][i][0]) if k not in holds)
    firsts = SS.layout(pms[bad])[0]
    submap = max(m for m, f in enumerate(firsts) if f <= fam["bad_scan"])
    assert [c[1] for c in every if c[0] == bad and c[3] == submap] == [rank]
    assert len(every) == 12 and [c for c in every if c[0] != bad] == without and len(without) == 8
    # the point in the map frame, at the pose of its scan: the box of its cloud at the match resolution is beyond 2^28 cells
    x, y = to_map_frame(np.array([fam["outlier"]], np.float64), SS.host_poses(pms[bad])[fam["bad_scan"]])[0]
    print("%s: the outlier at (%.0f, %.0f) in the map frame, %.3g cells" % (name, x, y, abs(x * y) / fam["p"]["Resolution"] ** 2))
    assert (abs(x) - 30.0) * (abs(y) - 30.0) / fam["p"]["Resolution"] ** 2 > 2 ** 28
    if rank == 0:
        # the refused candidate is the call's first: every map that can stand in for it has rank >= 1 or belongs to a later session
        assert every[0][:2] == (bad, 0) and every[0][3] == submap
        assert cands[2] == [every[0]] and fam["calls"][2]["mp"]["max_submaps"] == 1


def test_slot_history_alternates_the_three_searches_on_shared_slots(oracle):
    fam = M.family("slot_history")
    cands, _ = host("slot_history")
    kinds = [M.kind_of(c) for c in fam["calls"]]
    assert set(kinds) == {"single", "multi", "cross"} and len({c["k"] for c in fam["calls"]}) == 3 and fam["twin"]
    assert [c["mp"]["max_submaps"] for c in fam["calls"] if M.kind_of(c) == "multi"][:3] == [4, 2, 4]
    assert max(len(log[0]) for log in fam["logs"]) - 1 > max(c["k"] for c in fam["calls"])       # steps are left behind the last search
    model = oracle_run(oracle, fam)
    size = lambda o, m: len(model.pcmaps[o].submaps[m].p_cloud)
    seq = {}
    for q, got in enumerate(cands):
        for s, r, o, m, _, _ in got:
            seq.setdefault((s, r), []).append((q, o, m))
    # a slot of rank >= 1 that meets three different cloud sizes, smaller and then larger again (the final clouds' sizes: a
    # closed cloud does not change behind its split)
    waves = {}
    for key, v in seq.items():
        n = [size(o, m) for _, o, m in v]
        if key[1] >= 1 and len(set(n)) >= 3 and any(n[i] > n[i + 1] < n[i + 2] for i in range(len(n) - 2)):
            waves[key] = n
    foreign_then_own = [k for k, v in seq.items() if any(v[i][1] != k[0] and v[i + 1][1] == k[0] for i in range(len(v) - 1))]
    print("slot_history: sizes met by the slots whose cloud shrinks and grows %s; another session's cloud, then its own: %s" % (waves, foreign_then_own))
    assert waves and foreign_then_own
    # the thinned scans are one closed submap's own
    firsts = SS.layout(host("slot_history")[1][0])[0]
    assert [k for c, k in M.HISTORY_THIN if c == 0] == list(range(firsts[2], firsts[3]))


def test_cross_owners_has_a_searcher_that_is_no_track_and_a_track_that_does_not_search():
    fam = M.family("cross_owners")
    (pair, every), pms = host("cross_owners")
    assert [len(pm.submaps) - 1 for pm in pms] == fam["closed"] == [2, 0, 5, 1]
    B, C = fam["not_a_track"], fam["silent_track"]
    for got in (pair, every):
        assert any(c[0] == B for c in got) and all(c[2] != B for c in got)
    assert fam["calls"][1]["which"][C] == 0 and any(c[2] == C for c in every) and all(c[0] != C for c in every)
    counts = lambda got: sorted({len(m) for m in per_searcher(got, 4)} - {0})
    assert counts(pair) == [1, 2, 3] and counts(every) == [4]
    for got in (pair, every):
        named = [(c[2], c[3]) for c in got]
        assert any(named.count(x) >= 2 for x in named)                          # two searchers, one (map_session, submap)
    assert any(c[4] > c[5] for c in every) and any(c[4] > c[5] for c in pair)  # the owner's trajectory is the longer one
    assert len(pms[C].submaps) - 1 > len(pms[B].poses)                         # more closed submaps than the searcher has scans
    # no two sessions share a pose at a scan of the same number
    poses = [SS.host_poses(pm) for pm in pms]
    for a, b in itertools.combinations(range(4), 2):
        n = min(len(poses[a]), len(poses[b]))
        assert (np.abs(poses[a][:n, :2] - poses[b][:n, :2]).max(axis=1) > 0.01).all(), (a, b)


def test_cross_refused_empty_names_the_refused_cloud_twice_and_an_empty_searcher():
    fam = M.family("cross_refused_empty")
    (every, without, only), pms = host("cross_refused_empty")
    bad, e = fam["bad"], fam["empty"]
    assert any(tuple(pt) == W.GRID_OUTLIER for pt in fam["logs"][bad][0][0]) and SS.layout(pms[bad])[0][:2] == [0, 2]
    on_bad = [c for c in every if (c[2], c[3]) == (bad, fam["bad_submap"])]
    assert len(on_bad) == 2 and len({c[0] for c in on_bad}) == 2
    assert len(fam["logs"][e][0][-1]) == 0 and all(len(fam["logs"][i][0][-1]) == L.BEAMS for i in range(3) if i != e)
    assert len([c for c in every if c[0] == e]) == 4 and fam["calls"][2]["which"] == [1 if i == e else 0 for i in range(3)]
    assert only == [c for c in every if c[0] == e]
    assert fam["calls"][1]["against"] == [0 if i == bad else 1 for i in range(3)] and all(c[2] != bad for c in without)
    pairs = lambda got: sorted((c[0], c[2], c[3]) for c in got)
    assert pairs(without) == pairs(c for c in every if c[2] != bad)


def test_cross_zero_pose_searches_from_the_bit_pattern_of_zero(oracle):
    fam = M.family("cross_zero_pose")
    z = fam["zero"]
    (got,), _ = host("cross_zero_pose")
    assert any(c[0] == z for c in got) and all(c[2] == 1 - c[0] for c in got)
    model = oracle_run(oracle, fam)
    pm = model.pcmaps[z]
    poses = np.array([(q.tx, q.ty, q.th) for q in pm.poses], np.float64)
    assert poses[-1].tobytes() == np.zeros(3).tobytes()                         # +0.0 three times, not -0.0
    stored = np.ascontiguousarray(pm.submaps[-1].scans[-1], np.float32).reshape(-1, 2)
    assert len(stored) and robot_frame(stored, poses[-1]).tobytes() == stored.tobytes()


def test_decisions_is_the_whole_grid():
    fam = M.family("decisions")
    cands, _ = host("decisions")
    got = sorted((c["mp"]["min_overlap"], c["mp"]["max_d2"], c["lp"]["max_cost"], c["lp"]["top_k"]) for c in fam["calls"][:54])
    assert all(c["lp"]["step_xy"] == 0.1 for c in fam["calls"][:54]) and all(c["lp"]["step_xy"] == 0.5 for c in fam["calls"][54:])
    assert got == sorted(itertools.product((0.0, 0.5, 1.0), (0.0, 0.09, M.DBL_MAX), (-M.INF, 0.02, M.INF), (1, 8))) and len(got) == 54
    assert all(len(c) == 5 and [len(m) for m in per_searcher(c, 2)] == [2, 3] for c in cands)
    assert [len(log[0]) for log in fam["logs"]] == [8, 10]
