"""The loop search without a GPU: the gating (ndt_loop_gate, the rule ndt_sessions_loop_candidates applies per session) against
its numpy restatement on hand-made trajectories and layouts, the whole search as a prototype on the CPU oracle, and the header's
prototypes in the binding."""
import math
import os
import re

import numpy as np
import pytest

from loops_helpers import (FULL_LAP, HALF_LAP, expected_pose, gate_ref, loop_params_dict, loop_workload, pose_gap, robot_frame,
                           same_candidate)
from reloc_helpers import ref_cost, relocalize_ref
from session_correct_helpers import layout
from session_helpers import OracleSessions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ndt_score_lattice_multi_dev", "ndt_lattice_select_multi_dev", "ndt_loop_default_params", "ndt_loop_gate",
       "ndt_sessions_loop_candidates", "ndt_sessions_find_loops")


@pytest.fixture(scope="module")
def capi():
    from ndt_slam_amd import build, capi
    build.build()
    return capi


def test_the_headers_prototypes_are_bound(capi):
    src = open(os.path.join(ROOT, "include", "ndt_mi355x.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, src), name
        assert name in capi.PROTOTYPES and hasattr(capi.lib(), name), name
    for word in ("ndt_score_job", "ndt_loop_params", "ndt_loop_candidate", "ndt_loop;", "NDT_LOOP_MAX_CAND 8"):
        assert word in src, word
    p = capi.default_loop_params()
    assert (p.min_path, p.radius, p.step_xy, p.step_yaw) == (10.0, 2.0, 0.1, 1.0 * math.pi / 180)
    assert (p.half_x, p.half_y, p.half_yaw, p.top_k, p.local_max, p.max_cost) == (10, 10, 6, 4, 1, 0.02)
    assert list(p.info) == [1e4, 0.0, 0.0, 1e4, 0.0, 1e4] and capi.NDT_LOOP_MAX_CAND == 8


# ------------------------------------------------------------------------------------------ the gating
def square_lap(side=6.0, step=0.75, back=0.0, jitter=0.003, seed=4):
    """A trajectory once round a square of `side` metres, `step` per scan, ending `back` metres short of the start."""
    rng = np.random.default_rng(seed)
    n = int((4 * side - back) / step) + 1
    poses = np.zeros((n, 3))
    for k in range(n):
        d = k * step
        leg, along = int(d // side) % 4, d % side
        poses[k, :2] = [(along, 0.0), (side, along), (side - along, side), (0.0, side - along)][leg]
        poses[k, 2] = 90.0 * leg
    poses[:, :2] += rng.normal(0.0, jitter, (n, 2))
    return poses


def even_layout(n, per):
    """Submaps of `per` scans; the last one is the current submap.  -> (sub_first, sub_anchor, sub_offsets of 100 points each)."""
    first = list(range(0, n, per))
    last = [f - 1 for f in first[1:]] + [n - 1]
    anchor = [a + (e - a) // 2 if e > a else a for a, e in zip(first, last)]
    return np.array(first, np.int32), np.array(anchor, np.int32), np.arange(len(first) + 1, dtype=np.uint64) * 100


def check_gate(capi, poses, first, anchor, off, p, want_submap):
    got = capi.loop_gate(poses, first, anchor, off, p)
    ref = gate_ref(poses, first, anchor, off, **loop_params_dict(p))
    if want_submap is None:
        assert got is None and ref is None
        return None
    assert got is not None and ref is not None and ref["submap"] == want_submap
    assert got["session"] == 0 and same_candidate(got, ref)
    return got


def test_gating_against_the_numpy_restatement(capi):
    p = capi.default_loop_params()
    poses = square_lap()
    first, anchor, off = even_layout(len(poses), 4)
    got = check_gate(capi, poses, first, anchor, off, p, 0)                  # back at the start: the first submap
    assert got["anchor_scan"] == anchor[0] and got["newest_scan"] == len(poses) - 1 and got["nearest_scan"] == 0
    assert got["dist"] < 0.1 and got["path"] > 20.0
    L = got["lattice"]
    assert (L["nx"], L["ny"], L["nyaw"]) == (21, 21, 13) and L["step_x"] == L["step_y"] == 0.1
    assert abs(L["x0"] + 10 * 0.1 - poses[-1, 0]) < 1e-12 and abs(L["yaw0"] + 6 * p.step_yaw - math.radians(poses[-1, 2])) < 1e-12
    # the lap 3 m short of the start: submap 0's scans are more than `radius` away, nothing else has the path
    short = square_lap(back=3.0)
    f2, a2, o2 = even_layout(len(short), 4)
    check_gate(capi, short, f2, a2, o2, p, None)
    check_gate(capi, short, f2, a2, o2, capi.default_loop_params(radius=3.2), 0)
    # fewer than two closed submaps; a trajectory of one scan
    for k in (1, 2):
        check_gate(capi, poses, first[:k], anchor[:k], off[:k + 1], p, None)
    check_gate(capi, poses[:1], first[:1], np.zeros(1, np.int32), off[:2], p, None)
    # the newest closed submap is never a candidate, however near: three submaps, the lap's end inside the second
    few = poses[:9]
    f9, a9, o9 = even_layout(9, 4)
    check_gate(capi, few, f9, a9, o9, capi.default_loop_params(min_path=0.0, radius=50.0), 0)
    check_gate(capi, few, f9[:2], a9[:2], o9[:3], capi.default_loop_params(min_path=0.0, radius=50.0), None)


def test_gating_ties_empty_ranges_and_empty_clouds(capi):
    p = capi.default_loop_params()
    poses = square_lap(jitter=0.0)
    first, anchor, off = even_layout(len(poses), 4)
    # two submaps tied on dist: scans 0 and 5 mirror-placed around the last pose; the lower one wins
    tied = poses.copy()
    tied[-1, :2] = (0.0, 0.0)
    tied[0, :2] = (0.6, 0.0); tied[5, :2] = (-0.6, 0.0)
    tied[4, :2] = (3.0, 0.3)                                                 # (scan 4 out of the way of submap 1's other scans)
    ref = gate_ref(tied, first, anchor, off, **loop_params_dict(p))
    got = check_gate(capi, tied, first, anchor, off, p, 0)
    assert got["dist"] == 0.6 and ref["nearest_scan"] == 0
    swapped = tied.copy()
    swapped[0, :2] = (0.6000001, 0.0)                                        # a hair further: now submap 1
    assert check_gate(capi, swapped, first, anchor, off, p, 1)["nearest_scan"] == 5
    # submap 0 with an empty closed cloud: the tie goes to submap 1
    hollow = off.copy()
    hollow[1:] -= 100
    assert check_gate(capi, tied, first, anchor, hollow, p, 1)["dist"] == 0.6
    # submap 0 with an empty scan range (it closed without a scan of its own): sub_first[1] == sub_first[0]
    f3 = np.concatenate([[0], first]).astype(np.int32)
    a3 = np.concatenate([[0], anchor]).astype(np.int32)
    o3 = np.arange(len(f3) + 1, dtype=np.uint64) * 100
    assert check_gate(capi, tied, f3, a3, o3, p, 1)["nearest_scan"] == 0    # (the old submap 0 is now submap 1)


def test_gating_bounds_are_inclusive(capi):
    poses = square_lap()
    first, anchor, off = even_layout(len(poses), 4)
    ref = gate_ref(poses, first, anchor, off, 0.0, 50.0, 0.1, 0.01, (1, 1, 1))
    assert ref["submap"] == 0 and ref["dist"] > 0.0
    at = dict(min_path=ref["path"], radius=ref["dist"])
    check_gate(capi, poses, first, anchor, off, capi.default_loop_params(**at), 0)            # path == min_path, dist == radius
    above = capi.default_loop_params(min_path=float(np.nextafter(ref["path"], np.inf)), radius=50.0)
    got = capi.loop_gate(poses, first, anchor, off, above)
    assert got is None or got["submap"] != 0
    below = capi.default_loop_params(min_path=0.0, radius=float(np.nextafter(ref["dist"], -np.inf)))
    got = capi.loop_gate(poses, first, anchor, off, below)
    assert got is None or got["submap"] != 0
    assert same_candidate_or_none(got, gate_ref(poses, first, anchor, off, **loop_params_dict(below)))


def same_candidate_or_none(got, ref):
    return (got is None and ref is None) or (got is not None and ref is not None and same_candidate(got, ref))


def test_gating_refusals(capi):
    poses = square_lap()
    first, anchor, off = even_layout(len(poses), 4)
    for kw, text in ((dict(min_path=-1.0), "negative or not finite"), (dict(radius=float("nan")), "negative or not finite"),
                     (dict(step_xy=float("inf")), "negative or not finite"), (dict(step_yaw=-0.1), "negative or not finite"),
                     (dict(half_x=-1), "a negative half extent"), (dict(half_yaw=-3), "a negative half extent"),
                     (dict(half_x=2048, half_y=2048, half_yaw=0), "more than 2^24 poses"), (dict(top_k=0), "top_k must be in 1 .. 8"),
                     (dict(top_k=9), "top_k must be in 1 .. 8"), (dict(max_cost=float("nan")), "max_cost is NaN")):
        with pytest.raises(capi.NdtError, match=re.escape(text)):
            capi.loop_gate(poses, first, anchor, off, capi.default_loop_params(**kw))
    p = capi.default_loop_params()
    bad = poses.copy(); bad[3, 1] = np.inf
    with pytest.raises(capi.NdtError, match="scan 3: a pose is not finite"):
        capi.loop_gate(bad, first, anchor, off, p)
    for f, a, o in ((first + 1, anchor, off), (first[::-1].copy(), anchor, off), (first, anchor + 1000, off), (first, anchor, off[::-1].copy())):
        with pytest.raises(capi.NdtError, match="is not a set's layout"):
            capi.loop_gate(poses, f, a, o, p)
    assert capi.lib().ndt_loop_gate(None, 1, None, None, None, 1, None, None, None) == capi.NDT_E_ARG
    # the set's own calls check the set first
    import ctypes
    n = ctypes.c_int()
    assert capi.lib().ndt_sessions_loop_candidates(None, None, ctypes.byref(p), None, ctypes.byref(n)) == capi.NDT_E_ARG
    assert capi.lib().ndt_last_error(None).decode() == "null session set"
    assert capi.lib().ndt_sessions_find_loops(None, None, ctypes.byref(p), None, ctypes.byref(n), None) == capi.NDT_E_ARG
    assert capi.lib().ndt_last_error(None).decode() == "null session set"


# ------------------------------------------------------------------------------------------ the prototype on the oracle
def oracle_run(oracle, capi, n_frames, **params):
    (scans, odo), truth, p = loop_workload(n_frames=n_frames, **params)
    ses = OracleSessions(oracle, capi, 1, p)
    for k in range(n_frames):
        ses.step([scans[k]], odo[k:k + 1])
    pm = ses.pcmaps[0]
    traj = np.array([(q.tx, q.ty, q.th) for q in pm.poses], np.float64)
    first, anchor, _ = layout(pm)
    clouds = [np.ascontiguousarray(s.p_cloud, np.float32).reshape(-1, 2) for s in pm.submaps[:-1]]
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds]), [0]]).astype(np.uint64)
    off[-1] = off[-2]                                                       # (the current submap's part is not looked at)
    return dict(p=p, pm=pm, traj=traj, truth=truth, first=first, anchor=anchor, off=off, clouds=clouds, ses=ses)


@pytest.mark.parametrize("score_thre", [0.5, -1.0], ids=["matched", "odometry_only"])
def test_the_search_finds_the_loop_on_the_oracle(oracle, capi, score_thre):
    run = oracle_run(oracle, capi, FULL_LAP, score_thre=score_thre)
    lp = capi.default_loop_params()
    cand = capi.loop_gate(run["traj"], run["first"], run["anchor"], run["off"], lp)
    ref = gate_ref(run["traj"], run["first"], run["anchor"], run["off"], **loop_params_dict(lp))
    assert cand is not None and cand["submap"] == 0 and same_candidate(cand, ref)
    print("candidate: submap 0, dist %.3f m, path %.1f m, anchor %d" % (cand["dist"], cand["path"], cand["anchor_scan"]))
    p, pm = run["p"], run["pm"]
    newest = np.ascontiguousarray(pm.submaps[-1].scans[-1], np.float32).reshape(-1, 2)
    scan = oracle.approx_voxel_filter(robot_frame(newest, run["traj"][-1]), p["LeafSize"])
    om = oracle.Map(run["clouds"][0], oracle.default_params(resolution=p["Resolution"], step_size=p["StepSize"],
                                                            trans_eps=p["TransformationEpsilon"], max_iter=p["MaximumIterations"]))
    out = relocalize_ref(oracle, om, scan, ref["lattice"], lp.top_k, bool(lp.local_max))
    want = expected_pose(run["traj"], run["truth"], int(cand["anchor_scan"]), FULL_LAP - 1)
    cost = ref_cost(out["records"])
    gaps = [pose_gap((r["pose"][0], r["pose"][1], math.degrees(r["pose"][2])), want) for r in out["records"]]
    for c, (g, k) in enumerate(zip(gaps, cost)):
        print("candidate %d: cost %.5f, %.3f m and %.2f deg from the expected pose" % (c, k, g[0], g[1]))
    best = out["best"]
    assert len(cost) >= 1 and cost[best] < lp.max_cost / 2
    assert gaps[best][0] <= 0.05 and gaps[best][1] <= 1.0
    for g, k in zip(gaps, cost):
        assert g[0] <= 0.3 or k > 2 * lp.max_cost


def test_half_a_lap_has_no_candidate(oracle, capi):
    run = oracle_run(oracle, capi, HALF_LAP)
    lp = capi.default_loop_params()
    assert len(run["first"]) >= 3                                            # there are closed submaps to refuse
    assert capi.loop_gate(run["traj"], run["first"], run["anchor"], run["off"], lp) is None
    assert gate_ref(run["traj"], run["first"], run["anchor"], run["off"], **loop_params_dict(lp)) is None
