"""The loop search over several submaps without a GPU: the header's prototypes in the binding, the gating of several submaps
(ndt_loop_gate_multi) against its numpy restatement on test_loops_host's hand-made trajectories, the whole search with the
ranged decision as a prototype on the CPU oracle, and replay.loops_graph."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import fitness_workloads as W
from fit_points_helpers import ranged_best, ranged_of_records, ref_stats
from loops_helpers import FULL_LAP, expected_pose, gate_ref, loop_params_dict, loop_workload, pose_gap, robot_frame, same_candidate  # noqa: F401
from loops_multi_helpers import MULTI, decide_ref, gate_multi_ref
from reloc_helpers import ref_cost, relocalize_ref
from test_loops_host import even_layout, oracle_run, square_lap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ndt_fit_points_multi_dev", "ndt_fit_points_multi", "ndt_loop_multi_default_params", "ndt_loop_gate_multi",
       "ndt_sessions_loop_candidates_multi", "ndt_sessions_find_loops_multi")


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
    for word in ("NDT_LOOP_MAX_SUBMAPS 4", "ndt_loop_multi_params;", "ndt_loop_multi;", "fit[NDT_LOOP_MAX_CAND]", "max_submaps", "min_overlap"):
        assert word in src, word
    p, lp = capi.default_loop_multi_params(), capi.default_loop_params()
    assert bytes(p.loop) == bytes(lp)
    assert (p.max_submaps, p.reserved, p.max_d2, p.min_overlap) == (2, 0, 0.09, 0.5) and capi.NDT_LOOP_MAX_SUBMAPS == 4
    q = capi.default_loop_multi_params(max_submaps=3, radius=4.0, info=[1, 2, 3, 4, 5, 6])
    assert (q.max_submaps, q.loop.radius, list(q.loop.info)) == (3, 4.0, [1, 2, 3, 4, 5, 6])
    # ndt_loop_multi: an ndt_loop, eight ndt_fit_stats, rank and reserved
    D = capi.LOOP_MULTI_DTYPE
    assert D.names == ("loop", "fit", "rank", "reserved") and D.fields["loop"][0] == capi.LOOP_DTYPE
    assert D.fields["fit"][0].shape == (8,) and D.itemsize == capi.LOOP_DTYPE.itemsize + 8 * 32 + 8


# ------------------------------------------------------------------------------------------ the gating
def check_gate_multi(capi, poses, first, anchor, off, mp, want_submaps):
    got = capi.loop_gate_multi(poses, first, anchor, off, mp)
    ref = gate_multi_ref(poses, first, anchor, off, mp.max_submaps, **loop_params_dict(mp.loop))
    assert [r["submap"] for r in ref] == list(want_submaps) == got["submap"].tolist()
    assert all(g["session"] == 0 and same_candidate(g, r) for g, r in zip(got, ref))
    keys = [(float(g["dist"]), int(g["submap"])) for g in got]
    assert keys == sorted(keys)                                              # ascending (dist, submap)
    assert len({g["lattice"].tobytes() for g in got}) <= 1                   # one lattice per session
    one = capi.loop_gate(poses, first, anchor, off, mp.loop)
    assert (one is None) == (len(got) == 0) and (one is None or one.tobytes() == got[0].tobytes())
    return got


def test_gating_of_several_submaps_against_the_numpy_restatement(capi):
    poses = square_lap()
    first, anchor, off = even_layout(len(poses), 4)                          # 32 scans, 8 submaps; the lap ends at the start
    M = capi.default_loop_multi_params
    # max_submaps = 1: byte-equal to ndt_loop_gate
    one = check_gate_multi(capi, poses, first, anchor, off, M(max_submaps=1), [0])
    assert one[0].tobytes() == capi.loop_gate(poses, first, anchor, off, capi.default_loop_params()).tobytes()
    # a radius that reaches round the corner: the eligible submaps by gate_ref's arithmetic, nearest first
    wide = dict(radius=7.0, min_path=5.0)
    every = gate_multi_ref(poses, first, anchor, off, 8, **loop_params_dict(capi.default_loop_params(**wide)))
    order = [r["submap"] for r in every]
    assert len(order) >= 5 and order[0] == 0                                 # more are eligible than any call may ask for
    for k in (2, 3, 4):
        got = check_gate_multi(capi, poses, first, anchor, off, M(max_submaps=k, **wide), order[:k])      # truncation
        assert len(got) == k
    # fewer eligible than asked for
    few = dict(radius=3.2, min_path=5.0)
    n_few = len(gate_multi_ref(poses, first, anchor, off, 8, **loop_params_dict(capi.default_loop_params(**few))))
    assert 1 <= n_few < 4
    assert len(check_gate_multi(capi, poses, first, anchor, off, M(max_submaps=4, **few), order[:n_few])) == n_few
    # none: 3 m short of the start; fewer than two closed submaps
    short = square_lap(back=3.0)
    f2, a2, o2 = even_layout(len(short), 4)
    check_gate_multi(capi, short, f2, a2, o2, M(max_submaps=4), [])
    check_gate_multi(capi, poses, first[:2], anchor[:2], off[:3], M(max_submaps=4), [])


def test_gating_of_several_submaps_ties_empty_ranges_and_empty_clouds(capi):
    """The cases of test_loops_host.test_gating_ties_empty_ranges_and_empty_clouds: both tied submaps come, in index order."""
    M = capi.default_loop_multi_params
    poses = square_lap(jitter=0.0)
    first, anchor, off = even_layout(len(poses), 4)
    tied = poses.copy()
    tied[-1, :2] = (0.0, 0.0)
    tied[0, :2] = (0.6, 0.0); tied[5, :2] = (-0.6, 0.0)
    tied[4, :2] = (3.0, 0.3)
    got = check_gate_multi(capi, tied, first, anchor, off, M(max_submaps=2), [0, 1])
    assert got["dist"].tolist() == [0.6, 0.6] and got["nearest_scan"].tolist() == [0, 5]
    check_gate_multi(capi, tied, first, anchor, off, M(max_submaps=1), [0])
    swapped = tied.copy()
    swapped[0, :2] = (0.6000001, 0.0)                                        # a hair further: submap 1 first
    check_gate_multi(capi, swapped, first, anchor, off, M(max_submaps=2), [1, 0])
    hollow = off.copy()
    hollow[1:] -= 100                                                        # submap 0's closed cloud is empty
    assert 0 not in check_gate_multi(capi, tied, first, anchor, hollow, M(max_submaps=4), [1])["submap"].tolist()
    f3 = np.concatenate([[0], first]).astype(np.int32)                       # submap 0 without a scan of its own
    a3 = np.concatenate([[0], anchor]).astype(np.int32)
    o3 = np.arange(len(f3) + 1, dtype=np.uint64) * 100
    check_gate_multi(capi, tied, f3, a3, o3, M(max_submaps=2), [1, 2])


def test_gating_of_several_submaps_has_inclusive_bounds(capi):
    M = capi.default_loop_multi_params
    poses = square_lap()
    first, anchor, off = even_layout(len(poses), 4)
    base = dict(step_xy=0.1, step_yaw=0.01, half_x=1, half_y=1, half_yaw=1)
    every = gate_multi_ref(poses, first, anchor, off, 4, min_path=0.0, radius=50.0, step_xy=0.1, step_yaw=0.01, half=(1, 1, 1))
    second = every[1]
    # radius == the second's dist and min_path == its path: it is in; one step below either: it is not
    at = check_gate_multi(capi, poses, first, anchor, off, M(max_submaps=4, radius=second["dist"], min_path=0.0, **base),
                          [r["submap"] for r in every if r["dist"] <= second["dist"]])
    assert second["submap"] in at["submap"].tolist()
    below = capi.loop_gate_multi(poses, first, anchor, off, M(max_submaps=4, radius=float(np.nextafter(second["dist"], -np.inf)), min_path=0.0, **base))
    assert second["submap"] not in below["submap"].tolist() and len(below) == len(at) - 1
    on_path = capi.loop_gate_multi(poses, first, anchor, off, M(max_submaps=4, radius=50.0, min_path=second["path"], **base))
    above = capi.loop_gate_multi(poses, first, anchor, off, M(max_submaps=4, radius=50.0, min_path=float(np.nextafter(second["path"], np.inf)), **base))
    assert second["submap"] in on_path["submap"].tolist() and second["submap"] not in above["submap"].tolist()
    # max_d2 = 0 and min_overlap = 0 and 1 are legal
    for kw in (dict(max_d2=0.0), dict(min_overlap=0.0), dict(min_overlap=1.0), dict(max_d2=float("inf"))):
        assert len(capi.loop_gate_multi(poses, first, anchor, off, M(**kw))) == 1


def test_gating_of_several_submaps_refusals(capi):
    M = capi.default_loop_multi_params
    poses = square_lap()
    first, anchor, off = even_layout(len(poses), 4)
    nan = float("nan")
    for kw, text in ((dict(max_submaps=0), "max_submaps must be in 1 .. 4"), (dict(max_submaps=5), "max_submaps must be in 1 .. 4"),
                     (dict(max_submaps=-1), "max_submaps must be in 1 .. 4"), (dict(max_d2=nan), "max_d2 is NaN or negative"),
                     (dict(max_d2=-1e-300), "max_d2 is NaN or negative"), (dict(min_overlap=nan), "min_overlap is NaN or outside [0, 1]"),
                     (dict(min_overlap=-0.1), "min_overlap is NaN or outside [0, 1]"),
                     (dict(min_overlap=float(np.nextafter(1.0, 2.0))), "min_overlap is NaN or outside [0, 1]"),
                     # those of the existing gating, under the new name
                     (dict(min_path=-1.0), "negative or not finite"), (dict(half_x=-1), "a negative half extent"),
                     (dict(half_x=2048, half_y=2048, half_yaw=0), "more than 2^24 poses"), (dict(top_k=9), "top_k must be in 1 .. 8"),
                     (dict(max_cost=nan), "max_cost is NaN")):
        with pytest.raises(capi.NdtError, match=re.escape("ndt_loop_gate_multi: ") + ".*" + re.escape(text)):
            capi.loop_gate_multi(poses, first, anchor, off, M(**kw))
    bad = poses.copy(); bad[3, 1] = np.inf
    with pytest.raises(capi.NdtError, match="scan 3: a pose is not finite"):
        capi.loop_gate_multi(bad, first, anchor, off, M())
    with pytest.raises(capi.NdtError, match="is not a set's layout"):
        capi.loop_gate_multi(poses, first + 1, anchor, off, M())
    lib, n, p = capi.lib(), ctypes.c_int(), M()
    assert lib.ndt_loop_gate_multi(None, 1, None, None, None, 1, None, None, None) == capi.NDT_E_ARG
    assert lib.ndt_last_error(None).decode() == "ndt_loop_gate_multi: NULL pointer"
    assert lib.ndt_loop_multi_default_params(None) == capi.NDT_E_ARG
    assert lib.ndt_sessions_loop_candidates_multi(None, None, ctypes.byref(p), None, ctypes.byref(n)) == capi.NDT_E_ARG
    assert lib.ndt_last_error(None).decode() == "null session set"
    assert lib.ndt_sessions_find_loops_multi(None, None, ctypes.byref(p), None, ctypes.byref(n), None) == capi.NDT_E_ARG
    assert lib.ndt_last_error(None).decode() == "null session set"


# ------------------------------------------------------------------------------------------ the prototype on the oracle
def test_the_search_over_two_submaps_finds_both_loops_on_the_oracle(oracle, capi):
    """The lap of loops_helpers.loop_workload on the CPU oracle chain: the candidates, their refined records, brute-force ranged
    statistics, the decision restated.  Measured here (seed 33, 56 frames, 295 filtered points): submap 0's best slot 0.013 m /
    0.28 deg from the expected pose, submap 1's 0.129 m / 0.07 deg with full-cloud cost 0.842 and 244 points in range."""
    run = oracle_run(oracle, capi, FULL_LAP)
    mp = capi.default_loop_multi_params(**MULTI)
    lp = mp.loop
    arrays = (run["traj"], run["first"], run["anchor"], run["off"])
    cands = capi.loop_gate_multi(*arrays, mp)
    ref = gate_multi_ref(*arrays, mp.max_submaps, **loop_params_dict(lp))
    assert cands["submap"].tolist() == [0, 1] and all(same_candidate(c, r) for c, r in zip(cands, ref))
    # the truncation on real data: four are eligible within 10 m, the two nearest come
    far = capi.default_loop_multi_params(**dict(MULTI, radius=10.0))
    assert [r["submap"] for r in gate_multi_ref(*arrays, 4, **loop_params_dict(far.loop))] == [0, 1, 2, 3]
    assert capi.loop_gate_multi(*arrays, far)["submap"].tolist() == [0, 1]
    p, pm = run["p"], run["pm"]
    newest = np.ascontiguousarray(pm.submaps[-1].scans[-1], np.float32).reshape(-1, 2)
    scan = oracle.approx_voxel_filter(robot_frame(newest, run["traj"][-1]), p["LeafSize"])
    prm = oracle.default_params(resolution=p["Resolution"], step_size=p["StepSize"], trans_eps=p["TransformationEpsilon"],
                                max_iter=p["MaximumIterations"])
    print("filtered newest scan: %d points" % len(scan))
    for cand, r in zip(cands, ref):
        m = int(cand["submap"])
        cloud = run["clouds"][m]
        out = relocalize_ref(oracle, oracle.Map(cloud, prm), scan, r["lattice"], lp.top_k, bool(lp.local_max))
        rec = out["records"]
        fit = [ref_stats(W.brute_sq(cloud, W.queries_of(scan, (q["T00"], q["T10"], q["T03"], q["T13"]), bool(prm.transform_sse))), mp.max_d2)
               for q in rec]
        tri = [(f[0], f[2], f[4]) for f in fit]
        cost, best, found = decide_ref(rec["converged"], tri, mp.min_overlap, lp.max_cost)
        want = expected_pose(run["traj"], run["truth"], int(cand["anchor_scan"]), FULL_LAP - 1)
        gaps = [pose_gap((q["pose"][0], q["pose"][1], math.degrees(q["pose"][2])), want) for q in rec]
        full = ref_cost(rec)
        for c in range(len(rec)):
            print("submap %d slot %d: %.3f m %.2f deg off, full cost %.5f, in range %d of %d, ranged %.5f -> cost %g" %
                  (m, c, gaps[c][0], gaps[c][1], full[c], tri[c][1], tri[c][2], tri[c][0], cost[c]))
        assert found == 1 and len(rec) >= 1, m
        if m == 0:
            assert gaps[best][0] <= 0.05 and gaps[best][1] <= 1.0
        else:
            assert best == int(np.argmin([g[0] for g in gaps]))              # the slot nearest to the expected pose
            assert gaps[best][0] <= 0.2 and gaps[best][1] <= 1.0             # two lattice steps
            assert full[best] > 2 * lp.max_cost                              # the full-cloud rule refuses it
            fitness, n_in = ranged_of_records(cloud, scan, rec, mp.max_d2, bool(prm.transform_sse))
            assert ranged_best(rec, fitness, n_in) != best                   # the ranged fitness alone picks an alias


# ------------------------------------------------------------------------------------------ replay.loops_graph
def test_loops_graph_and_the_loop_closure_tuple(capi):
    from ndt_slam_amd import replay
    poses = square_lap(side=3.0)
    n = len(poses)
    info = [100.0, 0.0, 0.0, 100.0, 0.0, 50.0]
    loops = np.zeros(3, dtype=capi.LOOP_DTYPE)
    for k, (a, b) in enumerate(((1, n - 1), (5, n - 1), (0, n - 2))):
        e = loops[k]["edge"]
        e["from_"], e["to"] = a, b
        e["rel"], e["info"] = capi.pg_edge_between(poses[a], poses[b]) + 0.01 * k, np.arange(6) + k
    one = replay.loops_graph(poses, [loops[0]["edge"]], info)
    assert one.dtype == capi.PG_EDGE_DTYPE and one.tobytes() == replay.loop_graph(poses, loops[0]["edge"], info).tobytes() and len(one) == n
    three = replay.loops_graph(poses, [l["edge"] for l in loops], info)
    assert len(three) == n + 2 and three[:n - 1].tobytes() == one[:n - 1].tobytes()
    for k in range(3):
        e, g = loops[k]["edge"], three[n - 1 + k]
        assert (g["from"], g["to"]) == (e["from_"], e["to"]) and g["rel"].tobytes() == e["rel"].tobytes() and g["info"].tobytes() == e["info"].tobytes()
    assert len(replay.loops_graph(poses, [], info)) == n - 1
    lc = replay.LoopClosure(capi.default_loop_params(), None, info, 5, 10)
    assert lc._fields == ("loop", "pg", "odo_info", "every", "cooldown") and len(lc) == 5 and lc.multi is None and lc.remake_closed is False
    loop, pg, odo, every, cooldown = lc
    assert (every, cooldown) == (5, 10)
    mp = capi.default_loop_multi_params()
    assert replay.LoopClosure(mp.loop, None, info, 5, 10, multi=mp).multi is mp
