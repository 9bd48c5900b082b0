"""ndt_sessions_cross_candidates and ndt_sessions_find_cross_loops on the device: three sessions of the synthetic hall in one
map frame (test_gpu_loops' sizes: 181 beams, sepThre 5; seeds 33 and 35 drive the full lap, 34 half of it), behind step
FULL_LAP - 1.  The candidates are held to the host rule on the set's own read-outs; every candidate's search to the
composition of public calls on the comparison chain's data (the cloud of the session searched, the scan of the searcher),
byte for byte; then independence of the other searchers, tracks and max_submaps, the untouched SLAM state, the shapes of the
search (an empty scan, a refused map, a set of one session), the stats, the joint graph's convergence and the replay."""
import ctypes
import math

import numpy as np
import pytest

import pg_helpers as PG
import session_workloads as W
from ndt_slam_amd import synth
from cross_loops_helpers import assert_set_candidates, compose_cross, set_tracks
from loops_helpers import FULL_LAP, HALF_LAP, between, pose_gap
from loops_multi_helpers import MULTI
from session_correct_helpers import CorrectedChain
from session_helpers import lockstep, same_records, session_logs
from test_gpu_loops import params, run_lockstep
from test_gpu_loops_multi import assert_decision, field_rows
from test_gpu_posegraph import POSE_TOL
from test_gpu_sessions_correct import chain_poses, same_snapshot, snapshot
from gpu_support import gpu, sync, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

SPECS = ((33, FULL_LAP + 1), (34, HALF_LAP), (35, FULL_LAP + 1))


@pytest.fixture(scope="module")
def scene(gpu):
    """The set, a twin that never searches and the composed chain, all behind step FULL_LAP - 1."""
    capi, ctx = gpu
    logs, p = session_logs(SPECS, n_beams=181), params()
    ses, twin = (capi.Sessions(ctx, len(SPECS), capi.session_params_from_launch(p)) for _ in range(2))
    chain = CorrectedChain(capi, ctx, len(SPECS), p)
    run_lockstep(logs, FULL_LAP, ses, twin, chain)
    yield dict(capi=capi, ctx=ctx, logs=logs, p=p, ses=ses, twin=twin, chain=chain)
    ses.close(); twin.close(); chain.close()


def result_bytes(loops, recs, k):
    """Candidate k's guaranteed part -- its ndt_loop, its statistics, its written records -- from the memory the library wrote."""
    n = int(loops[k]["m"]["loop"]["n_cand"])
    return field_rows(loops, "m", "loop")[k].tobytes() + field_rows(loops, "m", "fit")[k].tobytes() + recs[k][:n].tobytes()


def key_of(l):
    return int(l["m"]["loop"]["cand"]["session"]), int(l["map_session"]), int(l["m"]["loop"]["cand"]["submap"])


def assert_cross_candidate(sc, cl, rec, mp):
    """One ndt_cross_loop and its records against the composition on the chain: the cloud of map_session, the scan of the searcher."""
    capi, chain = sc["capi"], sc["chain"]
    lm, loop = cl["m"], cl["m"]["loop"]
    a, b = int(loop["cand"]["session"]), int(cl["map_session"])
    ref, recs, fit = compose_cross(sc, a, b, loop["cand"], mp)
    n = ref["n_cand"]
    assert loop["status"] == ref["status"] == 0 and loop["n_cand"] == n and cl["reserved"] == 0 and lm["reserved"] == 0
    for f in ("cand_index", "cand_score"):
        assert loop[f][:n].tobytes() == ref[f].tobytes() and not loop[f][n:].any(), f
    assert rec[:n].tobytes() == recs.tobytes()
    assert lm["fit"][:n].tobytes() == fit.tobytes() and not lm["fit"][n:].tobytes().strip(b"\0")
    # the decision, and the edge from map_session's anchor pose to the searcher's newest scan
    assert_decision(capi, lm, rec, chain_poses(chain, b), mp)
    assert int(loop["edge"]["to"]) == len(chain_poses(chain, a)) - 1 and int(loop["edge"]["from_"]) < len(chain_poses(chain, b))


def test_candidates_are_the_host_rule_on_the_sets_read_outs(scene):
    capi, ses = scene["capi"], scene["ses"]
    for kw in (MULTI, dict(MULTI, max_submaps=4, radius=10.0), dict(MULTI, max_submaps=1, radius=1.0), dict(MULTI, max_submaps=3, radius=0.0)):
        mp = capi.default_loop_multi_params(**kw)
        got = ses.cross_candidates(mp)
        assert_set_candidates(capi, ses, got, mp)
        assert ses.stats().host_waits == 1
        print("radius %.1f, max_submaps %d: %s" % (mp.loop.radius, mp.max_submaps,
                                                 [(int(c["cand"]["session"]), int(c["map_session"]), int(c["cand"]["submap"])) for c in got]))
    mp = capi.default_loop_multi_params(**MULTI)
    got = ses.cross_candidates(mp)
    assert sorted(set(got["cand"]["session"].tolist())) == [0, 1, 2]          # everybody stands in somebody else's map
    assert all(int(c["cand"]["session"]) != int(c["map_session"]) for c in got)
    for which, against in (([1, 0, 0], None), (None, [0, 0, 1]), ([1, 0, 1], [1, 0, 1]), ([0, 1, 0], [0, 1, 0]), ([0, 0, 0], None),
                           (None, [0, 0, 0])):
        sub = ses.cross_candidates(mp, which, against)
        assert_set_candidates(capi, ses, sub, mp, which, against)
    assert len(ses.cross_candidates(mp, [0, 1, 0], [0, 1, 0])) == 0          # the one track is the searcher's own
    # the same records from the library's host gate on those read-outs
    who, tracks = set_tracks(ses)
    at = 0
    for i in range(len(SPECS)):
        poses = ses.trajectory(i)[0]
        alone = capi.cross_gate(poses[-1], len(poses) - 1, who.index(i), tracks, mp)
        mine = got[at:at + len(alone)]
        assert alone["map_session"].tolist() == [who.index(t) for t in mine["map_session"].tolist()]
        assert field_rows(alone, "cand", "lattice").tobytes() == field_rows(mine, "cand", "lattice").tobytes()
        assert alone["d2"].tobytes() == mine["d2"].tobytes() and alone["cand"]["nearest_scan"].tolist() == mine["cand"]["nearest_scan"].tolist()
        at += len(alone)
    assert at == len(got)


def test_every_candidate_equals_the_composition_of_public_calls(scene):
    capi, ses = scene["capi"], scene["ses"]
    mp = capi.default_loop_multi_params(**MULTI)
    before = [snapshot(ses, i) for i in range(len(SPECS))]
    loops, recs = ses.find_cross_loops(mp, want_records=True)
    st = ses.stats()
    cand = ses.cross_candidates(mp)
    assert len(loops) == len(cand) >= 4
    assert field_rows(loops, "m", "loop", "cand").tobytes() == field_rows(cand, "cand").tobytes()
    assert loops["map_session"].tolist() == cand["map_session"].tolist() and loops["m"]["rank"].tolist() == cand["rank"].tolist()
    assert (st.host_waits, st.sessions_stepped) == (3, len(loops)) and st.h2d_bytes > 0 and st.d2h_bytes > 0
    found = 0
    for cl, rec in zip(loops, recs):
        assert_cross_candidate(scene, cl, rec, mp)
        L = cl["m"]["loop"]
        found += int(L["found"])
        print("searcher %d in session %d's submap %d: n_cand %d best %d found %d cost %s n_in %s" % (
            L["cand"]["session"], cl["map_session"], L["cand"]["submap"], L["n_cand"], L["best"], L["found"], L["cand_cost"][:L["n_cand"]],
            cl["m"]["fit"]["n_in"][:L["n_cand"]]))
    assert found >= 1                                                        # two robots on the same lap do meet
    for i in range(len(SPECS)):
        assert same_snapshot(before[i], snapshot(ses, i)), i                 # nothing of the SLAM state moved
    assert ses.find_cross_loops(mp).tobytes() == loops.tobytes()            # without records


def test_a_candidate_depends_on_nobody_else(scene):
    capi, ses = scene["capi"], scene["ses"]
    mp = capi.default_loop_multi_params(**MULTI)
    loops, recs = ses.find_cross_loops(mp, want_records=True)
    base = {key_of(l): result_bytes(loops, recs, k) for k, l in enumerate(loops)}
    seen = set()
    for which, against, kw in (([1, 0, 0], None, MULTI), ([0, 0, 1], [1, 0, 0], MULTI), (None, [0, 0, 1], MULTI), ([0, 1, 1], None, MULTI),
                               (None, None, dict(MULTI, max_submaps=1)), (None, None, dict(MULTI, max_submaps=4)),
                               ([1, 0, 0], [0, 1, 1], dict(MULTI, max_submaps=3))):
        sub, rec = ses.find_cross_loops(capi.default_loop_multi_params(**kw), which, against, want_records=True)
        assert ses.stats().host_waits == (3 if len(sub) else 1)
        for k, l in enumerate(sub):
            assert which is None or which[key_of(l)[0]]
            assert against is None or against[key_of(l)[1]]
            if key_of(l) in base:
                assert result_bytes(sub, rec, k) == base[key_of(l)], (which, against, kw, key_of(l))
                seen.add(key_of(l))
    assert seen == set(base)                                                 # every candidate came again in some other company


def test_stats_and_calls_that_find_nothing(scene):
    capi, ses = scene["capi"], scene["ses"]
    mp = capi.default_loop_multi_params(**MULTI)
    ses.find_cross_loops(mp)
    every = ses.stats()
    ses.find_cross_loops(mp, [1, 0, 0])
    one = ses.stats()
    assert every.host_waits == one.host_waits == 3 and every.sessions_stepped > one.sessions_stepped >= 1
    assert every.h2d_bytes > one.h2d_bytes > 0 and every.d2h_bytes > one.d2h_bytes > 0
    # no eligible pair: the gate's wait alone
    none = ses.find_cross_loops(capi.default_loop_multi_params(**dict(MULTI, radius=0.0)))
    st = ses.stats()
    assert len(none) == 0 and (st.host_waits, st.sessions_stepped) == (1, 0) and st.h2d_bytes > 0 and st.d2h_bytes > 0
    # nobody searches, or nobody is searched: not even the gate
    for which, against in (([0, 0, 0], None), (None, [0, 0, 0])):
        assert len(ses.find_cross_loops(mp, which, against)) == 0
        st = ses.stats()
        assert (st.host_waits, st.sessions_stepped, st.h2d_bytes, st.d2h_bytes) == (0, 0, 0, 0)
    # the refusals of the multi search under the new names
    lib, E, n = capi.lib(), capi.NDT_E_ARG, ctypes.c_int(-7)
    out = np.zeros(4 * len(SPECS), capi.CROSS_LOOP_DTYPE)
    err = lambda: lib.ndt_last_error(scene["ctx"].h).decode()
    for name in ("ndt_sessions_find_cross_loops", "ndt_sessions_cross_candidates"):
        tail = (None,) if name.endswith("loops") else ()
        fn = getattr(lib, name)
        assert fn(ses.h, None, None, None, out.ctypes.data, ctypes.byref(n), *tail) == E and err() == name + ": NULL params or outputs"
        assert fn(ses.h, None, None, ctypes.byref(mp), None, ctypes.byref(n), *tail) == E and err() == name + ": NULL params or outputs"
        bad = capi.default_loop_multi_params(max_submaps=5)
        assert fn(ses.h, None, None, ctypes.byref(bad), out.ctypes.data, ctypes.byref(n), *tail) == E and "max_submaps must be in 1 .. 4" in err()
    assert n.value == -7 and not out.tobytes().strip(b"\0")


def test_the_step_after_a_search_is_the_twins(scene):
    """Behind the searches above (and one more here): the next step of the set, of the twin that never searched and of the
    chain are the same bytes.  (The module's last test on the scene: it steps it.)"""
    capi, ses, twin, chain, logs = scene["capi"], scene["ses"], scene["twin"], scene["chain"], scene["logs"]
    ses.find_cross_loops(capi.default_loop_multi_params(**dict(MULTI, max_submaps=4, radius=10.0)))
    for k, scans, odo, act in lockstep(logs):
        if k < FULL_LAP:
            continue
        a, b, c = ses.step(scans, odo, act), twin.step(scans, odo, act), chain.step(scans, odo, act)
        assert a.tobytes() == b.tobytes()
        assert all(same_records(x, y) for x, y in zip(a, c))
    for i in range(len(SPECS)):
        assert same_snapshot(snapshot(ses, i), snapshot(twin, i)), i


# ------------------------------------------------------------------------------------------ shapes of the search
SMALL = ((33, 12), (34, 12), (35, 12))             # sepThre 1: five closed submaps behind step 11
EMPTY_SESSION = 1
SMALL_LP = dict(radius=10.0, step_xy=0.1, step_yaw=math.radians(1.0), local_max=0, top_k=8, half_x=2, half_y=2, half_yaw=1)


def test_an_empty_newest_scan_and_a_set_of_one_session(gpu):
    capi, ctx = gpu
    p = W.launch_params(sepThre=1.0, score_thre=-1.0)
    logs = [([x.copy() for x in scans], odo.copy()) for scans, odo in session_logs(SMALL, n_beams=181)]
    logs[EMPTY_SESSION][0][11] = W.EMPTY
    ses = capi.Sessions(ctx, len(SMALL), capi.session_params_from_launch(p))
    chain = CorrectedChain(capi, ctx, len(SMALL), p)
    alone = capi.Sessions(ctx, 1, capi.session_params_from_launch(p))
    run_lockstep(logs, 12, ses, chain)
    run_lockstep(logs[:1], 12, alone)
    sc = dict(capi=capi, ctx=ctx, p=p, ses=ses, chain=chain)
    try:
        mp = capi.default_loop_multi_params(max_submaps=3, **SMALL_LP)
        loops, recs = ses.find_cross_loops(mp, want_records=True)
        assert loops["m"]["loop"]["cand"]["session"].tolist() == [0] * 3 + [1] * 3 + [2] * 3 and loops["m"]["rank"].tolist() == [0, 1, 2] * 3
        assert_set_candidates(capi, ses, ses.cross_candidates(mp), mp)
        for cl, rec in zip(loops, recs):
            L = cl["m"]["loop"]
            if L["cand"]["session"] == EMPTY_SESSION:
                assert (L["status"], L["found"], L["n_cand"], L["best"]) == (0, 0, 0, -1)
                assert not L["pose"].any() and not L["edge"]["rel"].any() and not cl["m"]["fit"].tobytes().strip(b"\0") and not L["cand_cost"].any()
            else:
                assert_cross_candidate(sc, cl, rec, mp)
                assert L["n_cand"] == 8
        # only the empty scan searches: its candidates are the empty record, nothing is queued behind the gate
        only = ses.find_cross_loops(mp, [0, 1, 0])
        st = ses.stats()
        assert len(only) == 3 and (st.host_waits, st.sessions_stepped) == (1, 3)
        assert all((l["m"]["loop"]["status"], l["m"]["loop"]["n_cand"], l["m"]["loop"]["best"]) == (0, 0, -1) for l in only)
        # a set of one session: its closed submaps are its own
        assert alone.trajectory(0)[1].size >= 3
        assert len(alone.find_cross_loops(mp)) == 0 and len(alone.cross_candidates(mp)) == 0
        st = alone.stats()
        assert (st.host_waits, st.sessions_stepped) == (1, 0)
    finally:
        ses.close(); chain.close(); alone.close()


def test_a_refused_map_costs_its_candidate_alone(gpu):
    """test_gpu_loops' GRID_OUTLIER log: session 1's first closed cloud spans more than 2^28 cells, so the build refuses the map
    of the candidate (searcher 0, session 1, submap 0) -- and nobody else's."""
    capi, ctx = gpu
    logs = [([x.copy() for x in scans], odo.copy()) for scans, odo in session_logs(((33, FULL_LAP), (35, FULL_LAP)), n_beams=181)]
    logs[1][0][0] = np.concatenate([logs[1][0][0], [W.GRID_OUTLIER]])
    ses = capi.Sessions(ctx, 2, capi.session_params_from_launch(params()))
    run_lockstep(logs, FULL_LAP, ses)
    try:
        mp = capi.default_loop_multi_params(**dict(MULTI, max_submaps=4))
        both, rec = ses.find_cross_loops(mp, None, want_records=True)
        keys = [key_of(l) for l in both]
        assert (0, 1, 0) in keys and sum(k[0] == 0 for k in keys) >= 2 and sum(k[0] == 1 for k in keys) >= 1
        for k, cl in enumerate(both):
            L = cl["m"]["loop"]
            if keys[k] == (0, 1, 0):
                assert L["status"] == capi.NDT_E_GRID
                assert L["found"] == 0 and L["n_cand"] == 0 and L["best"] == -1 and not L["cand_index"].any() and not L["pose"].any()
                assert not cl["m"]["fit"].tobytes().strip(b"\0")
            else:
                assert L["status"] == capi.NDT_OK and L["n_cand"] >= 1
                assert_decision(capi, cl["m"], rec[k], ses.trajectory(keys[k][1])[0], mp)
        assert ses.stats().host_waits == 3
        # a call without the refused candidate: searcher 1's results are the same bytes
        alone, rec1 = ses.find_cross_loops(mp, [0, 1], want_records=True)
        mine = [k for k in range(len(both)) if keys[k][0] == 1]
        assert [key_of(l) for l in alone] == [keys[k] for k in mine]
        assert all(result_bytes(alone, rec1, j) == result_bytes(both, rec, k) for j, k in enumerate(mine))
        # no map at all: the gate's wait and the boxes', nobody found
        near = capi.default_loop_multi_params(**dict(MULTI, max_submaps=1))
        first = ses.cross_candidates(near, [1, 0])
        if [(int(c["map_session"]), int(c["cand"]["submap"])) for c in first] == [(1, 0)]:
            only_bad = ses.find_cross_loops(near, [1, 0])
            assert only_bad["m"]["loop"]["status"].tolist() == [capi.NDT_E_GRID] and only_bad[0]["m"]["loop"]["found"] == 0
            assert ses.stats().host_waits == 2
    finally:
        ses.close()


# ------------------------------------------------------------------------------------------ the joint graph
def two_chains():
    """Two 56-node chains -- the lap as two drifting odometries saw it -- and one cross edge from chain 0's mid-chain anchor
    (scan 4 of its first submap's nine) to chain 1's last node, as the truth has it."""
    from ndt_slam_amd import replay
    trajs = []
    for seed, scale, bias in ((33, 1.015, 0.05), (35, 0.99, -0.05)):
        recs, truth = synth.replay_records(n_frames=FULL_LAP, n_beams=8, step=0.6, seed=seed, odo_scale=scale, odo_yaw_bias_deg=bias)
        trajs.append(np.array([[r["x"], r["y"], r["th"]] for r in recs], np.float64))
    truth = np.asarray(truth, np.float64).reshape(-1, 3)
    edge = np.zeros(1, dtype=PG.PG_EDGE_DTYPE)[0]
    edge["from"], edge["to"], edge["rel"], edge["info"] = 4, FULL_LAP - 1, PG.between(truth[4], truth[FULL_LAP - 1]), [1e4, 0, 0, 1e4, 0, 1e4]
    return replay.cross_graph(trajs, [[], []], [(0, 1, edge)], [100.0, 0, 0, 100.0, 0, 100.0])


def test_two_chains_joined_by_one_edge_converge(gpu):
    """Only the cross edge ties the second chain to node 0 (the gauge): the dense oracle and the device's preconditioned
    conjugate gradients both end converged, on the same poses (the optimum has zero residuals: chain 1 moves rigidly)."""
    capi, ctx = gpu
    nodes, arcs, off = two_chains()
    assert off.tolist() == [0, FULL_LAP, 2 * FULL_LAP] and len(arcs) == 2 * (FULL_LAP - 1) + 1
    assert (int(arcs[-1]["from"]), int(arcs[-1]["to"])) == (4, 2 * FULL_LAP - 1)
    ref = PG.oracle_optimize(nodes, arcs)
    assert ref["converged"]
    new, res = capi.optimize_pose_graphs(ctx, nodes, [0, len(nodes)], arcs, [0, len(arcs)], None)
    gap = max(max(pose_gap(a, b)) for a, b in zip(new, ref["poses"]))
    print("joint graph: device status %d converged %d iterations %d (cg %d) cost %.3e -> %.3e; oracle %d steps, cost %.3e; largest gap %.3e"
          % (res[0]["status"], res[0]["converged"], res[0]["iterations"], res[0]["cg_iterations"], res[0]["cost_initial"], res[0]["cost_final"],
             len(ref["steps"]), ref["costs"][-1], gap))
    assert res[0]["status"] == 0 and res[0]["converged"] == 1
    # the same poses: metres and degrees both under the bound in metres and radians (a degree is the larger number); the optimum
    # has zero residuals, so the cost is held as test_gpu_posegraph holds its zero-residual case, not relative to the oracle's
    assert gap <= POSE_TOL, gap
    assert res[0]["cost_final"] <= 1e-18 * res[0]["cost_initial"], (res[0]["cost_final"], res[0]["cost_initial"], ref["costs"][-1])


# ------------------------------------------------------------------------------------------ replay
def test_replay_closes_loops_between_two_sessions_of_the_same_lap(gpu):
    """Two sessions of the same lap with different odometry drifts (odometry only: score_thre -1, R40.1's settings) through
    run_sessions_resident: with LoopClosure(cross=...) a cross edge is found, both sessions are corrected in one correct(), and
    the pose of session 0's last scan seen from session 1's first anchor scan is nearer to the truth than without `cross`."""
    from ndt_slam_amd import replay
    from ndt_slam_amd.pose_estimator import Pose2D, Scan2D
    capi, ctx = gpu
    p = params(score_thre=-1.0)
    logs, truth = [], None
    for seed, scale, bias in ((33, 1.015, 0.05), (35, 0.99, -0.05)):
        recs, truth = synth.replay_records(n_frames=FULL_LAP + 1, n_beams=181, step=0.6, seed=seed, odo_scale=scale, odo_yaw_bias_deg=bias)
        logs.append([Scan2D(np.asarray(r["front"], np.float64).reshape(-1, 2), k, Pose2D(r["x"], r["y"], r["th"])) for k, r in enumerate(recs)])
    truth = np.asarray(truth, np.float64).reshape(-1, 3)
    mp = capi.default_loop_multi_params(**MULTI)
    info = np.array(mp.loop.info[:]) / 100.0

    def replayed(cross):
        corrections, edges = [], []

        class Counting(capi.Sessions):
            def correct(self, new_poses):
                out = super().correct(new_poses)
                corrections.append(dict(out))
                return out

            def find_cross_loops(self, *a, **kw):
                out = super().find_cross_loops(*a, **kw)
                edges.extend(key_of(l) for l in out if l["m"]["loop"]["status"] == 0 and l["m"]["loop"]["found"])
                return out

        ses = Counting(ctx, 2, capi.session_params_from_launch(p), archive=True)
        lc = replay.LoopClosure(loop=mp.loop, pg=None, odo_info=info, every=1, cooldown=10, multi=mp, cross=cross)
        poses = replay.run_sessions_resident(ctx, logs, sessions=ses, loop_closure=lc, **p)
        trajs, anchor = [ses.trajectory(i)[0] for i in range(2)], int(ses.trajectory(1)[2][0])
        assert all(np.array([(q.tx, q.ty, q.th) for q in poses[i]]).tobytes() == trajs[i].tobytes() for i in range(2))
        ses.close()
        return trajs, anchor, corrections, edges

    plain, anchor, n_plain, e_plain = replayed(None)
    cross, anchor2, n_cross, e_cross = replayed(mp)
    assert e_plain == [] and anchor == anchor2 and len(cross[0]) == len(plain[0]) == FULL_LAP + 1
    assert len(e_cross) >= 1 and all(a != b for a, b, _ in e_cross)
    joint = [d for d in n_cross if set(d) == {0, 1}]
    assert joint and all(v == capi.NDT_OK for d in n_cross for v in d.values())      # both sessions taken by one correct()
    want = between(truth[anchor], truth[FULL_LAP])
    gap_plain = pose_gap(between(plain[1][anchor], plain[0][-1]), want)
    gap_cross = pose_gap(between(cross[1][anchor], cross[0][-1]), want)
    print("session 0's last pose seen from session 1's scan %d: without cross %.3f m / %.2f deg off, with cross %.3f m / %.2f deg "
          "(%d cross edges found, %d joint corrections, %d corrections without cross)"
          % ((anchor,) + gap_plain + gap_cross + (len(e_cross), len(joint), len(n_plain))))
    assert gap_cross[0] < gap_plain[0]
