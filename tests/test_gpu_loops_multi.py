"""ndt_sessions_loop_candidates_multi and ndt_sessions_find_loops_multi on the device, on test_gpu_loops' scene (the lap of
loops_helpers.loop_workload, 181 beams, behind step FULL_LAP - 1) and on a small set in loop_shape_workloads' style.  Every
candidate is held to the numpy gating on the chain's layout; its ndt_loop part (guarantee a) byte for byte to the composition
of public single-job calls (loops_helpers.compose_loop); its ranged statistics (guarantee b) to Map.fit_points of a fresh map of
the closed cloud at the records' transforms; cand_cost, best, found, pose and edge to the decision restated in Python."""
import ctypes
import math

import numpy as np
import pytest

import session_workloads as W
from ndt_slam_amd import synth
from loops_helpers import (FULL_LAP, between, chain_layout, compose_loop, expected_pose, loop_params_dict, loop_workload, pose_gap,
                           same_candidate)
from loops_multi_helpers import MULTI, decide_ref, gate_multi_ref
from session_correct_helpers import CorrectedChain
from session_helpers import lockstep, same_records, session_logs
from test_gpu_loops import NAMED, SPECS, params, run_lockstep, scene  # noqa: F401
from test_gpu_sessions_correct import chain_poses, same_snapshot, snapshot
from gpu_support import gpu, sync, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu


def field_rows(arr, *path):
    """The memory of a (nested) field of a C-contiguous structured array, one row of bytes per element: numpy copies structured
    elements field by field, so a field view's .tobytes() does not carry the padding the library wrote (LOG.md R39.1)."""
    assert arr.flags.c_contiguous
    dt, at = arr.dtype, 0
    for name in path:
        dt, off = dt.fields[name][:2]
        at += off
    return arr.view(np.uint8).reshape(len(arr), -1)[:, at:at + dt.itemsize]


def multi_bytes(loops, recs, k):
    """Candidate k's whole ndt_loop_multi and its written records as bytes, from the memory the library wrote."""
    n = int(loops[k]["loop"]["n_cand"])
    return field_rows(loops)[k].tobytes() + recs[k][:n].tobytes()


def filtered_newest(sc, i):
    """Session i's newest scan as the search sees it: robot frame, pre-filtered (compose_loop's source)."""
    capi, ctx, chain = sc["capi"], sc["ctx"], sc["chain"]
    newest = np.ascontiguousarray(chain.pcmaps[i].submaps[-1].scans[-1], np.float32).reshape(-1, 2)
    if not len(newest):
        return newest
    robot = capi.repose_points(ctx, newest, [0, len(newest)], chain_poses(chain, i)[-1:], np.zeros((1, 3)))
    return ctx.prefilter(robot, sc["p"]["LeafSize"])


def assert_decision(capi, lm, rec, traj, mp):
    """cand_cost, best, found, pose and edge of one candidate from its own records and statistics, by the rule restated."""
    loop, n = lm["loop"], int(lm["loop"]["n_cand"])
    cost, best, found = decide_ref(rec[:n]["converged"], lm["fit"][:n], mp.min_overlap, mp.loop.max_cost)
    assert loop["cand_cost"][:n].tobytes() == cost.tobytes() and not loop["cand_cost"][n:].any()
    assert (int(loop["best"]), int(loop["found"])) == (best, found)
    e = loop["edge"]
    assert (e["from_"], e["to"]) == (loop["cand"]["anchor_scan"], loop["cand"]["newest_scan"])
    assert e["info"].tobytes() == np.array(mp.loop.info[:]).tobytes()
    if best < 0:
        assert not loop["pose"].any() and not e["rel"].any()
        return
    w = rec[best]["pose"]
    pose = np.array([w[0], w[1], w[2] * np.float64(180) / np.float64(np.pi)])
    assert loop["pose"].tobytes() == pose.tobytes()
    assert e["rel"].tobytes() == capi.pg_edge_between(traj[int(loop["cand"]["anchor_scan"])], pose).tobytes()


def assert_candidate(sc, lm, rec, mp):
    """One ndt_loop_multi and its records against the composition on the chain's session of the same index."""
    capi, ctx, chain = sc["capi"], sc["ctx"], sc["chain"]
    loop = lm["loop"]
    i, m = int(loop["cand"]["session"]), int(loop["cand"]["submap"])
    ref, recs = compose_loop(sc, i, loop["cand"], mp.loop)
    n = ref["n_cand"]
    # (a) what ndt_sessions_find_loops gives for this (session, submap)
    assert loop["status"] == ref["status"] == 0 and loop["n_cand"] == n
    for f in ("cand_index", "cand_score"):
        assert loop[f][:n].tobytes() == ref[f].tobytes() and not loop[f][n:].any(), f
    assert rec[:n].tobytes() == recs.tobytes()
    # (b) the ranged statistics of a fresh map of that closed cloud at every record's transform
    assert not lm["fit"][n:].tobytes().strip(b"\0") and lm["reserved"] == 0
    if n:
        src = filtered_newest(sc, i)
        gm = capi.Map(ctx, np.ascontiguousarray(chain.pcmaps[i].submaps[m].p_cloud, np.float32).reshape(-1, 2), chain.params)
        _, st = gm.fit_points(np.tile(src, (n, 1)), np.arange(n + 1) * len(src), rec[:n], max_d2=mp.max_d2, want_d2=False)
        gm.close()
        assert lm["fit"][:n].tobytes() == st.tobytes(), (i, m, lm["fit"][:n], st)
        assert all(int(s["n_points"]) == len(src) for s in st)
    assert_decision(capi, lm, rec, chain_poses(chain, i), mp)


def test_candidates_are_the_numpy_gating(scene):
    capi, ses, chain = scene["capi"], scene["ses"], scene["chain"]
    mp = capi.default_loop_multi_params(**MULTI)
    got = ses.loop_candidates_multi(mp)
    assert got["session"].tolist() == [0, 0, 2, 2, 3, 3] and got["submap"].tolist() == [0, 1] * 3      # the half lap has none
    assert ses.loop_candidates_multi(mp, NAMED)["session"].tolist() == [0, 0, 2, 2]
    for i in (0, 1, 2, 3):
        ref = gate_multi_ref(*chain_layout(chain, i), mp.max_submaps, **loop_params_dict(mp.loop))
        mine = got[got["session"] == i]
        assert len(mine) == len(ref) and all(same_candidate(c, r) for c, r in zip(mine, ref)), i
        tr = ses.trajectory(i)                                              # the same from the set's own read-outs
        sub_off = np.concatenate([[0], np.cumsum([len(x) for x in ses.global_map(i)[1]])])
        alone = capi.loop_gate_multi(tr[0], tr[1], tr[2], sub_off, mp)
        assert len(alone) == len(ref) and all(same_candidate(c, r) for c, r in zip(alone, ref)), i
    # max_submaps = 1: the bytes of ndt_sessions_loop_candidates, with the same loop parameters
    one = capi.default_loop_multi_params(**dict(MULTI, max_submaps=1))
    assert ses.loop_candidates_multi(one, NAMED).tobytes() == ses.loop_candidates(one.loop, NAMED).tobytes()
    for k in (3, 4):
        more = ses.loop_candidates_multi(capi.default_loop_multi_params(**dict(MULTI, max_submaps=k, radius=10.0)), [1, 0, 0, 0])
        ref = gate_multi_ref(*chain_layout(chain, 0), k, **loop_params_dict(capi.default_loop_params(radius=10.0)))
        assert len(more) == k and all(same_candidate(c, r) for c, r in zip(more, ref))


def test_loops_equal_the_composition_the_single_map_statistics_and_the_rule(scene):
    capi, ses, chain = scene["capi"], scene["ses"], scene["chain"]
    mp = capi.default_loop_multi_params(**MULTI)
    before = [snapshot(ses, i) for i in range(len(SPECS))]
    loops, recs = ses.find_loops_multi(mp, NAMED, want_records=True)
    named = ses.stats()
    assert field_rows(loops, "loop", "cand").tobytes() == field_rows(ses.loop_candidates_multi(mp, NAMED)).tobytes()
    assert loops["loop"]["cand"]["session"].tolist() == [0, 0, 2, 2] and loops["rank"].tolist() == [0, 1, 0, 1]
    for lm, rec in zip(loops, recs):
        assert_candidate(scene, lm, rec, mp)
        L = lm["loop"]
        print("session %d submap %d: n_cand %d best %d found %d cost %s n_in %s" % (
            L["cand"]["session"], L["cand"]["submap"], L["n_cand"], L["best"], L["found"], L["cand_cost"][:L["n_cand"]],
            lm["fit"]["n_in"][:L["n_cand"]]))
    # the outcome on session 0: both loops are found, with the pose bounds of the host prototype
    _, truth = synth.replay_records(n_frames=SPECS[0][1], n_beams=181, step=0.6, seed=SPECS[0][0])
    truth = np.asarray(truth, np.float64).reshape(-1, 3)
    traj = chain_poses(chain, 0)
    for lm, bound in zip(loops[:2], (0.05, 0.2)):
        L = lm["loop"]
        gap = pose_gap(L["pose"], expected_pose(traj, truth, int(L["cand"]["anchor_scan"]), FULL_LAP - 1))
        print("session 0 submap %d: found pose %.3f m / %.2f deg from the expected pose" % ((L["cand"]["submap"],) + gap))
        assert L["found"] == 1 and gap[0] <= bound and gap[1] <= 1.0
    # ndt_sessions_find_loops with the same loop parameters: one candidate per session, the rank-0 candidate's records; its
    # full-cloud rule refuses what submap 1 holds
    single, srec = ses.find_loops(mp.loop, NAMED, want_records=True)
    assert single["cand"]["session"].tolist() == [0, 2]
    for j, a in ((0, 0), (1, 2)):
        n = int(single[j]["n_cand"])
        assert field_rows(single, "cand")[j].tobytes() == field_rows(loops, "loop", "cand")[a].tobytes() and n == loops[a]["loop"]["n_cand"]
        assert srec[j][:n].tobytes() == recs[a][:n].tobytes()
        assert single[j]["cand_index"].tobytes() == loops[a]["loop"]["cand_index"].tobytes()
        assert single[j]["cand_score"].tobytes() == loops[a]["loop"]["cand_score"].tobytes()
    L1 = loops[1]["loop"]
    assert recs[1][int(L1["best"])]["fitness"] > 2 * mp.loop.max_cost
    # nothing of the SLAM state moved
    for i in range(len(SPECS)):
        assert same_snapshot(before[i], snapshot(ses, i)), i
    # independence: one session named, then all; max_submaps 1 against 2
    one, rec1 = ses.find_loops_multi(mp, [1, 0, 0, 0], want_records=True)
    single_stats = ses.stats()
    assert len(one) == 2 and all(multi_bytes(one, rec1, k) == multi_bytes(loops, recs, k) for k in range(2))
    every, rec4 = ses.find_loops_multi(mp, None, want_records=True)
    all_stats = ses.stats()
    assert every["loop"]["cand"]["session"].tolist() == [0, 0, 2, 2, 3, 3]
    assert all(multi_bytes(every, rec4, k) == multi_bytes(loops, recs, k) for k in range(4))
    narrow = capi.default_loop_multi_params(**dict(MULTI, max_submaps=1))
    first, recf = ses.find_loops_multi(narrow, NAMED, want_records=True)
    assert first["loop"]["cand"]["session"].tolist() == [0, 2]
    assert multi_bytes(first, recf, 0) == multi_bytes(loops, recs, 0) and multi_bytes(first, recf, 1) == multi_bytes(loops, recs, 2)
    assert ses.find_loops_multi(mp, NAMED).tobytes() == loops.tobytes()      # without records
    # two host waits whoever is named; sessions_stepped = J; zeros with no candidate
    assert (named.host_waits, named.sessions_stepped) == (2, 4) and (single_stats.host_waits, single_stats.sessions_stepped) == (2, 2)
    assert (all_stats.host_waits, all_stats.sessions_stepped) == (2, 6)
    assert all_stats.h2d_bytes > single_stats.h2d_bytes > 0 and all_stats.d2h_bytes > single_stats.d2h_bytes > 0
    assert len(ses.find_loops_multi(mp, [0, 1, 0, 0])) == 0
    none = ses.stats()
    assert (none.host_waits, none.sessions_stepped, none.h2d_bytes, none.d2h_bytes) == (0, 0, 0, 0)


def test_refusals(scene):
    capi, ctx, ses = scene["capi"], scene["ctx"], scene["ses"]
    lib, E = capi.lib(), capi.NDT_E_ARG
    out = np.zeros(4 * len(SPECS), capi.LOOP_MULTI_DTYPE)
    cout = np.zeros(4 * len(SPECS), capi.LOOP_CANDIDATE_DTYPE)
    n = ctypes.c_int(-7)
    good = capi.default_loop_multi_params(**MULTI)
    err = lambda: lib.ndt_last_error(ctx.h).decode()
    ses.find_loops_multi(good, NAMED)
    stats = ses.stats()

    def find(p=good, s=ses.h, o=out.ctypes.data, cnt=ctypes.byref(n)):
        return lib.ndt_sessions_find_loops_multi(s, None, None if p is None else ctypes.byref(p), o, cnt, None)

    def gate(p=good, s=ses.h, o=cout.ctypes.data, cnt=ctypes.byref(n)):
        return lib.ndt_sessions_loop_candidates_multi(s, None, None if p is None else ctypes.byref(p), o, cnt)

    nan = float("nan")
    for call, name in ((find, "ndt_sessions_find_loops_multi"), (gate, "ndt_sessions_loop_candidates_multi")):
        assert call(s=None) == E and lib.ndt_last_error(None).decode() == "null session set"
        for kw in (dict(p=None), dict(o=None), dict(cnt=None)):
            assert call(**kw) == E and err() == name + ": NULL params or outputs", kw
        for kw, text in ((dict(max_submaps=0), "max_submaps must be in 1 .. 4"), (dict(max_submaps=5), "max_submaps must be in 1 .. 4"),
                         (dict(max_d2=nan), "max_d2 is NaN or negative"), (dict(max_d2=-1.0), "max_d2 is NaN or negative"),
                         (dict(min_overlap=nan), "min_overlap is NaN or outside [0, 1]"), (dict(min_overlap=1.5), "min_overlap is NaN or outside [0, 1]"),
                         (dict(min_path=-1.0), "negative or not finite"), (dict(half_y=-1), "a negative half extent"),
                         (dict(half_x=2048, half_y=2048), "more than 2^24 poses"), (dict(top_k=0), "top_k must be in 1 .. 8"),
                         (dict(max_cost=nan), "max_cost is NaN")):
            assert call(p=capi.default_loop_multi_params(**kw)) == E and err().startswith(name + ": ") and text in err(), kw
    # an open ndt_map_rebuild_begin on the context.  (More than 2^31 - 1 lattice poses over all candidates need 128 candidates
    # of 2^24 poses: no set of this module has them.)
    cloud = to_dev(np.random.default_rng(1).uniform(-3, 3, (500, 2)).astype(np.float32))
    sync()
    own = capi.Map(ctx, params=capi.default_params(resolution=0.3, grid_margin=8), dev_ptr=cloud.data_ptr(), n=len(cloud))
    own.rebuild_begin(cloud.data_ptr(), len(cloud))
    try:
        assert find() == E and "ndt_map_rebuild_begin" in err()
    finally:
        own.rebuild_end()
    own.close()
    assert not out.tobytes().strip(b"\0") and not cout.tobytes().strip(b"\0") and n.value == -7
    after = ses.stats()
    assert (after.host_waits, after.h2d_bytes, after.d2h_bytes) == (stats.host_waits, stats.h2d_bytes, stats.d2h_bytes)
    assert len(ses.find_loops_multi(good, NAMED)) == 4


def test_the_step_after_a_search_is_the_twins(scene):
    """Behind the searches above (and one more here): the next step of the set, of a twin set that never searched and of the
    chain are the same bytes, and so are the states behind it.  (The module's last test on the scene: it steps it.)"""
    capi, ses, twin, chain, logs = scene["capi"], scene["ses"], scene["twin"], scene["chain"], scene["logs"]
    ses.find_loops_multi(capi.default_loop_multi_params(**dict(MULTI, max_submaps=4, radius=10.0)))
    for k, scans, odo, act in lockstep(logs):
        if k < FULL_LAP:
            continue
        a, b, c = ses.step(scans, odo, act), twin.step(scans, odo, act), chain.step(scans, odo, act)
        assert a.tobytes() == b.tobytes()
        assert all(same_records(x, y) for x, y in zip(a, c))
    for i in range(len(SPECS)):
        assert same_snapshot(snapshot(ses, i), snapshot(twin, i)), i


def test_a_refused_map_costs_its_candidate_alone(gpu):
    """test_gpu_loops' GRID_OUTLIER log: session 1's first closed cloud spans more than 2^28 cells, so the build refuses the map
    of the candidate (session 1, submap 0) -- and nobody else's."""
    capi, ctx = gpu
    logs = [([x.copy() for x in scans], odo.copy()) for scans, odo in session_logs(((33, FULL_LAP), (35, FULL_LAP)), n_beams=181)]
    logs[1][0][0] = np.concatenate([logs[1][0][0], [W.GRID_OUTLIER]])
    ses = capi.Sessions(ctx, 2, capi.session_params_from_launch(params()))
    run_lockstep(logs, FULL_LAP, ses)
    mp = capi.default_loop_multi_params(**MULTI)
    both, rec = ses.find_loops_multi(mp, None, want_records=True)
    L = both["loop"]
    assert L["cand"]["session"].tolist() == [0, 0, 1, 1] and L["cand"]["submap"].tolist() == [0, 1, 0, 1]
    assert L["status"].tolist() == [capi.NDT_OK, capi.NDT_OK, capi.NDT_E_GRID, capi.NDT_OK]
    bad = both[2]
    assert bad["loop"]["found"] == 0 and bad["loop"]["n_cand"] == 0 and bad["loop"]["best"] == -1 and bad["rank"] == 0
    assert not bad["loop"]["cand_index"].any() and not bad["loop"]["pose"].any() and not bad["fit"].tobytes().strip(b"\0")
    assert L["found"].tolist()[:2] == [1, 1] and L[3]["n_cand"] >= 1
    assert_decision(capi, both[3], rec[3], ses.trajectory(1)[0], mp)
    alone, rec1 = ses.find_loops_multi(mp, [1, 0], want_records=True)      # a call without the refused candidate
    assert len(alone) == 2 and all(multi_bytes(alone, rec1, k) == multi_bytes(both, rec, k) for k in range(2))
    assert ses.stats().host_waits == 2
    narrow = capi.default_loop_multi_params(**dict(MULTI, max_submaps=1))
    only_bad = ses.find_loops_multi(narrow, [0, 1])                         # no map at all: one wait, nobody found
    assert only_bad["loop"]["status"].tolist() == [capi.NDT_E_GRID] and only_bad[0]["loop"]["found"] == 0 and ses.stats().host_waits == 1
    ses.close()


# ------------------------------------------------------------------------------------------ a small set: shapes of the search
SMALL = ((33, 12), (34, 12), (35, 12))             # sepThre 1: five closed submaps behind step 11
EMPTY_SESSION = 1
SMALL_LP = dict(min_path=0.0, radius=10.0, step_xy=0.1, step_yaw=math.radians(1.0), local_max=0, top_k=8)


@pytest.fixture(scope="module")
def small(gpu):
    """Three sessions of twelve steps (loop_shape_workloads' launch: sepThre 1, odometry only) beside the composed chain;
    session 1's last scan has no points."""
    capi, ctx = gpu
    p = W.launch_params(sepThre=1.0, score_thre=-1.0)
    logs = [([x.copy() for x in scans], odo.copy()) for scans, odo in session_logs(SMALL, n_beams=181)]
    logs[EMPTY_SESSION][0][11] = W.EMPTY
    ses = capi.Sessions(ctx, len(SMALL), capi.session_params_from_launch(p))
    chain = CorrectedChain(capi, ctx, len(SMALL), p)
    run_lockstep(logs, 12, ses, chain)
    yield dict(capi=capi, ctx=ctx, p=p, ses=ses, chain=chain)
    ses.close(); chain.close()


def test_an_empty_newest_scan_gives_the_empty_record_for_each_of_its_candidates(small):
    capi, ses = small["capi"], small["ses"]
    mp = capi.default_loop_multi_params(max_submaps=3, half_x=2, half_y=2, half_yaw=1, **SMALL_LP)
    loops, recs = ses.find_loops_multi(mp, None, want_records=True)
    assert loops["loop"]["cand"]["session"].tolist() == [0] * 3 + [1] * 3 + [2] * 3 and loops["rank"].tolist() == [0, 1, 2] * 3
    assert ses.stats().host_waits == 2 and ses.stats().sessions_stepped == 9
    for lm, rec in zip(loops, recs):
        L = lm["loop"]
        if L["cand"]["session"] == EMPTY_SESSION:
            assert (L["status"], L["found"], L["n_cand"], L["best"]) == (0, 0, 0, -1)
            assert not L["pose"].any() and not L["edge"]["rel"].any() and not lm["fit"].tobytes().strip(b"\0") and not L["cand_cost"].any()
        else:
            assert_candidate(small, lm, rec, mp)
            assert L["n_cand"] == 8
    # every scan named is empty: nothing is queued
    only = ses.find_loops_multi(mp, [0, 1, 0])
    st = ses.stats()
    assert len(only) == 3 and (st.host_waits, st.sessions_stepped, st.h2d_bytes, st.d2h_bytes) == (0, 3, 0, 0)
    assert all((l["loop"]["status"], l["loop"]["n_cand"], l["loop"]["best"]) == (0, 0, -1) for l in only)


def test_dead_slots_have_zero_statistics(small):
    """top_k = 8 against a lattice of nine poses with local maxima only: fewer than eight are picked, the slots behind them
    are dead (map_of -1 in the match and in the verification) and their statistics stay zero."""
    capi, ses = small["capi"], small["ses"]
    mp = capi.default_loop_multi_params(max_submaps=2, half_x=1, half_y=1, half_yaw=0, **dict(SMALL_LP, local_max=1))
    loops, recs = ses.find_loops_multi(mp, [1, 0, 1], want_records=True)
    assert len(loops) == 4
    for lm, rec in zip(loops, recs):
        assert 1 <= lm["loop"]["n_cand"] < 8
        assert_candidate(small, lm, rec, mp)
    one = capi.default_loop_multi_params(max_submaps=2, half_x=0, half_y=0, half_yaw=0, **dict(SMALL_LP, local_max=1))
    loops, recs = ses.find_loops_multi(one, [1, 0, 1], want_records=True)
    for lm, rec in zip(loops, recs):
        assert lm["loop"]["n_cand"] == 1
        assert_candidate(small, lm, rec, one)


# ------------------------------------------------------------------------------------------ replay
def test_replay_closes_loops_over_several_submaps_and_leaves_the_single_path_alone(gpu):
    """The odometry-only lap through run_sessions_resident: with LoopClosure(multi=...) it runs, corrects and ends nearer to the
    truth than without a closure; with multi=None the trajectory is that of the manual sequence find_loops, loop_graph,
    optimise, correct -- the path as it was."""
    from ndt_slam_amd import replay
    from ndt_slam_amd.pose_estimator import Pose2D, Scan2D
    capi, ctx = gpu
    (scans, odo), truth, p = loop_workload(n_frames=FULL_LAP + 1, score_thre=-1.0)
    log = [Scan2D(scans[k], k, Pose2D(*odo[k])) for k in range(len(scans))]
    lp = capi.default_loop_params()
    info = np.array(lp.info[:]) / 100.0
    cooldown = 10

    def manual():
        ses, quiet = capi.Sessions(ctx, 1, capi.session_params_from_launch(p), archive=True), 0
        for k in range(len(scans)):
            assert ses.step([scans[k]], [odo[k]])[0]["stepped"]
            if k + 1 < quiet:
                continue
            found = [l for l in ses.find_loops(lp, np.array([1], np.uint8)) if l["status"] == 0 and l["found"]]
            if not found:
                continue
            traj = ses.trajectory(0)[0]
            new, res = capi.optimize_pose_graphs(ctx, traj, [0, len(traj)], replay.loop_graph(traj, found[0]["edge"], info), [0, len(traj)], None)
            if res[0]["status"] == 0 and res[0]["converged"]:
                assert ses.correct({0: new}) == {0: capi.NDT_OK}
                quiet = k + 1 + cooldown
        out = ses.trajectory(0)[0]
        ses.close()
        return out

    def replayed(lc):
        corrections = []

        class Counting(capi.Sessions):
            def correct(self, new_poses):
                out = super().correct(new_poses)
                corrections.append(dict(out))
                return out

        ses = Counting(ctx, 1, capi.session_params_from_launch(p), archive=True)
        poses = replay.run_sessions_resident(ctx, [log], sessions=ses, loop_closure=lc, **p)
        traj, anchor = ses.trajectory(0)[0], int(ses.trajectory(0)[2][0])
        assert lc is None or np.array([(q.tx, q.ty, q.th) for q in poses[0]]).tobytes() == traj.tobytes()
        ses.close()
        return traj, anchor, corrections

    plain, anchor, none = replayed(None)
    old, _, n_old = replayed(replay.LoopClosure(loop=lp, pg=None, odo_info=info, every=1, cooldown=cooldown))
    assert none == [] and len(n_old) >= 1 and old.tobytes() == manual().tobytes()
    mp = capi.default_loop_multi_params(**MULTI)
    new, _, n_new = replayed(replay.LoopClosure(loop=mp.loop, pg=None, odo_info=info, every=1, cooldown=cooldown, multi=mp))
    assert len(n_new) >= 1 and all(v == capi.NDT_OK for d in n_new for v in d.values()) and len(new) == len(plain) == FULL_LAP + 1
    want = between(truth[anchor], truth[len(new) - 1])
    gap_plain = pose_gap(between(plain[anchor], plain[-1]), want)
    gap_old, gap_new = pose_gap(between(old[anchor], old[-1]), want), pose_gap(between(new[anchor], new[-1]), want)
    print("closing pose seen from scan %d: no closure %.3f m off, single search %.3f m, several submaps %.3f m (%d and %d corrections)"
          % (anchor, gap_plain[0], gap_old[0], gap_new[0], len(n_old), len(n_new)))
    assert gap_new[0] < gap_plain[0]
