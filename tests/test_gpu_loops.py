"""ndt_sessions_loop_candidates and ndt_sessions_find_loops on the device.  The workload is loops_helpers.loop_workload: the
5 m circle, 0.6 m per frame, 181 beams, sepThre 5 -- frame 55 is back near frame 3, submap 0 holds the scans 0 .. 8.  Every
ndt_loop and every record is held byte for byte against the composition of public single-job calls on the composed chain's
own scans and closed clouds; the candidates against the numpy gating."""
import ctypes

import numpy as np
import pytest

import session_workloads as W
from loops_helpers import (FULL_LAP, HALF_LAP, assert_composed, chain_layout, compose_loop, expected_pose, gate_ref, loop_bytes,  # noqa: F401
                           loop_params_dict, loop_workload, pose_gap, same_candidate)
from session_correct_helpers import CorrectedChain
from session_helpers import lockstep, same_records, session_logs
from test_gpu_sessions_correct import same_state, snapshot, same_snapshot
from gpu_support import gpu, sync, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

# session 0: the full lap; 1: half a lap, then idle; 2: a full lap of another seed; 3: a full lap that no call names
SPECS = ((33, FULL_LAP + 1), (34, HALF_LAP), (35, FULL_LAP + 1), (36, FULL_LAP + 1))
NAMED = [1, 1, 1, 0]


def params(**kw):
    return W.launch_params(sepThre=5.0, **kw)


def run_lockstep(logs, upto, *sets):
    for k, scans, odo, act in lockstep(logs):
        if k == upto:
            break
        recs = [s.step(scans, odo, act) for s in sets]
        for r in recs[1:]:
            assert all(same_records(a, b) for a, b in zip(recs[0], r)), k


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


def test_candidates_are_the_numpy_gating(scene):
    capi, ses, chain = scene["capi"], scene["ses"], scene["chain"]
    lp = capi.default_loop_params()
    got = ses.loop_candidates(lp, NAMED)
    assert got["session"].tolist() == [0, 2]                                # the half lap has none, session 3 is not named
    assert ses.loop_candidates(lp)["session"].tolist() == [0, 2, 3]
    for c in got:
        i = int(c["session"])
        poses, first, anchor, off = chain_layout(chain, i)
        ref = gate_ref(poses, first, anchor, off, **loop_params_dict(lp))
        assert ref["submap"] == 0 and same_candidate(c, ref), i
        g, parts = ses.global_map(i)                                         # the same from the set's own read-outs
        tr = ses.trajectory(i)
        sub_off = np.concatenate([[0], np.cumsum([len(x) for x in parts])])
        alone = capi.loop_gate(tr[0], tr[1], tr[2], sub_off, lp)
        assert alone["submap"] == c["submap"] and alone["dist"] == c["dist"] and alone["lattice"].tobytes() == c["lattice"].tobytes()
    poses, first, anchor, off = chain_layout(chain, 1)
    assert gate_ref(poses, first, anchor, off, **loop_params_dict(lp)) is None and len(first) >= 3


def test_loops_equal_the_composition_of_single_calls_and_naming_changes_no_byte(scene):
    capi, ses = scene["capi"], scene["ses"]
    lp = capi.default_loop_params()
    before = [snapshot(ses, i) for i in range(len(SPECS))]
    loops, recs = ses.find_loops(lp, NAMED, want_records=True)
    three = ses.stats()
    assert loops["cand"]["session"].tolist() == [0, 2]
    assert loops["cand"].tobytes() == ses.loop_candidates(lp, NAMED).tobytes()
    for loop, rec in zip(loops, recs):
        assert_composed(scene, loop, rec, lp)
        assert loop["found"] == 1 and loop["best"] == 0 and loop["n_cand"] >= 2      # the loop is found, by the best-scoring pick
        print("session %d: cost %s" % (loop["cand"]["session"], loop["cand_cost"][:loop["n_cand"]]))
    # views taken before the call are still what the set gives: nothing of the SLAM state moved
    for i in range(len(SPECS)):
        assert same_snapshot(before[i], snapshot(ses, i)), i
    # one session named, then all four: a job's bytes do not change
    one, rec1 = ses.find_loops(lp, [1, 0, 0, 0], want_records=True)
    single = ses.stats()
    assert len(one) == 1 and loop_bytes(one[0], rec1[0]) == loop_bytes(loops[0], recs[0])
    every, rec4 = ses.find_loops(lp, None, want_records=True)
    many = ses.stats()
    assert every["cand"]["session"].tolist() == [0, 2, 3]
    assert loop_bytes(every[0], rec4[0]) == loop_bytes(loops[0], recs[0]) and loop_bytes(every[1], rec4[1]) == loop_bytes(loops[1], recs[1])
    other, rec2 = ses.find_loops(lp, [0, 0, 1, 0], want_records=True)
    assert loop_bytes(other[0], rec2[0]) == loop_bytes(loops[1], recs[1])
    # two host waits for one candidate and for three, none without a candidate
    assert (single.host_waits, single.sessions_stepped) == (2, 1) and (many.host_waits, many.sessions_stepped) == (2, 3)
    assert three.host_waits == 2 and many.h2d_bytes > single.h2d_bytes > 0 and many.d2h_bytes > single.d2h_bytes > 0
    assert len(ses.find_loops(lp, [0, 1, 0, 0])) == 0
    none = ses.stats()
    assert (none.host_waits, none.sessions_stepped, none.h2d_bytes, none.d2h_bytes) == (0, 0, 0, 0)
    # without records, and with another top_k
    assert ses.find_loops(lp, NAMED).tobytes() == loops.tobytes()
    lp2 = capi.default_loop_params(top_k=8, local_max=0, half_yaw=2)
    l2, r2 = ses.find_loops(lp2, [1, 0, 0, 0], want_records=True)
    assert l2[0]["n_cand"] == 8
    assert_composed(scene, l2[0], r2[0], lp2)


def test_a_refused_map_costs_its_candidate_alone(gpu):
    """Session 1's first scan carries the GRID_OUTLIER beam: its first closed cloud spans more than 2^28 cells of the match
    resolution, so the build refuses that candidate's map (NDT_E_GRID) -- and nobody else's."""
    capi, ctx = gpu
    logs = [([x.copy() for x in scans], odo.copy()) for scans, odo in session_logs(((33, FULL_LAP), (35, FULL_LAP)), n_beams=181)]
    logs[1][0][0] = np.concatenate([logs[1][0][0], [W.GRID_OUTLIER]])
    ses = capi.Sessions(ctx, 2, capi.session_params_from_launch(params()))
    run_lockstep(logs, FULL_LAP, ses)
    lp = capi.default_loop_params()
    cand = ses.loop_candidates(lp)
    assert cand["session"].tolist() == [0, 1] and cand["submap"].tolist() == [0, 0]
    both, rec = ses.find_loops(lp, None, want_records=True)
    assert both["status"].tolist() == [capi.NDT_OK, capi.NDT_E_GRID]
    bad = both[1]
    assert bad["found"] == 0 and bad["n_cand"] == 0 and bad["best"] == -1 and not bad["cand_index"].any() and not bad["pose"].any()
    assert both[0]["found"] == 1
    alone, rec1 = ses.find_loops(lp, [1, 0], want_records=True)
    assert loop_bytes(alone[0], rec1[0]) == loop_bytes(both[0], rec[0])
    only_bad = ses.find_loops(lp, [0, 1])                                    # no map at all: one wait, nobody found
    assert only_bad["status"].tolist() == [capi.NDT_E_GRID] and only_bad[0]["found"] == 0 and ses.stats().host_waits == 1
    ses.close()


def test_refusals(scene):
    capi, ctx, ses = scene["capi"], scene["ctx"], scene["ses"]
    lib, E = capi.lib(), capi.NDT_E_ARG
    out = np.zeros(len(SPECS), capi.LOOP_DTYPE)
    cout = np.zeros(len(SPECS), capi.LOOP_CANDIDATE_DTYPE)
    n = ctypes.c_int(-7)
    good = capi.default_loop_params()
    err = lambda: lib.ndt_last_error(ctx.h).decode()
    ses.find_loops(good, NAMED)
    stats = ses.stats()

    def find(p=good, s=ses.h, o=out.ctypes.data, cnt=ctypes.byref(n)):
        return lib.ndt_sessions_find_loops(s, None, None if p is None else ctypes.byref(p), o, cnt, None)

    def gate(p=good, s=ses.h, o=cout.ctypes.data, cnt=ctypes.byref(n)):
        return lib.ndt_sessions_loop_candidates(s, None, None if p is None else ctypes.byref(p), o, cnt)

    for call, name in ((find, "ndt_sessions_find_loops"), (gate, "ndt_sessions_loop_candidates")):
        assert call(s=None) == E and lib.ndt_last_error(None).decode() == "null session set"
        for kw in (dict(p=None), dict(o=None), dict(cnt=None)):
            assert call(**kw) == E and err() == name + ": NULL params or outputs", kw
        for kw, text in ((dict(min_path=-1.0), "negative or not finite"), (dict(radius=float("inf")), "negative or not finite"),
                         (dict(step_xy=float("nan")), "negative or not finite"), (dict(step_yaw=-1e-3), "negative or not finite"),
                         (dict(half_y=-1), "a negative half extent"), (dict(half_x=2048, half_y=2048), "more than 2^24 poses"),
                         (dict(top_k=0), "top_k must be in 1 .. 8"), (dict(top_k=9), "top_k must be in 1 .. 8"),
                         (dict(max_cost=float("nan")), "max_cost is NaN")):
            assert call(p=capi.default_loop_params(**kw)) == E and err().startswith(name + ": ") and text in err(), kw
    # an open ndt_map_rebuild_begin on the context
    cloud = to_dev(np.random.default_rng(1).uniform(-3, 3, (500, 2)).astype(np.float32))
    sync()
    own = capi.Map(ctx, params=capi.default_params(resolution=0.3, grid_margin=8), dev_ptr=cloud.data_ptr(), n=len(cloud))
    own.rebuild_begin(cloud.data_ptr(), len(cloud))
    try:
        assert find() == E and "ndt_map_rebuild_begin" in err()
    finally:
        own.rebuild_end()
    own.close()
    # nothing was written or queued: the outputs, the count and the stats are as they were
    assert not out.tobytes().strip(b"\0") and not cout.tobytes().strip(b"\0") and n.value == -7
    after = ses.stats()
    assert (after.host_waits, after.h2d_bytes, after.d2h_bytes) == (stats.host_waits, stats.h2d_bytes, stats.d2h_bytes)
    assert len(ses.find_loops(good, NAMED)) == 2


def test_the_step_after_a_search_is_the_twins(scene):
    """Behind the searches of the test above (and one more here): the next step of the set, of a twin set that never searched
    and of the chain are the same bytes, and so are the states behind it."""
    capi, ses, twin, chain, logs = scene["capi"], scene["ses"], scene["twin"], scene["chain"], scene["logs"]
    ses.find_loops(capi.default_loop_params(), NAMED)
    for k, scans, odo, act in lockstep(logs):
        if k < FULL_LAP:
            continue
        a, b, c = ses.step(scans, odo, act), twin.step(scans, odo, act), chain.step(scans, odo, act)
        assert a.tobytes() == b.tobytes()
        assert all(same_records(x, y) for x, y in zip(a, c))
    for i in range(len(SPECS)):
        assert same_snapshot(snapshot(ses, i), snapshot(twin, i)), i
        same_state(ses, chain, i, "after the search")


def test_end_to_end_from_the_search_to_the_corrected_state(gpu):
    """Odometry only (score_thre -1: no match is fused): the last pose has drifted about 0.25 m.  find_loops' edge + the
    odometry arcs -> ndt_pg_optimize_batch -> ndt_sessions_correct brings it nearer to where the scan truly is, and the next
    step is the corrected chain's."""
    capi, ctx = gpu
    (scans, odo), truth, p = loop_workload(n_frames=FULL_LAP + 1, score_thre=-1.0)
    logs = [(scans, odo)]
    ses = capi.Sessions(ctx, 1, capi.session_params_from_launch(p))
    chain = CorrectedChain(capi, ctx, 1, p)
    run_lockstep(logs, FULL_LAP, ses, chain)
    lp = capi.default_loop_params()
    loops = ses.find_loops(lp)
    assert len(loops) == 1 and loops[0]["found"] == 1 and loops[0]["cand"]["submap"] == 0
    loop = loops[0]
    poses = ses.trajectory(0)[0]
    n = len(poses)
    assert n == FULL_LAP and loop["edge"]["to"] == n - 1
    want = expected_pose(poses, truth, int(loop["edge"]["from_"]), n - 1)
    gap_before, gap_found = pose_gap(poses[-1], want), pose_gap(loop["pose"], want)
    print("last pose %.3f m / %.2f deg off, found pose %.3f m / %.2f deg off" % (gap_before + gap_found))
    assert gap_found[0] <= 0.05 and gap_found[1] <= 1.0
    edges = np.zeros(n, dtype=capi.PG_EDGE_DTYPE)
    for j in range(n - 1):
        edges[j]["from"], edges[j]["to"] = j, j + 1
        edges[j]["rel"] = capi.pg_edge_between(poses[j], poses[j + 1])
        edges[j]["info"] = np.array(lp.info[:]) / 100.0
    edges[n - 1]["from"], edges[n - 1]["to"] = loop["edge"]["from_"], loop["edge"]["to"]
    edges[n - 1]["rel"], edges[n - 1]["info"] = loop["edge"]["rel"], loop["edge"]["info"]
    new, res = capi.optimize_pose_graphs(ctx, poses, [0, n], edges, [0, n])
    assert res[0]["status"] == 0 and res[0]["converged"] == 1 and res[0]["cost_final"] <= res[0]["cost_initial"]
    assert ses.correct({0: new}) == {0: capi.NDT_OK} and chain.correct(0, new) == capi.NDT_OK
    # the anchor's pose moved too: the expected pose is taken again from the corrected trajectory
    gap_after = pose_gap(new[-1], expected_pose(new, truth, int(loop["edge"]["from_"]), n - 1))
    print("corrected last pose %.3f m / %.2f deg off" % gap_after)
    assert gap_after[0] < gap_before[0]
    same_state(ses, chain, 0, "corrected")
    for k, sc, od, act in lockstep(logs):
        if k < FULL_LAP:
            continue
        got, wantr = ses.step(sc, od, act), chain.step(sc, od, act)
        assert same_records(got[0], wantr[0])
    same_state(ses, chain, 0, "the step behind the correction")
    ses.close(); chain.close()
