"""What every call that changes or searches a session set shares and no other module states for all of them: the refusal
while an ndt_map_rebuild_begin is open on the context (NDT_E_ARG, the call's own name, the set's stats and state untouched,
the set alive), the order of the named-session refusals of ndt_sessions_correct and ndt_sessions_remake_closed, and the
shape of ndt_sessions_find_cross_loops' stats: the gate's part once plus a search's.

The set: two sessions of test_gpu_cross_loops' small workload (181 beams, sepThre 1: five closed submaps behind step 11) with
the scan archive, one occupancy grid per session, one small stand-alone map on the same context."""
import ctypes

import numpy as np
import pytest

import occ_helpers as H
import session_workloads as W
from session_helpers import lockstep, session_logs
from gpu_support import gpu, sync, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

SPECS = ((33, 14), (34, 14))                       # 12 steps behind the fixture; scans 12 and 13 for the steps of the test
STEPPED = 12
GEOM = H.Geometry(-12.0, -12.0, 0.1, 240, 240)
LP = dict(radius=10.0, min_path=1.0, step_xy=0.1, step_yaw=np.radians(1.0), local_max=0, top_k=8, half_x=2, half_y=2, half_yaw=1)
CALLS = ("ndt_sessions_step", "ndt_sessions_step_dev", "ndt_sessions_correct", "ndt_sessions_remake_closed", "ndt_sessions_find_loops",
         "ndt_sessions_find_loops_multi", "ndt_sessions_cross_candidates", "ndt_sessions_find_cross_loops", "ndt_sessions_occ_integrate",
         "ndt_sessions_occ_rebuild")
# The stats of the calls of test_find_cross_loops_counts_the_gate_once on this set, as the commit before the call bracket gave
# them: (host_waits, h2d_bytes, d2h_bytes).
PARENT_GATE = (1, 816, 128)                        # 6 candidates
PARENT_CROSS = (3, 4408, 12056)
PARENT_MULTI = (2, 3592, 11928)                    # 6 candidates


@pytest.fixture(scope="module")
def scene(gpu):
    capi, ctx = gpu
    p = W.launch_params(sepThre=1.0, score_thre=-1.0)
    logs = session_logs(SPECS, n_beams=181)
    ses = capi.Sessions(ctx, len(SPECS), capi.session_params_from_launch(p), archive=True)
    plain = capi.Sessions(ctx, len(SPECS), capi.session_params_from_launch(p))      # no archive; both sessions started
    steps = list(lockstep(logs))
    for k, scans, odo, act in steps[:STEPPED]:
        ses.step(scans, odo, act)
        if k < 2:
            plain.step(scans, odo, act)
    grids = [capi.OccGrid(ctx, GEOM) for _ in SPECS]
    ses.occ_integrate(grids)
    cloud = to_dev(np.random.default_rng(1).uniform(-3, 3, (500, 2)).astype(np.float32))
    sync()
    own = capi.Map(ctx, params=capi.default_params(resolution=0.3, grid_margin=8), dev_ptr=cloud.data_ptr(), n=len(cloud))
    yield dict(capi=capi, ctx=ctx, ses=ses, plain=plain, grids=grids, own=own, cloud=cloud, steps=steps)
    own.close(); ses.close(); plain.close()
    for g in grids:
        g.close()


def state(sc):
    """What a caller can read of the set without queuing anything that a pending map refuses."""
    ses, out = sc["ses"], []
    for i in range(ses.n):
        out.append(b"".join(np.ascontiguousarray(a).tobytes() for a in ses.trajectory(i)[:3]) + ses.global_map(i)[0].tobytes())
    return out


def grid_counts(sc):
    return [b"".join(a.tobytes() for a in g.counts()) for g in sc["grids"]]


def the_calls(sc):
    """{name: a call with valid arguments through the binding}; the two steps take the scans behind the fixture's."""
    capi, ses, grids = sc["capi"], sc["ses"], sc["grids"]
    lp, mp = capi.default_loop_params(**LP), capi.default_loop_multi_params(max_submaps=3, **LP)
    (_, scans_a, odo_a, act_a), (_, scans_b, odo_b, act_b) = sc["steps"][STEPPED], sc["steps"][STEPPED + 1]
    raw, off = capi.pack_scans(scans_b, dtype=np.float64)
    d_raw, d_odo = to_dev(raw), to_dev(np.ascontiguousarray(odo_b, np.float64))
    sync()
    sc["keep"] = (d_raw, d_odo)
    return {
        "ndt_sessions_step": lambda: ses.step(scans_a, odo_a, act_a),
        "ndt_sessions_step_dev": lambda: ses.step_dev(d_raw.data_ptr(), 16, off, d_odo.data_ptr(), act_b),
        "ndt_sessions_correct": lambda: ses.correct({i: ses.trajectory(i)[0] for i in range(ses.n)}),
        "ndt_sessions_remake_closed": lambda: ses.remake_closed(range(ses.n)),
        "ndt_sessions_find_loops": lambda: ses.find_loops(lp),
        "ndt_sessions_find_loops_multi": lambda: ses.find_loops_multi(mp),
        "ndt_sessions_cross_candidates": lambda: ses.cross_candidates(mp),
        "ndt_sessions_find_cross_loops": lambda: ses.find_cross_loops(mp),
        "ndt_sessions_occ_integrate": lambda: ses.occ_integrate(grids),
        "ndt_sessions_occ_rebuild": lambda: ses.occ_rebuild(grids),
    }


def triple(st):
    return st.host_waits, st.h2d_bytes, st.d2h_bytes


def fields(st):
    """Every field of an ndt_sessions_stats."""
    return tuple(getattr(st, name) for name, _ in st._fields_)


def test_find_cross_loops_counts_the_gate_once(scene):
    """find_cross_loops' waits and bytes are cross_candidates' plus those of a search of find_loops_multi's shape over its
    candidates -- no more: the figures of the commit before the bracket, and the search's read-back from its definition."""
    capi, ses = scene["capi"], scene["ses"]
    mp = capi.default_loop_multi_params(max_submaps=3, **LP)
    gate_n = len(ses.cross_candidates(mp))
    gate = triple(ses.stats())
    loops = ses.find_cross_loops(mp)
    cross, stepped = triple(ses.stats()), ses.stats().sessions_stepped
    multi_n = len(ses.find_loops_multi(mp))
    multi = triple(ses.stats())
    print("gate %s (%d candidates), cross %s, multi %s (%d candidates)" % (gate, gate_n, cross, multi, multi_n))
    assert len(loops) == gate_n == stepped and gate_n >= 2 and multi_n >= 2

    def search_d2h(J):      # the boxes of J maps; per slot a record, its index, its score, its statistics; per candidate a count
        return J * 64 + J * LP["top_k"] * (capi.RESULT_DTYPE.itemsize + 16 + capi.FIT_STATS_DTYPE.itemsize) + J * 4

    assert cross[0] == gate[0] + 2 and multi[0] == 2
    assert cross[2] == gate[2] + search_d2h(gate_n) and multi[2] == search_d2h(multi_n)
    assert cross[1] > gate[1] > 0
    assert (gate, cross, multi) == (PARENT_GATE, PARENT_CROSS, PARENT_MULTI)


def test_named_session_refusals_come_in_the_order_of_the_entries(scene):
    """Per entry: out of range, not started, named twice -- then (correct) its trajectory's refusals -- and only behind every
    entry the set-wide ones: no scan archive (remake_closed), then the pending map."""
    capi, ctx, ses, plain, own, cloud = (scene[k] for k in ("capi", "ctx", "ses", "plain", "own", "cloud"))
    lib, E = capi.lib(), capi.NDT_E_ARG
    err = lambda: lib.ndt_last_error(ctx.h).decode()
    status = np.zeros(4, np.int32)
    trajs = [np.ascontiguousarray(plain.trajectory(i)[0]) for i in range(plain.n)]

    def remake(s, which):
        w = np.array(which, np.int32)
        return lib.ndt_sessions_remake_closed(s.h, w.ctypes.data, len(w), status.ctypes.data)

    def correct(s, which, poses, ns=None):
        w = np.array(which, np.int32)
        ptrs = (ctypes.c_void_p * len(w))(*[None if a is None else a.ctypes.data for a in poses])
        n = np.array(ns if ns is not None else [0 if a is None else len(a) for a in poses], np.uintp)
        return lib.ndt_sessions_correct(s.h, w.ctypes.data, len(w), ptrs, n.ctypes.data, status.ctypes.data)

    before = fields(plain.stats())
    own.rebuild_begin(cloud.data_ptr(), len(cloud))
    try:
        # remake_closed on a set without an archive, a map pending: the entries first, in their order
        f = "ndt_sessions_remake_closed: "
        assert remake(plain, [5, 0, 0]) == E and err() == f + "entry 0: session 5 out of range"
        assert remake(plain, [0, 0, 5]) == E and err() == f + "entry 1: session 0 is entry 0 again"
        assert remake(plain, [0, 1]) == E and err() == f + "the set has no scan archive (ndt_sessions_archive_enable)"
        assert remake(ses, [0, 1]) == E and err() == f + "an ndt_map_rebuild_begin is open on the context"
        # correct: an entry's own refusals before the next entry's, all of them before the pending map
        f = "ndt_sessions_correct: "
        assert correct(plain, [5, 0, 0], [trajs[0]] * 3) == E and err() == f + "entry 0: session 5 out of range"
        assert correct(plain, [0, 0, 5], [trajs[0]] * 3) == E and err() == f + "entry 1: session 0 is entry 0 again"
        assert correct(plain, [0, 5], [None, trajs[0]]) == E and err() == f + "entry 0: session 0: NULL trajectory"
        assert correct(plain, [0, 5], [trajs[0], trajs[0]], ns=[1, 2]) == E and err().startswith(f + "entry 0: session 0: 1 poses for")
        bad = trajs[1].copy()
        bad[1, 2] = np.nan
        assert correct(plain, [1, 1], [bad, trajs[1]]) == E and err() == f + "entry 0: session 1: scan 1: a pose is not finite"
        assert correct(plain, [0, 1], trajs) == E and err() == f + "an ndt_map_rebuild_begin is open on the context"
    finally:
        own.rebuild_end()
    assert fields(plain.stats()) == before
    assert remake(plain, [0, 1]) == E and "no scan archive" in err()
    assert correct(plain, [0, 1], trajs) == capi.NDT_OK


def test_a_pending_map_refuses_every_call_and_touches_nothing(scene):
    """(The module's last test on the set: the calls that succeed behind ndt_map_rebuild_end step it.)"""
    capi, ctx, ses, own, cloud = (scene[k] for k in ("capi", "ctx", "ses", "own", "cloud"))
    calls = the_calls(scene)
    assert tuple(calls) == CALLS
    ses.find_loops_multi(capi.default_loop_multi_params(max_submaps=3, **LP))      # stats that are not all zero
    stats, before, counts = fields(ses.stats()), state(scene), grid_counts(scene)
    assert all(stats[:3])
    own.rebuild_begin(cloud.data_ptr(), len(cloud))
    try:
        for name, call in calls.items():
            with pytest.raises(capi.NdtError) as e:
                call()
            head = "%s -> %d: %s: " % (name, capi.NDT_E_ARG, name)
            assert str(e.value).startswith(head) and "an ndt_map_rebuild_begin is open on the context" in str(e.value), (name, str(e.value))
            assert capi.lib().ndt_last_error(ctx.h).decode().startswith(name + ": "), name
            assert fields(ses.stats()) == stats, name
        assert state(scene) == before
    finally:
        own.rebuild_end()
    assert state(scene) == before and grid_counts(scene) == counts
    # the set is alive: the same calls succeed, the searches and the grids first, the steps last
    for name in CALLS[4:] + CALLS[2:4] + CALLS[:2]:
        calls[name]()
    assert ses.stats().sessions_stepped == len(SPECS) and len(ses.trajectory(0)[0]) == STEPPED + 2
