"""ndt_sessions_*: device-resident lockstep sessions.  A step equals, byte for byte, the same step made of the existing
batched *_dev entry points with every scan triple recomputed (session_helpers.ComposedChain); sessions do not see each
other; the host path (replay.run_sessions) is reproduced within the project's parity bound; transfers and host waits of a
step do not depend on the number of sessions or the length of a submap."""
import ctypes

import numpy as np
import pytest

from session_helpers import ComposedChain, device_cloud, lockstep, same_records, session_logs
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

SPECS = ((33, 14), (34, 9), (35, 12), (36, 7), (37, 10))         # (seed, frames) of the five sessions
STARTS = [0, 0, 3, 0, 0]                                         # session 2 starts late


def launch_params(**kw):
    from ndt_slam_amd import replay
    return dict(replay.LAUNCH_PARAMS, **kw)


def views(ses, i):
    """(local map, p_cloud) of session i, read from the device."""
    tp, tn, _ = ses.local_map(i)
    cp, cn = ses.submap_cloud(i)
    return device_cloud(tp, tn), device_cloud(cp, cn)


def run_set(capi, ctx, logs, starts, p, order=None, with_views=True):
    """Steps `logs` through one capi.Sessions set (sessions in `order`) -> per step {session: (record, target, cloud)},
    and every session's global map at the end; keys are the sessions' indices in `logs`."""
    order = list(range(len(logs))) if order is None else list(order)
    ses = capi.Sessions(ctx, len(order), capi.session_params_from_launch(p))
    hist = []
    for k, scans, odo, act in lockstep([logs[i] for i in order], [starts[i] for i in order]):
        recs = ses.step(scans, odo, act)
        hist.append({i: (recs[j].copy(),) + (views(ses, j) if with_views and recs[j]["stepped"] else (None, None))
                     for j, i in enumerate(order)})
    glob = {i: ses.global_map(j) for j, i in enumerate(order)}
    ses.close()
    return hist, glob


@pytest.mark.parametrize("remove_moving", [True, False])
def test_step_equals_the_composed_chain(gpu, remove_moving):
    """5 sessions of different lengths, one starting late, sepThre = 2.5 m: per step and session the record, the local map,
    Submap::p_cloud and the NDT map's export are the bytes of the chain of *_dev entry points that recomputes every triple,
    also at every later step in which the session (1, 3 and 4 end early) does not step; at the end so is the global map."""
    capi, ctx = gpu
    p = launch_params(sepThre=2.5, removeMoving=remove_moving)
    logs = session_logs(SPECS)
    S = len(logs)
    ses = capi.Sessions(ctx, S, capi.session_params_from_launch(p))
    chain = ComposedChain(capi, ctx, S, p)
    splits, seen = [0] * S, [False] * S
    for k, scans, odo, act in lockstep(logs, STARTS):
        got, want = ses.step(scans, odo, act), chain.step(scans, odo, act)
        for i in range(S):
            assert same_records(got[i], want[i]), (k, i, got[i], want[i])
            assert bool(got[i]["stepped"]) == bool(act[i])
            if not got[i]["stepped"] and not seen[i]:
                continue
            # (a session that has stepped and does not now keeps its views: the chain's last ones, carried to this step's arenas)
            seen[i] = True
            splits[i] += int(got[i]["split"])
            target, cloud = views(ses, i)
            assert cloud.tobytes() == chain.p_cloud[i].tobytes(), (k, i, len(cloud), len(chain.p_cloud[i]))
            assert target.tobytes() == chain.target[i].tobytes(), (k, i, len(target), len(chain.target[i]))
            a, b = ses.map_export(i), chain.maps[i].export()
            assert all(a[f].tobytes() == b[f].tobytes() for f in b), (k, i)
        st = ses.stats()
        assert st.triples_run <= st.sessions_stepped == int(act.sum())
    assert sorted(splits)[-1] >= 2 and sum(1 for s in splits if s >= 1) >= 2, splits
    for i in range(S):
        g, parts = ses.global_map(i)
        wg, wparts = chain.global_map(i)
        assert g.tobytes() == np.ascontiguousarray(wg, np.float32).tobytes(), i
        assert len(parts) == len(wparts) and all(x.tobytes() == np.ascontiguousarray(y, np.float32).tobytes()
                                                  for x, y in zip(parts, wparts))
    ses.close()
    chain.close()


def test_sessions_do_not_see_each_other(gpu):
    """Session i's records and clouds are the same bytes in a set of 1 and in the set of 5, in both session orders."""
    capi, ctx = gpu
    p = launch_params(sepThre=2.5)
    logs = session_logs(SPECS)
    S = len(logs)
    solo = []
    for i in range(S):
        hist, glob = run_set(capi, ctx, [logs[i]], [STARTS[i]], p)
        solo.append(([h[0] for h in hist], glob[0]))
    for order in (list(range(S)), list(range(S))[::-1]):
        hist, glob = run_set(capi, ctx, logs, STARTS, p, order=order)
        for i in range(S):
            mine = [h[i] for h in hist if h[i][0]["stepped"]]
            alone = [h for h in solo[i][0] if h[0]["stepped"]]
            assert len(mine) == len(alone) == SPECS[i][1]
            for a, b in zip(mine, alone):
                assert same_records(a[0], b[0]), (order, i)
                assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes(), (order, i)
            assert glob[i][0].tobytes() == solo[i][1][0].tobytes()


class RecordingSessions:
    """capi.Sessions with every step's records kept."""

    def __init__(self, ses):
        self.ses, self.records = ses, []

    def step(self, scans, odo, active=None):
        r = self.ses.step(scans, odo, active)
        self.records.append((np.array(active, np.uint8), r))
        return r

    def global_map(self, i):
        return self.ses.global_map(i)

    def close(self):
        self.ses.close()


def test_resident_replay_reproduces_the_host_path(gpu, tmp_path):
    """The four logs of test_lockstep_replay_on_the_device: run_sessions_resident reproduces run_sessions' accepted lists
    and split steps completely, and every pose within 1e-4 m / 1e-4 rad (README's parity bound).  The two paths differ in
    the yaw read from the final transform (the modelled asinf / acosf on the device, the platform's on the host) and in
    the fusion arithmetic (device fp64 kernels vs numpy).  A miss reports the first step and term beyond the bound."""
    capi, ctx = gpu
    from ndt_slam_amd import replay, synth
    paths = []
    for i, (seed, n) in enumerate(((33, 14), (34, 9), (35, 12), (36, 6))):
        recs, _ = synth.replay_records(n_frames=n, n_beams=181, step=0.6, seed=seed)
        replay.write_log(tmp_path / ("log%d.txt" % i), recs)
        paths.append(tmp_path / ("log%d.txt" % i))
    p = launch_params(end_frame=20, sepThre=5.0)
    launchers = [replay.SlamLauncher(ctx, **p) for _ in paths]
    host = replay.run_sessions(ctx, [replay.read_log(q, sidelidar=False) for q in paths], launchers=launchers)
    rec = RecordingSessions(capi.Sessions(ctx, len(paths), capi.session_params_from_launch(p)))
    res = replay.run_sessions_resident(ctx, [replay.read_log(q, sidelidar=False) for q in paths],
                                       poses_names=[tmp_path / ("res%d.txt" % i) for i in range(4)], sessions=rec, **p)
    rec.close()
    for i, L in enumerate(launchers):
        mine = [r[i] for a, r in rec.records if a[i]]
        assert len(res[i]) == len(host[i]) == len(mine)
        accepted = [bool(r["successful"]) for r in mine if r["matched"]]
        assert accepted == L.smat.accepted, (i, accepted, L.smat.accepted)
        # split steps: the scan index at which each submap of the session starts
        starts = [k for k, r in enumerate(mine) if r["split"]]
        assert starts == [s.cntS for s in L.pcmap.submaps[1:]], (i, starts)
        for k, (a, b) in enumerate(zip(res[i], host[i])):
            d = (abs(a.tx - b.tx), abs(a.ty - b.ty), abs(np.radians((a.th - b.th + 180.0) % 360.0 - 180.0)))
            print("session %d step %d: |dx| %.3g |dy| %.3g |dth| %.3g rad" % ((i, k) + d))
            for term, v in zip(("tx", "ty", "th"), d):
                assert v < 1e-4, "session %d: first miss at step %d, term %s: %.3g" % (i, k, term, v)


def test_transfers_and_waits_do_not_grow(gpu):
    """One submap growing from 1 to 13 scans (no split), S in {1, 4, 32}: host_waits is the same at every step and for
    every S; the bytes uploaded beyond the raw scans are the same at every step for equal S; at most one triple per
    stepped session."""
    capi, ctx = gpu
    p = launch_params(sepThre=1e9)
    log = session_logs(((33, 13),), n_beams=121)[0]
    waits = set()
    for S in (1, 4, 32):
        ses = capi.Sessions(ctx, S, capi.session_params_from_launch(p))
        extra = set()
        for k, scans, odo, act in lockstep([log] * S):
            recs = ses.step(scans, odo, act)
            assert recs["stepped"].all() and not recs["split"].any()
            st = ses.stats()
            raw = sum(len(x) for x in scans) * 16
            waits.add(st.host_waits)
            extra.add(st.h2d_bytes - raw)
            assert st.sessions_stepped == S and st.triples_run == (S if k >= 2 else 0)
            assert st.triples_run <= st.sessions_stepped
        assert len(extra) == 1, (S, extra)
        ses.close()
    assert waits == {3}, waits


def test_bad_scan_skips_that_session_alone(gpu):
    """A non-finite raw coordinate: that session's step is skipped (status NDT_E_ARG, stepped 0), the other session is
    untouched, and the session's next step equals that of a run in which it was inactive instead."""
    capi, ctx = gpu
    p = launch_params(sepThre=2.5)
    logs = session_logs(SPECS[:2])
    bad = [[x.copy() for x in logs[1][0]], logs[1][1]]
    bad[0][4][7, 1] = np.inf
    a, _ = run_set(capi, ctx, [logs[0], bad], [0, 0], p)
    ses = capi.Sessions(ctx, 2, capi.session_params_from_launch(p))
    b = []
    for k, scans, odo, act in lockstep(logs[:2]):
        if k == 4:
            act[1] = 0
        recs = ses.step(scans, odo, act)
        b.append({i: (recs[i].copy(),) + (views(ses, i) if recs[i]["stepped"] else (None, None)) for i in range(2)})
    ses.close()
    assert a[4][1][0]["status"] == capi.NDT_E_ARG and not a[4][1][0]["stepped"]
    for k in range(len(a)):
        for i in range(2):
            if k == 4 and i == 1:
                continue
            assert same_records(a[k][i][0], b[k][i][0]), (k, i)
            if a[k][i][0]["stepped"]:
                assert a[k][i][1].tobytes() == b[k][i][1].tobytes() and a[k][i][2].tobytes() == b[k][i][2].tobytes()


def test_empty_scan_and_idle_step(gpu):
    """An empty raw scan on a matched step is what the chain of *_dev calls makes of it (ndt_align_batch_multi's NDT_E_ARG
    record: the not-converged cost, the predicted pose, a scan of no points in the submap); a step with `active` all zero
    is valid and changes nothing."""
    capi, ctx = gpu
    p = launch_params(sepThre=2.5)
    logs = session_logs(SPECS[:2])
    logs[1][0][3] = np.zeros((0, 2))
    S = 2
    ses = capi.Sessions(ctx, S, capi.session_params_from_launch(p))
    chain = ComposedChain(capi, ctx, S, p)
    for k, scans, odo, act in lockstep(logs):
        if k == 5:
            idle = ses.step(scans, odo, np.zeros(S, np.uint8))
            assert not idle["stepped"].any() and not idle["status"].any()
            st = ses.stats()
            assert (st.h2d_bytes, st.d2h_bytes, st.host_waits, st.triples_run, st.sessions_stepped) == (0, 0, 0, 0, 0)
        got, want = ses.step(scans, odo, act), chain.step(scans, odo, act)
        for i in range(S):
            assert same_records(got[i], want[i]), (k, i, got[i], want[i])
            if got[i]["stepped"]:
                target, cloud = views(ses, i)
                assert cloud.tobytes() == chain.p_cloud[i].tobytes() and target.tobytes() == chain.target[i].tobytes(), (k, i)
        if k == 3:
            assert got[1]["cost"] == 1e7 and not got[1]["successful"] and got[1]["matched"]
    ses.close()
    chain.close()


def test_refusals_name_their_index_and_leave_out_alone(gpu):
    capi, ctx = gpu
    L = capi.lib()
    err = lambda: L.ndt_last_error(ctx.h).decode()
    h = ctypes.c_void_p()
    prm = capi.default_session_params()
    assert L.ndt_sessions_create(ctx.h, 0, ctypes.byref(prm), ctypes.byref(h)) == capi.NDT_E_ARG and "n_sessions < 1" in err()
    for kw, text in ((dict(leaf=0.0), "leaf <= 0"), (dict(resol=0.0), "resol"), (dict(space=0.0), "space"),
                     (dict(match_resolution=0.0), "resolution"), (dict(fuse_del_time=0.0), "del_time")):
        bad = capi.default_session_params(**kw)
        assert L.ndt_sessions_create(ctx.h, 2, ctypes.byref(bad), ctypes.byref(h)) == capi.NDT_E_ARG and text in err(), kw
        assert not h.value
    ses = capi.Sessions(ctx, 3)
    scan = session_logs(((33, 1),), n_beams=61)[0][0][0]
    xy = np.ascontiguousarray(np.concatenate([scan] * 3))
    n = len(scan)
    odo = np.zeros((3, 3))
    out = np.full(3 * capi.SESSION_STEP_DTYPE.itemsize, 0xA5, np.uint8)
    canary = out.copy()

    def step(off, stride=16, odo_ptr=odo.ctypes.data):
        off = np.array(off, np.uint64)
        return L.ndt_sessions_step(ses.h, xy.ctypes.data, stride, off.ctypes.data, odo_ptr, None, out.ctypes.data)

    assert step([0, n, 2 * n, 3 * n], stride=12) == capi.NDT_E_ARG and "stride" in err()
    assert step([0, n, n - 1, 3 * n]) == capi.NDT_E_ARG and "session 1" in err() and "decrease" in err()
    assert step([0, n, 2 * n, 3 * n], odo_ptr=None) == capi.NDT_E_ARG and "NULL" in err()
    assert L.ndt_sessions_step(ses.h, xy.ctypes.data, 16, None, odo.ctypes.data, None, out.ctypes.data) == capi.NDT_E_ARG
    cloud = np.ascontiguousarray(scan, np.float32)
    m = capi.Map(ctx, cloud)
    import torch
    d = torch.from_numpy(cloud).to("cuda:0")
    torch.cuda.synchronize()
    m.rebuild_begin(d.data_ptr(), len(cloud))
    assert step([0, n, 2 * n, 3 * n]) == capi.NDT_E_ARG and "ndt_map_rebuild_begin" in err()
    m.rebuild_end()
    assert out.tobytes() == canary.tobytes()
    p, k = ctypes.c_void_p(), ctypes.c_size_t()
    assert L.ndt_sessions_submap_cloud(ses.h, 3, ctypes.byref(p), ctypes.byref(k)) == capi.NDT_E_ARG and "session 3" in err()
    # the set is as it was: a valid step goes through
    assert step([0, n, 2 * n, 3 * n]) == capi.NDT_OK
    recs = np.frombuffer(out.tobytes(), dtype=capi.SESSION_STEP_DTYPE)
    assert recs["stepped"].all() and not recs["matched"].any()
    m.close()
    ses.close()


def test_two_rounds_on_one_context_equal_fresh_runs(gpu):
    """create / step / destroy twice round on one context, with a single ndt_align in between: the same bytes."""
    capi, ctx = gpu
    from ndt_slam_amd import synth
    p = launch_params(sepThre=2.5)
    logs = session_logs(SPECS[:3])
    a, ga = run_set(capi, ctx, logs, STARTS[:3], p)
    cfg = synth.CONFIGS["C1"]
    world = synth.make_map(cfg["n_map"], cfg["half"])
    scan, _, init = synth.ScanFactory(world, cfg["half"], cfg["n_scan"]).make(0)
    m = capi.Map(ctx, world, capi.default_params(resolution=cfg["resolution"]))
    assert m.align(scan, init)["status"] == 0
    m.close()
    b, gb = run_set(capi, ctx, logs, STARTS[:3], p)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for i in x:
            assert same_records(x[i][0], y[i][0])
            if x[i][0]["stepped"]:
                assert x[i][1].tobytes() == y[i][1].tobytes() and x[i][2].tobytes() == y[i][2].tobytes()
    for i in ga:
        assert ga[i][0].tobytes() == gb[i][0].tobytes()
