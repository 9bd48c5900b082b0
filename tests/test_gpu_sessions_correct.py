"""ndt_sessions_correct and ndt_sessions_trajectory on the device: a resident set that takes an adjusted trajectory is, then
and at every later step, the composed chain that took the same one (session_correct_helpers.CorrectedChain: the moves by
ndt_repose_points, every triple of the current submap again by ndt_local_map_batch_dev, the map by ndt_map_build_batch_dev).
Every comparison is byte equality.  The logs are session_helpers.session_logs drives of 181 beams (matches are accepted:
tests/session_workloads.py), 0.609 m of odometry per step; with sepThre 1.5 a session splits at its steps 3, 6 and 9."""
import ctypes

import numpy as np
import pytest

import session_workloads as W
from session_correct_helpers import CorrectedChain, layout, smooth_adjustment
from session_helpers import device_cloud, lockstep, same_records, session_logs
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

SPECS, STARTS = ((33, 12), (34, 12), (35, 10)), [0, 0, 1]
_LOGS = {}


def logs_of(specs=SPECS):
    if specs not in _LOGS:
        _LOGS[specs] = session_logs(specs)
    return _LOGS[specs]


def views(ses, i):
    """(local map, p_cloud) of session i, read from the device."""
    tp, tn, _ = ses.local_map(i)
    cp, cn = ses.submap_cloud(i)
    return device_cloud(tp, tn), device_cloud(cp, cn)


def same_export(a, b):
    return (a is None) == (b is None) and (a is None or all(a[f].tobytes() == b[f].tobytes() for f in b))


def snapshot(ses, i):
    """Everything a caller can read of session i: both views, the map's export, the global map with its parts, the trajectory."""
    g, parts = ses.global_map(i)
    return views(ses, i) + (ses.map_export(i), g.copy(), [x.copy() for x in parts]) + ses.trajectory(i)


def same_snapshot(a, b):
    return (a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and same_export(a[2], b[2])
            and a[3].tobytes() == b[3].tobytes() and len(a[4]) == len(b[4]) and all(x.tobytes() == y.tobytes() for x, y in zip(a[4], b[4]))
            and a[5].tobytes() == b[5].tobytes() and a[6].tolist() == b[6].tolist() and a[7].tolist() == b[7].tolist() and a[8] == b[8])


def chain_poses(chain, i):
    return np.array([(q.tx, q.ty, q.th) for q in chain.pcmaps[i].poses], np.float64).reshape(-1, 3)


def same_state(ses, chain, i, tag):
    """Session i of the set against the chain: views, export, global map and parts, trajectory and its layout."""
    target, cloud = views(ses, i)
    assert cloud.tobytes() == chain.p_cloud[i].tobytes(), (tag, i, len(cloud), len(chain.p_cloud[i]))
    assert target.tobytes() == chain.target[i].tobytes(), (tag, i, len(target), len(chain.target[i]))
    assert same_export(ses.map_export(i), chain.maps[i].export() if chain.maps[i] is not None else None), (tag, i)
    g, parts = ses.global_map(i)
    wg, wparts = chain.global_map(i)
    assert g.tobytes() == np.ascontiguousarray(wg, np.float32).tobytes(), (tag, i)
    assert len(parts) == len(wparts) and all(x.tobytes() == np.ascontiguousarray(y, np.float32).tobytes()
                                              for x, y in zip(parts, wparts)), (tag, i)
    poses, sub_first, sub_anchor, store_first = ses.trajectory(i)
    assert poses.tobytes() == chain_poses(chain, i).tobytes(), (tag, i)
    if len(poses):
        firsts, anchors, first = layout(chain.pcmaps[i])
        assert sub_first.tolist() == firsts and sub_anchor.tolist() == anchors and store_first == first, (tag, i)
    else:
        assert sub_first.tolist() == [0] and store_first == 0, (tag, i)


def due(case, k, recs0):
    """Whether the correction of `case` comes behind step k, from session 0's records so far."""
    splits = [j for j, r in enumerate(recs0) if r["split"]]
    if case == "first_scan":                     # one scan: the cloud holds it twice
        return k == 0
    if case == "at_split":
        return splits == [k]
    if case == "after_split":
        return len(splits) >= 1 and k == splits[0] + 2
    return len(splits) >= 2 and k == splits[1] + 1          # two_closed


@pytest.mark.parametrize("case", ["first_scan", "at_split", "after_split", "two_closed"])
@pytest.mark.parametrize("rm", [1, 0])
def test_equal_to_the_chain_then_and_after(gpu, rm, case):
    capi, ctx = gpu
    logs, p = logs_of(), W.launch_params(sepThre=1.5, removeMoving=bool(rm))
    S = len(logs)
    ses = capi.Sessions(ctx, S, capi.session_params_from_launch(p))
    chain = CorrectedChain(capi, ctx, S, p)
    recs0, corrected_at = [], None
    for k, scans, odo, act in lockstep(logs, STARTS):
        got, want = ses.step(scans, odo, act), chain.step(scans, odo, act)
        for i in range(S):
            assert same_records(got[i], want[i]), (case, k, i, got[i], want[i])
            target, cloud = views(ses, i)
            assert cloud.tobytes() == chain.p_cloud[i].tobytes() and target.tobytes() == chain.target[i].tobytes(), (case, k, i)
            assert same_export(ses.map_export(i), chain.maps[i].export() if chain.maps[i] is not None else None), (case, k, i)
        recs0.append(got[0].copy())
        if corrected_at is None and due(case, k, recs0):
            corrected_at = k
            who = [i for i in (0, 2) if chain.started[i]]
            new = {i: smooth_adjustment(chain_poses(chain, i)) for i in who}
            for i in range(S):
                same_state(ses, chain, i, (case, k, "before"))
            status = ses.correct(new)
            assert status == {i: capi.NDT_OK for i in who}
            assert all(chain.correct(i, new[i]) == capi.NDT_OK for i in who)
            st = ses.stats()
            assert st.sessions_stepped == len(who) and st.host_waits <= 3
            for i in range(S):                    # (session 1 is not named)
                same_state(ses, chain, i, (case, k, "after"))
                if i in who:
                    assert ses.trajectory(i)[0].tobytes() == new[i].tobytes()
    assert corrected_at is not None and corrected_at <= k - 3, (case, corrected_at)
    if case == "two_closed":
        assert len(chain.pcmaps[0].submaps) >= 3
    for i in range(S):
        same_state(ses, chain, i, (case, "end"))
    ses.close()
    chain.close()


def run_pair(capi, ctx, logs, starts, p, at, correct):
    """Two sets stepped side by side; behind step `at`, correct(a) is called on the first.  Yields (k, a, b, got_a, got_b) per
    step, behind the correction where there is one."""
    S = len(logs)
    a, b = (capi.Sessions(ctx, S, capi.session_params_from_launch(p)) for _ in range(2))
    try:
        for k, scans, odo, act in lockstep(logs, starts):
            ga, gb = a.step(scans, odo, act), b.step(scans, odo, act)
            if k == at:
                correct(a)
            yield k, a, b, ga, gb
    finally:
        a.close()
        b.close()


def test_identity_changes_no_byte(gpu):
    """The stored trajectory given back: no view, export, global map or later record changes against an uncorrected twin."""
    capi, ctx = gpu
    logs, p = logs_of(), W.launch_params(sepThre=1.5)
    S, at = len(logs), 7
    before = {}

    def correct(a):
        for i in range(S):
            before[i] = snapshot(a, i)
        assert a.correct({i: a.trajectory(i)[0] for i in range(S)}) == {i: capi.NDT_OK for i in range(S)}

    for k, a, b, ga, gb in run_pair(capi, ctx, logs, STARTS, p, at, correct):
        for i in range(S):
            assert same_records(ga[i], gb[i]), (k, i)
            assert same_snapshot(snapshot(a, i), snapshot(b, i)), (k, i)
            if k == at:
                assert same_snapshot(snapshot(a, i), before[i]), i
                assert len(before[i][4]) >= 2                      # (closed clouds took part)
    assert k > at + 2


def test_partial_adjustment_leaves_the_first_closed_cloud_alone(gpu):
    """Every pose of the first closed submap bit-equal: its cloud keeps its bytes in the global map; the second closed cloud is
    ndt_repose_points of what it was, by its anchor's pair."""
    capi, ctx = gpu
    logs, p = logs_of(), W.launch_params(sepThre=1.5)
    ses = capi.Sessions(ctx, len(logs), capi.session_params_from_launch(p))
    done = False
    for k, scans, odo, act in lockstep(logs, STARTS):
        ses.step(scans, odo, act)
        old, sub_first, sub_anchor, _ = ses.trajectory(0)
        if len(sub_first) == 3 and not done:
            done = True
            _, parts = ses.global_map(0)
            parts = [x.copy() for x in parts]
            new = smooth_adjustment(old, start=int(sub_first[1]))
            assert sub_anchor[0] < sub_first[1] <= sub_anchor[1] and new[:sub_first[1]].tobytes() == old[:sub_first[1]].tobytes()
            assert ses.correct({0: new}) == {0: capi.NDT_OK}
            _, after = ses.global_map(0)
            assert len(after) == 3 and len(parts[0]) and len(parts[1])
            assert after[0].tobytes() == parts[0].tobytes()
            a = int(sub_anchor[1])
            want = capi.repose_points(ctx, parts[1], [0, len(parts[1])], old[a:a + 1], new[a:a + 1])
            assert after[1].tobytes() == want.tobytes() and after[1].tobytes() != parts[1].tobytes()
    assert done
    ses.close()


def test_neighbours_of_a_corrected_session_are_untouched(gpu):
    """One session of three corrected: the other two are, then and at every later step, those of a set without the call."""
    capi, ctx = gpu
    logs, p = logs_of(), W.launch_params(sepThre=1.5)
    at = 5

    def correct(a):
        assert a.correct({1: smooth_adjustment(a.trajectory(1)[0])}) == {1: capi.NDT_OK}

    differs = False
    for k, a, b, ga, gb in run_pair(capi, ctx, logs, STARTS, p, at, correct):
        for i in (0, 2):
            assert same_records(ga[i], gb[i]), (k, i)
            assert same_snapshot(snapshot(a, i), snapshot(b, i)), (k, i)
        differs = differs or (k >= at and not same_snapshot(snapshot(a, 1), snapshot(b, 1)))
    assert differs and k > at + 2


def test_span_error_costs_its_session_alone(gpu):
    """One scan of the current submap sent to tx = 1e8: its triples span more than 2^30 voxels.  That session gets NDT_E_ARG,
    empty views and keeps its map; its trajectory is the new one; the neighbour keeps every byte; the set steps on."""
    capi, ctx = gpu
    logs, p = logs_of(((33, 7), (34, 7))), W.launch_params(sepThre=1e9)
    at, seen = 4, {}

    def correct(a):
        seen["export"], seen["other"] = a.map_export(0), snapshot(a, 1)
        new = a.trajectory(0)[0].copy()
        assert len(new) == at + 1
        new[at - 1, 0] = 1e8
        assert a.correct({0: new, 1: a.trajectory(1)[0]}) == {0: capi.NDT_E_ARG, 1: capi.NDT_OK}          # (the call returns NDT_OK)
        target, cloud = views(a, 0)
        assert len(target) == 0 and len(cloud) == 0
        assert seen["export"] is not None and same_export(a.map_export(0), seen["export"])
        assert a.trajectory(0)[0].tobytes() == new.tobytes()
        assert same_snapshot(snapshot(a, 1), seen["other"])

    for k, a, b, ga, gb in run_pair(capi, ctx, logs, [0, 0], p, at, correct):
        assert same_records(ga[1], gb[1]) and same_snapshot(snapshot(a, 1), snapshot(b, 1)), k
        assert ga[0]["stepped"] == 1, k
    assert k == at + 2


def test_refusals_name_their_entry_and_change_nothing(gpu):
    capi, ctx = gpu
    L, E = capi.lib(), capi.NDT_E_ARG
    err = lambda: L.ndt_last_error(ctx.h).decode()
    logs, p = logs_of(((33, 3), (34, 3), (35, 1))), W.launch_params(sepThre=1e9)
    ses = capi.Sessions(ctx, 3, capi.session_params_from_launch(p))
    for k, scans, odo, act in lockstep(logs, [0, 0, 9]):
        if k < 3:
            ses.step(scans, odo, act)
    traj = [ses.trajectory(i)[0] for i in range(3)]
    assert [len(t) for t in traj] == [3, 3, 0]
    before = [snapshot(ses, i) for i in range(3)]
    status = np.full(4, 77, np.int32)

    def call(which, trajs, ns=None, h=ses.h):
        w = np.array(which or [0], np.int32)          # (n_corr = 0 with arrays that are not NULL)
        arrs = [np.ascontiguousarray(t, np.float64) for t in trajs]
        ptrs = (ctypes.c_void_p * max(len(arrs), 1))(*[a.ctypes.data if a.size else None for a in arrs])
        n = np.array(([len(a) for a in arrs] if ns is None else ns) or [0], np.uintp)
        return L.ndt_sessions_correct(h, w.ctypes.data, len(which), ptrs, n.ctypes.data, status.ctypes.data)

    assert call([0], [traj[0]], h=None) == E and "null session set" in L.ndt_last_error(None).decode()
    n1 = np.array([3], np.uintp)
    assert L.ndt_sessions_correct(ses.h, None, 1, None, n1.ctypes.data, status.ctypes.data) == E and "NULL" in err()
    assert call([], []) == E and "n_corr < 1" in err()
    assert call([0, 3], [traj[0], traj[0]]) == E and "entry 1" in err() and "session 3" in err()
    assert call([-1], [traj[0]]) == E and "entry 0" in err() and "session -1" in err()
    assert call([1, 2], [traj[1], np.zeros((1, 3))]) == E and "entry 1" in err() and "session 2" in err() and "not started" in err()
    assert call([0, 1, 0], [traj[0], traj[1], traj[0]]) == E and "entry 2" in err() and "session 0" in err() and "again" in err()
    assert call([0, 1], [traj[0], traj[1][:2]]) == E and "entry 1" in err() and "session 1" in err() and "stale" in err()
    bad = traj[1].copy()
    bad[1, 2] = np.nan
    assert call([0, 1], [traj[0], bad]) == E and "session 1" in err() and "scan 1" in err() and "not finite" in err()
    bad[1, 2] = np.inf
    assert call([1], [bad]) == E and "scan 1" in err()
    cloud = np.ascontiguousarray(logs[0][0][0], np.float32)
    m = capi.Map(ctx, cloud)
    import torch
    d = torch.from_numpy(cloud).to("cuda:0")
    torch.cuda.synchronize()
    m.rebuild_begin(d.data_ptr(), len(cloud))
    assert call([0], [traj[0]]) == E and "ndt_map_rebuild_begin" in err()
    m.rebuild_end()
    m.close()
    assert status.tolist() == [77] * 4
    assert all(same_snapshot(snapshot(ses, i), before[i]) for i in range(3))
    # the read-out's own refusals
    n = ctypes.c_size_t()
    buf = np.zeros((2, 3))
    assert L.ndt_sessions_trajectory(ses.h, 3, None, 0, ctypes.byref(n), None, None, None, None) == E and "session 3" in err()
    assert L.ndt_sessions_trajectory(ses.h, 0, buf.ctypes.data, 2, ctypes.byref(n), None, None, None, None) == E and "capacity" in err()
    assert L.ndt_sessions_trajectory(None, 0, None, 0, ctypes.byref(n), None, None, None, None) == E
    # the set is as it was: a valid correction goes through
    assert ses.correct({0: smooth_adjustment(traj[0])}) == {0: capi.NDT_OK}
    ses.close()


def test_waits_do_not_depend_on_the_sessions_corrected(gpu):
    """One session, then three whose current submaps hold different numbers of scans: the same host waits (at most 3), and
    triples_run is the number of triples in the corrected submaps."""
    capi, ctx = gpu
    logs, p = logs_of(), W.launch_params(sepThre=1.5)
    S = len(logs)
    ses = capi.Sessions(ctx, S, capi.session_params_from_launch(p))
    for k, scans, odo, act in lockstep(logs, STARTS):
        ses.step(scans, odo, act)
        if k == 8:
            break
    traj = [ses.trajectory(i) for i in range(S)]
    held = [len(t[0]) - t[3] for t in traj]
    assert len(set(held)) >= 2 and min(held) >= 3, held
    ses.correct({1: smooth_adjustment(traj[1][0])})
    one = ses.stats()
    assert (one.sessions_stepped, one.triples_run) == (1, held[1] - 2)
    ses.correct({i: smooth_adjustment(ses.trajectory(i)[0], scale=0.5) for i in range(S)})
    three = ses.stats()
    assert (three.sessions_stepped, three.triples_run) == (S, sum(h - 2 for h in held))
    assert one.host_waits == three.host_waits <= 3
    assert three.h2d_bytes > one.h2d_bytes > 0 and three.d2h_bytes > one.d2h_bytes > 0
    ses.close()


def test_end_to_end_from_trajectory_to_corrected_state(gpu):
    """trajectory -> odometry arcs (ndt_pg_edge_between) + one loop arc from the generator's true poses -> ndt_pg_optimize_batch ->
    correct: the trajectory reads back the optimiser's bytes and the state is the chain's.  No accuracy claim."""
    capi, ctx = gpu
    from ndt_slam_amd import synth
    n = 10
    recs, truth = synth.replay_records(n_frames=n, n_beams=181, step=0.6, seed=33)
    logs = [([np.asarray(r["front"], np.float64).reshape(-1, 2) for r in recs],
             np.array([[r["x"], r["y"], r["th"]] for r in recs], np.float64))]
    p = W.launch_params(sepThre=1.5)
    ses = capi.Sessions(ctx, 1, capi.session_params_from_launch(p))
    chain = CorrectedChain(capi, ctx, 1, p)
    for k, scans, odo, act in lockstep(logs):
        got, want = ses.step(scans, odo, act), chain.step(scans, odo, act)
        assert same_records(got[0], want[0]), k
    poses = ses.trajectory(0)[0]
    assert len(poses) == n and poses.tobytes() == chain_poses(chain, 0).tobytes()
    edges = np.zeros(n, dtype=capi.PG_EDGE_DTYPE)
    for j in range(n - 1):
        edges[j]["from"], edges[j]["to"] = j, j + 1
        edges[j]["rel"] = capi.pg_edge_between(poses[j], poses[j + 1])
        edges[j]["info"] = (100.0, 0.0, 0.0, 100.0, 0.0, 400.0)
    edges[n - 1]["from"], edges[n - 1]["to"] = 0, n - 1
    edges[n - 1]["rel"] = capi.pg_edge_between(truth[0], truth[n - 1])
    edges[n - 1]["info"] = (1000.0, 0.0, 0.0, 1000.0, 0.0, 4000.0)
    new, res = capi.optimize_pose_graphs(ctx, poses, [0, n], edges, [0, n])
    assert res[0]["status"] == 0 and res[0]["iterations"] >= 1 and new.tobytes() != poses.tobytes()
    assert ses.correct({0: new}) == {0: capi.NDT_OK} and chain.correct(0, new) == capi.NDT_OK
    assert ses.trajectory(0)[0].tobytes() == new.tobytes()
    same_state(ses, chain, 0, "end to end")
    ses.close()
    chain.close()
