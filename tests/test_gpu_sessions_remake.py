"""ndt_sessions_remake_closed on the device: every closed submap's cloud of a resident session again from the scan archive at
the poses the trajectory holds now.  The header's Definition is restated by session_remake_helpers.RemadeChain out of
ndt_resample, ndt_scan_to_map_batch_dev, ndt_local_map_batch_dev and ndt_map_build_batch_dev; on a set that was never corrected
the call must change no byte, which holds the scan-list rule and the transform to the set's own history.  Every comparison is
byte equality.  The workload is that of tests/test_gpu_sessions_correct.py: three drives of 181 beams, starts [0, 0, 1],
sepThre 1.5 -- a session splits at its steps 3, 6 and 9."""
import ctypes

import numpy as np
import pytest

import session_workloads as W
from loops_helpers import FULL_LAP, loop_workload
from session_correct_helpers import smooth_adjustment
from session_helpers import lockstep, same_records
from session_remake_helpers import RemadeChain
from test_gpu_sessions_correct import STARTS, chain_poses, due, logs_of, same_snapshot, same_state, snapshot
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu


def new_set(capi, ctx, S, p, archive=True):
    return capi.Sessions(ctx, S, capi.session_params_from_launch(p), archive=archive)


def stepped_pair(capi, ctx, logs, starts, p, n=2):
    """n archived sets stepped side by side: yields (k, sets, records per set) behind every step."""
    sets = [new_set(capi, ctx, len(logs), p) for _ in range(n)]
    try:
        for k, scans, odo, act in lockstep(logs, starts):
            yield k, sets, [s.step(scans, odo, act) for s in sets]
    finally:
        for s in sets:
            s.close()


def parts_of(ses, i):
    return [x.copy() for x in ses.global_map(i)[1]]


# ------------------------------------------------------------------------------------------ 1: identity
@pytest.mark.parametrize("rm", [1, 0])
def test_an_uncorrected_set_keeps_every_byte(gpu, rm):
    """Behind a step without a closed submap, at a split step, two steps behind a split and with two closed submaps: the
    snapshot before is the snapshot after, and every later step is that of a twin that never called."""
    capi, ctx = gpu
    logs, p = logs_of(), W.launch_params(sepThre=1.5, removeMoving=bool(rm))
    S = len(logs)
    recs0, called = [], []
    for k, (a, b), (ga, gb) in stepped_pair(capi, ctx, logs, STARTS, p):
        assert all(int(r["status"]) == 0 for r in ga)              # (the identity is claimed for sessions whose steps all had status 0)
        recs0.append(ga[0].copy())
        splits = [j for j, r in enumerate(recs0) if r["split"]]
        for i in range(S):
            assert same_records(ga[i], gb[i]), (k, i)
            assert same_snapshot(snapshot(a, i), snapshot(b, i)), (k, i)
        mark = ("none" if k == 1 else "at_split" if splits == [k] else "after_split" if splits and k == splits[0] + 2
                else "two_closed" if len(splits) >= 2 and k == splits[1] + 1 else None)
        if mark is None:
            continue
        who = [i for i in range(S) if len(a.trajectory(i)[0])]
        assert len(who) == S
        before = [snapshot(a, i) for i in range(S)]
        n_closed = [len(x[4]) - 1 for x in before]
        assert a.remake_closed(who) == {i: capi.NDT_OK for i in who}, mark
        for i in range(S):
            assert same_snapshot(snapshot(a, i), before[i]), (mark, i)
        called.append((mark, n_closed))
    assert [m for m, _ in called] == ["none", "at_split", "after_split", "two_closed"], called
    assert called[0][1] == [0, 0, 0] and called[1][1][0] == 1 and called[3][1][0] == 2, called
    assert k > splits[1] + 2


@pytest.mark.parametrize("rm", [1, 0])
def test_submaps_of_one_scan_and_the_empty_first_submap_keep_every_byte(gpu, rm):
    """sepThre 0: submap 0 closes before it holds a scan, every later one with its one scan, which it hands to nobody.  Called
    behind every step on one of two sets; the first call finds one closed submap without a point and queues nothing."""
    capi, ctx = gpu
    logs, p = logs_of(((33, 5), (34, 4))), W.launch_params(sepThre=0.0, removeMoving=bool(rm))
    for k, (a, b), (ga, gb) in stepped_pair(capi, ctx, logs, [0, 1], p):
        assert all(int(r["status"]) == 0 for r in ga)
        who = [i for i in range(2) if len(a.trajectory(i)[0])]
        before = [snapshot(a, i) for i in range(2)]
        for i in range(2):
            assert same_records(ga[i], gb[i]) and same_snapshot(before[i], snapshot(b, i)), (k, i)
        assert a.remake_closed(who) == {i: capi.NDT_OK for i in who}
        assert a.stats().host_waits == (0 if k == 0 else 2)
        assert all(same_snapshot(snapshot(a, i), before[i]) for i in range(2)), k
        if k == 4:
            sizes = [len(x) for x in before[0][4]]
            # (without removeMoving makeMap leaves out the first two scans of a submap that is not the first: those are empty)
            assert len(sizes) == 6 and sizes[0] == 0 and sizes[1] and (all(sizes[1:]) if rm else not any(sizes[2:])), sizes


# ------------------------------------------------------------------------------------------ 2: the chain
@pytest.mark.parametrize("case", ["at_split", "after_split", "two_closed"])
def test_equal_to_the_chain_then_and_after(gpu, case):
    """Sessions 0 and 2 corrected and remade, the set against the chain at the call and at every later step -- through a
    further split, where the remade cloud is a local map's first part and the next submap closes the ordinary way."""
    capi, ctx = gpu
    logs, p = logs_of(), W.launch_params(sepThre=1.5)
    S = len(logs)
    ses, chain = new_set(capi, ctx, S, p), RemadeChain(capi, ctx, S, p)
    recs0, at = [], None
    for k, scans, odo, act in lockstep(logs, STARTS):
        got, want = ses.step(scans, odo, act), chain.step(scans, odo, act)
        for i in range(S):
            assert same_records(got[i], want[i]), (case, k, i)
            if at is not None:
                same_state(ses, chain, i, (case, k))
        recs0.append(got[0].copy())
        if at is None and due(case, k, recs0):
            at = k
            who = [0, 2]
            assert all(chain.started[i] for i in who)
            new = {i: smooth_adjustment(chain_poses(chain, i)) for i in who}
            assert ses.correct(new) == {i: capi.NDT_OK for i in who}
            assert all(chain.correct(i, new[i]) == capi.NDT_OK for i in who)
            rigid = {i: parts_of(ses, i) for i in who}
            for i in range(S):
                same_state(ses, chain, i, (case, k, "corrected"))
            assert ses.remake_closed(who) == {i: capi.NDT_OK for i in who}
            assert all(chain.remake(i) == capi.NDT_OK for i in who)
            for i in range(S):                                     # (session 1 is not named)
                same_state(ses, chain, i, (case, k, "remade"))
            remade = {i: parts_of(ses, i) for i in who}
            for i in who:
                n_closed = len(rigid[i]) - 1
                # (session 2 is a step behind: at session 0's first split it has closed nothing yet, and keeps every byte)
                assert n_closed >= (0 if (case, i) == ("at_split", 2) else 1) and len(remade[i]) == len(rigid[i])
                assert all(remade[i][m].tobytes() != rigid[i][m].tobytes() for m in range(n_closed)), (case, i)
                assert remade[i][-1].tobytes() == rigid[i][-1].tobytes()          # (the current submap's part keeps its bytes)
                assert ses.trajectory(i)[0].tobytes() == new[i].tobytes()
    assert at is not None and any(r["split"] for r in recs0[at + 1:]), (case, at)
    ses.close()
    chain.close()


# ------------------------------------------------------------------------------------------ 3: a submap out of reach
def test_a_submap_the_adjustment_does_not_reach_keeps_its_bytes(gpu):
    capi, ctx = gpu
    logs, p = logs_of(), W.launch_params(sepThre=1.5)
    ses = new_set(capi, ctx, len(logs), p)
    done = False
    for k, scans, odo, act in lockstep(logs, STARTS):
        ses.step(scans, odo, act)
        old, sub_first, _, _ = ses.trajectory(0)
        if len(sub_first) == 3 and not done:
            done = True
            parts = parts_of(ses, 0)
            start = int(sub_first[1])                               # behind every scan of L_0 = [0, sub_first[1] - 1]
            new = smooth_adjustment(old, start=start)
            assert new[:start].tobytes() == old[:start].tobytes() and new[start:].tobytes() != old[start:].tobytes()
            assert ses.correct({0: new}) == {0: capi.NDT_OK}
            assert ses.remake_closed([0]) == {0: capi.NDT_OK}
            after = parts_of(ses, 0)
            assert len(after) == 3 and len(parts[0]) and len(parts[1])
            assert after[0].tobytes() == parts[0].tobytes()
            assert after[1].tobytes() != parts[1].tobytes()
    assert done
    ses.close()


# ------------------------------------------------------------------------------------------ 4: idempotence, neighbours
def test_a_second_call_and_a_further_named_session_change_nothing(gpu):
    capi, ctx = gpu
    logs, p = logs_of(), W.launch_params(sepThre=1.5)
    S, at = len(logs), 8
    for k, (a, b), _ in stepped_pair(capi, ctx, logs, STARTS, p):
        if k < at:
            continue
        new = {i: smooth_adjustment(a.trajectory(i)[0]) for i in (0, 2)}
        for s in (a, b):
            assert s.correct(new) == {0: capi.NDT_OK, 2: capi.NDT_OK}
        corrected = [snapshot(a, i) for i in range(S)]
        assert a.remake_closed([0, 2]) == {0: capi.NDT_OK, 2: capi.NDT_OK}
        once = [snapshot(a, i) for i in range(S)]
        assert len(once[0][4]) == 3 and not same_snapshot(once[0], corrected[0]) and same_snapshot(once[1], corrected[1])
        assert a.remake_closed([0, 2]) == {0: capi.NDT_OK, 2: capi.NDT_OK}
        assert all(same_snapshot(snapshot(a, i), once[i]) for i in range(S))
        ctx.set_option(capi.OPT_WORKGROUPS, 3)                      # (nor does the result depend on NDT_OPT_WORKGROUPS)
        try:
            assert b.remake_closed([2, 1, 0]) == {2: capi.NDT_OK, 1: capi.NDT_OK, 0: capi.NDT_OK}
        finally:
            ctx.set_option(capi.OPT_WORKGROUPS, 0)
        assert all(same_snapshot(snapshot(b, i), once[i]) for i in range(S))
        break


# ------------------------------------------------------------------------------------------ 5: the span error
def test_span_error_costs_its_session_alone(gpu):
    """Scan 0 of session 0 sent to tx = 1e8 with two submaps closed: the correction itself is NDT_OK (scan 0 is no anchor and
    not in the current store), the remake of L_0 spans more than 2^30 voxels -- session 0 gets NDT_E_ARG and keeps every byte,
    session 2 is remade and equals the chain."""
    capi, ctx = gpu
    logs, p = logs_of(), W.launch_params(sepThre=1.5)
    S = len(logs)
    ses, chain = new_set(capi, ctx, S, p), RemadeChain(capi, ctx, S, p)
    recs0, done = [], False
    for k, scans, odo, act in lockstep(logs, STARTS):
        got, want = ses.step(scans, odo, act), chain.step(scans, odo, act)
        recs0.append(got[0].copy())
        if not due("two_closed", k, recs0):
            continue
        done = True
        old, sub_first, sub_anchor, store_first = ses.trajectory(0)
        assert len(sub_first) == 3 and 0 not in sub_anchor.tolist() and store_first > 0          # (host data: checked before the call)
        bad = old.copy()
        bad[0, 0] = 1e8
        new2 = smooth_adjustment(chain_poses(chain, 2))
        assert ses.correct({0: bad, 2: new2}) == {0: capi.NDT_OK, 2: capi.NDT_OK}
        assert chain.correct(2, new2) == capi.NDT_OK
        before = [snapshot(ses, i) for i in range(S)]
        assert ses.remake_closed([0, 2]) == {0: capi.NDT_E_ARG, 2: capi.NDT_OK}                   # (the call returns NDT_OK)
        assert chain.remake(2) == capi.NDT_OK
        assert same_snapshot(snapshot(ses, 0), before[0]) and same_snapshot(snapshot(ses, 1), before[1])
        assert not same_snapshot(snapshot(ses, 2), before[2])
        same_state(ses, chain, 2, "span")
        break
    assert done
    ses.close()
    chain.close()


# ------------------------------------------------------------------------------------------ 6: refusals
def test_refusals_name_their_entry_and_change_nothing(gpu):
    import torch
    capi, ctx = gpu
    L, E = capi.lib(), capi.NDT_E_ARG
    err = lambda: L.ndt_last_error(ctx.h).decode()          # noqa: E731
    logs, p = logs_of(((33, 5), (34, 5), (35, 1))), W.launch_params(sepThre=1.5)
    ses, bare = new_set(capi, ctx, 3, p), new_set(capi, ctx, 3, p, archive=False)
    for k, scans, odo, act in lockstep(logs, [0, 0, 9]):
        if k < 5:
            for s in (ses, bare):
                s.step(scans, odo, act)
    assert [len(ses.trajectory(i)[0]) for i in range(3)] == [5, 5, 0] and len(ses.global_map(0)[1]) == 2
    before = [snapshot(s, i) for s in (ses, bare) for i in range(3)]
    status = np.full(4, 77, np.int32)

    def call(which, h=ses.h, n=None):
        w = np.array(which or [0], np.int32)
        return L.ndt_sessions_remake_closed(h, w.ctypes.data, len(which) if n is None else n, status.ctypes.data)

    assert call([0], h=None) == E and "null session set" in L.ndt_last_error(None).decode()
    assert L.ndt_sessions_remake_closed(ses.h, None, 1, status.ctypes.data) == E and "NULL" in err()
    assert L.ndt_sessions_remake_closed(ses.h, np.zeros(1, np.int32).ctypes.data, 1, None) == E and "NULL" in err()
    assert call([]) == E and "n_named < 1" in err()
    assert call([0], n=-2) == E and "n_named < 1" in err()
    assert call([0, 3]) == E and "entry 1" in err() and "session 3" in err() and "out of range" in err()
    assert call([-1]) == E and "entry 0" in err() and "session -1" in err()
    assert call([1, 2]) == E and "entry 1" in err() and "session 2" in err() and "not started" in err()
    assert call([0, 1, 0]) == E and "entry 2" in err() and "session 0" in err() and "again" in err()
    assert call([0], h=bare.h) == E and "no scan archive" in err()
    with pytest.raises(capi.NdtError, match="no scan archive"):
        bare.remake_closed([0])
    with pytest.raises(capi.NdtError, match="n_named < 1"):
        ses.remake_closed([])
    cloud = torch.rand((500, 2), dtype=torch.float32, device="cuda") * 10
    torch.cuda.synchronize()
    m = capi.Map(ctx, cloud.cpu().numpy(), capi.default_params(resolution=1.0))
    m.rebuild_begin(cloud.data_ptr(), 500)
    assert call([0]) == E and "ndt_map_rebuild_begin" in err()
    m.rebuild_end()
    m.close()
    assert status.tolist() == [77] * 4
    after = [snapshot(s, i) for s in (ses, bare) for i in range(3)]
    assert all(same_snapshot(x, y) for x, y in zip(after, before))
    assert ses.remake_closed([1, 0]) == {1: capi.NDT_OK, 0: capi.NDT_OK}          # the set is as it was: a valid call goes through
    ses.close()
    bare.close()


# ------------------------------------------------------------------------------------------ 7: waits
def test_waits_do_not_depend_on_the_sessions_named(gpu):
    """Two host waits for one session named and for three; sessions_stepped = the sessions named, triples_run = the triples of
    their closed submaps' scan lists; no wait at all while no named session has a closed submap (the header says so)."""
    capi, ctx = gpu
    logs, p = logs_of(), W.launch_params(sepThre=1.5)
    S = len(logs)
    ses = new_set(capi, ctx, S, p)
    from ndt_slam_amd import replay
    for k, scans, odo, act in lockstep(logs, STARTS):
        ses.step(scans, odo, act)
        if k == 1:
            assert ses.remake_closed([0, 1, 2]) == {0: 0, 1: 0, 2: 0}
            none = ses.stats()
            assert (none.host_waits, none.sessions_stepped, none.triples_run, none.h2d_bytes, none.d2h_bytes) == (0, 3, 0, 0, 0)
        if k == 6:                                  # (sessions 0 and 1 have closed two submaps, session 2 -- a step behind -- one)
            break
    triples = []
    for i in range(S):
        sub_first = ses.trajectory(i)[1]
        ranges = replay.closed_scan_ranges(sub_first, len(sub_first) - 1)
        triples.append(sum(max(last - first + 1 - 2, 0) for first, last in ranges))
    assert len(set(triples)) >= 2 and min(triples) >= 1, triples
    ses.remake_closed([1])
    one = ses.stats()
    assert (one.host_waits, one.sessions_stepped, one.triples_run) == (2, 1, triples[1])
    ses.remake_closed([2, 0, 1])
    three = ses.stats()
    assert (three.host_waits, three.sessions_stepped, three.triples_run) == (2, S, sum(triples))
    assert three.h2d_bytes > one.h2d_bytes > 0 and three.d2h_bytes > one.d2h_bytes > 0
    ses.close()


# ------------------------------------------------------------------------------------------ 8: replay
def test_replay_remakes_behind_a_correction_when_asked(gpu):
    """The lap of tests/test_gpu_occ_rebuild.py (odometry only, the loop closes near its end) through run_sessions_resident with
    LoopClosure(remake_closed=True): the global map's parts are those of the manual sequence find_loops, optimise, correct,
    remake_closed; with the flag off they are those of the sequence without the last call."""
    from ndt_slam_amd import replay
    from ndt_slam_amd.pose_estimator import Pose2D, Scan2D
    capi, ctx = gpu
    (scans, odo), _, p = loop_workload(n_frames=FULL_LAP + 1, score_thre=-1.0)
    log = [Scan2D(scans[k], k, Pose2D(*odo[k])) for k in range(len(scans))]
    lp = capi.default_loop_params()
    info = np.array(lp.info[:]) / 100.0
    cooldown = 10

    def manual(remake):
        ses, quiet, n_corr = new_set(capi, ctx, 1, p), 0, 0
        for k in range(len(scans)):
            rec = ses.step([scans[k]], [odo[k]])
            assert rec[0]["stepped"]
            if k + 1 < quiet:
                continue
            found = [l for l in ses.find_loops(lp, np.array([1], np.uint8)) if l["status"] == 0 and l["found"]]
            if not found:
                continue
            traj = ses.trajectory(0)[0]
            new, res = capi.optimize_pose_graphs(ctx, traj, [0, len(traj)], replay.loop_graph(traj, found[0]["edge"], info), [0, len(traj)], None)
            if res[0]["status"] != 0 or not res[0]["converged"]:
                continue
            assert ses.correct({0: new}) == {0: capi.NDT_OK}
            if remake:
                assert ses.remake_closed([0]) == {0: capi.NDT_OK}
            quiet, n_corr = k + 1 + cooldown, n_corr + 1
        out = parts_of(ses, 0), ses.trajectory(0)[0]
        ses.close()
        return out + (n_corr,)

    def replayed(**flag):
        calls = []

        class Counting(capi.Sessions):
            def remake_closed(self, which):
                calls.append(list(which))
                return super().remake_closed(which)

        ses = Counting(ctx, 1, capi.session_params_from_launch(p), archive=True)
        lc = replay.LoopClosure(loop=lp, pg=None, odo_info=info, every=1, cooldown=cooldown, **flag)
        poses = replay.run_sessions_resident(ctx, [log], sessions=ses, loop_closure=lc, **p)
        traj = ses.trajectory(0)[0]
        assert np.array([(q.tx, q.ty, q.th) for q in poses[0]]).tobytes() == traj.tobytes()
        out = parts_of(ses, 0), traj
        ses.close()
        return out + (calls,)

    want_on, traj_on, n_on = manual(True)
    want_off, traj_off, n_off = manual(False)
    got_on, gtraj_on, calls_on = replayed(remake_closed=True)
    got_off, gtraj_off, calls_off = replayed()
    assert n_on >= 1 and calls_on == [[0]] * n_on and calls_off == []
    for got, want in ((got_on, want_on), (got_off, want_off)):
        assert len(got) == len(want) >= 3 and all(x.tobytes() == y.tobytes() for x, y in zip(got, want))
    assert gtraj_on.tobytes() == traj_on.tobytes() and gtraj_off.tobytes() == traj_off.tobytes()
    assert any(x.tobytes() != y.tobytes() for x, y in zip(got_on, got_off))          # (the flag is not a no-op on this lap)
