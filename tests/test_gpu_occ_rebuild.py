"""The scan archive of a session set and ndt_sessions_occ_rebuild on the device (include/ndt_mi355x.h): the
grid a rebuild writes is what ndt_scan_to_map_batch_dev + the integrate rules give for the archived scans at the trajectory's
poses -- against the grids integrated step by step, against the numpy restatement fed with the single device call's float32
points (tests/occ_rebuild_helpers.py), before and after corrections, across run and scan boundaries, whoever else is named,
whatever NDT_OPT_WORKGROUPS is; a set with the archive is byte for byte its twin without.  Every comparison is integer or
byte equality."""
import ctypes

import numpy as np
import pytest

import occ_helpers as H
import occ_rebuild_helpers as R
from loops_helpers import FULL_LAP, loop_workload
from session_correct_helpers import smooth_adjustment
from session_helpers import lockstep, same_records, session_logs
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

GEOMS = [H.Geometry(-25.0, -25.0, 0.1, 500, 500), H.Geometry(-20.05, -20.05, 0.05, 800, 800),
         H.Geometry(-25.0, -25.0, 0.25, 200, 200), H.Geometry(-3.0, -3.0, 0.1, 60, 60)]      # (the last: most beams leave it)


def launch_params(**kw):
    from ndt_slam_amd import replay
    return dict(replay.LAUNCH_PARAMS, **kw)


def new_set(gpu, S, p, archive=True):
    capi, ctx = gpu
    return capi.Sessions(ctx, S, capi.session_params_from_launch(p), archive=archive)


def check_rebuilt(gpu, ses, i, grid, geom, max_range2=H.DBL_MAX, tag=""):
    """Session i's grid against the restatement over its archive and its trajectory as they are now -> the stats dict."""
    _, ctx = gpu
    want, st = R.restate(ctx, geom, ses.archive_scans(i), ses.trajectory(i)[0], max_range2)
    hit, pas = grid.counts()
    assert np.array_equal(hit, want[0]) and np.array_equal(pas, want[1]), (tag, i, int((hit != want[0]).sum()), int((pas != want[1]).sum()))
    return st


# ------------------------------------------------------------------------------------------ 1: rebuild equals incremental
def test_rebuild_equals_the_grids_integrated_step_by_step(gpu):
    capi, ctx = gpu
    p = launch_params(sepThre=2.5)
    logs = session_logs(((33, 9), (34, 6), (35, 8), (36, 5)))
    starts, S = [0, 0, 2, 0], 4                                                    # session 2 starts late, 1 and 3 end early
    ses, twin = new_set(gpu, S, p), new_set(gpu, S, p, archive=False)
    A, B = [capi.OccGrid(ctx, g) for g in GEOMS], [capi.OccGrid(ctx, g) for g in GEOMS]
    total = np.zeros(4, np.uint64)
    raws = [[] for _ in range(S)]
    for k, scans, odo, act in lockstep(logs, starts):
        recs, recs2 = ses.step(scans, odo, act), twin.step(scans, odo, act)
        total += np.array(H.stats_tuple(ses.occ_integrate(A, np.ascontiguousarray(recs["stepped"], np.uint8))), np.uint64)
        a, b = R.stats_fields(ses.stats()), R.stats_fields(twin.stats())
        assert a.pop("h2d_bytes") - b.pop("h2d_bytes") == R.table_b_moves_bytes(S) and a == b and a["host_waits"] == 3, (k, a, b)
        for i in range(S):
            assert same_records(recs[i], recs2[i]), (k, i)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(R.views(ses, i), R.views(twin, i))), (k, i)
            if recs[i]["stepped"]:
                raws[i].append(scans[i])
    st = ses.occ_rebuild(B)
    assert H.stats_tuple(st) == tuple(int(v) for v in total)
    for i in range(S):
        ha, pa = A[i].counts()
        hb, pb = B[i].counts()
        assert np.array_equal(ha, hb) and np.array_equal(pa, pb) and pb.sum() > 100, i
        n_scans, n_points = ses.archive_info(i)
        arch = ses.archive_scans(i)
        assert n_scans == len(ses.trajectory(i)[0]) == len(raws[i]) == len(arch) and n_points == sum(len(x) for x in arch)
        for k, raw in enumerate(raws[i]):
            assert arch[k].tobytes() == ctx.resample(raw, p["space"], p["space_thre"]).tobytes(), (i, k)
        ptr, n = ses.archive_view(i)
        assert n == n_points and ptr
    assert [len(x) for x in raws] == [9, 6, 8, 5]
    for x in A + B:
        x.close()
    ses.close(); twin.close()


# ------------------------------------------------------------------------------------------ 2: after a correction
def test_rebuild_follows_a_correction_and_the_steps_behind_it(gpu):
    capi, ctx = gpu
    p = launch_params(sepThre=2.5)
    logs, S = session_logs(((33, 8), (34, 8), (35, 8))), 3
    ses = new_set(gpu, S, p)
    inc, grids = [capi.OccGrid(ctx, g) for g in GEOMS[:S]], [capi.OccGrid(ctx, g) for g in GEOMS[:S]]
    steps = list(lockstep(logs))
    for k, scans, odo, act in steps[:6]:
        recs = ses.step(scans, odo, act)
        ses.occ_integrate(inc, np.ascontiguousarray(recs["stepped"], np.uint8))
    before = [ses.archive_scans(i) for i in range(S)]
    new = {i: smooth_adjustment(ses.trajectory(i)[0], scale=1.0 + i, start=1) for i in (0, 2)}
    assert ses.correct(new) == {0: capi.NDT_OK, 2: capi.NDT_OK}
    for i in range(S):                                                             # robot-frame points do not move
        assert all(x.tobytes() == y.tobytes() for x, y in zip(before[i], ses.archive_scans(i))), i
    st = ses.occ_rebuild(grids)
    sums = dict.fromkeys(H.STATS, 0)
    for i in range(S):
        if i in new:
            assert ses.trajectory(i)[0].tobytes() == new[i].tobytes()
        sums = H.add_stats(sums, check_rebuilt(gpu, ses, i, grids[i], GEOMS[i], tag="corrected"))
    assert H.stats_tuple(st) == H.stats_tuple(sums)
    assert R.grid_bytes(grids[1]) == R.grid_bytes(inc[1])                          # the uncorrected session: its incremental grid
    assert R.grid_bytes(grids[0]) != R.grid_bytes(inc[0]) and R.grid_bytes(grids[2]) != R.grid_bytes(inc[2])
    for k, scans, odo, act in steps[6:]:
        ses.step(scans, odo, act)
    ses.occ_rebuild(grids)
    for i in range(S):
        assert ses.archive_info(i)[0] == 8
        check_rebuilt(gpu, ses, i, grids[i], GEOMS[i], tag="two steps later")
    for x in inc + grids:
        x.close()
    ses.close()


# ------------------------------------------------------------------------------------------ 3: run and scan boundaries
def test_runs_of_256_beams_and_scan_boundaries(gpu):
    capi, ctx = gpu
    p = launch_params(score_thre=-1.0)                                             # (odometry only: no match of these scans is fused)
    sizes = [1, 255, 256, 0, 257, 513]
    ses = new_set(gpu, 1, p)
    for k, n in enumerate(sizes):
        raw = R.alternating_scan(n, 0.3 * k) if n else np.zeros((0, 2))
        rec = ses.step([raw], [[0.05 * k, -0.03 * k, 7.0 * k]])
        assert rec[0]["stepped"] == 1, (k, rec[0])
    arch = ses.archive_scans(0)
    assert np.abs(ses.trajectory(0)[0][:, :2]).max() < 1.0, ses.trajectory(0)[0]
    assert [len(x) for x in arch] == sizes and ses.archive_info(0) == (len(sizes), sum(sizes))
    for k, n in enumerate(sizes):
        assert arch[k].tobytes() == (R.alternating_scan(n, 0.3 * k) if n else np.zeros((0, 2))).tobytes(), k
    assert [len(x) for x in ses.archive_scans(0, 2, 3)] == sizes[2:5] and ses.archive_scans(0, len(sizes), 0) == []
    geom = H.Geometry(-2.55, -2.45, 0.1, 50, 50)                                   # the 3 m beams leave it but for the diagonals
    grid = capi.OccGrid(ctx, geom)
    for r2 in (H.DBL_MAX, 3.5 * 3.5):                                              # ... and 3.5 m cuts the 4 m beams
        st = ses.occ_rebuild([grid], max_range2=r2)
        wst = check_rebuilt(gpu, ses, 0, grid, geom, r2, tag=r2)
        assert H.stats_tuple(st) == H.stats_tuple(wst) and st["n_beams"] == sum(sizes), (st, wst)
        assert st["n_hit"] > 0 and st["n_pass"] > 1000
        if r2 != H.DBL_MAX:
            assert st["n_skipped"] == sum(n // 2 for n in sizes)                   # every second point lies at 4 m
        else:
            assert st["n_skipped"] == 0 and st["n_hit"] < sum(sizes)
    grid.close(); ses.close()


# ------------------------------------------------------------------------------------------ 4: independence
def test_a_grid_depends_on_its_own_session_alone(gpu):
    capi, ctx = gpu
    p = launch_params(sepThre=2.5)
    logs, S = session_logs(((33, 6), (34, 6), (35, 6))), 3
    ses, twin = new_set(gpu, S + 1, p), new_set(gpu, S + 1, p)                     # (session 3 never starts)
    pad = lambda scans, odo, act: (scans + [np.zeros((0, 2))], np.vstack([odo, np.zeros((1, 3))]), np.append(act, 0).astype(np.uint8))      # noqa: E731
    steps = [pad(*x[1:]) for x in lockstep(logs)]
    for scans, odo, act in steps[:5]:
        ses.step(scans, odo, act); twin.step(scans, odo, act)
    grids = [capi.OccGrid(ctx, g) for g in GEOMS[:S]] + [None]
    ses.occ_rebuild(grids)                                                         # all named: the unstarted one needs no grid
    want = [R.grid_bytes(g) for g in grids[:S]]
    for i in range(S):
        check_rebuilt(gpu, ses, i, grids[i], GEOMS[i], tag="all")
    for which in ([1, 0, 0, 0], [0, 1, 0, 1], [1, 0, 1, 0], [0, 0, 0, 1]):
        only = [g if w else None for g, w in zip(grids, which)]                    # (a session not taken needs none either)
        ses.occ_rebuild(only, np.array(which, np.uint8))
        assert [R.grid_bytes(g) for g in grids[:S]] == want, which
    for wg in (1, 3):
        ctx.set_option(capi.OPT_WORKGROUPS, wg)
        try:
            st = ses.occ_rebuild(grids)
        finally:
            ctx.set_option(capi.OPT_WORKGROUPS, 0)
        assert [R.grid_bytes(g) for g in grids[:S]] == want, wg
    once = [g.counts() for g in grids[:S]]
    st2 = [ses.occ_rebuild(grids, clear=c) for c in (True, False)]
    assert H.stats_tuple(st2[0]) == H.stats_tuple(st2[1]) == H.stats_tuple(st)
    for i in range(S):
        hit, pas = grids[i].counts()
        assert np.array_equal(hit, 2 * once[i][0]) and np.array_equal(pas, 2 * once[i][1]), i
    # the set is what it was: its views and its next step are those of the twin that never rebuilt
    for i in range(S):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(R.views(ses, i), R.views(twin, i))), i
    scans, odo, act = steps[5]
    a, b = ses.step(scans, odo, act), twin.step(scans, odo, act)
    assert all(same_records(x, y) for x, y in zip(a, b)) and bytes(ses.stats()) == bytes(twin.stats())
    for i in range(S):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(R.views(ses, i), R.views(twin, i))), i
    for g in grids[:S]:
        g.close()
    ses.close(); twin.close()


# ------------------------------------------------------------------------------------------ 5: growth
def test_the_archive_grows_and_keeps_what_it_held(gpu):
    capi, ctx = gpu
    p = launch_params(sepThre=2.5)
    (log,) = session_logs(((37, 10),))
    ses = new_set(gpu, 1, p)
    first = None
    for k, scans, odo, act in lockstep([log]):
        ses.step(scans, odo, act)
        if first is None:
            first = ses.archive_scans(0, 0, 1)[0].copy()
    arch = ses.archive_scans(0)
    assert R.growths([len(x) for x in arch]) >= 2, [len(x) for x in arch]
    assert arch[0].tobytes() == first.tobytes() == ctx.resample(log[0][0], p["space"], p["space_thre"]).tobytes() and len(first) > 16
    grid = capi.OccGrid(ctx, GEOMS[0])
    ses.occ_rebuild([grid])
    check_rebuilt(gpu, ses, 0, grid, GEOMS[0], tag="grown")
    grid.close(); ses.close()


# ------------------------------------------------------------------------------------------ 6: refusals
def test_refusals_leave_everything_as_it_was(gpu):
    import torch
    capi, ctx = gpu
    L = capi.lib()
    p = launch_params(sepThre=2.5)
    (log,) = session_logs(((33, 3),))
    ses, bare = new_set(gpu, 2, p), new_set(gpu, 2, p, archive=False)              # (session 1 never starts)
    for k, scans, odo, act in lockstep([log]):
        for s in (ses, bare):
            s.step(scans + [np.zeros((0, 2))], np.vstack([odo, np.zeros((1, 3))]), np.array([1, 0], np.uint8))
    g = GEOMS[3]
    grid, grid2, other_ctx = capi.OccGrid(ctx, g), capi.OccGrid(ctx, g), capi.Context(0)
    foreign = capi.OccGrid(other_ctx, g)
    ses.occ_rebuild([grid, None])
    before = R.grid_bytes(grid)
    st = np.full(4, 0x5A5A5A5A, np.uint64)
    hs = lambda *gs: (ctypes.c_void_p * len(gs))(*[x.h if x is not None else None for x in gs])      # noqa: E731

    def refuse(text, s=ses, occs=None, which=None, r2=H.DBL_MAX, code=-1):
        rc = L.ndt_sessions_occ_rebuild(s.h if s is not None else None, hs(grid, grid2) if occs is None else occs,
                                        None if which is None else which.ctypes.data, 1, r2, st.ctypes.data)
        msg = L.ndt_last_error(ctx.h if s is not None else None).decode()
        assert rc == code and text in msg, (text, rc, msg)

    refuse("null session set", s=None)
    refuse("NULL occs", occs=ctypes.c_void_p())
    refuse("no scan archive", s=bare)
    refuse("session 0: NULL grid", occs=hs(None, grid2))
    refuse("session 0: the grid belongs to another context", occs=hs(foreign, None))
    refuse("max_range2", r2=float("nan")); refuse("max_range2", r2=-1.0)
    assert L.ndt_sessions_archive_enable(ses.h) == 0                               # idempotent ...
    assert L.ndt_sessions_archive_enable(bare.h) == -1 and "session 0 has already started" in L.ndt_last_error(ctx.h).decode()
    assert L.ndt_sessions_archive_enable(None) == -1 and L.ndt_last_error(None).decode() == "null session set"
    # a repeated grid needs two taken sessions
    both = new_set(gpu, 2, p)
    for k, scans, odo, act in lockstep([log, log]):
        both.step(scans, odo, act)
    refuse("session 1: its grid is given twice", s=both, occs=hs(grid, grid))
    # the read-outs
    n, m = ctypes.c_size_t(77), ctypes.c_size_t(77)
    xy, off = np.full((4, 2), 5.5), np.full(8, 99, np.uint64)

    def refuse_read(text, rc):
        msg = L.ndt_last_error(ctx.h).decode()
        assert rc == -1 and text in msg, (text, rc, msg)
    refuse_read("no scan archive", L.ndt_sessions_archive_info(bare.h, 0, ctypes.byref(n), ctypes.byref(m)))
    refuse_read("no scan archive", L.ndt_sessions_archive_scans(bare.h, 0, 0, 1, None, 0, off.ctypes.data, ctypes.byref(n)))
    p_dev = ctypes.c_void_p(1234)
    refuse_read("no scan archive", L.ndt_sessions_archive_view(bare.h, 0, ctypes.byref(p_dev), ctypes.byref(n)))
    refuse_read("session 2 out of range", L.ndt_sessions_archive_info(ses.h, 2, ctypes.byref(n), ctypes.byref(m)))
    refuse_read("session -1 out of range", L.ndt_sessions_archive_view(ses.h, -1, ctypes.byref(p_dev), ctypes.byref(n)))
    refuse_read("outside the archive's 3", L.ndt_sessions_archive_scans(ses.h, 0, 2, 2, None, 0, off.ctypes.data, ctypes.byref(n)))
    refuse_read("outside the archive's 3", L.ndt_sessions_archive_scans(ses.h, 0, 4, 0, None, 0, off.ctypes.data, ctypes.byref(n)))
    refuse_read("outside the archive's 0", L.ndt_sessions_archive_scans(ses.h, 1, 0, 1, None, 0, off.ctypes.data, ctypes.byref(n)))
    refuse_read("capacity below", L.ndt_sessions_archive_scans(ses.h, 0, 0, 3, xy.ctypes.data, 4, off.ctypes.data, ctypes.byref(n)))
    assert (n.value, m.value, p_dev.value) == (77, 77, 1234) and (xy == 5.5).all() and (off == 99).all()
    with pytest.raises(capi.NdtError, match="no scan archive"):
        bare.archive_scans(0)
    # an open ndt_map_rebuild_begin on the context refuses as it does everywhere
    cloud = torch.rand((500, 2), dtype=torch.float32, device="cuda") * 10
    torch.cuda.synchronize()
    mp = capi.Map(ctx, cloud.cpu().numpy(), capi.default_params(resolution=1.0))
    mp.rebuild_begin(cloud.data_ptr(), 500)
    refuse("ndt_map_rebuild_begin")
    mp.rebuild_end()
    mp.close()
    assert (st == 0x5A5A5A5A).all() and R.grid_bytes(grid) == before and not np.frombuffer(R.grid_bytes(grid2), np.uint32).any()
    assert ses.archive_info(0)[0] == 3 and ses.archive_info(1) == (0, 0)
    foreign.close(); other_ctx.close(); grid.close(); grid2.close()
    ses.close(); bare.close(); both.close()


# ------------------------------------------------------------------------------------------ 7: the lap
def test_the_lap_closes_and_the_written_grid_is_the_rebuilt_one(gpu, tmp_path):
    """Odometry only (score_thre -1) around the 5 m circle: the loop closes near the end of the lap (behind scan 53), the session is corrected
    and its grid rebuilt.  Cells whose rendered value differs from a grid cast at the true poses, of 38 998 known ones, as
    measured on an MI355X (LOG.md R35.1): 3347 for the stale grid (integrated step by step, never rebuilt), 1821 for the
    rebuilt one.  Both are printed; nothing is asserted about the two counts."""
    from ndt_slam_amd import replay
    from ndt_slam_amd.pose_estimator import Pose2D, Scan2D
    capi, ctx = gpu
    (scans, odo), truth, p = loop_workload(n_frames=FULL_LAP + 1, score_thre=-1.0)
    log = [Scan2D(scans[k], k, Pose2D(*odo[k])) for k in range(len(scans))]
    geom = capi.OccGeometry(-25.0, -25.0, 0.1, 500, 500)
    hg = H.Geometry(-25.0, -25.0, 0.1, 500, 500)
    lp = capi.default_loop_params()
    lc = replay.LoopClosure(loop=lp, pg=None, odo_info=np.array(lp.info[:]) / 100.0, every=1, cooldown=10)
    corrections = []

    class Counting(capi.Sessions):
        def correct(self, new_poses):
            out = super().correct(new_poses)
            corrections.append((self.archive_info(0)[0], dict(out)))
            return out

    ses = Counting(ctx, 1, capi.session_params_from_launch(p), archive=True)
    stem = str(tmp_path / "lap")
    poses = replay.run_sessions_resident(ctx, [log], sessions=ses, occupancy=geom, occupancy_names=[stem], loop_closure=lc, **p)
    final = ses.trajectory(0)[0]
    print("corrections (scans in the trajectory, status):", corrections)
    assert len(corrections) >= 1 and all(v == capi.NDT_OK for _, d in corrections for v in d.values()), corrections
    assert np.array([(q.tx, q.ty, q.th) for q in poses[0]]).tobytes() == final.tobytes() and len(final) == FULL_LAP + 1
    arch = ses.archive_scans(0)
    assert all(a.tobytes() == replay.resample_points(s, p["space"], p["space_thre"]).tobytes() for a, s in zip(arch, scans))
    # (the steps behind the last correction were integrated on top of the rebuilt grid, at the poses the trajectory keeps)
    want, _ = R.restate_numpy(hg, arch, final)
    rebuilt = H.render(want[0], want[1], 1)
    replay.save_occupancy(stem + "_expect", rebuilt, hg)
    assert open(stem + ".pgm", "rb").read() == open(stem + "_expect.pgm", "rb").read()
    assert set(np.unique(replay.load_occupancy(stem)[0])) == {0, 205, 254}
    again = capi.OccGrid(ctx, hg)                                                  # ... and to the last counter on the device
    ses.occ_rebuild([again])
    check_rebuilt(gpu, ses, 0, again, hg, tag="lap")
    assert np.array_equal(again.render(1), rebuilt)
    again.close()
    # the measurement: against a grid cast at the true poses
    ideal = H.render(*R.restate_numpy(hg, arch, truth)[0], 1)
    stale_set = capi.Sessions(ctx, 1, capi.session_params_from_launch(p))
    stale_grid = capi.OccGrid(ctx, hg)
    for k in range(len(scans)):
        rec = stale_set.step([scans[k]], [odo[k]])
        stale_set.occ_integrate([stale_grid], np.ascontiguousarray(rec["stepped"], np.uint8))
    stale = stale_grid.render(1)
    print("cells whose rendered value differs from the grid cast at the true poses: stale %d, rebuilt %d (of %d known cells)"
          % (int((stale != ideal).sum()), int((rebuilt != ideal).sum()), int((ideal >= 0).sum())))
    stale_grid.close(); stale_set.close(); ses.close()
