"""Relocalisation on the device: the score sweep (ndt_score_*), the candidate pick (ndt_lattice_select_dev) and
ndt_relocalize, against the CPU oracle, the device's own ndt_eval_at and the numpy references of tests/reloc_helpers.py."""
import ctypes
import math

import numpy as np
import pytest

from reloc_helpers import (LAT, capi_lattice, crafted_volumes, edge_poses, eval_poses, lattice_poses, lattice_size, oracle_scores,
                           pose_error, ref_best, ref_select)
from gpu_support import gpu, sync, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

SMALL = dict(x0=-3.0, y0=4.0, yaw0=-0.4, step_x=0.6, step_y=0.45, step_yaw=0.2, nx=7, ny=5, nyaw=3)


@pytest.fixture(scope="module")
def maps(gpu, c1_world):
    capi, ctx = gpu
    m, sf, cfg = c1_world
    return capi.Map(ctx, m, capi.default_params(resolution=cfg["resolution"])), sf, cfg


def score_dev(gm, scan, poses=None, lattice=None, stride=8, stream=None, ctx=None, want_pairs=True):
    """One ndt_score_poses_dev / ndt_score_lattice_dev launch from torch buffers -> (score, pairs), read back."""
    import torch
    dev = torch.device("cuda", 0)
    scan = np.ascontiguousarray(scan, np.float32).reshape(-1, 2)
    n = len(scan)
    if stride != 8:
        wide = np.full((n, stride // 4), np.float32(7.5)); wide[:, :2] = scan
        scan = wide
    d_sc = to_dev(scan)
    P = len(poses) if poses is not None else lattice.size
    d_po = to_dev(np.ascontiguousarray(poses, np.float64).reshape(-1, 3)) if poses is not None else None
    d_s = torch.full((P,), -1.0, dtype=torch.float64, device=dev)
    d_p = torch.full((P,), -1, dtype=torch.int32, device=dev)
    sync()
    pp = d_p.data_ptr() if want_pairs else None
    if poses is not None:
        gm.score_poses_dev(d_sc.data_ptr(), n, d_po.data_ptr(), P, d_s.data_ptr(), pp, stride=stride, stream=stream, ctx=ctx)
    else:
        gm.score_lattice(d_sc.data_ptr(), n, lattice, d_s.data_ptr(), pp, stride=stride, stream=stream, ctx=ctx)
    sync()
    return d_s.cpu().numpy(), d_p.cpu().numpy().view(np.uint32)


def assert_matches_eval_at(gm, scan, poses, score, pairs):
    """Same pairs; the same non-negative terms in another order: |delta score| <= pairs * 2^-52 * |score|."""
    for q, p in enumerate(poses):
        if not np.isfinite(p).all():
            continue
        s0, _, _, pr0 = gm.eval_at(scan, p)
        assert pairs[q] == pr0, (q, p)
        assert abs(score[q] - s0) <= pr0 * 2.0 ** -52 * abs(s0), (q, p, score[q], s0)


# ------------------------------------------------------------------------------------------ 1, 3: against the oracle
@pytest.mark.parametrize("kw", [dict(), dict(preset="pcl18"), dict(radius_inclusive=1), dict(preset="pcl_new")],
                         ids=["default", "pcl18", "radius_inclusive", "pcl_new"])
def test_scores_match_the_oracle(gpu, oracle, c1_world, kw):
    capi, ctx = gpu
    m, sf, cfg = c1_world
    gm = capi.Map(ctx, m, capi.default_params(resolution=cfg["resolution"], **kw))
    om = oracle.Map(m, oracle.default_params(resolution=cfg["resolution"], **kw))
    for k in range(4):
        scan, _, poses = eval_poses(sf, k)
        s, p = gm.score_poses(scan, poses)
        s0, p0 = oracle_scores(oracle, om, scan, poses)
        assert np.array_equal(p, p0)                                     # same neighbour sets at every pose
        assert s == pytest.approx(s0, rel=1e-12, abs=1e-300)
        assert p[4] == 0 and s[4] == 0.0 and (s[p == 0] == 0.0).all()    # off the map: nothing
        assert (p > 0).sum() > 50
    gm.close()


# ------------------------------------------------------------------------------------------ 2: against ndt_eval_at
def test_scores_match_the_device_eval_at(gpu, maps):
    capi, ctx = gpu
    gm, sf, _ = maps
    for k in range(4):
        scan, _, poses = eval_poses(sf, k, n_random=60)
        s, p = gm.score_poses(scan, poses)
        assert_matches_eval_at(gm, scan, poses, s, p)


# ------------------------------------------------------------------------------------------ 4: determinism
def test_scores_do_not_depend_on_order_count_workgroups_form_or_stride(gpu, maps):
    capi, ctx = gpu
    gm, sf, _ = maps
    scan, truth, poses = eval_poses(sf, 1, n_random=995)                   # 1000 poses
    rng = np.random.default_rng(5)
    s_all, p_all = score_dev(gm, scan, poses)
    assert (p_all > 0).sum() > 100
    host_s, host_p = gm.score_poses(scan, poses)                           # host form = device form
    assert host_s.tobytes() == s_all.tobytes() and host_p.tobytes() == p_all.tobytes()
    perm = rng.permutation(len(poses))                                     # random order against sorted
    s, p = score_dev(gm, scan, poses[perm])
    assert s.tobytes() == s_all[perm].tobytes() and p.tobytes() == p_all[perm].tobytes()
    for P in (1, 63, 64, 65, 257, 1000):                                   # P poses taken from the one list
        sel = rng.choice(len(poses), P, replace=False)
        s, p = score_dev(gm, scan, poses[sel])
        assert s.tobytes() == s_all[sel].tobytes() and p.tobytes() == p_all[sel].tobytes(), P
    for wg in (1, 7):
        ctx.set_option(capi.OPT_WORKGROUPS, wg)
        try:
            s, p = score_dev(gm, scan, poses)
        finally:
            ctx.set_option(capi.OPT_WORKGROUPS, 0)
        assert s.tobytes() == s_all.tobytes() and p.tobytes() == p_all.tobytes(), wg
    s, p = score_dev(gm, scan, poses, stride=16)                           # stride 16 against packed
    assert s.tobytes() == s_all.tobytes() and p.tobytes() == p_all.tobytes()
    s, _ = score_dev(gm, scan, poses, want_pairs=False)                    # pairs_dev == NULL
    assert s.tobytes() == s_all.tobytes()
    # lattice form against list form on the lattice's own poses (a lattice that lies on scan 1's part of the map)
    lat = dict(SMALL, x0=truth[0] - 1.8, y0=truth[1] - 0.9, yaw0=truth[2] - 0.2)
    L = capi_lattice(capi, lat)
    lp = L.poses()
    assert lp.tobytes() == lattice_poses(lat).tobytes()
    s_lat, p_lat = score_dev(gm, scan, lattice=L)
    s_lst, p_lst = score_dev(gm, scan, lp)
    assert (p_lat > 0).sum() > 50
    assert s_lat.tobytes() == s_lst.tobytes() and p_lat.tobytes() == p_lst.tobytes()


# ------------------------------------------------------------------------------------------ 5: scan sizes, staging
STAGE_LIMIT = 8000       # capi.SCORE_STAGE_POINTS: scans of up to this many points are staged in LDS


@pytest.mark.parametrize("n", [1, 63, 64, 65, 360, STAGE_LIMIT, STAGE_LIMIT + 1])
def test_scan_sizes_and_both_scan_paths(gpu, maps, n):
    capi, ctx = gpu
    gm, sf, _ = maps
    assert capi.SCORE_STAGE_POINTS == STAGE_LIMIT
    scan0, truth, poses = eval_poses(sf, 0, n_random=8)
    if n <= len(scan0):
        scan = scan0[:n]
    else:                                                                  # scan 0 tiled with 1 cm of jitter
        rng = np.random.default_rng(n)
        reps = -(-n // len(scan0))
        scan = (np.tile(scan0, (reps, 1))[:n] + rng.normal(0.0, 0.01, (n, 2))).astype(np.float32)
    s, p = score_dev(gm, scan, poses)
    assert n < 63 or p[1] > 0                                              # the truth meets the map
    assert_matches_eval_at(gm, scan, poses, s, p)
    # the path taken when staging is not possible, on the same scan (beyond the limit there is no other)
    ctx.set_option(capi.OPT_SCORE_STAGE, 0)
    try:
        s2, p2 = score_dev(gm, scan, poses)
    finally:
        ctx.set_option(capi.OPT_SCORE_STAGE, 1)
    assert s2.tobytes() == s.tobytes() and p2.tobytes() == p.tobytes()


# ------------------------------------------------------------------------------------------ 6: edges
def test_non_finite_scan_points_and_poses(gpu, oracle, maps, c1_world):
    capi, ctx = gpu
    gm, sf, cfg = maps
    om = oracle.Map(c1_world[0], oracle.default_params(resolution=cfg["resolution"]))
    scan, truth, _ = sf.make(0)
    poses = edge_poses(truth)
    s, p = gm.score_poses(scan, poses)
    s0, p0 = oracle_scores(oracle, om, scan, poses)
    assert np.array_equal(p, p0) and s == pytest.approx(s0, rel=1e-12, abs=1e-300)
    assert ((p == 0) == (s == 0.0)).all()
    # NaN and inf points add nothing: the score of the finite points alone
    dirty = scan.copy()
    dirty[5] = [np.nan, 1.0]; dirty[77] = [np.inf, -np.inf]; dirty[200] = [0.5, np.nan]; dirty[359] = [-np.inf, 2.0]
    clean = np.delete(scan, [5, 77, 200, 359], axis=0)
    sd, pd = gm.score_poses(dirty, poses)
    sc, pc = gm.score_poses(clean, poses)
    assert np.array_equal(pd, pc) and pd[0] > 0
    assert (np.abs(sd - sc) <= pc * 2.0 ** -52 * np.abs(sc)).all()          # (the points sit on other lanes: another order)
    # a pose with a NaN or inf component: 0 and 0, the others as they were
    bad = poses.copy()
    bad[0] = [np.nan, truth[1], truth[2]]; bad[2] = [truth[0], np.inf, 0.0]; bad[3] = [truth[0], truth[1], -np.inf]
    bad[4] = [truth[0], truth[1], np.nan]
    sb, pb = gm.score_poses(scan, bad)
    for q in (0, 2, 3, 4):
        assert sb[q] == 0.0 and pb[q] == 0
    keep = [1, 5, 6, 7, 8, 9]
    assert sb[keep].tobytes() == s[keep].tobytes() and pb[keep].tobytes() == p[keep].tobytes()


def test_one_voxel_map_and_far_world_offset(gpu, oracle, c1_world):
    capi, ctx = gpu
    m, sf, cfg = c1_world
    rng = np.random.default_rng(9)
    blob = rng.uniform(0.02, 0.28, (40, 2)).astype(np.float32)             # one voxel at resolution 0.3
    gm = capi.Map(ctx, blob, capi.default_params(resolution=0.3))
    om = oracle.Map(blob, oracle.default_params(resolution=0.3))
    assert gm.info().n_cells == 1
    scan = rng.uniform(-0.6, 0.9, (65, 2)).astype(np.float32)
    poses = np.array([[0, 0, 0], [0.3, -0.3, 0.5], [-0.29, 0.31, 3.0], [5, 5, 0], [0.0, 0.0, -2.0]], dtype=np.float64)
    s, p = gm.score_poses(scan, poses)
    s0, p0 = oracle_scores(oracle, om, scan, poses)
    assert np.array_equal(p, p0) and p[0] > 0 and p[3] == 0
    assert s == pytest.approx(s0, rel=1e-12, abs=1e-300)
    gm.close()
    # the world moved to (8191.7, 8191.7): float32 coordinates with 1 mm of resolution left
    off = np.array([8191.7, 8191.7])
    far = (m.astype(np.float64) + off).astype(np.float32)
    gm = capi.Map(ctx, far, capi.default_params(resolution=cfg["resolution"]))
    om = oracle.Map(far, oracle.default_params(resolution=cfg["resolution"]))
    scan, truth, poses = eval_poses(sf, 2, n_random=40)
    poses = poses + np.array([off[0], off[1], 0.0])
    s, p = gm.score_poses(scan, poses)
    s0, p0 = oracle_scores(oracle, om, scan, poses)
    assert np.array_equal(p, p0) and p[1] > 0
    assert s == pytest.approx(s0, rel=1e-12, abs=1e-300)
    gm.close()


# ------------------------------------------------------------------------------------------ 7: the pick
def select_dev(capi, gm, L, score, pairs, top_k, local_max):
    import torch
    d_s, d_p = to_dev(np.ascontiguousarray(score, np.float64)), to_dev(np.ascontiguousarray(pairs, np.uint32).view(np.int32))
    d_c = torch.full((top_k,), -1, dtype=torch.int64, device=d_s.device)
    d_n = torch.full((1,), -1, dtype=torch.int32, device=d_s.device)
    sync()
    gm.lattice_select(L, d_s.data_ptr(), d_p.data_ptr(), top_k, local_max, d_c.data_ptr(), d_n.data_ptr())
    sync()
    n = int(d_n.cpu()[0])
    return d_c.cpu().numpy()[:max(n, 0)].astype(np.uint64), n


@pytest.fixture(scope="module")
def lat_volume(gpu, maps):
    """The device's own score volume of LAT for scan 0 (computed once, left unchanged)."""
    capi, ctx = gpu
    gm, sf, _ = maps
    scan, _, _ = sf.make(0)
    s, p = score_dev(gm, scan, lattice=capi_lattice(capi, LAT))
    s.setflags(write=False); p.setflags(write=False)
    return s, p


@pytest.mark.parametrize("local_max", [0, 1])
@pytest.mark.parametrize("top_k", [1, 16, 1024])
def test_pick_on_the_devices_own_volume(gpu, maps, lat_volume, top_k, local_max):
    capi, ctx = gpu
    gm = maps[0]
    s, p = lat_volume
    assert len(s) == lattice_size(LAT) and (p > 0).sum() > 1000
    got, n = select_dev(capi, gm, capi_lattice(capi, LAT), s, p, top_k, local_max)
    want = ref_select(s, p, (LAT["nx"], LAT["ny"], LAT["nyaw"]), top_k, local_max)
    assert n == len(want) and np.array_equal(got, want)


@pytest.mark.parametrize("vol", crafted_volumes(), ids=[v[0] for v in crafted_volumes()])
def test_pick_on_crafted_volumes(gpu, maps, vol):
    capi, ctx = gpu
    gm = maps[0]
    _, dims, s, p = vol
    L = capi.PoseLattice(0.0, 0.0, 0.0, 1.0, 1.0, 0.1, dims[0], dims[1], dims[2])
    for local_max in (0, 1):
        for top_k in (1, 16, 1024):
            got, n = select_dev(capi, gm, L, s, p, top_k, local_max)
            want = ref_select(s, p, dims, top_k, local_max)
            assert n == len(want) and np.array_equal(got, want), (local_max, top_k)


# ------------------------------------------------------------------------------------------ 8: end to end
def same_records(a, b):
    return len(a) == len(b) and all(a[f].tobytes() == b[f].tobytes() for f in a.dtype.names)


@pytest.mark.parametrize("k", [0, 2, 6])
def test_relocalize_end_to_end(gpu, maps, k):
    capi, ctx = gpu
    gm, sf, _ = maps
    scan, truth, _ = sf.make(k)
    L = capi_lattice(capi, LAT)
    out = gm.relocalize(scan, L, top_k=16, want_scores=True)
    s = out["scores"]
    # the volume is the sweep's, the candidates the reference pick on it (pairs > 0 <=> score != 0: d1 < 0, every e > 0)
    pairs = (s != 0.0).astype(np.uint32)
    want = ref_select(s, pairs, (LAT["nx"], LAT["ny"], LAT["nyaw"]), 16, True)
    assert np.array_equal(out["cand_index"], want) and len(want) == 16
    assert out["cand_score"].tobytes() == s[want.astype(np.int64)].tobytes()
    inits = lattice_poses(LAT, want.astype(np.int64))
    ref = gm.align_batch(scan, [0, len(scan)], inits, shared_scan=True)
    assert same_records(out["records"], ref)                               # byte-identical
    assert out["best"] == ref_best(ref)
    win = out["records"][out["best"]]
    dm, dr = pose_error(win["pose"], truth)
    print("scan %d: winner = candidate %d, %.4f m, %.2e rad, cost %.3g" % (k, out["best"], dm, dr, win["fitness"]))
    assert win["converged"] and dm <= 0.05 and dr <= 0.002
    # the scan already on the device: the same answer
    d_sc = to_dev(scan)
    sync()
    dev = gm.relocalize(None, L, top_k=16, want_scores=True, dev_ptr=d_sc.data_ptr(), n=len(scan), stride=8)
    assert np.array_equal(dev["cand_index"], out["cand_index"]) and dev["best"] == out["best"]
    assert same_records(dev["records"], out["records"]) and dev["scores"].tobytes() == s.tobytes()
    assert dev["cand_score"].tobytes() == out["cand_score"].tobytes()


def test_relocalize_a_scan_that_misses_the_map_and_the_estimators_form(gpu, maps, c1_world):
    capi, ctx = gpu
    gm, sf, _ = maps
    scan, _, _ = sf.make(0)
    far = (scan + np.float32(500.0)).astype(np.float32)                    # 500 m off: no pose of the lattice brings it back
    out = gm.relocalize(far, capi_lattice(capi, dict(LAT, nx=9, ny=9, nyaw=4)), top_k=16, want_scores=True)
    assert len(out["cand_index"]) == 0 and out["best"] == -1 and (out["scores"] == 0.0).all()
    # the estimator's form, on a scan that does meet it
    from ndt_slam_amd.pose_estimator import NOT_CONVERGED_COST, PoseEstimator, Scan2D
    scan, truth, _ = sf.make(0)
    pe = PoseEstimator(ctx=ctx, Resolution=0.3, LeafSize=1e-4)             # (a leaf that keeps every point)
    pe.setScanPair(Scan2D(scan.astype(np.float64)), c1_world[0])
    est, cost = pe.relocalize(capi_lattice(capi, LAT), top_k=16)
    assert cost < NOT_CONVERGED_COST
    assert math.hypot(est.tx - truth[0], est.ty - truth[1]) <= 0.05
    assert abs((math.radians(est.th) - truth[2] + math.pi) % (2 * math.pi) - math.pi) <= 0.002


# ------------------------------------------------------------------------------------------ 9: ordering
def test_a_rebuild_queued_behind_a_sweep_waits_for_it(gpu, c1_world):
    import torch
    capi, ctx = gpu
    m, sf, cfg = c1_world
    prm = capi.default_params(resolution=cfg["resolution"], grid_margin=8)
    old = m
    new = (m[:3000] + np.float32([0.45, -0.3])).astype(np.float32)        # another cloud on (nearly) the same grid
    d_old, d_new = to_dev(old), to_dev(new)
    sync()
    gm = capi.Map(ctx, params=prm, dev_ptr=d_old.data_ptr(), n=len(old))
    scan, _, _ = sf.make(0)
    L = capi_lattice(capi, LAT)
    s_ref, p_ref = score_dev(gm, scan, lattice=L)                          # waited for
    dev = torch.device("cuda", 0)
    d_sc = to_dev(scan)
    d_s = torch.zeros(L.size, dtype=torch.float64, device=dev)
    d_p = torch.zeros(L.size, dtype=torch.int32, device=dev)
    other = torch.cuda.Stream()
    sync()
    gm.score_lattice(d_sc.data_ptr(), len(scan), L, d_s.data_ptr(), d_p.data_ptr(), stream=other.cuda_stream)
    gm.rebuild_begin(d_new.data_ptr(), len(new))                           # on the context's stream, directly behind
    gm.rebuild_end()
    sync()
    assert d_s.cpu().numpy().tobytes() == s_ref.tobytes()                  # the old map's scores
    assert d_p.cpu().numpy().view(np.uint32).tobytes() == p_ref.tobytes()
    fresh = capi.Map(ctx, new, prm)                                        # afterwards the map is the new one
    assert gm.info().n_cells == fresh.info().n_cells
    s2, p2 = score_dev(gm, scan, lattice=L)
    s3, p3 = score_dev(fresh, scan, lattice=L)
    assert s2.tobytes() == s3.tobytes() and p2.tobytes() == p3.tobytes() and s2.tobytes() != s_ref.tobytes()
    gm.close(); fresh.close()


# ------------------------------------------------------------------------------------------ 10: refusals
def test_refusals_leave_the_context_usable(gpu, maps):
    """Every refusal of the sweep and the pick that a caller can provoke through the C ABI on one device.  (A map that was
    never built cannot be made through the ABI: every call that creates one builds it.)"""
    import torch
    capi, ctx = gpu
    gm, sf, _ = maps
    lib = capi.lib()
    scan, truth, poses = eval_poses(sf, 0, n_random=4)
    d_sc, d_po = to_dev(scan), to_dev(poses)
    P, n = len(poses), len(scan)
    d_s = torch.zeros(P, dtype=torch.float64, device=d_sc.device)
    d_p = torch.zeros(P, dtype=torch.int32, device=d_sc.device)
    d_c = torch.zeros(16, dtype=torch.int64, device=d_sc.device)
    d_n = torch.zeros(1, dtype=torch.int32, device=d_sc.device)
    sync()
    sc, po, s_, p_ = d_sc.data_ptr(), d_po.data_ptr(), d_s.data_ptr(), d_p.data_ptr()
    good = capi_lattice(capi, SMALL)
    err = lambda: lib.ndt_last_error(ctx.h).decode()
    E = capi.NDT_E_ARG

    assert lib.ndt_score_poses_dev(None, gm.h, sc, n, 8, po, P, s_, p_, None) == E
    assert lib.ndt_last_error(None).decode() == "null context"
    assert lib.ndt_score_lattice_dev(None, gm.h, sc, n, 8, ctypes.byref(good), s_, p_, None) == E
    assert lib.ndt_score_poses(None, gm.h, scan.ctypes.data, n, 8, poses.ctypes.data, P, s_, p_) == E
    assert lib.ndt_lattice_select_dev(None, ctypes.byref(good), s_, p_, 4, 1, d_c.data_ptr(), d_n.data_ptr(), None) == E
    assert lib.ndt_last_error(None).decode() == "null context"

    def poses_dev(**kw):
        a = dict(map=gm.h, scan=sc, n=n, stride=8, poses=po, P=P, score=s_, pairs=p_)
        a.update(kw)
        return lib.ndt_score_poses_dev(ctx.h, a["map"], a["scan"], a["n"], a["stride"], a["poses"], a["P"], a["score"], a["pairs"], None)

    def lattice_dev(lat, **kw):
        a = dict(map=gm.h, scan=sc, n=n, stride=8, score=s_)
        a.update(kw)
        return lib.ndt_score_lattice_dev(ctx.h, a["map"], a["scan"], a["n"], a["stride"], None if lat is None else ctypes.byref(lat),
                                         a["score"], p_, None)

    for kw in (dict(map=None), dict(scan=None), dict(poses=None), dict(score=None), dict(n=0), dict(n=2 ** 31), dict(P=0),
               dict(P=2 ** 31), dict(stride=4), dict(stride=12), dict(stride=0)):
        assert poses_dev(**kw) == E, kw
        assert "ndt_score_poses_dev" in err()
    for kw in (dict(map=None), dict(scan=None), dict(score=None), dict(n=0), dict(n=2 ** 31), dict(stride=20)):
        assert lattice_dev(good, **kw) == E, kw
    assert lattice_dev(None) == E
    bad_lattices = [dict(nx=0), dict(ny=-3), dict(nyaw=0), dict(x0=float("nan")), dict(step_y=float("inf")),
                    dict(yaw0=-float("inf")), dict(nx=65536, ny=32768, nyaw=1)]
    for kw in bad_lattices:
        lat = capi_lattice(capi, SMALL)
        for f, v in kw.items():
            setattr(lat, f, v)
        assert lattice_dev(lat) == E, kw
        assert lib.ndt_lattice_select_dev(ctx.h, ctypes.byref(lat), s_, p_, 4, 1, d_c.data_ptr(), d_n.data_ptr(), None) == E, kw
    for top_k in (0, -1, 1025):
        assert lib.ndt_lattice_select_dev(ctx.h, ctypes.byref(good), s_, p_, top_k, 1, d_c.data_ptr(), d_n.data_ptr(), None) == E
    for args in ((None, p_, d_c.data_ptr(), d_n.data_ptr()), (s_, None, d_c.data_ptr(), d_n.data_ptr()),
                 (s_, p_, None, d_n.data_ptr()), (s_, p_, d_c.data_ptr(), None)):
        assert lib.ndt_lattice_select_dev(ctx.h, ctypes.byref(good), args[0], args[1], 4, 1, args[2], args[3], None) == E
    # host forms
    sh, ph = np.zeros(P), np.zeros(P, np.uint32)
    assert lib.ndt_score_poses(ctx.h, gm.h, None, n, 8, poses.ctypes.data, P, sh.ctypes.data, ph.ctypes.data) == E
    assert lib.ndt_score_poses(ctx.h, gm.h, scan.ctypes.data, n, 8, None, P, sh.ctypes.data, ph.ctypes.data) == E
    assert lib.ndt_score_poses(ctx.h, gm.h, scan.ctypes.data, n, 8, poses.ctypes.data, P, None, ph.ctypes.data) == E
    assert lib.ndt_score_poses(ctx.h, gm.h, scan.ctypes.data, n, 6, poses.ctypes.data, P, sh.ctypes.data, ph.ctypes.data) == E
    with pytest.raises(capi.NdtError):
        gm.relocalize(scan, good, top_k=0)
    with pytest.raises(capi.NdtError):
        gm.relocalize(scan, good, top_k=1025)
    # a map of another device, where there is one
    if torch.cuda.device_count() > 1:
        ctx1 = capi.Context(1)
        assert lib.ndt_score_poses_dev(ctx1.h, gm.h, sc, n, 8, po, P, s_, p_, None) == E
        assert "another device" in lib.ndt_last_error(ctx1.h).decode()
        ctx1.close()
    # an open ndt_map_rebuild_begin on the context
    cloud = to_dev(np.asarray(sf.map64, dtype=np.float32))
    sync()
    own = capi.Map(ctx, params=capi.default_params(resolution=0.3, grid_margin=8), dev_ptr=cloud.data_ptr(), n=len(cloud))
    own.rebuild_begin(cloud.data_ptr(), len(cloud))
    try:
        assert poses_dev() == E and "ndt_map_rebuild_begin" in err()
        assert lattice_dev(good) == E and "ndt_map_rebuild_begin" in err()
        assert lib.ndt_lattice_select_dev(ctx.h, ctypes.byref(good), s_, p_, 4, 1, d_c.data_ptr(), d_n.data_ptr(), None) == E
        with pytest.raises(capi.NdtError):
            gm.relocalize(scan, good)
    finally:
        own.rebuild_end()
    own.close()
    # nothing was queued, nothing written, and the context works
    sync()
    assert (d_s.cpu().numpy() == 0.0).all() and (d_c.cpu().numpy() == 0).all()
    s, p = score_dev(gm, scan, poses)
    assert_matches_eval_at(gm, scan, poses[:5], s, p)
