"""ndt_occ_* on the device: counters, stats and renders against the numpy restatement (tests/occ_helpers.py), integer
equality throughout -- every octant and degenerate beam, the grid's borders, the skip rules, the boundaries of runs and of the
LDS prefix, contention on one cell, independence of order / batching / stride / form, accumulation and clear, ordering across
streams, the sessions form and the refusals.  The shapes are the smallest at which the kernels can go wrong."""
import ctypes

import numpy as np
import pytest

import occ_helpers as H
from session_helpers import lockstep, same_records, session_logs
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32
OFFSET_GEOM = H.Geometry(-1003.3, 707.1, 0.05, 64, 48)        # a world offset of the fitness tests; 0.05 is no short double
EXACT_GEOM = H.Geometry(0.0, 0.0, 0.25, 300, 300)


def centre(g, ix, iy):
    """The fp64 centre of cell (ix, iy) (arrays allowed) as float32 points [n, 2]."""
    ix, iy = np.asarray(ix, np.float64), np.asarray(iy, np.float64)
    return np.stack([g.x0 + (ix + 0.5) * g.res, g.y0 + (iy + 0.5) * g.res], axis=-1).astype(F).reshape(-1, 2)


def run_host(gpu, geoms, scans, origins, grid_of=None, max_range2=H.DBL_MAX, grids=None):
    """ndt_occ_integrate on new (or the given) grids -> (grids, stats tuple)."""
    capi, ctx = gpu
    if grids is None:
        grids = [capi.OccGrid(ctx, g) for g in geoms]
    xy, off = H.pack(scans)
    st = capi.integrate_occ(ctx, grids, xy, off, np.asarray(origins, np.float64), grid_of, max_range2)
    return grids, H.stats_tuple(st)


def check(gpu, geoms, scans, origins, grid_of=None, max_range2=H.DBL_MAX, what=""):
    """One host-form call against the helper: counters of every grid and the stats.  -> (expected counters, stats)."""
    grids, got = run_host(gpu, geoms, scans, origins, grid_of, max_range2)
    want, st = H.integrate(geoms, scans, origins, grid_of, max_range2)
    for k, g in enumerate(grids):
        hit, pas = g.counts()
        bad_h, bad_p = np.argwhere(hit != want[k][0]), np.argwhere(pas != want[k][1])
        assert not len(bad_h), (what, "hit", k, bad_h[:5].tolist(), hit[tuple(bad_h[0])], want[k][0][tuple(bad_h[0])])
        assert not len(bad_p), (what, "pass", k, bad_p[:5].tolist(), pas[tuple(bad_p[0])], want[k][1][tuple(bad_p[0])])
        g.close()
    assert got == H.stats_tuple(st), (what, got, H.stats_tuple(st))
    return want, st


def all_ends(g, ring=2):
    ix, iy = np.meshgrid(np.arange(-ring, g.nx + ring), np.arange(-ring, g.ny + ring))
    return centre(g, ix.ravel(), iy.ravel())


# ------------------------------------------------------------------------------------------ 1: every octant
@pytest.mark.parametrize("g", [OFFSET_GEOM, H.Geometry(0.0, 0.0, 0.25, 64, 48)], ids=["offset", "exact"])
def test_every_octant_and_degenerate_beam(gpu, g):
    """One scan from the middle of a 64 x 48 grid to every cell and a ring of two cells around the grid."""
    ends = all_ends(g)
    org = centre(g, 32, 24)[0].astype(np.float64)
    live, X1, Y1, X0, Y0 = H.classify(g, org, ends)
    dx, dy = np.abs(X1 - X0), np.abs(Y1 - Y0)
    L = np.maximum(dx, dy)
    assert live.all() and (X0, Y0) == (32, 24) and len(ends) == 68 * 52
    for cond in (L == 0, L == 1, (dx == dy) & (L > 1), dx == dy + 1, dy == dx + 1, (dx == 0) & (L > 1), (dy == 0) & (L > 1)):
        assert cond.any()
    want, st = check(gpu, [g], [ends], [org], what="octants")
    assert st["n_hit"] == 64 * 48 and want[0][1][24, 32] == int((L >= 1).sum())


# ------------------------------------------------------------------------------------------ 2: borders
@pytest.mark.parametrize("shape", [(64, 48), (1, 1), (1, 37), (37, 1)])
def test_borders_and_thin_grids(gpu, shape):
    """Origins outside the grid (beams that enter it, cross it with both ends outside, or miss it) and one inside."""
    g = H.Geometry(-1003.3, 707.1, 0.05, shape[0], shape[1])
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    ends = all_ends(g, ring=3)
    far = centre(g, rng.integers(-90, 160, size=400), rng.integers(-90, 140, size=400))
    # from (-7, -5) to the mirror cell and its neighbours: through the grid, both ends outside; and away from it: a miss
    j = np.arange(-2, 3)
    cross = centre(g, np.concatenate([shape[0] + 6 + j, -20 + j]), np.concatenate([shape[1] + 4 + j[::-1], -9 + j]))
    scans = [ends, far, np.concatenate([ends[::7], far]), far[::-1], cross]
    origins = [centre(g, -5, shape[1] + 9)[0], centre(g, shape[0] + 40, -30)[0], centre(g, shape[0] // 2, -70)[0],
               centre(g, shape[0] // 2, shape[1] // 2)[0], centre(g, -7, -5)[0]]
    want, st = check(gpu, [g], scans, np.asarray(origins, np.float64), what=str(shape))
    assert 0 < st["n_hit"] < st["n_beams"] and st["n_skipped"] == 0
    _, st_cross = H.integrate([g], [cross[:5]], [np.asarray(origins[4], np.float64)])
    _, st_miss = H.integrate([g], [cross[5:]], [np.asarray(origins[4], np.float64)])
    assert st_cross["n_pass"] > 0 and st_cross["n_hit"] == 0 and H.stats_tuple(st_miss) == (5, 0, 0, 0)


# ------------------------------------------------------------------------------------------ 3: skips
def test_skips(gpu):
    g0, g1 = EXACT_GEOM, H.Geometry(0.0, 0.0, 0.25, 64, 8)
    rng = np.random.default_rng(3)
    near = centre(g0, rng.integers(100, 200, size=300), rng.integers(100, 200, size=300))
    bad = near[:40].copy()
    bad[3, 0] = np.nan; bad[7, 1] = np.inf; bad[11] = (-np.inf, np.nan); bad[39, 0] = np.inf
    org = np.array([37.625, 37.625])                                              # cell (150, 150)
    long_ = np.array([[0.125 + 0.25 * 65536, 0.125], [0.125 + 0.25 * 65537, 0.125], [0.125, 0.125 + 0.25 * 65536],
                      [0.125 + 0.25 * 65536, 0.125 + 0.25 * 65537], [-0.125 - 0.25 * 65535, 0.125]], F)
    edge = np.array([[268435456.0 - 32.0, 0.125], [268435456.0 + 32.0, 0.125], [268435456.0, 0.125], [0.125, -268435456.0 - 64.0],
                     [0.125, -268435456.0]], F)                                   # cells 2^30 - 128, 2^30 + 128, 2^30, ...
    scans = [bad, near, near, long_, edge, near[:50], near[:60], near[:70], edge]
    origins = np.array([org, [np.nan, 37.625], [37.625, -np.inf], [0.125, 0.125], [268435456.0, 0.125], org, org, org,
                        [3.0e8, 0.125]])
    grid_of = np.array([0, 0, 1, 1, 0, -1, 2, 1, 0], np.int32)
    live_long = H.classify(g1, origins[3], long_)[0]
    assert live_long.tolist() == [True, False, True, False, True]                # L = 65536 lives, 65537 does not
    assert H.classify(g0, origins[4], edge)[0].tolist() == [True, False, True, False, False]
    assert not H.classify(g0, origins[8], edge)[0].any()                         # the origin's index is beyond 2^30
    want, st = check(gpu, [g0, g1], scans, origins, grid_of, what="skips")
    assert st["n_skipped"] == 4 + 300 + 300 + 2 + 3 + 50 + 60 + 0 + 5 and st["n_beams"] == sum(len(s) for s in scans)
    # the `>` of the range cut, at a value present among the squared lengths and at the double just below it
    d = near.astype(np.float64) - org
    d2 = np.sort(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    v = float(d2[len(d2) // 2])
    n_at = int((d2 == v).sum())
    _, st_in = check(gpu, [g0], [near], [org], max_range2=v, what="range at the value")
    _, st_out = check(gpu, [g0], [near], [org], max_range2=float(np.nextafter(v, 0.0)), what="range just below")
    assert st_out["n_skipped"] - st_in["n_skipped"] == n_at >= 1
    _, st0 = check(gpu, [g0], [near], [org], max_range2=0.0, what="range 0")
    assert st0["n_skipped"] == int((d2 > 0).sum())


# ------------------------------------------------------------------------------------------ 4: runs and the prefix
def test_run_and_prefix_boundaries(gpu):
    g0, g1 = EXACT_GEOM, H.Geometry(-100.0, 36.0, 0.25, 5400, 6)
    rng = np.random.default_rng(4)
    org = np.array([37.625, 37.625])
    scans, grid_of = [], []

    def add(s, k=0):
        scans.append(np.asarray(s, F).reshape(-1, 2)); grid_of.append(k)
    add(np.zeros((0, 2)))                                                         # an empty scan at the front
    for n in (1, 63, 64, 65, 255, 256, 257, 513, 1025):
        add(centre(g0, 150 + rng.integers(-40, 41, size=n), 150 + rng.integers(-40, 41, size=n)))
        if n == 65:
            add(np.zeros((0, 2))); add(np.zeros((0, 2)))                          # ... in the middle
    # runs whose items sum to T: four beams of 3 items and one of T - 12 (a horizontal beam of L = T - 13)
    for T in (63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025):
        add(centre(g0, [152, 148, 150, 150, 150 + T - 13], [150, 150, 152, 148, 150]))
    # 256 beams of one item each: the prefix is the identity; and 257: the second run holds one
    add(np.repeat(centre(g0, 150, 150), 256, axis=0)); add(np.repeat(centre(g0, 150, 150), 257, axis=0))
    # one beam with more items than all the others of its run together, into the long grid
    big = centre(g1, 400 + rng.integers(0, 4, size=256), 2 + rng.integers(-2, 3, size=256))
    big[100] = centre(g1, 400 + 5000, 3)[0]
    add(big, 1)
    add(np.zeros((0, 2)))                                                         # ... and at the back
    origins = np.tile(org, (len(scans), 1))
    origins[-2] = centre(g1, 400, 2)[0]
    want, st = check(gpu, [g0, g1], scans, origins, np.array(grid_of, np.int32), what="runs")
    assert st["n_skipped"] == 0 and want[1][1][3, 400 + 4999 - 0] >= 1


def test_more_scans_than_the_jobs_kernel_has_threads(gpu):
    """300 scans in one call, their lengths cycling through 0, 1, 255, 256, 257, 3, into three grids: occ_jobs_kernel numbers
    the runs in rounds of 256 scans and carries the count from one round into the next."""
    capi, ctx = gpu
    geoms = [H.Geometry(0.0, 0.0, 0.25, 64, 48), OFFSET_GEOM, H.Geometry(-3.0, -2.0, 0.125, 40, 56)]
    cells = [(32, 24), (30, 20), (21, 30)]
    rng = np.random.default_rng(44)
    lengths = [(0, 1, 255, 256, 257, 3)[b % 6] for b in range(300)]
    grid_of = rng.integers(0, 3, size=300).astype(np.int32)
    scans = [centre(geoms[k], cells[k][0] + rng.integers(-12, 13, size=n), cells[k][1] + rng.integers(-12, 13, size=n))
             for k, n in zip(grid_of, lengths)]
    origins = np.array([centre(geoms[k], cells[k][0] + rng.integers(-2, 3), cells[k][1] + rng.integers(-2, 3))[0] for k in grid_of], np.float64)
    runs = np.cumsum([-(-n // 256) for n in lengths])
    assert runs[255] < runs[256] < runs[-1] and len(set(grid_of[250:262].tolist())) == 3      # runs on both sides of the round's end
    want, st = check(gpu, geoms, scans, origins, grid_of, what="300 scans")
    assert st["n_beams"] == sum(lengths) and st["n_skipped"] == 0 and all(w[0].sum() > 0 for w in want)
    ctx.set_option(2, 1)                                                          # NDT_OPT_WORKGROUPS
    try:
        grids, got = run_host(gpu, geoms, scans, origins, grid_of)
    finally:
        ctx.set_option(2, 0)
    assert got == H.stats_tuple(st)
    for g, w in zip(grids, want):
        hit, pas = g.counts()
        assert np.array_equal(hit, w[0]) and np.array_equal(pas, w[1])
        g.close()


# ------------------------------------------------------------------------------------------ 5: contention
def test_contention_on_the_origin_cell(gpu):
    g = H.Geometry(-6.4, -6.4, 0.05, 256, 256)
    a = np.arange(4096) * (2 * np.pi / 4096)
    r = np.where(np.arange(4096) % 64 == 0, 0.0, 5.0)                            # some beams end in the origin cell itself
    org = np.array([0.013, -0.021])
    ends = np.stack([org[0] + r * np.cos(a), org[1] + r * np.sin(a)], axis=1).astype(F)
    want, st = check(gpu, [g], [ends], [org], what="circle")
    live, X1, Y1, X0, Y0 = H.classify(g, org, ends)
    L = np.maximum(np.abs(X1 - X0), np.abs(Y1 - Y0))
    assert live.all() and want[0][1][Y0, X0] == int((L >= 1).sum()) == 4096 - 64 and want[0][0][Y0, X0] == 64


# ------------------------------------------------------------------------------------------ 6: independence
def test_independence_of_order_batching_grid_stride_and_form(gpu):
    import torch
    capi, ctx = gpu
    geoms = [EXACT_GEOM, H.Geometry(-1003.3, 707.1, 0.05, 200, 150), H.Geometry(10.0, 10.0, 0.25, 120, 90)]
    centres = [np.array([37.625, 37.625]), centre(geoms[1], 100, 75)[0].astype(np.float64), np.array([25.125, 21.125])]
    rng = np.random.default_rng(6)
    grid_of = np.array([0, 1, 2, 1, 0, 2, 1], np.int32)
    sizes = (300, 1, 257, 0, 512, 77, 900)
    scans, origins = [], []
    for b in range(7):
        g, c = geoms[grid_of[b]], centres[grid_of[b]]
        scans.append((c + rng.uniform(-22.0, 22.0, size=(sizes[b], 2)) * g.res * 4).astype(F))
        origins.append(c + rng.uniform(-3.0, 3.0, size=2) * g.res)
    origins = np.array(origins)

    def result(grids, stats):
        out = b"".join(np.concatenate(g.counts()).tobytes() for g in grids) + bytes(np.array(stats, np.uint64))
        for g in grids:
            g.close()
        return out
    grids, st = run_host(gpu, geoms, scans, origins, grid_of)
    base = result(grids, st)
    want, wst = H.integrate(geoms, scans, origins, grid_of)
    assert base == b"".join(np.concatenate(w).tobytes() for w in want) + bytes(np.array(H.stats_tuple(wst), np.uint64))
    # reversed scan order
    grids, st = run_host(gpu, geoms, scans[::-1], origins[::-1], grid_of[::-1])
    assert result(grids, st) == base
    # each scan in a call of its own: the stats add up
    grids, tot = [capi.OccGrid(ctx, g) for g in geoms], np.zeros(4, np.uint64)
    for b in range(7):
        _, st = run_host(gpu, geoms, [scans[b]], origins[b:b + 1], grid_of[b:b + 1], grids=grids)
        tot += np.array(st, np.uint64)
    assert result(grids, tuple(int(v) for v in tot)) == base
    # one workgroup
    ctx.set_option(2, 1)                                                          # NDT_OPT_WORKGROUPS
    try:
        grids, st = run_host(gpu, geoms, scans, origins, grid_of)
    finally:
        ctx.set_option(2, 0)
    assert result(grids, st) == base
    # origins at stride 24 (pose triples) against stride 16
    grids, st = run_host(gpu, geoms, scans, np.concatenate([origins, np.full((7, 1), 33.0)], axis=1), grid_of)
    assert result(grids, st) == base
    # the device form, origins at stride 24
    dev = torch.device("cuda", 0)
    xy, off = H.pack(scans)
    d_xy, d_off = torch.from_numpy(xy).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev)
    d_org = torch.from_numpy(np.concatenate([origins, np.full((7, 1), -7.0)], axis=1)).to(dev)
    d_gof, d_st = torch.from_numpy(grid_of.copy()).to(dev), torch.full((4,), 99, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    grids = [capi.OccGrid(ctx, g) for g in geoms]
    capi.integrate_occ_dev(ctx, grids, d_gof.data_ptr(), d_xy.data_ptr(), d_off.data_ptr(), 7, len(xy), d_org.data_ptr(), 24, H.DBL_MAX,
                           d_st.data_ptr())
    hit0, _ = grids[0].counts()                                                   # (waits for the context's stream)
    st = tuple(int(v) for v in d_st.cpu().numpy())
    assert result(grids, st) == base and hit0.sum() > 0


# ------------------------------------------------------------------------------------------ 7: accumulation, clear, render
def test_accumulation_clear_and_render(gpu):
    capi, ctx = gpu
    g = H.Geometry(0.0, 0.0, 0.25, 40, 30)
    rng = np.random.default_rng(7)
    org = np.array([5.125, 3.625])                                                # cell (20, 14)
    a = centre(g, rng.integers(0, 40, size=200), rng.integers(0, 30, size=200))
    b = np.concatenate([centre(g, rng.integers(0, 40, size=150), rng.integers(0, 30, size=150)),
                        np.repeat(centre(g, 20, 14), 5, axis=0),                  # the origin cell: hits, and passes of the others
                        np.repeat(centre(g, 39, 29), 3, axis=0)])                 # a corner: hits, no pass
    grid = capi.OccGrid(ctx, g)
    grid.integrate(a, [0, len(a)], [org])
    grid.integrate(b, [0, len(b)], [org])
    want, _ = H.integrate([g], [a, b], [org, org])
    hit, pas = grid.counts()
    assert np.array_equal(hit, want[0][0]) and np.array_equal(pas, want[0][1])
    assert ((hit > 0) & (pas == 0)).any() and ((hit == 0) & (pas > 0)).any() and ((hit == 0) & (pas == 0)).any()
    for min_obs in (1, 3):
        r = grid.render(min_obs)
        assert r.dtype == np.int8 and np.array_equal(r, H.render(hit, pas, min_obs)), min_obs
    assert (grid.render(3) == -1).sum() > (grid.render(1) == -1).sum() and grid.render(1).max() == 100
    grid.clear()
    hit, pas = grid.counts()
    assert not hit.any() and not pas.any() and (grid.render(1) == -1).all()
    grid.integrate(a, [0, len(a)], [org])
    want, _ = H.integrate([g], [a], [org])
    hit, pas = grid.counts()
    assert np.array_equal(hit, want[0][0]) and np.array_equal(pas, want[0][1])
    geo = capi.OccGeometry()
    ctx.check(capi.lib().ndt_occ_geometry_get(grid.h, ctypes.byref(geo)), "ndt_occ_geometry_get")
    assert (geo.x0, geo.y0, geo.res, geo.nx, geo.ny) == tuple(g) and grid.cells_ptr()
    grid.close()


# ------------------------------------------------------------------------------------------ 8: ordering across streams
def test_render_and_counts_on_another_stream_see_the_finished_integrate(gpu):
    import torch
    capi, ctx = gpu
    g = H.Geometry(0.0, 0.0, 0.25, 512, 512)
    rng = np.random.default_rng(8)
    ends = centre(g, rng.integers(0, 512, size=6000), rng.integers(0, 512, size=6000))
    org = np.array([[64.125, 64.125, 0.0]])
    want, _ = H.integrate([g], [ends], org)
    dev = torch.device("cuda", 0)
    d_xy = torch.from_numpy(ends).to(dev)
    d_off = torch.from_numpy(np.array([0, len(ends)], np.int64)).to(dev)
    d_org = torch.from_numpy(org).to(dev)
    d_out = torch.full((512 * 512,), 77, dtype=torch.int8, device=dev)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    grid = capi.OccGrid(ctx, g)
    grid.integrate_dev(d_xy.data_ptr(), d_off.data_ptr(), 1, len(ends), d_org.data_ptr(), 24, stream=sa.cuda_stream)
    grid.render_dev(d_out.data_ptr(), 1, stream=sb.cuda_stream)                   # queued at once, on another stream
    hit, pas = grid.counts()                                                      # ... and on the context's own
    assert np.array_equal(hit, want[0][0]) and np.array_equal(pas, want[0][1])
    sb.synchronize()
    assert np.array_equal(d_out.cpu().numpy().reshape(512, 512), H.render(want[0][0], want[0][1], 1))
    grid.clear(stream=sa.cuda_stream)                                             # a clear on A, a read on the context's stream
    hit, pas = grid.counts()
    assert not hit.any() and not pas.any()
    torch.cuda.synchronize()
    grid.close()


# ------------------------------------------------------------------------------------------ 9: sessions
def test_sessions_integrate_their_newest_scan_and_change_nothing(gpu):
    import torch
    from ndt_slam_amd import replay
    capi, ctx = gpu
    p = dict(replay.LAUNCH_PARAMS, sepThre=2.5)
    logs = session_logs(((33, 9), (34, 6), (35, 8), (36, 5)))
    starts = [0, 0, 2, 0]                                                         # session 2 starts late, 1 and 3 end early
    S = 4
    geoms = [H.Geometry(-25.0, -25.0, 0.1, 500, 500), H.Geometry(-20.05, -20.05, 0.05, 800, 800),
             H.Geometry(-25.0, -25.0, 0.25, 200, 200), H.Geometry(-3.0, -3.0, 0.1, 60, 60)]      # (the last: most beams leave it)
    ses = capi.Sessions(ctx, S, capi.session_params_from_launch(p))
    twin = capi.Sessions(ctx, S, capi.session_params_from_launch(p))
    grids = [capi.OccGrid(ctx, g) for g in geoms]
    dev = torch.device("cuda", 0)
    exp_scans, exp_org, exp_of, total = [], [], [], np.zeros(4, np.uint64)
    for k, scans, odo, act in lockstep(logs, starts):
        recs, recs2 = ses.step(scans, odo, act), twin.step(scans, odo, act)
        st = ses.occ_integrate(grids, np.ascontiguousarray(recs["stepped"], np.uint8))
        total += np.array(H.stats_tuple(st), np.uint64)
        for i in range(S):
            assert same_records(recs[i], recs2[i]), (k, i)
            if not recs[i]["stepped"]:
                continue
            # the chain of the single entry points: resample, then growMap's transform at the record's pose
            lps = ctx.resample(scans[i], p["space"], p["space_thre"])
            d_in, d_off = torch.from_numpy(lps).to(dev), torch.from_numpy(np.array([0, len(lps)], np.int64)).to(dev)
            d_pose = torch.from_numpy(np.array(recs[i]["pose"], np.float64).reshape(1, 3)).to(dev)
            d_out = torch.zeros((max(len(lps), 1), 2), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            ctx.scan_to_map_batch_dev(d_in.data_ptr(), 16, d_off.data_ptr(), 1, len(lps), d_pose.data_ptr(), d_out.data_ptr())
            torch.cuda.synchronize()
            exp_scans.append(d_out.cpu().numpy()[:len(lps)].copy()); exp_org.append(np.array(recs[i]["pose"][:2], np.float64))
            exp_of.append(i)
        assert bytes(ses.stats()) == bytes(twin.stats()), k
    want, wst = H.integrate(geoms, exp_scans, exp_org, exp_of)
    assert len(exp_scans) == 9 + 6 + 8 + 5 and tuple(int(v) for v in total) == H.stats_tuple(wst)
    for i in range(S):
        hit, pas = grids[i].counts()
        assert np.array_equal(hit, want[i][0]) and np.array_equal(pas, want[i][1]), i
        assert pas.sum() > 100
    # which = None takes every started session again: its last scan a second time
    st = ses.occ_integrate(grids)
    last = [max(j for j in range(len(exp_of)) if exp_of[j] == i) for i in range(S)]
    _, st_last = H.integrate(geoms, [exp_scans[j] for j in last], [exp_org[j] for j in last], list(range(S)), counters=want)
    assert H.stats_tuple(st) == H.stats_tuple(st_last)
    for i in range(S):
        hit, pas = grids[i].counts()
        assert np.array_equal(hit, want[i][0]) and np.array_equal(pas, want[i][1]), i
    # a taken session without a grid is refused; one not taken needs none
    with pytest.raises(capi.NdtError):
        ses.occ_integrate([grids[0], None, grids[2], grids[3]])
    ses.occ_integrate([grids[0], None, grids[2], grids[3]], np.array([1, 0, 1, 1], np.uint8))
    for x in grids:
        x.close()
    ses.close(); twin.close()


# ------------------------------------------------------------------------------------------ 10: refusals
def test_refusals_leave_everything_as_it_was(gpu):
    capi, ctx = gpu
    L = capi.lib()
    g = H.Geometry(0.0, 0.0, 0.25, 16, 16)
    grid, other_ctx = capi.OccGrid(ctx, g), capi.Context(0)
    foreign = capi.OccGrid(other_ctx, g)
    ends = centre(g, [3, 9], [4, 12])
    grid.integrate(ends, [0, 2], [[2.1, 2.1]])
    before = np.concatenate(grid.counts()).tobytes()
    xy, off, org = np.ascontiguousarray(ends), np.array([0, 2], np.uint64), np.array([[2.1, 2.1, 0.0]])
    st = np.full(4, 0x5A5A5A5A, np.uint64)
    hs = lambda *gs: (ctypes.c_void_p * len(gs))(*[x.h if x is not None else None for x in gs])      # noqa: E731

    def refuse(text, occs=None, n_occ=1, xy_p=xy.ctypes.data, off_p=off.ctypes.data, B=1, org_p=org.ctypes.data, stride=24, r2=H.DBL_MAX,
               c=ctx.h):
        rc = L.ndt_occ_integrate(c, hs(grid) if occs is None else occs, n_occ, None, xy_p, off_p, B, org_p, stride, r2, st.ctypes.data)
        msg = L.ndt_last_error(c).decode()
        assert rc == -1 and text in msg, (text, rc, msg)
    refuse("null context", c=None)
    refuse("NULL array", xy_p=None); refuse("NULL array", off_p=None); refuse("NULL array", org_p=None)
    refuse("n_occ >= 1", n_occ=0); refuse("B >= 1", B=0)
    refuse("grid 0 is NULL", occs=hs(None))
    refuse("grid 1 belongs to another context", occs=hs(grid, foreign), n_occ=2)
    refuse("grid 1 is given twice", occs=hs(grid, grid), n_occ=2)
    refuse("origin_stride", stride=8); refuse("origin_stride", stride=20)
    refuse("max_range2", r2=float("nan")); refuse("max_range2", r2=-1.0)
    bad_off = np.array([2, 0], np.uint64)
    refuse("offsets decrease", off_p=bad_off.ctypes.data)
    assert L.ndt_occ_integrate_dev(ctx.h, hs(grid), 1, None, None, None, 1, 2, None, 24, H.DBL_MAX, None, None) == -1
    out = np.full(16 * 16, 55, np.int8)
    assert L.ndt_occ_render(ctx.h, grid.h, 0, out.ctypes.data) == -1 and "min_obs" in L.ndt_last_error(ctx.h).decode()
    assert L.ndt_occ_render(ctx.h, foreign.h, 1, out.ctypes.data) == -1 and L.ndt_occ_render(ctx.h, grid.h, 1, None) == -1
    assert L.ndt_occ_counts(ctx.h, grid.h, None, None) == -1 and L.ndt_occ_clear(ctx.h, foreign.h, None) == -1
    assert L.ndt_occ_clear(None, grid.h, None) == -1 and L.ndt_last_error(None).decode() == "null context"
    h = ctypes.c_void_p(1234)
    for bad, code in (((0.0, 0.0, 0.0, 4, 4), -1), ((0.0, np.nan, 0.1, 4, 4), -1), ((0.0, 0.0, 0.1, 0, 4), -1),
                      ((0.0, 0.0, 0.1, 1 << 15, 1 << 14), -4)):
        G = capi.OccGeometry(*bad)
        assert L.ndt_occ_create(ctx.h, ctypes.byref(G), ctypes.byref(h)) == code and h.value == 1234, bad
    assert (st == 0x5A5A5A5A).all() and (out == 55).all()
    assert np.concatenate(grid.counts()).tobytes() == before
    # an open ndt_map_rebuild_begin on the context refuses as it does everywhere
    import torch
    cloud = torch.rand((500, 2), dtype=torch.float32, device="cuda") * 10
    torch.cuda.synchronize()
    m = capi.Map(ctx, cloud.cpu().numpy(), capi.default_params(resolution=1.0))
    m.rebuild_begin(cloud.data_ptr(), 500)
    refuse("ndt_map_rebuild_begin")
    m.rebuild_end()
    m.close()
    foreign.close(); other_ctx.close(); grid.close()
