"""The map build on the device across the cloud shapes of tests/map_build_workloads.py: every family -- voxel sizes on both
sides of kBigVoxel, run counts on both sides of kBigRuns, shuffled voxels on both sides of kBigStage, finalize waves of
exactly kFinStage and kFinStage + 1 points, grids of kScanTile, kScanTile + 1 and 67 tiles of voxels, holes in runs, lattice
points, and one voxel per analytic case of leaf_finalize -- at leaves 0.1, 0.3 and 1 m and four offsets, against the C oracle
(equal, ties included) and against the exact rational reference (decided voxels, the bound the host test holds the oracle
to), and equal to itself through every way of building a map.  tests/test_map_build_host.py shows that the families reach
the paths they are named for and that the oracle agrees with the exact reference."""
import time

import numpy as np
import pytest

import map_build_workloads as W
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

COMBOS = [(leaf, off) for leaf in W.LEAVES for off in W.OFFSETS]
IDS = ["leaf%g@%g,%g" % (leaf, off[0], off[1]) for leaf, off in COMBOS]
ACCEPTED = ("accept", "raise1", "raise2")
INFO = ("min_bx", "min_by", "div_x", "div_y", "n_cells", "n_valid", "n_points")
TABLE = ("idx", "npts", "cent", "mean", "icov")
T0 = time.time()


def prm_of(mod, c):
    return mod.default_params(resolution=c.leaf, **W.params_of(c))


def snapshot(m):
    """(info fields, export arrays) of a map, device or oracle."""
    i = m.info()
    return tuple(int(getattr(i, k)) for k in INFO), m.export()


def same_bytes(a, b):
    return a[0] == b[0] and all(a[1][k].tobytes() == b[1][k].tobytes() for k in TABLE)


def assert_icov_close(g, o, what):
    """rel 1e-12 (the existing map-build tests' tolerance) where the two differ at all; inf and NaN only where both have it."""
    same = (g == o) | (np.isnan(g) & np.isnan(o))
    assert np.array_equal(np.isfinite(g), np.isfinite(o)), what
    assert g[~same] == pytest.approx(o[~same], rel=1e-12, abs=1e-300), what


_SOLO = {}


def solo(gpu, oracle, leaf, off):
    """[(case, device snapshot, oracle snapshot)] of one (leaf, offset): ndt_map_build from host memory, one map per case;
    built once and shared, unchanged, by the tests below."""
    capi, ctx = gpu
    key = (leaf, off)
    if key not in _SOLO:
        rows = []
        for c in W.cases(leaf, off):
            gm = capi.Map(ctx, c.cloud, prm_of(capi, c))
            rows.append((c, snapshot(gm), snapshot(oracle.Map(c.cloud, prm_of(oracle, c)))))
            gm.close()
        _SOLO[key] = rows
    return _SOLO[key]


@pytest.mark.parametrize("leaf,off", COMBOS, ids=IDS)
def test_every_family_equals_the_oracle(gpu, oracle, leaf, off):
    """ndt_map_info, cell indices, signed counts, float32 centroids and fp64 means equal; the inverse covariance at the
    tolerance of test_map_build_matches_oracle_bit_for_bit, on decided and undecided voxels alike: the device takes the
    oracle's side of every tie (the sign of a count IS the decision)."""
    for c, g, o in solo(gpu, oracle, leaf, off):
        assert g[0] == o[0], (c.name, g[0], o[0])
        for k in ("idx", "npts", "cent", "mean"):
            assert np.array_equal(g[1][k], o[1][k], equal_nan=True), (c.name, k)
        assert_icov_close(g[1]["icov"], o[1]["icov"], c.name)


@pytest.mark.parametrize("leaf,off", COMBOS, ids=IDS)
def test_every_family_against_the_exact_reference(gpu, oracle, leaf, off):
    """The device against exact_leaf on decided voxels, by the rule and the bound test_oracle_against_the_exact_reference
    applies to the oracle (map_build_workloads.icov_bound: derived, not measured)."""
    for c, g, _ in solo(gpu, oracle, leaf, off):
        T, ex, r2 = W.exact_cells(c)
        t = g[1]
        look = {int(v): k for k, v in enumerate(t["idx"])}
        assert set(look) == {v for v, e in ex.items() if e.decision != "below"}, c.name
        for v, k in look.items():
            e = ex[v]
            assert abs(int(t["npts"][k])) == e.n, (c.name, v)
            if not e.decided:
                continue
            assert (t["npts"][k] > 0) == (e.decision in ACCEPTED), (c.name, v, e.decision)
            mb = W.mean_bound(e)
            assert abs(t["mean"][k][0] - e.mean[0]) <= mb[0] and abs(t["mean"][k][1] - e.mean[1]) <= mb[1], (c.name, v)
            if e.icov is None:
                assert not t["icov"][k].any(), (c.name, v)
            else:
                assert np.abs(t["icov"][k] - np.array(e.icov)).max() <= W.icov_bound(e, r2), (c.name, v, e.n, e.decision)


@pytest.mark.parametrize("leaf,off", COMBOS, ids=IDS)
def test_one_result_whatever_the_form(gpu, oracle, leaf, off):
    """Byte-equal info and export between ndt_map_build from host memory and (a) ndt_map_build_dev with a 16-byte stride,
    (b) ndt_map_build_batch with every case of the (leaf, offset) in one call -- maps of 2 and of 541275 voxels, with no big
    voxel and with dozens, share the block prefixes and the one scan ticket -- and (c) the same call in reverse order."""
    import torch
    capi, ctx = gpu
    rows = solo(gpu, oracle, leaf, off)
    for c, g, _ in rows:
        wide = np.full((len(c.cloud), 4), np.nan, dtype=np.float32)
        wide[:, :2] = c.cloud
        d = torch.from_numpy(wide).cuda()
        torch.cuda.synchronize()
        gm = capi.Map(ctx, params=prm_of(capi, c), dev_ptr=d.data_ptr(), n=len(c.cloud), stride=16)
        assert same_bytes(snapshot(gm), g), ("stride 16", c.name)
        gm.close()
    for order in (rows, rows[::-1]):
        maps = capi.build_maps(ctx, [c.cloud for c, _, _ in order], [prm_of(capi, c) for c, _, _ in order])
        for (c, g, _), m in zip(order, maps):
            assert same_bytes(snapshot(m), g), ("batch", c.name)
        for m in maps:
            m.close()


CHAINS = (("sizes[min_pts=6]", "tiles[1031x525]"), ("wave_m[1536|1537]", "runs_k[200]"), ("shuffled[1537]", "leaves[ub=0,id=0,em=0]"),
          ("holes[129]", "tiles[2731x3]"), ("tiles[1031x525]", "live[1]"))


@pytest.mark.parametrize("leaf,off", COMBOS, ids=IDS)
def test_rebuild_chains(gpu, oracle, leaf, off):
    """A -> B -> A through one handle, with ndt_map_build and with ndt_map_rebuild_begin / _end, for pairs that differ in
    grid size (2 voxels against 541275), in the length of the big-voxel list and in the bounding box: the build queued
    with the stale grid sees points outside it, and every buffer is re-used at another size."""
    import torch
    capi, ctx = gpu
    by_name = {c.name: (c, g) for c, g, _ in solo(gpu, oracle, leaf, off)}
    for a, b in CHAINS:
        (ca, ga), (cb, gb) = by_name[a], by_name[b]
        gm = capi.Map(ctx, ca.cloud, prm_of(capi, ca))
        for c, g in ((cb, gb), (ca, ga)):
            gm.rebuild(xy=c.cloud, params=prm_of(capi, c))
            assert same_bytes(snapshot(gm), g), ("rebuild", a, b, c.name)
        for c, g in ((cb, gb), (ca, ga), (ca, ga)):
            d = torch.from_numpy(c.cloud).cuda()
            torch.cuda.synchronize()
            gm.params = prm_of(capi, c)
            gm.rebuild_begin(d.data_ptr(), len(c.cloud), 8)
            gm.rebuild_end()                                    # (third turn: the same cloud again, the speculative grid fits)
            assert same_bytes(snapshot(gm), g), ("rebuild_begin/_end", a, b, c.name)
        gm.close()


@pytest.mark.parametrize("leaf,off", COMBOS, ids=IDS)
def test_an_evaluation_on_every_cloud(gpu, oracle, leaf, off):
    """One ndt_eval_at per case at a pose that puts a scan of the cloud's own points a fraction of a voxel beside them: pairs
    equal, score, gradient and Hessian at the tolerances of test_single_evaluation_matches_oracle -- the centroid grid and
    the record array in HBM are the ones export showed.  (ndt_eval_at's kernel has an empty window: every point reads the HBM
    tables, global_pairs / load_rec_global.  The 48-byte LDS records the match kernel stages from them, fill_window_fetch, are
    held by tests/test_gpu_match_window_geometry.py.)
    The `leaves` cases with eig_mult 0 and no identity start hold voxels whose inverse covariance is not finite
    (leaf_finalize's third return; they stay in the search set, as in PCL).  A pair with such a voxel has a NaN exponent and
    is dropped by updateDerivatives' check -- or, for the diagonal line's (inf, -inf, inf) and a point on its far side, an
    exponent of -inf, e = 0, and then 0 * inf in the reference's own gradient: where the ORACLE's sums are NaN (it poisons
    itself exactly as PCL would) there is nothing to compare the gradient and the Hessian with, and the pair count and the
    score alone are held; the device drops those pairs too and stays finite.  No other case may have a NaN there."""
    capi, ctx = gpu
    for c in W.cases(leaf, off):
        scan, p = W.on_cloud_scan(c)
        gm, om = capi.Map(ctx, c.cloud, prm_of(capi, c)), oracle.Map(c.cloud, prm_of(oracle, c))
        s, g, H, pairs = gm.eval_at(scan, p)
        s0, g0, H0, pairs0 = om.eval_at(scan, p)
        gm.close()
        assert pairs == pairs0 and pairs > 0, c.name
        assert s == pytest.approx(s0, rel=1e-12, abs=1e-300), c.name
        assert np.isfinite(g).all() and np.isfinite(H).all(), c.name
        if not (np.isfinite(g0).all() and np.isfinite(H0).all()):
            assert c.family == "leaves" and c.prm["eig_mult"] == 0.0 and not c.prm["cov_init_identity"], c.name
            continue
        assert g == pytest.approx(g0, rel=1e-9, abs=1e-10 * (np.abs(g0).max() + 1e-300)), c.name
        assert H == pytest.approx(H0, rel=1e-9, abs=1e-10 * (np.abs(H0).max() + 1e-300)), c.name


def test_report_the_wall_time_of_this_module():
    print("\n  test_gpu_map_build_geometry.py: %.1f s from import to here" % (time.time() - T0))
