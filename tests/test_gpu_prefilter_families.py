"""The device pre-filter on the slot-collision cloud families of tests/prefilter_workloads.py: every family down every path
of the two kernels, the point stride, the second round of the workgroups' batch loop and of the pack loop, a scan's
independence of its place in a batch, and the isolation of a scan whose coordinates the reference leaves undefined.
Equal shape and equal bytes against the CPU oracle throughout (tests/test_prefilter_model_host.py holds the oracle to the
Python model on the same families); no tolerances."""
import ctypes

import numpy as np
import pytest

import prefilter_workloads as W
from gpu_support import gpu, same_bits, sync, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu
EMPTY = np.zeros((0, 2), np.float32)
SENTINEL = np.float32(-777.0)


def reference(oracle, cloud, leaf):
    return oracle.approx_voxel_filter(cloud, leaf).reshape(-1, 2) if len(cloud) else EMPTY


def batch_on_device(capi, ctx, scans, leaf, width=2):
    """ndt_prefilter_batch_dev on scans of [n, width] float32 -> (filtered scans, offsets, the whole output buffer)."""
    import torch
    allp, off = capi.pack_scans(scans, width=width)
    d_raw, d_off = to_dev(allp), to_dev(off.astype(np.int64))
    d_out = torch.full((len(allp) + 1, 2), float(SENTINEL), dtype=torch.float32, device=d_raw.device)
    d_ooff = torch.full((len(scans) + 1,), 7, dtype=torch.int64, device=d_raw.device)
    sync()
    ctx.prefilter_batch_dev(d_raw.data_ptr(), 4 * width, d_off.data_ptr(), len(scans), len(allp), leaf, d_out.data_ptr(),
                            d_ooff.data_ptr())
    sync()
    ooff, out = d_ooff.cpu().numpy(), d_out.cpu().numpy()
    return [out[int(ooff[b]):int(ooff[b + 1])] for b in range(len(scans))], ooff, out


def batch_on_host(capi, ctx, scans, leaf, width=2):
    """ndt_prefilter_batch through ctypes -> (filtered scans, offsets, the whole output buffer)."""
    allp, off = capi.pack_scans(scans, width=width)
    out = np.full((len(allp) + 1, 2), SENTINEL)
    ooff = np.full(len(scans) + 1, 7, np.uint64)
    ctx.check(capi.lib().ndt_prefilter_batch(ctx.h, allp.ctypes.data, 4 * width, off.ctypes.data, len(scans), ctypes.c_float(leaf),
                                             out.ctypes.data, ooff.ctypes.data), "ndt_prefilter_batch")
    return [out[int(ooff[b]):int(ooff[b + 1])] for b in range(len(scans))], ooff, out


def check_batch(oracle, scans, leaf, got, ooff, out):
    """Every scan its single-scan reference, the offsets their running count, the sentinel behind the total untouched."""
    want = [reference(oracle, s, leaf) for s in scans]
    want_off = np.concatenate([[0], np.cumsum([len(w) for w in want])])
    assert np.array_equal(ooff.astype(np.int64), want_off)
    for b, (g, w) in enumerate(zip(got, want)):
        assert same_bits(g, w), b
    assert np.all(out[int(want_off[-1]):] == SENTINEL)
    return want


# ---- every family down every path ----
CASES = [(f, n) for f in sorted(W.FAMILIES) for n in W.SORTED_LENGTHS + W.EIGHT_WAVE_LENGTHS] + \
        [(f, n) for f in W.LONG_FAMILIES for n in W.LONG_LENGTHS]


@pytest.mark.parametrize("family,n", CASES, ids=["%s-%d" % c for c in CASES])
def test_family_matches_oracle_bit_for_bit(gpu, oracle, family, n):
    capi, ctx = gpu
    make, leaf = W.FAMILIES[family]
    cloud = make(n)
    assert same_bits(ctx.prefilter(cloud, leaf), oracle.approx_voxel_filter(cloud, leaf))


def test_one_voxel_summed_over_three_tiles(gpu, oracle):
    capi, ctx = gpu
    cloud = W.no_flush(20000, V=1)
    ref = oracle.approx_voxel_filter(cloud, 0.05)
    assert ref.shape == (1, 2) and same_bits(ctx.prefilter(cloud, 0.05), ref)


@pytest.mark.parametrize("tail", [False, True], ids=["parked_65534", "tail_65535"])
def test_count_limits_of_the_parked_flush(gpu, oracle, tail):
    capi, ctx = gpu
    cloud = W.count_limit(tail)
    ref = oracle.approx_voxel_filter(cloud, 0.05)
    assert len(cloud) == W.SORT_MAX and len(ref) == (1 if tail else 2)
    assert same_bits(ctx.prefilter(cloud, 0.05), ref)


# ---- stride 16: the reference's own pcl::PointXYZ layout ----
@pytest.mark.parametrize("n", [5000, 66113])
def test_stride_16_is_byte_identical_to_stride_8(gpu, oracle, n):
    capi, ctx = gpu
    make, leaf = W.FAMILIES["one_wave"]
    cloud = make(n)
    wide = np.full((n, 4), np.nan, np.float32)
    wide[:, :2] = cloud
    ref = oracle.approx_voxel_filter(cloud, leaf)
    narrow = ctx.prefilter(cloud, leaf)
    assert same_bits(narrow, ref)
    out = np.full((n, 2), SENTINEL)
    m = ctypes.c_size_t()
    ctx.check(capi.lib().ndt_prefilter(ctx.h, wide.ctypes.data, n, 16, ctypes.c_float(leaf), out.ctypes.data, ctypes.byref(m)),
              "ndt_prefilter")
    assert same_bits(out[:m.value], narrow)
    other = W.eight_slots(777, leaf=leaf)
    wide_other = np.full((777, 4), np.nan, np.float32)
    wide_other[:, :2] = other
    want = [reference(oracle, other, leaf), ref, EMPTY, reference(oracle, other, leaf)]
    for call in (batch_on_host, batch_on_device):
        got, ooff, out = call(capi, ctx, [wide_other, wide, np.zeros((0, 4), np.float32), wide_other], leaf, width=4)
        assert all(same_bits(g, w) for g, w in zip(got, want)), call.__name__
        assert np.all(out[int(ooff[-1]):] == SENTINEL)


# ---- the second scan of a workgroup ----
def test_second_round_of_the_workgroups(gpu, oracle):
    """More scans than workgroups: scan b + G starts from what scan b left in the workgroup -- slots, per-wave mask words,
    queues, flush bitmap, output count -- unless every one of them is reset.  Both kernels: tiny scans everywhere, two long
    ones on workgroup 5."""
    import torch
    capi, ctx = gpu
    G = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    scans = W.second_round_batch(G)
    B = len(scans)
    assert B == G + 100 and B > G
    assert len(scans[5]) == len(scans[5 + G]) == W.SECOND_ROUND_LONG > W.SORT_MAX
    got, ooff, out = batch_on_device(capi, ctx, scans, W.SECOND_ROUND_LEAF)
    want = check_batch(oracle, scans, W.SECOND_ROUND_LEAF, got, ooff, out)
    assert sum(len(w) for w in want[G:]) > 0 and any(len(w) == 0 for w in want[G:])


# ---- the second step of the pack kernel's loop over gridDim.y ----
def test_second_step_of_the_pack_loop(gpu, oracle):
    capi, ctx = gpu
    rng = np.random.default_rng(65538)
    B = 65538
    sizes = rng.integers(1, 4, B)
    sizes[[0, 2, 65533, 65534, 65535, 65537]] = 0                       # empty scans on both sides of index 65535
    pts = (rng.normal(size=(int(sizes.sum()), 2)) * 3.0).astype(np.float32)
    scans = np.split(pts, np.cumsum(sizes)[:-1])
    got, ooff, out = batch_on_host(capi, ctx, scans, 0.05)
    want = check_batch(oracle, scans, 0.05, got, ooff, out)
    assert len(want[65536]) > 0 and int(ooff[65535]) < int(ooff[B])


# ---- a scan's result does not depend on where it stands ----
def test_position_independence(gpu, oracle):
    capi, ctx = gpu
    leaf = 0.05
    a, c = W.one_slot(3000, K=5, run=1, leaf=leaf), W.no_flush(3000, leaf=leaf)
    long_scan = W.one_wave(66113, leaf=leaf)
    ra, rc, rl = (reference(oracle, s, leaf) for s in (a, c, long_scan))
    assert same_bits(ctx.prefilter(a, leaf), ra) and same_bits(ctx.prefilter(c, leaf), rc)
    batch = [a, c, long_scan, a, EMPTY, c, a[:1], c, a]
    want = [ra, rc, rl, ra, EMPTY, rc, a[:1], rc, ra]
    for call in (batch_on_host, batch_on_device):
        got, ooff, out = call(capi, ctx, batch, leaf)
        assert all(same_bits(g, w) for g, w in zip(got, want)), call.__name__
        assert np.all(out[int(ooff[-1]):] == SENTINEL)


# ---- a scan the reference leaves undefined stays inside its bounds and leaves the others alone ----
@pytest.mark.parametrize("n2", [500, 66113], ids=["by_slot", "step_by_step"])
def test_an_undefined_scan_is_isolated(gpu, oracle, n2):
    """Scan 2 holds NaN, +-Inf, +-3e38 and finite coordinates with |x / leaf| >= 2^31: (int)floorf() of those has no defined
    value in the reference.  Nothing is asserted about scan 2's values (include/ndt_mi355x.h, ndt_prefilter)."""
    capi, ctx = gpu
    leaf = 0.05
    rng = np.random.default_rng(n2)
    clean = [W.one_wave(900, leaf=leaf), W.one_slot(66113, K=5, run=3, leaf=leaf), W.eight_slots(n2, leaf=leaf),
             W.no_flush(700, leaf=leaf), W.tile_edges(8193, leaf=leaf)]
    bad = clean[2].copy()
    poison = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 2.0 ** 31 * leaf, -(2.0 ** 31) * leaf, 2.2e8, -2.2e8, 1e30],
                      np.float32)
    assert np.all(~np.isfinite(poison) | (np.abs(poison.astype(np.float64) / leaf) >= 2.0 ** 31))
    at = rng.permutation(n2)[:200]
    bad[at, rng.integers(0, 2, 200)] = poison[rng.integers(0, len(poison), 200)]
    bad[[0, n2 - 1]] = [[np.nan, np.nan], [np.inf, -3e38]]
    dirty = clean[:2] + [bad] + clean[3:]
    good, good_off, _ = batch_on_device(capi, ctx, clean, leaf)
    got, ooff, out = batch_on_device(capi, ctx, dirty, leaf)
    again, ooff2, out2 = batch_on_device(capi, ctx, dirty, leaf)
    for b in (0, 1, 3, 4):
        assert same_bits(got[b], good[b]) and same_bits(got[b], reference(oracle, clean[b], leaf)), b
    assert np.all(np.diff(ooff) >= 0) and 1 <= len(got[2]) <= n2
    assert np.all(out[int(ooff[-1]):] == SENTINEL)
    assert np.array_equal(ooff, ooff2) and out.tobytes() == out2.tobytes()
