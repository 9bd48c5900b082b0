"""The second round of every one-workgroup offsets scan (block_excl_offsets, ndt_common.hip.h): inputs with more items than
the workgroup has threads, so that the carry of the first round is used.  Each result is held to the oracle its neighbours in
the suite use, for equal bytes and equal order; the shapes are the smallest that get there (LOG R26 has the table)."""
import ctypes

import numpy as np
import pytest

import occ_helpers as H
from local_map_helpers import host_call, oracle_local_map, room_scans
from ndt_slam_amd import replay
from test_gpu_occupancy import centre, check
from test_gpu_resample import resample_on_device
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu
EMPTY = np.zeros((0, 2), np.float32)
LEAF = 0.05


def test_prefilter_batch_of_1100_tiny_scans(gpu, oracle):
    """prefilter_offsets_kernel<false>: 1100 counts, two rounds of 1024."""
    capi, ctx = gpu
    rng = np.random.default_rng(1100)
    sizes = rng.integers(1, 4, 1100)
    sizes[[0, 5, 1023, 1024, 1099]] = 0                                       # empty scans, on both sides of the round's end
    scans = [(rng.normal(size=(int(n), 2)) * 3.0).astype(np.float32) for n in sizes]
    B = len(scans)
    allp, off = capi.pack_scans(scans)
    out = np.full((len(allp) + 1, 2), np.float32(-777.0))
    ooff = np.full(B + 1, 7, np.uint64)
    ctx.check(capi.lib().ndt_prefilter_batch(ctx.h, allp.ctypes.data, 8, off.ctypes.data, B, ctypes.c_float(LEAF), out.ctypes.data,
                                             ooff.ctypes.data), "ndt_prefilter_batch")
    want = [oracle.approx_voxel_filter(x, LEAF).reshape(-1, 2) if len(x) else EMPTY for x in scans]
    want_off = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint64)
    assert np.array_equal(ooff, want_off)
    assert want_off[1024] > 0 and want_off[B] > want_off[1024]                # a carry, and items behind it
    assert out[:int(want_off[B])].tobytes() == np.concatenate(want).tobytes()
    assert np.all(out[int(want_off[B]):] == np.float32(-777.0))


def test_remove_neighbors_with_more_than_1024_blocks(gpu, oracle):
    """make_map_sub_offsets_kernel through ndt_remove_neighbors: 1025 units of 256 base points in its one submap."""
    capi, ctx = gpu
    rng = np.random.default_rng(262145)
    nb = 262145 + 7
    assert (nb + 255) // 256 > 1024
    base = rng.uniform(-40, 40, (nb, 2)).astype(np.float32)
    at = np.array([0, 1, 255, 256, 70000, 131071, 200000, 262143, 262144, 262150, nb - 1])    # hits in both rounds
    lst = np.concatenate([base[at] + np.float32(0.01), rng.uniform(50, 60, (5, 2)).astype(np.float32)]).astype(np.float32)
    d = np.sqrt(((base[:, None, :] - lst[None, :, :]) ** 2).sum(-1, dtype=np.float32), dtype=np.float32)
    keep = ~(d.astype(np.float64) < 0.1).any(1)
    assert not keep[at].any() and len(at) <= (~keep).sum() < 2000
    got = ctx.remove_neighbors(base, lst, 0.1)
    assert got.shape == base[keep].shape and got.tobytes() == base[keep].tobytes()
    assert got.tobytes() == oracle.remove_neighbors(base, lst, 0.1).tobytes()


@pytest.fixture(scope="module")
def big_submap(oracle):
    """Four scans of about 72 000 points with a moving object: a result of more than 262 144 points, more than 1024 units."""
    scans = room_scans(np.random.default_rng(262144), 4, 80000, 300)
    item = (scans, True, True, True, 0.05, 0.1, None)
    ref = np.ascontiguousarray(oracle.make_map(*item[:6]), np.float32).reshape(-1, 2)
    assert 262144 < len(ref) < sum(len(s) for s in scans)                     # something was removed
    return item, ref


def test_make_map_of_more_than_1024_units(gpu, big_submap):
    """make_map_sub_offsets_kernel through ndt_make_map: the one submap of a single call (no second level)."""
    capi, ctx = gpu
    item, ref = big_submap
    got = ctx.make_map(*item[:6])
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes()


def test_local_maps_item_of_more_than_1024_units(gpu, oracle, big_submap):
    """make_map_sub_offsets_kernel with a second level behind it: the same submap as one item of a batched call, a small one on either side."""
    capi, ctx = gpu
    item, ref = big_submap
    small = (room_scans(np.random.default_rng(5), 4, 300, 15), True, True, True, 0.05, 0.1, None)
    small_ref = np.ascontiguousarray(oracle.make_map(*small[:6]), np.float32).reshape(-1, 2)
    rc, clouds, targets, status = host_call(capi, ctx, [small, item, small], -1.0, want_target=False)
    assert rc == 0 and targets is None and not status.any()
    for got, want in zip(clouds, (small_ref, ref, small_ref)):
        assert got.shape == want.shape and got.tobytes() == want.tobytes()


def test_local_maps_of_1100_tiny_submaps(gpu, oracle):
    """make_map_sub_scan_kernel and prefilter_offsets_kernel<true>: 1100 submaps of two 3-point scans, some behind a previous
    cloud; per item the oracle's make_map, then its prefilter behind the previous cloud."""
    capi, ctx = gpu
    rng = np.random.default_rng(1101)
    items = []
    for s in range(1100):
        scans = [(rng.normal(size=(3, 2)) * 4.0).astype(np.float32) for _ in range(2)]
        prev = (rng.normal(size=(1 + s % 4, 2)) * 4.0).astype(np.float32) if s % 3 == 0 else None
        items.append((scans, s % 2 == 0, s % 7 != 0, s % 5 != 0, 0.05, 0.1, prev))
    want = [oracle_local_map(oracle, it, LEAF) for it in items]
    assert len({len(w[0]) for w in want}) >= 3                                # clouds of 0, 3 and 6 points
    rc, clouds, targets, status = host_call(capi, ctx, items, LEAF)
    assert rc == 0 and not status.any()
    for s, (p_cloud, target, n_prev) in enumerate(want):
        assert clouds[s].shape == p_cloud.shape and clouds[s].tobytes() == p_cloud.tobytes(), (s, "cloud")
        assert targets[s].shape == target.shape and targets[s].tobytes() == target.tobytes(), (s, "target")
    assert sum(len(c) for c in clouds[1024:]) > 0 and sum(len(t) for t in targets[1024:]) > 0


def test_resample_batch_of_1100_tiny_scans(gpu):
    """resample_offsets_kernel: 1100 totals and statuses; one scan is not finite."""
    capi, ctx = gpu
    rng = np.random.default_rng(1102)
    scans = [np.cumsum(rng.uniform(0.01, 0.2, (3, 2)), axis=0) + rng.normal(size=2) for _ in range(1100)]
    bad = 1030
    scans[bad] = scans[bad].copy(); scans[bad][1, 0] = np.nan
    r64, r32, oo, st = resample_on_device(capi, ctx, scans, 0.05, 0.25)
    assert st[bad] == capi.NDT_E_ARG and not np.delete(st, bad).any() and oo[bad + 1] == oo[bad]
    n_ref = 0
    for b, s in enumerate(scans):
        assert oo[b] == n_ref, b
        if b == bad:
            continue
        ref = replay.resample_points(s, 0.05, 0.25)
        n_ref += len(ref)
        assert r64[b].shape == ref.shape and np.array_equal(r64[b].view(np.uint64), ref.view(np.uint64)), b
        assert np.array_equal(r32[b].view(np.uint32), ref.astype(np.float32).view(np.uint32)), b
    assert oo[-1] == n_ref and oo[1024] > 0


def test_occ_integrate_of_300_scans(gpu):
    """occ_jobs_kernel: more scans than its 256 threads, two beams each, a few scans empty."""
    g = H.Geometry(0.0, 0.0, 0.25, 120, 90)
    rng = np.random.default_rng(300)
    scans, origins = [], []
    for s in range(300):
        n = 0 if s in (3, 255, 256) else 2
        scans.append(centre(g, rng.integers(-3, 124, size=n), rng.integers(-3, 94, size=n)))
        origins.append(centre(g, rng.integers(0, 120), rng.integers(0, 90))[0].astype(np.float64))
    want, st = check(gpu, [g], scans, np.array(origins), what="300 scans")
    assert st["n_beams"] == 2 * 297 and st["n_skipped"] == 0 and want[0][0].sum() > 0
