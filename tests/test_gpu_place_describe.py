"""place_describe_kernel held to the host definition (ndt_place_describe) and to the numpy restatement of
tests/place_helpers.py, byte for byte, on every boundary of the descriptor's rules."""
import numpy as np
import pytest

import place_helpers as H
from gpu_support import gpu, sync, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu


def check(capi, ctx, clouds, centres, cloud_of, p, strides=(8, 16)):
    """The batch on the device at every stride against both references; returns the descriptors."""
    ref = np.stack([H.describe_ref(clouds[c], centres[k], p) for k, c in enumerate(cloud_of)])
    host = np.stack([capi.place_describe(clouds[c], centres[k], p) for k, c in enumerate(cloud_of)])
    assert host.tobytes() == ref.tobytes()
    for stride in strides:
        got = capi.place_describe_batch(ctx, clouds, centres, cloud_of, p, stride=stride)
        assert got.dtype == np.uint64 and got.shape == ref.shape and got.tobytes() == ref.tobytes(), stride
    return ref


@pytest.mark.parametrize("centre", H.CENTRES)
@pytest.mark.parametrize("n_rings,width,r_min", [(1, 0.5, 0.25), (20, 0.5, 0.25), (32, 0.37, 0.0), (20, 0.5, 1.0)])
def test_boundaries(gpu, centre, n_rings, width, r_min):
    capi, ctx = gpu
    p = capi.default_place_params(n_rings=n_rings, ring_width=width, r_min=r_min)
    xy = H.cloud_about(H.boundary_points(p, np.random.default_rng(5)), centre)
    perm = np.random.default_rng(6).permutation(len(xy))
    # the whole family, the same points permuted, and 300 of its points each as a cloud of its own: a point's own cell
    pick = np.random.default_rng(7).choice(len(xy), 300, replace=False)
    clouds = [xy, xy[perm]] + [xy[k:k + 1] for k in pick]
    d = check(capi, ctx, clouds, [centre] * len(clouds), list(range(len(clouds))), p)
    assert d[0].tobytes() == d[1].tobytes()                                          # permuting the points changes no byte


def test_exact_edges_and_degenerate_clouds(gpu):
    capi, ctx = gpu
    p = capi.default_place_params()
    f = np.float32
    clouds = [np.array([[1.5, 2.0]], f), np.array([[np.nextafter(f(1.5), f(0)), 2.0]], f), np.array([[10.0, 0.0]], f),
              np.array([[np.nextafter(f(10), f(0)), 0.0]], f), np.array([[0.25, 0.0]], f), np.array([[np.nextafter(f(0.25), f(0)), 0.0]], f),
              np.zeros((0, 2), f), np.zeros((1, 2), f), np.array([[np.nan, 1.0], [np.inf, 0.0], [1.0, -np.inf], [3e38, 3e38]], f)]
    d = check(capi, ctx, clouds, [(0.0, 0.0)] * len(clouds), list(range(len(clouds))), p)
    assert [np.flatnonzero(x).tolist() for x in d] == [[5], [4], [], [19], [0], [], [], [], []]
    q = capi.default_place_params(r_min=0.0)
    assert check(capi, ctx, clouds[7:8], [(0.0, 0.0)], [0], q)[0, 0] == 1 << 7       # a point at the centre


@pytest.mark.parametrize("min_pts", [1, 2, 3])
def test_min_pts_and_a_crowded_cell(gpu, min_pts):
    capi, ctx = gpu
    p = capi.default_place_params(min_pts=min_pts)
    rng = np.random.default_rng(min_pts)
    a = np.array([[1.1, 0.3]], np.float32).repeat(min_pts - 1, axis=0)               # a cell one point short
    b = np.array([[-2.2, 1.4]], np.float32).repeat(min_pts, axis=0)                  # a cell with exactly enough
    c = (np.array([[3.3, -3.1]]) + rng.uniform(-0.01, 0.01, (3000, 2))).astype(np.float32)     # 3 000 points in one cell
    d = check(capi, ctx, [np.concatenate([a, b, c])], [(0.0, 0.0)], [0], p)
    assert H.popcount(d).sum() == 2


def hall(rng, n):
    """n points on the walls of a 24 x 16 m rectangle and a few pillars: a cloud with structure in every ring."""
    t = rng.uniform(0, 1, n)
    side = rng.integers(0, 4, n)
    x = np.where(side == 0, 24 * t, np.where(side == 1, 24 * t, np.where(side == 2, 0.0, 24.0)))
    y = np.where(side == 0, 0.0, np.where(side == 1, 16.0, 16 * t))
    return np.stack([x, y], axis=1).astype(np.float32) + rng.normal(0, 0.01, (n, 2)).astype(np.float32)


def test_many_centres_many_clouds_and_alone(gpu):
    capi, ctx = gpu
    rng = np.random.default_rng(21)
    p = capi.default_place_params()
    big = hall(rng, 5000)
    centres = rng.uniform([1, 1], [23, 15], (300, 2))
    d = check(capi, ctx, [big], centres, [0] * 300, p, strides=(8,))                 # 300 centres on one cloud
    assert len(set(x.tobytes() for x in d)) > 250
    clouds = [hall(rng, int(n)) for n in rng.integers(0, 400, 257)]                  # 257 clouds in one call, empty ones among them
    clouds[3] = np.zeros((0, 2), np.float32)
    cs = rng.uniform([1, 1], [23, 15], (257, 2))
    d = check(capi, ctx, clouds, cs, list(range(257)), p, strides=(16,))
    for k in (0, 3, 100, 256):                                                       # a descriptor alone = the same one in the batch
        assert capi.place_describe_batch(ctx, [clouds[k]], cs[k:k + 1], [0], p).tobytes() == d[k].tobytes()
    # several centres naming clouds in any order, with an option that changes the grid
    order = rng.integers(0, 257, 500)
    cs2 = rng.uniform([1, 1], [23, 15], (500, 2))
    want = capi.place_describe_batch(ctx, clouds, cs2, order, p)
    ctx.set_option(capi.OPT_WORKGROUPS, 1)
    try:
        assert capi.place_describe_batch(ctx, clouds, cs2, order, p).tobytes() == want.tobytes()
    finally:
        ctx.set_option(capi.OPT_WORKGROUPS, 0)
    assert want.tobytes() == np.stack([H.describe_ref(clouds[c], cs2[k], p) for k, c in enumerate(order)]).tobytes()


def test_device_form(gpu):
    """ndt_place_describe_batch_dev on the caller's buffers: clouds in the middle of a larger array, a non-zero first offset."""
    import torch
    capi, ctx = gpu
    rng = np.random.default_rng(22)
    p = capi.default_place_params(n_rings=32)
    clouds = [hall(rng, 700), np.zeros((0, 2), np.float32), hall(rng, 1300)]
    pts, off = capi.pack_scans([hall(rng, 50)] + clouds)
    d_xy = to_dev(pts)
    centres, cloud_of = rng.uniform([1, 1], [23, 15], (40, 2)), rng.integers(0, 3, 40)
    d_desc = torch.full((40, 32), -1, dtype=torch.int64, device=d_xy.device)
    sync()
    capi.place_describe_batch_dev(ctx, d_xy.data_ptr(), 8, off[1:], centres, cloud_of, p, d_desc.data_ptr())
    sync()
    got = d_desc.cpu().numpy().view(np.uint64)
    assert got.tobytes() == np.stack([H.describe_ref(clouds[c], centres[k], p) for k, c in enumerate(cloud_of)]).tobytes()


def test_refusals_with_a_context(gpu):
    capi, ctx = gpu
    p = capi.default_place_params()
    xy = [np.ones((3, 2), np.float32)]
    for kw, word in ((dict(n_rings=33), "n_rings"), (dict(ring_width=-1.0), "ring_width"), (dict(min_pts=0), "min_pts")):
        with pytest.raises(capi.NdtError, match=word):
            capi.place_describe_batch(ctx, xy, [(0.0, 0.0)], [0], capi.default_place_params(**kw))
    with pytest.raises(capi.NdtError, match="cloud_of"):
        capi.place_describe_batch(ctx, xy, [(0.0, 0.0)], [1], p)
    with pytest.raises(capi.NdtError, match="centre"):
        capi.place_describe_batch(ctx, xy, [(np.inf, 0.0)], [0], p)
    with pytest.raises(capi.NdtError, match="stride_bytes"):
        capi.place_describe_batch_dev(ctx, 256, 12, [0, 3], [(0.0, 0.0)], [0], p, 256)
    assert capi.place_describe_batch(ctx, xy, np.zeros((0, 2)), [], p).shape == (0, 20)          # nothing to do
