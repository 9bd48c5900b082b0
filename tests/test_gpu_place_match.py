"""place_match_kernel and place_pick_kernel held to the host definition (ndt_place_match_host) and to the numpy restatement of
tests/place_helpers.py: out, n_out and table byte for byte."""
import numpy as np
import pytest

import place_helpers as H
from gpu_support import gpu, sync, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def check(capi, ctx, q, qg, d, first, group, p, numpy_too=True):
    """The device against the host definition (and the restatement); returns the device's (hits, n, table)."""
    got = capi.place_match(ctx, q, qg, d, first, group, p)
    assert same(got, capi.place_match_host(q, qg, d, first, group, p))
    if numpy_too:
        assert same(got, H.match_ref(capi, q, qg, d, first, group, p))
    return got


@pytest.mark.parametrize("n_rings", [1, 8, 9, 20, 24, 25, 32])
def test_rotations_and_ragged_items(gpu, n_rings):
    capi, ctx = gpu
    rng = np.random.default_rng(n_rings)
    p = capi.default_place_params(n_rings=n_rings, top_k=4)
    base = H.random_desc(rng, 1, n_rings)[0]
    rot = np.stack([H.rotl(base, s) for s in range(64)])                             # a descriptor's own 64 rotations, one item each
    hits, n, table = check(capi, ctx, base[None], [-1], rot, np.arange(65), np.ones(64), capi.default_place_params(n_rings=n_rings, top_k=16))
    assert n[0] == 16 and hits[0]["key"].tolist() == [65536] * 16 and hits[0]["item"].tolist() == list(range(16))
    assert hits[0]["shift"].tolist() == [(64 - s) % 64 for s in range(16)]
    # items of 0, 3, 1, 300 (more than one stage of entries), 0 and 36 descriptors, with zero and repeated descriptors among them
    d = H.random_desc(rng, 340, n_rings)
    d[7] = 0
    d[9] = d[8]
    d[200] = d[100]
    first = np.array([0, 0, 3, 4, 304, 304, 340], np.int32)
    group = np.array([0, 1, 0, 2, 2, -1], np.int32)
    q = np.stack([H.rotl(d[2], 17), d[8], np.zeros(n_rings, np.uint64), H.random_desc(rng, 1, n_rings)[0], H.rotl(d[100], 63)])
    hits, n, table = check(capi, ctx, q, [0, -1, 2, 1, -1], d, first, group, p)
    assert n[2] == 0 and not hits[2].view(np.uint8).any()                            # the all-zero query
    assert hits[4, 0]["desc"] == 100 and hits[4, 0]["key"] == 65536                  # equal descriptors inside an item: the lower index
    assert table[0, 0] == 0 and table[0, 2] == 0 and table[0, 4] == 0                # no descriptor / own group / no descriptor


def test_ties_and_zero(gpu):
    capi, ctx = gpu
    p = capi.default_place_params(top_k=16)
    full, zero = np.full((2, 20), ~np.uint64(0)), np.zeros((2, 20), np.uint64)
    h, n, t = check(capi, ctx, full[:1], [-1], full, [0, 1, 2], [5, 5], p)           # every shift ties: shift 0; two equal items: the lower first
    assert n[0] == 2 and h[0, :2]["shift"].tolist() == [0, 0] and h[0, :2]["item"].tolist() == [0, 1]
    h, n, t = check(capi, ctx, full[:1], [5], full, [0, 1, 2], [5, 6], p)            # own-group exclusion
    assert n[0] == 1 and h[0, 0]["item"] == 1 and t[0, 0] == 0
    for q, d in ((zero, full), (full, zero), (zero, zero)):                          # all-zero query, entry, both: key 0, nothing returned
        h, n, t = check(capi, ctx, q[:1], [-1], d, [0, 1, 2], [1, 2], p)
        assert n[0] == 0 and (t >> np.uint64(32)).max() == 0 and t[0, 1] == 0xFFFFFFFF - (1 << 6) and not h.view(np.uint8).any()


def test_min_key_and_top_k(gpu):
    capi, ctx = gpu
    rng = np.random.default_rng(31)
    d, q = H.random_desc(rng, 6, 20), H.random_desc(rng, 1, 20)
    h, n, t = check(capi, ctx, q, [-1], d, np.arange(7), np.zeros(6, int), capi.default_place_params(top_k=16))
    keys = sorted((t[0] >> np.uint64(32)).tolist(), reverse=True)
    assert n[0] == 6 and h[0, :6]["key"].tolist() == keys and not h[0, 6:].view(np.uint8).any()       # fewer eligible items than top_k
    for mk, want in ((keys[2], sum(v >= keys[2] for v in keys)), (keys[2] + 1, sum(v > keys[2] for v in keys))):
        assert check(capi, ctx, q, [-1], d, np.arange(7), np.zeros(6, int), capi.default_place_params(top_k=16, min_key=mk))[1][0] == want
    for top_k in (1, 4, 16):
        assert check(capi, ctx, q, [-1], d, np.arange(7), np.zeros(6, int), capi.default_place_params(top_k=top_k))[1][0] == min(top_k, 6)


def related(rng, n_q, n_desc, n_rings):
    """Entries, and queries that are rotated, thinned copies of some of them (so that keys spread) or unrelated."""
    d = H.random_desc(rng, n_desc, n_rings)
    src, s = rng.integers(0, n_desc, n_q), rng.integers(0, 64, n_q)
    q = np.stack([H.rotl(d[a], b) for a, b in zip(src, s)]) & H.random_desc(rng, n_q, n_rings, density=0.8)
    return q, d


@pytest.mark.parametrize("n_q,n_items", [(1, 1), (1, 1000), (257, 1), (257, 1000)])
def test_sizes(gpu, n_q, n_items):
    capi, ctx = gpu
    rng = np.random.default_rng(n_q + n_items)
    p = capi.default_place_params(top_k=4)
    per = rng.integers(0, 4, n_items)
    per[0] = 3
    first = np.concatenate([[0], np.cumsum(per)]).astype(np.int32)
    q, d = related(rng, n_q, max(int(first[-1]), 1), 20)
    group, qg = rng.integers(0, 5, n_items), rng.integers(-1, 5, n_q)
    got = check(capi, ctx, q, qg, d, first, group, p, numpy_too=n_q == 1 or n_items == 1)
    # a query alone = the same query in the batch; the grid does not change a byte
    for k in sorted({0, n_q // 2, n_q - 1}):
        alone = capi.place_match(ctx, q[k:k + 1], qg[k:k + 1], d, first, group, p)
        assert same(alone, [x[k:k + 1] for x in got])
    ctx.set_option(capi.OPT_WORKGROUPS, 1)
    try:
        assert same(capi.place_match(ctx, q, qg, d, first, group, p), got)
    finally:
        ctx.set_option(capi.OPT_WORKGROUPS, 0)


def test_device_form_without_a_table(gpu):
    import torch
    capi, ctx = gpu
    rng = np.random.default_rng(41)
    p = capi.default_place_params(top_k=4)
    q, d = related(rng, 9, 150, 20)
    first, group, qg = np.arange(0, 151, 3), rng.integers(0, 3, 50), rng.integers(-1, 3, 9)
    d_q, d_d = to_dev(q.view(np.int64)), to_dev(d.view(np.int64))
    want = capi.place_match_host(q, qg, d, first, group, p)
    for with_table in (False, True):
        d_out = torch.full((9 * 4 * 8,), -1, dtype=torch.int32, device=d_q.device)
        d_n = torch.full((9,), -1, dtype=torch.int32, device=d_q.device)
        d_t = torch.full((9, 50), -1, dtype=torch.int64, device=d_q.device)
        sync()
        capi.place_match_dev(ctx, d_q.data_ptr(), qg, d_d.data_ptr(), first, group, p, d_out.data_ptr(), d_n.data_ptr(),
                             d_t.data_ptr() if with_table else None)
        sync()
        assert d_out.cpu().numpy().tobytes() == want[0].tobytes() and d_n.cpu().numpy().tobytes() == want[1].tobytes()
        assert not with_table or d_t.cpu().numpy().tobytes() == want[2].tobytes()


def test_refusals_with_a_context(gpu):
    capi, ctx = gpu
    d = np.zeros((2, 20), np.uint64)
    for kw, word in ((dict(top_k=17), "top_k"), (dict(min_key=0), "min_key"), (dict(ring_width=0.0), "ring_width")):
        with pytest.raises(capi.NdtError, match=word):
            capi.place_match(ctx, d[:1], [-1], d.reshape(-1), [0, 1], [0], capi.default_place_params(**kw))
    p = capi.default_place_params()
    with pytest.raises(capi.NdtError, match="decreases"):
        capi.place_match(ctx, d[:1], [-1], d, [0, 2, 1], [0, 0], p)
    h, n, t = capi.place_match(ctx, d[:1], [-1], d[:0], [0], [], p)                  # no item: nothing returned
    assert n[0] == 0 and not h.view(np.uint8).any() and t.shape == (1, 0)
