"""The host definitions of the place section (ndt_place_describe, ndt_place_key, ndt_place_match_host) held to the numpy
restatement of tests/place_helpers.py, bit for bit, on the families the device tests use, and every refusal.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import place_helpers as H


@pytest.fixture(scope="module")
def capi():
    from ndt_slam_amd import build, capi
    build.build()
    return capi


def params(capi, **kw):
    return capi.default_place_params(**kw)


def test_defaults_and_layout(capi):
    p = params(capi)
    assert (p.ring_width, p.r_min, p.n_rings, p.min_pts, p.min_key, p.top_k, p.centre_stride, p.reserved) == (0.5, 0.25, 20, 1, 1, 4, 1, 0)
    assert C.sizeof(capi.PlaceParams) == 40 and C.sizeof(capi.PlaceHit) == 32 and C.sizeof(capi.PlaceCandidate) == 64
    assert capi.PLACE_HIT_DTYPE.itemsize == 32 and capi.PLACE_CANDIDATE_DTYPE.itemsize == 64


@pytest.mark.parametrize("centre", H.CENTRES)
@pytest.mark.parametrize("n_rings,width,r_min", [(1, 0.5, 0.25), (20, 0.5, 0.25), (32, 0.37, 0.0), (20, 0.5, 1.0)])
def test_describe_boundaries(capi, centre, n_rings, width, r_min):
    p = params(capi, n_rings=n_rings, ring_width=width, r_min=r_min)
    xy = H.cloud_about(H.boundary_points(p, np.random.default_rng(5)), centre)
    keep, ring, sector = H.cells_ref(xy, centre, p)
    assert keep.sum() > 50
    if (n_rings, r_min) == (20, 0.25):                     # (with the default geometry the families reach every ring and every sector)
        assert set(sector[keep]) == set(range(64)) and set(ring[keep]) == set(range(n_rings))
    ref = H.describe_ref(xy, centre, p)
    for stride in (8, 16):
        assert capi.place_describe(xy, centre, p, stride=stride).tobytes() == ref.tobytes()
    perm = np.random.default_rng(6).permutation(len(xy))
    assert capi.place_describe(xy[perm], centre, p).tobytes() == ref.tobytes()
    # every point on its own: the cell of each point, not only the union
    for k in np.random.default_rng(7).choice(len(xy), 150, replace=False):
        assert capi.place_describe(xy[k:k + 1], centre, p).tobytes() == H.describe_ref(xy[k:k + 1], centre, p).tobytes(), xy[k]


def test_describe_exact_edges(capi):
    p = params(capi)                                       # width 0.5: (1.5, 2.0) has r2 = 6.25 = edge2[5] exactly -> ring 5
    d = capi.place_describe(np.array([[1.5, 2.0]], np.float32), (0.0, 0.0), p)
    assert np.flatnonzero(d).tolist() == [5] and d.tobytes() == H.describe_ref([[1.5, 2.0]], (0.0, 0.0), p).tobytes()
    below = np.array([[np.nextafter(np.float32(1.5), np.float32(0)), 2.0]], np.float32)
    assert np.flatnonzero(capi.place_describe(below, (0.0, 0.0), p)).tolist() == [4]
    assert not capi.place_describe(np.array([[10.0, 0.0]], np.float32), (0.0, 0.0), p).any()          # the outer edge is outside
    assert capi.place_describe(np.array([[np.nextafter(np.float32(10), np.float32(0)), 0.0]], np.float32), (0.0, 0.0), p)[19] == 1
    assert capi.place_describe(np.array([[0.25, 0.0]], np.float32), (0.0, 0.0), p)[0] == 1            # r_min itself counts
    assert not capi.place_describe(np.array([[np.nextafter(np.float32(0.25), np.float32(0)), 0.0]], np.float32), (0.0, 0.0), p).any()
    q = params(capi, r_min=0.0)
    assert capi.place_describe(np.zeros((1, 2), np.float32), (0.0, 0.0), q)[0] == 1 << 7              # the centre: a = b = 0, sub = 7
    assert not capi.place_describe(np.zeros((0, 2), np.float32), (0.0, 0.0), p).any()


@pytest.mark.parametrize("min_pts", [1, 2, 3])
def test_describe_min_pts(capi, min_pts):
    p = params(capi, min_pts=min_pts)
    rng = np.random.default_rng(min_pts)
    a = np.array([[1.1, 0.3]], np.float32).repeat(min_pts - 1, axis=0)               # a cell one point short
    b = np.array([[-2.2, 1.4]], np.float32).repeat(min_pts, axis=0)                  # a cell with exactly enough
    c = (np.array([[3.3, -3.1]]) + rng.uniform(-0.01, 0.01, (3000, 2))).astype(np.float32)     # a crowded cell
    xy = np.concatenate([a, b, c])
    got, ref = capi.place_describe(xy, (0.0, 0.0), p), H.describe_ref(xy, (0.0, 0.0), p)
    assert got.tobytes() == ref.tobytes() and H.popcount(got).sum() == 2


def test_key_and_match_against_numpy(capi):
    rng = np.random.default_rng(11)
    for n_rings in (1, 20, 32):
        p = params(capi, n_rings=n_rings, top_k=4)
        d = H.random_desc(rng, 40, n_rings)
        d[7] = 0
        d[9] = d[8]                                                                  # equal descriptors inside an item
        q = np.stack([H.rotl(d[3], 17), d[8], np.zeros(n_rings, np.uint64), H.random_desc(rng, 1, n_rings)[0]])
        for s in (0, 1, 17, 63):
            assert capi.place_key(q[0], d[3], s) == H.key_ref(q[0], d[3], s)[:2]
        assert capi.place_key(q[0], d[3], 17)[0] == 65536 and capi.place_key(q[2], d[7], 5) == (0, 0)
        first = np.array([0, 0, 3, 4, 12, 12, 40], np.int32)                         # items of 0, 3, 1, 8, 0 and 28 descriptors
        group = np.array([0, 1, 0, 2, 2, -1], np.int32)
        qg = np.array([0, -1, 2, 1], np.int32)
        got, ref = capi.place_match_host(q, qg, d, first, group, p), H.match_ref(capi, q, qg, d, first, group, p)
        for a, b in zip(got, ref):
            assert a.tobytes() == b.tobytes()
        assert got[1][2] == 0 and not got[0][2].view(np.uint8).any()                 # the all-zero query: nothing is returned


def test_match_rules(capi):
    rng = np.random.default_rng(12)
    p = params(capi, top_k=16)
    base = H.random_desc(rng, 1, 20)[0]
    rot = np.stack([H.rotl(base, s) for s in range(64)])                             # entry s = base rotated by s
    first, group = np.arange(65, dtype=np.int32), np.full(64, 1, np.int32)
    hits, n, table = capi.place_match_host(base[None], [-1], rot, first, group, params(capi, top_k=1))
    # query = rotl(entry, shift): entry s needs the shift 64 - s
    for s in (0, 1, 40, 63):
        h, k, _ = capi.place_match_host(base[None], [-1], rot[s:s + 1], [0, 1], [1], p)
        assert k[0] == 1 and h[0, 0]["key"] == 65536 and h[0, 0]["shift"] == (64 - s) % 64
    assert n[0] == 1 and hits[0, 0]["item"] == 0 and hits[0, 0]["key"] == 65536       # all 64 tie at 65536: the lower item wins
    full = np.full((2, 20), ~np.uint64(0))
    h, k, t = capi.place_match_host(full[:1], [-1], full, [0, 1, 2], [5, 5], p)      # every shift ties: shift 0; two equal items: the lower first
    assert k[0] == 2 and h[0, :2]["shift"].tolist() == [0, 0] and h[0, :2]["item"].tolist() == [0, 1] and h[0, :2]["key"].tolist() == [65536] * 2
    h, k, t = capi.place_match_host(full[:1], [-1], full, [0, 2], [5], p)            # equal descriptors inside an item: the lower index
    assert k[0] == 1 and h[0, 0]["desc"] == 0 and t[0, 0] == (65536 << 32) | 0xFFFFFFFF
    h, k, t = capi.place_match_host(full[:1], [5], full, [0, 1, 2], [5, 6], p)       # own-group exclusion
    assert k[0] == 1 and h[0, 0]["item"] == 1 and t[0, 0] == 0
    # min_key at a hit's key and one above it; fewer eligible items than top_k leave zero records
    d = H.random_desc(rng, 6, 20)
    q = H.random_desc(rng, 1, 20)
    h, k, t = capi.place_match_host(q, [-1], d, np.arange(7), np.zeros(6), p)
    keys = sorted((t[0] >> np.uint64(32)).tolist(), reverse=True)
    assert k[0] == 6 and h[0, :6]["key"].tolist() == keys and not h[0, 6:].view(np.uint8).any()
    for mk, want in ((keys[2], 3 + keys[3:].count(keys[2])), (keys[2] + 1, sum(v > keys[2] for v in keys))):
        h, k, _ = capi.place_match_host(q, [-1], d, np.arange(7), np.zeros(6), params(capi, top_k=16, min_key=mk))
        assert k[0] == want
    for top_k in (1, 4, 16):
        pk = params(capi, top_k=top_k)
        got, ref = capi.place_match_host(q, [-1], d, np.arange(7), np.zeros(6), pk), H.match_ref(capi, q, [-1], d, np.arange(7), np.zeros(6, int), pk)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, ref)) and got[1][0] == min(top_k, 6)


def test_key_rises_strictly_with_the_overlap():
    """What the device match relies on: for one (na + nb) the key of c + 1 exceeds the key of c, so the best shift of an entry
    is the one of largest overlap and equal keys mean equal overlaps."""
    for N in (1, 2, 3, 64, 1000, 2047, 2048, 4095, 4096):
        c = np.arange(0, min(N // 2, 2048) + 1, dtype=np.int64)
        key = (c * 65536) // (N - c)
        assert np.all(np.diff(key) > 0)


def test_refusals(capi):
    L, E = capi.lib(), capi.NDT_E_ARG
    xy = np.zeros((4, 2), np.float32)
    desc = np.zeros(32, np.uint64)

    def refused(rc, word):
        assert rc == E and word in L.ndt_last_error(None).decode(), (rc, L.ndt_last_error(None))

    for field, bad in (("ring_width", 0.0), ("ring_width", float("nan")), ("ring_width", float("inf")), ("r_min", -0.1), ("r_min", float("nan")),
                       ("n_rings", 0), ("n_rings", 33), ("min_pts", 0), ("min_key", 0), ("min_key", 65537), ("top_k", 0), ("top_k", 17),
                       ("centre_stride", 0), ("reserved", 1)):
        p = params(capi, **{field: bad})
        refused(L.ndt_place_describe(xy.ctypes.data, 4, 8, 0.0, 0.0, C.byref(p), desc.ctypes.data), field)
        out, n = np.zeros(16, capi.PLACE_HIT_DTYPE), np.zeros(1, np.int32)
        first, group = np.array([0, 1], np.int32), np.zeros(1, np.int32)
        refused(L.ndt_place_match_host(desc.ctypes.data, group.ctypes.data, 1, desc.ctypes.data, first.ctypes.data, group.ctypes.data, 1,
                                       C.byref(p), None, out.ctypes.data, n.ctypes.data), field)
    p = params(capi)
    refused(L.ndt_place_describe(xy.ctypes.data, 4, 12, 0.0, 0.0, C.byref(p), desc.ctypes.data), "stride_bytes")
    refused(L.ndt_place_describe(xy.ctypes.data, 4, 8, float("nan"), 0.0, C.byref(p), desc.ctypes.data), "centre")
    refused(L.ndt_place_describe(None, 4, 8, 0.0, 0.0, C.byref(p), desc.ctypes.data), "NULL")
    refused(L.ndt_place_describe(xy.ctypes.data, 4, 8, 0.0, 0.0, None, desc.ctypes.data), "NULL")
    refused(L.ndt_place_describe(xy.ctypes.data, 4, 8, 0.0, 0.0, C.byref(p), None), "NULL")
    assert L.ndt_place_default_params(None) == E
    k = C.c_int()
    refused(L.ndt_place_key(desc.ctypes.data, desc.ctypes.data, 0, 0, C.byref(k), None), "n_rings")
    refused(L.ndt_place_key(desc.ctypes.data, desc.ctypes.data, 20, 64, C.byref(k), None), "shift")
    refused(L.ndt_place_key(desc.ctypes.data, desc.ctypes.data, 20, -1, C.byref(k), None), "shift")
    refused(L.ndt_place_key(None, desc.ctypes.data, 20, 0, C.byref(k), None), "NULL")
    out, n, g = np.zeros(16, capi.PLACE_HIT_DTYPE), np.zeros(2, np.int32), np.zeros(2, np.int32)
    args = lambda first, n_q=1, n_items=2: (desc.ctypes.data, g.ctypes.data, n_q, desc.ctypes.data, np.asarray(first, np.int32).ctypes.data,
                                            g.ctypes.data, n_items, C.byref(p), None, out.ctypes.data, n.ctypes.data)
    refused(L.ndt_place_match_host(*args([1, 1, 1])), "item_first[0]")
    refused(L.ndt_place_match_host(*args([0, 1, 0])), "decreases")
    refused(L.ndt_place_match_host(*args([0, 1, (1 << 26) + 1])), "2^26")
    refused(L.ndt_place_match_host(*args([0, 1, 1], n_q=-1)), "< 0")
    refused(L.ndt_place_match_host(*args([0, 1, 1], n_items=-1)), "< 0")
    refused(L.ndt_place_match_host(desc.ctypes.data, g.ctypes.data, 1, desc.ctypes.data, None, g.ctypes.data, 1, C.byref(p), None,
                                   out.ctypes.data, n.ctypes.data), "NULL")
    # the calls that take a context or a set refuse a NULL one first
    assert L.ndt_place_describe_batch(None, None, 8, None, 0, None, None, 0, C.byref(p), None) == E and b"null context" in L.ndt_last_error(None)
    assert L.ndt_place_describe_batch_dev(None, None, 8, None, 0, None, None, 0, C.byref(p), None, None) == E
    assert L.ndt_place_match(None, None, None, 0, None, None, None, 0, C.byref(p), None, None, None) == E
    assert L.ndt_place_match_dev(None, None, None, 0, None, None, None, 0, C.byref(p), None, None, None, None) == E
    cand, m = np.zeros(4, capi.PLACE_CANDIDATE_DTYPE), C.c_int()
    assert L.ndt_sessions_place_candidates(None, None, None, C.byref(p), cand.ctypes.data, C.byref(m)) == E
    assert b"null session set" in L.ndt_last_error(None)


def test_align_frames_undoes_an_unknown_offset(capi):
    """B = A's trajectory as a robot that started in another frame reports it; one exact edge between a scan of A and a scan of
    B brings every pose of B back onto A's."""
    from ndt_slam_amd import replay
    rng = np.random.default_rng(0)
    ta = np.column_stack([rng.uniform(-5, 5, (10, 2)), rng.uniform(-180, 180, 10)])
    for phi, shift in ((200.0, (30.0, -12.0)), (70.0, (-3.0, 4.0)), (0.0, (0.0, 0.0))):
        c, s = np.cos(np.radians(phi)), np.sin(np.radians(phi))
        tb = np.column_stack([c * ta[:, 0] - s * ta[:, 1] + shift[0], s * ta[:, 0] + c * ta[:, 1] + shift[1], (ta[:, 2] + phi + 180) % 360 - 180])
        e = np.zeros(1, capi.PG_EDGE_DTYPE)[0]
        e["from"], e["to"], e["rel"] = 3, 9, capi.pg_edge_between(ta[3], ta[9])
        d = replay.align_frames(tb, e, ta) - ta
        d[:, 2] = (d[:, 2] + 180) % 360 - 180
        assert np.abs(d).max() < 1e-9
