"""What the place-recognition tests share: the numpy restatement of the descriptor, the key and the match (the rules of the
place section of include/ndt_mi355x.h, written from the rules and sharing no code with the library), and the point families that
sit on every boundary of those rules."""
import math

import numpy as np

SECTORS = 64
# the fp64 nearest tan(j pi / 32), j = 1 .. 7: this module's own copy of the header's literals
TAN = [float.fromhex(h) for h in ("0x1.936bb8c5b2da2p-4", "0x1.975f5e0553158p-3", "0x1.36a08355c63dcp-2", "0x1.a827999fcef32p-2",
                                  "0x1.11ab7190834ebp-1", "0x1.561b82ab7f990p-1", "0x1.a43002ae4284fp-1")]
for _j, _t in enumerate(TAN, 1):
    assert _t == np.tan(_j * np.pi / 32), (_j, _t)
assert TAN == sorted(TAN) and TAN[3] < 0.5 < TAN[4] < 1.0


def edges2(p):
    """edge2[j], j = 1 .. n_rings: two rounded products each."""
    e = np.arange(1, p.n_rings + 1, dtype=np.float64) * np.float64(p.ring_width)
    return e * e


def cells_ref(xy, centre, p):
    """(kept mask, ring, sector) of every float32 point: every operation elementwise in fp64, rounded once."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        dx = xy[:, 0].astype(np.float64) - np.float64(centre[0])
        dy = xy[:, 1].astype(np.float64) - np.float64(centre[1])
        r2 = dx * dx + dy * dy
        e2 = edges2(p)
        rmin2 = np.float64(p.r_min) * np.float64(p.r_min)
        keep = np.isfinite(r2) & ~(r2 < rmin2) & ~(r2 >= e2[-1])
        ring = (r2[:, None] >= e2[None, :]).sum(axis=1)
        ax, ay = np.abs(dx), np.abs(dy)
        a, b = np.maximum(ax, ay), np.minimum(ax, ay)
        sub = np.zeros(len(xy), np.int64)
        for t in TAN:
            sub += b >= np.float64(t) * a
        s16 = np.where(ay > ax, 15 - sub, sub)
        sector = np.where(dx >= 0, np.where(dy >= 0, s16, 63 - s16), np.where(dy >= 0, 31 - s16, 32 + s16))
    return keep, ring, sector


def describe_ref(xy, centre, p):
    """The descriptor of a cloud about a centre: [n_rings] uint64."""
    keep, ring, sector = cells_ref(xy, centre, p)
    cnt = np.zeros((p.n_rings, SECTORS), np.int64)
    np.add.at(cnt, (ring[keep], sector[keep]), 1)
    bits = (cnt >= p.min_pts).astype(np.uint64) << np.arange(SECTORS, dtype=np.uint64)
    return np.bitwise_or.reduce(bits, axis=1)


def popcount(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return np.unpackbits(a.view(np.uint8)).reshape(a.shape + (64,)).sum(axis=-1).astype(np.int64)


def rotl(a, s):
    a = np.asarray(a, np.uint64)
    s = int(s) % 64
    return a if s == 0 else (a << np.uint64(s)) | (a >> np.uint64(64 - s))


def key_ref(Q, D, s):
    """(key, overlap, n_query, n_entry) of a query against an entry at the shift s."""
    c = int(popcount(np.asarray(Q, np.uint64) & rotl(D, s)).sum())
    na, nb = int(popcount(Q).sum()), int(popcount(D).sum())
    den = na + nb - c
    return (0 if den == 0 else (c * 65536) // den), c, na, nb


def match_ref(capi, q_desc, q_group, d_desc, item_first, item_group, p):
    """(hits [n_q, top_k] PLACE_HIT_DTYPE, n [n_q], table [n_q, n_items]) by the rules, every shift of every entry tried."""
    q_desc, d_desc = np.asarray(q_desc, np.uint64).reshape(-1, p.n_rings), np.asarray(d_desc, np.uint64).reshape(-1, p.n_rings)
    n_q, n_items = len(q_desc), len(item_group)
    table = np.zeros((n_q, n_items), np.uint64)
    hits, n = np.zeros((n_q, p.top_k), capi.PLACE_HIT_DTYPE), np.zeros(n_q, np.int32)
    nb = popcount(d_desc).sum(axis=1)
    rots = np.stack([rotl(d_desc, s) for s in range(SECTORS)], axis=1) if len(d_desc) else np.zeros((0, SECTORS, p.n_rings), np.uint64)
    for q in range(n_q):
        na = int(popcount(q_desc[q]).sum())
        c = popcount(rots & q_desc[q][None, None, :]).sum(axis=2)                      # [desc, shift]
        den = na + nb[:, None] - c
        key = np.where(den == 0, 0, (c * 65536) // np.maximum(den, 1))
        found = []
        for i in range(n_items):
            a, e = int(item_first[i]), int(item_first[i + 1])
            if (q_group[q] >= 0 and q_group[q] == item_group[i]) or e <= a:
                continue
            k = key[a:e]
            d, s = np.unravel_index(int(np.argmax(k)), k.shape)                        # (the first maximum: lowest descriptor, then lowest shift)
            d += a
            table[q, i] = (int(k.max()) << 32) | (0xFFFFFFFF - ((int(d) << 6) | int(s)))
            if k.max() >= p.min_key:
                found.append((-int(k.max()), i, int(d), int(s)))
        found.sort()
        for r, (mk, i, d, s) in enumerate(found[:p.top_k]):
            kk, cc, qa, qb = key_ref(q_desc[q], d_desc[d], s)
            assert kk == -mk
            hits[q, r] = (i, d, s, kk, cc, qa, qb, r)
        n[q] = min(len(found), p.top_k)
    return hits, n, table


def f32_neighbours(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def boundary_points(p, rng):
    """Points (about the origin) on every boundary of the descriptor's rules, as float64 offsets; the caller adds a centre."""
    pts = []
    w = p.ring_width
    for z in (0.0, -0.0):                                                   # the axes and diagonals, each sign of zero
        for r in (0.3, 1.0, 2.75):
            pts += [(r, z), (-r, z), (z, r), (z, -r), (r, r), (-r, r), (r, -r), (-r, -r)]
    for t in TAN:                                                           # the float32 neighbours either side of b = T a, all octants
        for a in (0.15 * p.n_rings * w, 0.33 * p.n_rings * w, 0.6 * p.n_rings * w):
            for b in f32_neighbours(np.float32(t * a)):
                for sx in (1, -1):
                    for sy in (1, -1):
                        pts += [(sx * a, sy * float(b)), (sx * float(b), sy * a)]
    for j in range(1, p.n_rings + 1):                                       # ring edges: on the edge and next to it
        r = j * w
        for x in f32_neighbours(r):
            pts += [(float(x), 0.0), (0.0, -float(x))]
        pts += [(0.6 * r, 0.8 * r), (-0.8 * r, 0.6 * r)]                      # (3-4-5 triangles: (1.5, 2.0) with width 0.5 is r2 exactly on an edge)
    for x in f32_neighbours(p.r_min):                                       # the r_min boundary
        pts += [(float(x), 0.0), (0.0, float(x))]
    pts += [(0.0, 0.0), (-0.0, -0.0), (float("nan"), 1.0), (1.0, float("nan")), (float("inf"), 0.0), (0.0, -float("inf")), (1e30, 1e30)]
    pts += list(rng.uniform(-1.2 * p.n_rings * w, 1.2 * p.n_rings * w, size=(200, 2)))
    return np.array(pts, dtype=np.float64)


def cloud_about(offsets, centre):
    """float32 points at centre + offsets (rounded once to float32), so that the offsets the rules see are near the crafted ones."""
    with np.errstate(all="ignore"):
        return (np.asarray(offsets, np.float64) + np.asarray(centre, np.float64)[None, :]).astype(np.float32)


def random_desc(rng, n, n_rings, density=0.3):
    bits = rng.random((n, n_rings, SECTORS)) < density
    return np.bitwise_or.reduce(bits.astype(np.uint64) << np.arange(SECTORS, dtype=np.uint64), axis=2)


# the world offsets of every family; the third is the second rounded to float32, about which the crafted offsets that are
# multiples of 2^-14 -- the ring edges of the default width among them -- are met exactly by float32 points
CENTRES = [(0.0, 0.0), (-1003.3, 707.1), (float(np.float32(-1003.3)), float(np.float32(707.1)))]
