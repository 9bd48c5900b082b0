"""Maps, query sets and a brute-force reference for the nearest-raw-point search behind getFitnessScore (row a7,
ndt_fitness.hip.h).  Tests only: tests/test_fitness_brute_force.py (CPU) and tests/test_gpu_fitness_geometry.py import it.

The reference here is not a ring search: `brute_sq` takes the minimum over ALL map points of the float32 expression the
kernels evaluate, so a misconception shared by the device search and the oracle's ring search cannot hide behind it.

Exact sums.  A float32 distance d = m 2^e (0.5 <= m < 1) is a whole multiple of 2^(e - 24).  For n non-zero distances with
exponents in [e_min, e_max] every partial sum, in any order, is a whole multiple of 2^(e_min - 24) below
2^(e_max + ceil(log2 n)): it fits the 53 bits of a double when  e_max - e_min + 1 <= 29 - ceil(log2 n)  (`max_binades`).
`stratify` cuts a query set into such scans.  Their sum is exact however it is added, the mean is ONE correctly rounded
division of that sum by a whole number, and so the device's mean must be bit-equal to `expected_mean`: a single query
that is wrong by one float32 ulp changes it.  Scans that cannot be stratified (phases mixed inside one wave) are compared at
`loose_rel(n)` = n 2^-53, the worst case of any summation order over non-negative terms.
"""
import math
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F = np.float32
DBL_MAX = float(np.finfo(np.float64).max)

LEAVES = (0.05, 0.07, 0.1, 0.3, 0.5, 1.0, 2.0)
OFFSETS = ((0.0, 0.0), (-1003.3, 707.1), (2000.0, -1500.0), (8191.7, 8191.7))
GPU_LEAVES = LEAVES                                    # the leaves the GPU module builds every family at (every offset)
# family -> the phase it is named for: classify() must find at least MIN_SHARE of its live queries there
FAMILIES = {
    "sparse": "far", "dense1": "heavy", "row": "clamped", "column": "clamped", "one": "clamped", "lattice": "on_wall",
    "islands": "walk", "frame": "blind", "buckets": "near", "straddle": "ring1",
    "narrow7": "clamped", "narrow8": "clamped", "narrow9": "clamped", "narrow16": "clamped", "narrow17": "clamped",
    "flat9": "clamped",
}
MIN_SHARE = 0.25
# (div_x, div_y) the degenerate families must have, whatever the leaf and the offset (None: not fixed)
GRID_OF = {"row": (None, 1), "column": (1, None), "one": (1, 1), "narrow7": (7, 24), "narrow8": (8, 24), "narrow9": (9, 24),
           "narrow16": (16, 24), "narrow17": (17, 24), "flat9": (24, 9), "frame": (22, 22)}

Workload = namedtuple("Workload", "family leaf offset map queries")
Grid = namedtuple("Grid", "leaf inv min_bx min_by div_x div_y")


# ------------------------------------------------------------------------------------------ the reference
def brute_sq(map_xy, queries, with_index=False, pairs_per_chunk=1 << 22):
    """Float32 squared distance from every query to its nearest map point: the minimum over ALL map points of
    F(ex * ex) + F(ey * ey) (two rounded products, one rounded sum -- the library is built with -ffp-contract=off).  A
    query with a NaN coordinate gives NaN, one whose every distance overflows gives inf: non-finite stays non-finite.
    with_index: also the index of the (first) nearest point."""
    m = np.ascontiguousarray(map_xy, dtype=F).reshape(-1, 2)
    q = np.ascontiguousarray(queries, dtype=F).reshape(-1, 2)
    out = np.empty(len(q), dtype=F)
    arg = np.zeros(len(q), dtype=np.int64)
    mx, my = np.ascontiguousarray(m[:, 0]), np.ascontiguousarray(m[:, 1])
    step = max(1, pairs_per_chunk // max(len(m), 1))
    with np.errstate(over="ignore", invalid="ignore"):
        for i0 in range(0, len(q), step):
            ex = q[i0:i0 + step, 0, None] - mx[None, :]
            ey = q[i0:i0 + step, 1, None] - my[None, :]
            ex *= ex
            ey *= ey
            ex += ey
            assert ex.dtype == F
            out[i0:i0 + step] = ex.min(axis=1)
            if with_index:
                arg[i0:i0 + step] = ex.argmin(axis=1)
    return (out, arg) if with_index else out


def expected_mean(d):
    """getFitnessScore of a scan whose float32 distances are d: the exactly rounded sum of the finite ones over their
    number, DBL_MAX when there is none."""
    d = np.asarray(d)
    fin = np.isfinite(d)
    n = int(fin.sum())
    if n == 0:
        return DBL_MAX
    return math.fsum(d[fin].astype(np.float64).tolist()) / n


def queries_of(scan, T, sse=True):
    """The float32 transform of the scan by T = (c, s, tx, ty) (oracle/ndt_numpy.py, fitness): both transform_sse forms."""
    c, s, tx, ty = [F(v) for v in T]
    scan = np.ascontiguousarray(scan, dtype=F).reshape(-1, 2)
    x, y = scan[:, 0], scan[:, 1]
    with np.errstate(over="ignore", invalid="ignore"):
        if not sse:
            qx = F(F(c * x) + F(-s * y)) + tx
            qy = F(F(s * x) + F(c * y)) + ty
        else:
            qx = F(c * x) + F(F(-s * y) + tx)
            qy = F(s * x) + F(F(c * y) + ty)
    return np.stack([qx, qy], axis=1).astype(F)


def scan_for(queries, pose):
    """A float32 scan in the sensor frame whose transform by `pose` (x, y, yaw) lands about on `queries` (the test takes
    the queries it compares from the record's own matrix: this only aims)."""
    q = np.asarray(queries, dtype=np.float64) - np.asarray(pose[:2], dtype=np.float64)[None, :]
    c, s = math.cos(pose[2]), math.sin(pose[2])
    return np.stack([c * q[:, 0] + s * q[:, 1], -s * q[:, 0] + c * q[:, 1]], axis=1).astype(F)


# ------------------------------------------------------------------------------------------ the grid
def grid_of(map_xy, leaf):
    """The voxel grid of a map as the library lays it out: floor(x * inv_leaf) in float32, inv_leaf = 1.0f / leaf."""
    m = np.ascontiguousarray(map_xy, dtype=F).reshape(-1, 2)
    leaf = F(leaf)
    inv = F(1.0) / leaf
    v = np.floor(m * inv).astype(np.int64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    return Grid(leaf, inv, int(lo[0]), int(lo[1]), int(hi[0] - lo[0] + 1), int(hi[1] - lo[1] + 1))


def voxel_of(G, pts):
    """Unclamped voxel coordinates relative to the grid, as float64 (queries may lie beyond any int; NaN stays NaN)."""
    p = np.ascontiguousarray(pts, dtype=F).reshape(-1, 2)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.floor(p * G.inv).astype(np.float64)
    v[:, 0] -= G.min_bx
    v[:, 1] -= G.min_by
    return v


def classify(map_xy, leaf, queries, d, arg=None):
    """Lower bounds, from the brute-force distances and the grid alone, for the number of queries that MUST take each
    phase of the device search (boolean masks per query; `counts(masks)` sums them):
      live     finite query (the others are dropped before the search)
      far      d > (0.999 leaf)^2: the stopping bound of ring 1 is missed, phase 3 runs
      near     live, finite distance and not far
      clamped  the query lies outside the grid: its home voxel is clamped, nothing is pruned
      blind    inside the grid and d > (2 sqrt2 (leaf + slack))^2: the whole 3 x 3 neighbourhood lies nearer than that, so
               it is empty and the query enters phase 3 without a point in hand
      walk     inside and d > (9 sqrt2 (leaf + slack))^2: no voxel the occupancy tiles cover (8 away) holds a point, the
               ring walk behind them finds it
      on_wall  a coordinate of the query is a float32 lattice line k * leaf or one float32 step beside it
      heavy    inside, and a voxel with >= 1000 points lies within two voxels of the home voxel
      ring1    (needs arg) inside, not far, and the nearest point lies in another voxel of the 3 x 3 neighbourhood: only
               the ring-1 phase can have found it
      quiet    d == 0, or the 3 x 3 neighbourhood of the (clamped) home voxel holds no point outside the home voxel:
               the query has no ring-1 work
    slack = max(1e-3 leaf, 2.5e-7 (|qx| + |qy| + leaf)) is near_walls' allowance for the float32 voxel rounding."""
    m = np.ascontiguousarray(map_xy, dtype=F).reshape(-1, 2)
    q = np.ascontiguousarray(queries, dtype=F).reshape(-1, 2)
    G = grid_of(m, leaf)
    L = float(G.leaf)
    d64 = np.asarray(d, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        live = np.isfinite(q).all(axis=1)
        v = voxel_of(G, q)
        inside = live & (v[:, 0] >= 0) & (v[:, 0] < G.div_x) & (v[:, 1] >= 0) & (v[:, 1] < G.div_y)
        slack = np.maximum(1e-3 * L, 2.5e-7 * (np.abs(q[:, 0].astype(np.float64)) + np.abs(q[:, 1].astype(np.float64)) + L))
        far = live & (d64 > (0.999 * L) ** 2)
        blind = inside & (d64 > (2 * math.sqrt(2) * (L + slack)) ** 2)
        walk = inside & (d64 > (9 * math.sqrt(2) * (L + slack)) ** 2)
        k = np.rint(q.astype(np.float64) / L)
        line = (k * L).astype(F)
        on = (q == line) | (q == np.nextafter(line, F(np.inf))) | (q == np.nextafter(line, F(-np.inf)))
    out = dict(live=live, far=far, near=live & np.isfinite(d64) & ~far, clamped=live & ~inside, blind=blind, walk=walk,
               on_wall=live & on.any(axis=1))
    # occupancy of the grid, and the home voxel of every live query clamped into it
    mv = voxel_of(G, m).astype(np.int64)
    cnt = np.zeros((G.div_y, G.div_x), dtype=np.int64)
    np.add.at(cnt, (mv[:, 1], mv[:, 0]), 1)
    hx = np.clip(np.where(live, v[:, 0], 0), 0, G.div_x - 1).astype(np.int64)
    hy = np.clip(np.where(live, v[:, 1], 0), 0, G.div_y - 1).astype(np.int64)
    heavy = np.zeros(len(q), dtype=bool)
    for y, x in zip(*np.nonzero(cnt >= 1000)):
        heavy |= inside & (np.abs(hx - x) <= 2) & (np.abs(hy - y) <= 2)
    out["heavy"] = heavy
    pad = np.pad(cnt, 1)
    around = sum(pad[1 + dy + hy, 1 + dx + hx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy)
    out["quiet"] = live & ((d64 == 0.0) | (around == 0))
    if arg is not None:
        px, py = mv[arg, 0], mv[arg, 1]
        cheb = np.maximum(np.abs(px - hx), np.abs(py - hy))
        out["ring1"] = inside & ~far & (cheb == 1)
    return out


def counts(masks):
    return {k: int(v.sum()) for k, v in masks.items()}


# ------------------------------------------------------------------------------------------ exact sums
def max_binades(n):
    """How many binades the non-zero distances of an n-point scan may span for every partial sum to be exact in fp64."""
    return 29 - max(0, int(math.ceil(math.log2(max(n, 1)))))


def binades(d):
    """Number of binades the non-zero finite entries of d span (0: there is none)."""
    d = np.asarray(d, dtype=np.float64)
    d = d[np.isfinite(d) & (d != 0.0)]
    if len(d) == 0:
        return 0
    e = np.frexp(d)[1]
    return int(e.max() - e.min() + 1)


def sum_is_exact(d):
    return binades(d) <= max_binades(len(d))


def loose_rel(n):
    """Relative bound of a scan that is NOT stratified: any order of adding n non-negative terms in fp64."""
    return n * 2.0 ** -53


def stratify(queries, d, n_max):
    """Index arrays (ascending, so a scan keeps the input order) that cut the query set into scans of at most n_max points
    whose non-zero distances span at most max_binades(n_max) binades.  Queries without a finite non-zero distance (on a map
    point, dropped, out of reach) add nothing to a sum: they are dealt out over the scans."""
    d = np.asarray(d, dtype=np.float64)
    n = len(d)
    plain = np.isfinite(d) & (d != 0.0)
    idx = np.flatnonzero(plain)
    e = np.frexp(d[idx])[1]
    order = np.argsort(e, kind="stable")
    idx, e = idx[order], e[order]
    room = max_binades(n_max)
    assert room >= 1, n_max
    groups, s = [], 0
    while s < len(idx):
        t = s
        while t < len(idx) and t - s < n_max and e[t] - e[s] + 1 <= room:
            t += 1
        groups.append(idx[s:t])
        s = t
    if not groups:
        groups = [np.zeros(0, dtype=np.int64)]
    rest = np.flatnonzero(~plain)
    out = []
    for grp in groups:
        free = max(n_max - len(grp), 0)
        out.append(np.sort(np.concatenate([grp, rest[:free]])))
        rest = rest[free:]
    while len(rest):                                       # more queries without a distance than room beside the others
        out.append(rest[:n_max])
        rest = rest[n_max:]
    assert sum(len(o) for o in out) == n
    return [o for o in out if len(o)]


# ------------------------------------------------------------------------------------------ maps and queries
def _rng(*key):
    return np.random.Generator(np.random.Philox(np.random.SeedSequence([20240607] + [int(k) for k in key])))


def lattice_base(leaf, offset):
    """The world offset moved onto the voxel lattice, so that a family has the same shape in voxels wherever it stands."""
    L = float(F(leaf))
    return np.array([round(offset[0] / L) * L, round(offset[1] / L) * L]), L


def _box_queries(rng, lo, hi, L, n, reach):
    return rng.uniform(lo - reach * L, hi + reach * L, size=(n, 2))


def _snap(rng, q, L, share):
    """A share of the queries onto lattice lines (x, y or both), a third of those one float32 step beside the line."""
    n = len(q)
    out = q.astype(F)
    pick = rng.random(n) < share
    axis = rng.integers(0, 3, n)                           # 0: x, 1: y, 2: both
    step = rng.integers(-1, 2, (n, 2))
    for a in (0, 1):
        sel = pick & ((axis == a) | (axis == 2))
        line = (np.rint(q[sel, a] / L) * L).astype(F)
        up, dn = np.nextafter(line, F(np.inf)), np.nextafter(line, F(-np.inf))
        out[sel, a] = np.where(step[sel, a] > 0, up, np.where(step[sel, a] < 0, dn, line))
    return out


def make(family, leaf, offset, n_queries=1024):
    """The map and the query set of one (family, leaf, offset): deterministic (numpy Philox, seeded by the three)."""
    fam_id = list(FAMILIES).index(family)
    rng = _rng(fam_id, LEAVES.index(leaf) if leaf in LEAVES else int(leaf * 1e4), OFFSETS.index(tuple(offset)) if tuple(offset) in OFFSETS else 99)
    base, L = lattice_base(leaf, offset)
    n = n_queries
    reach, snap, on_pts = 12.0, 0.3, 0.05
    extra = None
    if family == "sparse":
        m = rng.uniform(0, 60, (800, 2))
    elif family == "dense1":
        m = np.concatenate([rng.uniform(0, 60, (300, 2)), rng.uniform(30.1, 30.9, (5001, 2))])
        extra = rng.uniform(28.0, 33.0, (n // 2, 2))       # inside the full voxel, its neighbours, two voxels away
    elif family == "row":
        m = np.stack([rng.uniform(0, 200, 1500), rng.uniform(0.1, 0.9, 1500)], axis=1)
    elif family == "column":
        m = np.stack([rng.uniform(0.1, 0.9, 1500), rng.uniform(0, 200, 1500)], axis=1)
    elif family == "one":
        m = rng.uniform(0.1, 0.8, (7, 2))
        far_out = rng.uniform(-1, 1, (n // 8, 2))          # every side and corner, out to 10^3 voxels
        far_out = np.sign(far_out) * 10.0 ** rng.uniform(-0.3, 3.0, far_out.shape) * (rng.random(far_out.shape) < 0.7)
        extra = 0.5 + far_out
    elif family == "lattice":
        m = rng.uniform(0, 40, (1500, 2))
        m = np.where(rng.random((1500, 1)) < 0.5, np.rint(m), m)
        snap, reach = 0.7, 3.0
    elif family == "islands":
        m = np.concatenate([rng.normal(0, 1.5, (600, 2)), rng.normal(0, 1.5, (600, 2)) + np.array([70.3, 51.7])])
        reach = 2.0
    elif family == "frame":
        t = rng.uniform(0, 22, 4 * 90)
        u = rng.uniform(0.1, 0.9, 4 * 90)
        side = np.repeat(np.arange(4), 90)
        m = np.where((side < 2)[:, None], np.stack([t, u + 21 * (side == 1)], axis=1), np.stack([u + 21 * (side == 3), t], axis=1))
        m = np.concatenate([m, [[0.5, 0.5], [21.5, 21.5]]])
        reach = 1.0
    elif family == "buckets":
        # row 1: voxels 0..29 hold 1..30 points; row 3: 30..1; one point in row 0 shifts the parity of every start
        parts = [[[3.5, 0.5]]]
        for k in range(30):
            parts.append(np.stack([k + rng.uniform(0.1, 0.9, k + 1), 1 + rng.uniform(0.1, 0.9, k + 1)], axis=1))
            parts.append(np.stack([k + rng.uniform(0.1, 0.9, 30 - k), 3 + rng.uniform(0.1, 0.9, 30 - k)], axis=1))
        m = np.concatenate(parts)
        reach = 2.0
    elif family == "straddle":
        # one triple per voxel of an 18 x 18 block: the query a third of the wall slack inside a wall of its voxel, a point
        # as far beyond that wall, and a point of its own voxel 0.9 slack away -- so the nearest point lies in the next
        # voxel, nearer to the query than the slack by which near_walls must mistrust the wall
        u = max(1e-3, 2.5e-7 * (abs(base[0]) + abs(base[1]) + 20 * L) / L)
        vx, vy = [a.ravel().astype(np.float64) for a in np.meshgrid(np.arange(1, 19), np.arange(1, 19))]
        side, t = rng.integers(0, 4, len(vx)), rng.uniform(0.2, 0.8, len(vx))
        sgn = np.where(side % 2 == 0, 1.0, -1.0)            # 0: left wall, 1: right, 2: lower, 3: upper
        wall = np.where(side % 2 == 0, 0.0, 1.0)
        a = wall + sgn * 0.3 * u                            # the query's coordinate across the wall, the other point's, the home point's
        qa, oa, ha = a, wall - sgn * 0.3 * u, a
        al = np.stack([t, t, t + 0.9 * u])                  # ... and along it
        horiz = (side < 2)[None, :]
        xs = np.where(horiz, np.stack([qa, oa, ha]), al) + vx[None, :]
        ys = np.where(horiz, al, np.stack([qa, oa, ha])) + vy[None, :]
        extra = np.stack([xs[0], ys[0]], axis=1)
        m = np.concatenate([np.stack([xs[1], ys[1]], axis=1), np.stack([xs[2], ys[2]], axis=1), [[0.5, 0.5], [19.5, 19.5]]])
        reach, snap, on_pts = 2.0, 0.3, 0.08
    elif family.startswith("narrow") or family == "flat9":
        w, h = (24, 9) if family == "flat9" else (int(family[6:]), 24)
        m = np.concatenate([np.floor(rng.uniform(0, 1, (160, 2)) * [w, h]) + rng.uniform(0.1, 0.9, (160, 2)),
                            [[0.5, 0.5], [w - 0.5, h - 0.5]]])
    else:
        raise KeyError(family)
    # (shapes in voxels; wherever the shape of the grid depends on it the points keep a tenth of a voxel clear of the
    # lattice: the float32 voxel coordinate of a point 8 km out at leaf 0.05 is good to 1 / 64 voxel)
    lo, hi = m.min(axis=0), m.max(axis=0)
    q = _box_queries(rng, lo, hi, 1.0, n, reach)
    if extra is not None:
        q[:len(extra)] = extra
    map32 = (base[None, :] + m * L).astype(F)
    qw = base[None, :] + q * L
    q32 = _snap(rng, qw, L, snap)
    if family == "straddle":
        q32[:len(extra)] = qw[:len(extra)].astype(F)       # (the designed queries stay where they were put)
    sel = rng.random(n) < on_pts
    if family == "straddle":
        sel[:len(extra)] = False
    q32[sel] = map32[rng.integers(0, len(map32), int(sel.sum()))]
    rng.shuffle(q32, axis=0)
    return Workload(family, leaf, tuple(offset), map32, q32)


def out_of_reach(like, n):
    """n queries so far from everything near `like` that every float32 squared distance overflows: they have no distance."""
    s = np.where((np.arange(2 * n).reshape(n, 2) % 3) == 0, -1.0, 1.0)
    return (s * 3.0e19 + np.asarray(like, dtype=np.float64)[None, :]).astype(F)


# ring-needing lanes per 64-point chunk: both sides of the joint ring work's limits (1 .. 12 lanes share the work, 0 and 13 ..
# 64 do not), 320 chunks = 20480 points, above the 20000 a scan may have to be put in voxel order
WAVE_CHUNKS = (0, 1, 12, 13, 64, 2, 11, 14, 32, 63) * 32


def wave_scan(W, chunks):
    """A scan of len(chunks) * 64 points over the map of workload W for the wave-composition test: chunk j holds exactly
    chunks[j] queries that need ring 1 (classify: ring1) in its FIRST lanes and 64 - chunks[j] queries without ring-1 work
    (classify: quiet -- on a map point, or with an empty 3 x 3 neighbourhood) behind them; ten chunks of far and of clamped
    queries follow.  The non-zero distances are drawn from a window of binades narrow enough for an exact sum
    (`sum_is_exact`)."""
    rng = _rng(77, len(chunks), list(FAMILIES).index(W.family))
    G = grid_of(W.map, W.leaf)
    L = float(G.leaf)
    lo = np.array([G.min_bx, G.min_by]) * L
    hi = lo + np.array([G.div_x, G.div_y]) * L
    pool = rng.uniform(lo, hi, size=(60000, 2)).astype(F)
    d, arg = brute_sq(W.map, pool, with_index=True)
    cl = classify(W.map, W.leaf, pool, d, arg)
    n = 64 * len(chunks)
    room = max_binades(n)
    eL = int(np.frexp(L * L)[1])
    e = np.frexp(d.astype(np.float64))[1]
    lo_e = eL + 7 - room                                    # window [lo_e, eL + 6]: up to 64 leaf^2, down as far as the sum allows
    ring = np.flatnonzero(cl["ring1"] & (e >= lo_e) & (d > 0))
    blind = np.flatnonzero(cl["blind"] & cl["quiet"] & (e <= eL + 6))
    need = int(sum(chunks))
    assert len(ring) >= need, (len(ring), need)
    ring = ring[:need]
    out = np.empty((n, 2), dtype=F)
    r = b = 0
    for j, k in enumerate(chunks):
        s = 64 * j
        out[s:s + k] = pool[ring[r:r + k]]; r += k
        for i in range(s + k, s + 64):
            if (i % 5 == 0) and len(blind):
                out[i] = pool[blind[b % len(blind)]]; b += 1
            else:
                out[i] = W.map[(7 * i) % len(W.map)]
    # far and clamped queries beside them: ten more chunks, from the grid and six voxels around it, inside the same window
    wide = rng.uniform(lo - 6 * L, hi + 6 * L, size=(20000, 2)).astype(F)
    dw = brute_sq(W.map, wide)
    cw = classify(W.map, W.leaf, wide, dw)
    ew = np.frexp(dw.astype(np.float64))[1]
    ok = (ew >= lo_e) & (ew <= eL + 6) & (dw > 0)
    far, clamped = np.flatnonzero(cw["far"] & ~cw["clamped"] & ok)[:320], np.flatnonzero(cw["clamped"] & ok)[:320]
    tail = np.concatenate([far, clamped])
    return np.concatenate([out, wide[rng.permutation(tail)]])


# ------------------------------------------------------------------------------------------ on a mismatch
def localise(fitness_of, map_xy, leaf, scan, T, sse=True, what=""):
    """Bisect a scan whose mean differs from brute force down to one point with `fitness_of(sub_scan)` (the single-query
    search, ndt_fitness_at) and say which query it is: the next rewrite of the search needs the query, not a mean."""
    scan = np.ascontiguousarray(scan, dtype=F).reshape(-1, 2)
    q = queries_of(scan, T, sse)
    d = brute_sq(map_xy, q)
    idx = np.arange(len(scan))

    def agrees(sel):
        got, want = fitness_of(scan[sel]), expected_mean(d[sel])
        return got == want if sum_is_exact(d[sel]) else abs(got - want) <= loose_rel(len(sel)) * abs(want)
    if agrees(idx):
        return "%s: ndt_fitness_at agrees with brute force on this scan -- the difference is in the batch path" % what
    while len(idx) > 1:
        half = idx[:len(idx) // 2]
        idx = half if not agrees(half) else idx[len(idx) // 2:]
    i = int(idx[0])
    G = grid_of(map_xy, leaf)
    v = np.nan_to_num(voxel_of(G, q[i:i + 1])[0], nan=-1.0, posinf=2.0 ** 31, neginf=-2.0 ** 31)
    got = fitness_of(scan[i:i + 1])
    return ("%s: point %d, query (%r, %r), voxel (%d, %d) of a %d x %d grid, cx & 7 = %d, cy & 7 = %d, leaf %r: brute force %r, "
            "device %r" % (what, i, float(q[i, 0]), float(q[i, 1]), int(v[0]), int(v[1]), G.div_x, G.div_y,
                           int(np.clip(v[0], 0, G.div_x - 1)) & 7, int(np.clip(v[1], 0, G.div_y - 1)) & 7, float(G.leaf),
                           float(d[i]), got))


# ------------------------------------------------------------------------------------------ the match at other geometries
MATCH_OFFSETS = ((-1003.3, 707.1), (2000.0, -1500.0))
MATCH_LEAVES = (0.1, 0.3, 1.0)


def shifted_world(offset):
    """The C1 wall world (5k-point map, 360-point scans) moved by `offset`: -> (map, make) with make(k) = (scan in the sensor
    frame, truth, init), the poses moved with the map."""
    from ndt_slam_amd import synth
    cfg = synth.CONFIGS["C1"]
    m0 = synth.make_map(cfg["n_map"], cfg["half"])
    sf = synth.ScanFactory(m0, cfg["half"], cfg["n_scan"])
    off = np.array([offset[0], offset[1], 0.0])

    def make(k):
        scan, truth, init = sf.make(k)
        return scan, truth + off, init + off
    return (m0.astype(np.float64) + off[None, :2]).astype(F), make
