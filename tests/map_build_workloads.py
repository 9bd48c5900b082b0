"""Clouds, a path census and an exact reference for the map build (row a2, ndt_map_build.hip.h).  Tests only:
tests/test_map_build_host.py (CPU) and tests/test_gpu_map_build_geometry.py import it.

The build's kernels choose between data paths by constants (kBigVoxel 16, kBigRuns 64, kBigStage 512, kFinStage 1536,
kScanTile 8192, the 64 lanes of a wave).  Every family below is a function of (leaf, offset) that returns clouds aimed at
named paths; `paths_of` says, from the cloud alone, which paths a build of it MUST take; `exact_leaf` restates the
statistics of one voxel in exact rational arithmetic, sharing no code with the oracle or the device.

Why the run counts are exact.  map_count / map_scatter cut the cloud into aligned chunks of 64 consecutive points (a wave)
and place every maximal run of equal voxel keys inside a chunk as one block of `perm` ("wave-run").  map_order counts a new
run wherever two neighbouring entries of a voxel's segment are not consecutive point numbers.  Two wave-runs that lie next
to each other in the segment can only fuse when the last number of one is the first number of the other minus one, i.e.
when they are the two parts of ONE run of the cloud cut by a multiple of 64 (and the later part's atomic came first).  So
the number of runs map_order sees lies in [cloud_runs, wave_runs]: cloud_runs counts maximal runs of consecutive point
numbers of the voxel in the cloud, wave_runs counts them again after cutting at every multiple of 64.  A path is CERTAIN
only when both ends of that interval lie on the same side of kBigRuns; `runs_k` builds its clouds so that no run crosses a
multiple of 64 and the two counts are equal (its `long` variant crosses on purpose and stays below kBigRuns at both ends).
"""
import os
import sys
from collections import namedtuple
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import fitness_workloads as FW  # noqa: E402

F = np.float32
LEAVES = (0.1, 0.3, 1.0)
OFFSETS = FW.OFFSETS
FAR_OFFSET = OFFSETS[3]
# the constants of ndt_map_build.hip.h the clouds aim at
K_BIG_VOXEL, K_BIG_RUNS, K_BIG_STAGE, K_FIN_STAGE, K_SCAN_TILE, WAVE = 16, 64, 512, 1536, 8192, 64

DEFAULTS = dict(min_pts=6, eig_mult=0.01, cov_unbiased=0, cov_init_identity=1)     # the default preset (PCL 1.10)

Case = namedtuple("Case", "family name leaf offset cloud prm purpose")


def params_of(case_or_prm):
    p = dict(DEFAULTS)
    p.update(case_or_prm.prm if isinstance(case_or_prm, Case) else case_or_prm)
    return p


def _rng(*key):
    return np.random.Generator(np.random.Philox(np.random.SeedSequence([20250101] + [int(k) for k in key])))


def _key(leaf, offset):
    return LEAVES.index(leaf), OFFSETS.index(tuple(offset))


def _world(leaf, offset, vox, u):
    """float32 points at (vox + u) voxels from the lattice-snapped base."""
    base, L = FW.lattice_base(leaf, offset)
    return (base[None, :] + (np.asarray(vox, dtype=np.float64) + np.asarray(u, dtype=np.float64)) * L).astype(F)


def _interleave(counts, run=1):
    """Voxel number of every cloud point: the voxels take turns, `run` points at a time, until each has had its count."""
    counts = np.asarray(counts, dtype=np.int64)
    vid = np.repeat(np.arange(len(counts)), counts)
    j = np.concatenate([np.arange(c) for c in counts]) if len(counts) else np.zeros(0, np.int64)
    order = np.lexsort((vid, j // run))
    return vid[order]


def _fill(rng, vid, vox):
    """A uniform point a tenth of a voxel clear of the walls for every entry of vid (voxel coordinates vox[vid])."""
    vox = np.asarray(vox, dtype=np.float64)
    return vox[vid], rng.uniform(0.1, 0.9, (len(vid), 2))


def _cloud(rng, leaf, offset, vid, vox, targets=None):
    """The float32 cloud of `_fill`, with the points of every target voxel (default: all) of three or more points drawn
    again until the voxel is order-sensitive (`order_sensitive`): far from the origin all points of a voxel share one
    float32 exponent, the fp64 sums of a small voxel are then exact in any order and only the float32 centroid sum can
    tell two orders apart -- which it does for most draws, not for all."""
    v, u = _fill(rng, vid, vox)
    c = _world(leaf, offset, v, u)
    for k in (np.unique(vid) if targets is None else targets):
        m = np.flatnonzero(vid == k)
        if len(m) < 3:
            continue
        for _ in range(200):
            if order_sensitive(c[m]):
                break
            c[m] = _world(leaf, offset, v[m], rng.uniform(0.1, 0.9, (len(m), 2)))
        else:
            raise AssertionError("no order-sensitive draw for voxel %d of %d points" % (k, len(m)))
    return c


# ------------------------------------------------------------------------------------------ the families
SIZES = (1, 5, 6, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512, 513, 5001)


def fam_sizes(leaf, offset):
    """One voxel per size in one grid row, the voxels' points interleaved one by one: a voxel of n points arrives as about n
    runs (the last voxels, once the others are used up, as fewer)."""
    rng = _rng(1, *_key(leaf, offset))
    vid = _interleave(SIZES, 1)
    cloud = _cloud(rng, leaf, offset, vid, [(i, 0) for i in range(len(SIZES))])
    purpose = {"order:a", "order:b", "order:c", "order:d", "order:n16", "order:n17", "order:n512", "order:n513",
               "order:a_n%4=0", "order:a_n%4=1", "order:a_n%4=2", "order:a_n%4=3", "fin:stream", "leaf:below_min_pts"}
    return [Case("sizes", "sizes[min_pts=%d]" % mp, leaf, offset, cloud, dict(min_pts=mp), purpose) for mp in (6, 3, 10)]


RUNS_K = (1, 2, 63, 64, 65, 200)


def fam_runs_k(leaf, offset):
    """Two voxels A and B alternating in blocks: each gets exactly k runs.  k <= 2: blocks of 32 points (A B | A B: a block
    starts at a multiple of 32 and never crosses a multiple of 64); k >= 63: blocks of 2 points (a block starts at an even
    number).  Strict alternation: between two runs of A lies a run of B, so no two runs of A are consecutive numbers and none
    can fuse; cloud_runs == wave_runs == k.  `long`: A has a run of 200 points from point 10 on (cut at 64, 128 and 192: four
    wave-runs that may or may not fuse in perm) and a second run of 20: between 2 and 5 runs, the merge path either way."""
    out = []
    for k in RUNS_K:
        rng = _rng(2, k, *_key(leaf, offset))
        blk = 32 if k <= 2 else 2
        vid = np.tile(np.repeat([0, 1], blk), k)
        purpose = {"order:b" if k <= K_BIG_RUNS else "order:c"}
        if k in (64, 65):
            purpose.add("order:runs%d" % k)
        out.append(Case("runs_k", "runs_k[%d]" % k, leaf, offset, _cloud(rng, leaf, offset, vid, [(0, 0), (1, 0)]), {}, purpose))
    rng = _rng(2, 999, *_key(leaf, offset))
    vid = np.concatenate([np.ones(10, int), np.zeros(200, int), np.ones(20, int), np.zeros(20, int), np.ones(7, int)])
    out.append(Case("runs_k", "runs_k[long]", leaf, offset, _cloud(rng, leaf, offset, vid, [(0, 0), (1, 0)]), {},
                    {"order:b", "runs:split_by_64"}))
    return out


SHUFFLED_N = (17, 65, 512, 513, 1537)


def fam_shuffled(leaf, offset):
    """One voxel of n points scattered through a background of other voxels' points.  n <= 513: every point of the voxel
    goes into a gap of its own between two background points, so each is a run of one (n runs, exactly); n = 1537: a random
    interleave with 300 background points (path (d) whatever the runs, and a finalize wave of more than kFinStage)."""
    out = []
    for n in SHUFFLED_N:
        rng = _rng(3, n, *_key(leaf, offset))
        nbg = max(300, n + 10) if n <= 513 else 300
        bgv = rng.integers(0, 12, (nbg, 2))
        bgv[(bgv == 5).all(axis=1)] = (6, 5)
        bgv[0], bgv[1] = (0, 0), (11, 11)
        if n <= 513:
            gaps = np.sort(rng.choice(nbg - 1, n, replace=False)) + 1          # in front of background point `gap`
            is_v = np.zeros(nbg + n, bool)
            is_v[gaps + np.arange(n)] = True
        else:
            is_v = np.zeros(nbg + n, bool)
            is_v[rng.choice(nbg + n - 2, n, replace=False) + 1] = True
        vox = np.empty((nbg + n, 2))
        vox[is_v] = (5, 5)
        vox[~is_v] = bgv
        tab = np.array([(5, 5)] + [(k % 12, k // 12) for k in range(144)])
        cloud = _cloud(rng, leaf, offset, np.where(is_v, 0, 1 + (vox[:, 1] * 12 + vox[:, 0]).astype(np.int64)), tab)
        purpose = {17: {"order:b"}, 65: {"order:c", "order:runs65"}, 512: {"order:c", "order:n512"}, 513: {"order:d", "order:n513"},
                   1537: {"order:d", "fin:stream"}}[n]
        out.append(Case("shuffled", "shuffled[%d]" % n, leaf, offset, cloud, {}, purpose))
    return out


def _wave_counts(total):
    head = [1, 7, 8, 9, 16, 17, 0, 2, 3, 4, 5, 6, 10, 11, 12, 13, 14, 15, 23, 24, 25, 31, 32, 33, 40, 41, 47, 48, 49, 0]
    k = WAVE - len(head)
    rest = total - sum(head)
    tail = [rest // k + (1 if i < rest % k else 0) for i in range(k)]
    assert min(tail) > 0
    return head + tail


def fam_wave_m(leaf, offset):
    """A grid row of 128 voxels: voxels 0 .. 63 (one finalize wave) hold exactly kFinStage points, voxels 64 .. 127 exactly
    kFinStage + 1 (the wave streams from memory); the counts run through every remainder modulo 8, 8, 9, 16, 17 and two
    empty voxels.  In random cloud order, min_pts 1 so that every voxel shows.  live[N]: a row of N voxels (the last
    finalize wave partly live)."""
    rng = _rng(4, *_key(leaf, offset))
    counts = _wave_counts(K_FIN_STAGE) + _wave_counts(K_FIN_STAGE + 1)
    vid = rng.permutation(np.repeat(np.arange(128), counts))
    purpose = {"fin:lds", "fin:stream", "fin:m1536", "fin:m1537", "fin:stream_empty", "fin:stream_n8", "fin:stream_n9"} | \
              {"fin:stream_n%%8=%d" % r for r in range(8)}
    out = [Case("wave_m", "wave_m[1536|1537]", leaf, offset, _cloud(rng, leaf, offset, vid, [(i, 0) for i in range(128)]),
                dict(min_pts=1), purpose)]
    for N in (1, 63, 64, 65):
        rng = _rng(4, N, *_key(leaf, offset))
        vid = rng.permutation(np.repeat(np.arange(N), 6 + np.arange(N) % 4))
        out.append(Case("wave_m", "live[%d]" % N, leaf, offset, _cloud(rng, leaf, offset, vid, [(i, 0) for i in range(N)]), {},
                        {"fin:partial_wave" if N % WAVE else "fin:full_wave", "fin:lds"}))
    return out


TILE_GRIDS = ((128, 64), (2731, 3), (1031, 525))       # 8192, 8193 and 541275 voxels (67 scan tiles)


def fam_tiles(leaf, offset):
    """Grids of exactly kScanTile and kScanTile + 1 voxels and one of 67 tiles, empty but for voxels of 20 points (big: they
    enter the list of big voxels, whose position travels through the second look-back) and of 7 points: the first and the
    last voxel of the grid, and the voxels on both sides of tile boundaries."""
    out = []
    for W, H in TILE_GRIDS:
        rng = _rng(5, W, *_key(leaf, offset))
        ng = W * H
        nt = (ng + K_SCAN_TILE - 1) // K_SCAN_TILE
        gs = {}
        for t in sorted({1, nt // 2, nt - 2, nt - 1} - {0}):
            if t < nt:
                b = t * K_SCAN_TILE
                for g, c in ((b - 2, 7), (b - 1, 20), (b, 20), (b + 1, 7), (b + 7, 20), (b + 8, 20)):
                    if 0 <= g < ng:
                        gs.setdefault(g, c)
        for g, c in ((0, 20), (1, 7), (9, 20), (ng - 1, 20), (ng - 2, 7)):
            gs.setdefault(g, c)
        g = np.array(sorted(gs))
        vid = _interleave([gs[k] for k in g], 4)
        cloud = _cloud(rng, leaf, offset, vid, np.stack([g % W, g // W], axis=1))
        purpose = {"scan:ng=%d" % ng if nt <= 2 else "scan:tiles>65", "scan:big_first_tile", "scan:big_last_tile", "order:b", "order:a"}
        if nt > 1:
            purpose |= {"scan:big_straddles", "scan:big_carried"}
        out.append(Case("tiles", "tiles[%dx%d]" % (W, H), leaf, offset, cloud, {}, purpose))
    return out


HOLE_LENGTHS = (1, 63, 64, 65, 129)


def fam_holes(leaf, offset):
    """NaN and +-Inf points in the middle of runs, cloud lengths around the wave size, and points exactly on the lattice:
    float32(k * leaf) on both sides of zero for ALL three leaves, -0.0 and denormals (only at the zero offset: elsewhere
    they would span a grid of 10^9 voxels, so there the lattice points are float32(base + k * leaf)).  min_pts 1: every
    occupied voxel shows, and its count is checked against numpy's float32 floor(x * inv_leaf)."""
    rng = _rng(6, *_key(leaf, offset))
    base, L = FW.lattice_base(leaf, offset)
    pts = []
    bad = [(np.nan, 0.5), (np.inf, 0.5), (0.5, -np.inf), (np.nan, np.nan)]
    for r in range(26):                                     # runs of five points of one voxel, a hole inside every other run
        vx = (r * 3) % 7
        run = _world(leaf, offset, np.tile([(vx, r % 2)], (5, 1)), rng.uniform(0.1, 0.9, (5, 2)))
        run = [tuple(p) for p in run]
        if r % 2 == 0:
            b = bad[(r // 2) % 4]
            run.insert(2, tuple(base[a] + b[a] if np.isfinite(b[a]) else b[a] for a in (0, 1)))
        pts += run
    pts = np.array(pts, dtype=F)
    lat = []
    at_zero = tuple(offset) == (0.0, 0.0)
    for lf in LEAVES:
        for k in (1, 2, 3, 7, 10, 33):
            for s in (1, -1):
                x = F(s * k) * F(lf) if at_zero else F(base[0] + s * k * float(F(lf)))
                y = F(s * k) * F(lf) if at_zero else F(base[1] + s * k * float(F(lf)))
                lat += [(x, F(base[1] + 0.5 * L)), (F(base[0] + 0.5 * L), y), (x, y)]
    if at_zero:
        tiny = F(1e-45)
        lat += [(F(-0.0), F(-0.0)), (F(0.0), F(-0.0)), (tiny, -tiny), (-tiny, tiny), (F(-1e-39), F(1e-39))]
    lat = np.array(lat, dtype=F)
    out = []
    for n in HOLE_LENGTHS:
        cloud = pts[:n].copy()
        purpose = {"runs:padding" if n % WAVE else "runs:full_wave"}
        if n >= 63:
            purpose |= {"runs:hole_mid_run", "runs:head_mid_wave"}
        out.append(Case("holes", "holes[%d]" % n, leaf, offset, cloud, dict(min_pts=1), purpose))
    cloud = np.concatenate([pts[:40], lat, pts[40:]])
    out.append(Case("holes", "holes[lattice]", leaf, offset, cloud, dict(min_pts=1), {"runs:hole_mid_run", "voxel:on_lattice"}))
    return out


LEAF_CASES = ("square", "ellipse_x", "ellipse_y", "ellipse_d", "line_x", "line_y", "line_d", "identical", "ulps", "at_min_pts",
              "below_min_pts")
LEAF_INSENSITIVE = ("identical", "ulps", "below_min_pts")  # one point nine times; sums of nine numbers three steps apart; no cell
EIG_MULTS = (0.01, 0.5, 1.0, 0.0)
# (cov_unbiased, cov_init_identity, eig_mult): every pair of switches, every eig_mult with and without the identity start
LEAF_PARAMS = tuple((ub, idn, em) for ub in (0, 1) for idn in (1, 0) for em in EIG_MULTS)


def leaf_voxel(name):
    """Voxel coordinates of a `leaves` case (one voxel per case, every second voxel of one row)."""
    return (2 * LEAF_CASES.index(name), 0)


def fam_leaves(leaf, offset):
    """One voxel per analytic case of leaf_finalize.  Every coordinate is a whole multiple of `step`, the float32 spacing at
    the far corner of the case's voxel, so the symmetric sets are symmetric EXACTLY (cxx == cyy, cxy == 0, ... as rationals)
    while the points still use every bit of a float32 -- the float32 centroid stays order-sensitive.
      square      24 points invariant under the quarter turn about the centre: cxx == cyy, cxy == 0 (rad == 0)
      ellipse_x   24 points invariant under both reflections, wide in x: cxy == 0, hd > 0;  ellipse_y: hd < 0
      ellipse_d   24 points invariant under x <-> y, long on the diagonal: hd == 0, cxy != 0
      line_x/y/d  12 points exactly collinear;  identical: 9 times one point;  ulps: 9 points within 3 steps
      at_min_pts / below_min_pts: 6 and 5 random points (min_pts 6)"""
    rng = _rng(7, *_key(leaf, offset))
    base, L = FW.lattice_base(leaf, offset)
    def grid_of_case(name):
        """(step per axis, half-extent in steps, centre in steps): the float32 spacing at the far wall of the case's own
        voxel -- one step for both axes where the case is symmetric between x and y, else one per axis (the y of a row
        of voxels is small at the zero offset, and a coarse y would make line_y's sums exact in any order)."""
        v = leaf_voxel(name)
        step = np.array([float(np.spacing(F(max(abs(base[a] + (v[a] + s) * L) for s in (0, 1))))) for a in (0, 1)])
        if name in ("square", "ellipse_d", "line_d"):
            step[:] = step.max()
        res = max(int(0.35 * L / step.max()), 4)
        return step, res, np.array([round((base[a] + (v[a] + 0.5) * L) / step[a]) for a in (0, 1)], dtype=np.int64)

    def ints(n, lo, hi):
        return rng.integers(lo, hi + 1, n)
    def square(res):
        a, b = ints(6, res // 4, res), ints(6, 0, res)
        return np.concatenate([np.stack([a, b], 1), np.stack([-b, a], 1), np.stack([-a, -b], 1), np.stack([b, -a], 1)])

    def ellipse(res):
        a, b = ints(6, res // 2, res), ints(6, res // 4, res // 3)        # l1 / l2 about 0.15: clear of every eig_mult
        return np.concatenate([np.stack([a, b], 1), np.stack([-a, b], 1), np.stack([a, -b], 1), np.stack([-a, -b], 1)])

    def ellipse_d(res):
        t = rng.permutation(np.arange(-6, 6)) * (res // 12) + ints(12, 0, res // 24)   # l1 / l2 about 0.25
        s = ints(12, res // 8, res // 6)
        return np.concatenate([np.stack([t + s, t - s], 1), np.stack([t - s, t + s], 1)])

    def line(res, ax, ay):
        t = rng.permutation(np.arange(-6, 6)) * max(res // 8, 1) + ints(12, 0, max(res // 16, 0))
        return np.stack([t * ax, t * ay], 1)
    makers = (("square", square), ("ellipse_x", ellipse), ("ellipse_y", lambda r: ellipse(r)[:, ::-1]), ("ellipse_d", ellipse_d),
              ("line_x", lambda r: line(r, 1, 0)), ("line_y", lambda r: line(r, 0, 1)), ("line_d", lambda r: line(r, 1, 1)),
              ("identical", lambda r: np.tile([[3, -2]], (9, 1))), ("ulps", lambda r: ints(18, 0, 3).reshape(9, 2)),
              ("at_min_pts", lambda r: ints(12, -r, r).reshape(6, 2)), ("below_min_pts", lambda r: ints(10, -r, r).reshape(5, 2)))
    parts = []
    for name, mk in makers:
        step, res, centre = grid_of_case(name)
        for _ in range(200):                                # (drawn again until order-sensitive, see _cloud; `identical` never is)
            p = (centre + mk(res)) * step[None, :]
            if name in LEAF_INSENSITIVE or order_sensitive(p.astype(F)):
                break
        else:
            raise AssertionError("no order-sensitive draw for " + name)
        parts.append((name, p))
    counts = [len(p) for _, p in parts]
    vid = _interleave(counts, 3)
    nxt = [0] * len(parts)
    rows = []
    for k in vid:
        name, p = parts[k]
        rows.append(p[nxt[k]])
        nxt[k] += 1
    cloud = np.array(rows, dtype=np.float64).astype(F)
    assert np.array_equal(cloud.astype(np.float64), np.array(rows)), "the leaves cloud must be exact in float32"
    out = []
    for ub, idn, em in LEAF_PARAMS:
        prm = dict(cov_unbiased=ub, cov_init_identity=idn, eig_mult=em)
        purpose = {"leaf:unbiased=%d" % ub, "leaf:identity=%d" % idn, "leaf:rad=0", "leaf:hd>0", "leaf:hd<0", "leaf:hd=0,cxy!=0",
                   "leaf:below_min_pts"}
        out.append(Case("leaves", "leaves[ub=%d,id=%d,em=%g]" % (ub, idn, em), leaf, offset, cloud, prm, purpose))
    return out


FAMILIES = dict(sizes=fam_sizes, runs_k=fam_runs_k, shuffled=fam_shuffled, wave_m=fam_wave_m, tiles=fam_tiles, holes=fam_holes,
                leaves=fam_leaves)
_CASES = {}


def cases(leaf, offset, family=None):
    """Every case of one (leaf, offset), built once."""
    key = (leaf, tuple(offset))
    if key not in _CASES:
        _CASES[key] = [c for f in FAMILIES.values() for c in f(leaf, tuple(offset))]
    return [c for c in _CASES[key] if family is None or c.family == family]


# ------------------------------------------------------------------------------------------ the voxels of a cloud
Table = namedtuple("Table", "grid key members")


def voxel_table(cloud, leaf):
    """The grid and, per occupied voxel index, the numbers of its points in cloud order -- from numpy's float32
    floor(x * inv_leaf) alone (inv_leaf = 1.0f / leaf); key is -1 for a point with a non-finite coordinate."""
    c = np.ascontiguousarray(cloud, dtype=F).reshape(-1, 2)
    fin = np.isfinite(c).all(axis=1)
    G = FW.grid_of(c[fin], leaf)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.floor(np.where(fin[:, None], c, 0) * G.inv).astype(np.int64)
    key = np.where(fin, (v[:, 1] - G.min_by) * G.div_x + (v[:, 0] - G.min_bx), -1)
    order = np.argsort(key, kind="stable")
    sk = key[order]
    cut = np.flatnonzero(np.diff(sk)) + 1
    members = {int(sk[s]): order[s:e] for s, e in zip(np.concatenate([[0], cut]), np.concatenate([cut, [len(sk)]])) if sk[s] >= 0}
    return Table(G, key, members)


# ------------------------------------------------------------------------------------------ the path census
ORDER_PATHS = ("order:a", "order:b", "order:c", "order:d")
ALL_PATHS = ORDER_PATHS + (
    "order:n16", "order:n17", "order:runs64", "order:runs65", "order:n512", "order:n513",
    "order:a_n%4=0", "order:a_n%4=1", "order:a_n%4=2", "order:a_n%4=3",
    "runs:head_mid_wave", "runs:hole_mid_run", "runs:padding", "runs:full_wave", "runs:split_by_64", "voxel:on_lattice",
    "scan:ng=8192", "scan:ng=8193", "scan:tiles>65", "scan:big_first_tile", "scan:big_last_tile", "scan:big_straddles", "scan:big_carried",
    "fin:lds", "fin:stream", "fin:m1536", "fin:m1537", "fin:stream_empty", "fin:stream_n8", "fin:stream_n9", "fin:partial_wave",
    "fin:full_wave") + tuple("fin:stream_n%%8=%d" % r for r in range(8))
ALL_LEAF = ("leaf:unbiased=0", "leaf:unbiased=1", "leaf:identity=0", "leaf:identity=1", "leaf:rad=0", "leaf:hd>0", "leaf:hd<0",
            "leaf:hd=0,cxy!=0", "leaf:z_first", "leaf:z_mid", "leaf:z_last", "leaf:reject", "leaf:accept", "leaf:raise1",
            "leaf:raise2", "leaf:singular", "leaf:below_min_pts")


def run_bounds(nums):
    """(cloud_runs, wave_runs) of the ascending point numbers of one voxel: the interval the run count of its segment of
    `perm` lies in (module docstring)."""
    d = np.diff(nums)
    cloud_runs = 1 + int((d != 1).sum())
    wave_runs = 1 + int(((d != 1) | (nums[1:] % WAVE == 0)).sum())
    return cloud_runs, wave_runs


def order_path(n, cloud_runs, wave_runs):
    """The path map_order_kernel must take for a voxel, or None where the run count straddles kBigRuns."""
    if n <= K_BIG_VOXEL:
        return "order:a"
    if n > K_BIG_STAGE:
        return "order:d"
    if wave_runs <= K_BIG_RUNS:
        return "order:b"
    if cloud_runs > K_BIG_RUNS:
        return "order:c"
    return None


def paths_of(cloud, leaf):
    """-> (table, {label: sorted voxel indices}) -- which voxels of a build of `cloud` must take which path; labels that
    describe the whole cloud carry the voxel list [-1].  From the cloud alone."""
    T = voxel_table(cloud, leaf)
    ng = T.grid.div_x * T.grid.div_y
    n_pts = len(T.key)
    got = {}

    def hit(label, g=-1):
        got.setdefault(label, []).append(int(g))
    counts = {g: len(m) for g, m in T.members.items()}
    for g, m in T.members.items():
        n = len(m)
        cr, wr = run_bounds(m)
        p = order_path(n, cr, wr)
        if p:
            hit(p, g)
        if p == "order:a":
            hit("order:a_n%%4=%d" % (n % 4), g)
        if n in (16, 17, 512, 513):
            hit("order:n%d" % n, g)
        if K_BIG_VOXEL < n <= K_BIG_STAGE and cr == wr and cr in (64, 65):
            hit("order:runs%d" % cr, g)
        if wr > cr:
            hit("runs:split_by_64", g)
    # wave_runs(): the lanes of every aligned chunk of 64 points
    hit("runs:padding" if n_pts % WAVE else "runs:full_wave")
    for s in range(0, n_pts, WAVE):
        k = T.key[s:s + WAVE]
        if len(k) > 1 and (k[1:] != k[:-1]).any():
            hit("runs:head_mid_wave")
        neg = np.flatnonzero(k < 0)
        if any(0 < i < len(k) - 1 and k[i - 1] >= 0 and k[i - 1] == k[i + 1] for i in neg):
            hit("runs:hole_mid_run")
    c32 = np.ascontiguousarray(cloud, dtype=F).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = c32 * T.grid.inv
        if ((scaled == np.floor(scaled)) & (T.key >= 0)[:, None]).any():      # a coordinate exactly on a wall of its voxel
            hit("voxel:on_lattice")
    # the scan: tiles of kScanTile voxels
    nt = (ng + K_SCAN_TILE - 1) // K_SCAN_TILE
    if ng in (K_SCAN_TILE, K_SCAN_TILE + 1):
        hit("scan:ng=%d" % ng)
    if nt > 65:
        hit("scan:tiles>65")
    big = sorted(g for g, c in counts.items() if c > K_BIG_VOXEL)
    for g in big:
        t = g // K_SCAN_TILE
        if t == 0:
            hit("scan:big_first_tile", g)
        if t == nt - 1:
            hit("scan:big_last_tile", g)
        if t > 0 and big[0] // K_SCAN_TILE < t:
            hit("scan:big_carried", g)
        if g % K_SCAN_TILE == K_SCAN_TILE - 1 and counts.get(g + 1, 0) > K_BIG_VOXEL:
            hit("scan:big_straddles", g)
    # map_finalize: a wave is 64 consecutive voxel indices, aligned
    if ng % WAVE:
        hit("fin:partial_wave")
    else:
        hit("fin:full_wave")
    waves = {}
    for g, c in counts.items():
        waves[g // WAVE] = waves.get(g // WAVE, 0) + c
    for w, m in waves.items():
        streamed = m > K_FIN_STAGE
        if m in (K_FIN_STAGE, K_FIN_STAGE + 1):
            hit("fin:m%d" % m)
        live = range(w * WAVE, min((w + 1) * WAVE, ng))
        for g in live:
            c = counts.get(g, 0)
            if c:
                hit("fin:stream" if streamed else "fin:lds", g)
            if streamed and c:
                hit("fin:stream_n%%8=%d" % (c % 8), g)
                if c in (8, 9):
                    hit("fin:stream_n%d" % c, g)
            if streamed and not c:
                hit("fin:stream_empty")
    return T, {k: sorted(v) for k, v in got.items()}


# ------------------------------------------------------------------------------------------ order sensitivity ("teeth")
def sums_in_order(p32):
    """What a voxel IS in the build: the float32 centroid sums and the fp64 sums of its points added up in the given order,
    as bytes."""
    p = np.ascontiguousarray(p32, dtype=F).reshape(-1, 2)
    f = np.cumsum(p, axis=0, dtype=F)[-1]
    d = p.astype(np.float64)
    prod = np.stack([d[:, 0], d[:, 1], d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 1] * d[:, 1]], axis=1)
    return f.tobytes() + np.cumsum(prod, axis=0)[-1].tobytes()


def order_sensitive(p32):
    """True when the reverse order and eight seeded random orders of the points EACH change a bit of `sums_in_order`.  An
    order that only swaps the first two points adds the same numbers in the same tree (addition commutes) and is drawn
    again; a voxel of fewer than three points has no other order and is never sensitive."""
    p = np.ascontiguousarray(p32, dtype=F).reshape(-1, 2)
    n = len(p)
    if n < 3:
        return False
    want = sums_in_order(p)
    rng = _rng(8, n)                                        # (the same orders for every voxel of n points)
    others = [np.arange(n)[::-1]]
    while len(others) < 9:
        o = rng.permutation(n)
        if not (set(o[:2].tolist()) == {0, 1} and np.array_equal(o[2:], np.arange(2, n))):
            others.append(o)
    return all(sums_in_order(p[o]) != want for o in others)


# ------------------------------------------------------------------------------------------ the exact reference
getcontext().prec = 80
Exact = namedtuple("Exact", "n decision mean icov l1 l2 czz thr kappa labels decided margin")


def _dec(fr):
    return Decimal(fr.numerator) / Decimal(fr.denominator)


def _exact_sum(values):
    """The exact sum of float64 values (each a dyadic rational) as a Fraction: integer arithmetic on a common scale."""
    num, den = 0, 1
    for v in values:
        a, b = float(v).as_integer_ratio()
        if b > den:
            num *= b // den
            den = b
        num += a * (den // b)
    return Fraction(num, den)


def exact_leaf(points32, prm, r2=None):
    """Mean, covariance (PCL's formula), the decision and the inverse covariance of one voxel in exact arithmetic.
    Sums and the covariance: fractions.Fraction (float32 inputs are exact rationals).  In-plane eigenvalues: tr -+ rad, rad
    the square root of the rational hd^2 + cxy^2 as an 80-digit Decimal.  z eigenvalue: czz, exact.
      decision  'below' (n < min_pts: no cell), 'reject', 'accept', 'raise1', 'raise2' (how many of the two smallest of
                {l1, l2, czz} lie below eig_mult * largest), 'singular' (kept, but the regularised 2 x 2 block has a zero
                eigenvalue: no inverse exists)
      icov      (xx, xy, yy) as floats rounded from the Decimal result, or None
      decided   l1 is further than `margin` from 0 and from the threshold, l2 further than `margin` from the threshold,
                margin = 16 n ulp(r2) (r2: the largest x^2 + y^2 of the CLOUD, default of the voxel): the rounding the
                one-pass covariance can commit cannot flip the decision.  czz and a threshold that is a multiple of the
                compared eigenvalue itself are exact on both sides and are not judged.
    No numpy linear algebra, nothing shared with the oracle."""
    p = np.ascontiguousarray(points32, dtype=F).reshape(-1, 2)
    n = len(p)
    P = params_of(prm)
    if n < P["min_pts"]:
        return Exact(n, "below", None, None, None, None, None, None, None, ("leaf:below_min_pts",), True, 0.0)
    x, y = p[:, 0].astype(np.float64), p[:, 1].astype(np.float64)
    sx, sy = _exact_sum(x), _exact_sum(y)
    ident = Fraction(1 if P["cov_init_identity"] else 0)
    sxx = _exact_sum(x * x) + ident                        # (the product of two float32 is exact in fp64)
    syy = _exact_sum(y * y) + ident
    sxy = _exact_sum(x * y)
    szz = ident
    N = Fraction(n)
    mx, my = sx / N, sy / N
    labels = ["leaf:unbiased=%d" % P["cov_unbiased"], "leaf:identity=%d" % P["cov_init_identity"]]
    if P["cov_unbiased"]:
        if n == 1:
            return Exact(n, "undefined", (float(mx), float(my)), None, None, None, None, None, None, tuple(labels), False, 0.0)
        cxx, cxy, cyy, czz = (sxx - sx * mx) / (N - 1), (sxy - sy * mx) / (N - 1), (syy - sy * my) / (N - 1), szz / (N - 1)
    else:
        f = (N - 1) / N
        cxx, cxy, cyy, czz = (sxx / N - mx * mx) * f, (sxy / N - mx * my) * f, (syy / N - my * my) * f, szz / N * f
    hd, tr = (cxx - cyy) / 2, (cxx + cyy) / 2
    rad2 = hd * hd + cxy * cxy
    rad = _dec(rad2).sqrt()
    det = cxx * cyy - cxy * cxy                            # l1 * l2: its sign and zero are exact
    l2 = _dec(tr) + rad
    l1 = l2 if rad2 == 0 else Decimal(0) if det == 0 else _dec(det) / l2       # (no cancellation: l1 l2 = det)
    z = _dec(czz)
    # czz against l1 = tr - rad and l2 = tr + rad, exactly, without the square root.  For a planar cloud czz is the identity
    # start's share, which cxx and cyy hold as well: czz <= l1 always, and the other two orderings of leaf_finalize can only
    # be reached through rounding (identical points far from the origin)
    z_le_l1 = tr - czz >= 0 and (tr - czz) ** 2 >= rad2
    z_le_l2 = czz - tr <= 0 or (czz - tr) ** 2 <= rad2
    if rad2 == 0:
        labels.append("leaf:rad=0")
    elif hd > 0:
        labels.append("leaf:hd>0")
    elif hd < 0:
        labels.append("leaf:hd<0")
    else:
        labels.append("leaf:hd=0,cxy!=0")
    labels.append("leaf:z_first" if z_le_l1 else "leaf:z_mid" if z_le_l2 else "leaf:z_last")
    ev = sorted([l1, l2, z])
    r2 = float((x * x + y * y).max()) if r2 is None else r2
    margin = 16.0 * n * float(np.spacing(r2))
    em = Decimal(Fraction(P["eig_mult"]).numerator) / Decimal(Fraction(P["eig_mult"]).denominator)
    thr = em * ev[2]
    mean = (float(mx), float(my))
    m = Decimal(margin)
    if ev[2] <= 0:
        labels.append("leaf:reject")
        # everything is zero exactly: identical points without the identity start, where a rounding residue of either sign
        # decides -- or ONE point under the (n - 1) / n normalisation, whose factor is an exact zero on every side
        return Exact(n, "reject", mean, None, float(l1), float(l2), float(z), 0.0, None, tuple(labels),
                     n == 1 and not P["cov_unbiased"], margin)
    z_is_top = not z_le_l2
    decided = abs(l1) > m and abs(l1 - thr) > m * (1 + (0 if z_is_top else em))
    if z_is_top:
        decided = decided and abs(l2 - thr) > m
    raised = int(ev[0] < thr) + int(ev[0] < thr and ev[1] < thr)
    n1, n2 = max(l1, thr), max(l2, thr)
    if n1 == 0:
        labels += ["leaf:singular"]
        return Exact(n, "singular", mean, None, float(l1), float(l2), float(z), float(thr), None, tuple(labels), False, margin)
    decision = ("accept", "raise1", "raise2")[raised]
    labels += ["leaf:accept"] + (["leaf:" + decision] if raised else [])
    # icov = P1 / n1 + P2 / n2 with the spectral projectors of the exact covariance (isotropic: I / n1)
    if rad2 == 0:
        ic = (1 / n1, Decimal(0), 1 / n1)
    else:
        gap = l2 - l1
        p2xx, p2xy, p2yy = (_dec(cxx) - l1) / gap, _dec(cxy) / gap, (_dec(cyy) - l1) / gap
        ic = ((1 - p2xx) / n1 + p2xx / n2, -p2xy / n1 + p2xy / n2, (1 - p2yy) / n1 + p2yy / n2)
    return Exact(n, decision, mean, tuple(float(v) for v in ic), float(l1), float(l2), float(z), float(thr), float(n2 / n1),
                 tuple(labels), bool(decided), margin)


# The rounding of the oracle's (and the device's) fp64 route from the covariance to its inverse, by counting operations,
# u = 2^-53 each: hd, tr (2), rad (5), l1, l2 (2), the eigenvector and its norm (8), the rebuilt covariance (13), the
# determinant (3) and the quotients (3): 36.  The subtractions tr - rad and cxx cyy - cxy^2 cancel to 1 / kappa of their
# operands (kappa: largest over smallest in-plane eigenvalue of the regularised covariance), which multiplies the
# relative error by kappa.
REBUILD_OPS = 36


def icov_bound(ex, r2):
    """|icov_c - exact| allowed per entry: (n ulp(r2) max|icov| + REBUILD_OPS 2^-53 kappa) max|icov|."""
    big = max(abs(v) for v in ex.icov)
    return (ex.n * float(np.spacing(r2)) * big + REBUILD_OPS * 2.0 ** -53 * max(ex.kappa, 1.0)) * big


def mean_bound(ex):
    """n ulps of the exact mean, per coordinate."""
    return tuple(ex.n * float(np.spacing(abs(v))) for v in ex.mean)


_EXACT = {}


def exact_cells(case):
    """{voxel index: Exact} of every occupied voxel of a case, and the cloud's r2; computed once per case."""
    key = (case.name, case.leaf, case.offset)
    if key not in _EXACT:
        T = voxel_table(case.cloud, case.leaf)
        c = case.cloud[np.isfinite(case.cloud).all(axis=1)].astype(np.float64)
        r2 = float((c ** 2).sum(axis=1).max())
        _EXACT[key] = (T, {g: exact_leaf(case.cloud[m], case.prm, r2) for g, m in T.members.items()}, r2)
    return _EXACT[key]


def on_cloud_scan(case, n=256):
    """A scan and a pose for one evaluation on the cloud: every k-th finite point relative to the lattice base, and the pose
    that puts it back a fraction of a voxel beside where it was."""
    base, L = FW.lattice_base(case.leaf, case.offset)
    c = case.cloud[np.isfinite(case.cloud).all(axis=1)]
    c = c[np.abs(c.astype(np.float64) - base[None, :]).max(axis=1) < 1e5]
    k = max(len(c) // n, 1)
    scan = (c[::k].astype(np.float64) - base[None, :]).astype(F)
    return scan, np.array([base[0] + 0.21 * L, base[1] - 0.13 * L, 0.0])
