"""Map / scan pairs and a census for the LDS window of the match kernel (ndt_match.hip.h: region_from_bbox,
fill_window_plan, fill_window_fetch, pass_units; ndt_point.hip.h: eval_point).  Tests only: tests/test_match_window_host.py
(CPU) and tests/test_gpu_match_window_geometry.py import it.

In the match kernel a point's derivative terms come from one of two data paths: slot numbers, centroids and 48-byte records
staged in LDS (fast), or the same arithmetic on the dense grid in HBM (slow: the point lies in the window's outer ring or
outside it, or one of its nine voxels is occupied and has no LDS record).  Every family below is a small (map cloud, scan,
initial guess, parameters) aimed at named edges of that choice; `window_census` restates, in numpy integers and sharing no
code with the device or the oracle, what the set-up decides at the first pose: the window, the record capacity, the
marked cells and their word-wise dilation, kept / skipped / nspill / clipped, and the path of every point; `pairs_at`
counts the (point, voxel) pairs of a pass from the exported float32 centroids.

What is "occupied".  map_finalize_kernel (ndt_map_build.hip.h) sets a voxel's bit in the occupancy words exactly when
write_voxel returns non-zero, i.e. when the voxel holds at least min_pts points -- whether leaf_finalize then accepts the
covariance or not (a rejected voxel keeps its bit, its count is exported negative).  That is the set ndt_map_export lists
in `idx`, so the census takes the grid from Map.info() and the occupied set from export()["idx"] of the ORACLE's map.

The first pose.  Every initial guess but those of `walk` has yaw 0: the float32 matrix is exactly (1, 0, tx, ty) and the
census transforms in numpy float32, operation for operation as tf_apply_t does in the case's transform_sse form.  `walk`
needs a yaw; its float32 cosine and sine are numpy's, and every family keeps every finite transformed point FACE_MARGIN of
a leaf away from the voxel faces (test_match_window_host.py asserts it), so one ulp in cos or sin moves no point into
another voxel.  `radius_tie` instead places its points at voxel centres, exactly.

The dilation.  fill_window_plan dilates the marked-cell bitmap by two cells on 32-bit words of the row-major cell string.
Rows are not word aligned and nothing masks the row ends, so a mark in the first (last) two columns of the window also
reaches the last (first) two columns of the row before (after) it.  `dilate_words` does the same on the same words.  A
mark can only sit in those columns when the window was cut down in x, which needs a box wider than 128 cells: the leak is
reachable at rw = 128 alone (`row_phase[128c]`); at the other widths of `row_phase` the marks sit in the first and last
two columns of the BOX, five cells inside the window, as near the row ends as region_from_bbox lets a mark come.

grid_margin.  The oracle ignores ndt_params::grid_margin (its grid is always the cloud's box), the device widens its grid
by it.  The window is laid out in absolute voxel coordinates, so the census of a `grid_edge` case is the same for both
margins; the device's records must be byte-identical across them.
"""
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import map_build_workloads as MB  # noqa: E402

F = np.float32
# the constants of ndt_point.hip.h / ndt_match.hip.h the families aim at
K_REGION_MARGIN, K_REGION_CELLS, K_POOL_BYTES, CELL_ENTRY_BYTES = 5, 16384, 147 * 1024, 48
K_BLOCK, K_SUB, K_SORT_REGS, K_WORDS = 1024, 4, 10 * 1024, 16384 // 32
FLAG_WINDOW_SPILL, FLAG_REGION_CLIPPED = 1, 2
FACE_MARGIN = 1e-3
FAST, RING, NONRES = 0, 1, 2            # a point's path at the first pose (non-finite points count as RING: outside every window)

Case = namedtuple("Case", "family name cloud scan init prm expect")
Grid = namedtuple("Grid", "min_bx min_by div_x div_y")
Census = namedtuple("Census", "region cap clipped clip kept skipped nspill flags marked occ keep resident leaked path vox finite "
                              "cells_off_grid nonres_grid")

DEFAULTS = dict(resolution=0.5, max_iter=3, stale_h_ang=0)


def params_of(case, mod):
    """ndt_params of a case from capi or the oracle module."""
    p = dict(DEFAULTS)
    p.update(case.prm)
    return mod.default_params(**p)


def _rng(*key):
    return np.random.Generator(np.random.Philox(np.random.SeedSequence([20250607] + [int(k) & 0xFFFF for k in key])))


# ------------------------------------------------------------------------------------------ the census
def first_matrix(pose):
    """(c, s, tx, ty) in float32 of a pose (tx, ty, yaw): exact for yaw 0; else numpy's cosine and sine of the float32 yaw."""
    yaw = F(pose[2])
    if yaw == 0:
        c, s = F(1.0), F(0.0)
    else:
        c, s = F(np.cos(np.float64(yaw))), F(np.sin(np.float64(yaw)))
    return c, s, F(pose[0]), F(pose[1])


def transform(T, scan, sse):
    """tf_apply_t in numpy float32: every product and every sum rounded once, in the order of the transform_sse form."""
    c, s, tx, ty = T
    p = np.ascontiguousarray(scan, dtype=F).reshape(-1, 2)
    x, y = p[:, 0], p[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        a, b, cc, d = c * x, F(-s) * y, s * x, c * y
        if sse:
            return a + (b + tx), cc + (d + ty)
        return (a + b) + tx, (cc + d) + ty


def voxel_coord(x, leaf):
    """floor(x * inv_leaf) in float32 clamped to +-1e9, NaN -> -1e9, as an int64 (inv_leaf = 1.0f / leaf)."""
    inv = F(1.0) / F(leaf)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(np.asarray(x, dtype=F) * inv)
    f = np.where(np.isnan(f), F(-1.0e9), np.minimum(np.maximum(f, F(-1.0e9)), F(1.0e9)))
    return f.astype(np.int64)


def face_margin(x, leaf):
    """Distance of float32 coordinates to the nearest voxel face, in leaves (float64 arithmetic on the float32 values)."""
    t = np.asarray(x, dtype=np.float64) * float(F(1.0) / F(leaf))
    fr = t - np.floor(t)
    return np.minimum(fr, 1.0 - fr)


def region_from_bbox(bbox, sensor):
    """(x0, y0, rw, rh), clipped, labels: the window of a voxel bounding box (xmin, ymin, xmax, ymax; grid-relative) and the
    sensor's voxel, as region_from_bbox in ndt_match.hip.h.  bbox None (no finite point): an empty window."""
    if bbox is None:
        return (0, 0, 0, 0), 0, ()
    x0, x1 = bbox[0] - K_REGION_MARGIN, bbox[2] + K_REGION_MARGIN
    y0, y1 = bbox[1] - K_REGION_MARGIN, bbox[3] + K_REGION_MARGIN
    w, h = x1 - x0 + 1, y1 - y0 + 1
    clipped, labels = 0, []
    if w * h > K_REGION_CELLS:
        clipped = 1
        w2 = min(w, 128)
        h2 = K_REGION_CELLS // w2
        labels.append("w>128" if w > 128 else "w<=128")
        if h2 > h:
            h2 = h
            labels.append("h2=h")
        elif h > 128 and w > 128:
            labels.append("h>128")
        cx0, cy0 = sensor[0] - w2 // 2, sensor[1] - h2 // 2
        for name, c, lo, hi in (("x", cx0, x0, x1 - w2 + 1), ("y", cy0, y0, y1 - h2 + 1)):
            if c < lo:
                labels.append("c%s0<%s0" % (name, name))
            elif c > hi:
                labels.append("c%s0>%s1" % (name, name))
        x0 = x0 if cx0 < x0 else min(cx0, x1 - w2 + 1)
        y0 = y0 if cy0 < y0 else min(cy0, y1 - h2 + 1)
        w, h = w2, h2
    far = 1 << 30
    x0, y0 = min(max(x0, -far), far), min(max(y0, -far), far)
    return (int(x0), int(y0), int(w), int(h)), clipped, tuple(labels)


def cap_of(rw, rh):
    """Record slots of the pool beside the slot table: kPoolBytes, 2 bytes per cell rounded up to 16, 48-byte records, two
    sentinels."""
    slot_bytes = ((rw * rh * 2 + 15) // 16) * 16
    return min((K_POOL_BYTES - slot_bytes) // CELL_ENTRY_BYTES - 2, 0xFFF0)


def pack_words(bits):
    """bool per cell (row-major) -> the K_WORDS 32-bit words of the window's bitmaps: bit k of word i is cell 32 i + k."""
    b = np.zeros(K_REGION_CELLS, np.uint8)
    bits = np.asarray(bits, dtype=bool).ravel()
    b[:len(bits)] = bits
    return np.packbits(b, bitorder="little").view("<u4").astype(np.uint32)


def unpack_words(words, ncell):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")[:ncell].astype(bool)


def _at(a, off):
    """a[i + off] for every i, zero outside the array (word_at of fill_window_plan)."""
    out = np.zeros_like(a)
    n = len(a)
    if off == 0:
        out[:] = a
    elif 0 < off < n:
        out[:n - off] = a[off:]
    elif -n < off < 0:
        out[-off:] = a[:n + off]
    return out


def dilate_words(wmap, rw):
    """The marked-cell words dilated by two cells in x and in y as fill_window_plan does it: shifts of whole 32-bit words
    with the neighbouring words' bits carried in, rows one after the other in one cell string -- the row-end leak included."""
    M = np.uint64(0xFFFFFFFF)
    w = np.asarray(wmap, dtype=np.uint64)
    s = lambda k: np.uint64(k)
    pv, nx = _at(w, -1), _at(w, 1)
    dx = (w | (w << s(1)) | (w << s(2)) | (w >> s(1)) | (w >> s(2)) | (pv >> s(31)) | (pv >> s(30)) | (nx << s(31)) | (nx << s(30))) & M
    k = dx.copy()
    for m in (1, 2):
        sft = m * rw
        q, b = sft >> 5, sft & 31
        k |= (_at(dx, -q) << s(b)) & M
        k |= _at(dx, q) >> s(b)
        if b:
            k |= _at(dx, -q - 1) >> s(32 - b)
            k |= (_at(dx, q + 1) << s(32 - b)) & M
    return k.astype(np.uint32)


def dilate_2d(marked, rw, rh):
    """The dilation one would draw: Chebyshev distance two inside the window, nothing across row ends."""
    m = np.asarray(marked, dtype=bool).reshape(rh, rw)
    pad = np.zeros((rh + 4, rw + 4), bool)
    pad[2:-2, 2:-2] = m
    out = np.zeros((rh, rw), bool)
    for dy in range(5):
        for dx in range(5):
            out |= pad[dy:dy + rh, dx:dx + rw]
    return out


def plan(marked, occ, rw, rh):
    """(keep, kept, skipped, nspill, resident) of a window from its marked and occupied cells (row-major bools)."""
    ncell = rw * rh
    keep_w = dilate_words(pack_words(marked), rw) & pack_words(occ)
    keep = unpack_words(keep_w, ncell)
    occ = np.asarray(occ, dtype=bool).ravel()
    kept, skipped = int(keep.sum()), int((occ & ~keep).sum())
    cap = cap_of(rw, rh)
    nspill = skipped + max(kept - cap, 0)
    resident = keep & (np.cumsum(keep) - 1 < cap)
    return keep, kept, skipped, nspill, resident


def occupancy_grid(grid, occupied):
    g = np.zeros(grid.div_x * grid.div_y, bool)
    g[np.asarray(occupied, dtype=np.int64)] = True
    return g.reshape(grid.div_y, grid.div_x)


def voxels_at(grid, pose, scan, prm):
    """(ix, iy grid-relative int64, finite, xt, yt) of a scan at a pose, in the case's transform form."""
    xt, yt = transform(first_matrix(pose), scan, bool(prm.get("transform_sse", 1)))
    leaf = prm.get("resolution", DEFAULTS["resolution"])
    fin = np.isfinite(xt) & np.isfinite(yt)
    return voxel_coord(xt, leaf) - grid.min_bx, voxel_coord(yt, leaf) - grid.min_by, fin, xt, yt


def _touches(mask2d, ix, iy):
    """Per point: does the 3 x 3 neighbourhood of (ix, iy) hold a set cell of mask2d (cells outside it are clear)?"""
    h, w = mask2d.shape
    wide = np.zeros((h + 2, w + 2), bool)           # wide[j + 1, i + 1]: any of mask2d[j - 1 .. j + 1, i - 1 .. i + 1], for i, j from -1 on
    for dy in range(3):
        for dx in range(3):
            wide[dy:dy + h, dx:dx + w] |= mask2d
    ok = (ix >= -1) & (ix <= w) & (iy >= -1) & (iy <= h)
    out = np.zeros(len(ix), bool)
    out[ok] = wide[iy[ok] + 1, ix[ok] + 1]
    return out


def window_census(grid, occupied, scan, init, prm):
    """What the match kernel's set-up decides for (scan, init) on a map with `grid` (min_bx, min_by, div_x, div_y) and the
    occupied voxel indices `occupied` (iy * div_x + ix); prm: the case's parameter dict (resolution, transform_sse)."""
    grid = Grid(int(grid.min_bx), int(grid.min_by), int(grid.div_x), int(grid.div_y))
    leaf = prm.get("resolution", DEFAULTS["resolution"])
    ix, iy, fin, _, _ = voxels_at(grid, init, scan, prm)
    bbox = (int(ix[fin].min()), int(iy[fin].min()), int(ix[fin].max()), int(iy[fin].max())) if fin.any() else None
    T = first_matrix(init)
    sensor = (int(voxel_coord(T[2], leaf)) - grid.min_bx, int(voxel_coord(T[3], leaf)) - grid.min_by)
    (x0, y0, rw, rh), clipped, labels = region_from_bbox(bbox, sensor)
    cap = cap_of(rw, rh)
    occ_grid = occupancy_grid(grid, occupied)
    lx, ly = ix - x0, iy - y0
    inside = fin & (lx >= 0) & (lx < rw) & (ly >= 0) & (ly < rh)
    marked = np.zeros((rh, rw), bool)
    marked[ly[inside], lx[inside]] = True
    # the window's cells in the grid
    gx, gy = x0 + np.arange(rw), y0 + np.arange(rh)
    okx, oky = (gx >= 0) & (gx < grid.div_x), (gy >= 0) & (gy < grid.div_y)
    occ = np.zeros((rh, rw), bool)
    if okx.any() and oky.any():
        occ[np.ix_(oky, okx)] = occ_grid[np.ix_(gy[oky], gx[okx])]
    cells_off_grid = rw * rh - int(okx.sum()) * int(oky.sum())
    keep, kept, skipped, nspill, resident = plan(marked, occ, rw, rh)
    keep, resident = keep.reshape(rh, rw), resident.reshape(rh, rw)
    leaked = int((keep & ~dilate_2d(marked, rw, rh)).sum())
    flags = (FLAG_WINDOW_SPILL if nspill > 0 else 0) | (FLAG_REGION_CLIPPED if clipped else 0)
    if len(scan) == 0:
        flags = 0
    # occupied voxels of the grid without an LDS record (outside the window, or left out of it)
    nonres_grid = occ_grid.copy()
    if okx.any() and oky.any():
        sub = nonres_grid[np.ix_(gy[oky], gx[okx])]
        sub &= ~resident[np.ix_(oky, okx)]
        nonres_grid[np.ix_(gy[oky], gx[okx])] = sub
    inwin = fin & (lx >= 1) & (lx <= rw - 2) & (ly >= 1) & (ly <= rh - 2)
    path = np.full(len(ix), RING, np.int8)
    touch = _touches(occ & ~resident, lx, ly)
    path[inwin & touch] = NONRES
    path[inwin & ~touch] = FAST
    return Census((x0, y0, rw, rh), cap, clipped, labels, kept, skipped, nspill, flags, marked, occ, keep, resident, leaked, path,
                  np.stack([ix, iy], axis=1), fin, cells_off_grid, nonres_grid)


def slow_points_at(grid, census, pose, scan, prm, margin=FACE_MARGIN):
    """Points of `scan` at `pose` (any yaw) that are certain to leave the fast path because their 3 x 3 neighbourhood holds an
    occupied voxel without an LDS record: only points at least `margin` leaves from every voxel face count."""
    leaf = prm.get("resolution", DEFAULTS["resolution"])
    ix, iy, fin, xt, yt = voxels_at(grid, pose, scan, prm)
    sure = fin & (face_margin(np.where(fin, xt, 0), leaf) >= margin) & (face_margin(np.where(fin, yt, 0), leaf) >= margin)
    return sure & _touches(census.nonres_grid, ix, iy)


def pairs_at(grid, export, pose, scan, prm, voxels=None):
    """Per point: the number of (point, voxel) pairs of a derivative pass at `pose` -- voxels of the 3 x 3 neighbourhood of the
    point's own voxel whose float32 centroid (export["cent"]) lies inside the radius, flann's float32 ex * ex + ey * ey against
    r2 = (float) (res * res), `<=` with radius_inclusive -- counted over all occupied voxels or over the indices `voxels` only."""
    leaf = prm.get("resolution", DEFAULTS["resolution"])
    ix, iy, fin, xt, yt = voxels_at(grid, pose, scan, prm)
    idx = np.asarray(export["idx"], dtype=np.int64)
    cent = np.asarray(export["cent"], dtype=F)
    if voxels is not None:
        pick = np.isin(idx, np.asarray(voxels, dtype=np.int64))
        idx, cent = idx[pick], cent[pick]
    vx, vy = idx % grid.div_x, idx // grid.div_x
    r2 = F(float(leaf) * float(leaf))
    out = np.zeros(len(ix), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, len(ix), 1024):
            e = slice(s, s + 1024)
            ex, ey = xt[e, None] - cent[None, :, 0], yt[e, None] - cent[None, :, 1]
            dd = ex * ex + ey * ey
            near = (np.abs(ix[e, None] - vx[None, :]) <= 1) & (np.abs(iy[e, None] - vy[None, :]) <= 1) & fin[e, None]
            out[e] = (near & ((dd <= r2) if prm.get("radius_inclusive", 0) else (dd < r2))).sum(axis=1)
    return out


def path_counts(census):
    return {k: int((census.path == v).sum()) for k, v in (("fast", FAST), ("ring", RING), ("nonres", NONRES))}


# ------------------------------------------------------------------------------------------ building blocks
def _uniq(vox):
    return np.unique(np.asarray(vox, dtype=np.int64).reshape(-1, 2), axis=0)


def _block(xa, xb, ya, yb):
    """Voxels xa .. xb by ya .. yb (inclusive), row-major: x runs fastest."""
    xs, ys = np.arange(xa, xb + 1), np.arange(ya, yb + 1)
    return np.stack(np.meshgrid(xs, ys, indexing="xy"), axis=-1).reshape(-1, 2)


def _nbhd(vox, r=1):
    o = _block(-r, r, -r, r)
    return _uniq((np.asarray(vox)[:, None, :] + o[None, :, :]).reshape(-1, 2))


def _ring_of(c, r):
    """The square ring of voxels at Chebyshev distance r around voxel c: walls around a sensor."""
    b = _block(c[0] - r, c[0] + r, c[1] - r, c[1] + r)
    return b[np.abs(b - np.asarray(c)).max(axis=1) == r]


def _cloud(rng, vox, leaf, per=6):
    """`per` float32 points in every voxel, a fifth of a voxel clear of its faces: occupied at min_pts 6, a full-rank covariance."""
    vox = np.asarray(vox, dtype=np.float64)
    u = rng.uniform(0.2, 0.8, (len(vox), per, 2))
    return ((vox[:, None, :] + u) * leaf).reshape(-1, 2).astype(F)


TRUTH = (0.25, 0.25)                    # the sensor's position in the map for the yaw-0 families: voxel (0, 0) at leaf 0.5
DELTA = (0.03, -0.02)                   # the initial guess is off by this much


def _scan(rng, vox, leaf, truth=TRUTH):
    """One float32 scan point per voxel, within a tenth of a voxel of its centre (where the voxel's own points have their
    mean, give or take: the true pose is then an optimum of the score), in the sensor's frame."""
    vox = np.asarray(vox, dtype=np.float64)
    w = (vox + rng.uniform(0.4, 0.6, vox.shape)) * leaf
    return (w - np.asarray(truth)[None, :]).astype(F)


def _init(truth=TRUTH, delta=DELTA):
    return (truth[0] + delta[0], truth[1] + delta[1], 0.0)


def _case(family, name, cloud, scan, init, prm=None, **expect):
    return Case(family, name, np.ascontiguousarray(cloud, dtype=F), np.ascontiguousarray(scan, dtype=F),
                tuple(float(v) for v in init), dict(prm or {}), expect)


# ------------------------------------------------------------------------------------------ the families
def fam_interior():
    """Control: a 20 x 14 block of scan voxels inside a map block two voxels wider, four far corner voxels that make the grid
    larger than the window.  Everything resident, every point fast, flags 0."""
    rng = _rng(1)
    sv = _block(0, 19, 0, 13)
    mv = _uniq(np.concatenate([_block(-2, 21, -2, 15), [(-25, -25), (45, -25), (-25, 40), (45, 40)]]))
    return [_case("interior", "interior", _cloud(rng, mv, 0.5), _scan(rng, sv, 0.5), _init(), spill=False, clipped=False,
                  fast=len(sv), ring=0, nonres=0)]


RING_COLS = (-66, -65, -64, -63, -62, 61, 62, 63, 64, 65)
RING_ROWS = (-65, -64, -63, -62, -31, 0, 29, 61, 62, 63, 64)


def fam_ring():
    """A box of 171 x 151 cells cut down to 128 x 128 around the sensor's voxel (0, 0): window columns and rows -64 .. 63.
    Scan points in the window columns 0, 1, 2, 125, 126, 127 (lx = 1 is the first fast column and reads slot column 0), two
    columns outside on either side, the same for the rows; the map holds the 3 x 3 neighbourhood of every scan voxel, so
    occupied voxels lie on both sides of the border."""
    rng = _rng(2)
    cross = np.array([(c, r) for c in RING_COLS for r in RING_ROWS])
    sv = _uniq(np.concatenate([cross, cross[:, ::-1], _ring_of((0, 0), 8), [(-80, 3), (80, -3), (3, -70), (-3, 70)]]))
    return [_case("ring", "ring", _cloud(rng, _nbhd(sv), 0.5), _scan(rng, sv, 0.5), _init(), spill=None, clipped=True,
                  fast=60, ring=100, labels=("w>128", "h>128"))]


CLIP_SHAPES = (
    # name, box (xa, xb, ya, yb) in voxels around the sensor's voxel (0, 0), the labels region_from_bbox must report
    ("both", (-80, 80, -75, 75), ("w>128", "h>128")),
    ("tall", (-25, 24, -140, 149), ("w<=128",)),
    ("flat", (-200, 199, -15, 14), ("w>128", "h2=h")),
    ("sensor_low", (20, 200, 20, 160), ("w>128", "h>128", "cx0<x0", "cy0<y0")),
    ("sensor_high", (-200, -20, -160, -20), ("w>128", "h>128", "cx0>x1", "cy0>y1")),
)


def fam_clip_shapes():
    """One case per branch of region_from_bbox's cut: 150 random scan voxels in the box, the box's four extreme voxels, and
    walls around the sensor where it lies inside the box.  The map holds the 3 x 3 neighbourhood of every scan voxel."""
    out = []
    for k, (name, (xa, xb, ya, yb), labels) in enumerate(CLIP_SHAPES):
        rng = _rng(3, k)
        sv = [np.stack([rng.integers(xa, xb + 1, 150), rng.integers(ya, yb + 1, 150)], axis=1),
              [(xa, (ya + yb) // 2), (xb, (ya + yb) // 2), ((xa + xb) // 2, ya), ((xa + xb) // 2, yb)]]
        if xa < 0 < xb and ya < 0 < yb:
            sv.append(_ring_of((0, 0), 6))
        sv = _uniq(np.concatenate(sv))
        out.append(_case("clip_shapes", "clip_shapes[%s]" % name, _cloud(rng, _nbhd(sv), 0.5), _scan(rng, sv, 0.5), _init(),
                         spill=None, clipped=True, fast=10, ring=10, labels=labels))
    return out


GRID_EDGE_SIDES = ("left", "right", "bottom", "top", "corner", "far")


def _grid_edge_voxels(side):
    """(map voxels, scan voxels, truth) of one side.  The map is the block 0 .. 19 squared (`far`: see fam_grid_edge)."""
    over, rows = np.array([-4, -3, -2, -1, 0, 1, 2]), np.arange(3, 16, 3)
    core = _block(5, 9, 5, 9)
    if side == "left":
        edge = [(x, y) for x in over for y in rows]
    elif side == "right":
        edge = [(19 - x, y) for x in over for y in rows]
    elif side == "bottom":
        edge = [(y, x) for x in over for y in rows]
    elif side == "top":
        edge = [(y, 19 - x) for x in over for y in rows]
    else:
        edge = [(x, y) for x in over for y in over]
    return _block(0, 19, 0, 19), _uniq(np.concatenate([core, edge])), (3.25, 3.25)


def fam_grid_edge():
    """The scan overhangs the map on each side and at a corner: window cells with negative grid coordinates or beyond div_x /
    div_y, points in voxel -1 and div (inside the padded grid: pairs with the map's edge voxels) and two and more voxels out
    (no pairs).  In these five the window holds the whole scan and the overhanging points are fast -- their slots are the
    window's "outside the search set" cells.  `far`: the sensor stands 150 voxels from the map's left edge inside walls of its
    own, two returns 75 and 85 voxels below and above stretch the box, and the 128 x 128 window around the sensor leaves the
    left edge outside: there the points in voxel -1 and div_y take the slow path at the edge of the padded grid.  Every case
    with grid_margin 0 and 8."""
    out = []
    for k, side in enumerate(GRID_EDGE_SIDES):
        rng = _rng(4, k)
        if side == "far":
            truth = (75.25, 7.75)                   # voxel (150, 15)
            mv = _uniq(np.concatenate([_block(0, 5, 0, 29), _nbhd(_ring_of((150, 15), 6))]))
            sv = _uniq(np.concatenate([[(x, y) for x in (-3, -2, -1, 0, 1) for y in range(4, 25, 4)], [(2, 30), (3, -1), (2, 32), (4, -3)],
                                       _ring_of((150, 15), 6), [(150, -60), (150, 100)]]))
        else:
            mv, sv, truth = _grid_edge_voxels(side)
        cloud, scan = _cloud(rng, mv, 0.5), _scan(rng, sv, 0.5, truth)
        for mg in (0, 8):
            out.append(_case("grid_edge", "grid_edge[%s,margin=%d]" % (side, mg), cloud, scan, _init(truth), dict(grid_margin=mg),
                             spill=None, clipped=(side == "far"), fast=10, ring=(12 if side == "far" else 0), off_grid=True))
    return out


ROW_WIDTHS = (11, 31, 32, 33, 63, 64, 65, 127, 128)


def fam_row_phase():
    """Window widths on both sides of the 32-bit words of the bitmaps: a box rw - 10 voxels wide and 6 high (a window of rw x
    16), scan points in the first two and last two columns of the box and one in the middle, over a map block that fills the
    window -- its occupancy runs are rw >= 32 bits long from a start bit >= 1 of the map's occupancy words, because two stray
    single points (no voxel: fewer than min_pts) make the grid three voxels wider than the block.  Occupied voxels the marks do
    not reach are left out: the window spills by `skipped`.
    [128c]: a box 150 wide cut to 128 columns; marks in window columns 0 and 1 in ten rows and in columns 126 and 127 in the
    ten rows above, blocks of occupied voxels at both row ends: the word-wise dilation reaches the far ends of the
    neighbouring rows and gives those voxels records (`leaked` > 0)."""
    out = []
    for rw in ROW_WIDTHS:
        rng = _rng(5, rw)
        bw = rw - 10
        cols = sorted({0, 1, bw // 2, bw - 2, bw - 1} & set(range(bw)))
        sv = _uniq([(x, y) for x in cols for y in range(6)] + [(0, 0), (bw - 1, 5)])
        mv = _block(-5, bw + 4, -5, 10)
        stray = (np.array([(-8, -7), (bw + 9, 13)]) + 0.5) * 0.5
        cloud = np.concatenate([_cloud(rng, mv, 0.5), stray.astype(F)])
        out.append(_case("row_phase", "row_phase[%d]" % rw, cloud, _scan(rng, sv, 0.5), _init(), spill=True, clipped=False,
                         fast=len(sv), ring=0, nonres=0, rw=rw, leaked=0))
    rng = _rng(5, 999)
    sv = _uniq([(x, y) for x in (-64, -63) for y in range(-10, 0)] + [(x, y) for x in (62, 63) for y in range(0, 10)] +
               [(-70, 0), (69, 0), (0, -60), (0, 59)] + [tuple(v) for v in _ring_of((0, 0), 6)])
    mv = _uniq(np.concatenate([_block(-66, -61, -15, 14), _block(60, 65, -15, 14), _nbhd(_ring_of((0, 0), 6)),
                               _nbhd([(-70, 0), (69, 0), (0, -60), (0, 59)])]))
    out.append(_case("row_phase", "row_phase[128c]", _cloud(rng, mv, 0.5), _scan(rng, sv, 0.5), _init(), spill=True, clipped=True,
                     fast=40, ring=20, rw=128, leaked=1))
    return out


POOL_BOX = 70
POOL_CAP = cap_of(POOL_BOX + 10, POOL_BOX + 10)
POOL_K = (POOL_CAP - 1, POOL_CAP, POOL_CAP + 1, POOL_CAP + 200)


def fam_pool_edge():
    """A window of 80 x 80 cells (box 70 x 70) whose map is occupied in exactly K voxels -- the first K - 1 of the box in
    row-major order and its last voxel -- each holding one scan point: skipped = 0, kept = K.  K = cap - 1 and cap: no spill.
    K = cap + 1 and cap + 200: the window spills and the K - cap highest voxels in row-major order have no record; the scan
    points in and beside them take the slow path from the first pass on."""
    out = []
    cells = _block(0, POOL_BOX - 1, 0, POOL_BOX - 1)          # row-major: x fastest
    for K in POOL_K:
        rng = _rng(6, K)
        sv = np.concatenate([cells[:K - 1], cells[-1:]])
        spill = K > POOL_CAP
        out.append(_case("pool_edge", "pool_edge[cap%+d]" % (K - POOL_CAP), _cloud(rng, sv, 0.5), _scan(rng, sv, 0.5), _init(),
                         dict(max_iter=2), spill=spill, clipped=False, fast=POOL_CAP - 300, ring=0,
                         nonres=(K - POOL_CAP if spill else 0), kept=K))
    return out


WALK_INITS = ((0.1, 0.1, 0.08), (-0.1, 0.05, -0.1), (0.0, 0.0, 0.12))


def fam_walk():
    """Four walls of 500 points 5 m from the sensor fix the pose; four fully occupied blocks of 14 x 14 voxels stand 22 m out,
    each with six isolated scan points.  The initial yaw is off by 0.08 to 0.12 rad, which puts the far points 3.5 to 5 cells
    from where they end up: while the pose converges they walk out of the two-cell dilation of their first cells into
    occupied voxels that got no record (skipped > 0, the -inf sentinel), and back to the slow path point by point."""
    rng = _rng(7)
    leaf = 0.5
    def four_walls(r, n, half, sigma):
        """n points on each of the walls x = 5, x = -5, y = 5, y = -5, |along| < half, sigma across."""
        t, d = r.uniform(-half, half, (4, n)), 5.0 + r.normal(0.0, sigma, (4, n))
        return np.concatenate([np.stack([d[0], t[0]], 1), np.stack([-d[1], t[1]], 1), np.stack([t[2], d[2]], 1), np.stack([t[3], -d[3]], 1)])

    walls = four_walls(rng, 500, 5.0, 0.03)
    centres = ((44, 0), (-44, 0), (0, 44), (0, -44))
    blocks = np.concatenate([_block(cx - 7, cx + 6, cy - 7, cy + 6) for cx, cy in centres])
    cloud = np.concatenate([walls.astype(F), _cloud(rng, blocks, leaf)])
    out = []
    for k, init in enumerate(WALK_INITS):
        r = _rng(7, 1 + k)
        parts = [four_walls(r, 60, 4.5, 0.02)]
        for cx, cy in centres:
            v = np.stack([r.integers(cx - 4, cx + 4, 6), r.integers(cy - 4, cy + 4, 6)], axis=1)
            parts.append((v + r.uniform(0.25, 0.75, v.shape)) * leaf)
        scan = np.concatenate(parts).astype(F)
        # keep the points that stand clear of the voxel faces at the first pose (the census is certain about those)
        xt, yt = transform(first_matrix(init), scan, True)
        ok = (face_margin(xt, leaf) >= 4 * FACE_MARGIN) & (face_margin(yt, leaf) >= 4 * FACE_MARGIN)
        out.append(_case("walk", "walk[%d]" % k, cloud, scan[ok], init, dict(max_iter=6), spill=True, clipped=False, fast=200,
                         ring=0, nonres=0))
    return out


def fam_degenerate_records():
    """The `leaves` cases of map_build_workloads with eig_mult 0 and no identity start, at leaf 1 m: the exactly collinear
    voxels keep a non-finite inverse covariance (leaf_finalize's third return) and stay in the search set.  The scan is
    the cloud's own points moved a fraction of a voxel (on_cloud_scan), so those voxels are marked, resident, and their
    records reach the pass through fill_window_fetch's finite_icov, not load_rec_global's."""
    out = []
    for c in MB.cases(1.0, MB.OFFSETS[0], "leaves"):
        if c.prm["eig_mult"] == 0.0 and not c.prm["cov_init_identity"]:
            scan, p = MB.on_cloud_scan(c)
            prm = dict(MB.params_of(c), resolution=1.0, max_iter=2)
            out.append(_case("degenerate_records", "degenerate_records[ub=%d]" % c.prm["cov_unbiased"], c.cloud, scan, p, prm,
                             spill=False, clipped=False, fast=len(scan), ring=0, nonres=0))
    return out


TIE_LEAVES = (0.5, 1.0)
TIE_SHIFT = (4.0, 4.0)


def tie_centroid(v, leaf):
    return (np.asarray(v, dtype=np.float64) + 0.5) * leaf


def fam_radius_tie():
    """A 6 x 6 block of voxels (16 .. 21 squared) whose six points are three pairs mirrored about the voxel's centre, all
    multiples of leaf / 16: the float32 sum of the six is exact and the float32 centroid IS the centre.  Scan points at the
    centres of the inner 4 x 4 voxels: to the four neighbours' centroids the float32 distance is ex * ex + ey * ey = leaf *
    leaf + 0 = r2 exactly -- in the radius with radius_inclusive 1, outside with 0.  Beside each a point one float32 step to
    the left and one to the right (one tie moves inside, the opposite one outside), and 40 ordinary points.  The initial
    guess is the exact translation (4, 4), yaw 0: x + 4 is exact for every point."""
    out = []
    off = np.array([(4, 2), (-4, -2), (2, -4), (-2, 4), (3, 3), (-3, -3)], dtype=np.float64) / 16.0
    for leaf in TIE_LEAVES:
        rng = _rng(9, int(leaf * 10))
        mv = _block(16, 21, 16, 21)
        cloud = np.concatenate([(tie_centroid(v, leaf)[None, :] + off * leaf) for v in mv]).astype(F)
        world = []
        for v in _block(17, 20, 17, 20):
            c = tie_centroid(v, leaf).astype(F)
            world += [c, (np.nextafter(c[0], F(-np.inf)), c[1]), (np.nextafter(c[0], F(np.inf)), c[1])]
        world = np.array(world, dtype=F).astype(np.float64)
        plain = (_block(16, 21, 16, 21)[rng.integers(0, 36, 40)] + rng.uniform(0.25, 0.75, (40, 2))) * leaf
        scan = np.concatenate([world - np.asarray(TIE_SHIFT), plain - np.asarray(TIE_SHIFT)]).astype(F)
        assert np.array_equal((scan[:len(world)] + F(4.0)).astype(np.float64), world), "x + 4 must give the tie points back exactly"
        for incl in (0, 1):
            out.append(_case("radius_tie", "radius_tie[leaf=%g,incl=%d]" % (leaf, incl), cloud, scan, TIE_SHIFT + (0.0,),
                             dict(resolution=leaf, radius_inclusive=incl, max_iter=2), spill=False, clipped=False, fast=len(scan),
                             ring=0, nonres=0, ties=4 * 16))
    return out


SCAN_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 3073, 4097, 5121, 10240, 10241)
SCAN_HOLES = (2049, 5121)


def fam_scan_sizes():
    """Scans of n points over one fully occupied 30 x 30 block: per_lane = ceil(n / 1024) runs through 1 .. 5 and 10 (the empty
    runs of short scans, the last round with lanes past the end), and the set-up takes order_scan_regs up to 10240 points and
    compute_region + sort_points for 10241.  [n,holes]: NaN and Inf points at the first and last positions of lane runs of
    the input (they sort behind every cell: the last lanes' runs of the ordered copy)."""
    rng = _rng(10)
    cloud = _cloud(rng, _block(0, 29, 0, 29), 0.5)
    out = []
    for n in SCAN_SIZES:
        r = _rng(10, n)
        sv = np.stack([r.integers(5, 25, n), r.integers(5, 25, n)], axis=1)
        scan = _scan(r, sv, 0.5, (7.25, 7.25))
        out.append(_case("scan_sizes", "scan_sizes[%d]" % n, cloud, scan, _init((7.25, 7.25)), dict(max_iter=2), spill=None,
                         clipped=False, fast=n, ring=0, nonres=0))
        if n in SCAN_HOLES:
            holes = scan.copy()
            bad = [(np.nan, 0.5), (np.inf, 0.5), (0.5, -np.inf), (np.nan, np.nan), (-np.inf, np.inf), (0.25, np.nan)]
            at = [0, 1, K_BLOCK - 1, K_BLOCK, n - 2, n - 1]
            for i, b in zip(at, bad):
                holes[i] = b
            out.append(_case("scan_sizes", "scan_sizes[%d,holes]" % n, cloud, holes, _init((7.25, 7.25)), dict(max_iter=2), spill=None,
                             clipped=False, fast=n - len(at), ring=len(at), nonres=0))
    return out


FAMILIES = dict(interior=fam_interior, ring=fam_ring, clip_shapes=fam_clip_shapes, grid_edge=fam_grid_edge, row_phase=fam_row_phase,
                pool_edge=fam_pool_edge, walk=fam_walk, degenerate_records=fam_degenerate_records, radius_tie=fam_radius_tie,
                scan_sizes=fam_scan_sizes)
_CASES = {}


def cases(family=None):
    """Every case, built once."""
    if not _CASES:
        for name, f in FAMILIES.items():
            _CASES[name] = f()
    return [c for name, cs in _CASES.items() for c in cs if family is None or name == family]


def case(name):
    return next(c for c in cases() if c.name == name)


_CENSUS = {}


def census_of(c, oracle):
    """(grid, census) of a case from the ORACLE's map (built once per case and kept)."""
    if c.name not in _CENSUS:
        om = oracle.Map(c.cloud, params_of(c, oracle))
        i = om.info()
        grid = Grid(int(i.min_bx), int(i.min_by), int(i.div_x), int(i.div_y))
        _CENSUS[c.name] = (om, grid, window_census(grid, om.export()["idx"], c.scan, c.init, dict(DEFAULTS, **c.prm)))
    return _CENSUS[c.name]
