"""The match-window families of tests/match_window_workloads.py on the CPU: the census itself on hand-worked windows (so that
it is not trusted blindly), then every family against the census and the oracle alone -- the flags it must raise, the
paths its points must take at the first pose (a floor above zero for the path it is named after), the face margins that
make the census certain, kept against cap, and for `walk` the oracle's own trace: while the pose converges, points must
come to stand beside occupied voxels that got no LDS record.  What tests/test_gpu_match_window_geometry.py then holds the
device to is shown here to reach the paths it is for, and -- last section -- to have teeth: each way the window code could
go wrong that a family is aimed at changes the pair count of a pass, an integer the GPU module holds equal."""
import numpy as np
import pytest

import match_window_workloads as W

NAMES = [c.name for c in W.cases()]


def grid_of_cells(rw, rh, pairs):
    """bool [rh, rw] with the (lx, ly) of `pairs` set."""
    m = np.zeros((rh, rw), bool)
    for lx, ly in pairs:
        m[ly, lx] = True
    return m


def dilate_by_shifts(marked, rw, rh):
    """The dilation as one shift of the whole cell string (a Python integer of 16384 bits): c + dy rw + dx for dx, dy in
    -2 .. 2, bits below 0 and from 16384 on dropped.  What the word-wise form must equal."""
    s = 0
    for c in np.flatnonzero(np.asarray(marked).ravel()):
        s |= 1 << int(c)
    full = (1 << W.K_REGION_CELLS) - 1
    h = s | (s << 1) | (s << 2) | (s >> 1) | (s >> 2)
    h &= full
    out = h
    for m in (1, 2):
        out |= (h << (m * rw)) | (h >> (m * rw))
    out &= full
    return np.array([(out >> c) & 1 for c in range(rw * rh)], dtype=bool).reshape(rh, rw)


# ------------------------------------------------------------------------------------------ the census on hand-worked windows
def test_window_of_a_box_by_hand():
    """One voxel: 11 x 11.  23 x 2 voxels: 33 x 12.  200 x 200 around a sensor at (100, 100): 210 x 210 cut to 128 x 128 from
    (36, 36).  The same box with the sensor at its low corner and beyond its high corner: the window is pushed back inside the
    box plus its margin.  A box 50 wide and 400 high: 60 columns, 16384 // 60 = 273 rows.  A box 600 wide and 20 high: 128
    columns, and the 128 rows the table would allow are cut to the box's 30."""
    assert W.region_from_bbox((7, 9, 7, 9), (0, 0)) == ((2, 4, 11, 11), 0, ())
    assert W.region_from_bbox((0, 0, 22, 1), (3, 3)) == ((-5, -5, 33, 12), 0, ())
    assert W.region_from_bbox((0, 0, 199, 199), (100, 100)) == ((36, 36, 128, 128), 1, ("w>128", "h>128"))
    assert W.region_from_bbox((0, 0, 199, 199), (0, 0)) == ((-5, -5, 128, 128), 1, ("w>128", "h>128", "cx0<x0", "cy0<y0"))
    assert W.region_from_bbox((0, 0, 199, 199), (500, 500)) == ((77, 77, 128, 128), 1, ("w>128", "h>128", "cx0>x1", "cy0>y1"))
    assert W.region_from_bbox((0, 0, 49, 399), (25, 200)) == ((-5, 200 - 136, 60, 273), 1, ("w<=128",))
    assert W.region_from_bbox((0, 0, 599, 19), (300, 10)) == ((300 - 64, -5, 128, 30), 1, ("w>128", "h2=h"))
    assert W.region_from_bbox(None, (0, 0)) == ((0, 0, 0, 0), 0, ())
    # 127 x 129 = 16383 cells fit, 128 x 129 do not
    assert W.region_from_bbox((0, 0, 116, 118), (0, 0))[1] == 0 and W.region_from_bbox((0, 0, 117, 118), (0, 0))[1] == 1


def test_capacity_by_hand():
    """11 x 11: 242 bytes of slots round up to 256; (150528 - 256) // 48 = 3130 records, two of them sentinels.  128 x 128:
    32768 bytes of slots, 2453 records, 2451 usable."""
    assert W.cap_of(11, 11) == 3128
    assert W.cap_of(128, 128) == 2451
    assert W.cap_of(80, 80) == (147 * 1024 - 12800) // 48 - 2 == W.POOL_CAP == 2867


def test_dilation_of_an_11_by_11_window_by_hand():
    """A mark in the middle reaches its 5 x 5 block.  A mark in column 0 of row 5 reaches columns 0 .. 2 of rows 3 .. 7 and --
    the cell string goes on into the row before -- columns 9 and 10 of rows 2 .. 6."""
    mid = W.unpack_words(W.dilate_words(W.pack_words(grid_of_cells(11, 11, [(5, 5)])), 11), 121).reshape(11, 11)
    assert np.array_equal(mid, grid_of_cells(11, 11, [(x, y) for x in range(3, 8) for y in range(3, 8)]))
    assert np.array_equal(mid, W.dilate_2d(grid_of_cells(11, 11, [(5, 5)]), 11, 11))
    edge = W.unpack_words(W.dilate_words(W.pack_words(grid_of_cells(11, 11, [(0, 5)])), 11), 121).reshape(11, 11)
    want = [(x, y) for x in (0, 1, 2) for y in range(3, 8)] + [(x, y) for x in (9, 10) for y in range(2, 7)]
    assert np.array_equal(edge, grid_of_cells(11, 11, want))
    assert int((edge & ~W.dilate_2d(grid_of_cells(11, 11, [(0, 5)]), 11, 11)).sum()) == 10


def test_dilation_of_a_33_by_12_window_by_hand():
    """Cell (32, 0) is bit 0 of the second word.  It reaches columns 30 .. 32 of rows 0 .. 2 and, over the row end, columns 0
    and 1 of rows 0 .. 3 (one row up from the leak's own row 1, two rows down).  The window's last cell (32, 11) reaches
    columns 30 .. 32 of rows 9 .. 11, columns 0 and 1 of rows 10 and 11, and bits past the window's 396 cells that no occupied
    voxel can meet."""
    a = W.unpack_words(W.dilate_words(W.pack_words(grid_of_cells(33, 12, [(32, 0)])), 33), 396).reshape(12, 33)
    want = [(x, y) for x in (30, 31, 32) for y in (0, 1, 2)] + [(x, y) for x in (0, 1) for y in (0, 1, 2, 3)]
    assert np.array_equal(a, grid_of_cells(33, 12, want))
    b = W.unpack_words(W.dilate_words(W.pack_words(grid_of_cells(33, 12, [(32, 11)])), 33), 396).reshape(12, 33)
    want = [(x, y) for x in (30, 31, 32) for y in (9, 10, 11)] + [(x, y) for x in (0, 1) for y in (10, 11)]
    assert np.array_equal(b, grid_of_cells(33, 12, want))


@pytest.mark.parametrize("rw,rh", [(11, 11), (31, 20), (32, 16), (33, 12), (63, 40), (64, 64), (65, 30), (127, 129), (128, 128)])
def test_word_wise_dilation_is_one_shift_of_the_cell_string(rw, rh):
    """Random marks, with marks forced into the window's four corner cells and both ends of a middle row: the word-wise form
    equals the dilation written as shifts of one 16384-bit integer, for row widths on both sides of the word size."""
    rng = np.random.Generator(np.random.Philox(rw * 1000 + rh))
    m = rng.random((rh, rw)) < 0.02
    for lx, ly in ((0, 0), (rw - 1, 0), (0, rh - 1), (rw - 1, rh - 1), (0, rh // 2), (rw - 1, rh // 2)):
        m[ly, lx] = True
    got = W.unpack_words(W.dilate_words(W.pack_words(m), rw), rw * rh).reshape(rh, rw)
    assert np.array_equal(got, dilate_by_shifts(m, rw, rh))
    assert not (W.dilate_2d(m, rw, rh) & ~got).any()              # the drawn dilation is a subset: the leak only adds


def test_plan_by_hand():
    """11 x 11, one mark in the middle, occupied: the mark's own voxel, one two cells away (kept), one three cells away and
    one in a corner (skipped): kept 2, skipped 2, nspill 2, the kept ones resident and numbered in row-major order."""
    marked = grid_of_cells(11, 11, [(5, 5)])
    occ = grid_of_cells(11, 11, [(5, 5), (7, 3), (8, 5), (0, 0)])
    keep, kept, skipped, nspill, resident = W.plan(marked, occ, 11, 11)
    assert (kept, skipped, nspill) == (2, 2, 2)
    assert np.array_equal(keep.reshape(11, 11), grid_of_cells(11, 11, [(5, 5), (7, 3)]))
    assert np.array_equal(resident, keep)


def test_census_of_a_small_scene_by_hand():
    """A 20 x 20 grid from (-3, -2), leaf 0.5, pose (0, 0, 0).  Four points: voxel (4, 4) [grid (7, 6)], its neighbour (5, 4),
    voxel (10, 4) six columns on, and a NaN.  Box (7, 6) .. (13, 6): window (2, 1) 17 x 11.  Occupied: grid (7, 6), (8, 7)
    (beside the first two points), (13, 9) (three rows above the third: skipped), (2, 3) (the window's first column: skipped).
    Every finite point is inside the ring and beside nothing without a record: fast.  The NaN counts as outside."""
    grid = W.Grid(-3, -2, 20, 20)
    occupied = [6 * 20 + 7, 7 * 20 + 8, 9 * 20 + 13, 3 * 20 + 2]
    scan = np.array([(2.2, 2.3), (2.7, 2.2), (5.3, 2.1), (np.nan, 0.0)], dtype=np.float32)
    cs = W.window_census(grid, occupied, scan, (0.0, 0.0, 0.0), dict(resolution=0.5, transform_sse=1))
    assert cs.region == (2, 1, 17, 11) and cs.cap == W.cap_of(17, 11) and not cs.clipped
    assert (cs.kept, cs.skipped, cs.nspill, cs.flags) == (2, 2, 2, W.FLAG_WINDOW_SPILL)
    assert cs.path.tolist() == [W.FAST, W.FAST, W.FAST, W.RING]
    assert cs.vox[:3].tolist() == [[7, 6], [8, 6], [13, 6]] and cs.finite.tolist() == [True, True, True, False]
    # the third point three rows up stands beside the skipped voxel: certain to leave the fast path there
    up = W.slow_points_at(grid, cs, (0.0, 1.5, 0.0), scan, dict(resolution=0.5))
    assert up.tolist() == [False, False, True, False]
    # ... and a point in the window's first column is in the ring
    cs2 = W.window_census(grid, occupied, np.concatenate([scan, [(-0.3, 1.2)]]).astype(np.float32), (0.0, 0.0, 0.0), dict(resolution=0.5))
    assert cs2.region == (-3, -1, 22, 13) and cs2.path.tolist()[:3] == [W.FAST] * 3 and cs2.path[4] == W.FAST


def test_the_two_transform_forms_round_differently():
    """(a + b) + tx against a + (b + tx): the census follows the case's transform_sse, and the two are not the same function."""
    T = W.first_matrix((0.1, -0.2, 0.3))
    p = np.random.Generator(np.random.Philox(5)).uniform(-30, 30, (4000, 2)).astype(np.float32)
    xs, ys = W.transform(T, p, True)
    xn, yn = W.transform(T, p, False)
    assert xs.dtype == np.float32 and ((xs != xn) | (ys != yn)).any() and np.abs(xs - xn).max() < 1e-5


# ------------------------------------------------------------------------------------------ the families
def test_every_family_is_there():
    fams = {c.family for c in W.cases()}
    assert fams == set(W.FAMILIES) == {"interior", "ring", "clip_shapes", "grid_edge", "row_phase", "pool_edge", "walk",
                                       "degenerate_records", "radius_tie", "scan_sizes"}
    assert len(set(NAMES)) == len(NAMES)
    for c in W.cases():
        assert len(c.cloud) <= 30000 and len(c.scan) <= 10241, c.name
        assert c.init[2] == 0.0 or c.family == "walk", c.name


@pytest.mark.parametrize("name", NAMES)
def test_a_case_reaches_what_it_is_for(oracle, name):
    """The flags, the path counts (a floor where the expectation is positive, none at all where it is zero), the branch of
    the cut, the face margin of every finite point at the first pose, and what a family promises beyond that."""
    c = W.case(name)
    om, grid, cs = W.census_of(c, oracle)
    e = c.expect
    prm = dict(W.DEFAULTS, **c.prm)
    leaf = prm["resolution"]
    assert bool(cs.clipped) == e["clipped"], (cs.region, cs.clip)
    if e["spill"] is not None:
        assert (cs.nspill > 0) == e["spill"], (cs.kept, cs.skipped, cs.cap)
    assert cs.flags == (W.FLAG_WINDOW_SPILL if cs.nspill > 0 else 0) | (W.FLAG_REGION_CLIPPED if cs.clipped else 0)
    got = W.path_counts(cs)
    for k in ("fast", "ring", "nonres"):
        if k in e:
            assert (got[k] >= e[k]) if e[k] > 0 else (got[k] == 0), (k, got, e[k])
    if "labels" in e:
        assert set(cs.clip) == set(e["labels"]), cs.clip
    _, _, fin, xt, yt = W.voxels_at(grid, c.init, c.scan, prm)
    assert W.face_margin(xt[fin], leaf).min() >= W.FACE_MARGIN and W.face_margin(yt[fin], leaf).min() >= W.FACE_MARGIN
    assert cs.region[2] * cs.region[3] <= W.K_REGION_CELLS and cs.kept + cs.skipped == int(cs.occ.sum())
    if "leaked" in e:
        assert (cs.leaked >= e["leaked"]) if e["leaked"] else (cs.leaked == 0), cs.leaked
    if "rw" in e:
        assert cs.region[2] == e["rw"] and (cs.region[3] == 16 or cs.clipped), cs.region
    if "kept" in e:
        assert cs.kept == e["kept"] and cs.skipped == 0 and cs.cap == W.POOL_CAP and cs.nspill == max(e["kept"] - cs.cap, 0)
    if e.get("off_grid"):
        assert cs.cells_off_grid > 0


def test_ring_points_sit_in_the_columns_and_rows_they_are_for(oracle):
    """Points in window columns and rows 0, 1, 2, rw - 3, rw - 2, rw - 1, and one and two cells outside on every side; the
    first and the last fast column and row (1 and rw - 2) hold fast points, 0 and rw - 1 only ring points; occupied voxels on
    both sides of every border."""
    c = W.case("ring")
    _, grid, cs = W.census_of(c, oracle)
    x0, y0, rw, rh = cs.region
    assert (rw, rh) == (128, 128)
    l = cs.vox - np.array([x0, y0])
    for a in (0, 1):
        for v in (-2, -1, 0, 1, 2, rw - 3, rw - 2, rw - 1, rw, rw + 1):
            assert (l[:, a] == v).sum() >= 5, (a, v)
        for v in (1, rw - 2):
            assert ((l[:, a] == v) & (cs.path == W.FAST)).sum() >= 3, (a, v)
        for v in (0, rw - 1):
            assert ((l[:, a] == v) & (cs.path != W.RING)).sum() == 0, (a, v)
    occ = W.occupancy_grid(grid, _occupied(oracle, c))
    assert occ[:, x0 - 1].any() and occ[:, x0].any() and occ[:, x0 + rw - 1].any() and occ[:, x0 + rw].any()
    assert occ[y0 - 1].any() and occ[y0].any() and occ[y0 + rh - 1].any() and occ[y0 + rh].any()


def _occupied(oracle, c):
    return W.census_of(c, oracle)[0].export()["idx"]


def test_clip_shapes_cover_every_branch(oracle):
    seen = set()
    for c in W.cases("clip_shapes"):
        seen |= set(W.census_of(c, oracle)[2].clip)
    assert seen >= {"w>128", "w<=128", "h>128", "h2=h", "cx0<x0", "cy0<y0", "cx0>x1", "cy0>y1"}


@pytest.mark.parametrize("side", W.GRID_EDGE_SIDES)
def test_grid_edge_points_stand_on_and_beyond_the_padded_grid(oracle, side):
    """Points in voxel -1 or div (inside the padded grid), points two and more voxels out (no pairs), window cells off the
    grid; the census does not depend on grid_margin; in `far` the points on the padded edge are outside the window."""
    c0, c8 = (W.case("grid_edge[%s,margin=%d]" % (side, m)) for m in (0, 8))
    (_, grid, cs), (_, grid8, cs8) = W.census_of(c0, oracle), W.census_of(c8, oracle)
    assert grid == grid8 and cs.region == cs8.region and cs.flags == cs8.flags and np.array_equal(cs.path, cs8.path)
    assert c0.prm["grid_margin"] == 0 and c8.prm["grid_margin"] == 8 and c0.scan.tobytes() == c8.scan.tobytes()
    ix, iy = cs.vox[:, 0], cs.vox[:, 1]
    on_edge = (((ix == -1) | (ix == grid.div_x)) & (iy >= -1) & (iy <= grid.div_y)) | \
              (((iy == -1) | (iy == grid.div_y)) & (ix >= -1) & (ix <= grid.div_x))
    beyond = (ix < -1) | (ix > grid.div_x) | (iy < -1) | (iy > grid.div_y)
    assert on_edge.sum() >= 5 and beyond.sum() >= 2, (int(on_edge.sum()), int(beyond.sum()))
    x0, y0, rw, rh = cs.region
    assert x0 < 0 or y0 < 0 or x0 + rw > grid.div_x or y0 + rh > grid.div_y
    if side == "far":
        assert (cs.path[on_edge] == W.RING).all() and (iy[on_edge] == grid.div_y).any() and (ix[on_edge] == -1).any()
    else:
        assert (cs.path[on_edge] == W.FAST).all()


@pytest.mark.parametrize("rw", W.ROW_WIDTHS)
def test_row_phase_occupancy_runs_cross_the_maps_words(oracle, rw):
    """Every window row is one run of rw occupied voxels of the map; the runs start at bit >= 1 of a word of the map's bitmap
    in most rows and are 32 bits and longer from rw = 32 on; marks sit in the first two and last two columns of the box."""
    c = W.case("row_phase[%d]" % rw)
    _, grid, cs = W.census_of(c, oracle)
    x0, y0, _, rh = cs.region
    assert cs.occ.all()
    starts = [((y0 + ly) * grid.div_x + x0) & 31 for ly in range(rh)]
    assert sum(s >= 1 for s in starts) >= rh - 2 and len(set(starts)) >= 4, starts
    cols = set(np.flatnonzero(cs.marked.any(axis=0)).tolist())
    assert cols >= ({5, rw - 6} if rw == 11 else {5, 6, rw - 7, rw - 6}) and min(cols) == 5 and max(cols) == rw - 6


def test_row_phase_128c_marks_the_windows_own_first_and_last_columns(oracle):
    c = W.case("row_phase[128c]")
    _, grid, cs = W.census_of(c, oracle)
    cols = set(np.flatnonzero(cs.marked.any(axis=0)).tolist())
    assert {0, 1, 126, 127} <= cols and cs.leaked >= 20
    leak = cs.keep & ~W.dilate_2d(cs.marked, 128, 128)
    assert set(np.flatnonzero(leak.any(axis=0)).tolist()) <= {0, 1, 126, 127}


def test_pool_edge_leaves_out_the_highest_voxels(oracle):
    """K = cap + 1 and cap + 200: the occupied voxels without a record are the K - cap last ones in row-major order, and the
    census names the scan points in and beside them; K <= cap: none."""
    for c in W.cases("pool_edge"):
        _, grid, cs = W.census_of(c, oracle)
        K = c.expect["kept"]
        out = cs.occ & ~cs.resident
        assert int(out.sum()) == max(K - cs.cap, 0)
        if K > cs.cap:
            order = np.flatnonzero(cs.occ.ravel())
            assert np.array_equal(np.flatnonzero(out.ravel()), order[cs.cap:])
            l = cs.vox - np.array(cs.region[:2])
            inside = out[l[:, 1], l[:, 0]]
            assert int(inside.sum()) == K - cs.cap and (cs.path[inside] == W.NONRES).all()
            assert (cs.path == W.NONRES).sum() > inside.sum() or K - cs.cap == 1


def distinct_rows(tr):
    return [k for k in range(len(tr)) if k == 0 or not np.array_equal(tr[k], tr[k - 1])]


@pytest.mark.parametrize("name", [c.name for c in W.cases("walk")])
def test_walk_leaves_the_resident_set_in_the_oracles_trace(oracle, name):
    """The oracle's own match: it converges within a dozen passes, and over the poses of its trace at least 8 points (counted
    only where they stand FACE_MARGIN clear of every voxel face) have a 3 x 3 neighbourhood that holds an occupied voxel the
    first pose left without a record -- none at the first pose itself, where the dilation covers every neighbourhood."""
    c = W.case(name)
    om, grid, cs = W.census_of(c, oracle)
    prm = dict(W.DEFAULTS, **c.prm)
    ref, tr = om.align(c.scan, c.init, trace_cap=64)
    assert ref["converged"] and 4 <= len(tr) <= 16 and 0.08 <= abs(c.init[2]) <= 0.12
    counts = [int(W.slow_points_at(grid, cs, tr[k][5:8], c.scan, prm).sum()) for k in distinct_rows(tr)]
    assert counts[0] == 0 and sum(counts) >= 8 and sum(n > 0 for n in counts) >= 2, counts
    assert cs.skipped > 0 and cs.kept < cs.cap                     # the spill is by `skipped`, not by the pool


@pytest.mark.parametrize("name", [c.name for c in W.cases("degenerate_records")])
def test_degenerate_records_are_resident_and_beside_fast_points(oracle, name):
    c = W.case(name)
    om, grid, cs = W.census_of(c, oracle)
    ex = om.export()
    bad = ~np.isfinite(ex["icov"]).all(axis=1)
    assert bad.sum() >= 2
    x0, y0, rw, rh = cs.region
    for g in ex["idx"][bad]:
        gx, gy = int(g) % grid.div_x, int(g) // grid.div_x
        assert cs.resident[gy - y0, gx - x0]
        near = (np.abs(cs.vox[:, 0] - gx) <= 1) & (np.abs(cs.vox[:, 1] - gy) <= 1)
        assert (cs.path[near] == W.FAST).sum() >= 3


@pytest.mark.parametrize("leaf", W.TIE_LEAVES)
def test_radius_ties_are_exact_and_counted_by_the_inclusive_test_only(oracle, leaf):
    """The centroids the oracle exports ARE the voxel centres; at the first pose the float32 distance of 4 x 16 (point,
    centroid) pairs equals r2 exactly, the one-step neighbours fall one float32 step inside and outside; the oracle's pair
    count at that pose differs between radius_inclusive 1 and 0 by exactly the number of ties."""
    c0, c1 = (W.case("radius_tie[leaf=%g,incl=%d]" % (leaf, i)) for i in (0, 1))
    (om0, grid, cs), (om1, _, _) = W.census_of(c0, oracle), W.census_of(c1, oracle)
    ex = om0.export()
    want = np.array([W.tie_centroid((16 + g % 6, 16 + g // 6), leaf) for g in ex["idx"]], dtype=np.float32)
    assert np.array_equal(ex["cent"], want)
    xt, yt = W.transform(W.first_matrix(c0.init), c0.scan, True)
    ex_, ey_ = xt[:, None] - ex["cent"][None, :, 0], yt[:, None] - ex["cent"][None, :, 1]
    dd = ex_ * ex_ + ey_ * ey_
    r2 = np.float32(float(leaf) * float(leaf))
    assert dd.dtype == np.float32
    ties = int((dd == r2).sum())
    assert ties >= c0.expect["ties"]
    near = np.abs(dd.astype(np.float64) / float(r2) - 1.0) < 1e-5          # (one step of a coordinate near 10 is 4e-6 of leaf^2)
    assert int((near & (dd < r2)).sum()) >= 16 and int((near & (dd > r2)).sum()) >= 16
    p0, p1 = om0.eval_at(c0.scan, c0.init)[3], om1.eval_at(c1.scan, c1.init)[3]
    assert p1 - p0 == ties and p0 == int((dd < r2).sum())


def test_scan_sizes_cover_the_run_partition_and_both_setups():
    ns = sorted({len(c.scan) for c in W.cases("scan_sizes")})
    assert ns == sorted(W.SCAN_SIZES)
    per_lane = {-(-n // W.K_BLOCK) for n in ns}
    assert per_lane >= {1, 2, 3, 4, 5, 10, 11}
    assert {p % W.K_SUB for p in per_lane} == {0, 1, 2, 3} and any(p < W.K_SUB for p in per_lane)     # every remainder; empty runs
    assert W.K_SORT_REGS in ns and W.K_SORT_REGS + 1 in ns and any(n % W.K_BLOCK == 0 for n in ns) and any(n % W.K_BLOCK == 1 for n in ns)
    for n in W.SCAN_HOLES:
        s = W.case("scan_sizes[%d,holes]" % n).scan
        bad = ~np.isfinite(s).all(axis=1)
        assert bad[[0, 1, W.K_BLOCK - 1, W.K_BLOCK, n - 2, n - 1]].all() and bad.sum() == 6


@pytest.mark.parametrize("name", NAMES)
def test_a_trace_row_is_a_function_of_its_pose_in_the_oracle(oracle, name):
    """What the GPU module relies on, shown on the oracle: eval_at at the three pose columns of a trace row gives that row's
    score and gradient back to the last bit (row 0 too when the initial yaw is 0: the guess matrix is (1, 0, tx, ty) and
    p0 is read back from it)."""
    c = W.case(name)
    om = W.census_of(c, oracle)[0]
    ref, tr = om.align(c.scan, c.init, trace_cap=64)
    assert 2 <= len(tr) < 64
    for k in distinct_rows(tr):
        if k == 0 and c.init[2] != 0.0:
            continue
        s, g, _, _ = om.eval_at(c.scan, tr[k][5:8])
        assert s == tr[k][1] and np.array_equal(g, tr[k][2:5], equal_nan=True), (name, k)


# ------------------------------------------------------------------------------------------ teeth
# The GPU module holds integers: the pairs of every executed pass (through kbar) and, with them, the score's terms.  For each
# way the window code could go wrong that the families are aimed at, the pair count of a pass changes -- shown here from
# the census and the oracle's exported centroids, in numpy.
@pytest.mark.parametrize("name", [c.name for c in W.cases() if c.init[2] == 0.0])
def test_the_census_counts_the_oracles_pairs_at_the_first_pose(oracle, name):
    """The numpy pair count (the census's voxel of every point, the exported float32 centroids, the float32 radius test)
    equals the oracle's at the first pose: the census and the oracle agree on which voxel every point is in."""
    c = W.case(name)
    om, grid, cs = W.census_of(c, oracle)
    per_point = W.pairs_at(grid, om.export(), c.init, c.scan, dict(W.DEFAULTS, **c.prm))
    assert int(per_point.sum()) == int(om.eval_at(c.scan, c.init)[3]) > 0


def nonresident(grid, cs):
    return np.flatnonzero(cs.nonres_grid.ravel())


def test_a_pass_that_ignored_the_missing_records_would_lose_pairs(oracle):
    """eval_point's `lowx != -inf`: pool_edge beyond cap at the first pose, walk at the poses of the oracle's trace -- the
    points the census sends to the slow path have pairs with voxels that have no LDS record."""
    for c in W.cases("pool_edge"):
        om, grid, cs = W.census_of(c, oracle)
        lost = W.pairs_at(grid, om.export(), c.init, c.scan, dict(W.DEFAULTS, **c.prm), nonresident(grid, cs))
        assert (lost[cs.path == W.FAST] == 0).all() and int(lost.sum()) >= max(c.expect["kept"] - cs.cap, 0)
        assert (lost.sum() > 0) == (c.expect["kept"] > cs.cap)
    for c in W.cases("walk"):
        om, grid, cs = W.census_of(c, oracle)
        prm = dict(W.DEFAULTS, **c.prm)
        tr = om.align(c.scan, c.init, trace_cap=64)[1]
        lost = [int(W.pairs_at(grid, om.export(), tr[k][5:8], c.scan, prm, nonresident(grid, cs))[W.slow_points_at(grid, cs, tr[k][5:8], c.scan, prm)].sum())
                for k in distinct_rows(tr)]
        assert lost[0] == 0 and sum(lost) >= 8, lost


def test_the_voxel_numbered_cap_has_pairs(oracle):
    """fill_window_fetch's `next < cap`: at K = cap + 1 the one voxel without a record (number `cap` in row-major order) is
    in the radius of the points in and beside it; were it given slot `cap` -- the "outside the search set" sentinel -- those
    pairs would vanish without a trace in the flags."""
    c = W.case("pool_edge[cap+1]")
    om, grid, cs = W.census_of(c, oracle)
    out = nonresident(grid, cs)
    assert len(out) == 1
    assert int(W.pairs_at(grid, om.export(), c.init, c.scan, dict(W.DEFAULTS, **c.prm), out).sum()) >= 1


@pytest.mark.parametrize("name", [c.name for c in W.cases("degenerate_records")])
def test_the_degenerate_records_are_in_the_radius_of_fast_points(oracle, name):
    """fill_window_fetch's finite_icov: fast points pair with the voxels whose inverse covariance is not finite."""
    c = W.case(name)
    om, grid, cs = W.census_of(c, oracle)
    ex = om.export()
    bad = ex["idx"][~np.isfinite(ex["icov"]).all(axis=1)]
    hit = W.pairs_at(grid, ex, c.init, c.scan, dict(W.DEFAULTS, **c.prm), bad)
    assert int(hit[cs.path == W.FAST].sum()) >= 10


@pytest.mark.parametrize("n", [n for n in W.SCAN_SIZES if n % W.K_BLOCK])
def test_a_lane_past_the_end_would_add_pairs(oracle, n):
    """pass_units' `base + k * kBlock >= n`: the lane at position n of the last round reads the copy's last point again
    (min(i, n - 1)).  The ordered copy ends with the points of the highest marked cell; every one of them has pairs, so a
    lane that evaluated it twice would raise the pass's pair count."""
    c = W.case("scan_sizes[%d]" % n)
    om, grid, cs = W.census_of(c, oracle)
    per_point = W.pairs_at(grid, om.export(), c.init, c.scan, dict(W.DEFAULTS, **c.prm))
    l = cs.vox - np.array(cs.region[:2])
    key = l[:, 1] * cs.region[2] + l[:, 0]
    assert (per_point[key == key.max()] > 0).all()


def test_the_families_raise_every_combination_of_the_two_flags(oracle):
    assert {W.census_of(c, oracle)[2].flags for c in W.cases()} == {0, 1, 2, 3}
