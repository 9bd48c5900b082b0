"""The nearest-raw-point search behind getFitnessScore (row a7, ndt_fitness.hip.h) against brute force, on map geometries the
synthetic wall worlds never produce (tests/fitness_workloads.py): one voxel, one row, one column, grids narrower than an
occupancy tile, a voxel with 5001 points, buckets of 1 .. 30 points, points and queries on the voxel lattice, islands far
apart -- at leaves 0.05 .. 2 m and world offsets up to 8 km.  The search has three device paths that must give the same
float32 distance for every query:

  1. ndt_fitness_at: one lane per query (nearest_ring1_lane + nearest_far),
  2. a batch with scans of its own: the wave's joint ring-1 work, nearest_far inline,
  3. `shared_scan` launches: the far queries listed per match and finished from the occupancy tiles,

each with a MULTI instance (ndt_align_batch_multi) and a transform_sse on / off instance.  The reference is the minimum over
ALL map points (fitness_workloads.brute_sq) of the queries the record's own float32 matrix gives; scans are cut so that
their fp64 sum is exact in any order (stratify) and compared for EQUALITY: one query wrong by a float32 ulp fails.  A scan
that cannot be cut (its distances come from a pose the test does not choose) is compared bit for bit when its sum happens
to be exact and within n 2^-53 otherwise (n <= 900: below the 1e-13 of the older a7 tests).  Every match stays at its seed
(STILL).  The last section holds the match itself (eval_at, align, align_batch) to the C oracle at world offsets and leaves
other than the two every other test uses."""
import math

import numpy as np
import pytest

import fitness_workloads as W
from ndt_slam_amd.capi import pack_scans as ragged
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32
IDENT = (F(1.0), F(0.0), F(0.0), F(0.0))
CASES = [(leaf, off) for leaf in W.GPU_LEAVES for off in W.OFFSETS]
# The match must not move the scan: the search is the subject, and a test can only cut a scan by distances it knows before
# the launch.  max_iter = 0 still takes one Newton step (the loop tests its bound at the end); with no voxel allowed a normal
# distribution (min_pts beyond any bucket) there is nothing to step along, and the record's matrix is the seed's.  The
# buckets of raw points, which are all the fitness search reads, do not depend on min_pts.
STILL = dict(max_iter=0, min_pts=1 << 30)


def sse_of(leaf, off):
    """transform_sse of the maps of one (leaf, offset): both forms at every leaf and at every offset."""
    return (W.GPU_LEAVES.index(leaf) + W.OFFSETS.index(off) + 1) % 2


_cache = {}


def prepared(family, leaf, off):
    """(workload, brute-force distances, nearest indices, stratified cuts) of one case, computed once per session."""
    key = (family, leaf, off)
    if key not in _cache:
        w = W.make(family, leaf, off)
        d, arg = W.brute_sq(w.map, w.queries, with_index=True)
        _cache[key] = (w, d, arg, W.stratify(w.queries, d, 900))
    return _cache[key]


def build(gpu, w, sse=1):
    capi, ctx = gpu
    gm = capi.Map(ctx, w.map, capi.default_params(resolution=w.leaf, transform_sse=sse, **STILL))
    i, G = gm.info(), W.grid_of(w.map, w.leaf)
    assert (i.min_bx, i.min_by, i.div_x, i.div_y) == (G.min_bx, G.min_by, G.div_x, G.div_y), (w.family, w.leaf, w.offset)
    assert i.n_points == len(w.map)
    return gm


def T_of(r):
    return (r["T00"], r["T10"], r["T03"], r["T13"])


def check_record(gm, w, r, scan, sse, what, exact_required=False):
    """One record against brute force on the queries its own matrix gives.  -> True if the comparison was bit for bit."""
    assert int(r["status"]) == 0, what
    q = W.queries_of(scan, T_of(r), sse)
    d = W.brute_sq(w.map, q)
    want = W.expected_mean(d)
    exact = W.sum_is_exact(d)
    assert exact or not exact_required, what
    ok = (r["fitness"] == want) if exact else (r["fitness"] == pytest.approx(want, rel=W.loose_rel(len(d)), abs=0.0))
    if not ok:
        c, s, tx, ty = T_of(r)
        pytest.fail("fitness %r, brute force %r (%s).  %s" % (
            float(r["fitness"]), want, "exact sum" if exact else "rel %.2e" % W.loose_rel(len(d)),
            W.localise(lambda sub: gm.fitness_at(sub, c, s, tx, ty), w.map, w.leaf, scan, T_of(r), sse, what=str(what))))
    return exact


def moved_poses(w):
    b, L = W.lattice_base(w.leaf, w.offset)
    return [(b[0] + 3.7 * L, b[1] - 1.9 * L, 0.6), (b[0] - 40.5 * L, b[1] + 27.25 * L, -2.2)]


# ------------------------------------------------------------------------------------------ path 1
@pytest.mark.parametrize("family", list(W.FAMILIES))
def test_fitness_at_equals_brute_force(gpu, family):
    """ndt_fitness_at on the stratified scans of every (leaf, offset): bit-equal.  And scans of ONE point, where the result
    IS the float32 distance (DBL_MAX for a point without one): a strided sample of every case."""
    for leaf, off in CASES:
        w, d, arg, cuts = prepared(family, leaf, off)
        gm = build(gpu, w)
        what = (family, leaf, off)
        for cut in cuts:
            assert W.sum_is_exact(d[cut])
            got = gm.fitness_at(w.queries[cut], *IDENT)
            if got != W.expected_mean(d[cut]):
                pytest.fail(W.localise(lambda s: gm.fitness_at(s, *IDENT), w.map, leaf, w.queries[cut], IDENT, what=str(what)))
        for i in range(W.OFFSETS.index(off), len(w.queries), 37):
            got = gm.fitness_at(w.queries[i:i + 1], *IDENT)
            assert got == (float(d[i]) if np.isfinite(d[i]) else W.DBL_MAX), (what, i, w.queries[i].tolist(), float(d[i]), got)
        gone = W.out_of_reach(w.map[0], 70)
        assert gm.fitness_at(gone, *IDENT) == W.DBL_MAX, what
        gm.close()


# ------------------------------------------------------------------------------------------ paths 2 and 3
@pytest.mark.parametrize("family", list(W.FAMILIES))
def test_batch_with_own_scans_equals_brute_force(gpu, family):
    """Path 2, one ragged launch per map: the stratified scans at the identity pose (the queries ARE the scan points) and
    through two rotations and shifts, both transform forms.  A first launch of the uncut scans (<= 900 points, n 2^-53)
    gives the float32 matrix of every pose; the scans of the second are cut by the distances that matrix gives."""
    n_exact = 0
    for leaf, off in CASES:
        w, d, arg, cuts = prepared(family, leaf, off)
        sse = sse_of(leaf, off)
        gm = build(gpu, w, sse)
        poses = [(0.0, 0.0, 0.0)] + moved_poses(w)
        whole = [w.queries[:900]] + [W.scan_for(w.queries[:900], p) for p in poses[1:]]
        scans, offs = ragged(whole)
        first = gm.align_batch(scans, offs, np.array(poses))
        assert T_of(first[0]) == IDENT
        parts, inits, owner = [], [], []
        for k, r in enumerate(first):
            check_record(gm, w, r, whole[k], sse, (family, leaf, off, "uncut", k))
            dk = W.brute_sq(w.map, W.queries_of(whole[k], T_of(r), sse))
            for cut in W.stratify(None, dk, 900):
                parts.append(whole[k][cut]); inits.append(poses[k]); owner.append(k)
        # a scan of nothing but points out of reach, a scan of NaN points, and both among ordinary points
        gone, nan = W.out_of_reach(w.map[0], 70), np.full((3, 2), np.nan, dtype=F)
        for extra in (gone, nan, np.concatenate([gone[:5], parts[0][:300], nan])):
            parts.append(extra.astype(F)); inits.append(poses[0]); owner.append(0)
        scans, offs = ragged(parts)
        res = gm.align_batch(scans, offs, np.array(inits))
        for b, r in enumerate(res):
            assert T_of(r) == T_of(first[owner[b]]), (family, leaf, off, b)
            n_exact += check_record(gm, w, r, parts[b], sse, (family, leaf, off, "cut", b), exact_required=True)
        assert res[len(parts) - 3]["fitness"] == W.DBL_MAX and res[len(parts) - 2]["fitness"] == W.DBL_MAX
        gm.close()
    assert n_exact >= 6 * len(CASES)


def class_scans(w, d, arg, cuts):
    """name -> scan for the shared-scan launches: the stratified cuts, and scans made of ONE kind of query so that the far
    lists of a match fill its slot completely: all blind (the back list), all far with a point in hand (the front list),
    every far query (both lists, meeting), no far query."""
    cl = W.classify(w.map, w.leaf, w.queries, d, arg)
    G = W.grid_of(w.map, w.leaf)
    mv = W.voxel_of(G, w.map).astype(np.int64)
    qv = W.voxel_of(G, w.queries)
    with np.errstate(invalid="ignore"):
        hx, hy = np.clip(np.nan_to_num(qv[:, 0]), 0, G.div_x - 1), np.clip(np.nan_to_num(qv[:, 1]), 0, G.div_y - 1)
    in_hand = cl["far"] & np.isfinite(d) & (np.maximum(np.abs(mv[arg, 0] - hx), np.abs(mv[arg, 1] - hy)) <= 1)
    out = {"cut%d" % k: w.queries[c] for k, c in enumerate(cuts)}
    masks = {"all_blind": cl["blind"], "all_in_hand": in_hand, "all_far": cl["far"] & np.isfinite(d), "none_far": cl["near"]}
    for name, m in masks.items():                          # (the largest part of each whose sum is exact)
        idx = np.flatnonzero(m)
        if len(idx):
            part = max(W.stratify(None, d[idx], 900), key=len)
            if len(part) >= 40:
                out[name] = w.queries[idx[part]]
    return out, {k: int(v.sum()) for k, v in masks.items()}


@pytest.mark.parametrize("family", list(W.FAMILIES))
def test_shared_scan_equals_brute_force_and_the_own_scan_launch(gpu, family):
    """Path 3: every scan as a `shared_scan` launch with several seeds -- the identity twice (the distances known, the sum
    exact), a small rotation and shift, and a shift of the whole scan by a few voxels (most queries far, with a point in
    hand) and by twenty (every query far and blind or clamped).  Scans of one kind of query fill a match's far lists
    completely from either end.  Every record against brute force, and the launch byte for byte against the same matches
    with scans of their own (path 2: the ring walk instead of the tiles)."""
    n_exact = 0
    filled = dict(all_blind=0, all_in_hand=0, all_far=0, none_far=0)
    for leaf, off in CASES:
        w, d, arg, cuts = prepared(family, leaf, off)
        sse = sse_of(leaf, off)
        gm = build(gpu, w, sse)
        L = float(F(leaf))
        seeds = np.array([(0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (2.3 * L, -3.1 * L, 0.0), (20.5 * L, 23.25 * L, 0.0),
                          (-0.4 * L, 0.3 * L, 0.002)])
        scans, have = class_scans(w, d, arg, cuts)
        for name, scan in scans.items():
            n = len(scan)
            sh = gm.align_batch(scan, np.array([0, n], np.uint64), seeds, shared_scan=True)
            own = gm.align_batch(np.tile(scan, (len(seeds), 1)), (np.arange(len(seeds) + 1) * n).astype(np.uint64), seeds)
            assert sh.tobytes() == own.tobytes(), (family, leaf, off, name)
            assert T_of(sh[0]) == IDENT and sh[0]["fitness"] == sh[1]["fitness"]
            for b, r in enumerate(sh):
                n_exact += check_record(gm, w, r, scan, sse, (family, leaf, off, name, "seed", b), exact_required=b < 2)
            if name in filled:
                filled[name] += 1
        gm.close()
    assert n_exact >= 4 * len(CASES)
    # the family named for a far phase fills the lists it should
    if W.FAMILIES[family] in ("blind", "walk"):
        assert filled["all_blind"] == len(CASES)
    if W.FAMILIES[family] == "far":
        assert filled["all_in_hand"] == len(CASES) and filled["all_far"] == len(CASES) and filled["none_far"] == len(CASES)


# ------------------------------------------------------------------------------------------ MULTI
MULTI_SETS = [("sparse", 0), ("dense1", 1), ("one", 2), ("frame", 3), ("narrow9", 1), ("buckets", 2), ("islands", 3), ("row", 0)]


@pytest.mark.parametrize("leaf", W.GPU_LEAVES)
def test_multi_map_launch_equals_brute_force(gpu, leaf):
    """ndt_align_batch_multi: eight maps of different families, sizes and world offsets at one leaf in ONE launch, the matches
    dealt to the maps by a shuffled map_of -- with scans of their own (every stratified scan of every map, bit-equal) and
    as `shared_scan` (one scan, a seed per match that carries it onto that match's map).  Against brute force on each
    match's own map."""
    capi, ctx = gpu
    prm = capi.default_params(resolution=leaf, **STILL)
    work = [prepared(fam, leaf, W.OFFSETS[oi]) for fam, oi in MULTI_SETS]
    maps = [capi.Map(ctx, w.map, prm) for w, _, _, _ in work]
    parts, map_of = [], []
    for mi, (w, d, arg, cuts) in enumerate(work):
        for cut in cuts:
            parts.append(w.queries[cut]); map_of.append(mi)
    rng = np.random.Generator(np.random.Philox(31))
    order = rng.permutation(len(parts))
    parts, map_of = [parts[i] for i in order], np.array([map_of[i] for i in order], dtype=np.int32)
    assert len(set(map_of.tolist())) == len(maps) and np.any(np.diff(map_of) < 0)
    scans, offs = ragged(parts)
    res = capi.align_batch_multi(ctx, maps, scans, offs, np.zeros((len(parts), 3)), map_of=map_of)
    for b, r in enumerate(res):
        assert T_of(r) == IDENT
        check_record(maps[map_of[b]], work[map_of[b]][0], r, parts[b], 1, (leaf, "multi", b, MULTI_SETS[map_of[b]]), exact_required=True)
    # shared scan: points of a 60 x 60-voxel box around the origin, carried onto map m by the seed (base of m, yaw 0)
    L = float(F(leaf))
    local = (rng.uniform(-6, 66, (900, 2)) * L).astype(F)
    local[::50] = np.nan
    map_of = rng.permutation(np.repeat(np.arange(len(maps)), 3)).astype(np.int32)
    seeds = np.array([[*W.lattice_base(leaf, work[mi][0].offset)[0], 0.0] for mi in map_of])
    seeds[:, :2] += rng.uniform(-2, 2, (len(seeds), 2)) * L
    sh = capi.align_batch_multi(ctx, maps, local, np.array([0, len(local)], np.uint64), seeds, map_of=map_of, shared_scan=True)
    own = capi.align_batch_multi(ctx, maps, np.tile(local, (len(seeds), 1)), (np.arange(len(seeds) + 1) * len(local)).astype(np.uint64),
                                 seeds, map_of=map_of)
    assert sh.tobytes() == own.tobytes()
    for b, r in enumerate(sh):
        check_record(maps[map_of[b]], work[map_of[b]][0], r, local, 1, (leaf, "multi shared", b, MULTI_SETS[map_of[b]]))
    for m in maps:
        m.close()


# ------------------------------------------------------------------------------------------ wave composition
@pytest.mark.parametrize("leaf,oi", [(0.3, 1), (0.1, 3), (1.0, 0)])
def test_ring_work_of_a_wave_at_every_composition(gpu, leaf, oi):
    """The joint ring-1 work of a wave (nearest_ring1_wave) is used when 1 .. 12 of its lanes need ring 1; with none it is
    skipped and from 13 on every lane walks alone.  A scan above the sort limit (20000 points: NDT_FLAG_UNSORTED) is read in
    input order, so chunk j of 64 points holds exactly WAVE_CHUNKS[j] ring-needing queries -- 0, 1, 12, 13, 64 and values
    between -- beside queries on map points and blind ones; chunks of far and clamped queries follow.  The distances are
    drawn from a window of binades that keeps the 20k-point sum exact: bit-equal, paths 1, 2 and 3."""
    capi, ctx = gpu
    w = W.make("sparse", leaf, W.OFFSETS[oi])
    q = W.wave_scan(w, W.WAVE_CHUNKS)
    d, arg = W.brute_sq(w.map, q, with_index=True)
    cl = W.classify(w.map, leaf, q, d, arg)
    for j, k in enumerate(W.WAVE_CHUNKS):
        s = slice(64 * j, 64 * j + 64)
        assert int(cl["ring1"][s].sum()) == k and int(cl["quiet"][s].sum()) == 64 - k, (j, k)
    tail = slice(64 * len(W.WAVE_CHUNKS), len(q))
    assert len(q) > 20000 and int(cl["far"][tail].sum()) >= 200 and int(cl["clamped"][tail].sum()) >= 200
    assert W.sum_is_exact(d)
    want = W.expected_mean(d)
    for sse in (1, 0):
        gm = build(gpu, w, sse)
        seeds = np.zeros((3, 3))
        own = gm.align_batch(np.tile(q, (3, 1)), (np.arange(4) * len(q)).astype(np.uint64), seeds)
        sh = gm.align_batch(q, np.array([0, len(q)], np.uint64), seeds, shared_scan=True)
        assert np.all(own["status"] == 0) and np.all(own["flags"] & capi.FLAG_UNSORTED), own["flags"]
        assert sh.tobytes() == own.tobytes()
        for r in own:
            assert T_of(r) == IDENT
            if r["fitness"] != want:
                pytest.fail(W.localise(lambda s: gm.fitness_at(s, *IDENT), w.map, leaf, q, IDENT, what="wave scan, leaf %r" % leaf))
        assert gm.fitness_at(q, *IDENT) == want
        gm.close()


# ------------------------------------------------------------------------------------------ the match at other geometries
@pytest.mark.parametrize("off", W.MATCH_OFFSETS)
@pytest.mark.parametrize("leaf", W.MATCH_LEAVES)
def test_match_at_an_offset_and_other_leaves(gpu, oracle, leaf, off):
    """eval_at (same neighbour pairs, score / gradient / Hessian at the tolerances of test_single_evaluation_matches_oracle),
    align and a 24-scan align_batch (the exact-path parity of test_gpu_parity) against the C oracle, for the C1 wall world
    moved 1.2 km and 2.5 km from the origin at leaves 0.1, 0.3 and 1 m."""
    from test_gpu_parity import assert_result_parity
    capi, ctx = gpu
    m, make = W.shifted_world(off)
    gm = capi.Map(ctx, m, capi.default_params(resolution=leaf))
    om = oracle.Map(m, oracle.default_params(resolution=leaf))
    gi, oi = gm.info(), om.info()
    assert (gi.min_bx, gi.min_by, gi.div_x, gi.div_y, gi.n_cells, gi.n_valid) == (oi.min_bx, oi.min_by, oi.div_x, oi.div_y, oi.n_cells, oi.n_valid)
    for k in range(3):
        scan, truth, init = make(k)
        for p in (init, truth, [truth[0], truth[1], 5e-5]):
            s, g, H, pairs = gm.eval_at(scan, p)
            s0, g0, H0, pairs0 = om.eval_at(scan, p)
            assert pairs == pairs0
            assert s == pytest.approx(s0, rel=1e-12, abs=1e-300)
            assert g == pytest.approx(g0, rel=1e-9, abs=1e-10 * (np.abs(g0).max() + 1e-300))
            assert H == pytest.approx(H0, rel=1e-9, abs=1e-10 * (np.abs(H0).max() + 1e-300))
        assert_result_parity(gm.align(scan, init), om.align(scan, init, run_stats=True))
    made = [make(k) for k in range(24)]
    scans, offs = ragged([x[0] for x in made])
    inits = np.array([x[2] for x in made])
    res = gm.align_batch(scans, offs, inits)
    ref = om.align_batch(scans, offs, inits, nthreads=4, run_stats=True)
    for b in range(24):
        assert_result_parity(res[b], ref[b])
    gm.close()
