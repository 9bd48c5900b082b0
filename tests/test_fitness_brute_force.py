"""The fitness reference held to brute force, on the CPU (row a7).

tests/fitness_workloads.py builds maps the synthetic wall worlds never produce -- one voxel, one row, one column, grids
narrower than an occupancy tile, a voxel with 5001 points, points and queries on the voxel lattice, islands far apart --
at leaves whose float32 reciprocal rounds every way and at world offsets up to 8 km.  Here the CPU oracle's ring search
(oracle/ndt_oracle.c, fitness_pass) is compared with the minimum over ALL map points on every one of them: bit for bit on
scans cut so that their fp64 sum is exact in any order (fitness_workloads.stratify).  The module also holds the workloads to
what they claim (classify), so that none can stop reaching the phase it is named for without a test failing.
tests/test_gpu_fitness_geometry.py runs the same workloads through the three device paths."""
import math

import numpy as np
import pytest

import fitness_workloads as W

F = np.float32
IDENT = (F(1.0), F(0.0), F(0.0), F(0.0))


_cache = {}


def prepared(family, leaf, off):
    """(workload, brute-force distances, nearest indices) of one case, computed once per session."""
    key = (family, leaf, off)
    if key not in _cache:
        w = W.make(family, leaf, off)
        _cache[key] = (w,) + W.brute_sq(w.map, w.queries, with_index=True)
    return _cache[key]


def oracle_map(oracle, map_xy, leaf, **kw):
    return oracle.Map(map_xy, oracle.default_params(resolution=leaf, **kw))


# ------------------------------------------------------------------------------------------ the helpers themselves
def test_brute_sq_against_a_plain_double_loop():
    rng = np.random.Generator(np.random.Philox(5))
    m = (rng.normal(0, 3, (37, 2)) + [1003.3, -707.1]).astype(F)
    q = (rng.normal(0, 5, (23, 2)) + [1003.3, -707.1]).astype(F)
    q[3] = m[11]
    q[5, 0] = np.nan
    q[7] = [3e19, -3e19]
    d, arg = W.brute_sq(m, q, with_index=True, pairs_per_chunk=100)       # (several chunks)
    for i in range(len(q)):
        best, at = F(np.inf), 0
        for j in range(len(m)):
            ex, ey = F(q[i, 0] - m[j, 0]), F(q[i, 1] - m[j, 1])
            with np.errstate(over="ignore", invalid="ignore"):
                dd = F(F(ex * ex) + F(ey * ey))
            if dd < best:
                best, at = dd, j
        if i == 5:
            assert np.isnan(d[i])
        else:
            assert d[i] == best and (arg[i] == at or i == 7), i
    assert d[3] == 0.0 and np.isinf(d[7])
    assert W.expected_mean(d) == math.fsum(float(x) for x in d if np.isfinite(x)) / 21
    assert W.expected_mean(d[[5, 7]]) == W.DBL_MAX and W.expected_mean(d[:0]) == W.DBL_MAX


def test_queries_of_is_the_oracles_transform(oracle):
    """Both transform_sse forms: a one-point map makes the oracle's fitness the squared distance of the moved point."""
    rng = np.random.Generator(np.random.Philox(6))
    scan = rng.normal(0, 20, (64, 2)).astype(F)
    T = (F(math.cos(0.7)), F(math.sin(0.7)), F(-1003.3), F(707.1))
    m = np.array([[-1000.0, 700.0]], dtype=F)
    for sse in (1, 0):
        om = oracle_map(oracle, m, 0.3, transform_sse=sse)
        q = W.queries_of(scan, T, sse)
        d = W.brute_sq(m, q)
        for i in range(len(scan)):
            assert om.fitness(scan[i:i + 1], *T) == float(d[i])
    assert W.queries_of(scan, IDENT).tobytes() == scan.tobytes()


def test_stratify_gives_scans_whose_sum_is_exact():
    rng = np.random.Generator(np.random.Philox(7))
    d = (10.0 ** rng.uniform(-12, 9, 5000)).astype(F)
    d[::17] = 0.0
    d[5::101] = np.inf
    d[9::103] = np.nan
    for n_max in (64, 900, 4096):
        cuts = W.stratify(None, d, n_max)
        assert np.array_equal(np.sort(np.concatenate(cuts)), np.arange(len(d)))
        for c in cuts:
            assert 0 < len(c) <= n_max and np.all(np.diff(c) > 0)
            assert W.binades(d[c]) <= W.max_binades(n_max) and W.sum_is_exact(d[c])
            # exact means: whatever the order, the running fp64 sum is the exact sum
            v = d[c][np.isfinite(d[c])].astype(np.float64)
            for _ in range(3):
                rng.shuffle(v)
                assert float(np.cumsum(v)[-1]) == math.fsum(v.tolist())
                assert float(np.add.reduce(v)) == math.fsum(v.tolist())       # (pairwise: another order)
    assert not W.sum_is_exact(d)                          # (and the unstratified set is not)
    assert W.max_binades(900) == 19 and W.max_binades(20480) == 14 and W.loose_rel(900) < 1e-13


# ------------------------------------------------------------------------------------------ the workloads' claims
@pytest.mark.parametrize("family", list(W.FAMILIES))
def test_family_reaches_the_phase_it_is_named_for(family):
    phase = W.FAMILIES[family]
    for leaf in W.LEAVES:
        for off in W.OFFSETS:
            w, d, arg = prepared(family, leaf, off)
            if leaf == 0.3:                               # (the generators are deterministic)
                again = W.make(family, leaf, off)
                assert w.map.tobytes() == again.map.tobytes() and w.queries.tobytes() == again.queries.tobytes()
            cl = W.classify(w.map, leaf, w.queries, d, arg)
            c = W.counts(cl)
            assert c[phase] >= W.MIN_SHARE * c["live"], (family, leaf, off, c)
            G = W.grid_of(w.map, leaf)
            want = W.GRID_OF.get(family, (None, None))
            assert want[0] in (None, G.div_x) and want[1] in (None, G.div_y), (family, leaf, off, G)
            # every family: queries on the lattice, on map points, outside the grid
            assert c["on_wall"] >= 0.15 * c["live"] and int((d == 0).sum()) >= 20 and c["clamped"] >= 50, (family, leaf, off, c)
            if family == "one":
                v = W.voxel_of(G, w.queries)
                for sx in (-1, 0, 1):                     # every side and corner, and 10^2 voxels out and more
                    for sy in (-1, 0, 1):
                        assert int(((np.sign(v[:, 0]) == sx) & (np.sign(v[:, 1]) == sy)).sum()) >= 5, (sx, sy)
                assert int((np.abs(v).max(axis=1) >= 100).sum()) >= 10
            if family == "dense1":
                mv = W.voxel_of(G, w.map).astype(np.int64)
                cells, n_in = np.unique(mv, axis=0, return_counts=True)
                assert n_in.max() >= 5001
                hv = cells[np.argmax(n_in)]
                ring = np.abs(W.voxel_of(G, w.queries) - hv[None, :]).max(axis=1)
                for r in (0, 1, 2):                       # from inside, from the neighbours, from two voxels away
                    assert int((ring == r).sum()) >= 15, (r, leaf, off)
            if family == "buckets":
                mv = W.voxel_of(G, w.map).astype(np.int64)
                cnt = np.zeros((G.div_y, G.div_x), dtype=np.int64)
                np.add.at(cnt, (mv[:, 1], mv[:, 0]), 1)
                assert cnt[1].tolist() == list(range(1, 31)) and cnt[3].tolist() == list(range(30, 0, -1))
                start = np.concatenate([[0], np.cumsum(cnt.ravel())])[:-1].reshape(cnt.shape)
                for row in (1, 3):                        # both parities of the first point, pair counts about 6 and 12
                    seen = {(int(s) & 1, int(n - (s & 1)) >> 1) for s, n in zip(start[row], cnt[row])}
                    for pairs in (0, 1, 5, 6, 7, 11, 12, 13):
                        assert (0, pairs) in seen or (1, pairs) in seen, (row, pairs)
                    assert {p for p, _ in seen} == {0, 1}


@pytest.mark.parametrize("leaf,oi", [(0.3, 1), (0.1, 3), (1.0, 0)])
def test_wave_scan_holds_the_compositions_it_claims(leaf, oi):
    chunks = W.WAVE_CHUNKS
    assert len(chunks) * 64 > 20000 and {0, 1, 12, 13, 64} <= set(chunks)
    w = W.make("sparse", leaf, W.OFFSETS[oi])
    q = W.wave_scan(w, chunks)
    d, arg = W.brute_sq(w.map, q, with_index=True)
    cl = W.classify(w.map, w.leaf, q, d, arg)
    for j, k in enumerate(chunks):
        s = slice(64 * j, 64 * j + 64)
        assert int(cl["ring1"][s].sum()) == k and int(cl["quiet"][s].sum()) == 64 - k, (j, k)
    tail = slice(64 * len(chunks), len(q))
    assert int(cl["far"][tail].sum()) >= 200 and int(cl["clamped"][tail].sum()) >= 200
    assert W.sum_is_exact(d) and len(q) == 64 * len(chunks) + 640


# ------------------------------------------------------------------------------------------ the oracle against brute force
@pytest.mark.parametrize("family", list(W.FAMILIES))
def test_oracle_fitness_equals_brute_force(oracle, family, record_property):
    """Bit-equal on every stratified scan of every (leaf, offset): the oracle adds the distances in input order, the sum of
    such a scan is exact in any order.  The whole query set (not stratified) within n 2^-53."""
    n_strat = 0
    for leaf in W.LEAVES:
        for off in W.OFFSETS:
            w, d, _ = prepared(family, leaf, off)
            om = oracle_map(oracle, w.map, leaf)
            i = om.info()
            G = W.grid_of(w.map, leaf)
            assert (i.min_bx, i.min_by, i.div_x, i.div_y) == (G.min_bx, G.min_by, G.div_x, G.div_y)
            for cut in W.stratify(w.queries, d, 1024):
                assert W.sum_is_exact(d[cut])
                got = om.fitness(w.queries[cut], *IDENT)
                if got != W.expected_mean(d[cut]):
                    pytest.fail(W.localise(lambda s: om.fitness(s, *IDENT), w.map, leaf, w.queries[cut], IDENT,
                                           what="oracle, %s leaf %r offset %r" % (family, leaf, off)))
                n_strat += 1
            assert om.fitness(w.queries, *IDENT) == pytest.approx(W.expected_mean(d), rel=W.loose_rel(len(d)), abs=0.0)
    record_property("stratified_scans_bit_equal", n_strat)
    print("%s: oracle bit-equal to brute force on %d stratified scans" % (family, n_strat))
    assert n_strat >= len(W.LEAVES) * len(W.OFFSETS)


@pytest.mark.parametrize("sse", [1, 0])
def test_oracle_fitness_at_moved_poses_equals_brute_force(oracle, sse):
    """The same through a rotation and a shift (both transform forms): the queries are the float32 transform of the scan."""
    for family in ("sparse", "lattice", "one", "frame"):
        for leaf, off in ((0.07, W.OFFSETS[1]), (0.5, W.OFFSETS[3])):
            w = W.make(family, leaf, off)
            om = oracle_map(oracle, w.map, leaf, transform_sse=sse)
            pose = (off[0] + 3.7 * leaf, off[1] - 1.9 * leaf, 0.6)
            T = (F(math.cos(pose[2])), F(math.sin(pose[2])), F(pose[0]), F(pose[1]))
            scan = W.scan_for(w.queries, pose)
            q = W.queries_of(scan, T, sse)
            d = W.brute_sq(w.map, q)
            for cut in W.stratify(q, d, 1024):
                assert om.fitness(scan[cut], *T) == W.expected_mean(d[cut]), (family, leaf, off)


def test_oracle_fitness_of_degenerate_scans(oracle):
    """A scan with nothing in reach (every float32 distance overflows) and NaN points: DBL_MAX, as the reference's
    getFitnessScore gives for no correspondence; such points among others are not counted; an empty scan."""
    for family in ("one", "row", "sparse"):
        w = W.make(family, 0.3, W.OFFSETS[2])
        om = oracle_map(oracle, w.map, 0.3)
        gone = W.out_of_reach(w.map[0], 70)
        assert np.isinf(W.brute_sq(w.map, gone)).all()
        assert om.fitness(gone, *IDENT) == W.DBL_MAX
        nan = np.full((5, 2), np.nan, dtype=F)
        assert om.fitness(nan, *IDENT) == W.DBL_MAX
        assert om.fitness(np.zeros((0, 2), dtype=F), *IDENT) == W.DBL_MAX
        mixed = np.concatenate([gone[:3], w.queries[:200], nan[:2], [[np.nan, w.map[0, 1]], [w.map[0, 0], np.inf]]]).astype(F)
        d = W.brute_sq(w.map, mixed)
        assert int(np.isfinite(d).sum()) == 200
        for cut in W.stratify(mixed, d, 1024):
            assert om.fitness(mixed[cut], *IDENT) == W.expected_mean(d[cut])
