"""The map-build families of tests/map_build_workloads.py on the CPU: the path census (every family reaches the paths it
is for, all together reach every path, both sides of every constant), their teeth (the voxels a family is for change a
bit under every other order of their points), and the C oracle against the exact rational reference and against the NumPy
restatement -- so that what tests/test_gpu_map_build_geometry.py holds the device to is itself held to something that
shares no code with it."""
import numpy as np
import pytest

from oracle import ndt_numpy as NP

import map_build_workloads as W

COMBOS = [(leaf, off) for leaf in W.LEAVES for off in W.OFFSETS]
IDS = ["leaf%g@%g,%g" % (leaf, off[0], off[1]) for leaf, off in COMBOS]
ACCEPTED = ("accept", "raise1", "raise2")
# For a planar cloud czz is the identity start's share of the sums, and cxx and cyy hold the same share: czz <= l1 in exact
# arithmetic, always.  The second and third ordering of {l1, l2, czz} in leaf_finalize are reached only through rounding
# (identical points far from the origin, where l1 = czz + noise), never by construction.
UNREACHABLE = ("leaf:z_mid", "leaf:z_last")
_CENSUS = {}


def census(leaf, off):
    """[(case, table, {label: voxels}, {voxel: Exact}, r2)] of one (leaf, offset), once."""
    key = (leaf, off)
    if key not in _CENSUS:
        rows = []
        for c in W.cases(leaf, off):
            T, got = W.paths_of(c.cloud, c.leaf)
            _, ex, r2 = W.exact_cells(c)
            for g, e in ex.items():
                for lab in e.labels:
                    got.setdefault(lab, []).append(g)
            rows.append((c, T, got, ex, r2))
        _CENSUS[key] = rows
    return _CENSUS[key]


def leaf_case_of(T, g):
    """The name of the `leaves` case in voxel g (one grid row, every second voxel, from the first)."""
    assert T.grid.div_y == 1 and g % 2 == 0
    return W.LEAF_CASES[g // 2]


_SENSITIVE = {}


def sensitive(c, T, g):
    """order_sensitive of voxel g of a case, once per cloud (the parameter variants of a family share theirs)."""
    key = (id(c.cloud), g)
    if key not in _SENSITIVE:
        _SENSITIVE[key] = W.order_sensitive(c.cloud[T.members[g]])
    return _SENSITIVE[key]


def toothed(c, T, label, voxels):
    """The voxels of a label that count: cloud-level labels (voxel -1) as they are, voxels by their order sensitivity."""
    if voxels[0] < 0:
        return voxels
    if c.family == "leaves":
        return [g for g in voxels if leaf_case_of(T, g) in W.LEAF_INSENSITIVE or sensitive(c, T, g)]
    return [g for g in voxels if sensitive(c, T, g)]


@pytest.mark.parametrize("leaf,off", COMBOS, ids=IDS)
def test_every_family_reaches_the_paths_it_is_for(leaf, off):
    """Every label of a case's purpose is in its census, on voxels with teeth: every voxel of three or more points under a
    per-voxel label of the purpose is order-sensitive (reverse and eight random orders each change a bit of the float32
    centroid sum or an fp64 sum), and at least one such voxel exists."""
    for c, T, got, ex, _ in census(leaf, off):
        assert c.purpose <= set(got), (c.name, sorted(c.purpose - set(got)))
        for label in sorted(c.purpose):
            voxels = got[label]
            if voxels[0] < 0 or label.startswith("leaf:"):
                continue
            ok = toothed(c, T, label, voxels)
            assert ok, (c.name, label, "no order-sensitive voxel")
            blunt = [g for g in voxels if g not in ok and len(T.members[g]) >= 3]
            assert not blunt, (c.name, label, blunt)
        if c.family == "leaves":
            for g, m in T.members.items():
                name = leaf_case_of(T, g)
                assert name in W.LEAF_INSENSITIVE or sensitive(c, T, g), (c.name, name)


def test_all_families_together_reach_every_path():
    """Every order path, both finalize paths, both sides of kBigVoxel, kBigRuns, kBigStage, kFinStage and kScanTile, every
    remainder of the streamed loop and of the 4-wide rank, and every reachable branch and return of leaf_finalize -- each
    on a voxel with teeth where the label is per voxel.  The census is printed (pytest -s) for LOG.md."""
    reached = {}
    for leaf, off in COMBOS:
        for c, T, got, ex, _ in census(leaf, off):
            for label, voxels in got.items():
                if label.startswith("leaf:") or toothed(c, T, label, voxels):
                    reached.setdefault(label, set()).add(c.name)
    print()
    for label in W.ALL_PATHS + W.ALL_LEAF:
        names = sorted(reached.get(label, ()))
        print("  census %-22s %3d cases: %s" % (label, len(names), ", ".join(names[:4]) + (" ..." if len(names) > 4 else "")))
    missing = [p for p in W.ALL_PATHS + W.ALL_LEAF if p not in reached and p not in UNREACHABLE]
    assert not missing, missing
    assert not [p for p in UNREACHABLE if p in reached], "a planar cloud reached an ordering of czz that needs czz > l1"


def _oracle_table(oracle, c):
    prm = oracle.default_params(resolution=c.leaf, **W.params_of(c))
    t = oracle.Map(c.cloud, prm).export()
    return t, {int(g): k for k, g in enumerate(t["idx"])}


@pytest.mark.parametrize("leaf,off", COMBOS, ids=IDS)
def test_oracle_against_the_exact_reference(oracle, leaf, off):
    """The C oracle on every family against exact_leaf.  Every occupied voxel of min_pts or more points is a cell, with the
    count numpy's float32 floor gives it (`holes`: lattice points, -0.0, denormals, non-finite points dropped).  On decided
    voxels: the same decision; the mean within n ulps of the exact mean; the inverse covariance within
      (n ulp(r^2) max|icov| + 36 * 2^-53 * kappa) * max|icov|
    -- the first-order effect of the one-pass covariance's rounding (docstring of
    test_c_vs_numpy_at_an_offset_and_other_leaves) plus the rounding of the 36 operations from the covariance to its
    inverse, two of which cancel to 1 / kappa (map_build_workloads.REBUILD_OPS).  The worst ratio per family is printed."""
    worst = {}
    for c, T, got, ex, r2 in census(leaf, off):
        t, look = _oracle_table(oracle, c)
        cells = {g for g, e in ex.items() if e.decision != "below"}
        assert set(look) == cells, c.name
        for g in cells:
            e, k = ex[g], look[g]
            assert abs(int(t["npts"][k])) == e.n == len(T.members[g]), (c.name, g)
            if not e.decided:
                continue
            assert (t["npts"][k] > 0) == (e.decision in ACCEPTED), (c.name, g, e.decision, int(t["npts"][k]))
            mb = W.mean_bound(e)
            assert abs(t["mean"][k][0] - e.mean[0]) <= mb[0] and abs(t["mean"][k][1] - e.mean[1]) <= mb[1], (c.name, g)
            if e.icov is None:
                assert not t["icov"][k].any(), (c.name, g)              # rejected: the inverse stays zero
                continue
            ratio = float(np.abs(t["icov"][k] - np.array(e.icov)).max() / W.icov_bound(e, r2))
            assert ratio <= 1.0, (c.name, g, e.n, e.decision, ratio)
            if ratio > worst.get(c.family, (0.0,))[0]:
                worst[c.family] = (ratio, c.name, e.n, e.decision)
    print("\n  oracle / exact, worst |d icov| over its bound:", ", ".join("%s %.3f" % (f, v[0]) for f, v in sorted(worst.items())))


def undecided_by_design(c, T, g, e):
    """Why a voxel may be undecided (None: it may not).  margin = 16 n ulp(r^2), r^2 the cloud's largest x^2 + y^2."""
    far = c.offset == W.FAR_OFFSET and c.leaf == 0.1
    if c.family == "sizes" and far and e.n == 5001:
        return "margin 16 * 5001 * 2^-25 = 2.4e-3 m^2 against eigenvalues of 7e-4 m^2 (a 0.1 m voxel 11.6 km out)"
    if c.family != "leaves":
        return None
    name, P = leaf_case_of(T, g), W.params_of(c)
    if not P["cov_init_identity"]:
        if name in ("line_x", "line_y", "line_d", "identical"):
            return "l1 is exactly zero: a rounding residue of either sign decides"
        if name == "ulps":
            return "a spread of three float32 steps: a variance of 2^-46 r^2 against a margin of 144 * 2^-52 r^2"
        if far and name in ("ellipse_x", "ellipse_y", "ellipse_d"):
            return "a short axis of four float32 steps (4e-3 m) 11.6 km out: l1 = 1e-5 m^2, the margin is 1.1e-5 m^2"
    if P["eig_mult"] == 1.0 and name in ("square", "identical", "ulps"):
        return "l1 equals l2 (or nearly), and with eig_mult 1 the threshold IS l2: a tie by construction"
    return None


@pytest.mark.parametrize("leaf,off", COMBOS, ids=IDS)
def test_only_the_named_voxels_are_undecided(leaf, off):
    """Every voxel of every family is decided -- the exact eigenvalues lie further from zero and from the threshold than 16
    times the rounding of the one-pass covariance -- but for the cases `undecided_by_design` names: the exactly collinear
    and identical-point cases without the identity start, everywhere; ties built on purpose; and, at leaf 0.1 at
    (8191.7, 8191.7) alone, the voxels whose smallest eigenvalue the offset's float32 grid swamps."""
    for c, T, got, ex, _ in census(leaf, off):
        for g, e in ex.items():
            if not e.decided:
                assert undecided_by_design(c, T, g, e), (c.name, g, e.n, e.decision, e.l1, e.thr, e.margin)


def test_the_oracle_returns_minus_one_on_collinear_points(oracle):
    """eig_mult 0, no identity start, exactly collinear points: nothing is raised and the determinant is zero or a rounding
    residue.  The oracle takes leaf_finalize's third return for at least the axis-parallel lines: the cell stays in the
    table, flagged rejected, with an infinite inverse (PCL keeps icov_ as computed)."""
    seen = []
    for leaf, off in COMBOS:
        for c in W.cases(leaf, off, "leaves"):
            if c.prm["eig_mult"] == 0.0 and not c.prm["cov_init_identity"]:
                t, look = _oracle_table(oracle, c)
                for name in ("line_x", "line_y", "line_d"):
                    k = look[2 * W.LEAF_CASES.index(name)]
                    if np.isinf(t["icov"][k]).any():
                        assert t["npts"][k] < 0
                        seen.append((leaf, off, c.name, name))
    assert len(seen) >= len(COMBOS), seen


@pytest.mark.parametrize("leaf,off", COMBOS, ids=IDS)
def test_oracle_against_the_numpy_restatement(oracle, leaf, off):
    """The C oracle against oracle/ndt_numpy.py `Cells` (eigh, general inverse) on every family, as
    test_cell_table_c_vs_numpy does on the C1 wall world: the cells, and on decided voxels the signed counts and the
    float32 centroids, equal."""
    for c, T, got, ex, _ in census(leaf, off):
        P = W.params_of(c)
        fin = np.isfinite(c.cloud).all(axis=1)              # (Cells takes the bounding box with numpy's min: no NaN)
        cells = NP.Cells(c.cloud[fin], leaf, min_pts=P["min_pts"], eig_mult=P["eig_mult"], unbiased=bool(P["cov_unbiased"]),
                         init_identity=bool(P["cov_init_identity"]))
        t, look = _oracle_table(oracle, c)
        assert np.array_equal(t["idx"], cells.idx), c.name
        assert np.array_equal(np.abs(t["npts"]), np.abs(cells.npts)), c.name
        dec = np.array([ex[int(g)].decided for g in t["idx"]], dtype=bool)
        assert np.array_equal(t["npts"][dec], cells.npts[dec]), c.name
        assert np.array_equal(t["cent"][dec], cells.cent[dec]), c.name
