"""The inputs of tests/optimizer_cases.py on the CPU: do they reach the branches they claim (the oracle's census), are the
matches fair comparisons (stable under permutations of the point order), and is the oracle -- the GPU tests' yardstick --
right on them (mpmath at 50 digits, the vendored Eigen's JacobiSVD fixture)?  tests/test_gpu_optimizer_branches.py then holds
the device to the oracle on the same inputs."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import optimizer_cases as OC      # noqa: E402

import mpmath as mp      # noqa: E402
EPS = OC.EPS
U = EPS / 2                       # unit roundoff of fp64


@pytest.fixture(scope="module")
def maps(oracle, c1_world):
    m, _, cfg = c1_world
    return {k: oracle.Map(m, oracle.default_params(resolution=cfg["resolution"], **kw)) for k, kw in OC.PARAM_SETS.items()}


@pytest.fixture(scope="module")
def runs(oracle, c1_world, maps):
    """Every match of the list through the oracle once: [(entry, scan, init, result, trace, census of this match)]."""
    out = []
    for e in OC.MATCHES:
        scan, init = OC.match_inputs(c1_world, e)
        oracle.census_reset()
        res, tr = maps[e[0]].align(scan, init, trace_cap=512)
        out.append((e, scan, init, res, tr, oracle.census_get()))
    return out


def _total(censuses):
    tot = {}
    for c in censuses:
        for k, v in c.items():
            tot[k] = tot.get(k, 0) + v
    return tot


# ------------------------------------------------------------------------------------------------------------ census
def test_match_list_reaches_the_branches_of_its_table(oracle, c1_world, maps, runs):
    assert 80 <= len(OC.MATCHES) <= 140 and len(set(OC.MATCHES)) == len(OC.MATCHES)
    assert {e[0] for e in OC.MATCHES} == set(OC.PARAM_SETS)
    tot = _total(r[5] for r in runs)
    oracle.census_reset()
    for name, pset, scan, init in OC.special_matches(c1_world):
        maps[pset].align(scan, init)
    special = oracle.census_get()
    print("census of the match list:", {k: v for k, v in tot.items() if v})
    print("census of the special scans:", {k: v for k, v in special.items() if v})
    for k, least in OC.MATCH_BRANCHES.items():
        assert tot[k] + special[k] >= least, (k, tot[k], special[k])
    # the tables name every branch once: one the matches reach without a claim is a claim to add, one they are said not to
    # reach and do is a line to correct
    assert sorted(list(OC.MATCH_BRANCHES) + list(OC.MATCH_UNREACHED)) == sorted(oracle.CENSUS_NAMES)
    assert set(OC.NEVER_REACHED) <= set(OC.MATCH_UNREACHED)
    for k in OC.MATCH_UNREACHED:
        assert tot[k] + special[k] == 0, (k, tot[k], special[k])
    # a dropped eigenvalue of a non-zero matrix: the yaw eigenvalue of the origin copies, and no other
    assert OC.nonzero_drops(tot) == [0, 0, 0]
    nz = OC.nonzero_drops(special)
    assert nz[:2] == [0, 0] and nz[2] >= OC.MATCH_NONZERO_DROP2, nz
    # the origin copies: a zero yaw row (rank 2: the yaw eigenvalue dropped) with a non-zero gradient, and a step taken
    oracle.census_reset()
    for name, pset, scan, init in OC.special_matches(c1_world):
        if name.startswith("origin_copies"):
            r, tr = maps[pset].align(scan, init, trace_cap=64)
            assert np.all(r["H"].reshape(3, 3)[2] == 0.0) and np.any(tr[0, 2:4] != 0.0) and tr[0, 4] == 0.0 and r["iters"] > 0, name
    c = oracle.census_get()
    assert c["s3_jacobi_nonzero"] >= 3 and OC.nonzero_drops(c)[2] >= OC.MATCH_NONZERO_DROP2


def test_degenerate_scans_end_as_the_contract_says(oracle, c1_world, maps):
    """include/ndt_mi355x.h (ndt_align): no point with a finite image in reach of a voxel -> zero Newton step,
    iters 0, converged 1, the parameter vector and matrix of the guess; fitness DBL_MAX when no image is finite."""
    for name, pset, scan, init in OC.special_matches(c1_world):
        if name not in OC.SPECIAL_DEGENERATE:
            continue
        oracle.census_reset()
        r, tr = maps[pset].align(scan, init, trace_cap=8)
        c = oracle.census_get()
        assert (int(r["status"]), int(r["iters"]), int(r["converged"]), len(tr)) == (0, 0, 1, 1), name
        assert c["exit_nrm_zero"] == 1 and c["s3_jacobi"] == 1 and c["s3_jacobi_nonzero"] == 0 and c["s3_nan"] == 0, name
        assert r["score"] == 0.0 and np.all(r["H"] == 0.0), name
        if "nan" in name:
            assert r["fitness"] == np.finfo(np.float64).max, name
        if "guess" in name:
            assert np.isnan(r["pose"]).any() and (np.isnan(r["T00"]) or np.isnan(r["T03"])), name


def test_unit_rows_reach_every_branch_of_solve3(oracle):
    rows, groups = OC.solve3_rows()
    assert len(rows) >= 2000
    per_group = {}
    for name, sl in groups.items():
        oracle.census_reset()
        for r in rows[sl]:
            H, b = OC.rows_to_matrix(r)
            oracle.solve3(H, b)
        per_group[name] = oracle.census_get()
    tot = _total(per_group.values())
    print("solve3 census:", {k: v for k, v in tot.items() if k.startswith("s3_")})
    for k in oracle.CENSUS_NAMES:
        if k.startswith("s3_"):
            assert tot[k] >= 6, (k, tot[k])
    assert per_group["nan_entry"]["s3_nan"] == 6
    one = per_group["one_pair"]
    for k in ("s3_rot01", "s3_rot02", "s3_rot12", "s3_skip01", "s3_skip02", "s3_skip12"):
        assert one[k] >= 6, (k, one[k])
    assert per_group["svd6"]["s3_jacobi_nonzero"] >= 20 and per_group["exact_rank"]["s3_adjugate"] == 0
    assert per_group["scales"]["s3_jacobi_nonzero"] >= 10 and per_group["scales"]["s3_drop0"] + per_group["scales"]["s3_drop1"] >= 1


@pytest.fixture(scope="module")
def mt_all(oracle, c1_world, maps):
    harvested = OC.harvest_mt_rows(oracle, c1_world, maps)
    return OC.mt_rows(harvested)


def test_unit_rows_reach_every_branch_of_mt_trial_and_mt_update(oracle, mt_all):
    rows, groups = mt_all
    assert len(rows) >= 3000 and groups["harvested"].stop - groups["harvested"].start >= 100
    per_group = {}
    for name, sl in groups.items():
        oracle.census_reset()
        for r in rows[sl]:
            oracle.mt_trial(*r)
            oracle.mt_update(*r)
        per_group[name] = oracle.census_get()
    tot = _total(per_group.values())
    print("mt census:", {k: v for k, v in tot.items() if k.startswith(("mt_", "mu_"))})
    made = _total(per_group[g] for g in per_group if g != "harvested")        # the constructed rows alone reach every branch
    for k in oracle.CENSUS_NAMES:
        if k.startswith(("mt_", "mu_")):
            assert made[k] >= 10, (k, made[k])
    assert per_group["independent"]["mt_nan"] >= 20 and per_group["ties"]["mu_converged"] >= 10


# ------------------------------------------------------------------------------------------------------------ stability
def test_every_match_keeps_its_trace_under_permutations_of_the_point_order(oracle, c1_world, maps, runs):
    """A condition on the INPUTS: the device sums a scan's terms in another order than the oracle, so a match whose path
    depends on the order of summation (a branch decided by a rounding) compares nothing.  Such an entry is replaced in
    optimizer_cases.MATCHES; the GPU test leaves no entry out."""
    for e, scan, init, res, tr, _ in runs:
        assert len(tr) == int(res["flags"]) <= 512, e
        for j in range(1, 9):
            r2, tr2 = maps[e[0]].align(OC.permuted(scan, j), init, trace_cap=512)
            assert OC.traces_agree(tr2, tr), (e, j)
            assert (int(r2["iters"]), int(r2["converged"]), int(r2["ref_evals"])) == \
                   (int(res["iters"]), int(res["converged"]), int(res["ref_evals"])), (e, j)


def test_every_match_keeps_its_trace_under_ulps_of_noise_in_the_newton_system(oracle, c1_world, maps, runs):
    """The other condition on the inputs (optimizer_cases.perturbed_newton): what a permutation cannot show for a scan of one
    point, and what an exp() that rounds the other way does to any scan."""
    for e, scan, init, res, tr, _ in runs:
        for j in range(OC.N_PERTURBATIONS):
            with OC.perturbed_newton(oracle, 100 * j + 7):
                r2, tr2 = maps[e[0]].align(scan, init, trace_cap=512)
            assert OC.traces_agree(tr2, tr), (e, j)
            assert (int(r2["iters"]), int(r2["converged"]), int(r2["ref_evals"])) == \
                   (int(res["iters"]), int(res["converged"]), int(res["ref_evals"])), (e, j)
    r2, tr2 = maps[runs[0][0][0]].align(runs[0][1], runs[0][2], trace_cap=512)          # the hook is gone again
    assert r2.tobytes() == runs[0][3].tobytes()


def test_census_and_ring_change_no_result(oracle, c1_world, maps, runs):
    """... and the ring holds the calls of the line searches: every mt_update row is followed by the mt_trial row of the
    same trial with the interval that mt_update leaves, and every row's trial value is a step length of the trace."""
    n_searched = 0
    for e, scan, init, res, tr, cen in runs:
        oracle.ring_enable(True)
        try:
            r2, tr2 = maps[e[0]].align(scan, init, trace_cap=512)
            ring = oracle.ring_get()
        finally:
            oracle.ring_enable(False)
        assert r2.tobytes() == res.tobytes() and tr2.tobytes() == tr.tobytes() and len(oracle.ring_get()) == 0
        n_trial = sum(v for k, v in cen.items() if k.startswith("mt_c"))
        n_update = cen["mu_u1"] + cen["mu_u2"] + cen["mu_u3"] + cen["mu_converged"]
        assert (int(np.sum(ring[:, 0] == 0)), int(np.sum(ring[:, 0] == 1))) == (n_trial, n_update), e
        assert np.all(np.isin(ring[:, 7], tr[:, 0])), e
        n_searched += n_trial > 0
        n_same = 0
        for a, b in zip(ring[:-1], ring[1:]):
            if b[0] == 1:                                                    # a search: trial, (update, trial)*, update
                assert a[0] == 0, (e, a, b)
            elif a[0] == 1 and np.array_equal(a[7:], b[7:]):                 # the search goes on with the updated interval
                _, interval = oracle.mt_update(*a[1:])
                assert interval == list(b[1:7]), (e, a, b)
                n_same += 1
            else:                                                            # the first inner trial of the next search
                assert np.all(b[1:7] == [0.0, 0.0, b[3], 0.0, 0.0, b[3]]), (e, b)
        assert n_same == n_trial - int(np.sum(np.all(ring[:, [0, 1, 4]] == 0, axis=1))), e
    print('matches with an inner line-search trial:', n_searched)
    assert n_searched >= 30


def test_ring_keeps_the_newest_rows(oracle):
    """The ring holds 8192 rows: after more calls than that it returns the newest 8192, oldest first."""
    row = [0.0, 4.0, -4.0, 5.0, 9.0, 6.0]
    oracle.ring_enable(True)
    try:
        for i in range(8192 + 37):
            oracle.mt_trial(*row, 3.0 + i, 1.0, 2.0)
        ring = oracle.ring_get()
        few = oracle.ring_get(cap=10)
    finally:
        oracle.ring_enable(False)
    assert len(ring) == 8192 and np.array_equal(ring[:, 7], 3.0 + np.arange(37, 8192 + 37))
    assert np.all(ring[:, 0] == 0) and np.all(ring[:, 1:7] == row) and np.all(ring[:, 8:] == [1.0, 2.0])
    assert np.array_equal(few, ring[:10]) and len(oracle.ring_get()) == 0


# ------------------------------------------------------------------------------------------------------------ high precision
class R:
    """A value at 50 digits with a first-order bound of the error its fp64 evaluation (round to nearest, no contraction:
    every + - * / sqrt correctly rounded) can have made: the running error analysis of the formula, operation by operation."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0):
        self.v, self.e = mp.mpf(v), mp.mpf(e)

    @staticmethod
    def _rounded(v, e):
        return R(v, e + U * abs(v))

    def __add__(self, o):
        o = o if isinstance(o, R) else R(o)
        return R._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = o if isinstance(o, R) else R(o)
        return R._rounded(self.v - o.v, self.e + o.e)

    def __neg__(self):
        return R(-self.v, self.e)

    def __mul__(self, o):
        o = o if isinstance(o, R) else R(o)
        return R._rounded(self.v * o.v, abs(self.v) * o.e + abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = o if isinstance(o, R) else R(o)
        if abs(o.v) <= 2 * o.e:
            return R(self.v / o.v if o.v else mp.inf, mp.inf)
        q = self.v / o.v
        return R._rounded(q, (self.e + abs(q) * o.e) / (abs(o.v) - o.e))

    def sqrt(self):
        if self.v - 2 * self.e <= 0:
            return R(mp.sqrt(self.v) if self.v >= 0 else mp.nan, mp.inf)
        return R._rounded(mp.sqrt(self.v), self.e / (2 * mp.sqrt(self.v - self.e)))


def mt_trial_reference(row):
    """-> (case, [candidate R values]) of More-Thuente's trial value on one row, the formulas of ndt_oracle_mt_trial (PCL's
    trialValueSelectionMT) at 50 digits.  The case is decided as the code decides it: by exact
    comparisons of the fp64 inputs (g_t * g_l as the fp64 product).  More than one candidate: a tie within the error bound."""
    a_l, f_l, g_l, a_u, f_u, g_u, a_t, f_t, g_t = (float(v) for v in row)
    A_l, F_l, G_l, A_u, F_u, G_u, A_t, F_t, G_t = (R(v) for v in (a_l, f_l, g_l, a_u, f_u, g_u, a_t, f_t, g_t))

    def cubic(A0, F0, G0):
        z = R(3) * (F_t - F0) / (A_t - A0) - G_t - G0
        w = (z * z - G_t * G0).sqrt()
        return A0 + (A_t - A0) * (w - G0 - z) / (G_t - G0 + R(2) * w)

    if f_t > f_l:
        a_c = cubic(A_l, F_l, G_l)
        a_q = A_l - R(0.5) * (A_l - A_t) * G_l / (G_l - (F_l - F_t) / (A_l - A_t))
        avg = R(0.5) * (a_q + a_c)
        kc, kq = a_c - A_l, a_q - A_l
        if abs(abs(kc.v) - abs(kq.v)) <= kc.e + kq.e:
            return 1, [a_c, avg]
        return 1, [a_c] if abs(kc.v) < abs(kq.v) else [avg]
    if g_t * g_l < 0:
        a_c = cubic(A_l, F_l, G_l)
        a_s = A_l - (A_l - A_t) / (G_l - G_t) * G_l
        kc, ks = a_c - A_t, a_s - A_t
        if abs(abs(kc.v) - abs(ks.v)) <= kc.e + ks.e:
            return 2, [a_c, a_s]
        return 2, [a_c] if abs(kc.v) >= abs(ks.v) else [a_s]
    if abs(g_t) <= abs(g_l):
        a_c = cubic(A_l, F_l, G_l)
        a_s = A_l - (A_l - A_t) / (G_l - G_t) * G_l
        lim = A_t + R(0.66) * (A_u - A_t)
        kc, ks = a_c - A_t, a_s - A_t
        if mp.isnan(a_c.v) or a_c.e == mp.inf or abs(abs(kc.v) - abs(ks.v)) <= kc.e + ks.e:
            ns = [a_c, a_s]
        else:
            ns = [a_c] if abs(kc.v) < abs(ks.v) else [a_s]
        out = []
        for a_n in ns:
            if mp.isnan(a_n.v) or a_n.e == mp.inf or abs(a_n.v - lim.v) <= a_n.e + lim.e:
                out += [a_n, lim]
            elif a_t > a_l:
                out.append(a_n if a_n.v < lim.v else lim)
            else:
                out.append(a_n if lim.v < a_n.v else lim)
        return 3, out
    return 4, [cubic(A_u, F_u, G_u)]


def test_oracle_mt_trial_against_50_digits(oracle, mt_all):
    """ndt_oracle_mt_trial within the running error bound of its own formula (times 2: the bound is first order), per case.
    Rows whose bound is unbounded (a denominator or radicand not separated from 0 by its own error) are counted, not judged:
    there both sides of a comparison are rounding noise, and only agreement of the device WITH the oracle means anything.
    Every row is judged.  The bound is the formula's own conditioning, so it is as wide as the row is ill-conditioned: where
    a radicand or a denominator nearly cancels -- most often on the rows built from independent values -- it admits errors
    of 1e-2 relative (the worst measured: 4e-2), and what this test judges there is the selection logic (which case, which
    candidate, which side of the limit), not the last digits.  The device's last digits are judged against the oracle's,
    bit for bit, in tests/test_gpu_optimizer_branches.py."""
    mp.mp.dps = 50
    rows, groups = mt_all
    worst = {}
    judged = unbounded = both_nan = 0
    sel = np.arange(len(rows))
    for i in sel:
        got = oracle.mt_trial(*rows[i])
        case, cands = mt_trial_reference(rows[i])
        if all(mp.isnan(c.v) for c in cands):
            assert np.isnan(got), (i, rows[i])                      # a negative radicand: NaN on both sides
            both_nan += 1
            continue
        fin = [c for c in cands if not mp.isnan(c.v) and c.e != mp.inf]
        if len(fin) < len(cands) or np.isnan(got):
            unbounded += 1
            continue
        judged += 1
        err, c = min(((abs(mp.mpf(got) - c.v), c) for c in fin), key=lambda t: t[0])
        assert err <= 2 * c.e + mp.mpf(5e-324), (i, case, rows[i], got, c.v, err, c.e)
        scale = max(abs(c.v), abs(rows[i][0]), abs(rows[i][6]))
        rel = float(err / scale) if scale else 0.0
        worst[case] = max(worst.get(case, 0.0), rel)
    print("mt_trial vs 50 digits: judged %d, NaN on both sides %d, unbounded %d, worst error / max(|a|, |a_l|, |a_t|) per case: %s"
          % (judged, both_nan, unbounded, worst))
    assert judged >= 0.6 * len(sel) and both_nan >= 50 and set(worst) == {1, 2, 3, 4}


def _mp_pinv_solve(H, b):
    """Pseudo-inverse solve at 50 digits with JacobiSVD's default threshold (singular values <= 6 eps max dropped).
    -> (x, ratio of the smallest kept to the largest eigenvalue magnitude, closest distance of a ratio to the threshold)"""
    A, Q = mp.matrix(H.tolist()), mp.eye(3)                     # cyclic Jacobi at 50 digits (mp.eigsy gives up at condition 1e18)
    for sweep in range(60):
        off = abs(A[0, 1]) + abs(A[0, 2]) + abs(A[1, 2])
        if off <= mp.mpf(10) ** -60 * (abs(A[0, 0]) + abs(A[1, 1]) + abs(A[2, 2])) or off == 0:
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            if A[p, q] == 0:
                continue
            theta = (A[q, q] - A[p, p]) / (2 * A[p, q])
            t = mp.sign(theta if theta != 0 else 1) / (abs(theta) + mp.sqrt(theta * theta + 1))
            c = 1 / mp.sqrt(t * t + 1)
            G = mp.eye(3)
            G[p, p] = G[q, q] = c; G[p, q] = t * c; G[q, p] = -t * c
            A, Q = G.T * A * G, Q * G
    lam = [A[i, i] for i in range(3)]
    big = max(abs(v) for v in lam)
    x = mp.matrix(3, 1)
    kept, gap = [], mp.inf
    for i in range(3):
        if big == 0:
            continue
        ratio = abs(lam[i]) / big
        gap = min(gap, abs(mp.log(ratio / (6 * EPS))) if ratio > 0 else mp.inf)
        if ratio <= 6 * EPS:
            continue
        kept.append(ratio)
        q = Q[:, i]
        pr = sum(q[j] * mp.mpf(float(b[j])) for j in range(3)) / lam[i]
        x += q * pr
    return np.array([float(x[j]) for j in range(3)]), (float(min(kept)) if kept else 1.0), float(gap)


@pytest.mark.filterwarnings("ignore::RuntimeWarning")          # the rows at 1e+-300 overflow and underflow on purpose
def test_oracle_solve3_against_50_digits_and_jacobisvd(oracle):
    """ndt_oracle_solve3 on the unit rows: the adjugate branch within the running error bound of its own formula against the
    exact solution; the Jacobi branch against the 50-digit pseudo-inverse at the bound test_newton_solve_against_jacobisvd_6x6
    holds it to (max(1e-13, 16 eps / ratio), relative to the solution's norm), rows with an eigenvalue within a factor 4 of
    the threshold left to the Eigen fixture; the svd6 rows against the fixture at that test's bounds.
    A sample, not every row: every row of every group but "random_cond", of which every third row is judged (500 of 1500;
    a row costs a 50-digit eigen-decomposition).  The rows with a NaN or an infinity have no reference and are left to the
    census test and to the device-against-oracle comparison."""
    mp.mp.dps = 50
    rows, groups = OC.solve3_rows()
    z = np.load(OC.GOLD)
    d, sv, n_real = z["svd6_dp3_eig"], z["svd6_sv_eig"], int(z["svd6_n_real"])
    worst = {"svd6_real": 0.0, "svd6_degraded": 0.0, "svd6_rank_deficient": 0.0, "adjugate": 0.0, "jacobi": 0.0}
    for k, r in enumerate(rows[groups["svd6"]]):
        H, b = OC.rows_to_matrix(r)
        mine = oracle.solve3(H, b)
        rel = np.linalg.norm(mine - d[k]) / np.linalg.norm(d[k])
        ratio = sv[k, 2] / sv[k, 0]
        kind = "svd6_real" if k < n_real else "svd6_rank_deficient" if ratio < 6 * EPS else "svd6_degraded"
        bound = 1e-12 if k < n_real else 1e-13 if ratio < 6 * EPS else max(1e-13, 16 * EPS / ratio)
        assert rel < bound, (k, rel, ratio)
        worst[kind] = max(worst[kind], rel)
    n_adj = n_jac = n_edge = 0
    for name in ("random_cond", "exact_rank", "one_pair", "diagonal", "scales"):
        sl = groups[name]
        for i in range(sl.start, sl.stop, 3 if name == "random_cond" else 1):
            H, b = OC.rows_to_matrix(rows[i])
            if not (np.all(np.isfinite(H)) and np.all(np.isfinite(b))):
                continue
            oracle.census_reset()
            mine = oracle.solve3(H, b)
            adj = oracle.census_get()["s3_adjugate"] == 1
            with np.errstate(over="ignore", under="ignore"):
                s = float(np.abs(H).max())
            if s == 0.0:                                        # the zero matrix (every other row is judged after an exact
                assert np.all(mine == 0.0)                      #   rescaling by a power of two: 1e+-300 leaves no headroom)
                continue
            k2 = 2.0 ** -np.floor(np.log2(s))
            Hn, xs = H * k2, None
            if adj:
                # running error of (adj H) b / det H against the exact H^-1 b
                a00, a01, a02, a11, a12, a22 = (R(v) for v in (H[0, 0], H[0, 1], H[0, 2], H[1, 1], H[1, 2], H[2, 2]))
                c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
                c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
                det = a00 * c00 + a01 * c01 + a02 * c02
                b0, b1, b2 = (R(v) for v in b)
                xs = [(c00 * b0 + c01 * b1 + c02 * b2) / det, (c01 * b0 + c11 * b1 + c12 * b2) / det, (c02 * b0 + c12 * b1 + c22 * b2) / det]
                n_adj += 1
                for j in range(3):
                    assert xs[j].e != mp.inf, (name, i)
                    err = abs(mp.mpf(float(mine[j])) - xs[j].v)
                    assert err <= 2 * xs[j].e + mp.mpf(5e-324), (name, i, j, mine, xs[j].v, err, xs[j].e)
                nx = max(abs(x.v) for x in xs)
                if nx:
                    worst["adjugate"] = max(worst["adjugate"], float(max(abs(mp.mpf(float(mine[j])) - xs[j].v) for j in range(3)) / nx))
                continue
            ref, ratio, gap = _mp_pinv_solve(Hn, b)
            ref = ref * k2
            if gap < np.log(4.0) or not np.all(np.isfinite(ref)) or s < 1e-290:
                n_edge += 1                                      # threshold ties / denormal eigenvalues: the fixture and the device-vs-oracle test
                continue
            n_jac += 1
            with np.errstate(over="ignore", under="ignore"):
                nr = np.linalg.norm(ref)
            if nr <= 1e-30 * np.linalg.norm(b) / s:             # the gradient lies in the dropped directions: zero up to rounding
                assert np.linalg.norm(mine) <= 1e-13 * np.linalg.norm(b) / (s * ratio), (name, i, mine)
                continue
            big = np.abs(ref).max()                              # (norms of scaled vectors: 1e199 squared leaves the range)
            rel = np.linalg.norm(mine / big - ref / big) / np.linalg.norm(ref / big)
            assert rel < max(1e-13, 16 * EPS / ratio), (name, i, rel, ratio, mine, ref)
            worst["jacobi"] = max(worst["jacobi"], rel)
    print("solve3 worst relative errors:", worst, "| adjugate rows %d, Jacobi rows %d, near the threshold %d" % (n_adj, n_jac, n_edge))
    assert n_adj >= 100 and n_jac >= 300


def test_oracle_yaw_from_T_against_50_digits(oracle):
    """ndt_oracle_yaw_from_T = the float32 rounding of asin / acos at 50 digits (the a9 model: correctly rounded asinf /
    acosf).  A sample, not every row: every edge row and every sixth of the 1e5 others (the strata are generated in blocks,
    so a stride keeps each of them).  The oracle rounds twice (fp64 libm, then float32): a difference is
    possible only where the 50-digit value lies within 2^-29 relative of a float32 rounding boundary -- counted, at most 1 ulp."""
    mp.mp.dps = 50
    T = OC.yaw_rows()
    sel = np.concatenate([np.arange(0, len(T) - 36, 6), np.arange(len(T) - 36, len(T))])
    n_diff = 0
    for i in sel:
        t00, t10 = float(T[i, 0]), float(T[i, 1])
        got = oracle.yaw_from_T(t00, t10)
        if (t00 > 0 and t10 > 0) or (t00 > 0 and t10 < 0):
            v = mp.asin(mp.mpf(t10))
        elif t00 < 0 and t10 > 0:
            v = mp.acos(mp.mpf(t00))
        else:
            v = -mp.acos(mp.mpf(t00))
        want = float(np.float32(float(v)))                      # float(v): correctly rounded to fp64 by mpmath
        if got != want:
            n_diff += 1
            assert abs(got - float(v)) <= float(np.spacing(np.float32(want))) * (0.5 + 2.0 ** -28), (i, t00, t10, got, want)
    print("yaw_from_T: %d rows judged, %d differ from the 50-digit value's float32 rounding (double rounding)" % (len(sel), n_diff))
    assert n_diff <= 2
