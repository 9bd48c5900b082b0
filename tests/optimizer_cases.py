"""Inputs that take the optimiser (ndt_optimizer.hip.h: solve3, mt_trial, mt_update, begin_outer / advance_step, yaw_from_T)
through the branches whole matches on the synthetic worlds never reach.  Shared by tests/test_optimizer_cases_host.py (the
oracle on these inputs: census, stability, high-precision reference) and tests/test_gpu_optimizer_branches.py (the device
against the oracle on the same inputs).  Everything is generated from fixed seeds; nothing here depends on a GPU.

Two kinds of input:
  unit rows  -- argument tuples for ndt_selftest_optimizer / ndt_oracle_solve3 / _mt_trial / _mt_update / _yaw_from_T;
  the match list -- tiny matches on the C1 map (MATCHES, SPECIAL) whose line searches leave the usual path.
"""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "eigen_golden.npz")
EPS = float(np.finfo(np.float64).eps)

# ------------------------------------------------------------------------------------------------------------ the match list
# Parameter sets (on top of the C1 resolution); the wider ones open branches the launch-file values never reach.
PARAM_SETS = {
    "default": dict(),
    "step1": dict(step_size=1.0),
    "step5": dict(step_size=5.0),
    "eps1e-4": dict(trans_eps=1e-4),
    "conv_ge": dict(conv_ge=1, max_iter=3),
    "stale_h": dict(stale_h_ang=1),
}
# initial error: uniform in +-(metres, degrees); a match's scale is seed % 3
ERR_SCALES = ((0.2, 3.0), (1.0, 15.0), (3.0, 60.0))

# (parameter set, k of ScanFactory.make(k), points of the sub-scan, seed).  Picked with the oracle's census
# (oracle/ndt_oracle.h) from 1..64-point sub-scans of the C1 scans at the three error scales, so that every branch a match
# can reach is taken (MATCH_BRANCHES); frozen.  Every entry keeps its trace, on the oracle, under 8 permutations of the point
# order and under N_PERTURBATIONS perturbations of the Newton system by +-4 ulp (perturbed_newton: a one-point scan has no
# other order, yet a Hessian of condition 1e8 turns the last bit of exp() into 2e-9 m of the next trial pose);
# tests/test_optimizer_cases_host.py checks both on every run.  A match that fails either is no fair comparison of two
# correct implementations and must be replaced here, never left out of the GPU comparison.
MATCHES = [
    ("default", 0, 1, 2), ("default", 0, 3, 4), ("default", 0, 3, 5), ("default", 7, 16, 92),
    ("default", 12, 1, 147), ("default", 12, 3, 150), ("default", 12, 16, 151), ("default", 12, 16, 153),
    ("default", 13, 1, 158), ("default", 19, 3, 234), ("default", 19, 64, 238), ("default", 21, 1, 253),
    ("default", 25, 3, 304), ("default", 25, 16, 308), ("default", 45, 3, 546), ("default", 49, 64, 599),
    ("default", 49, 64, 600), ("default", 50, 16, 608), ("default", 52, 1, 627), ("step1", 8, 3, 821),
    ("step1", 8, 3, 822), ("step1", 14, 3, 893), ("step1", 15, 64, 912), ("step1", 16, 16, 920),
    ("step1", 18, 1, 937), ("step1", 18, 16, 943), ("step1", 21, 1, 974), ("step1", 21, 64, 984),
    ("step1", 23, 64, 1008), ("step1", 25, 16, 1029), ("step1", 25, 64, 1031), ("step1", 28, 1, 1058),
    ("step5", 7, 3, 1170), ("step5", 8, 3, 1181), ("step5", 13, 64, 1246), ("step5", 14, 1, 1249),
    ("step5", 15, 1, 1263), ("step5", 16, 16, 1279), ("step5", 17, 1, 1285), ("step5", 17, 16, 1293),
    ("step5", 21, 3, 1337), ("step5", 22, 64, 1354), ("step5", 26, 64, 1403), ("step5", 28, 16, 1423),
    ("step5", 28, 64, 1427), ("eps1e-4", 1, 64, 1463), ("eps1e-4", 3, 16, 1483), ("eps1e-4", 7, 1, 1525),
    ("eps1e-4", 8, 3, 1542), ("eps1e-4", 10, 3, 1565), ("eps1e-4", 10, 16, 1568), ("eps1e-4", 10, 64, 1572),
    ("eps1e-4", 13, 16, 1604), ("eps1e-4", 15, 1, 1623), ("eps1e-4", 17, 64, 1656), ("eps1e-4", 20, 64, 1690),
    ("eps1e-4", 21, 1, 1694), ("eps1e-4", 21, 3, 1697), ("conv_ge", 0, 16, 1808), ("conv_ge", 0, 64, 1810),
    ("conv_ge", 1, 16, 1819), ("conv_ge", 2, 16, 1831), ("conv_ge", 3, 3, 1840), ("conv_ge", 6, 3, 1877),
    ("conv_ge", 6, 64, 1883), ("conv_ge", 8, 16, 1903), ("conv_ge", 10, 3, 1924), ("conv_ge", 13, 16, 1963),
    ("conv_ge", 14, 1, 1969), ("conv_ge", 15, 1, 1982), ("conv_ge", 16, 64, 2002), ("conv_ge", 21, 64, 2064),
    ("conv_ge", 24, 1, 2091), ("stale_h", 3, 16, 2205), ("stale_h", 3, 64, 2208), ("stale_h", 7, 16, 2251),
    ("stale_h", 11, 64, 2302), ("stale_h", 16, 3, 2358), ("stale_h", 17, 64, 2375), ("stale_h", 18, 1, 2377),
    ("stale_h", 19, 1, 2389), ("stale_h", 20, 1, 2401), ("stale_h", 22, 3, 2428), ("stale_h", 26, 3, 2478),
    ("stale_h", 26, 16, 2481),
]

# Every census name (oracle/ndt_oracle.py) is in exactly one of the three tables below.
#
# Branches the matches (MATCHES and special_matches together) must reach, with the least number of hits.  s3_drop0 and
# s3_drop1 are reached by all-zero Hessians only (scans that miss the map); the one non-zero matrix with a dropped
# eigenvalue that a match solves is the origin copies' (MATCH_NONZERO_DROP2).
MATCH_BRANCHES = {
    "s3_adjugate": 3, "s3_jacobi": 3, "s3_jacobi_nonzero": 3, "s3_rot01": 3, "s3_rot02": 3, "s3_rot12": 3,
    "s3_skip02": 3, "s3_skip12": 3, "s3_drop0": 3, "s3_drop1": 3, "s3_drop2": 3,
    "mt_c1_cubic": 3, "mt_c1_average": 3, "mt_c2_cubic": 1, "mt_c2_secant": 3, "mt_c3_secant_bwd_lim": 3,
    "mu_u1": 3, "mu_u2": 3, "mu_u3": 3, "mu_converged": 3,
    "ls_flip": 3, "ls_open_closes": 3, "ls_trial_closed": 3, "ls_clamp_min": 3, "ls_repeat": 3,
    "exit_nrm_zero": 3, "exit_max_iter": 3, "exit_trans_eps": 3,
}
# least number of s3_drop2 hits inside a NON-zero matrix (nonzero_drops), all of them the origin copies'
MATCH_NONZERO_DROP2 = 3
# Branches of solve3, mt_trial and mt_update that NO match reaches (nor any of the 2 520 candidates the list was picked
# from): the unit rows below cover them, and only they.
UNIT_ROWS_ONLY = (
    "s3_nan", "s3_skip01",
    "mt_c3_secant_bwd_an", "mt_c3_secant_fwd_an", "mt_c3_secant_fwd_lim", "mt_c3_cubic_bwd_an", "mt_c3_cubic_bwd_lim",
    "mt_c3_cubic_fwd_an", "mt_c3_cubic_fwd_lim", "mt_c4", "mt_nan",
)
# Branches of the state machine (begin_outer / advance_step) that NOTHING in the suite reaches, on either side: no match
# takes them, and the state machine has no entry point of its own for a unit row (tests).
#   ls_clamp_max   an inner trial above step_size.  A search starts from the interval [0, 0] and its first trial is at most
#                  step_size; a_u is only ever set to an earlier trial, and each case of mt_trial interpolates between a_l
#                  and a_t or steps from a_t towards a_u.  5 880 matches searched with the census (step_size 0.002 .. 5)
#                  gave no hit.
#   ls_dphi0_zero  a Newton direction exactly orthogonal to the gradient.
#   exit_nrm_nan   a NaN Newton step: needs a non-finite Hessian, which no input produces through the API.
NEVER_REACHED = ("ls_clamp_max", "ls_dphi0_zero", "exit_nrm_nan")
MATCH_UNREACHED = UNIT_ROWS_ONLY + NEVER_REACHED


def nonzero_drops(census):
    """Hits of s3_drop0 / 1 / 2 inside non-zero matrices: the zero matrix (s3_jacobi - s3_jacobi_nonzero calls) drops all three."""
    zero = census["s3_jacobi"] - census["s3_jacobi_nonzero"]
    return [census["s3_drop%d" % k] - zero for k in range(3)]


def match_inputs(c1_world, entry):
    """-> (scan float32 [n, 2], init [3]) of one MATCHES entry."""
    _, sf, _ = c1_world
    pset, k, n, seed = entry
    scan, truth, _ = sf.make(k)
    rng = np.random.default_rng(seed)
    sel = np.sort(rng.choice(len(scan), size=n, replace=False))
    m, deg = ERR_SCALES[seed % 3]
    init = truth + np.array([rng.uniform(-m, m), rng.uniform(-m, m), math.radians(rng.uniform(-deg, deg))])
    return np.ascontiguousarray(scan[sel]), init


def special_matches(c1_world):
    """-> [(name, parameter set, scan, init)]: the scans no sub-scan family contains."""
    m, sf, cfg = c1_world
    out = []
    # copies of the sensor origin placed near a wall: x' = t for every point, so the yaw column of the Jacobian is exactly
    # zero -- a Hessian with a zero yaw row (rank 2) and a non-zero gradient
    for k, d in ((0, (0.07, -0.05)), (3, (-0.04, 0.09)), (7, (0.11, 0.02))):
        scan, truth, _ = sf.make(k)
        c, s = math.cos(truth[2]), math.sin(truth[2])
        wall = truth[:2] + np.array([c * scan[0, 0] - s * scan[0, 1], s * scan[0, 0] + c * scan[0, 1]])   # a map point, roughly
        out.append(("origin_copies_%d" % k, "default", np.zeros((5, 2), np.float32), np.array([wall[0] + d[0], wall[1] + d[1], truth[2]])))
    scan, truth, init = sf.make(2)
    out.append(("all_nan", "default", np.full((7, 2), np.nan, np.float32), init))
    out.append(("one_nan_point", "default", np.array([[np.nan, 1.0]], np.float32), init))
    out.append(("misses_the_map", "default", scan[:16], np.array([init[0] + 500.0, init[1] - 300.0, init[2]])))
    out.append(("misses_the_map_1pt", "step1", scan[:1], np.array([init[0] - 900.0, init[1], init[2]])))
    # a guess that is not finite: the transform is NaN from the start (include/ndt_mi355x.h, ndt_align's contract)
    out.append(("nan_yaw_guess", "default", scan[:16], np.array([init[0], init[1], np.nan])))
    out.append(("nan_xy_guess", "default", scan[:16], np.array([np.nan, init[1], init[2]])))
    return out


SPECIAL_DEGENERATE = ("all_nan", "one_nan_point", "misses_the_map", "misses_the_map_1pt", "nan_yaw_guess", "nan_xy_guess")


def permuted(scan, j):
    """The j-th fixed permutation of a scan's point order (j = 0: as it is)."""
    return scan if j == 0 else np.ascontiguousarray(scan[np.random.default_rng(1000 + j).permutation(len(scan))])


class perturbed_newton:
    """Context: the oracle's Newton step solves (H, -g) with every entry moved by -ulps .. +ulps units in the last place
    (symmetric H kept symmetric), drawn from `seed`.  Two correct implementations of a pass differ by that much in its
    totals: another order of summation, an exp() that rounds the other way (1 ulp each for glibc's and the device
    library's, and the entries of g and H are sums of terms of both signs, which doubles it: 4 -- argued, not measured;
    LOG.md R20.1 has what was measured).  A match whose trace does not survive this is decided by roundings in its pass
    totals."""

    def __init__(self, oracle, seed, ulps=4):
        rng = np.random.default_rng(seed)

        def solve(H, b, x):
            Hn = np.array([H[i] for i in range(9)]).reshape(3, 3)
            bn = np.array([b[i] for i in range(3)])
            k = np.triu(rng.integers(-ulps, ulps + 1, (3, 3)))
            Hn = Hn * (1.0 + (k + np.triu(k, 1).T) * EPS)
            bn = bn * (1.0 + rng.integers(-ulps, ulps + 1, 3) * EPS)
            r = oracle.solve3(Hn, bn)
            for i in range(3):
                x[i] = r[i]

        self.oracle = oracle
        self.hooks = oracle.Hooks(oracle.SOLVE_FN(solve), oracle.INITP_FN())

    def __enter__(self):
        self.oracle.set_hooks(self.hooks)
        return self

    def __exit__(self, *exc):
        self.oracle.set_hooks(None)
        return False


N_PERTURBATIONS = 6


def traces_agree(tr, ref):
    """The trace tolerances of test_c1_matches_oracle_with_same_step_sequence, plus the trial poses (abs 1e-9)."""
    if len(tr) != len(ref):
        return False
    a, b = tr[:, 0], ref[:, 0]
    if not np.all(np.abs(a - b) <= 1e-12 + 1e-8 * np.abs(b)):
        return False
    s, r = tr[:, 1], ref[:, 1]
    nz = r != 0
    if not (np.all(np.abs(s[nz] - r[nz]) <= 1e-10 * np.abs(r[nz])) and np.all(s[~nz] == 0)):
        return False
    return bool(np.all(np.abs(tr[:, 5:8] - ref[:, 5:8]) <= 1e-9))


# ------------------------------------------------------------------------------------------------------------ solve3 rows
def _sym_rows(H, b):
    H = np.asarray(H, float).reshape(-1, 3, 3)
    b = np.asarray(b, float).reshape(-1, 3)
    return np.concatenate([H[:, 0, 0:1], H[:, 0, 1:2], H[:, 0, 2:3], H[:, 1, 1:2], H[:, 1, 2:3], H[:, 2, 2:3], b], axis=1)


def rows_to_matrix(row):
    """One solve3 row -> (H [3, 3], b [3])."""
    h = row[:6]
    return np.array([[h[0], h[1], h[2]], [h[1], h[3], h[4]], [h[2], h[4], h[5]]]), np.array(row[6:9])


def solve3_rows():
    """-> (rows [n, 9] = Hxx Hxy Hxt Hyy Hyt Htt b0 b1 b2, {group name: slice})."""
    rng = np.random.default_rng(31)
    parts, groups, at = [], {}, 0

    def add(name, H, b):
        nonlocal at
        r = _sym_rows(H, b)
        parts.append(r); groups[name] = slice(at, at + len(r)); at += len(r)

    z = np.load(GOLD)
    add("svd6", z["svd6_H_in"], -z["svd6_g_in"])                  # the Newton step's own call: solve3(H, -g)
    # random symmetric matrices, condition 1 .. 1e18, signs of the eigenvalues mixed
    n = 1500
    Q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    lam = np.stack([np.ones(n), 10.0 ** (-rng.uniform(0, 9, n)), 10.0 ** (-rng.uniform(0, 18, n))], axis=1)
    lam *= rng.choice([-1.0, 1.0], size=(n, 3)) * (10.0 ** rng.uniform(-3, 6, n))[:, None]
    H = np.einsum("nij,nj,nkj->nik", Q, lam, Q)
    add("random_cond", 0.5 * (H + H.transpose(0, 2, 1)), rng.normal(size=(n, 3)))
    # exact rank 2 / rank 1 from small integers (every product and sum below is exact, so det == 0 exactly)
    Hs, bs = [], []
    vecs = [np.array(v, float) for v in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, -1, 0), (1, 0, -2),
                                        (0, 3, 1), (1, 2, 3), (2, -1, 1), (-3, 1, 2), (1, 1, 1), (4, -2, 1))]
    for i, u in enumerate(vecs):
        for s in (1.0, 0.25, 3.0, 4096.0):
            Hs.append(s * np.outer(u, u)); bs.append(rng.integers(-4, 5, 3).astype(float))               # rank 1
            for v in vecs[i + 1:]:
                Hs.append(s * np.outer(u, u) + np.outer(v, v)); bs.append(rng.integers(-4, 5, 3).astype(float))   # rank 2 (or 1)
    add("exact_rank", Hs, bs)
    # the degenerate direction placed so that one rotation pair is taken (apq != 0) and the other two are skipped, per pair;
    # then two pairs taken; each with the gradient inside and across the null space
    Hs, bs = [], []
    for p, q in ((0, 1), (0, 2), (1, 2)):
        r = 3 - p - q
        for lr in (0.0, 2.0, -0.5, 1e-20):
            for off in (1.0, -1.0, 0.5):
                Hm = np.zeros((3, 3)); Hm[p, p] = Hm[q, q] = abs(off); Hm[p, q] = Hm[q, p] = off; Hm[r, r] = lr
                for b in ((1.0, 2.0, 3.0), (0.0, 0.0, 1.0), (1.0, -1.0, 0.0)):
                    Hs.append(Hm); bs.append(b)
    add("one_pair", Hs, bs)
    # diagonal matrices (regular: adjugate; singular: Jacobi without a rotation) and the zero matrix
    Hs, bs = [], []
    for d in ((1, 2, 3), (1, 2, 0), (1, 0, 3), (0, 2, 3), (5, 0, 0), (0, 5, 0), (0, 0, 5), (0, 0, 0), (-1, 2, 0), (1e-12, 1, 1), (1, 1e-17, 1), (1, 1, 1e-30)):
        for b in ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (-2.0, 0.5, 7.0)):
            Hs.append(np.diag(np.array(d, float))); bs.append(b)
    add("diagonal", Hs, bs)
    # a NaN in each of the six entries (and an infinity: det is NaN / inf, not the NaN guard)
    Hs, bs = [], []
    base = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, 0.25], [0.5, 0.25, 2.0]])
    for i in range(3):
        for j in range(i, 3):
            for bad in (np.nan, np.inf):
                Hm = base.copy(); Hm[i, j] = Hm[j, i] = bad
                Hs.append(Hm); bs.append((1.0, 2.0, 3.0))
    add("nan_entry", Hs, bs)
    # overall scales 1e-300 .. 1e300 (det overflows / underflows: the DBL_MAX and DBL_MIN guards), regular and rank 2
    Hs, bs = [], []
    sing = np.outer([1.0, 2.0, 0.0], [1.0, 2.0, 0.0]) + np.outer([0.0, 1.0, 1.0], [0.0, 1.0, 1.0])
    for e in (-320, -310, -305, -300, -200, -110, -100, -50, 0, 50, 100, 103, 110, 200, 300, 305):
        for Hm in (base, sing, np.diag([1.0, 2.0, 0.0])):
            for be in (0, e):
                with np.errstate(over="ignore", under="ignore"):
                    Hs.append(Hm * float("1e%d" % e) if e > -308 else Hm * 1e-300 * float("1e%d" % (e + 300)))
                    bs.append(np.array([1.0, -2.0, 0.5]) * (float("1e%d" % be) if be > -308 else 1e-300))
    add("scales", Hs, bs)
    return np.concatenate(parts), groups


# ------------------------------------------------------------------------------------------------------------ More-Thuente rows
def _poly_rows(rng, n, degree):
    """Rows from polynomials f of the given degree: (a_l, a_u, a_t) in both directions, f and f' exact in shape, so the
    cubic step of a cubic (the quadratic step of a quadratic) is the polynomial's own stationary point."""
    c = rng.normal(size=(n, 4)) * np.array([1.0, 1.0, 0.5, 0.2])
    if degree == 2:
        c[:, 3] = 0.0
    f = lambda a: c[:, 0] + c[:, 1] * a + c[:, 2] * a * a + c[:, 3] * a * a * a          # noqa: E731
    g = lambda a: c[:, 1] + 2 * c[:, 2] * a + 3 * c[:, 3] * a * a                        # noqa: E731
    a_l = rng.uniform(0, 2, n) * (rng.random(n) < 0.7)
    a_t = a_l + rng.uniform(0.01, 3, n) * rng.choice([-1.0, 1.0], n, p=[0.35, 0.65])
    near = rng.random(n) < 0.4                                  # a_u close behind a_t: the 0.66 safeguard binds
    a_u = np.where(near, a_t + (a_t - a_l) * rng.uniform(0.01, 0.5, n), a_t + (a_t - a_l) * rng.uniform(0.5, 4, n))
    a_u = np.where(rng.random(n) < 0.2, a_l + (a_t - a_l) * rng.uniform(0.0, 0.9, n), a_u)
    return np.stack([a_l, f(a_l), g(a_l), a_u, f(a_u), g(a_u), a_t, f(a_t), g(a_t)], axis=1)


def mt_rows(harvested=None):
    """-> (rows [n, 9] = a_l f_l g_l a_u f_u g_u a_t f_t g_t, {group: slice}); used for mt_trial AND mt_update.
    harvested: rows recorded from the oracle's own line searches on the match list (harvest_mt_rows)."""
    rng = np.random.default_rng(77)
    parts, groups, at = [], {}, 0

    def add(name, r):
        nonlocal at
        r = np.asarray(r, float).reshape(-1, 9)
        parts.append(r); groups[name] = slice(at, at + len(r)); at += len(r)

    if harvested is not None and len(harvested):
        add("harvested", harvested)
    add("quadratics", _poly_rows(rng, 1200, 2))
    add("cubics", _poly_rows(rng, 2400, 3))
    # the known-answer rows of tests/test_oracle_units.py: f = (a - 2)^2 and f = a^3 - 3 a
    f, g = (lambda a: (a - 2.0) ** 2), (lambda a: 2.0 * (a - 2.0))
    f3, g3 = (lambda a: a ** 3 - 3.0 * a), (lambda a: 3.0 * a * a - 3.0)
    add("known_answers", [
        (0.0, f(0), g(0), 0.0, f(0), g(0), 5.0, f(5.0), g(5.0)), (0.0, f(0), g(0), 5.0, f(5), g(5), 3.0, f(3.0), g(3.0)),
        (0.0, f(0), g(0), 5.0, f(5), g(5), 1.0, f(1.0), g(1.0)), (0.0, f(0), g(0), 1.5, f(1.5), g(1.5), 1.0, f(1.0), g(1.0)),
        (0.0, f3(0), g3(0), 0.0, f3(0), g3(0), 3.0, f3(3.0), g3(3.0)), (0.0, f3(0), g3(0), 3.0, f3(3), g3(3), 0.5, f3(0.5), g3(0.5))])
    # values that belong to no polynomial: independent f and g -- among them negative radicands (NaN on both sides),
    # case 4 (|g_t| > |g_l|, same sign, f_t <= f_l) and every tie of mt_update (g_t == 0, a_t == a_l)
    n = 1500
    r = rng.normal(size=(n, 9))
    r[:, 0] = np.abs(r[:, 0]) * (rng.random(n) < 0.5); r[:, 6] = np.abs(r[:, 6]) + 0.01; r[:, 3] = r[:, 6] + np.abs(r[:, 3])
    same = rng.random(n) < 0.6
    r[same, 8] = np.abs(r[same, 8]) * np.sign(r[same, 2])
    low = rng.random(n) < 0.6
    r[low, 7] = r[low, 1] - np.abs(r[low, 7])
    add("independent", r)
    t = _poly_rows(rng, 60, 3)
    t[:20, 8] = 0.0; t[20:30, 8] = -0.0; t[30:45, 6] = t[30:45, 0]; t[45:, 7] = t[45:, 1]
    add("ties", t)
    return np.concatenate(parts), groups


def harvest_mt_rows(oracle, c1_world, maps):
    """Run the match list through the oracle with the ring enabled -> the distinct (a_l .. g_t) tuples of every
    ndt_oracle_mt_trial / ndt_oracle_mt_update call of its line searches.  maps: {parameter set: oracle.Map}."""
    oracle.ring_enable(True)
    rows = []
    try:
        for e in MATCHES:
            scan, init = match_inputs(c1_world, e)
            maps[e[0]].align(scan, init)
            rows.append(oracle.ring_get()[:, 1:])
            oracle.ring_enable(True)
    finally:
        oracle.ring_enable(False)
    rows = np.concatenate(rows) if rows else np.zeros((0, 9))
    return np.unique(rows, axis=0)


# ------------------------------------------------------------------------------------------------------------ yaw_from_T rows
def yaw_rows():
    """-> [n, 2] float32 (T00, T10): the float32 cos / sin of about 1e5 yaws, and the sign quadrants with a zero entry."""
    rng = np.random.default_rng(9)
    yaws = np.concatenate([
        rng.uniform(-math.pi, math.pi, 60_000),
        np.round(rng.uniform(-2, 2, 30_000)) * (math.pi / 2) + rng.uniform(-0.01, 0.01, 30_000),
        np.round(rng.uniform(-2, 2, 4_000)) * (math.pi / 2) + rng.uniform(-1e-6, 1e-6, 4_000),
        rng.uniform(-1e-3, 1e-3, 4_000), rng.uniform(-1e-7, 1e-7, 2_000),
        np.array([0.0, -0.0, math.pi, -math.pi, math.pi / 2, -math.pi / 2, math.pi / 4])]).astype(np.float32)
    T = np.stack([np.cos(yaws), np.sin(yaws)], axis=1).astype(np.float32)
    edge = np.array([(a, b) for a in (1.0, -1.0, 0.0, -0.0, 0.5, -0.5) for b in (1.0, -1.0, 0.0, -0.0, 0.5, -0.5)], np.float32)
    return np.concatenate([T, edge])


def bits(a):
    """float64 array -> its bit patterns with every NaN folded to one value (NaN for NaN)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    u = a.view(np.uint64).copy()
    u[np.isnan(a)] = np.uint64(0x7FF8000000000000)
    return u


def ulp_distance(a, b):
    """Distance in units in the last place between two float64 arrays (NaN vs NaN: 0; NaN vs number: 2^63)."""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float64).view(np.int64).astype(object)
        return np.array([v if v >= 0 else -(v & 0x7FFFFFFFFFFFFFFF) for v in i.ravel()], dtype=object).reshape(np.shape(x))
    a, b = np.asarray(a, float), np.asarray(b, float)
    d = np.abs(key(a) - key(b))
    na, nb = np.isnan(a), np.isnan(b)
    d[na & nb] = 0
    d[na ^ nb] = 1 << 63
    return d
