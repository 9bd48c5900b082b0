"""Oracle and workloads of the robust pose-graph tests (ndt_pg_optimize_robust_batch; tests only).

oracle_optimize_robust   the header's graduated non-convexity restated densely on pg_helpers' model: Geman-McClure arcs
                         rho = sigma c / (sigma + c), sigma = mu phi, the weighted normal equations solved by
                         numpy.linalg.solve, the halving step rule on F_mu, the level schedule, every decision's margin.
drifted                  a figure-eight whose odometry has drifted by metres, true loop arcs, optionally gross false ones.
robust_workload          the named cases the CPU and GPU tests share, made once per process.
"""
import functools
import math

import numpy as np

import pg_helpers as H

MU_MAX = 1e12
PHI = 9.0                                              # about the 97 % quantile of chi-square with 3 degrees of freedom
FALSE_OFFSET = (6.0, -4.0, 90.0)
MARGIN_MIN = 1e-3                                      # every decision of a workload whose counts the GPU tests compare ...
# ... and every trial's |Ft - F| / F: a thousand times the 1e-15 to which a sum of a few hundred arcs is evaluated.  (A trial's
# RELATIVE margin is taken against the change its own step predicts, not against F: a Gauss-Newton step of length d moves F
# by about d^T H d, so next to a level's minimiser |Ft - F| / F falls like the square of the step whatever the workload.)
TRIAL_F_MIN = 1e-12


def arc_chi2(x, edges):
    r = H.residuals(x, edges)
    return np.einsum("ea,eab,eb->e", r, H.omegas(edges), r)


def arc_weights(c, phi, mu):
    """w_e = (sigma / (sigma + c))^2 with sigma = mu phi for the robust arcs (phi > 0), 1 for the plain ones."""
    w = np.ones(len(c))
    rb = phi > 0
    t = (mu * phi[rb]) / (mu * phi[rb] + c[rb])
    w[rb] = t * t
    return w


def cost_mu(x, edges, phi, mu):
    """F_mu = sum rho_mu(c_e): c for a plain arc, sigma c / (sigma + c) for a robust one."""
    c = arc_chi2(x, edges)
    rho = c.copy()
    rb = phi > 0
    sig = mu * phi[rb]
    rho[rb] = sig * c[rb] / (sig + c[rb])
    return float(rho.sum())


def weighted_normal_equations(x, edges, w):
    """pg_helpers.normal_equations with every arc's blocks and gradient scaled by w_e."""
    e = edges.copy()
    e["info"] = edges["info"] * w[:, None]
    return H.normal_equations(x, e)


def auto_mu0(x, edges, phi):
    rb = phi > 0
    if not rb.any():
        return 1.0
    return float(min(MU_MAX, max(1.0, 2.0 * float((arc_chi2(x, edges)[rb] / phi[rb]).max()))))


def oracle_optimize_robust(poses, edges, phi, mu0=0.0, factor=1.4, eps_level=1e-3, level_iter=3, eps_step=1e-9, max_iter=200,
                           max_halvings=8):
    """The header's method with a dense solve in place of the conjugate gradients.
    -> dict: poses (deg, wrapped; the last accepted ones), weights and chi2 (at mu = 1 at those poses), mu0, levels, iterations
    (accepted steps), trips, converged, cost_initial / cost_final (F_1), iterates (deg, wrapped: the poses behind every TRIP,
    accepted or not), accepted (bool per trip), mus (the level every trip ran at), steps (max|s d| of every trip), rejected
    (bool per arc),
    margins: {"level": [...], "trial": [...], "trial_f": [...], "reject": [...], "step": [...]} -- the relative distance of every
    decision from a tie: |max|s d| - eps_level| / eps_level where a level with mu > 1 looked at it; for every trial
    |Ft - F| / ((2 s - s^2) d^T H d), the change of F_mu as a part of what the weighted quadratic model predicts for the step
    s d (the trial is accepted or not by the sign of that change), and under trial_f the same change as a part of F;
    |c - phi| / phi of every robust arc at the end; |max|s d| - eps_step| / eps_step at mu = 1."""
    def out_deg(x):
        out = x.copy()
        out[:, 2] = H.wrap_deg(out[:, 2] / H.DEG)
        out[0] = poses[0]
        return out

    phi = np.asarray(phi, np.float64)
    x = np.array(poses, np.float64)
    x[:, 2] *= H.DEG
    rb = phi > 0
    mu_start = (auto_mu0(x, edges, phi) if mu0 == 0 else float(mu0)) if rb.any() else 1.0
    mu, levels, in_level, iters, conv = mu_start, 1, 0, 0, False
    cost_initial = cost_mu(x, edges, phi, 1.0)
    F = cost_mu(x, edges, phi, mu)
    iterates, mus, steps, accepts = [], [], [], []
    margins = {"level": [], "trial": [], "trial_f": [], "reject": [], "step": []}
    trips = 0
    for _ in range(max_iter):
        trips += 1
        w = arc_weights(arc_chi2(x, edges), phi, mu)
        Hm, b = weighted_normal_equations(x, edges, w)
        d = np.linalg.solve(Hm[3:, 3:], -b[3:]).reshape(-1, 3)
        dHd = float(d.reshape(-1) @ Hm[3:, 3:] @ d.reshape(-1))
        s, accepted = 1.0, False
        for h in range(max_halvings + 1):
            if h:
                s *= 0.5
            xt = x.copy()
            xt[1:] += s * d
            Ft = cost_mu(xt, edges, phi, mu)
            if math.isfinite(Ft):
                margins["trial"].append(abs(Ft - F) / ((2.0 * s - s * s) * dHd) if dHd > 0 else math.inf)
                margins["trial_f"].append(abs(Ft - F) / F if F > 0 else math.inf)
            if math.isfinite(Ft) and Ft <= F:
                accepted = True
                break
        dmax = s * float(np.abs(d).max())
        mus.append(mu)
        steps.append(dmax)
        end_level = False
        if accepted:
            x, F = xt, Ft
            iters += 1
            in_level += 1
        iterates.append(out_deg(x))
        accepts.append(accepted)
        if mu > 1.0:
            if not accepted:
                end_level = True
            else:
                margins["level"].append(abs(dmax - eps_level) / eps_level if eps_level > 0 else math.inf)
                end_level = dmax < eps_level or in_level >= level_iter
            if end_level:
                mu = max(1.0, mu / factor)
                levels += 1
                in_level = 0
                F = cost_mu(x, edges, phi, mu)
            continue
        margins["step"].append(abs(dmax - eps_step) / eps_step if eps_step > 0 else math.inf)
        if not accepted:
            conv = dmax < eps_step
            break
        if dmax < eps_step:
            conv = True
            break
    c = arc_chi2(x, edges)
    margins["reject"] = list(np.abs(c[rb] - phi[rb]) / phi[rb])
    return {"poses": out_deg(x), "weights": arc_weights(c, phi, 1.0), "chi2": c, "mu0": mu_start, "levels": levels,
            "iterations": iters, "trips": trips, "converged": bool(conv), "cost_initial": cost_initial,
            "cost_final": cost_mu(x, edges, phi, 1.0), "iterates": iterates, "mus": mus, "steps": steps, "accepted": accepts,
            "rejected": rb & (c > phi), "margins": margins}


def smallest_margin(ref, kinds=("level", "trial", "reject", "step")):
    return min([math.inf] + [float(v) for k in kinds for v in ref["margins"][k]])


# ---- workloads ----

def loop_sets(N):
    return ([(N - 1, 0)], [(N - 1, 0), (N - 2, 1)], [(N - 1, 0), (N - 2, 1), (N // 2, 0)])


def false_arc(N):
    return (N // 3, 2 * N // 3, FALSE_OFFSET)


def drifted(N, seed, scale, loops, false_arcs=(), phi=PHI):
    """-> (start poses [N, 3], edges, phi per arc, is_false per arc).  The chain is pg_helpers' figure-eight with odometry noise
    scale * (0.05 m, 0.05 m, 1/30 rad) per arc at OMEGA_ODO, the start its composition from the first pose; true loop arcs
    between the pairs `loops` at OMEGA_LOOP with noise (0.002, 0.002, 0.001); false arcs (a, b, offset): the true relation of
    (a, b) composed with offset (m, m, deg), at OMEGA_LOOP.  Odometry arcs are plain (phi 0), loop arcs robust."""
    rng = np.random.default_rng(seed)
    truth = H.eight_truth(N)
    sig = scale * np.array([0.05, 0.05, 1.0 / 30.0])
    rows, start = [], [truth[0].copy()]
    for k in range(N - 1):
        rel = H._noisy(H.between(truth[k], truth[k + 1]), rng, sig)
        rows.append((k, k + 1, rel, H.OMEGA_ODO))
        start.append(H.compose(start[-1], rel))
    for a, b in loops:
        rows.append((a, b, H._noisy(H.between(truth[a], truth[b]), rng, (0.002, 0.002, 0.001)), H.OMEGA_LOOP))
    for a, b, off in false_arcs:
        rows.append((a, b, H.compose(H.between(truth[a], truth[b]), np.asarray(off, np.float64)), H.OMEGA_LOOP))
    n_loop = len(loops) + len(false_arcs)
    ph = np.concatenate([np.zeros(N - 1), np.full(n_loop, float(phi))])
    bad = np.concatenate([np.zeros(N - 1 + len(loops), bool), np.ones(len(false_arcs), bool)])
    return np.array(start), H.make_edges(rows), ph, bad


def padded(N, seed, E):
    """drifted(N, seed, 0.3, two true loops and the false one) with plain duplicates of the chain's arcs behind it up to E arcs."""
    poses, edges, phi, bad = drifted(N, seed, 0.3, loop_sets(N)[1], [false_arc(N)])
    k = E - len(edges)
    extra = edges[np.arange(k) % (N - 1)].copy()
    return poses, np.concatenate([edges, extra]), np.concatenate([phi, np.zeros(k)]), np.concatenate([bad, np.zeros(k, bool)])


def two_nodes():
    """One robust arc between two nodes, the start 0.4 m and 10 degrees off."""
    edges = H.make_edges([(0, 1, np.array([1.0, 0.2, 5.0]), H.OMEGA_LOOP)])
    return np.array([[0.0, 0.0, 0.0], [1.3, 0.5, 15.0]]), edges, np.array([PHI]), np.zeros(1, bool)


def four_nodes():
    """A square of four nodes: three odometry arcs, the true closing arc (3, 0) and a false arc (2, 0)."""
    truth = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 90.0], [2.0, 2.0, 180.0], [0.0, 2.0, -90.0]])
    rng = np.random.default_rng(4)
    rows, start = [], [truth[0].copy()]
    for k in range(3):
        rel = H._noisy(H.between(truth[k], truth[k + 1]), rng, (0.05, 0.05, 1.0 / 30.0))
        rows.append((k, k + 1, rel, H.OMEGA_ODO))
        start.append(H.compose(start[-1], rel))
    rows.append((3, 0, H._noisy(H.between(truth[3], truth[0]), rng, (0.002, 0.002, 0.001)), H.OMEGA_LOOP))
    rows.append((2, 0, H.compose(H.between(truth[2], truth[0]), np.array([1.5, -1.0, 40.0])), H.OMEGA_LOOP))
    return np.array(start), H.make_edges(rows), np.array([0.0, 0.0, 0.0, PHI, PHI]), np.array([0, 0, 0, 0, 1], bool)


# name -> (maker, its arguments): the cases whose counts the GPU tests hold to the oracle.  Seeds are chosen so that every
# decision of the oracle's run has a margin of MARGIN_MIN and more (tests/test_pg_robust_host.py asserts it).
def _case(N, seed, scale, k, with_false=True):
    return (drifted, (N, seed, scale, tuple(loop_sets(N)[k]), (false_arc(N),) if with_false else ()))


ROBUST_WORKLOADS = {
    "two": (two_nodes, ()), "four": (four_nodes, ()),
    "d24a": _case(24, 1, 1.0, 0), "d24b": _case(24, 2, 1.0, 2), "d24c": _case(24, 2, 0.3, 1), "d24t": _case(24, 3, 1.0, 1, False),
    "d65a": _case(65, 1, 1.0, 1), "d65b": _case(65, 2, 0.3, 2), "d257": _case(257, 1, 0.3, 2),
    "p127": (padded, (24, 1, 127)), "p128": (padded, (24, 1, 128)), "p129": (padded, (24, 1, 129)),
}
# the parameters the GPU comparisons run with: the defaults but for eps_step.  At mu = 1 the steps fall from about 1e-5 to 1e-7
# and on to 1e-9, and a trial of a step of 1e-7 changes F by 1e-14 of itself: whether it is accepted is rounding, and the
# count of accepted steps with it.  1e-4 ends every run at its first or second step at mu = 1, whose trial is decided by
# TRIAL_F_MIN and more; the device and the oracle then stand at the same iterate, not yet at the minimiser both approach.
CMP_EPS_STEP = 1e-4


def classification_cases():
    """The issue's starting set at scale 1.0: (N, seed, loops, with_false)."""
    return [(N, seed, tuple(loops), wf) for N in (24, 65) for loops in loop_sets(N) for seed in (2, 5) for wf in (False, True)]


@functools.lru_cache(maxsize=None)
def robust_workload(name, **kw):
    """(start poses, edges, phi, is_false, the oracle's run with CMP_EPS_STEP and otherwise the defaults or **kw) of
    ROBUST_WORKLOADS[name], made once per process; read-only."""
    fn, args = ROBUST_WORKLOADS[name]
    poses, edges, phi, bad = fn(*args)
    prm = dict(eps_step=CMP_EPS_STEP)
    prm.update(kw)
    ref = oracle_optimize_robust(poses, edges, phi, **prm)
    for a in (poses, edges, phi, bad):
        a.setflags(write=False)
    return poses, edges, phi, bad, ref


def pack_robust(graphs):
    """[(poses, edges, phi)] -> (poses, node_offsets, edges, edge_offsets, phi) of one batched call."""
    poses, no, edges, eo = H.pack([(p, e) for p, e, _ in graphs])
    phi = np.concatenate([np.asarray(f, np.float64) for _, _, f in graphs]) if int(eo[-1]) else np.zeros(0)
    return poses, no, edges, eo, np.ascontiguousarray(phi)
