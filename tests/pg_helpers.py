"""Oracle and workloads of the pose-graph tests (ndt_pg_*, ndt_repose_points; tests only).

oracle_optimize   a dense numpy restatement of the header's model: the same residuals and analytic Jacobians, the normal
                  equations solved by numpy.linalg.solve, full Gauss-Newton steps, no halving.
oracle_optimize_halving
                  the header's whole method, step rule included: "a step d is taken only if F does not rise; otherwise it is
                  halved, up to max_halvings times", every accepted iterate kept, and how the run ended.
figure_eight ...  the graph generators; far_start: a figure-eight's arcs from a start metres and tens of degrees away.
repose_ref        the numpy restatement of ndt_repose_points (fp64, one operation per rounding, then float32).
"""
import functools
import math

import numpy as np

PG_EDGE_DTYPE = np.dtype([("from", "i4"), ("to", "i4"), ("rel", "f8", 3), ("info", "f8", 6)], align=True)
OMEGA_ODO = np.array([[400.0, 30.0, 5.0], [30.0, 380.0, -8.0], [5.0, -8.0, 900.0]])
OMEGA_LOOP = np.diag([2500.0, 2500.0, 4000.0])
DEG = math.pi / 180.0


def info6(M):
    M = np.asarray(M, np.float64)
    return np.array([M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]])


def info33(v):
    return np.array([[v[0], v[1], v[2]], [v[1], v[3], v[4]], [v[2], v[4], v[5]]], np.float64)


def wrap_rad(v):
    return (np.asarray(v, np.float64) + math.pi) % (2.0 * math.pi) - math.pi


def wrap_deg(v):
    return (np.asarray(v, np.float64) + 180.0) % 360.0 - 180.0


# ---- poses (tx, ty, th[deg]) ----

def between(frm, to):
    """Pose2D::calMotion(to, from): the pose of `to` in `from`'s frame."""
    c, s = math.cos(frm[2] * DEG), math.sin(frm[2] * DEG)
    dx, dy = to[0] - frm[0], to[1] - frm[1]
    return np.array([c * dx + s * dy, -s * dx + c * dy, float(wrap_deg(to[2] - frm[2]))])


def compose(p, rel):
    """Pose2D::calPredPose(rel, p): p (+) rel."""
    c, s = math.cos(p[2] * DEG), math.sin(p[2] * DEG)
    return np.array([c * rel[0] - s * rel[1] + p[0], s * rel[0] + c * rel[1] + p[1], float(wrap_deg(p[2] + rel[2]))])


def inverse(rel):
    return between(rel, np.zeros(3))


def make_edges(rows):
    """[(from, to, rel[3], Omega 3x3)] -> PG_EDGE_DTYPE array."""
    e = np.zeros(len(rows), PG_EDGE_DTYPE)
    for k, (a, b, rel, om) in enumerate(rows):
        e[k]["from"], e[k]["to"], e[k]["rel"], e[k]["info"] = a, b, rel, info6(om)
    return e


# ---- the model ----

def residuals(x, edges):
    """x: [N, 3] poses in radians -> [E, 3] residuals."""
    i, j = edges["from"], edges["to"]
    c, s = np.cos(x[i, 2]), np.sin(x[i, 2])
    dx, dy = x[j, 0] - x[i, 0], x[j, 1] - x[i, 1]
    r = np.empty((len(edges), 3))
    r[:, 0] = c * dx + s * dy - edges["rel"][:, 0]
    r[:, 1] = -s * dx + c * dy - edges["rel"][:, 1]
    r[:, 2] = wrap_rad(x[j, 2] - x[i, 2] - edges["rel"][:, 2] * DEG)
    return r


def jacobians(x, edges):
    """-> (A, B): [E, 3, 3] each, d r / d x_from and d r / d x_to."""
    i, j = edges["from"], edges["to"]
    c, s = np.cos(x[i, 2]), np.sin(x[i, 2])
    dx, dy = x[j, 0] - x[i, 0], x[j, 1] - x[i, 1]
    E = len(edges)
    A, B = np.zeros((E, 3, 3)), np.zeros((E, 3, 3))
    A[:, 0, 0], A[:, 0, 1], A[:, 0, 2] = -c, -s, -s * dx + c * dy
    A[:, 1, 0], A[:, 1, 1], A[:, 1, 2] = s, -c, -c * dx - s * dy
    A[:, 2, 2] = -1.0
    B[:, 0, 0], B[:, 0, 1] = c, s
    B[:, 1, 0], B[:, 1, 1] = -s, c
    B[:, 2, 2] = 1.0
    return A, B


def omegas(edges):
    v = edges["info"]
    O = np.empty((len(edges), 3, 3))
    O[:, 0, 0], O[:, 0, 1], O[:, 0, 2] = v[:, 0], v[:, 1], v[:, 2]
    O[:, 1, 0], O[:, 1, 1], O[:, 1, 2] = v[:, 1], v[:, 3], v[:, 4]
    O[:, 2, 0], O[:, 2, 1], O[:, 2, 2] = v[:, 2], v[:, 4], v[:, 5]
    return O


def cost(x, edges):
    r = residuals(x, edges)
    return float(np.einsum("ea,eab,eb->", r, omegas(edges), r))


def cost_deg(poses, edges):
    x = np.array(poses, np.float64)
    x[:, 2] *= DEG
    return cost(x, edges)


def normal_equations(x, edges):
    """-> dense H [3N, 3N] and b [3N] of F = sum r^T Omega r (H = sum J^T Omega J, b = sum J^T Omega r)."""
    N = len(x)
    r, (A, B), O = residuals(x, edges), jacobians(x, edges), omegas(edges)
    H, b = np.zeros((N, 3, N, 3)), np.zeros((N, 3))
    i, j = edges["from"], edges["to"]
    OA, OB = O @ A, O @ B
    At, Bt = A.transpose(0, 2, 1), B.transpose(0, 2, 1)
    Hv = H.transpose(0, 2, 1, 3)                       # [N, N, 3, 3] view
    np.add.at(Hv, (i, i), At @ OA)
    np.add.at(Hv, (i, j), At @ OB)
    np.add.at(Hv, (j, i), Bt @ OA)
    np.add.at(Hv, (j, j), Bt @ OB)
    Or = np.einsum("eab,eb->ea", O, r)
    np.add.at(b, i, np.einsum("eba,eb->ea", A, Or))
    np.add.at(b, j, np.einsum("eba,eb->ea", B, Or))
    return H.reshape(3 * N, 3 * N), b.reshape(3 * N)


def oracle_optimize(poses, edges, eps_step=1e-12, max_iter=30):
    """Full Gauss-Newton steps, node 0 fixed, until max|d| < eps_step.  -> dict: poses (deg, wrapped), costs (the initial one and
    one per step), steps (max|d| of every step), converged."""
    x = np.array(poses, np.float64)
    x[:, 2] *= DEG
    costs, steps, conv = [cost(x, edges)], [], False
    for _ in range(max_iter):
        H, b = normal_equations(x, edges)
        d = np.linalg.solve(H[3:, 3:], -b[3:])
        x[1:] += d.reshape(-1, 3)
        costs.append(cost(x, edges))
        steps.append(float(np.abs(d).max()))
        if steps[-1] < eps_step:
            conv = True
            break
    out = x.copy()
    out[:, 2] = wrap_deg(out[:, 2] / DEG)
    out[0] = poses[0]
    return {"poses": out, "costs": costs, "steps": steps, "converged": conv}


END_ACCEPTED, END_RUNOUT_BELOW, END_RUNOUT_ABOVE, END_MAX_ITER = "accepted step below eps_step", "run-out below eps_step", \
    "run-out above eps_step", "max_iter"


def oracle_optimize_halving(poses, edges, eps_step=1e-12, max_iter=30, max_halvings=8):
    """The header's method with a dense solve in place of the conjugate gradients: the Gauss-Newton step d of the normal
    equations (node 0 fixed), tried at s = 1, 1/2, ... (max_halvings halvings at the most); the first trial whose F is finite
    and does not rise is taken.  The run ends at an accepted step with max|s d| < eps_step (END_ACCEPTED), at a step that no
    trial accepts (END_RUNOUT_BELOW / END_RUNOUT_ABOVE by the last trial's max|s d|) or at max_iter.
    -> dict: poses (deg, wrapped; the last accepted ones), costs (the initial one and one per accepted step), steps (max|s d| of
    every accepted step), converged, end, and per accepted step iterates (deg, wrapped), halvings, margins (the smallest
    |Ft - F| / F over the step's trials: how far the closest decision of the step was from a tie); refused: None, or
    (trials, max|s d| of the last trial, margin) of the step that ran out."""
    def out_deg(x):
        out = x.copy()
        out[:, 2] = wrap_deg(out[:, 2] / DEG)
        out[0] = poses[0]
        return out

    x = np.array(poses, np.float64)
    x[:, 2] *= DEG
    F = cost(x, edges)
    costs, steps, iterates, halvings, margins, refused, end = [F], [], [], [], [], None, END_MAX_ITER
    for _ in range(max_iter):
        H, b = normal_equations(x, edges)
        d = np.linalg.solve(H[3:, 3:], -b[3:]).reshape(-1, 3)
        s, margin, accepted = 1.0, math.inf, False
        for h in range(max_halvings + 1):
            if h:
                s *= 0.5
            xt = x.copy()
            xt[1:] += s * d
            Ft = cost(xt, edges)
            margin = min(margin, abs(Ft - F) / F) if math.isfinite(Ft) else margin
            if math.isfinite(Ft) and Ft <= F:
                accepted = True
                break
        dmax = s * float(np.abs(d).max())
        if not accepted:
            refused = (h + 1, dmax, margin)
            end = END_RUNOUT_BELOW if dmax < eps_step else END_RUNOUT_ABOVE
            break
        x, F = xt, Ft
        costs.append(F)
        steps.append(dmax)
        iterates.append(out_deg(x))
        halvings.append(h)
        margins.append(margin)
        if dmax < eps_step:
            end = END_ACCEPTED
            break
    return {"poses": out_deg(x), "costs": costs, "steps": steps, "converged": end in (END_ACCEPTED, END_RUNOUT_BELOW), "end": end,
            "iterates": iterates, "halvings": halvings, "margins": margins, "refused": refused}


def iterations_at(res, eps_step):
    """The number of steps the oracle's run takes until one is below eps_step."""
    for k, s in enumerate(res["steps"]):
        if s < eps_step:
            return k + 1
    return None


# ---- workloads ----

def eight_truth(N):
    t = np.arange(N) / float(N)
    th = np.arctan2(np.cos(2 * math.pi * t), 2 * np.cos(4 * math.pi * t))
    return np.stack([10 * np.sin(4 * math.pi * t), 10 * np.sin(2 * math.pi * t), th / DEG], axis=1)


def loop_pairs(N, n_loops=5):
    pairs = [(N - 1, 0), (N - 2, 1), (N // 2, 0), (3 * N // 4, N // 4), (N // 2 + 1, 1)]
    k = 0
    while len(pairs) < n_loops:                        # (the timing script's denser graphs)
        k += 1
        pairs.append((N - 1 - 7 * k, 5 * k))
    return pairs[:n_loops]


def _noisy(rel, rng, sig):
    n = rng.normal(0.0, 1.0, 3) * np.asarray(sig)
    return np.array([rel[0] + n[0], rel[1] + n[1], float(wrap_deg(rel[2] + n[2] / DEG))])


def figure_eight(N, n_loops=5, reverse_chain=False, duplicate=False):
    """-> (start poses [N, 3], edges).  Seed = N."""
    rng = np.random.default_rng(N)
    truth = eight_truth(N)
    sig = np.array([0.01, 0.01, 0.004]) * math.sqrt(10.0 / N)
    rows, start = [], [truth[0].copy()]
    for k in range(N - 1):
        if reverse_chain:                              # the arc stored as (k + 1 -> k)
            rel = _noisy(between(truth[k + 1], truth[k]), rng, sig)
            rows.append((k + 1, k, rel, OMEGA_ODO))
            start.append(compose(start[-1], inverse(rel)))
        else:
            rel = _noisy(between(truth[k], truth[k + 1]), rng, sig)
            rows.append((k, k + 1, rel, OMEGA_ODO))
            start.append(compose(start[-1], rel))
    for a, b in loop_pairs(N, n_loops):
        if a != b and 0 <= a < N and 0 <= b < N:
            rows.append((a, b, _noisy(between(truth[a], truth[b]), rng, (0.002, 0.002, 0.001)), OMEGA_LOOP))
    if duplicate:                                      # two more arcs between pairs that have one already
        a, b = N // 3, N // 3 + 1
        rows.append((a, b, _noisy(between(truth[a], truth[b]), rng, sig), OMEGA_ODO))
        a, b = loop_pairs(N)[0]
        rows.append((a, b, _noisy(between(truth[a], truth[b]), rng, (0.002, 0.002, 0.001)), OMEGA_LOOP))
    return np.array(start), make_edges(rows)


def shuffled(N):
    """The figure-eight with the nodes 1 .. N-1 permuted."""
    poses, edges = figure_eight(N)
    rng = np.random.default_rng(1000 + N)
    new_of = np.concatenate([[0], 1 + rng.permutation(N - 1)])
    out = np.empty_like(poses)
    out[new_of] = poses
    e = edges.copy()
    e["from"], e["to"] = new_of[edges["from"]], new_of[edges["to"]]
    return out, e


def star(N=40):
    """All arcs from node 0, plus every third (j, j + 2); the start is the truth disturbed."""
    rng = np.random.default_rng(7000 + N)
    truth = eight_truth(N)
    rows = [(0, j, _noisy(between(truth[0], truth[j]), rng, (0.01, 0.01, 0.004)), OMEGA_ODO) for j in range(1, N)]
    rows += [(j, j + 2, _noisy(between(truth[j], truth[j + 2]), rng, (0.002, 0.002, 0.001)), OMEGA_LOOP) for j in range(1, N - 2, 3)]
    start = truth.copy()
    start[1:, :2] += rng.normal(0.0, 0.05, (N - 1, 2))
    start[1:, 2] = wrap_deg(start[1:, 2] + rng.normal(0.0, 0.02, N - 1) / DEG)
    return start, make_edges(rows)


def far_start(N, sxy, sth, seed):
    """The arcs of figure_eight(N) from a start that drift has taken away: the nodes 1 .. N-1 moved by normal(0, sxy) metres in
    x and y, then turned by normal(0, sth) degrees."""
    poses, edges = figure_eight(N)
    rng = np.random.default_rng(seed)
    start = poses.copy()
    start[1:, :2] += rng.normal(0.0, sxy, (N - 1, 2))
    start[1:, 2] = wrap_deg(start[1:, 2] + rng.normal(0.0, sth, N - 1))
    return start, edges


def hub(N=300, at=7):
    """Every node tied to node `at` (every second arc stored towards it), plus every third (j, j + 2); the start is the truth
    disturbed.  The hub is a free node: its list holds N - 1 arcs."""
    rng = np.random.default_rng(9000 + N)
    truth = eight_truth(N)
    rows = []
    for j in range(N):
        if j == at:
            continue
        a, b = (j, at) if j % 2 else (at, j)
        rows.append((a, b, _noisy(between(truth[a], truth[b]), rng, (0.01, 0.01, 0.004)), OMEGA_ODO))
    rows += [(j, j + 2, _noisy(between(truth[j], truth[j + 2]), rng, (0.002, 0.002, 0.001)), OMEGA_LOOP) for j in range(1, N - 2, 3)]
    start = truth.copy()
    start[1:, :2] += rng.normal(0.0, 0.05, (N - 1, 2))
    start[1:, 2] = wrap_deg(start[1:, 2] + rng.normal(0.0, 0.02, N - 1) / DEG)
    return start, make_edges(rows)


def dense(N, E):
    """The chain of figure_eight(N) and E - (N - 1) arcs between random pairs, in either direction, pairs repeated."""
    poses, chain = figure_eight(N, n_loops=0)
    rng = np.random.default_rng(11000 + 7 * N + E)
    truth = eight_truth(N)
    rows = []
    while len(rows) < E - len(chain):
        a, b = (int(v) for v in rng.integers(0, N, 2))
        if a != b:
            rows.append((a, b, _noisy(between(truth[a], truth[b]), rng, (0.002, 0.002, 0.001)), OMEGA_LOOP))
    return poses, np.concatenate([chain, make_edges(rows)])


def scaled_info(N):
    """figure_eight(N) with every arc's information scaled by its own 10**uniform(-3, 3)."""
    poses, edges = figure_eight(N)
    rng = np.random.default_rng(13000 + N)
    e = edges.copy()
    e["info"] *= (10.0 ** rng.uniform(-3.0, 3.0, len(e)))[:, None]
    return poses, e


EIGHT_SIZES = (24, 63, 64, 65, 255, 256, 257, 1000)
WORKLOADS = {("eight", n): functools.partial(figure_eight, n) for n in EIGHT_SIZES}
WORKLOADS.update({("eight", 4): functools.partial(figure_eight, 4),
                  ("shuffled", 40): functools.partial(shuffled, 40), ("shuffled", 120): functools.partial(shuffled, 120),
                  ("star", 40): functools.partial(star, 40), ("star", 120): functools.partial(star, 120),
                  ("duplicate", 24): functools.partial(figure_eight, 24, duplicate=True),
                  ("reversed", 65): functools.partial(figure_eight, 65, reverse_chain=True)})


DENSE_SIZES = ((24, 127), (24, 128), (24, 129), (24, 600), (12, 1025))      # 2 E: 254, 256, 258 around the key array's 256; 2050
SHAPE_WORKLOADS = {("hub", 300): functools.partial(hub, 300, 7), ("scaled", 24): functools.partial(scaled_info, 24),
                   ("scaled", 65): functools.partial(scaled_info, 65)}
SHAPE_WORKLOADS.update({("dense%d_" % n, e): functools.partial(dense, n, e) for n, e in DENSE_SIZES})

# (N, sxy [m], sth [deg], seed) of far_start
FAR_STARTS = {"far24a": (24, 2.0, 60.0, 2), "far24b": (24, 1.5, 50.0, 2), "far65": (65, 2.0, 60.0, 9),
              "far257": (257, 2.0, 40.0, 4)}             # (N = 257: the node loops take two trips)
FAR_STEP_MIN = 1e-6                                    # a step the GPU test compares is longer than this ...
FAR_MARGIN_MIN = 1e-6                                  # ... and none of its decisions is closer to a tie than this
# (workload, max_halvings, eps_step, the end, accepted steps): a coarse eps_step between the length of a halved step and that of
# its full step -- `converged` is judged on the step taken (or the last one tried), not on the full one
FAR_COARSE_CASES = (("far24a", 8, 18.0, END_ACCEPTED, 2), ("far257", 1, 18.6, END_RUNOUT_BELOW, 2))
FAR_CAP_NAME = "far24a"
FAR_CAP_CASES = ((0, 2), (1, 3))                       # (max_halvings, the step of far24a that needs one more)


@functools.lru_cache(maxsize=None)
def far_workload(name):
    """(start poses, edges, the halving oracle's run to 1e-12 with the default max_halvings, the number of compared steps:
    those in front of the first one that is not longer than FAR_STEP_MIN) of FAR_STARTS[name], made once per process."""
    poses, edges = far_start(*FAR_STARTS[name])
    ref = oracle_optimize_halving(poses, edges, eps_step=1e-12, max_iter=30, max_halvings=8)
    k = next((i for i, s in enumerate(ref["steps"]) if not s > FAR_STEP_MIN), len(ref["steps"]))
    poses.setflags(write=False)
    edges.setflags(write=False)
    return poses, edges, ref, k


def rigid_move(poses, to_xy, turn_deg):
    """Every pose turned by turn_deg about pose 0's position, then translated so that pose 0 lies at to_xy."""
    p = np.asarray(poses, np.float64)
    c, s = math.cos(turn_deg * DEG), math.sin(turn_deg * DEG)
    d = p[:, :2] - p[0, :2]
    out = np.empty_like(p)
    out[:, 0] = c * d[:, 0] - s * d[:, 1] + to_xy[0]
    out[:, 1] = s * d[:, 0] + c * d[:, 1] + to_xy[1]
    out[:, 2] = wrap_deg(p[:, 2] + turn_deg)
    return out


@functools.lru_cache(maxsize=None)
def workload(key):
    """(start poses, edges, the oracle's run to 1e-12) of WORKLOADS[key] or SHAPE_WORKLOADS[key], made once per process;
    read-only."""
    poses, edges = (WORKLOADS.get(key) or SHAPE_WORKLOADS[key])()
    ref = oracle_optimize(poses, edges, eps_step=1e-12)
    poses.setflags(write=False)
    edges.setflags(write=False)
    return poses, edges, ref


def pack(graphs):
    """[(poses, edges)] -> (poses [sum N, 3], node_offsets, edges, edge_offsets) of one batched call."""
    no = np.zeros(len(graphs) + 1, np.uint64)
    eo = np.zeros(len(graphs) + 1, np.uint64)
    no[1:] = np.cumsum([len(p) for p, _ in graphs])
    eo[1:] = np.cumsum([len(e) for _, e in graphs])
    poses = np.concatenate([np.asarray(p, np.float64).reshape(-1, 3) for p, _ in graphs]) if int(no[-1]) else np.zeros((0, 3))
    edges = np.concatenate([np.asarray(e, PG_EDGE_DTYPE) for _, e in graphs]) if int(eo[-1]) else np.zeros(0, PG_EDGE_DTYPE)
    return np.ascontiguousarray(poses), no, np.ascontiguousarray(edges), eo


def pose_error(a, b):
    """-> (largest |d tx|, |d ty| in metres, largest |d th| in radians) between two pose arrays."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    dt = np.abs(wrap_deg(a[:, 2] - b[:, 2])) * DEG
    return float(np.abs(a[:, :2] - b[:, :2]).max()), float(dt.max())


# ---- re-posing ----

def repose_ref(xy, seg_offsets, old_poses, new_poses):
    """PointCloudMap::remakeMaps' point correction in numpy: relativePoint under the old pose, globalPoint under the new one,
    every operation rounded on its own in fp64, then float32.  A segment with bit-equal poses is copied through."""
    xy = np.asarray(xy, np.float32)
    out = xy.copy()
    for k in range(len(seg_offsets) - 1):
        a, b = int(seg_offsets[k]), int(seg_offsets[k + 1])
        po, pn = np.asarray(old_poses[k], np.float64), np.asarray(new_poses[k], np.float64)
        if po.tobytes() == pn.tobytes() or a >= b:
            continue
        a1, a2 = float(po[2]) * math.pi / 180, float(pn[2]) * math.pi / 180
        c1, s1, c2, s2 = math.cos(a1), math.sin(a1), math.cos(a2), math.sin(a2)
        dx = xy[a:b, 0].astype(np.float64) - po[0]
        dy = xy[a:b, 1].astype(np.float64) - po[1]
        lx = dx * c1 + dy * s1
        ly = dx * (-s1) + dy * c1
        gx = c2 * lx + (-s2) * ly + pn[0]
        gy = s2 * lx + c2 * ly + pn[1]
        out[a:b, 0], out[a:b, 1] = gx.astype(np.float32), gy.astype(np.float32)
    return out
