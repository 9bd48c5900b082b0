"""Oracle and workloads of the pose-graph tests (ndt_pg_*, ndt_repose_points; tests only).

oracle_optimize   a dense numpy restatement of the header's model: the same residuals and analytic Jacobians, the normal
                  equations solved by numpy.linalg.solve, full Gauss-Newton steps, no halving.
figure_eight ...  the graph generators.
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


EIGHT_SIZES = (24, 63, 64, 65, 255, 256, 257, 1000)
WORKLOADS = {("eight", n): functools.partial(figure_eight, n) for n in EIGHT_SIZES}
WORKLOADS.update({("eight", 4): functools.partial(figure_eight, 4),
                  ("shuffled", 40): functools.partial(shuffled, 40), ("shuffled", 120): functools.partial(shuffled, 120),
                  ("star", 40): functools.partial(star, 40), ("star", 120): functools.partial(star, 120),
                  ("duplicate", 24): functools.partial(figure_eight, 24, duplicate=True),
                  ("reversed", 65): functools.partial(figure_eight, 65, reverse_chain=True)})


@functools.lru_cache(maxsize=None)
def workload(key):
    """(start poses, edges, the oracle's run to 1e-12) of WORKLOADS[key], made once per process; read-only."""
    poses, edges = WORKLOADS[key]()
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
