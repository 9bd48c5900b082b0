"""References of the pose-graph covariance tests (ndt_pg_marginals_batch, ndt_pg_relative_cov, ndt_pg_edge_chi2; tests only,
numpy only).

dense_marginals    inv(H[3:, 3:]) of the header's H through pg_helpers.normal_equations, the weights applied to each arc's info.
chain_compounding  a second reference for graphs that are a pure chain: the covariance pushed along the chain arc by arc.  It
                   restates the Jacobians itself and shares no code with normal_equations.
relative_cov_ref, edge_chi2_ref
                   dense restatements of the two host helpers.
decision_fixture   the candidates of the consistency gate: a figure-eight's five true loop arcs and the same five forged.
The workloads are pg_helpers' generators.
"""
import functools
import math

import numpy as np

import pg_helpers as H

CHI2_3_99 = 11.34                                     # chi-square, 3 degrees of freedom, 99 %


def radians(poses):
    x = np.array(poses, np.float64).reshape(-1, 3)
    x[:, 2] *= H.DEG
    return x


def dense_marginals(poses, edges, weight=None):
    """-> Sigma [3 N, 3 N]: inv(H[3:, 3:]) at the poses given (deg), node 0's rows and columns zero."""
    e = np.array(edges, H.PG_EDGE_DTYPE)
    if weight is not None:
        e["info"] = e["info"] * np.asarray(weight, np.float64).reshape(-1, 1)
    Hd, _ = H.normal_equations(radians(poses), e)
    S = np.zeros_like(Hd)
    S[3:, 3:] = np.linalg.inv(Hd[3:, 3:])
    return S


def block(S, a, b):
    return S[3 * a:3 * a + 3, 3 * b:3 * b + 3]


def dense_query(S, a, b):
    """(Saa, Sab, Sbb) as the header defines them, from a dense Sigma."""
    sym = lambda M: 0.5 * (M + M.T)
    return sym(block(S, a, a)), block(S, a, b).copy(), sym(block(S, b, b))


def _arc_jacobians(xi, xj):
    """d r / d x_from, d r / d x_to of the header's residual at two poses in radians, written out entry by entry."""
    c, s = math.cos(xi[2]), math.sin(xi[2])
    dx, dy = xj[0] - xi[0], xj[1] - xi[1]
    A = np.array([[-c, -s, -s * dx + c * dy], [s, -c, -c * dx - s * dy], [0.0, 0.0, -1.0]])
    B = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
    return A, B


def chain_compounding(poses, edges):
    """A pure chain (arc k ties the nodes k and k + 1, stored in either direction) -> Sigma [3 N, 3 N] with node 0 fixed:
    Sigma_{k+1} = F Sigma_k F^T + G Omega^-1 G^T with F = -J_next^-1 J_prev, G = J_next^-1; Sigma_{a, b} = Sigma_a Phi^T for
    a < b with Phi = F_{b-1} ... F_a."""
    x = radians(poses)
    N = len(x)
    assert len(edges) == N - 1
    F = [None] * (N - 1)
    diag = [np.zeros((3, 3))]
    for k in range(N - 1):
        e = edges[k]
        i, j = int(e["from"]), int(e["to"])
        assert {i, j} == {k, k + 1}
        A, B = _arc_jacobians(x[i], x[j])
        J_prev, J_next = (A, B) if i == k else (B, A)
        G = np.linalg.inv(J_next)
        F[k] = -G @ J_prev
        diag.append(F[k] @ diag[k] @ F[k].T + G @ np.linalg.inv(H.info33(e["info"])) @ G.T)
    S = np.zeros((3 * N, 3 * N))
    for a in range(N):
        row = diag[a]
        S[3 * a:3 * a + 3, 3 * a:3 * a + 3] = row
        for b in range(a + 1, N):
            row = row @ F[b - 1].T
            S[3 * a:3 * a + 3, 3 * b:3 * b + 3] = row
            S[3 * b:3 * b + 3, 3 * a:3 * a + 3] = row.T
    return S


def _wrap(v):
    return (v + math.pi) % (2.0 * math.pi) - math.pi


def relative_cov_ref(pose_a, pose_b, Saa, Sab, Sbb):
    """ndt_pg_relative_cov restated: [Ja Jb] [[Saa Sab] [Sab^T Sbb]] [Ja Jb]^T."""
    xa, xb = radians([pose_a])[0], radians([pose_b])[0]
    Ja, Jb = _arc_jacobians(xa, xb)
    J = np.hstack([Ja, Jb])
    S = np.block([[np.asarray(Saa).reshape(3, 3), np.asarray(Sab).reshape(3, 3)], [np.asarray(Sab).reshape(3, 3).T, np.asarray(Sbb).reshape(3, 3)]])
    C = J @ S @ J.T
    return 0.5 * (C + C.T)


def edge_chi2_ref(pose_a, pose_b, edge, rel_cov):
    """ndt_pg_edge_chi2 restated: r^T (rel_cov + Omega^-1)^-1 r."""
    xa, xb = radians([pose_a])[0], radians([pose_b])[0]
    c, s = math.cos(xa[2]), math.sin(xa[2])
    dx, dy = xb[0] - xa[0], xb[1] - xa[1]
    r = np.array([c * dx + s * dy - edge["rel"][0], -s * dx + c * dy - edge["rel"][1], _wrap(xb[2] - xa[2] - edge["rel"][2] * H.DEG)])
    C = np.asarray(rel_cov, np.float64).reshape(3, 3)
    return float(r @ np.linalg.solve(0.5 * (C + C.T) + np.linalg.inv(H.info33(edge["info"])), r))


def dense_consistency(poses, odo_edges, candidates):
    """d2 of every candidate arc against the odometry-only graph, on the dense reference alone."""
    S = dense_marginals(poses, odo_edges)
    out = []
    for e in candidates:
        a, b = int(e["from"]), int(e["to"])
        C = relative_cov_ref(poses[a], poses[b], *dense_query(S, a, b))
        out.append(edge_chi2_ref(poses[a], poses[b], e, C))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def decision_fixture(N):
    """figure_eight(N) with the odometry arcs' information set to the generator's own noise, diag(1 / sigma^2) with
    sigma = (0.01, 0.01, 0.004) sqrt(10 / N), and the loop arcs' to diag(1 / (0.002, 0.002, 0.001)^2) -> (poses, the odometry
    arcs, the odometry information as six numbers, the candidates: the five true loop arcs, then the same five with
    rel[0] += 1.0, the forged flags); read-only."""
    poses, edges = H.figure_eight(N)
    sig = np.array([0.01, 0.01, 0.004]) * math.sqrt(10.0 / N)
    odo_info = H.info6(np.diag(1.0 / sig ** 2))
    odo, loops = edges[:N - 1].copy(), edges[N - 1:].copy()
    assert len(loops) == 5 and (np.abs(odo["from"] - odo["to"]) == 1).all()
    odo["info"] = odo_info
    loops["info"] = H.info6(np.diag(1.0 / np.array([0.002, 0.002, 0.001]) ** 2))
    forged = loops.copy()
    forged["rel"][:, 0] += 1.0
    cands = np.concatenate([loops, forged])
    flags = np.array([False] * 5 + [True] * 5)
    for a in (poses, odo, odo_info, cands, flags):
        a.setflags(write=False)
    return poses, odo, odo_info, cands, flags


@functools.lru_cache(maxsize=None)
def decision_dense(N):
    poses, odo, _, cands, _ = decision_fixture(N)
    d2 = dense_consistency(poses, odo, cands)
    d2.setflags(write=False)
    return d2


def query_nodes(N):
    """The nodes the GPU tests query, where they exist: {0, 1, 2, 64, 65, N / 2, N - 2, N - 1}."""
    return sorted({v for v in (0, 1, 2, 64, 65, N // 2, N - 2, N - 1) if 0 <= v < N})


def query_pairs(N):
    """Pairs over query_nodes(N): every a == b, adjacent nodes, a < b and a > b, in the same piece of the sweep and across."""
    nodes = query_nodes(N)
    pairs = [(a, a) for a in nodes]
    pairs += [(a, b) for a, b in zip(nodes[:-1], nodes[1:])] + [(b, a) for a, b in zip(nodes[:-1], nodes[1:])]
    pairs += [(nodes[0], nodes[-1]), (nodes[-1], nodes[1 % len(nodes)]), (nodes[len(nodes) // 2], nodes[-1])]
    return list(dict.fromkeys(pairs))
