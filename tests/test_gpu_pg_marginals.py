"""ndt_pg_marginals_batch* on the device against the dense inverse of tests/pg_marginal_helpers.py: the blocks on graphs from two
nodes to 300 and around the pieces of the sweep and the trips of the node loops, pure chains against the chain compounding, the
bytes that must not depend on the batch or the slot of a column, arc weights, per-query faults and synchronous refusals, and the
consistency gate on the decision fixture through replay.loop_consistency."""
import ctypes as C
import functools

import numpy as np
import pytest

import pg_helpers as H
import pg_marginal_helpers as M
from gpu_support import gpu, to_dev, sync  # noqa: F401

pytestmark = pytest.mark.gpu

# Every entry of the three blocks against the graph's dense value, as a part of max|Sigma_dense|.  A numpy prototype of the
# same PCG (cg_rtol = 1e-10) lies within 4.3e-11 of the dense inverse over exactly these workloads (hub(300) the worst; 1.4e-11
# at cg_rtol = 1e-12), so the bound leaves a factor of 23 for the device's different summation order.
BLOCK_TOL = 1e-9

WORKLOADS = {("eight", n): functools.partial(H.figure_eight, n) for n in (2, 4, 24, 65, 66, 257, 258)}
WORKLOADS.update({("shuffled", 120): functools.partial(H.shuffled, 120), ("star", 40): functools.partial(H.star, 40),
                  ("hub", 300): functools.partial(H.hub, 300, 7), ("scaled", 65): functools.partial(H.scaled_info, 65),
                  ("dense24_", 600): functools.partial(H.dense, 24, 600),
                  ("far", 65): functools.partial(H.far_start, *H.FAR_STARTS["far65"])})      # linearised away from the minimum


@functools.lru_cache(maxsize=None)
def workload(key):
    """(poses, edges, the dense Sigma) of a workload, made once per process; read-only."""
    poses, edges = WORKLOADS[key]()
    S = M.dense_marginals(poses, edges)
    for a in (poses, edges, S):
        a.setflags(write=False)
    return poses, edges, S


def marginals(gpu, graphs, queries, weight=None, **prm):
    """One host-form call over [(poses, edges)] -> one record per query."""
    capi, ctx = gpu
    poses, no, edges, eo = H.pack(graphs)
    return capi.pose_graph_marginals(ctx, poses, no, edges, eo, queries, weight, capi.default_pg_params(**prm))


def blocks(rec):
    return rec["Saa"].reshape(3, 3), rec["Sab"].reshape(3, 3), rec["Sbb"].reshape(3, 3)


def worst_gap(recs, pairs, S):
    gap = 0.0
    for rec, (a, b) in zip(recs, pairs):
        for got, want in zip(blocks(rec), M.dense_query(S, a, b)):
            gap = max(gap, float(np.abs(got - want).max()))
    return gap


# ------------------------------------------------------------------------------------------ 1: against the dense inverse
@pytest.mark.parametrize("key", sorted(WORKLOADS, key=str))
def test_blocks_against_the_dense_inverse(gpu, key):
    poses, edges, S = workload(key)
    N = len(poses)
    pairs = M.query_pairs(N)
    recs = marginals(gpu, [(poses, edges)], [(0, a, b) for a, b in pairs])
    scale = float(np.abs(S).max())
    gap = worst_gap(recs, pairs, S)
    print("pg marginals %s%s: N %d E %d queries %d | max|Sigma| %.4g | worst gap %.3g of it | cg iterations %d .. %d (cap %d)"
          % (key[0], key[1], N, len(edges), len(pairs), scale, gap / scale, recs["cg_iterations"].min(), recs["cg_iterations"].max(), 6 * N))
    assert (recs["status"] == 0).all() and (recs["converged"] == 1).all()
    assert gap <= BLOCK_TOL * scale
    for rec, (a, b) in zip(recs, pairs):
        Saa, Sab, Sbb = blocks(rec)
        assert (Saa == Saa.T).all() and (Sbb == Sbb.T).all()
        if a == 0:
            assert (Saa == 0).all() and (Sab == 0).all()
        if b == 0:
            assert (Sbb == 0).all() and (Sab == 0).all()
        if a == b:
            assert Sab.tobytes() == Saa.tobytes() == Sbb.tobytes()
        assert rec["cg_iterations"] == 0 if a == b == 0 else 1 <= rec["cg_iterations"] <= 6 * N


# ------------------------------------------------------------------------------------------ 2: pure chains
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("N", [24, 66, 257])
def test_pure_chains_take_one_or_two_iterations(gpu, N, reverse):
    """T = H exactly: the preconditioner is the inverse.  Held to the chain compounding, which shares nothing with the dense H."""
    poses, edges = H.figure_eight(N, n_loops=0, reverse_chain=reverse)
    S = M.chain_compounding(poses, edges)
    pairs = M.query_pairs(N)
    recs = marginals(gpu, [(poses, edges)], [(0, a, b) for a, b in pairs])
    scale = float(np.abs(S).max())
    gap = worst_gap(recs, pairs, S)
    print("pg marginals chain N %d reverse %d: worst gap %.3g of max|Sigma| | cg iterations up to %d" % (N, reverse, gap / scale, recs["cg_iterations"].max()))
    assert (recs["status"] == 0).all() and (recs["converged"] == 1).all() and recs["cg_iterations"].max() <= 2
    assert gap <= BLOCK_TOL * scale


# ------------------------------------------------------------------------------------------ 3: bytes
BATCH_KEYS = (("eight", 24), ("eight", 65), ("star", 40), ("eight", 66), ("dense24_", 600), ("eight", 4))


def batch_queries():
    """40 queries over the 6 graphs of BATCH_KEYS, the graphs interleaved."""
    per = [[(g, a, b) for a, b in M.query_pairs(len(workload(k)[0]))] for g, k in enumerate(BATCH_KEYS)]
    out, i = [], 0
    while len(out) < 40:
        for q in per:
            if i < len(q) and len(out) < 40:
                out.append(q[i])
        i += 1
    return out


def test_a_query_does_not_depend_on_the_batch_or_its_order(gpu):
    graphs = [workload(k)[:2] for k in BATCH_KEYS]
    qs = batch_queries()
    assert len(qs) == 40 and {q[0] for q in qs} == set(range(6))
    fwd = marginals(gpu, graphs, qs)
    rev = marginals(gpu, graphs, qs[::-1])[::-1]
    assert (fwd["status"] == 0).all() and (fwd["converged"] == 1).all()
    assert fwd.tobytes() == rev.tobytes()
    for k, (g, a, b) in enumerate(qs):
        alone = marginals(gpu, [graphs[g]], [(0, a, b)])
        assert alone[0].tobytes() == fwd[k].tobytes(), (g, a, b)


def test_a_column_does_not_depend_on_its_slot_or_the_other_node(gpu):
    poses, edges, _ = workload(("eight", 66))
    a, b, c = 65, 2, 33
    r = marginals(gpu, [(poses, edges)], [(0, a, b), (0, a, a), (0, c, a), (0, b, a), (0, 0, a), (0, a, 0), (0, 0, 0)])
    assert (r["status"] == 0).all() and (r["converged"] == 1).all()
    assert r[0]["Saa"].tobytes() == r[1]["Saa"].tobytes() == r[2]["Sbb"].tobytes() == r[3]["Sbb"].tobytes() == r[4]["Sbb"].tobytes() \
        == r[5]["Saa"].tobytes()
    assert r[0]["Sbb"].tobytes() == r[3]["Saa"].tobytes()
    for k in range(7):
        Saa, Sab, Sbb = blocks(r[k])
        assert (Saa == Saa.T).all() and (Sbb == Sbb.T).all()
    for k, zero in ((4, ("Saa", "Sab")), (5, ("Sab", "Sbb")), (6, ("Saa", "Sab", "Sbb"))):
        for f in zero:
            assert r[k][f].tobytes() == np.zeros(9).tobytes(), (k, f)                # (exactly +0.0)
    assert r[6]["cg_iterations"] == 0


def test_no_weights_are_weights_of_one_and_the_device_form_is_the_host_form(gpu):
    import torch
    capi, ctx = gpu
    graphs = [workload(k)[:2] for k in BATCH_KEYS[:3]]
    qs = [q for q in batch_queries() if q[0] < 3]
    poses, no, edges, eo = H.pack(graphs)
    before = poses.copy()
    want = capi.pose_graph_marginals(ctx, poses, no, edges, eo, qs)
    assert poses.tobytes() == before.tobytes()
    ones = capi.pose_graph_marginals(ctx, poses, no, edges, eo, qs, np.ones(len(edges)))
    assert ones.tobytes() == want.tobytes()
    d_p, d_e = to_dev(poses.reshape(-1)), to_dev(edges.view(np.uint8))
    d_w = to_dev(np.ones(len(edges)))
    for w in (None, d_w):
        d_o = torch.full((len(qs) * capi.PG_MARGINAL_DTYPE.itemsize,), 0xEE, dtype=torch.uint8, device="cuda")
        sync()                                            # (the context works on a stream of its own)
        capi.pose_graph_marginals_dev(ctx, d_p.data_ptr(), no, d_e.data_ptr(), eo, qs, d_o.data_ptr(), w.data_ptr() if w is not None else None)
        sync()
        assert d_o.cpu().numpy().tobytes() == want.tobytes()
        assert d_p.cpu().numpy().tobytes() == before.tobytes()


# ------------------------------------------------------------------------------------------ 4: weights
def test_an_arc_of_weight_zero_is_an_arc_that_is_not_there(gpu):
    poses, edges, _ = workload(("eight", 24))
    N, E = len(poses), len(edges)
    pairs = M.query_pairs(N)
    qs = [(0, a, b) for a, b in pairs]
    w = np.ones(E)
    w[E - 1] = 0.0                                        # the last arc: every sum ends with + 0.0, the bytes are the smaller graph's
    assert marginals(gpu, [(poses, edges)], qs, w).tobytes() == marginals(gpu, [(poses, edges[:E - 1])], qs).tobytes()
    w = np.ones(E)
    w[N - 1] = 0.0                                        # the first loop arc: its sums change their order
    without = np.concatenate([edges[:N - 1], edges[N:]])
    S = M.dense_marginals(poses, without)
    assert np.abs(S - M.dense_marginals(poses, edges, w)).max() <= 1e-12 * np.abs(S).max()
    recs = marginals(gpu, [(poses, edges)], qs, w)
    assert (recs["converged"] == 1).all() and worst_gap(recs, pairs, S) <= BLOCK_TOL * np.abs(S).max()
    w = np.concatenate([np.ones(N - 1), [0.3, 2.0, 0.0, 1e-3, 1.0]])                 # (a robust call's weights, and one above 1)
    S = M.dense_marginals(poses, edges, w)
    recs = marginals(gpu, [(poses, edges)], qs, w)
    assert (recs["converged"] == 1).all() and worst_gap(recs, pairs, S) <= BLOCK_TOL * np.abs(S).max()


@pytest.mark.parametrize("N", [24, 65])
def test_closing_loops_shrinks_the_uncertainty(gpu, N):
    poses, edges, _ = workload(("eight", N))
    w = np.concatenate([np.ones(N - 1), np.zeros(5)])
    (closed,), (open_,) = marginals(gpu, [(poses, edges)], [(0, N - 1, N - 1)]), marginals(gpu, [(poses, edges)], [(0, N - 1, N - 1)], w)
    assert closed["converged"] == 1 and open_["converged"] == 1 and open_["cg_iterations"] <= 2
    t_closed, t_open = np.trace(closed["Sbb"].reshape(3, 3)), np.trace(open_["Sbb"].reshape(3, 3))
    print("pg marginals N %d: trace Sbb of the last node %.4g with the loops, %.4g without" % (N, t_closed, t_open))
    assert 0.0 < t_closed < t_open


# ------------------------------------------------------------------------------------------ 5: faults and refusals
def test_a_fault_costs_its_own_query_alone(gpu):
    good = workload(("eight", 24))[:2]
    poses, edges = good
    E = len(edges)
    nan_pose = poses.copy()
    nan_pose[7, 1] = np.inf
    bad_arc = edges.copy()
    bad_arc["to"][3] = 24
    graphs = [good, (nan_pose, edges), good, good, (poses, bad_arc), (np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]), np.zeros(0, H.PG_EDGE_DTYPE))]
    w = np.ones(5 * E)                                    # (the last graph has no arcs)
    w[2 * E + 5] = np.nan                                 # graph 2
    w[3 * E + E - 1] = -0.5                               # graph 3
    qs = [(0, 5, 20), (1, 5, 20), (2, 5, 20), (3, 5, 20), (4, 5, 20), (5, 1, 1), (5, 0, 1), (5, 0, 0),
          (-1, 1, 2), (6, 1, 2), (0, -1, 2), (0, 2, 24), (0, 24, 24), (0, 20, 5)]
    recs = marginals(gpu, graphs, qs, w)
    zero = np.zeros(27).tobytes()
    for k in (1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12):
        r = recs[k]
        assert (r["status"], r["converged"], r["cg_iterations"]) == (-1, 0, 0), (k, r)
        assert np.concatenate([r["Saa"], r["Sab"], r["Sbb"]]).tobytes() == zero, k
    r = recs[7]                                           # both nodes are node 0: nothing to solve, on a graph without arcs too
    assert (r["status"], r["converged"], r["cg_iterations"]) == (0, 1, 0) and np.concatenate([r["Saa"], r["Sab"], r["Sbb"]]).tobytes() == zero
    alone = marginals(gpu, [good], [(0, 5, 20), (0, 20, 5)])
    assert recs[0].tobytes() == alone[0].tobytes() and recs[13].tobytes() == alone[1].tobytes()
    assert recs[0]["converged"] == 1 and recs[0]["Saa"].tobytes() == recs[13]["Sbb"].tobytes()


def test_a_node_that_nothing_ties_to_node_0_and_the_iteration_cap(gpu):
    poses, edges, _ = workload(("eight", 24))
    p = np.vstack([poses, [[1.0, 1.0, 10.0], [2.0, 1.0, 20.0], [3.0, 2.0, 30.0]]])
    e = np.concatenate([edges, H.make_edges([(24, 25, [1.0, 0.0, 10.0], H.OMEGA_ODO), (25, 26, [1.0, 0.5, 10.0], H.OMEGA_ODO)])])
    recs = marginals(gpu, [(p, e), (poses, edges)], [(0, 5, 25), (0, 5, 6), (1, 5, 6)])
    zero = np.zeros(27).tobytes()
    for r in recs[:2]:                                    # (the factor is the graph's: a query of tied nodes ends the same way)
        assert (r["status"], r["converged"]) == (0, 0) and np.concatenate([r["Saa"], r["Sab"], r["Sbb"]]).tobytes() == zero
    assert recs[2]["converged"] == 1
    # a chain cut by a weight of 0
    chain = H.figure_eight(24, n_loops=0)
    w = np.ones(23)
    w[11] = 0.0
    r, = marginals(gpu, [chain], [(0, 3, 20)], w)
    assert (r["status"], r["converged"]) == (0, 0) and np.concatenate([r["Saa"], r["Sab"], r["Sbb"]]).tobytes() == zero
    # the cap
    r, = marginals(gpu, [(poses, edges)], [(0, 5, 20)], cg_max_iter=1)
    assert (r["status"], r["converged"], r["cg_iterations"]) == (0, 0, 1) and np.concatenate([r["Saa"], r["Sab"], r["Sbb"]]).tobytes() == zero
    r, = marginals(gpu, [chain], [(0, 5, 20)], cg_max_iter=2, max_iter=1, max_halvings=0, eps_step=0.0)      # (the other fields are not read)
    assert (r["status"], r["converged"]) == (0, 1) and r["cg_iterations"] <= 2


def test_synchronous_refusals(gpu):
    capi, ctx = gpu
    L = capi.lib()
    poses, no, edges, eo = H.pack([workload(("eight", 24))[:2]])
    qs = np.zeros(1, capi.PG_QUERY_DTYPE)
    qs[0]["a"], qs[0]["b"] = 5, 20
    out = np.zeros(1, capi.PG_MARGINAL_DTYPE)
    ok = capi.default_pg_params()

    def call(p=poses.ctypes.data, n=no.ctypes.data, e=edges.ctypes.data, o=eo.ctypes.data, G=1, w=None, q=qs.ctypes.data, Q=1, prm=ok,
             r=out.ctypes.data, dev=False):
        prm = C.byref(prm) if prm is not None else None
        if dev:
            return L.ndt_pg_marginals_batch_dev(ctx.h, p, n, e, o, G, w, q, Q, prm, r, None)
        return L.ndt_pg_marginals_batch(ctx.h, p, n, e, o, G, w, q, Q, prm, r)

    for dev in (False, True):
        for kw in (dict(p=None), dict(n=None), dict(e=None), dict(o=None), dict(prm=None), dict(r=None), dict(G=0), dict(G=-3), dict(q=None),
                   dict(Q=0), dict(Q=-1)):
            assert call(dev=dev, **kw) == capi.NDT_E_ARG, (dev, kw)
        down = np.array([5, 2], np.uint64)
        assert call(n=down.ctypes.data, dev=dev) == capi.NDT_E_ARG
        assert call(o=down.ctypes.data, dev=dev) == capi.NDT_E_ARG
        for bad in (dict(cg_max_iter=-1), dict(cg_rtol=0.0), dict(cg_rtol=1.0), dict(cg_rtol=float("nan")), dict(max_iter=0)):
            assert call(prm=capi.default_pg_params(**bad), dev=dev) == capi.NDT_E_ARG, (dev, bad)
    assert L.ndt_pg_marginals_batch(None, poses.ctypes.data, no.ctypes.data, edges.ctypes.data, eo.ctypes.data, 1, None, qs.ctypes.data, 1,
                                    C.byref(ok), out.ctypes.data) == capi.NDT_E_ARG
    assert out.tobytes() == np.zeros(1, capi.PG_MARGINAL_DTYPE).tobytes()
    # an open ndt_map_rebuild_begin on the context
    import torch
    cloud = torch.rand((4000, 2), dtype=torch.float32, device="cuda") * 20
    torch.cuda.synchronize()
    m = capi.Map(ctx, dev_ptr=cloud.data_ptr(), n=4000, params=capi.default_params())
    m.rebuild_begin(cloud.data_ptr(), 4000)
    try:
        assert call() == capi.NDT_E_ARG and "rebuild" in L.ndt_last_error(ctx.h).decode()
        assert call(dev=True) == capi.NDT_E_ARG
    finally:
        m.rebuild_end()
    m.close()
    assert call() == 0 and out["converged"][0] == 1 and out["status"][0] == 0


# ------------------------------------------------------------------------------------------ 6: the consistency gate
@pytest.mark.parametrize("N", [24, 65, 257])
def test_consistency_gate_on_the_decision_fixture(gpu, N):
    """The five true loop arcs of a figure-eight pass the 99 % bound of chi-square(3) against the odometry in between, the same
    five with rel[0] += 1.0 do not -- on the dense reference first, then through replay.loop_consistency."""
    from ndt_slam_amd import replay
    capi, ctx = gpu
    poses, odo, odo_info, cands, forged = M.decision_fixture(N)
    ref = M.decision_dense(N)
    assert (ref[~forged] < M.CHI2_3_99).all() and (ref[forged] > M.CHI2_3_99).all()
    assert replay.loops_graph(poses, [], odo_info)["info"].tobytes() == odo["info"].tobytes()
    d2 = replay.loop_consistency(ctx, poses, odo_info, list(cands))
    print("consistency N %d: true d2 %s (dense %s) | forged d2 %s" % (N, np.round(d2[~forged], 3), np.round(ref[~forged], 3), np.round(d2[forged], 1)))
    assert (d2[~forged] < M.CHI2_3_99).all() and (d2[forged] > M.CHI2_3_99).all()
    assert (np.abs(d2 - ref) <= 1e-6 * ref).all()
