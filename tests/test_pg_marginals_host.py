"""The references of the pose-graph covariances without a device (tests/pg_marginal_helpers.py): the dense inverse against the
chain compounding on pure chains, ndt_pg_relative_cov and ndt_pg_edge_chi2 through the library against their restatements and
their refusals, and the decision fixture of the consistency gate on the dense reference alone."""
import ctypes as C

import numpy as np
import pytest

import pg_helpers as H
import pg_marginal_helpers as M


@pytest.fixture(scope="module")
def capi():
    from ndt_slam_amd import build, capi as c
    build.build()
    c.lib()
    return c


def test_record_layouts(capi):
    assert capi.PG_QUERY_DTYPE.itemsize == 16
    assert capi.PG_MARGINAL_DTYPE.itemsize == 232
    assert [capi.PG_MARGINAL_DTYPE.fields[f][1] for f in ("Saa", "Sab", "Sbb", "cg_iterations", "converged", "status", "pad")] == \
        [0, 72, 144, 216, 220, 224, 228]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("N", [2, 24, 66, 257])
def test_dense_inverse_against_chain_compounding(N, reverse):
    """Two references that share no code agree to 1e-10 max|Sigma| on pure chains."""
    poses, edges = H.figure_eight(N, n_loops=0, reverse_chain=reverse)
    D, K = M.dense_marginals(poses, edges), M.chain_compounding(poses, edges)
    scale = np.abs(D).max()
    diag = max(np.abs(M.block(D, a, a) - M.block(K, a, a)).max() for a in range(N))
    off = np.abs(D - K).max()
    print("chain N %d reverse %d: max|Sigma| %.3g | diagonal blocks %.3g cross blocks %.3g (of max|Sigma|)" % (N, reverse, scale, diag / scale, off / scale))
    assert off <= 1e-10 * scale
    assert (D[:3] == 0).all() and (D[:, :3] == 0).all()


def test_relative_cov_and_edge_chi2_against_their_restatements(capi):
    rng = np.random.default_rng(5)
    for N, name in ((24, "eight"), (65, "far")):
        poses, edges = H.figure_eight(N) if name == "eight" else H.far_start(*H.FAR_STARTS["far65"])
        S = M.dense_marginals(poses, edges)
        for a, b in M.query_pairs(N):
            if a == b or b == 0 and a == 0:
                continue
            Saa, Sab, Sbb = M.dense_query(S, a, b)
            m = np.zeros(1, capi.PG_MARGINAL_DTYPE)
            m[0]["Saa"], m[0]["Sab"], m[0]["Sbb"] = Saa.reshape(9), Sab.reshape(9), Sbb.reshape(9)
            got = capi.pg_relative_cov(poses[a], poses[b], m[0])
            want = M.relative_cov_ref(poses[a], poses[b], Saa, Sab, Sbb)
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (name, a, b)
            assert (got == got.T).all()
            e = H.make_edges([(a, b, H.between(poses[a], poses[b]) + rng.normal(0, 0.05, 3), H.OMEGA_LOOP if a % 2 else H.OMEGA_ODO)])[0]
            d2 = capi.pg_edge_chi2(poses[a], poses[b], e, got)
            ref = M.edge_chi2_ref(poses[a], poses[b], e, want)
            assert abs(d2 - ref) <= 1e-12 * ref, (name, a, b, d2, ref)


def test_edge_chi2_without_a_covariance_is_the_arcs_own_chi_square(capi):
    """rel_cov = 0: d2 = r^T Omega r, the heading difference wrapped."""
    a, b = np.array([1.0, 2.0, 170.0]), np.array([1.5, 2.5, -175.0])
    e = H.make_edges([(0, 1, np.array([0.3, -0.4, 10.0]), H.OMEGA_ODO)])[0]
    x = np.array([a, b])
    x[:, 2] *= H.DEG
    want = H.cost(x, H.make_edges([(0, 1, e["rel"], H.OMEGA_ODO)]))
    assert abs(capi.pg_edge_chi2(a, b, e, np.zeros((3, 3))) - want) <= 1e-12 * want


def test_helper_refusals(capi):
    L = capi.lib()
    a, b = np.array([0.0, 0.0, 10.0]), np.array([1.0, 0.5, 30.0])
    m = np.zeros(1, capi.PG_MARGINAL_DTYPE)
    m[0]["Sbb"] = np.diag([1e-4, 2e-4, 1e-5]).reshape(9)
    cov = np.zeros(9)
    d2 = C.c_double(-1.0)
    e = H.make_edges([(0, 1, np.array([1.0, 0.4, 20.0]), H.OMEGA_LOOP)])
    args = [a.ctypes.data, b.ctypes.data, m.ctypes.data, cov.ctypes.data]
    assert L.ndt_pg_relative_cov(*args) == 0 and (cov.reshape(3, 3) == cov.reshape(3, 3).T).all() and cov[0] > 0
    for k in range(4):
        assert L.ndt_pg_relative_cov(*[None if i == k else v for i, v in enumerate(args)]) == capi.NDT_E_ARG
    assert b"ndt_pg_relative_cov" in L.ndt_last_error(None)
    nan_pose = np.array([0.0, np.nan, 0.0])
    assert L.ndt_pg_relative_cov(nan_pose.ctypes.data, args[1], args[2], args[3]) == capi.NDT_E_ARG
    bad = m.copy()
    bad[0]["Sab"][4] = np.inf
    assert L.ndt_pg_relative_cov(args[0], args[1], bad.ctypes.data, args[3]) == capi.NDT_E_ARG
    zero = np.zeros(1, capi.PG_MARGINAL_DTYPE)                               # (what a query that did not converge gives)
    assert L.ndt_pg_relative_cov(args[0], args[1], zero.ctypes.data, args[3]) == capi.NDT_E_ARG
    neg = m.copy()
    neg[0]["Sbb"][0] = -1e-4
    assert L.ndt_pg_relative_cov(args[0], args[1], neg.ctypes.data, args[3]) == capi.NDT_E_ARG
    with pytest.raises(capi.NdtError, match="positive definite"):
        capi.pg_relative_cov(a, b, zero[0])

    good = np.diag([1e-3, 1e-3, 1e-4]).reshape(9).copy()
    args = [a.ctypes.data, b.ctypes.data, e.ctypes.data, good.ctypes.data, C.addressof(d2)]
    assert L.ndt_pg_edge_chi2(*args) == 0 and d2.value >= 0.0
    for k in range(5):
        assert L.ndt_pg_edge_chi2(*[None if i == k else v for i, v in enumerate(args)]) == capi.NDT_E_ARG
    assert L.ndt_pg_edge_chi2(nan_pose.ctypes.data, *args[1:]) == capi.NDT_E_ARG
    for field, k, v in (("rel", 1, np.nan), ("info", 0, np.inf), ("info", 0, -1.0), ("info", 5, 0.0)):
        e2 = e.copy()
        e2[0][field][k] = v
        assert L.ndt_pg_edge_chi2(args[0], args[1], e2.ctypes.data, args[3], args[4]) == capi.NDT_E_ARG, (field, k, v)
    for c in (np.diag([-1.0, 1e-3, 1e-3]), np.full((3, 3), np.nan)):
        c = np.ascontiguousarray(c.reshape(9))
        assert L.ndt_pg_edge_chi2(args[0], args[1], args[2], c.ctypes.data, args[4]) == capi.NDT_E_ARG


@pytest.mark.parametrize("N", [24, 65, 257])
def test_decision_fixture_on_the_dense_reference(N):
    """A true loop arc is consistent with the odometry in between at the 99 % bound of chi-square(3), a forged one is not."""
    _, _, _, cands, forged = M.decision_fixture(N)
    d2 = M.decision_dense(N)
    print("consistency N %d: true d2 %s | forged d2 %s" % (N, np.round(d2[~forged], 2), np.round(d2[forged], 1)))
    assert len(cands) == 10 and (d2[~forged] < M.CHI2_3_99).all() and (d2[forged] > M.CHI2_3_99).all()


def test_loop_closure_carries_a_consistency_bound():
    from ndt_slam_amd import replay
    lc = replay.LoopClosure(None, None, None, 1, 2)
    assert lc.consistency is None and len(lc) == 5 and lc._fields == ("loop", "pg", "odo_info", "every", "cooldown")
    assert replay.LoopClosure(None, None, None, 1, 2, consistency=M.CHI2_3_99).consistency == M.CHI2_3_99


def test_close_loops_drops_the_edges_above_the_bound_before_the_graph_is_built(capi, monkeypatch):
    """_close_loops with a bound: loop_consistency sees every session's found edges with that session's trajectory; an edge above
    the bound never reaches a graph, a session left without edges is not in the batch; without a bound nothing is asked."""
    from ndt_slam_amd import replay
    trajs = {0: np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]]), 1: np.array([[0.0, 0, 0], [0, 1, 90], [0, 2, 90]])}

    def loop(session, frm, to, found=1):
        l = np.zeros(1, capi.LOOP_DTYPE)[0]
        l["found"], l["cand"]["session"], l["edge"]["from_"], l["edge"]["to"] = found, session, frm, to
        l["edge"]["info"] = H.info6(H.OMEGA_LOOP)
        return l

    class Sessions:
        def find_loops(self, params, which):
            return [loop(0, 0, 3), loop(0, 1, 3), loop(1, 0, 2), loop(1, 0, 1, found=0)]

        def trajectory(self, i):
            return (trajs[i],)

        def correct(self, fix):
            self.fixed = sorted(fix)
            return self.fixed

    d2_of = {(0, 0, 3): 3.0, (0, 1, 3): 500.0, (1, 0, 2): 40.0}
    asked, batches = [], []

    def consistency(ctx, poses, odo_info, edges):
        i = next(k for k, t in trajs.items() if t.tobytes() == np.asarray(poses).tobytes())
        asked.append((i, len(edges)))
        return np.array([d2_of[(i, int(e["from_"]), int(e["to"]))] for e in edges])

    def closing(ctx, lc, poses, node_offsets, edges, edge_offsets, n_loop_arcs):
        batches.append((len(node_offsets) - 1, list(n_loop_arcs), [(int(e["from"]), int(e["to"])) for e in edges if abs(int(e["from"]) - int(e["to"])) != 1]))
        return poses, np.ones(len(node_offsets) - 1, dtype=bool)

    monkeypatch.setattr(replay, "loop_consistency", consistency)
    monkeypatch.setattr(replay, "_optimize_closing", closing)
    info = H.info6(H.OMEGA_ODO)
    s = Sessions()
    done = replay._close_loops(None, s, replay.LoopClosure(None, None, info, 1, 2, consistency=M.CHI2_3_99), np.ones(2, np.uint8))
    assert asked == [(0, 2), (1, 1)] and batches == [(1, [1], [(0, 3)])] and s.fixed == [0] and done.tolist() == [1, 0]
    asked.clear(); batches.clear()
    done = replay._close_loops(None, Sessions(), replay.LoopClosure(None, None, info, 1, 2), np.ones(2, np.uint8))
    assert asked == [] and batches == [(2, [2, 1], [(0, 3), (1, 3), (0, 2)])] and done.tolist() == [1, 1]
