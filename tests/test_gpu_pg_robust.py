"""ndt_pg_optimize_robust_batch* on the device against the dense graduated-non-convexity oracle of tests/pg_robust_helpers.py:
the invariant that ties it to ndt_pg_optimize_batch, counts, poses and weights on the drifted workloads from two nodes to 257
and around the key array's power of two, independence of the batch, the per-graph faults and the synchronous refusals, the caps,
a component held by a rejected arc alone, and a resident two-session set that a forged loop arc no longer bends."""
import ctypes as C

import numpy as np
import pytest

import pg_helpers as H
import pg_robust_helpers as R
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-8                                       # metres and radians: the plain optimiser's parity bound
WEIGHT_TOL = 1e-6                                     # dw/dc <= 2 / phi and dc <= 2 |Omega r| POSE_TOL for a kept arc; a rejected arc's weight is below it
MU0_RTOL = 1e-12                                      # a max of sums of nine products


def params(capi, **kw):
    kw.setdefault("pg_eps_step", R.CMP_EPS_STEP)
    return capi.default_pg_robust_params(**kw)


def solve(gpu, graphs, prm=None, **kw):
    """One host-form call over [(poses, edges, phi)] -> [(poses, record, weights, chi2)] per graph."""
    capi, ctx = gpu
    poses, no, edges, eo, phi = R.pack_robust(graphs)
    out, res, w, c = capi.optimize_pose_graphs_robust(ctx, poses, no, edges, eo, phi, prm if prm is not None else params(capi, **kw))
    return [(out[int(no[g]):int(no[g + 1])], res[g], w[int(eo[g]):int(eo[g + 1])], c[int(eo[g]):int(eo[g + 1])]) for g in range(len(graphs))]


def solve_dev(gpu, graphs, prm=None, **kw):
    """The same through ndt_pg_optimize_robust_batch_dev, the arrays in torch tensors."""
    import torch
    capi, ctx = gpu
    poses, no, edges, eo, phi = R.pack_robust(graphs)
    dev = torch.device("cuda", 0)
    E = max(len(edges), 1)
    d_p = torch.from_numpy(poses.reshape(-1).copy() if poses.size else np.zeros(3)).to(dev)
    d_e = torch.from_numpy((edges if edges.size else np.zeros(1, H.PG_EDGE_DTYPE)).view(np.uint8).copy()).to(dev)
    d_f = torch.from_numpy(phi.copy() if phi.size else np.zeros(1)).to(dev)
    d_r = torch.zeros(len(graphs) * capi.PG_ROBUST_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_w, d_c = torch.full((E,), -1.0, dtype=torch.float64, device=dev), torch.full((E,), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()                          # (the context works on a stream of its own)
    capi.optimize_pose_graphs_robust_dev(ctx, d_p.data_ptr(), no, d_e.data_ptr(), eo, d_r.data_ptr(), d_f.data_ptr(), d_w.data_ptr(),
                                         d_c.data_ptr(), prm if prm is not None else params(capi, **kw))
    torch.cuda.synchronize()
    out = d_p.cpu().numpy().reshape(-1, 3)
    res = np.frombuffer(d_r.cpu().numpy().tobytes(), dtype=capi.PG_ROBUST_RESULT_DTYPE)
    w, c = d_w.cpu().numpy(), d_c.cpu().numpy()
    return [(out[int(no[g]):int(no[g + 1])], res[g], w[int(eo[g]):int(eo[g + 1])], c[int(eo[g]):int(eo[g + 1])]) for g in range(len(graphs))]


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def workload(name):
    return R.robust_workload(name)[:3]


# ------------------------------------------------------------------------------------------ 1: the invariant
@pytest.mark.parametrize("name", ["eight24", "far24a", "dense24_128"])
def test_without_robust_arcs_it_is_the_plain_optimiser_byte_for_byte(gpu, name):
    capi, ctx = gpu
    poses, edges = {"eight24": lambda: H.workload(("eight", 24))[:2], "far24a": lambda: H.far_workload("far24a")[:2],
                    "dense24_128": lambda: H.workload(("dense24_", 128))[:2]}[name]()
    for pg in (dict(), dict(max_iter=3), dict(max_halvings=1, eps_step=1e-6)):
        want_p, want_r = capi.optimize_pose_graphs(ctx, poses, [0, len(poses)], edges, [0, len(edges)], capi.default_pg_params(**pg))
        for phi, mu0 in ((None, 0.0), (np.zeros(len(edges)), 0.0), (np.zeros(len(edges)), 1.0), (np.zeros(len(edges)), 1e6)):
            prm = capi.default_pg_robust_params(mu0=mu0, **{"pg_" + k: v for k, v in pg.items()})
            if "max_iter" not in pg:
                prm.pg.max_iter = capi.default_pg_params().max_iter
            got_p, got_r, w, c = capi.optimize_pose_graphs_robust(ctx, poses, [0, len(poses)], edges, [0, len(edges)], phi, prm)
            assert got_p.tobytes() == want_p.tobytes(), (name, pg, mu0)
            assert got_r[0]["pg"].tobytes() == want_r[0].tobytes(), (name, pg, mu0, got_r[0], want_r[0])
            assert (w == 1.0).all() and len(w) == len(edges)
            assert (got_r[0]["mu0"], got_r[0]["levels"], got_r[0]["n_robust"], got_r[0]["n_rejected"]) == (1.0, 1, 0, 0)
            x = np.array(got_p)
            x[:, 2] *= H.DEG
            assert np.allclose(c, R.arc_chi2(x, edges), rtol=1e-9, atol=1e-18)


# ------------------------------------------------------------------------------------------ 2: against the oracle
@pytest.mark.parametrize("name", sorted(R.ROBUST_WORKLOADS))
def test_counts_poses_and_weights_against_the_oracle(gpu, name):
    """Every decision of these workloads is far from a tie (tests/test_pg_robust_host.py), so the counts are the oracle's; the
    poses are the oracle's iterate at the same trip (POSE_TOL) and the weights follow (WEIGHT_TOL)."""
    poses, edges, phi, bad, ref = R.robust_workload(name)
    (got, r, w, c), = solve(gpu, [(poses, edges, phi)])
    rb = phi > 0
    d_xy, d_th = H.pose_error(got, ref["poses"])
    dw = float(np.abs(w - ref["weights"]).max())
    print("pg robust %s: N %d E %d | mu0 %.9g (oracle %.9g) levels %d (%d) steps %d (%d) rejected %d (%d) cg %d | d_xy %.3g m d_th %.3g rad "
          "d_w %.3g | F_1 %.6g -> %.9g (oracle %.9g)"
          % (name, len(poses), len(edges), r["mu0"], ref["mu0"], r["levels"], ref["levels"], r["pg"]["iterations"], ref["iterations"],
             r["n_rejected"], int(ref["rejected"].sum()), r["pg"]["cg_iterations"], d_xy, d_th, dw, r["pg"]["cost_initial"],
             r["pg"]["cost_final"], ref["cost_final"]))
    assert r["pg"]["status"] == 0 and r["pg"]["converged"] == 1 and r["n_robust"] == int(rb.sum())
    assert abs(r["mu0"] - ref["mu0"]) <= MU0_RTOL * ref["mu0"]
    assert (r["levels"], r["pg"]["iterations"], r["n_rejected"]) == (ref["levels"], ref["iterations"], int(ref["rejected"].sum()))
    assert ((rb & (c > phi)) == ref["rejected"]).all() and (ref["rejected"][rb] == bad[rb]).all()
    assert d_xy <= POSE_TOL and d_th <= POSE_TOL
    assert dw <= WEIGHT_TOL and (w[~rb] == 1.0).all()
    assert np.allclose(c, ref["chi2"], rtol=1e-5, atol=1e-9)
    assert abs(r["pg"]["cost_initial"] - ref["cost_initial"]) <= 1e-12 * ref["cost_initial"]
    assert abs(r["pg"]["cost_final"] - ref["cost_final"]) <= 1e-6 * ref["cost_final"] + 1e-12
    assert got[0].tobytes() == poses[0].tobytes()


def test_given_mu0_is_taken_and_one_means_no_schedule(gpu):
    """mu0 = 1: one level, and on this drifted case a true arc is rejected, as the oracle says -- what the schedule is for."""
    poses, edges, phi, bad = R.drifted(24, 2, 1.0, R.loop_sets(24)[1], [R.false_arc(24)])
    ref = R.oracle_optimize_robust(poses, edges, phi, mu0=1.0, eps_step=R.CMP_EPS_STEP)
    assert R.smallest_margin(ref) >= R.MARGIN_MIN and min(ref["margins"]["trial_f"]) >= R.TRIAL_F_MIN and (ref["rejected"] & ~bad).any()
    (got, r, w, c), = solve(gpu, [(poses, edges, phi)], mu0=1.0)
    assert (r["mu0"], r["levels"], r["pg"]["iterations"], r["pg"]["converged"]) == (1.0, 1, ref["iterations"], 1)
    assert ((phi > 0) & (c > phi)).tolist() == ref["rejected"].tolist() and H.pose_error(got, ref["poses"]) <= (POSE_TOL, POSE_TOL)
    (_, r, _, _), = solve(gpu, [(poses, edges, phi)], mu0=500.0, factor=2.0, level_iter=1)
    ref = R.oracle_optimize_robust(poses, edges, phi, mu0=500.0, factor=2.0, level_iter=1, eps_step=R.CMP_EPS_STEP)
    assert r["mu0"] == 500.0 and r["levels"] == ref["levels"] == 10          # 500 / 2^9 < 1


# ------------------------------------------------------------------------------------------ 3: independence
def bad_phi(value):
    poses, edges, phi = workload("d24a")
    f = np.array(phi)
    f[len(f) - 2] = value
    return poses, edges, f


def test_independence(gpu):
    graphs = [workload("d24a"), bad_phi(-1.0), workload("two"), workload("four"), workload("d257")]
    batch = solve(gpu, graphs)
    assert [int(r["pg"]["status"]) for _, r, _, _ in batch] == [0, -1, 0, 0, 0]
    for g in range(len(graphs)):
        solo, = solve(gpu, [graphs[g]])
        assert same(batch[g], solo), g
    again, rev, dev = solve(gpu, graphs), solve(gpu, graphs[::-1])[::-1], solve_dev(gpu, graphs)
    for g in range(len(graphs)):
        assert same(batch[g], again[g]), g
        assert same(batch[g], rev[g]), g
        assert same(batch[g], dev[g]), g
    # a batch whose offsets do not start at zero: the graphs' own ranges alone are read and written
    capi, ctx = gpu
    poses, no, edges, eo, phi = R.pack_robust(graphs)
    out, res, w, c = capi.optimize_pose_graphs_robust(ctx, poses, no[2:], edges, eo[2:], phi, params(capi))
    assert out[:int(no[2])].tobytes() == poses[:int(no[2])].tobytes() and not w[:int(eo[2])].any() and not c[:int(eo[2])].any()
    for k, g in enumerate(range(2, len(graphs))):
        assert same(batch[g], (out[int(no[g]):int(no[g + 1])], res[k], w[int(eo[g]):int(eo[g + 1])], c[int(eo[g]):int(eo[g + 1])])), g


# ------------------------------------------------------------------------------------------ 4: faults, refusals, caps
@pytest.mark.parametrize("value", [-1.0, -1e-300, float("nan"), float("inf"), float("-inf")])
def test_a_bad_phi_costs_its_graph_alone(gpu, value):
    good = workload("d24a")
    alone, = solve(gpu, [good])
    bad = bad_phi(value)
    a, (p, r, w, c), b = solve(gpu, [good, bad, good])
    assert r["pg"]["status"] == -1
    assert (r["pg"]["iterations"], r["pg"]["converged"], r["pg"]["cost_initial"], r["mu0"], r["levels"], r["n_robust"], r["n_rejected"]) == \
        (0, 0, 0.0, 0.0, 0, 0, 0)
    assert p.tobytes() == bad[0].tobytes() and not w.any() and not c.any() and len(w) == len(bad[1])
    assert same(a, alone) and same(b, alone)


def test_graphs_without_arcs_or_nodes(gpu):
    lone = (np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 500.0]]), np.zeros(0, H.PG_EDGE_DTYPE), np.zeros(0))
    none = (np.zeros((0, 3)), np.zeros(0, H.PG_EDGE_DTYPE), np.zeros(0))
    good = workload("four")
    a, b, c = solve(gpu, [lone, none, good])
    for p, r, w, _ in (a, b):
        assert (r["pg"]["status"], r["pg"]["converged"], r["pg"]["iterations"], r["mu0"], r["levels"], r["n_robust"]) == (0, 1, 0, 1.0, 1, 0)
        assert len(w) == 0
    assert a[0].tobytes() == lone[0].tobytes() and same(c, solve(gpu, [good])[0])


def test_synchronous_refusals(gpu):
    capi, ctx = gpu
    L = capi.lib()
    poses, no, edges, eo, phi = R.pack_robust([workload("four")])
    res = np.zeros(1, capi.PG_ROBUST_RESULT_DTYPE)
    before = poses.copy()

    def call(prm, dev, p=poses.ctypes.data, r=res.ctypes.data):
        ref = C.byref(prm) if prm is not None else None
        if dev:
            return L.ndt_pg_optimize_robust_batch_dev(ctx.h, p, no.ctypes.data, edges.ctypes.data, eo.ctypes.data, 1, None, ref, r, None, None, None)
        return L.ndt_pg_optimize_robust_batch(ctx.h, p, no.ctypes.data, edges.ctypes.data, eo.ctypes.data, 1, phi.ctypes.data, ref, r, None, None)

    nan = float("nan")
    for dev in (False, True):
        assert call(None, dev) == capi.NDT_E_ARG and call(capi.default_pg_robust_params(), dev, p=None) == capi.NDT_E_ARG
        assert call(capi.default_pg_robust_params(), dev, r=None) == capi.NDT_E_ARG
        for bad in (dict(mu0=0.5), dict(mu0=-1.0), dict(mu0=1.0000001e12), dict(mu0=nan), dict(factor=1.0), dict(factor=1.04), dict(factor=1.1e6),
                    dict(factor=nan), dict(eps_level=-1e-9), dict(eps_level=nan), dict(eps_level=float("inf")), dict(level_iter=0),
                    dict(level_iter=10001), dict(pg_max_iter=0), dict(pg_max_iter=10001), dict(pg_eps_step=-1.0), dict(pg_cg_rtol=1.0),
                    dict(pg_max_halvings=61), dict(pg_cg_max_iter=-1)):
            assert call(capi.default_pg_robust_params(**bad), dev) == capi.NDT_E_ARG, (dev, bad)
            assert "out of range" in capi.lib().ndt_last_error(ctx.h).decode()
    assert poses.tobytes() == before.tobytes() and not res["pg"]["iterations"][0] and not res["levels"][0]
    # the ends of every range are taken (host form; a tiny graph)
    for ok in (dict(mu0=1.0), dict(mu0=1e12), dict(factor=1.05), dict(factor=1e6), dict(eps_level=0.0), dict(level_iter=1), dict(level_iter=10000)):
        assert call(capi.default_pg_robust_params(**ok), False) == capi.NDT_OK, ok
    d = capi.default_pg_robust_params()
    ref = capi.default_pg_params()
    assert (d.pg.max_iter, d.mu0, d.factor, d.eps_level, d.level_iter) == (200, 0.0, 1.4, 1e-3, 3)
    assert (d.pg.eps_step, d.pg.cg_max_iter, d.pg.cg_rtol, d.pg.max_halvings) == (ref.eps_step, ref.cg_max_iter, ref.cg_rtol, ref.max_halvings)
    assert C.sizeof(capi.PgRobustParams) == 72 and capi.PG_ROBUST_RESULT_DTYPE.itemsize == 56


@pytest.mark.parametrize("name, short", [("d24a", 1), ("d65b", 1), ("d24a", 40)])
def test_max_iter_bounds_the_trips_of_all_levels(gpu, name, short):
    """max_iter below the oracle's trip count: converged = 0 and the poses are the oracle's iterate behind that trip."""
    poses, edges, phi, _, ref = R.robust_workload(name)
    cap = ref["trips"] - short
    (got, r, w, c), = solve(gpu, [(poses, edges, phi)], pg_max_iter=cap)
    want = ref["iterates"][cap - 1]
    n_acc = sum(ref["accepted"][:cap])
    print("pg robust cap %s: max_iter %d of %d trips | steps %d (oracle %d) levels %d | d %s" % (name, cap, ref["trips"], r["pg"]["iterations"],
                                                                                             n_acc, r["levels"], H.pose_error(got, want)))
    assert r["pg"]["status"] == 0 and r["pg"]["converged"] == 0 and r["pg"]["iterations"] == n_acc
    assert H.pose_error(got, want) <= (POSE_TOL, POSE_TOL)
    x = np.array(got)
    x[:, 2] *= H.DEG
    assert abs(r["pg"]["cost_final"] - R.cost_mu(x, edges, phi, 1.0)) <= 1e-9 * r["pg"]["cost_final"]      # F_1, also from inside a level


def test_a_component_held_by_a_rejected_arc_alone_ends(gpu):
    """Three more nodes whose only tie to node 0's component is a gross robust arc: once its weight is below the pivot floor the
    chain matrix is not positive definite and the run ends by the rules -- finite poses, a consistent record, neighbours alone."""
    poses, edges, phi = workload("d24a")
    p = np.vstack([poses, [[1.0, 1.0, 10.0], [2.0, 1.0, 20.0], [3.0, 2.0, 30.0]]])
    e = np.concatenate([edges, H.make_edges([(24, 25, [1.0, 0.0, 10.0], H.OMEGA_ODO), (25, 26, [1.0, 0.5, 10.0], H.OMEGA_ODO),
                                             (3, 24, [40.0, -30.0, 120.0], H.OMEGA_LOOP)])])
    f = np.concatenate([phi, [0.0, 0.0, R.PHI]])
    good = workload("four")
    (got, r, w, c), other = solve(gpu, [(p, e, f), good])
    print("pg robust held by a rejected arc: %s weights %s" % (r, w[f > 0]))
    assert r["pg"]["status"] == 0 and r["pg"]["converged"] in (0, 1) and np.isfinite(got).all() and np.isfinite(w).all() and np.isfinite(c).all()
    assert 0 <= r["pg"]["iterations"] <= 200 and 1 <= r["levels"] <= 201 and r["n_robust"] == int((f > 0).sum())
    assert r["n_rejected"] == int(((f > 0) & (c > f)).sum()) and got[0].tobytes() == p[0].tobytes()
    assert ((w > 0) & (w <= 1.0)).all() and (w[f == 0] == 1.0).all()
    x = np.array(got)
    x[:, 2] *= H.DEG
    assert abs(r["pg"]["cost_final"] - R.cost_mu(x, e, f, 1.0)) <= 1e-9 * r["pg"]["cost_final"]
    assert same(other, solve(gpu, [good])[0])


# ------------------------------------------------------------------------------------------ 5: a resident set
def test_a_forged_loop_no_longer_bends_a_resident_set(gpu):
    """Two resident sessions of ten steps; each trajectory's graph (replay.loops_graph) gets one forged arc between scan 1 and
    the last scan that puts the last scan 25 m and 120 degrees from where it is.  The robust call rejects it, robust_keep keeps
    neither graph, and correct() with the robust poses all the same leaves the trajectories where they were; the plain
    optimiser on the same graphs moves them by metres.  The bound: the rejected arc keeps the weight (phi / c)^2 with c about
    2500 * 25^2, so it still pulls with 3e-11 * 2500 * 25 = 2e-6 N-like units on a chain of nine arcs of stiffness 100 each: about
    2e-7 m, below 1e-6."""
    capi, ctx = gpu
    from ndt_slam_amd import replay
    import session_workloads as W
    from session_helpers import lockstep, session_logs
    logs = session_logs(((33, 10), (34, 10)))
    ses = capi.Sessions(ctx, 2, capi.session_params_from_launch(W.launch_params(sepThre=1.5)))
    try:
        for k, scans, odo, act in lockstep(logs):
            ses.step(scans, odo, act)
        trajs = [ses.trajectory(i)[0].copy() for i in range(2)]
        odo_info = (100.0, 0.0, 0.0, 100.0, 0.0, 400.0)
        graphs = []
        for t in trajs:
            forged = np.zeros(1, dtype=capi.PG_EDGE_DTYPE)[0]
            forged["from"], forged["to"] = 1, len(t) - 1
            forged["rel"] = H.compose(H.between(t[1], t[-1]), np.array([20.0, -15.0, 120.0]))
            forged["info"] = H.info6(H.OMEGA_LOOP)
            graphs.append(replay.loops_graph(t, [forged], odo_info))
        no = np.array([0, len(trajs[0]), len(trajs[0]) + len(trajs[1])], dtype=np.uint64)
        eo = np.array([0, len(graphs[0]), len(graphs[0]) + len(graphs[1])], dtype=np.uint64)
        phi = np.zeros(int(eo[2]))
        phi[int(eo[1]) - 1] = phi[int(eo[2]) - 1] = R.PHI
        new, res, w, c = capi.optimize_pose_graphs_robust(ctx, np.concatenate(trajs), no, np.concatenate(graphs), eo, phi)
        plain, pres = capi.optimize_pose_graphs(ctx, np.concatenate(trajs), no, np.concatenate(graphs), eo)
        moved = [float(np.abs(plain[int(no[g]):int(no[g + 1]), :2] - trajs[g][:, :2]).max()) for g in range(2)]
        stayed = [float(np.abs(new[int(no[g]):int(no[g + 1]), :2] - trajs[g][:, :2]).max()) for g in range(2)]
        print("pg robust resident: %s | weights of the forged arcs %s chi2 %s | moved by: robust %s m, plain %s m"
              % (res, w[phi > 0], c[phi > 0], stayed, moved))
        assert (res["pg"]["status"] == 0).all() and (res["pg"]["converged"] == 1).all() and res["n_rejected"].tolist() == [1, 1]
        assert (c[phi > 0] > phi[phi > 0]).all() and (w[phi > 0] < 1e-9).all() and (w[phi == 0] == 1.0).all()
        assert replay.robust_keep(res, c, phi, eo).tolist() == [False, False]
        assert ses.correct({g: new[int(no[g]):int(no[g + 1])] for g in range(2)}) == {0: capi.NDT_OK, 1: capi.NDT_OK}
        for g in range(2):
            after = ses.trajectory(g)[0]
            assert H.pose_error(after, trajs[g]) <= (1e-6, 1e-6), (g, H.pose_error(after, trajs[g]))
            assert pres[g]["status"] == 0 and moved[g] > 0.1
    finally:
        ses.close()
