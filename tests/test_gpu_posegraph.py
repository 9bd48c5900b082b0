"""ndt_pg_optimize_batch* and ndt_repose_points* on the device against the numpy restatements of tests/pg_helpers.py: the
smallest graphs, parity with the dense oracle at the wave and workgroup boundaries, independence of the batch, the per-graph
faults and the caps, re-posing at the block boundaries and two world offsets, a short run of sessions closed by one loop arc,
the step rule iterate by iterate from far starts against the halving oracle, and graphs of other shapes (a free hub, many arcs,
information over six decades, a world offset)."""
import ctypes as C

import numpy as np
import pytest

import pg_helpers as H
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

PARITY_KEYS = [("eight", n) for n in H.EIGHT_SIZES] + [("star", 40), ("star", 120), ("shuffled", 40), ("shuffled", 120),
                                                        ("duplicate", 24), ("reversed", 65)]
POSE_TOL = 1e-8                                       # metres and radians: the bound the issue derives (see test_parity)


def solve(gpu, graphs, **prm):
    """One host-form call -> [(poses, record)] per graph."""
    capi, ctx = gpu
    poses, no, edges, eo = H.pack(graphs)
    out, res = capi.optimize_pose_graphs(ctx, poses, no, edges, eo, capi.default_pg_params(**prm))
    return [(out[int(no[g]):int(no[g + 1])], res[g]) for g in range(len(graphs))]


def solve_dev(gpu, graphs, **prm):
    """The same through ndt_pg_optimize_batch_dev, the arrays in torch tensors."""
    import torch
    capi, ctx = gpu
    poses, no, edges, eo = H.pack(graphs)
    dev = torch.device("cuda", 0)
    d_p = torch.from_numpy(poses.reshape(-1).copy() if poses.size else np.zeros(3)).to(dev)
    d_e = torch.from_numpy((edges if edges.size else np.zeros(1, H.PG_EDGE_DTYPE)).view(np.uint8).copy()).to(dev)
    d_r = torch.zeros(len(graphs) * capi.PG_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()                          # (the context works on a stream of its own)
    capi.optimize_pose_graphs_dev(ctx, d_p.data_ptr(), no, d_e.data_ptr(), eo, d_r.data_ptr(), capi.default_pg_params(**prm))
    torch.cuda.synchronize()
    out = d_p.cpu().numpy().reshape(-1, 3)
    res = np.frombuffer(d_r.cpu().numpy().tobytes(), dtype=capi.PG_RESULT_DTYPE)
    return [(out[int(no[g]):int(no[g + 1])], res[g]) for g in range(len(graphs))]


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ------------------------------------------------------------------------------------------ 1: the smallest graphs
def test_two_nodes_one_arc(gpu):
    capi, _ = gpu
    p0 = np.array([-1003.3, 707.1, 170.0])
    rel = np.array([1.5, -0.25, 25.0])                                  # the heading of node 1 crosses 180
    poses = np.array([p0, [-1000.0, 700.0, 3.0]])
    edges = H.make_edges([(0, 1, rel, H.OMEGA_ODO)])
    want = H.compose(p0, rel)
    (got, r), = solve(gpu, [(poses, edges)], max_iter=1)
    assert (r["status"], r["iterations"], r["converged"]) == (0, 1, 0), r
    assert np.abs(got[1, :2] - want[:2]).max() <= 1e-11 and abs(H.wrap_deg(got[1, 2] - want[2])) <= 1e-11, (got, want)
    assert -180 <= got[1, 2] < 180
    assert got[0].tobytes() == p0.tobytes()
    assert r["cost_final"] <= 1e-18 * r["cost_initial"]
    (got2, r2), = solve(gpu, [(poses, edges)])
    assert r2["converged"] == 1 and r2["iterations"] <= 2, r2
    assert H.pose_error(got2, np.array([p0, want])) <= (1e-11, 1e-11)
    # the arc stored the other way round
    (got3, r3), = solve(gpu, [(poses, H.make_edges([(1, 0, H.inverse(rel), H.OMEGA_ODO)]))])
    assert r3["converged"] == 1 and H.pose_error(got3, np.array([p0, want])) <= (1e-10, 1e-10), (got3, want)


def test_three_nodes_consistent(gpu):
    capi, _ = gpu
    poses = np.array([[1.0, 2.0, -175.0], [1.8, 2.3, 178.0], [2.9, 2.2, -160.0]])
    edges = H.make_edges([(0, 1, H.between(poses[0], poses[1]), H.OMEGA_ODO), (1, 2, H.between(poses[1], poses[2]), H.OMEGA_ODO),
                          (2, 0, H.between(poses[2], poses[0]), H.OMEGA_LOOP)])
    (got, r), = solve(gpu, [(poses, edges)])
    assert r["status"] == 0 and r["converged"] == 1, r
    assert H.pose_error(got, poses) < (1e-9, 1e-9)                      # eps_step
    assert r["cost_final"] <= r["cost_initial"] <= 1e-20
    assert got[0].tobytes() == poses[0].tobytes()


def test_four_nodes_one_loop(gpu):
    poses, edges, ref = H.workload(("eight", 4))
    edges = edges[:4]                                                   # the chain and its first loop arc (3 -> 0)
    ref = H.oracle_optimize(poses, edges)
    (got, r), = solve(gpu, [(poses, edges)])
    assert r["status"] == 0 and r["converged"] == 1, r
    assert H.pose_error(got, ref["poses"]) <= (POSE_TOL, POSE_TOL)
    assert r["iterations"] <= H.iterations_at(ref, 1e-9) + 1
    assert abs(r["cost_final"] - ref["costs"][-1]) <= 1e-9 * ref["costs"][-1]


# ------------------------------------------------------------------------------------------ 2: parity
@pytest.fixture(scope="module")
def parity_run(gpu):
    """Every parity workload in ONE call (they do not see each other: test_independence)."""
    graphs = [H.workload(k)[:2] for k in PARITY_KEYS]
    return dict(zip(PARITY_KEYS, solve(gpu, graphs)))


@pytest.mark.parametrize("key", PARITY_KEYS, ids=lambda k: "%s%d" % k)
def test_parity(parity_run, key):
    """Within 1e-8 m / 1e-8 rad of the oracle run to 1e-12: a contracting Newton iteration that stops at a step below 1e-9 is
    within 1e-9 of the minimiser, the linear solves at 1e-10 add less, 10x margin is left."""
    poses, edges, ref = H.workload(key)
    got, r = parity_run[key]
    d_xy, d_th = H.pose_error(got, ref["poses"])
    want_it = H.iterations_at(ref, 1e-9)
    rel_cost = abs(r["cost_final"] - ref["costs"][-1]) / ref["costs"][-1]
    print("pg parity %s%d: N %d E %d | d_xy %.3g m d_th %.3g rad | iterations %d (oracle %d) cg %d | cost %.6g -> %.12g rel %.3g"
          % (key[0], key[1], len(poses), len(edges), d_xy, d_th, r["iterations"], want_it, r["cg_iterations"], r["cost_initial"],
             r["cost_final"], rel_cost))
    assert r["status"] == 0 and r["converged"] == 1, r
    assert d_xy <= POSE_TOL and d_th <= POSE_TOL, (d_xy, d_th)
    assert r["iterations"] <= want_it + 1, (r["iterations"], want_it)
    assert rel_cost <= 1e-9, rel_cost
    assert r["cost_final"] <= r["cost_initial"]
    assert abs(r["cost_initial"] - ref["costs"][0]) <= 1e-12 * ref["costs"][0]
    assert got[0].tobytes() == poses[0].tobytes()
    assert (got[:, 2] >= -180).all() and (got[:, 2] < 180).all()
    assert r["cg_iterations"] <= r["iterations"] * 6 * len(poses) + 6 * len(poses)


# ------------------------------------------------------------------------------------------ 3: independence
def invalid_graph():
    poses, edges, _ = H.workload(("eight", 24))
    e = edges.copy()
    e[7]["to"] = 24                                                     # outside the graph
    return np.array(poses), e


def test_independence(gpu):
    two = (np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 5.0]]), H.make_edges([(0, 1, [1.1, 0.0, 4.0], H.OMEGA_ODO)]))
    graphs = [H.workload(("eight", 24))[:2], invalid_graph(), two, H.workload(("star", 40))[:2], H.workload(("eight", 257))[:2]]
    batch = solve(gpu, graphs)
    assert [int(r["status"]) for _, r in batch] == [0, -1, 0, 0, 0]
    assert batch[1][0].tobytes() == graphs[1][0].tobytes()
    for g in range(len(graphs)):
        solo, = solve(gpu, [graphs[g]])
        assert same(batch[g], solo), g
    again, rev, dev = solve(gpu, graphs), solve(gpu, graphs[::-1])[::-1], solve_dev(gpu, graphs)
    for g in range(len(graphs)):
        assert same(batch[g], again[g]), g
        assert same(batch[g], rev[g]), g
        assert same(batch[g], dev[g]), g
    # a batch whose offsets do not start at zero (host form: the graphs' own ranges alone are read and written)
    capi, ctx = gpu
    poses, no, edges, eo = H.pack(graphs)
    out, res = capi.optimize_pose_graphs(ctx, poses, no[2:], edges, eo[2:])
    assert out[:int(no[2])].tobytes() == poses[:int(no[2])].tobytes()
    for k, g in enumerate(range(2, len(graphs))):
        assert out[int(no[g]):int(no[g + 1])].tobytes() == batch[g][0].tobytes() and res[k].tobytes() == batch[g][1].tobytes()


# ------------------------------------------------------------------------------------------ 4: faults and caps
def _faults():
    poses, edges, _ = H.workload(("eight", 24))
    out = {}
    for name in ("from_low", "to_high", "self_arc", "nan_pose", "inf_pose0", "nan_rel", "inf_info", "info_not_pd", "info_zero", "info_minor"):
        p, e = np.array(poses), edges.copy()
        if name == "from_low":
            e[3]["from"] = -1
        elif name == "to_high":
            e[len(e) - 1]["to"] = 24
        elif name == "self_arc":
            e[5]["to"] = e[5]["from"]
        elif name == "nan_pose":
            p[13, 1] = np.nan
        elif name == "inf_pose0":
            p[0, 2] = np.inf
        elif name == "nan_rel":
            e[0]["rel"][2] = np.nan
        elif name == "inf_info":
            e[20]["info"][5] = np.inf
        elif name == "info_not_pd":
            e[9]["info"] = H.info6(np.diag([400.0, -1.0, 900.0]))
        elif name == "info_zero":
            e[9]["info"] = 0.0
        elif name == "info_minor":
            e[9]["info"] = H.info6([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
        out[name] = (p, e)
    return out


def test_per_graph_faults(gpu):
    good = H.workload(("eight", 24))[:2]
    alone, = solve(gpu, [good])
    faults = _faults()
    graphs = []
    for name in faults:
        graphs += [faults[name], good]
    got = solve(gpu, graphs)
    for k, name in enumerate(faults):
        p, r = got[2 * k]
        assert r["status"] == -1 and r["iterations"] == 0 and r["converged"] == 0, (name, r)
        assert p.tobytes() == faults[name][0].tobytes(), name
        assert same(got[2 * k + 1], alone), name                         # the neighbour is not disturbed
    # no arcs: NDT_OK, converged, untouched; so is a graph without nodes
    lone = (np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 500.0]]), np.zeros(0, H.PG_EDGE_DTYPE))
    none = (np.zeros((0, 3)), np.zeros(0, H.PG_EDGE_DTYPE))
    a, b, c = solve(gpu, [lone, none, good])
    for p, r in (a, b):
        assert (r["status"], r["converged"], r["iterations"], r["cg_iterations"]) == (0, 1, 0, 0), r
    assert a[0].tobytes() == lone[0].tobytes() and same(c, alone)


def test_disconnected_graph_ends(gpu):
    poses, edges, _ = H.workload(("eight", 24))
    p = np.vstack([poses, [[1.0, 1.0, 10.0], [2.0, 1.0, 20.0], [3.0, 2.0, 30.0]]])
    e = np.concatenate([edges, H.make_edges([(24, 25, [1.0, 0.0, 10.0], H.OMEGA_ODO), (25, 26, [1.0, 0.5, 10.0], H.OMEGA_ODO)])])
    good = H.workload(("eight", 24))[:2]
    (got, r), other = solve(gpu, [(p, e), good])
    assert r["status"] == 0 and r["converged"] == 0, r
    assert np.isfinite(got).all() and r["cost_final"] <= r["cost_initial"]
    assert got[0].tobytes() == p[0].tobytes()
    assert same(other, solve(gpu, [good])[0])
    # the same with the free nodes in the middle of the numbering
    new_of = np.concatenate([np.arange(10), np.arange(10, 24) + 3, [10, 11, 12]])
    p2 = np.empty_like(p)
    p2[new_of] = p
    e2 = e.copy()
    e2["from"], e2["to"] = new_of[e["from"]], new_of[e["to"]]
    (got2, r2), = solve(gpu, [(p2, e2)])
    assert r2["status"] == 0 and r2["converged"] == 0 and np.isfinite(got2).all() and r2["cost_final"] <= r2["cost_initial"], r2


def test_caps(gpu):
    poses, edges, ref = H.workload(("eight", 24))
    (got, r), = solve(gpu, [(poses, edges)], max_iter=1)
    assert (r["iterations"], r["converged"], r["status"]) == (1, 0, 0), r
    assert r["cost_final"] < r["cost_initial"]
    assert abs(H.cost_deg(got, edges) - r["cost_final"]) <= 1e-9 * r["cost_final"]
    assert got[0].tobytes() == poses[0].tobytes()
    sp, se, _ = H.workload(("shuffled", 120))
    (got, r), = solve(gpu, [(sp, se)], cg_max_iter=1)
    assert r["status"] == 0 and r["cost_final"] <= r["cost_initial"], r
    assert r["cg_iterations"] <= 20 and np.isfinite(got).all()
    assert got[0].tobytes() == sp[0].tobytes()
    (got, r), = solve(gpu, [(sp, se)], max_halvings=0)
    assert r["status"] == 0 and r["converged"] == 1 and H.pose_error(got, H.workload(("shuffled", 120))[2]["poses"]) <= (POSE_TOL, POSE_TOL)


def test_synchronous_refusals(gpu):
    capi, ctx = gpu
    L = capi.lib()
    poses, no, edges, eo = H.pack([H.workload(("eight", 24))[:2]])
    res = np.zeros(1, capi.PG_RESULT_DTYPE)
    ok = capi.default_pg_params()
    before = poses.copy()

    def call(p=poses.ctypes.data, n=no.ctypes.data, e=edges.ctypes.data, o=eo.ctypes.data, G=1, prm=ok, r=res.ctypes.data, dev=False):
        if dev:
            return L.ndt_pg_optimize_batch_dev(ctx.h, p, n, e, o, G, C.byref(prm) if prm is not None else None, r, None)
        return L.ndt_pg_optimize_batch(ctx.h, p, n, e, o, G, C.byref(prm) if prm is not None else None, r)

    for dev in (False, True):
        for kw in (dict(p=None), dict(n=None), dict(e=None), dict(o=None), dict(prm=None), dict(r=None), dict(G=0), dict(G=-3)):
            assert call(dev=dev, **kw) == capi.NDT_E_ARG, (dev, kw)
        down = np.array([5, 2], np.uint64)
        assert call(n=down.ctypes.data, dev=dev) == capi.NDT_E_ARG
        assert call(o=down.ctypes.data, dev=dev) == capi.NDT_E_ARG
        for bad in (dict(max_iter=0), dict(max_iter=10001), dict(eps_step=-1.0), dict(eps_step=float("nan")), dict(cg_max_iter=-1),
                    dict(cg_rtol=0.0), dict(cg_rtol=1.0), dict(cg_rtol=float("nan")), dict(max_halvings=-1), dict(max_halvings=61)):
            assert call(prm=capi.default_pg_params(**bad), dev=dev) == capi.NDT_E_ARG, (dev, bad)
    assert poses.tobytes() == before.tobytes() and not res["iterations"][0]
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
    assert call() == 0 and res["converged"][0] == 1
    # re-posing
    xy, off, pz = np.zeros((4, 2), np.float32), np.array([0, 4], np.uint64), np.zeros((1, 3))

    def rp(x=xy.ctypes.data, s=8, o=off.ctypes.data, K=1, a=pz.ctypes.data, b=pz.ctypes.data, out=xy.ctypes.data, so=8, dev=False):
        if dev:
            return L.ndt_repose_points_dev(ctx.h, x, s, o, K, a, b, out, so, None)
        return L.ndt_repose_points(ctx.h, x, s, o, K, a, b, out, so)

    for dev in (False, True):
        for kw in (dict(x=None), dict(o=None), dict(a=None), dict(b=None), dict(out=None), dict(K=0), dict(s=4), dict(s=10), dict(so=6),
                   dict(so=16)):                                         # (out == xy at another stride)
            assert rp(dev=dev, **kw) == capi.NDT_E_ARG, (dev, kw)
    down = np.array([3, 1], np.uint64)
    assert rp(o=down.ctypes.data) == capi.NDT_E_ARG


# ------------------------------------------------------------------------------------------ 5: re-posing
SEG_SIZES = (0, 1, 255, 256, 257, 0, 700)


def repose_case(offset, seed):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(SEG_SIZES)]).astype(np.uint64)
    n = int(off[-1])
    xy = (rng.uniform(-30.0, 30.0, (n, 2)) + np.asarray(offset)).astype(np.float32)
    K = len(SEG_SIZES)
    old = np.stack([offset[0] + rng.uniform(-5, 5, K), offset[1] + rng.uniform(-5, 5, K), rng.uniform(-180, 180, K)], axis=1)
    new = old + np.stack([rng.normal(0, 0.3, K), rng.normal(0, 0.3, K), rng.normal(0, 2.0, K)], axis=1)
    new[:, 2] = H.wrap_deg(new[:, 2])
    new[3] = old[3]                                                      # the 256-point segment: bit-equal poses
    return xy, off, old, new


def ulps32(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def check_reposed(got, want, what):
    d = ulps32(np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1))
    n_diff = int((d != 0).sum())
    print("repose %s: %d coordinates, %d not bit-equal, largest distance %d ulp" % (what, d.size, n_diff, int(d.max()) if d.size else 0))
    assert d.max() <= 1, (what, int(d.max()))
    assert n_diff * 10000 <= d.size, (what, n_diff, d.size)


@pytest.mark.parametrize("offset", [(-1003.3, 707.1), (8191.7, 8191.7)], ids=["offset_a", "offset_b"])
def test_repose_against_the_restatement(gpu, offset):
    import torch
    capi, ctx = gpu
    xy, off, old, new = repose_case(offset, 77)
    want = H.repose_ref(xy, off, old, new)
    a, b = int(off[3]), int(off[4])
    assert want[a:b].tobytes() == xy[a:b].tobytes() and want[:a].tobytes() != xy[:a].tobytes()
    # host form, stride 8, out of place and in place
    got = capi.repose_points(ctx, xy, off, old, new)
    check_reposed(got, want, "host 8")
    assert got[a:b].tobytes() == xy[a:b].tobytes()
    inpl = xy.copy()
    assert capi.repose_points(ctx, inpl, off, old, new, out=inpl) is inpl and inpl.tobytes() == got.tobytes()
    # host form, stride 16 in and out: the other eight bytes of a row stay
    wide = np.full((len(xy), 4), 7.5, np.float32)
    wide[:, :2] = xy
    outw = np.full((len(xy), 4), -3.25, np.float32)
    capi.repose_points(ctx, wide, off, old, new, out=outw)
    assert outw[:, :2].tobytes() == got.tobytes() and (outw[:, 2:] == -3.25).all()
    # device form: stride 16 -> 8 out of place, then stride 16 in place
    dev = torch.device("cuda", 0)
    d_in, d_out = torch.from_numpy(wide).to(dev), torch.zeros((len(xy), 2), dtype=torch.float32, device=dev)
    d_off, d_old, d_new = torch.from_numpy(off.astype(np.int64)).to(dev), torch.from_numpy(old).to(dev), torch.from_numpy(new).to(dev)
    torch.cuda.synchronize()
    capi.repose_points_dev(ctx, d_in.data_ptr(), 16, d_off.data_ptr(), len(SEG_SIZES), d_old.data_ptr(), d_new.data_ptr(), d_out.data_ptr(), 8)
    capi.repose_points_dev(ctx, d_in.data_ptr(), 16, d_off.data_ptr(), len(SEG_SIZES), d_old.data_ptr(), d_new.data_ptr(), d_in.data_ptr(), 16)
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == got.tobytes()
    back = d_in.cpu().numpy()
    assert back[:, :2].tobytes() == got.tobytes() and (back[:, 2:] == 7.5).all()
    # a segment range that does not start at zero (host form): the points in front stay
    part = capi.repose_points(ctx, xy, off[2:], old[2:], new[2:])
    assert part[:int(off[2])].tobytes() == xy[:int(off[2])].tobytes() and part[int(off[2]):].tobytes() == got[int(off[2]):].tobytes()


# ------------------------------------------------------------------------------------------ 6: with sessions
def test_sessions_odometry_arcs_loop_arc_and_reposed_map(gpu):
    from ndt_slam_amd import replay
    from session_helpers import lockstep, session_logs
    capi, ctx = gpu
    p = dict(replay.LAUNCH_PARAMS, sepThre=2.5)
    logs = session_logs(((33, 14), (34, 9), (35, 12), (36, 7), (37, 10)))      # (tests/test_gpu_sessions.py: some of them split)
    ses = capi.Sessions(ctx, len(logs), capi.session_params_from_launch(p))
    recs = [[] for _ in logs]
    for k, scans, odo, act in lockstep(logs):
        out = ses.step(scans, odo, act)
        for i in range(len(logs)):
            if out[i]["stepped"]:
                recs[i].append(out[i].copy())
    fallback = H.info6(H.OMEGA_ODO)                                       # the caller's, where a covariance is refused
    graphs, n_cov = [], 0
    for i in range(len(logs)):
        poses = np.array([r["pose"] for r in recs[i]])
        e = np.zeros(len(poses) - 1, capi.PG_EDGE_DTYPE)
        for k in range(len(poses) - 1):
            e[k]["from"], e[k]["to"] = k, k + 1
            e[k]["rel"] = capi.pg_edge_between(poses[k], poses[k + 1])
            try:
                e[k]["info"] = capi.pg_info_from_cov(recs[i][k + 1]["cov"].reshape(3, 3), poses[k][2])
                n_cov += 1
            except capi.NdtError:
                e[k]["info"] = fallback
        graphs.append((poses, e))
    print("sessions: %d of %d arcs take their information from the step records' covariances" % (n_cov, sum(len(e) for _, e in graphs)))
    # the arc-only graphs are consistent: nothing moves
    for (poses, e), (got, r) in zip(graphs, solve(gpu, graphs)):
        assert r["status"] == 0 and r["converged"] == 1, r
        assert H.pose_error(got, poses) < (1e-9, 1e-9)
    # one loop arc on the session with the most submaps that moves its last pose: last -> first, the first pose as seen from
    # the last, disturbed
    s0 = max(range(len(logs)), key=lambda i: int(recs[i][-1]["submap"]))
    poses, e = graphs[s0]
    n = len(poses)
    loop = np.zeros(1, capi.PG_EDGE_DTYPE)
    loop[0]["from"], loop[0]["to"] = n - 1, 0
    loop[0]["rel"] = H.between(poses[n - 1], poses[0]) + np.array([0.25, -0.15, 2.0])
    loop[0]["info"] = H.info6(H.OMEGA_LOOP)
    e2 = np.concatenate([e, loop])
    (new_poses, r), = solve(gpu, [(poses, e2)])
    ref = H.oracle_optimize(poses, e2)
    assert r["status"] == 0 and r["converged"] == 1 and r["cost_final"] < r["cost_initial"], r
    assert H.pose_error(new_poses, ref["poses"]) <= (POSE_TOL, POSE_TOL)
    assert np.abs(new_poses[n - 1, :2] - poses[n - 1, :2]).max() > 0.01
    # re-pose the session's global map by submap: a submap moves with the pose of its first scan
    cloud, parts = ses.global_map(s0)
    off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint64)
    first = [next(k for k, rec in enumerate(recs[s0]) if rec["submap"] == j) for j in range(len(parts))]
    assert len(parts) >= 2 and int(off[-1]) == len(cloud)
    old, new = poses[first], new_poses[first]
    assert old[0].tobytes() == new[0].tobytes()                          # node 0: the first submap keeps its bytes
    got = capi.repose_points(ctx, cloud, off, old, new)
    check_reposed(got, H.repose_ref(cloud, off, old, new), "sessions")
    assert got[:int(off[1])].tobytes() == cloud[:int(off[1])].tobytes() and got[int(off[1]):].tobytes() != cloud[int(off[1]):].tobytes()
    # the set's own resident state is not rewritten
    again, _ = ses.global_map(s0)
    assert again.tobytes() == cloud.tobytes()
    ses.close()


# ------------------------------------------------------------------------------------------ 7: the step rule, from far starts
FAR_NAMES = sorted(H.FAR_STARTS)
# The largest deviation of a compared iterate from the halving oracle's seen on an MI355X (m or rad; LOG R24.1 has every one).
# The decisions have margin (tests/test_pg_host.py), so the conjugate gradients' tolerance is the one source of a difference:
# factor 10 for it.  A wrong number of halvings moves the largest component by half the step at least, so the bound never
# exceeds 1e-3 of the step.
ITER_DEV = 2.7e-9


def iterate_bound(step):
    return min(10.0 * ITER_DEV, 1e-3 * step)


def gradient_l1(iterate, edges):
    x = np.array(iterate, np.float64)
    x[:, 2] *= H.DEG
    return float(np.abs(H.normal_equations(x, edges)[1][3:]).sum())


def check_iterate(got, r, ref, k, edges, what):
    """(got, r) against the oracle's k-th accepted iterate: the poses under iterate_bound, cost_final under what that bound
    allows (dF = 2 b^T dx, b the oracle's own gradient there) plus test_parity's 1e-9 of F.  -> (d_xy, d_th)."""
    want, step = ref["iterates"][k - 1], ref["steps"][k - 1]
    d_xy, d_th = H.pose_error(got, want)
    tol = iterate_bound(step)
    tol_f = 2.0 * gradient_l1(want, edges) * tol + 1e-9 * ref["costs"][k]
    print("pg %s step %d: |s d| %.3g halvings %d margin %.2g | d_xy %.3g m d_th %.3g rad (bound %.3g) | F %.9g oracle %.9g, diff %.3g (bound %.3g)"
          % (what, k, step, ref["halvings"][k - 1], ref["margins"][k - 1], d_xy, d_th, tol, r["cost_final"], ref["costs"][k],
             abs(r["cost_final"] - ref["costs"][k]), tol_f))
    assert r["status"] == 0 and r["iterations"] == k, (what, k, r)
    assert d_xy <= tol and d_th <= tol, (what, k, d_xy, d_th, tol)
    assert abs(r["cost_final"] - ref["costs"][k]) <= tol_f, (what, k, r["cost_final"], ref["costs"][k], tol_f)
    assert got[0].tobytes() == want[0].tobytes()
    assert (got[:, 2] >= -180).all() and (got[:, 2] < 180).all()
    return d_xy, d_th


@pytest.fixture(scope="module")
def far_runs(gpu):
    """{(name, k): (poses, record)} of every far-start workload with max_iter = k, k = 1 .. its compared steps (one call per k
    for all of them), and {(name, 0)}: with the defaults."""
    work = {n: H.far_workload(n) for n in FAR_NAMES}
    runs = {}
    for k in range(1, max(w[3] for w in work.values()) + 1):
        names = [n for n in FAR_NAMES if work[n][3] >= k]
        for n, res in zip(names, solve(gpu, [work[n][:2] for n in names], max_iter=k, max_halvings=8)):
            runs[n, k] = res
    for n, res in zip(FAR_NAMES, solve(gpu, [work[n][:2] for n in FAR_NAMES])):
        runs[n, 0] = res
    return runs


@pytest.mark.parametrize("name", FAR_NAMES)
def test_far_start_iterates(far_runs, name):
    """The k-th accepted iterate of the device is the halving oracle's, for every k whose step is longer than 1e-6: the same
    number of halvings at every step (the oracle's decisions have a margin of 1e-6 of F, the device evaluates F to 1e-13)."""
    poses, edges, ref, n_cmp = H.far_workload(name)
    dev_halvings, prev_got, prev_want = [], np.array(poses), np.array(poses)
    for k in range(1, n_cmp + 1):
        got, r = far_runs[name, k]
        check_iterate(got, r, ref, k, edges, name)
        assert r["converged"] == 0 and r["cost_initial"] == far_runs[name, 1][1]["cost_initial"], (k, r)
        assert r["cost_final"] <= r["cost_initial"]
        # the halvings the device took, read off the length of its step in x and y next to the oracle's
        want = ref["iterates"][k - 1]
        ratio = np.abs(want[:, :2] - prev_want[:, :2]).max() / np.abs(got[:, :2] - prev_got[:, :2]).max()
        dev_halvings.append(ref["halvings"][k - 1] + int(round(np.log2(ratio))))
        prev_got, prev_want = got, want
    print("pg %s halvings per step: device %s oracle %s" % (name, dev_halvings, ref["halvings"][:n_cmp]))
    assert dev_halvings == ref["halvings"][:n_cmp]
    assert abs(far_runs[name, 1][1]["cost_initial"] - ref["costs"][0]) <= 1e-12 * ref["costs"][0]
    # the whole run with the defaults
    got, r = far_runs[name, 0]
    want_it = H.iterations_at(ref, 1e-9)
    d_xy, d_th = H.pose_error(got, ref["poses"])
    print("pg %s defaults: d_xy %.3g m d_th %.3g rad | iterations %d (oracle %d at 1e-9, %d at 1e-12, ends: %s) cg %d | cost %.6g -> %.12g"
          % (name, d_xy, d_th, r["iterations"], want_it, len(ref["steps"]), ref["end"], r["cg_iterations"], r["cost_initial"], r["cost_final"]))
    assert r["status"] == 0 and r["converged"] == 1, r
    assert d_xy <= POSE_TOL and d_th <= POSE_TOL, (d_xy, d_th)
    assert n_cmp <= r["iterations"] <= want_it + 1, (r["iterations"], want_it)
    assert abs(r["cost_final"] - ref["costs"][-1]) <= 1e-9 * ref["costs"][-1]
    assert got[0].tobytes() == poses[0].tobytes()


@pytest.mark.parametrize("max_halvings, k", H.FAR_CAP_CASES)
def test_halving_cap_runs_out_above_eps_step(gpu, max_halvings, k):
    """Step k needs one halving more than allowed: the run ends there with converged = 0 and the poses of step k - 1."""
    poses, edges, ref, _ = H.far_workload(H.FAR_CAP_NAME)
    (got, r), = solve(gpu, [(poses, edges)], max_halvings=max_halvings)
    assert (r["status"], r["converged"], r["iterations"]) == (0, 0, k - 1), r
    check_iterate(got, r, ref, k - 1, edges, "%s max_halvings=%d" % (H.FAR_CAP_NAME, max_halvings))
    assert abs(H.cost_deg(got, edges) - r["cost_final"]) <= 1e-9 * r["cost_final"]
    assert got[0].tobytes() == poses[0].tobytes()


@pytest.mark.parametrize("name, max_halvings, eps_step, end, n_steps", H.FAR_COARSE_CASES)
def test_converged_is_judged_on_the_step_taken(gpu, name, max_halvings, eps_step, end, n_steps):
    """eps_step between the halved and the full length of a step: an accepted halved step below it ends the run converged, and
    so does a run-out whose last trial is below it; the poses are the oracle's iterate of that count."""
    poses, edges, ref, _ = H.far_workload(name)
    (got, r), = solve(gpu, [(poses, edges)], max_halvings=max_halvings, eps_step=eps_step)
    assert (r["status"], r["converged"], r["iterations"]) == (0, 1, n_steps), (end, r)
    check_iterate(got, r, ref, n_steps, edges, "%s eps_step=%g max_halvings=%d" % (name, eps_step, max_halvings))
    assert abs(H.cost_deg(got, edges) - r["cost_final"]) <= 1e-9 * r["cost_final"]


def test_independence_under_halving(gpu):
    graphs = [H.far_workload(n)[:2] for n in FAR_NAMES] + [H.workload(("eight", 24))[:2], invalid_graph()]
    for prm in ({}, dict(max_iter=3)):                                    # (the third step of far24a and far257 is halved twice)
        batch = solve(gpu, graphs, **prm)
        assert [int(r["status"]) for _, r in batch] == [0] * len(FAR_NAMES) + [0, -1]
        assert batch[-1][0].tobytes() == graphs[-1][0].tobytes()
        rev, dev = solve(gpu, graphs[::-1], **prm)[::-1], solve_dev(gpu, graphs, **prm)
        for g in range(len(graphs)):
            solo, = solve(gpu, [graphs[g]], **prm)
            assert same(batch[g], solo), (prm, g)
            assert same(batch[g], rev[g]), (prm, g)
            assert same(batch[g], dev[g]), (prm, g)


# ------------------------------------------------------------------------------------------ 8: other shapes
SHAPE_KEYS = sorted(H.SHAPE_WORKLOADS)
PERMUTED = ("dense24_", 129)

def permuted_arcs(key):
    poses, edges, _ = H.workload(key)
    return poses, edges[np.random.default_rng(17).permutation(len(edges))]


@pytest.fixture(scope="module")
def shape_run(gpu):
    """Every shape workload and one with its arc list permuted in ONE call with the defaults."""
    keys = SHAPE_KEYS + ["permuted"]
    graphs = [H.workload(k)[:2] for k in SHAPE_KEYS] + [permuted_arcs(PERMUTED)]
    return dict(zip(keys, solve(gpu, graphs)))


@pytest.mark.parametrize("key", SHAPE_KEYS, ids=lambda k: "%s%d" % k)
def test_shape_parity(shape_run, key):
    """test_parity's bound and assertions on a free node of degree N - 1, on key arrays at and around a power of two and far
    more arcs than nodes, and on information matrices over six decades (condition number of H 1e7 and 9e7: measured with the
    default cg_rtol they stay 1e4 below POSE_TOL, LOG R24.1, so they run with it like the others)."""
    poses, edges, ref = H.workload(key)
    got, r = shape_run[key]
    d_xy, d_th = H.pose_error(got, ref["poses"])
    want_it = H.iterations_at(ref, 1e-9)
    print("pg shape %s%d: N %d E %d | d_xy %.3g m d_th %.3g rad | iterations %d (oracle %d) cg %d converged %d | cost %.6g -> %.12g rel %.3g"
          % (key[0], key[1], len(poses), len(edges), d_xy, d_th, r["iterations"], want_it, r["cg_iterations"], r["converged"],
             r["cost_initial"], r["cost_final"], abs(r["cost_final"] - ref["costs"][-1]) / ref["costs"][-1]))
    assert r["status"] == 0 and r["converged"] == 1, r
    assert d_xy <= POSE_TOL and d_th <= POSE_TOL, (d_xy, d_th)
    assert r["iterations"] <= want_it + 1, (r["iterations"], want_it)
    assert abs(r["cost_final"] - ref["costs"][-1]) <= 1e-9 * ref["costs"][-1]
    assert r["cost_final"] <= r["cost_initial"]
    assert abs(r["cost_initial"] - ref["costs"][0]) <= 1e-12 * ref["costs"][0]
    assert got[0].tobytes() == poses[0].tobytes()
    assert (got[:, 2] >= -180).all() and (got[:, 2] < 180).all()
    assert r["cg_iterations"] <= r["iterations"] * 6 * len(poses) + 6 * len(poses)


def test_permuted_arc_list(shape_run):
    """The order of the arcs changes the order of every node's sums and nothing else: within POSE_TOL, not bit-equal."""
    (a, ra), (b, rb) = shape_run[PERMUTED], shape_run["permuted"]
    d_xy, d_th = H.pose_error(a, b)
    print("pg permuted arcs %s%d: d_xy %.3g m d_th %.3g rad | iterations %d / %d" % (PERMUTED + (d_xy, d_th, ra["iterations"], rb["iterations"])))
    assert rb["status"] == 0 and rb["converged"] == 1, rb
    assert d_xy <= POSE_TOL and d_th <= POSE_TOL, (d_xy, d_th)
    assert abs(ra["cost_final"] - rb["cost_final"]) <= 1e-9 * ra["cost_final"]


# ------------------------------------------------------------------------------------------ 9: a world offset and a rigid motion
WORLD_XY, WORLD_TURN = (8191.7, -8003.3), 137.0
WORLD_FACTOR = 8191.7 / 10.0                           # the figure-eight spans +-10 m about its node 0; moved, it lies 8.2 km out


@pytest.mark.parametrize("name", ["eight65", "far65"])
def test_rigid_motion_of_the_start(gpu, name):
    """The arcs are relative, so the minimiser moves with the start.  Bound: POSE_TOL times WORLD_FACTOR, the ratio of the
    coordinates' sizes (819): POSE_TOL rests on steps down to eps_step being decided by F, every coordinate difference in F is
    rounded at the size of the coordinates, so the rounding of F -- and with it the length of a step that F can no longer
    decide -- is at most that much larger."""
    poses, edges = H.workload(("eight", 65))[:2] if name == "eight65" else H.far_workload("far65")[:2]
    moved = H.rigid_move(poses, WORLD_XY, WORLD_TURN)
    (a, ra), (b, rb) = solve(gpu, [(poses, edges), (moved, edges)])
    factor = WORLD_FACTOR
    d_xy, d_th = H.pose_error(b, H.rigid_move(a, WORLD_XY, WORLD_TURN))
    print("pg rigid %s: factor %.0f bound %.3g | d_xy %.3g m d_th %.3g rad | iterations %d / %d converged %d / %d | cost_final %.12g / %.12g"
          % (name, factor, POSE_TOL * factor, d_xy, d_th, ra["iterations"], rb["iterations"], ra["converged"], rb["converged"],
             ra["cost_final"], rb["cost_final"]))
    assert np.abs(moved[:, :2]).max() >= 8191.7 and np.abs(H.workload(("eight", 65))[0][:, :2]).max() <= 10.2
    assert ra["status"] == 0 and rb["status"] == 0 and ra["converged"] == 1 and rb["converged"] == 1, (ra, rb)
    assert d_xy <= POSE_TOL * factor and d_th <= POSE_TOL * factor, (d_xy, d_th)
    assert b[0].tobytes() == moved[0].tobytes()
    assert abs(rb["cost_final"] - ra["cost_final"]) <= 1e-9 * factor * ra["cost_final"]
