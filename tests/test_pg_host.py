"""Pose graphs without a GPU: the oracle of tests/pg_helpers.py against finite differences and on every workload the GPU
tests compare with, the halving oracle against the full-step one and the conditions under which its iterates may be compared
with the device's, and the two host helpers of the library (ndt_pg_edge_between, ndt_pg_info_from_cov) against numpy."""
import ctypes as C
import math

import numpy as np
import pytest

import pg_helpers as H


@pytest.fixture(scope="module")
def capi():
    from ndt_slam_amd import build, capi as c
    build.build()
    c.lib()
    return c


def test_record_layouts(capi):
    assert capi.PG_EDGE_DTYPE == H.PG_EDGE_DTYPE
    assert capi.PG_EDGE_DTYPE.itemsize == 80 == C.sizeof(capi.PgEdge)
    assert [capi.PG_EDGE_DTYPE.fields[f][1] for f in ("from", "to", "rel", "info")] == [0, 4, 8, 32]
    assert capi.PG_RESULT_DTYPE.itemsize == 32
    assert C.sizeof(capi.PgParams) == 40
    p = capi.default_pg_params()
    assert (p.max_iter, p.eps_step, p.cg_max_iter, p.cg_rtol, p.max_halvings) == (20, 1e-9, 0, 1e-10, 8)
    assert capi.lib().ndt_pg_default_params(None) == capi.NDT_E_ARG


def test_jacobians_against_central_differences():
    poses, edges, _ = H.workload(("eight", 24))
    rng = np.random.default_rng(5)
    x = np.array(poses)
    x[:, 2] *= H.DEG
    x += rng.normal(0.0, 0.05, x.shape)                # away from the start: nothing special about the point
    A, B = H.jacobians(x, edges)
    h = 1e-6
    worst = 0.0
    for e in range(len(edges)):
        for node, J in ((int(edges[e]["from"]), A[e]), (int(edges[e]["to"]), B[e])):
            for k in range(3):
                xp, xm = x.copy(), x.copy()
                xp[node, k] += h
                xm[node, k] -= h
                d = (H.residuals(xp, edges[e:e + 1])[0] - H.residuals(xm, edges[e:e + 1])[0]) / (2 * h)
                worst = max(worst, float(np.abs(d - J[:, k]).max()))
    # central differences of a smooth function: h^2 f''' / 6 with |f'''| <= |t_j - t_i| < 30 m, plus rounding 1e-16 * 30 / h
    assert worst < 1e-8, worst


def test_normal_equations_are_the_gradient_and_gauss_newton_hessian():
    poses, edges, _ = H.workload(("star", 40))
    x = np.array(poses)
    x[:, 2] *= H.DEG
    Hm, b = H.normal_equations(x, edges)
    assert np.abs(Hm - Hm.T).max() <= 1e-9 * np.abs(Hm).max()
    h, worst = 1e-6, 0.0
    for idx in range(3, 30):
        xp, xm = x.copy().reshape(-1), x.copy().reshape(-1)
        xp[idx] += h
        xm[idx] -= h
        g = (H.cost(xp.reshape(-1, 3), edges) - H.cost(xm.reshape(-1, 3), edges)) / (2 * h)
        worst = max(worst, abs(g - 2.0 * b[idx]) / max(1.0, abs(g)))
    assert worst < 1e-6, worst


@pytest.mark.parametrize("key", sorted(H.WORKLOADS), ids=lambda k: "%s%d" % k)
def test_oracle_converges_in_full_steps(key):
    """The halving rule never changes the minimiser the GPU tests compare with: the oracle's full steps converge in at most 7
    at eps_step 1e-9 and its cost never rises (beyond the rounding of a sum of |E| terms)."""
    poses, edges, ref = H.workload(key)
    assert ref["converged"], ref["steps"]
    k = H.iterations_at(ref, 1e-9)
    assert k is not None and k <= 7, ref["steps"]
    c = ref["costs"]
    for a, b in zip(c, c[1:]):
        assert b <= a + 1e-12 * max(1.0, a), c
    assert np.isfinite(ref["poses"]).all()
    assert ref["poses"][0].tobytes() == poses[0].tobytes()
    assert (ref["poses"][:, 2] >= -180).all() and (ref["poses"][:, 2] < 180).all()


@pytest.mark.parametrize("key", sorted(H.SHAPE_WORKLOADS), ids=lambda k: "%s%d" % k)
def test_shape_workloads_are_what_they_claim_and_converge_in_full_steps(key):
    poses, edges, ref = H.workload(key)
    N, E = len(poses), len(edges)
    assert ref["converged"] and 3 <= H.iterations_at(ref, 1e-9) <= 6, ref["steps"]
    assert np.isfinite(ref["poses"]).all() and ref["poses"][0].tobytes() == poses[0].tobytes()
    degree = np.bincount(np.concatenate([edges["from"], edges["to"]]), minlength=N)
    if key[0] == "hub":
        towards = int((edges["to"] == 7).sum())
        assert degree[7] >= N - 1 and degree[np.arange(N) != 7].max() <= 4 and abs(2 * towards - (N - 1)) <= 1 and degree[0] >= 1
    elif key[0].startswith("dense"):
        assert (N, E) == (int(key[0][5:-1]), key[1]) and (degree > 0).all()
        assert set(2 * e for _, e in H.DENSE_SIZES) >= {254, 256, 258}         # at and on either side of a key array of 256
        assert (edges["from"][N - 1:] > edges["to"][N - 1:]).any() and (edges["from"][N - 1:] < edges["to"][N - 1:]).any()
    else:
        x = np.array(poses)
        x[:, 2] *= H.DEG
        Hm, _ = H.normal_equations(x, edges)
        scale = edges["info"][:, 0] / H.figure_eight(N)[1]["info"][:, 0]
        assert np.linalg.cond(Hm[3:, 3:]) >= 1e7 and scale.max() / scale.min() >= 1e5


# ---- the halving oracle, and the conditions on the far-start workloads (every one a condition on the reference alone) ----

def test_halving_oracle_takes_the_full_step_oracles_steps():
    """Where no step raises F the two oracles are the same arithmetic: equal bit for bit in every cost and step length and in
    the iterate reached, for as long as the steps are longer than 1e-6 (shorter ones are decided by the rounding of F)."""
    for key in sorted(H.WORKLOADS):
        poses, edges, ref = H.workload(key)
        k = next((i for i, s in enumerate(ref["steps"]) if not s > H.FAR_STEP_MIN), len(ref["steps"]))
        assert k >= 2, (key, ref["steps"])
        hv = H.oracle_optimize_halving(poses, edges, eps_step=0.0, max_iter=k)
        assert hv["end"] == H.END_MAX_ITER and hv["halvings"] == [0] * k, (key, hv["halvings"])
        assert hv["steps"] == ref["steps"][:k] and hv["costs"] == ref["costs"][:k + 1], key
        full = H.oracle_optimize(poses, edges, eps_step=0.0, max_iter=k)
        assert hv["poses"].tobytes() == full["poses"].tobytes() == hv["iterates"][-1].tobytes(), key


def test_halving_oracle_ends():
    poses, edges, ref, k = H.far_workload("far24a")
    assert ref["converged"] and ref["end"] in (H.END_ACCEPTED, H.END_RUNOUT_BELOW)
    assert len(ref["iterates"]) == len(ref["steps"]) == len(ref["halvings"]) == len(ref["margins"]) == len(ref["costs"]) - 1
    for a, b in zip(ref["costs"], ref["costs"][1:]):
        assert b <= a                                                    # the rule itself: nothing that raises F is taken
    cut = H.oracle_optimize_halving(poses, edges, eps_step=1e-12, max_iter=3)
    assert cut["end"] == H.END_MAX_ITER and not cut["converged"] and cut["poses"].tobytes() == ref["iterates"][2].tobytes()
    coarse = H.oracle_optimize_halving(poses, edges, eps_step=1e-3)
    n = H.iterations_at(ref, 1e-3)
    assert coarse["end"] == H.END_ACCEPTED and coarse["converged"] and len(coarse["steps"]) == n
    assert coarse["poses"].tobytes() == ref["iterates"][n - 1].tobytes()
    for it in ref["iterates"]:
        assert it[0].tobytes() == poses[0].tobytes() and (it[:, 2] >= -180).all() and (it[:, 2] < 180).all()
    # a run-out below eps_step: from the minimiser, with an eps_step that every proposed step is below
    at_min = H.oracle_optimize_halving(ref["poses"], edges, eps_step=1e-3, max_halvings=0)
    assert at_min["end"] in (H.END_RUNOUT_BELOW, H.END_ACCEPTED) and at_min["converged"]


@pytest.mark.parametrize("name", sorted(H.FAR_STARTS))
def test_far_starts_can_be_compared_iterate_by_iterate(name):
    """What makes a comparison of iterates with the device mean something: every compared step is longer than 1e-6, none of its
    decisions (Ft <= F at every trial) is closer to a tie than 1e-6 of F -- the device evaluates F to about 1e-13 of it -- there
    are six such steps at least, and the run ends in the minimum that the near start of the same arcs reaches."""
    poses, edges, ref, k = H.far_workload(name)
    N = H.FAR_STARTS[name][0]
    print("far start %s: N %d E %d | F %.4g -> %.6f | halvings %s | steps %s | margins %s | %d compared, ends: %s"
          % (name, N, len(edges), ref["costs"][0], ref["costs"][-1], ref["halvings"], ["%.2g" % s for s in ref["steps"]],
             ["%.2g" % s for s in ref["margins"]], k, ref["end"]))
    assert k >= 6, (k, ref["steps"])
    assert all(s > H.FAR_STEP_MIN for s in ref["steps"][:k])
    assert all(m >= H.FAR_MARGIN_MIN for m in ref["margins"][:k]), ref["margins"]
    assert max(ref["halvings"][:k]) >= 1, ref["halvings"]
    assert ref["converged"], ref["end"]
    near = H.workload(("eight", N))[2]
    assert H.pose_error(ref["poses"], near["poses"]) <= (1e-8, 1e-8)
    assert abs(ref["costs"][-1] - near["costs"][-1]) <= 1e-9 * near["costs"][-1]
    assert ref["costs"][0] > 1e4 * ref["costs"][-1]                       # a far start indeed


def test_far_starts_hold_a_step_of_one_halving_and_a_step_of_two():
    seen = set()
    for name in H.FAR_STARTS:
        _, _, ref, k = H.far_workload(name)
        seen |= set(ref["halvings"][:k])
    assert {0, 1, 2} <= seen, seen
    assert max(H.FAR_STARTS[n][0] for n in H.FAR_STARTS) > 256            # one of them takes the node loops round twice


@pytest.mark.parametrize("max_halvings, k", H.FAR_CAP_CASES)
def test_cap_cases_run_out_above_eps_step(max_halvings, k):
    """With max_halvings one below what step k of far24a needs, the run ends at that step, refused at every trial, after
    exactly k - 1 accepted steps; the refused trials are the first ones of the full run's step k, so their margin is its."""
    poses, edges, ref, n_cmp = H.far_workload(H.FAR_CAP_NAME)
    assert k <= n_cmp and ref["halvings"][k - 1] == max_halvings + 1, ref["halvings"]
    cap = H.oracle_optimize_halving(poses, edges, eps_step=1e-9, max_iter=20, max_halvings=max_halvings)
    assert cap["end"] == H.END_RUNOUT_ABOVE and not cap["converged"]
    assert len(cap["steps"]) == k - 1 and cap["halvings"] == ref["halvings"][:k - 1]
    assert cap["poses"].tobytes() == ref["iterates"][k - 2].tobytes()
    trials, dmax, margin = cap["refused"]
    assert trials == max_halvings + 1 and dmax > 1.0 and margin >= ref["margins"][k - 1] >= H.FAR_MARGIN_MIN


@pytest.mark.parametrize("name, max_halvings, eps_step, end, n_steps", H.FAR_COARSE_CASES)
def test_coarse_eps_step_cases_end_on_the_length_of_the_halved_step(name, max_halvings, eps_step, end, n_steps):
    """The run ends `converged` at a step whose halved length is below eps_step and whose full length is above it, by a
    tenth of eps_step at least on either side; every step in front of it is longer than eps_step by as much."""
    poses, edges, ref, _ = H.far_workload(name)
    run = H.oracle_optimize_halving(poses, edges, eps_step=eps_step, max_iter=20, max_halvings=max_halvings)
    assert run["end"] == end and run["converged"] and len(run["steps"]) == n_steps
    assert run["poses"].tobytes() == ref["iterates"][n_steps - 1].tobytes()
    if end == H.END_ACCEPTED:
        last, halvings, front = run["steps"][-1], run["halvings"][-1], run["steps"][:-1]
        assert run["margins"][-1] >= H.FAR_MARGIN_MIN
    else:
        trials, last, margin = run["refused"]
        halvings, front = trials - 1, run["steps"]
        assert margin >= H.FAR_MARGIN_MIN
    assert halvings >= 1 and last <= 0.9 * eps_step and last * 2 ** halvings >= 1.1 * eps_step, (last, halvings)
    assert all(s >= 1.1 * eps_step for s in front), front


def test_rigid_move_keeps_every_arc():
    poses, edges, _ = H.workload(("eight", 65))
    moved = H.rigid_move(poses, (8191.7, -8003.3), 137.0)
    assert np.abs(moved[0, :2] - (8191.7, -8003.3)).max() == 0.0
    for e in edges[::7]:
        a, b = int(e["from"]), int(e["to"])
        d = H.between(moved[a], moved[b]) - H.between(poses[a], poses[b])
        assert np.abs(d[:2]).max() <= 1e-11 and abs(H.wrap_deg(d[2])) <= 1e-11      # 8e3 m in fp64: 1e-12
    assert abs(H.cost_deg(moved, edges) - H.cost_deg(poses, edges)) <= 1e-6 * H.cost_deg(poses, edges)


def test_figure_eight_heading_crosses_180():
    t = H.eight_truth(256)[:, 2]
    jumps = np.abs(np.diff(t)) > 180
    assert int(jumps.sum()) == 2


def test_edge_between_against_numpy(capi):
    rng = np.random.default_rng(11)
    for _ in range(200):
        a = np.array([rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(-180, 180)])
        b = np.array([rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(-180, 180)])
        rel = capi.pg_edge_between(a, b)
        ref = H.between(a, b)
        assert np.abs(rel[:2] - ref[:2]).max() <= 1e-12 and abs(rel[2] - ref[2]) <= 1e-12
        assert -180 <= rel[2] < 180
        back = H.compose(a, rel)
        assert np.abs(back[:2] - b[:2]).max() <= 1e-10 and abs(H.wrap_deg(back[2] - b[2])) <= 1e-10
    # MyUtil::sub_angle's range at its ends
    assert capi.pg_edge_between([0, 0, -170.0], [0, 0, 170.0])[2] == -20.0
    assert capi.pg_edge_between([0, 0, 90.0], [0, 0, -90.0])[2] == -180.0
    # only rel is written
    e = np.zeros(1, capi.PG_EDGE_DTYPE)
    e[0]["from"], e[0]["to"], e[0]["info"] = 3, 4, np.arange(6)
    a, b = np.array([1.0, 2.0, 30.0]), np.array([2.0, 2.5, 50.0])
    assert capi.lib().ndt_pg_edge_between(a.ctypes.data, b.ctypes.data, e.ctypes.data) == 0
    assert (e[0]["from"], e[0]["to"]) == (3, 4) and (e[0]["info"] == np.arange(6)).all()
    assert np.allclose(e[0]["rel"], H.between(a, b), rtol=0, atol=1e-12)


def test_edge_between_refusals(capi):
    L = capi.lib()
    a, e = np.zeros(3), np.zeros(1, capi.PG_EDGE_DTYPE)
    assert L.ndt_pg_edge_between(None, a.ctypes.data, e.ctypes.data) == capi.NDT_E_ARG
    assert L.ndt_pg_edge_between(a.ctypes.data, None, e.ctypes.data) == capi.NDT_E_ARG
    assert L.ndt_pg_edge_between(a.ctypes.data, a.ctypes.data, None) == capi.NDT_E_ARG
    for bad in (np.nan, np.inf):
        with pytest.raises(capi.NdtError):
            capi.pg_edge_between([0, bad, 0], [0, 0, 0])
        with pytest.raises(capi.NdtError):
            capi.pg_edge_between([0, 0, 0], [0, 0, bad])


def _random_spd(rng):
    M = rng.normal(0.0, 1.0, (3, 3))
    return M @ M.T * np.array([[1e-4, 1e-4, 1e-5], [1e-4, 1e-4, 1e-5], [1e-5, 1e-5, 1e-6]]) + np.diag([1e-5, 1e-5, 1e-7])


def test_info_from_cov_against_numpy(capi):
    rng = np.random.default_rng(12)
    for _ in range(200):
        Cw = _random_spd(rng)
        Cw = 0.5 * (Cw + Cw.T)
        th = rng.uniform(-180, 180)
        c, s = math.cos(th * H.DEG), math.sin(th * H.DEG)
        R3 = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
        ref = np.linalg.inv(R3.T @ Cw @ R3)
        got = H.info33(capi.pg_info_from_cov(Cw, th))
        # inverting a 3 x 3 with condition number k loses k * 2^-53 relative to its norm
        k = np.linalg.cond(Cw)
        assert np.abs(got - ref).max() <= 64 * k * 2.0 ** -53 * np.abs(ref).max(), (got, ref)
    # heading 0 is the plain inverse; an identity stays one
    assert np.allclose(capi.pg_info_from_cov(np.eye(3), 37.0), [1, 0, 0, 1, 0, 1], rtol=0, atol=1e-15)
    # a pair that differs in its last bits is averaged, not refused
    Cw = np.diag([1e-4, 2e-4, 1e-6])
    Cw[0, 1], Cw[1, 0] = 1e-5, 1e-5 * (1 + 1e-15)
    assert np.isfinite(capi.pg_info_from_cov(Cw, 10.0)).all()


def test_info_from_cov_refusals(capi):
    L = capi.lib()
    info, eye = np.zeros(6), np.eye(3)
    assert L.ndt_pg_info_from_cov(None, 0.0, info.ctypes.data) == capi.NDT_E_ARG
    assert L.ndt_pg_info_from_cov(eye.ctypes.data, 0.0, None) == capi.NDT_E_ARG
    bad = [np.zeros((3, 3)),                                            # a first scan's covariance
           np.diag([1.0, 1.0, 0.0]), np.diag([1.0, -1.0, 1.0]),
           np.array([[1.0, 2.0, 0], [2.0, 1.0, 0], [0, 0, 1.0]]),       # second minor negative
           np.array([[1.0, 0, 0], [0, 1.0, 1.0], [0, 1.0, 1.0]]),       # singular
           np.array([[1.0, 0.1, 0], [0.2, 1.0, 0], [0, 0, 1.0]]),       # not symmetric
           np.array([[1.0, np.nan, 0], [np.nan, 1.0, 0], [0, 0, 1.0]]),
           np.diag([np.inf, 1.0, 1.0]),
           np.diag([1.67e-35, 4.455e-3, 1.277e-4]),                     # a first matched scan's: positive, and singular to working precision
           np.array([[1e-4, 0, 1e-5], [0, 1e-4, 0], [1e-5, 0, 1e-6 * (1 + 1e-14)]])]   # the heading's pivot at 1e-14 of its entry
    for Cw in bad:
        with pytest.raises(capi.NdtError):
            capi.pg_info_from_cov(Cw, 20.0)
    with pytest.raises(capi.NdtError):
        capi.pg_info_from_cov(eye, np.nan)
    assert (info == 0).all()


def test_batched_calls_refuse_without_a_context(capi):
    L = capi.lib()
    z = np.zeros(8, np.uint64)
    prm = capi.default_pg_params()
    assert L.ndt_pg_optimize_batch(None, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, 1, C.byref(prm), z.ctypes.data) == capi.NDT_E_ARG
    assert L.ndt_pg_optimize_batch_dev(None, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, 1, C.byref(prm), z.ctypes.data,
                                       None) == capi.NDT_E_ARG
    assert L.ndt_repose_points(None, z.ctypes.data, 8, z.ctypes.data, 1, z.ctypes.data, z.ctypes.data, z.ctypes.data, 8) == capi.NDT_E_ARG
    assert L.ndt_repose_points_dev(None, z.ctypes.data, 8, z.ctypes.data, 1, z.ctypes.data, z.ctypes.data, z.ctypes.data, 8, None) == capi.NDT_E_ARG
    assert L.ndt_last_error(None).decode() == "null context"


def test_repose_restatement_is_the_composition_of_the_two_transforms():
    rng = np.random.default_rng(3)
    xy = (rng.uniform(-20, 20, (500, 2)) + np.array([-1003.3, 707.1])).astype(np.float32)
    off = np.array([0, 100, 100, 350, 500], np.uint64)
    old = np.array([[-1000.0, 700.0, 10.0], [0, 0, 0], [-1003.0, 705.0, -170.0], [-990.0, 710.0, 179.0]])
    new = old + np.array([[0.3, -0.2, 1.5], [1, 1, 1], [0, 0, 0], [-0.1, 0.4, 2.0]])
    out = H.repose_ref(xy, off, old, new)
    assert out[100:350].tobytes() == xy[100:350].tobytes()              # bit-equal poses: copied through
    for k in (0, 3):
        a, b = int(off[k]), int(off[k + 1])
        for i in range(a, b, 17):
            local = H.between(old[k], [xy[i, 0], xy[i, 1], old[k][2]])[:2]
            world = H.compose(new[k], [local[0], local[1], 0.0])[:2]
            assert np.abs(world - out[i]).max() <= 2e-4                 # float32 at 1000 m: half an ulp is 3e-5
    assert H.repose_ref(out, off, old, new).tobytes() != out.tobytes()
    assert H.repose_ref(xy, off, old, new).tobytes() == out.tobytes()
