"""Pose graphs without a GPU: the oracle of tests/pg_helpers.py against finite differences and on every workload the GPU
tests compare with, and the two host helpers of the library (ndt_pg_edge_between, ndt_pg_info_from_cov) against numpy."""
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
