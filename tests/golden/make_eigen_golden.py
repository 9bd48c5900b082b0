#!/usr/bin/env python3
"""Generates tests/golden/eigen_golden.npz: outputs of the reference's OWN vendored Eigen 3.3.90
(/root/reference/include/Eigen, header-only, compiled here with plain g++ and no stand-ins) for the small-matrix
steps of the hot path that the oracle restates by hand (VERDICT r03 "pin what can be pinned").

Build-container only: /root/reference does not exist on the GPU box and nothing of Eigen travels -- what is
committed are inputs and Eigen's outputs (data), plus this script and make_eigen_golden.cpp (ours).

Sections of the file (inputs `*_in`, Eigen outputs `*_eig`):
  svd6_*    JacobiSVD<Matrix<double,6,6>>(H, FullU|FullV).solve(-g) on block-embedded H of real C1 passes
            (every derivative pass of 24 matches) + near-singular / singular variants of them
  leaf_*    VoxelGridCovariance's per-leaf block on the per-voxel sums of the C1 map (both covariance presets),
            of 400 voxels of the C3 map and of hand-made edge leaves (identical points, collinear, unsymmetrised cov_)
  inv3_*    Matrix3d::inverse() on -H of final results and on Kalman sums
  init_*    (Translation3f * AngleAxisf).matrix() and Affine3f.rotation().eulerAngles(0,1,2) over yaw strata
  step_*    the line search's float matrix for sampled x_t
  replay_*  the 24 C1 matches replayed by the oracle with Eigen's solve / Eigen's initial p / Eigen's cell table
            substituted through the oracle's test hooks: iteration counts, float32 transforms, step sequences
"""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from ndt_slam_amd import synth          # noqa: E402
from oracle import ndt_oracle as O      # noqa: E402

REF_INC = "/root/reference/include"
SO = os.path.join(ROOT, "oracle", "_ref", "libeigen_ref.so")
N_C1 = 24


def build_eigen_ref():
    """g++ on make_eigen_golden.cpp against the reference's vendored Eigen, output only into oracle/_ref/."""
    if not os.path.isdir(os.path.join(REF_INC, "Eigen")):
        raise SystemExit("the reference's vendored Eigen is not here (%s): run this in the build container" % REF_INC)
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    src = os.path.join(HERE, "make_eigen_golden.cpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-fPIC", "-shared", "-I" + REF_INC,
                               src, "-o", SO])
    return SO


class Eig:
    """ctypes face of oracle/_ref/libeigen_ref.so."""

    def __init__(self, so=None):
        self.L = L = C.CDLL(so or build_eigen_ref())
        vp = C.c_void_p
        L.eig_svd6_solve.argtypes = [vp] * 5
        L.eig_leaf.restype = C.c_int
        L.eig_leaf.argtypes = [C.c_int, vp, vp, C.c_double, C.c_int, vp, vp, vp, vp, vp]
        L.eig_inv3.argtypes = [vp, vp]
        L.eig_init_guess.argtypes = [C.c_float] * 3 + [vp] * 5
        L.eig_step_matrix.argtypes = [vp, vp]

    def version(self):
        v = (C.c_int * 3)()
        self.L.eig_version(v)
        return tuple(v)

    def svd6_solve(self, H3, g3):
        H3 = np.ascontiguousarray(H3, np.float64).reshape(9)
        g3 = np.ascontiguousarray(g3, np.float64).reshape(3)
        dp3, dp6, sv6 = np.zeros(3), np.zeros(6), np.zeros(6)
        self.L.eig_svd6_solve(H3.ctypes.data, g3.ctypes.data, dp3.ctypes.data, dp6.ctypes.data, sv6.ctypes.data)
        return dp3, dp6, sv6

    def leaf(self, n, pt_sum, cov_acc, mult, unbiased):
        pt_sum = np.ascontiguousarray(pt_sum, np.float64).reshape(3)
        cov_acc = np.ascontiguousarray(cov_acc, np.float64).reshape(9)
        mean, cov, evals, evecs, icov = np.zeros(3), np.zeros(9), np.zeros(3), np.zeros(9), np.zeros(9)
        nr = self.L.eig_leaf(int(n), pt_sum.ctypes.data, cov_acc.ctypes.data, float(mult), int(unbiased),
                             mean.ctypes.data, cov.ctypes.data, evals.ctypes.data, evecs.ctypes.data, icov.ctypes.data)
        return nr, mean, cov.reshape(3, 3), evals, evecs.reshape(3, 3), icov.reshape(3, 3)

    def inv3(self, A):
        A = np.ascontiguousarray(A, np.float64).reshape(9)
        out = np.zeros(9)
        self.L.eig_inv3(A.ctypes.data, out.ctypes.data)
        return out.reshape(3, 3)

    def init_guess(self, tx, ty, yaw):
        M, t, er, el, R = (np.zeros(16, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32),
                           np.zeros(3, np.float32), np.zeros(9, np.float32))
        self.L.eig_init_guess(np.float32(tx), np.float32(ty), np.float32(yaw), M.ctypes.data, t.ctypes.data,
                              er.ctypes.data, el.ctypes.data, R.ctypes.data)
        return M.reshape(4, 4), t, er, el, R.reshape(3, 3)

    def step_matrix(self, x_t):
        x_t = np.ascontiguousarray(x_t, np.float64).reshape(6)
        M = np.zeros(16, np.float32)
        self.L.eig_step_matrix(x_t.ctypes.data, M.ctypes.data)
        return M.reshape(4, 4)


# ---- the oracle's pin points (oracle/ndt_oracle.h, end) ----
def oracle_pins():
    L = O.lib()
    vp = C.c_void_p
    L.ndt_oracle_leaf.restype = C.c_int
    L.ndt_oracle_leaf.argtypes = [C.POINTER(O.Params), C.c_int, vp, vp, vp]
    L.ndt_oracle_inv3.argtypes = [vp, vp]
    L.ndt_oracle_init_guess.argtypes = [C.POINTER(O.Params), vp, vp, vp]
    L.ndt_oracle_step_matrix.argtypes = [C.POINTER(O.Params), vp, vp]
    L.ndt_oracle_map_override_cells.argtypes = [vp, vp, vp, vp]
    L.ndt_oracle_map_export_sums.argtypes = [vp, vp]
    return L


SOLVE_FN, INITP_FN, Hooks = O.SOLVE_FN, O.INITP_FN, O.Hooks      # ndt_oracle_hooks, declared once in oracle/ndt_oracle.py


def map_sums(M):
    n = M.info().n_cells
    out = np.zeros((n, 7))
    oracle_pins().ndt_oracle_map_export_sums(M.h, out.ctypes.data)
    return out


def leaf_inputs_from_sums(s, identity):
    """(n, pt_sum[3], cov_acc[3,3]) as PCL's accumulation leaves them for a z = 0 voxel."""
    n = int(s[0])
    pt_sum = np.array([s[1], s[2], 0.0])
    cov = np.array([[s[3], s[4], 0.0], [s[4], s[5], 0.0], [0.0, 0.0, s[6]]])
    return n, pt_sum, cov


def eigen_cell_table(E, M, prm):
    """The cell table with the fp64 part computed by Eigen through eig_leaf: (mean[n,2], icov[n,3], npts)."""
    sums = map_sums(M)
    t = M.export()
    mean, icov, npts = t["mean"].copy(), t["icov"].copy(), t["npts"].copy()
    for c in range(len(sums)):
        n, ps, cv = leaf_inputs_from_sums(sums[c], prm.cov_init_identity)
        nr, mu, cov, evals, evecs, ic = E.leaf(n, ps, cv, prm.eig_mult, prm.cov_unbiased)
        mean[c] = mu[:2]
        if nr > 0:
            # PCL keeps the full (possibly unsymmetric at the last bit) 3x3; the SE(2) reduction holds xx, xy, yy
            icov[c] = [ic[0, 0], 0.5 * (ic[0, 1] + ic[1, 0]), ic[1, 1]]
            npts[c] = n
        else:
            icov[c] = 0.0
            npts[c] = -n
    return mean, icov, npts


def main():
    E = Eig()
    L = oracle_pins()
    out = {"eigen_version": np.array(E.version())}
    rng = np.random.Generator(np.random.Philox(4))

    # ------------------------------------------------------------------ C1 workload (the golden matches)
    cfg = synth.CONFIGS["C1"]
    m = synth.make_map(cfg["n_map"], cfg["half"])
    sf = synth.ScanFactory(m, cfg["half"], cfg["n_scan"])
    scans, off, truths, inits = sf.batch(0, N_C1)
    prm = O.default_params(resolution=cfg["resolution"])
    M = O.Map(m, prm)

    # ------------------------------------------------------------------ svd6: every pass of the 24 matches
    Hs, gs = [], []
    base_res, base_traces = [], []
    for b in range(N_C1):
        sc = scans[int(off[b]):int(off[b + 1])]
        r, tr = M.align(sc, inits[b], trace_cap=512)
        base_res.append(r)
        base_traces.append(tr)
        for row in tr:
            s, g, H, _ = M.eval_at(sc, row[5:8])
            Hs.append(H)
            gs.append(g)
    Hs, gs = np.array(Hs), np.array(gs)
    n_real = len(Hs)
    # near-singular variants: shrink the weakest eigen-direction of a real H by 1e-6 .. 1e-15, and exact rank loss
    extra_H, extra_g = [], []
    for k in range(120):
        H = Hs[rng.integers(n_real)]
        g = gs[rng.integers(n_real)]
        w, V = np.linalg.eigh(0.5 * (H + H.T))
        j = int(np.argmin(np.abs(w)))
        w2 = w.copy()
        w2[j] *= 10.0 ** (-rng.uniform(6, 15))
        if k % 10 == 0:
            w2[j] = 0.0
        extra_H.append((V * w2) @ V.T)
        extra_g.append(g)
    for k in range(20):                               # a corridor: no information along x at all
        H = Hs[rng.integers(n_real)].copy()
        H[0, :] = 0.0
        H[:, 0] = 0.0
        extra_H.append(H)
        extra_g.append(gs[rng.integers(n_real)] * np.array([0.0, 1.0, 1.0]))
    svd_H = np.concatenate([Hs, np.array(extra_H)])
    svd_g = np.concatenate([gs, np.array(extra_g)])
    dp3 = np.zeros((len(svd_H), 3))
    dp6 = np.zeros((len(svd_H), 6))
    sv6 = np.zeros((len(svd_H), 6))
    for i in range(len(svd_H)):
        dp3[i], dp6[i], sv6[i] = E.svd6_solve(svd_H[i], svd_g[i])
    out.update(svd6_H_in=svd_H, svd6_g_in=svd_g, svd6_dp3_eig=dp3, svd6_dp6_eig=dp6, svd6_sv_eig=sv6,
               svd6_n_real=np.array(n_real))

    # ------------------------------------------------------------------ leaves
    leaf_rows = []       # (preset_unbiased, identity, n, sums[6]) + Eigen outputs

    def add_leaves(Mx, px, pick=None):
        sums = map_sums(Mx)
        idx = range(len(sums)) if pick is None else pick
        for c in idx:
            leaf_rows.append((px.cov_unbiased, px.cov_init_identity, sums[c]))

    add_leaves(M, prm)
    prm_new = O.default_params("pcl_new", resolution=cfg["resolution"])
    M_new = O.Map(m, prm_new)
    add_leaves(M_new, prm_new)
    c3 = synth.CONFIGS["C3"]
    m3 = synth.make_map(c3["n_map"], c3["half"])
    prm3 = O.default_params(resolution=c3["resolution"])
    M3 = O.Map(m3, prm3)
    n3 = M3.info().n_cells
    add_leaves(M3, prm3, pick=rng.choice(n3, 400, replace=False))
    del M3
    # hand-made edge leaves: six identical points; exactly collinear; two clusters; huge offset; tiny spread
    def sums_of(pts, identity):
        sx = sy = 0.0
        sxx, sxy, syy, szz = (1.0, 0.0, 1.0, 1.0) if identity else (0.0, 0.0, 0.0, 0.0)
        for x, y in np.asarray(pts, np.float32).astype(np.float64):
            sx += x; sy += y; sxx += x * x; sxy += x * y; syy += y * y
        return np.array([len(pts), sx, sy, sxx, sxy, syy, szz])
    edge = [
        [(1.25, -3.5)] * 6,
        [(0.1 * k, 0.2 * k) for k in range(8)],
        [(10.0 + 0.01 * k, -7.0) for k in range(7)],
        [(200.0 + 0.3 * (k % 2), 150.0 + 0.001 * k) for k in range(12)],
        [(-255.9 + 1e-4 * k, 255.9 - 1e-4 * k * k) for k in range(9)],
        [(0.0, 0.0), (0.3, 0.0), (0.0, 0.3), (0.3, 0.3), (0.15, 0.15), (0.1, 0.2)],
    ]
    for pts in edge:
        for (ub, idn) in ((0, 1), (1, 0), (0, 0)):
            leaf_rows.append((ub, idn, sums_of(pts, idn)))
    nL = len(leaf_rows)
    leaf_in = np.zeros((nL, 9))          # unbiased, identity, n, sx, sy, sxx, sxy, syy, szz
    leaf_nr = np.zeros(nL, np.int32)
    leaf_mean, leaf_cov, leaf_evals = np.zeros((nL, 3)), np.zeros((nL, 3, 3)), np.zeros((nL, 3))
    leaf_evecs, leaf_icov = np.zeros((nL, 3, 3)), np.zeros((nL, 3, 3))
    for i, (ub, idn, s) in enumerate(leaf_rows):
        leaf_in[i] = [ub, idn] + list(s)
        n, ps, cv = leaf_inputs_from_sums(s, idn)
        leaf_nr[i], leaf_mean[i], leaf_cov[i], leaf_evals[i], leaf_evecs[i], leaf_icov[i] = E.leaf(n, ps, cv, 0.01, ub)
    out.update(leaf_in=leaf_in, leaf_nr_eig=leaf_nr, leaf_mean_eig=leaf_mean, leaf_cov_eig=leaf_cov,
               leaf_evals_eig=leaf_evals, leaf_evecs_eig=leaf_evecs, leaf_icov_eig=leaf_icov)

    # ------------------------------------------------------------------ inv3
    inv_in = [-(np.asarray(r["H"]).reshape(3, 3)) for r in base_res]
    for k in range(200):
        A = rng.normal(size=(3, 3))
        S = A @ A.T * 10.0 ** rng.uniform(-6, 6) + np.diag(rng.uniform(0, 1e-3, 3))
        inv_in.append(S if k % 3 else A)
    inv_in = np.array(inv_in)
    out.update(inv3_in=inv_in, inv3_eig=np.array([E.inv3(A) for A in inv_in]))

    # ------------------------------------------------------------------ init guess + step matrix
    yaws = np.concatenate([
        inits[:, 2], rng.uniform(-math.pi, math.pi, 400),
        math.pi / 2 + rng.uniform(-0.01, 0.01, 60), -math.pi / 2 + rng.uniform(-0.01, 0.01, 60),
        math.pi - rng.uniform(0, 0.01, 60), -math.pi + rng.uniform(0, 0.01, 60),
        rng.uniform(-2e-4, 2e-4, 60), [0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi]])
    txy = np.concatenate([inits[:, :2], rng.uniform(-250, 250, (len(yaws) - N_C1, 2))])
    init_in = np.column_stack([txy, yaws])
    init_M = np.zeros((len(yaws), 4, 4), np.float32)
    init_t, init_er, init_el = (np.zeros((len(yaws), 3), np.float32) for _ in range(3))
    init_R = np.zeros((len(yaws), 3, 3), np.float32)
    for i, (tx, ty, yw) in enumerate(init_in):
        init_M[i], init_t[i], init_er[i], init_el[i], init_R[i] = E.init_guess(tx, ty, yw)
    out.update(init_in=init_in, init_M_eig=init_M, init_trans_eig=init_t, init_euler_rotation_eig=init_er,
               init_euler_linear_eig=init_el, init_rotation_eig=init_R)
    step_in = np.zeros((len(yaws), 6))
    step_in[:, 0:2] = txy + rng.normal(0, 0.05, txy.shape)
    step_in[:, 3] = -0.0                                   # roll, pitch as eulerAngles returns them for a z rotation
    step_in[:, 5] = yaws + rng.normal(0, 0.01, len(yaws))
    out.update(step_in=step_in, step_M_eig=np.array([E.step_matrix(x) for x in step_in]))

    # ------------------------------------------------------------------ replays of the 24 C1 matches
    def run_all(Mx, cap=512):
        rs, trs = [], []
        for b in range(N_C1):
            r, tr = Mx.align(scans[int(off[b]):int(off[b + 1])], inits[b], trace_cap=cap)
            rs.append(r)
            trs.append(tr)
        return np.array(rs), trs

    def pack(trs):
        cap = max(len(t) for t in trs)
        a = np.full((N_C1, cap, 8), np.nan)
        for b, t in enumerate(trs):
            a[b, :len(t)] = t
        return a

    @SOLVE_FN
    def eig_solve(Hp, bp, xp):
        H = np.array([Hp[i] for i in range(9)])
        b = np.array([bp[i] for i in range(3)])
        d, _, _ = E.svd6_solve(H, -b)          # the oracle passes b = -g; eig_svd6_solve negates its gradient itself
        for i in range(3):
            xp[i] = d[i]

    @INITP_FN
    def eig_initp(Tp, pp):
        # the oracle has built T = (c, s, tx, ty) from the caller's pose; PCL reads the angles back from that matrix.
        # Rebuild the same float matrix through Eigen from (tx, ty) and the yaw whose cos/sin it holds is not possible
        # in general, so the hook receives the matrix and asks Eigen for the angles of exactly those entries:
        c, s, tx, ty = Tp[0], Tp[1], Tp[2], Tp[3]
        e = euler_of_matrix(c, s)
        pp[0], pp[1], pp[2] = float(np.float32(tx)), float(np.float32(ty)), float(e)

    # eulerAngles of rotation() for given float entries: through eig_init_guess's own path we can only pass a yaw, so
    # find it from the table made above (every C1 init is in init_in) -- keyed by the float entries
    table = {}
    for i in range(len(init_in)):
        table[(init_M[i, 0, 0].tobytes(), init_M[i, 1, 0].tobytes())] = init_er[i, 2]

    def euler_of_matrix(c, s):
        return table[(np.float32(c).tobytes(), np.float32(s).tobytes())]

    base_r, base_t = np.array(base_res), base_traces
    hk = Hooks(eig_solve, INITP_FN())
    L.ndt_oracle_set_hooks(C.byref(hk))
    solve_r, solve_t = run_all(M)
    hk2 = Hooks(SOLVE_FN(), eig_initp)
    L.ndt_oracle_set_hooks(C.byref(hk2))
    initp_r, initp_t = run_all(M)
    L.ndt_oracle_set_hooks(None)
    M_e = O.Map(m, prm)
    mean_e, icov_e, npts_e = eigen_cell_table(E, M_e, prm)
    L.ndt_oracle_map_override_cells(M_e.h, mean_e.ctypes.data, icov_e.ctypes.data, npts_e.ctypes.data)
    cells_r, cells_t = run_all(M_e)
    hk3 = Hooks(eig_solve, eig_initp)
    L.ndt_oracle_set_hooks(C.byref(hk3))
    all_r, all_t = run_all(M_e)
    L.ndt_oracle_set_hooks(None)
    out.update(replay_scans=scans, replay_offsets=off, replay_inits=inits, replay_map=m,
               replay_resolution=np.float32(cfg["resolution"]),
               replay_base_results=base_r, replay_base_trace=pack(base_t),
               replay_solve_results=solve_r, replay_solve_trace=pack(solve_t),
               replay_initp_results=initp_r, replay_initp_trace=pack(initp_t),
               replay_cells_results=cells_r, replay_cells_trace=pack(cells_t),
               replay_all_results=all_r, replay_all_trace=pack(all_t),
               replay_cells_mean_eig=mean_e, replay_cells_icov_eig=icov_e, replay_cells_npts_eig=npts_e)

    path = os.path.join(HERE, "eigen_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; Eigen", E.version(), "|", len(svd_H), "solves,", nL, "leaves,",
          len(inv_in), "inverses,", len(init_in), "init guesses")
    for name, rr in (("solve", solve_r), ("init_p", initp_r), ("cells", cells_r), ("all", all_r)):
        same_T = sum(all(rr[b][k] == base_r[b][k] for k in ("T00", "T10", "T03", "T13")) for b in range(N_C1))
        same_it = int(np.sum(rr["iters"] == base_r["iters"]))
        dpose = np.abs(rr["pose"] - base_r["pose"]).max()
        print("replay %-7s identical float32 T: %d/%d, identical iters: %d/%d, max |dpose| %.3g" %
              (name, same_T, N_C1, same_it, N_C1, dpose))


if __name__ == "__main__":
    main()
