"""The four device entry points either side of the match -- ndt_predict_batch_dev, ndt_fuse_batch_dev,
ndt_resample_batch_dev (and the host entry ndt_resample), ndt_scan_to_map_batch_dev -- against the reference's OWN
code: the vectors of tests/golden/front_ref_golden.npz (made in the build container by
tests/golden/make_front_ref_golden.{cpp,py}).  Only the committed fixture is read here.

Bounds: DESIGN.md section 2, table "front-end pins".  Angles, resampled points, counts and offsets: bit-equal.
Prediction: the device's double cos / sin may differ from libm by one ulp, so TOL = 1e-11 relative and 1e-12 x
max(1, |dx| + |dy| + |last.tx| + |last.ty|) absolute.  Fusion: the oracle-against-reference bound of
tests/front_ref_bounds.py plus the tolerance tests/test_gpu_fuse.py has between oracle and device.  Transform: within
one float32 ulp, bit-equal on at least 99 % of the coordinates.  Every test prints the largest difference it saw.
"""
import hashlib
import os

import numpy as np
import pytest

import front_ref_bounds as FB
from gpu_support import gpu, same_bits, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu
TOL = 1e-11
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "front_ref_golden.npz")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLD)


def predict_on_device(ctx, cur, prev, last):
    import torch
    B = len(cur)
    d_cur, d_prev, d_last = to_dev(cur), to_dev(prev), to_dev(last)
    d_mo = torch.zeros(B, 3, dtype=torch.float64, device="cuda:0"); d_pred = torch.zeros_like(d_mo); d_init = torch.zeros_like(d_mo)
    ctx.predict_batch_dev(d_cur.data_ptr(), d_prev.data_ptr(), d_last.data_ptr(), B, d_mo.data_ptr(), d_pred.data_ptr(), d_init.data_ptr())
    torch.cuda.synchronize()
    return d_mo.cpu().numpy(), d_pred.cpu().numpy(), d_init.cpu().numpy()


def test_predict_batch_against_the_reference(gpu, z):
    capi, ctx = gpu
    v = z["pred_in"]
    cur, prev, last = v[:, 0:3], v[:, 3:6], v[:, 6:9]
    mo, pred, init = predict_on_device(ctx, cur, prev, last)          # every prediction vector in one launch
    m_ref, p_ref = z["pred_motion_ref"], z["pred_pred_ref"]
    assert same_bits(mo[:, 2], m_ref[:, 2]) and same_bits(pred[:, 2], p_ref[:, 2])      # no trigonometry in the angles
    size = np.maximum(1.0, np.abs(cur[:, 0] - prev[:, 0]) + np.abs(cur[:, 1] - prev[:, 1]) + np.abs(last[:, 0]) + np.abs(last[:, 1]))
    worst = 0.0
    for got, ref in ((mo[:, :2], m_ref[:, :2]), (pred[:, :2], p_ref[:, :2]), (init[:, :2], p_ref[:, :2])):
        d = np.abs(got - ref)
        tol = np.maximum(TOL * np.abs(ref), 1e-12 * size[:, None])
        worst = max(worst, float((d / tol).max()))
        bad = np.nonzero((d > tol).any(1))[0]
        assert len(bad) == 0, (bad[:8], got[bad[:8]], ref[bad[:8]])
    assert np.abs(init[:, 2] - np.deg2rad(p_ref[:, 2])).max() <= TOL * np.pi
    differ = int((mo[:, :2] != m_ref[:, :2]).sum() + (pred[:, :2] != p_ref[:, :2]).sum())
    print("predict: largest difference %.3g of its bound; %d of %d translation outputs not bit-equal; largest |d| %.3g m"
          % (worst, differ, 4 * len(v), max(np.abs(mo[:, :2] - m_ref[:, :2]).max(), np.abs(pred[:, :2] - p_ref[:, :2]).max())))


def records(capi, est, H, fitness, converged):
    res = np.zeros(len(est), dtype=capi.RESULT_DTYPE)
    res["pose"], res["H"], res["fitness"], res["converged"] = est, H, fitness, converged
    return res


def fuse_on_device(capi, ctx, prm, score_thre, est, H, fitness, converged, pred, motion, last, last_cov):
    import torch
    B = len(est)
    p = capi.default_fuse_params(del_time=prm[0], coe_vel=prm[1], coe_omega=prm[2], coe_ndt_cov=prm[3], score_thre=score_thre)
    d_res = to_dev(np.frombuffer(records(capi, est, H, fitness, converged).tobytes(), np.uint8).copy())
    d_pred, d_mo, d_last, d_lc = to_dev(pred), to_dev(motion), to_dev(last), to_dev(np.asarray(last_cov).reshape(B, 9))
    d_fused = torch.zeros(B, 3, dtype=torch.float64, device="cuda:0"); d_cov = torch.zeros(B, 9, dtype=torch.float64, device="cuda:0")
    d_ok = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
    ctx.fuse_batch_dev(d_res.data_ptr(), d_pred.data_ptr(), d_mo.data_ptr(), d_last.data_ptr(), d_lc.data_ptr(), B, p,
                       d_fused.data_ptr(), d_cov.data_ptr(), d_ok.data_ptr())
    torch.cuda.synchronize()
    return d_fused.cpu().numpy(), d_cov.cpu().numpy(), d_ok.cpu().numpy()


def fuse_within(f, c, f_ref, c_ref, bound):
    """bound = the oracle-against-reference pair (fused, cov) of tests/front_ref_bounds.py; added to it, the
    oracle-against-device tolerance of tests/test_gpu_fuse.py:73-74.  -> (ok, fused difference / its bound, cov likewise)."""
    scale = np.abs(c_ref).max()
    tf = bound[0] * np.maximum(1.0, np.abs(f_ref)) + np.maximum(FB.DEVICE_FUSED_TOL * np.abs(f_ref), FB.DEVICE_FUSED_TOL)
    tc = bound[1] * scale + np.maximum(FB.DEVICE_COV_REL * np.abs(c_ref), FB.DEVICE_COV_ABS * scale)
    df, dc = np.abs(f - f_ref), np.abs(c - c_ref)
    return bool((df <= tf).all() and (dc <= tc).all()), float((df / tf).max()), float((dc / np.where(tc > 0, tc, 1.0)).max())


def test_fuse_batch_against_the_reference(gpu, z):
    capi, ctx = gpu
    sets = np.unique(z["fuse_prm"], axis=0)
    assert len(sets) == 3
    worst_f = worst_c = big_f = big_c = 0.0
    for prm in sets:                                                  # the parameters are per launch: one launch per set
        idx = np.nonzero((z["fuse_prm"] == prm).all(1))[0]
        fused, cov, ok = fuse_on_device(capi, ctx, prm, float(z["score_thre"]), z["fuse_est"][idx], z["fuse_H"][idx], z["fuse_fitness"][idx],
                                        z["fuse_converged"][idx], z["fuse_pred"][idx], z["fuse_motion"][idx], z["fuse_last"][idx],
                                        z["fuse_lastcov"][idx])
        assert np.array_equal(ok, z["fuse_ok"][idx])
        for j, i in enumerate(idx):
            f_ref, c_ref = z["fuse_fused_ref"][i], z["fuse_cov_ref"][i]
            if z["fuse_nonfinite"][i]:                                # Qmat + cov_hat singular: which entries are finite
                assert np.array_equal(np.isfinite(fused[j]), np.isfinite(f_ref)) and np.array_equal(np.isfinite(cov[j]), np.isfinite(c_ref)), i
                continue
            good, rf, rc = fuse_within(fused[j], cov[j], f_ref, c_ref, FB.fusion_bound("oracle", FB.decade(z["fuse_cond"][i])))
            worst_f, worst_c = max(worst_f, rf), max(worst_c, rc)
            big_f = max(big_f, float((np.abs(fused[j] - f_ref) / np.maximum(1.0, np.abs(f_ref))).max()))
            big_c = max(big_c, float(np.abs(cov[j] - c_ref).max() / np.abs(c_ref).max()))
            assert good, (i, fused[j], f_ref, cov[j], c_ref)
    print("fuse: largest scaled difference fused %.3g, cov %.3g (%.3g / %.3g of their bounds)" % (big_f, big_c, worst_f, worst_c))


def test_chained_run_on_the_device_step_by_step(gpu, z):
    """The 60 steps with the DEVICE's fused pose and covariance fed back as lastPose / lastCov: one predict and one fuse
    launch per step, each step against the reference's."""
    capi, ctx = gpu
    odo, prm = z["chain_odo"], z["chain_prm"]
    last, last_cov = odo[0].copy(), np.zeros(9)
    big_f = big_c = 0.0
    for k in range(len(z["chain_ok"])):
        mo, pred, _ = predict_on_device(ctx, odo[k + 1][None], odo[k][None], last[None])
        fused, cov, ok = fuse_on_device(capi, ctx, prm, float(z["score_thre"]), z["chain_est"][k][None], z["chain_H"][k][None],
                                        z["chain_fitness"][k][None], np.ones(1, np.int32), pred, mo, last[None], last_cov[None])
        assert ok[0] == z["chain_ok"][k], k
        f_ref, c_ref = z["chain_fused_ref"][k], z["chain_cov_ref"][k]
        good, _, _ = fuse_within(fused[0], cov[0], f_ref, c_ref, FB.chain_bound("oracle", k))
        big_f = max(big_f, float((np.abs(fused[0] - f_ref) / np.maximum(1.0, np.abs(f_ref))).max()))
        big_c = max(big_c, float(np.abs(cov[0] - c_ref).max() / max(np.abs(c_ref).max(), 1e-300)))
        assert good, (k, fused[0], f_ref, cov[0], c_ref)
        last, last_cov = fused[0], cov[0]
    print("chain on the device: largest scaled difference fused %.3g, cov %.3g over 60 steps" % (big_f, big_c))


def resample_on_device(capi, ctx, scans, space, space_thre):
    import torch
    B = len(scans)
    raw, off = capi.pack_scans(scans, np.float64, offsets_dtype=np.int64)
    cap = capi.resample_capacity(len(raw), space, space_thre)
    d_raw, d_off = to_dev(raw), to_dev(off)
    d64 = torch.full((cap, 2), -1.0, dtype=torch.float64, device="cuda:0")
    d32 = torch.full((cap, 2), -1.0, dtype=torch.float32, device="cuda:0")
    d_oo = torch.full((B + 1,), -1, dtype=torch.int64, device="cuda:0")
    d_st = torch.full((B,), 7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.resample_batch_dev(d_raw.data_ptr(), 16, d_off.data_ptr(), B, len(raw), space, space_thre, d64.data_ptr(), d32.data_ptr(),
                           d_oo.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    return d64.cpu().numpy(), d32.cpu().numpy(), d_oo.cpu().numpy(), d_st.cpu().numpy()


def resampler_vectors(z):
    """-> {(space, space_thre): [(input, reference output or None, count, sha64, sha32)]}: every resampler vector."""
    by = {}
    off, xy = z["rs_off"], z["rs_xy"]
    for v in range(len(z["rs_space"])):
        ref = xy[off[2 * v + 1]:off[2 * v + 2]]
        by.setdefault((float(z["rs_space"][v]), float(z["rs_thre"][v])), []).append((xy[off[2 * v]:off[2 * v + 1]], ref, len(ref), None, None))
    so, grid, full, at = z["rs_syn_in_off"], float(z["rs_syn_grid"]), z["rs_syn_full_ref"], 0
    for s in range(len(so) - 1):
        n = int(z["rs_syn_count_ref"][s])
        ref = full[at:at + n] if at < len(full) else None
        at += n if ref is not None else 0
        by[(0.05, 0.25)].append((z["rs_syn_in_i16"][so[s]:so[s + 1]].astype(np.float64) / grid, ref, n,
                                 str(z["rs_syn_sha64_ref"][s]), str(z["rs_syn_sha32_ref"][s])))
    return by


@pytest.mark.parametrize("order", ["as_recorded", "reversed"])
def test_resample_batch_against_the_reference(gpu, z, order):
    """Per parameter pair (the parameters are per launch) ONE ragged batch that holds every vector of the pair, empty
    scans included; then the same with the scans in reversed order, which moves every offset."""
    capi, ctx = gpu
    n_pts = 0
    for (space, thre), vec in sorted(resampler_vectors(z).items()):
        if order == "reversed":
            vec = vec[::-1]
        o64, o32, oo, st = resample_on_device(capi, ctx, [v[0] for v in vec], space, thre)
        assert np.all(st == capi.NDT_OK), (space, thre, st)
        assert oo[0] == 0 and np.array_equal(np.diff(oo), [v[2] for v in vec]), (space, thre)      # counts and offsets
        for b, (_, ref, n, sha64, sha32) in enumerate(vec):
            g64, g32 = o64[oo[b]:oo[b + 1]], o32[oo[b]:oo[b + 1]]
            if ref is not None:
                assert same_bits(g64, ref), (space, thre, b)
                assert same_bits(g32, ref.astype(np.float32)), (space, thre, b)
            if sha64 is not None:
                assert hashlib.sha256(np.ascontiguousarray(g64).tobytes()).hexdigest() == sha64, (space, thre, b)
                assert hashlib.sha256(np.ascontiguousarray(g32).tobytes()).hexdigest() == sha32, (space, thre, b)
            n_pts += n
    print("resample (%s): %d output points bit-equal to the reference's" % (order, n_pts))


def test_host_resample_entry_against_the_reference(gpu, z):
    capi, ctx = gpu
    for (space, thre), vec in sorted(resampler_vectors(z).items()):
        for b, (xy, ref, n, sha64, _) in enumerate(vec):
            got = ctx.resample(xy, space, thre)
            assert got.dtype == np.float64 and len(got) == n, (space, thre, b)
            if ref is not None:
                assert same_bits(got, ref.reshape(-1, 2)), (space, thre, b)
            if sha64 is not None:
                assert hashlib.sha256(got.tobytes()).hexdigest() == sha64, (space, thre, b)


def ulp_distance(a, b):
    """Distance in float32 ulps (monotone integer map of the bit patterns)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def test_scan_to_map_against_the_reference(gpu, z):
    import torch
    capi, ctx = gpu
    xy, off, poses, ref = z["gm_xy_in"], z["gm_off"], z["gm_pose_in"], z["gm_out32_ref"]
    d_out = torch.full((len(xy), 2), np.nan, dtype=torch.float32, device="cuda:0")
    d_xy, d_off, d_p = to_dev(xy), to_dev(off), to_dev(poses)
    torch.cuda.synchronize()
    ctx.scan_to_map_batch_dev(d_xy.data_ptr(), 16, d_off.data_ptr(), len(poses), len(xy), d_p.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all()
    d = ulp_distance(got, ref)
    differ = int((d != 0).sum())
    print("scan_to_map: %d of %d coordinates not bit-equal to the reference's float32 (largest distance %d ulp)" % (differ, d.size, d.max()))
    assert d.max() <= 1
    assert differ <= d.size // 100
