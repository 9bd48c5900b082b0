"""Every restatement of the rows either side of the match against the reference's OWN code.

tests/golden/front_ref_golden.npz holds inputs and the outputs of the reference's src/Pose2D.cpp, src/MyUtil.cpp,
src/PoseFuser.cpp and src/ScanPointResampler.cpp, compiled in the build container behind
tests/golden/make_front_ref_golden.{cpp,py} (what the driver does itself is listed in the generator's docstring).
Held against it here: the C oracle (oracle.predict / oracle.fuse), the numpy twin of tests/test_fuse_oracle.py, and the
host mirrors replay.add_angle / sub_angle / calMotion / calPredPose / PoseFuser / resample_points /
ScanMatcher.matchScanBegin / matchScanEnd / growMap and pose_estimator.Pose2D.

Bounds (DESIGN.md section 2, table "front-end pins"): the restatements that claim to be verbatim -- angles, Rmat,
prediction, the resampler's points and counts, the float64 transform -- were measured bit-equal on every vector and
are asserted bit-equal.  Fusion is not verbatim (Eigen's evaluation order; np.linalg.inv in the mirror and the twin):
tests/front_ref_bounds.py holds the largest difference measured per restatement, per output and per condition-number
decade (per step for the chained run), scaled as tests/test_gpu_fuse.py scales; asserted is 4 x that, and for the C
oracle never more than the tolerance tests/test_gpu_fuse.py has between oracle and device.
`python tests/test_front_ref_pins.py` prints the tables as measured now.
"""
import hashlib
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ndt_slam_amd import replay                                    # noqa: E402
from ndt_slam_amd.pose_estimator import RAD2DEG, Pose2D, Scan2D    # noqa: E402
from test_fuse_oracle import numpy_kalman_update, numpy_odometry_covariance, result_record   # noqa: E402
import front_ref_bounds as FB                                      # noqa: E402
from gpu_support import same_bits                                  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "front_ref_golden.npz")
RESTATEMENTS = ("oracle", "twin", "replay")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLD)


def pose3(p):
    return np.array([p.tx, p.ty, p.th])


# ---- the fixture itself ---------------------------------------------------------------------------------------------
def test_fixture_is_what_the_issue_asks_for(z):
    assert tuple(z["eigen_version"]) == (3, 3, 90)
    assert "-ffp-contract=off" in str(z["built_flags"]) and "-march" not in str(z["built_flags"]) and str(z["built_compiler"])
    n = len(z["fuse_ok"])
    assert 0 < z["fuse_nonfinite"].sum() < 0.02 * n
    assert set(np.unique(z["fuse_ok"])) == {0, 1} and len(np.unique(z["fuse_prm"], axis=0)) == 3
    assert (np.abs(z["fuse_lastcov"]).max(1) == 0).sum() >= 2                        # the second scan of a run
    assert (np.abs(z["fuse_motion"]).max(1) == 0).sum() >= 2                         # zero motion
    lc = z["fuse_lastcov"].reshape(-1, 3, 3)
    assert (np.abs(lc - lc.transpose(0, 2, 1)).max((1, 2)) > 0).sum() >= 2           # an unsymmetric lastCov
    fin = ~z["fuse_nonfinite"]
    assert z["fuse_cond"][fin].min() < 10 and z["fuse_cond"][fin].max() > 0.99e10
    assert len(z["chain_ok"]) == 60 and 5 < z["chain_ok"].sum() < 55
    assert len(z["rs_syn_count_ref"]) == 32 and np.all(np.diff(z["rs_syn_in_off"]) == 1081)
    assert len(z["gm_pose_in"]) == 24 and len(z["pred_in"]) >= 200
    size = os.path.getsize(GOLD)
    others = [os.path.getsize(os.path.join(os.path.dirname(GOLD), f)) for f in os.listdir(os.path.dirname(GOLD))
              if f.endswith(".npz") and f != os.path.basename(GOLD)]
    assert size <= max(others) and size < (1 << 20)


# ---- verbatim restatements: bit-equal ---------------------------------------------------------------------------------
def test_angle_helpers_are_the_references_bit_for_bit(z):
    """MyUtil::add_angle / sub_angle (src/MyUtil.cpp:4-23): [-180, 180), one wrap only."""
    for (a, b), s, d in zip(z["ang_in"], z["ang_add_ref"], z["ang_sub_ref"]):
        assert same_bits(np.float64(replay.add_angle(a, b)), s), (a, b)
        assert same_bits(np.float64(replay.sub_angle(a, b)), d), (a, b)
    # the vectors do sit on the edges: exactly +-180 comes out as -180 / -180, one ulp below 180 stays, 540 wraps once
    assert replay.add_angle(170.0, 10.0) == -180.0 and replay.sub_angle(-170.0, 10.0) == -180.0
    assert (z["ang_add_ref"] >= 180).any() and (z["ang_add_ref"] < -180).any()       # inputs outside the interval stay outside


def test_pose2d_rotation_matrix_is_the_references(z):
    """pose_estimator.Pose2D.setPose against Pose2D::calRmat (include/ndt_slam/Pose2D.h:43-48), row / column order included."""
    for th, r in zip(z["rmat_in"], z["rmat_ref"]):
        assert same_bits(np.array(Pose2D(0.0, 0.0, th).Rmat, np.float64).ravel(), r), th
    assert z["rmat_ref"][1][1] == -1.0 and z["rmat_ref"][1][2] == 1.0               # th = 90: Rmat[0][1] = -sin, Rmat[1][0] = +sin


def test_prediction_is_the_references_bit_for_bit(z, oracle):
    """oracle.predict and replay.calMotion / calPredPose against Pose2D::calMotion + calPredPose (src/Pose2D.cpp:5-37)
    chained as src/ScanMatcher.cpp:27-32 chains them: every output, angles included, bit-equal (the oracle and the
    reference build call the same libm)."""
    for v, m, p in zip(z["pred_in"], z["pred_motion_ref"], z["pred_pred_ref"]):
        mo, pr = oracle.predict(v[0:3], v[3:6], v[6:9])
        assert same_bits(mo, m) and same_bits(pr, p), v
        m2 = replay.calMotion(Pose2D(*v[0:3]), Pose2D(*v[3:6]))
        p2 = replay.calPredPose(m2, Pose2D(*v[6:9]))
        assert same_bits(pose3(m2), m) and same_bits(pose3(p2), p), v


def test_resampler_mirror_is_the_references_points_and_counts(z):
    """replay.resample_points against ScanPointResampler::resamplePoints (src/ScanPointResampler.cpp:4-62)."""
    off, xy = z["rs_off"], z["rs_xy"]
    for v in range(len(z["rs_space"])):
        got = replay.resample_points(xy[off[2 * v]:off[2 * v + 1]], z["rs_space"][v], z["rs_thre"][v])
        ref = xy[off[2 * v + 1]:off[2 * v + 2]]
        assert len(got) == len(ref) and same_bits(got, ref), (v, z["rs_space"][v], z["rs_thre"][v], len(got), len(ref))
    so, grid = z["rs_syn_in_off"], float(z["rs_syn_grid"])
    full, at = z["rs_syn_full_ref"], 0
    for s in range(len(so) - 1):
        got = replay.resample_points(z["rs_syn_in_i16"][so[s]:so[s + 1]].astype(np.float64) / grid, 0.05, 0.25)
        assert len(got) == z["rs_syn_count_ref"][s], s
        if at < len(full):
            assert same_bits(got, full[at:at + len(got)]), s
            at += len(got)
        assert hashlib.sha256(got.tobytes()).hexdigest() == str(z["rs_syn_sha64_ref"][s]), s
        assert hashlib.sha256(got.astype(np.float32).tobytes()).hexdigest() == str(z["rs_syn_sha32_ref"][s]), s
    assert at == len(full)


class CapturePcmap:
    """Stands in for PointCloudMap behind ScanMatcher: keeps what growMap hands over."""
    localMap_cloud = np.zeros((0, 2), np.float32)

    def __init__(self):
        self.lastPose, self.lps = Pose2D(), None

    def addPose(self, p):
        pass

    def addPoints(self, lps):
        self.lps = np.asarray(lps)
        self.cloud = np.ascontiguousarray(lps, dtype=np.float32).reshape(-1, 2)     # as replay.PointCloudMap.addPoints does

    def setLastPose(self, p):
        self.lastPose = p

    def getLastPose(self):
        return self.lastPose

    def setLastScan(self, s):
        pass

    def makeLocalMap(self):
        pass


class NoEstimator:
    def setScanPair(self, cur, ref):
        pass


def test_grow_map_mirror_is_the_references_transform(z):
    """replay.ScanMatcher.growMap against Pose2D::globalPoint (src/Pose2D.cpp:55-59, the expression of
    src/ScanMatcher.cpp:100-101): float64 bit-equal, and so is the float32 the map cloud stores."""
    off = z["gm_off"]
    for b, pose in enumerate(z["gm_pose_in"]):
        cap = CapturePcmap()
        replay.ScanMatcher(None, cap, None).growMap(Scan2D(z["gm_xy_in"][off[b]:off[b + 1]]), Pose2D(*pose))
        assert same_bits(cap.lps, z["gm_out64_ref"][off[b]:off[b + 1]]), b
        assert same_bits(cap.cloud, z["gm_out32_ref"][off[b]:off[b + 1]]), b
    assert same_bits(z["pt_global_ref"], z["pt_global_out_ref"])                    # the two overloads agree
    for pose, p, g, r in zip(z["pt_pose_in"], z["pt_in"], z["pt_global_ref"], z["pt_relative_ref"]):
        cap = CapturePcmap()
        replay.ScanMatcher(None, cap, None).growMap(Scan2D(p.reshape(1, 2)), Pose2D(*pose))
        assert same_bits(cap.lps[0], g), pose
        # relativePoint has no restatement in the tree; recorded, and it does invert globalPoint (rounding of |p| + |t|)
        back = np.array(Pose2D(*pose).Rmat) @ r + pose[:2]
        assert np.abs(back - p).max() <= 8 * np.finfo(float).eps * (np.abs(p).max() + np.abs(pose[:2]).max())


# ---- fusion: measured bounds -------------------------------------------------------------------------------------------
def fuse_oracle(O, prm, ok, est, H, pred, motion, last, lc, fitness, converged, score_thre):
    p = O.default_fuse_params(del_time=prm[0], coe_vel=prm[1], coe_omega=prm[2], coe_ndt_cov=prm[3], score_thre=score_thre)
    k, f, c = O.fuse(result_record(O, est, H, fitness=fitness, converged=converged), pred, motion, last, lc.reshape(3, 3), p)
    assert k == ok
    return f, c.ravel()


def fuse_twin(O, prm, ok, est, H, pred, motion, last, lc, fitness, converged, score_thre):
    with np.errstate(all="ignore"):
        if not ok:
            return np.array(pred), numpy_odometry_covariance(prm[0], prm[1], prm[2], motion, last, lc.reshape(3, 3)).ravel()
        try:
            mu, cov = numpy_kalman_update(prm[0], prm[1], prm[2], prm[3], est, H, pred, motion, last, lc.reshape(3, 3))
        except np.linalg.LinAlgError:                                               # numpy refuses an exactly singular matrix
            return np.full(3, np.nan), np.full(9, np.nan)
    return np.array([mu[0], mu[1], np.rad2deg(mu[2])]), cov.ravel()


def fuse_replay(O, prm, ok, est, H, pred, motion, last, lc, fitness, converged, score_thre):
    """ScanMatcher.matchScanEnd (the accept test and both branches) over replay.PoseFuser, with the cost, estPose and
    Qmat pose_estimator.PoseEstimator.finishEstimate derives from a match record."""
    sm = replay.ScanMatcher(NoEstimator(), CapturePcmap(), replay.PoseFuser(prm[1], prm[2], prm[0]), scthre=score_thre)
    sm.lastCov = lc.reshape(3, 3)
    sm._pending = (Scan2D(np.zeros((0, 2))), Pose2D(*motion), Pose2D(*last), Pose2D(*pred))
    cost = fitness if converged else 10000000.0
    with np.errstate(all="ignore"):
        try:
            Q = np.linalg.inv(-H.reshape(3, 3)) * prm[3]
        except np.linalg.LinAlgError:
            Q = np.full((3, 3), np.inf)
        try:
            assert sm.matchScanEnd(cost, Pose2D(est[0], est[1], RAD2DEG(est[2])), Q) == bool(ok)
        except np.linalg.LinAlgError:
            return np.full(3, np.nan), np.full(9, np.nan)
    return pose3(sm.poses[-1]), np.asarray(sm.Covs[-1]).ravel()


FUSERS = {"oracle": fuse_oracle, "twin": fuse_twin, "replay": fuse_replay}


def fuse_errors(f, c, f_ref, c_ref):
    """(fused, cov) differences scaled as tests/test_gpu_fuse.py:72-74 scales its tolerances: fused per entry by
    max(1, |ref|), cov by the largest |entry| of the reference covariance."""
    scale = np.abs(c_ref).max()
    return float((np.abs(f - f_ref) / np.maximum(1.0, np.abs(f_ref))).max()), float(np.abs(c - c_ref).max() / (scale if scale > 0 else 1.0))


def measure_fusion(z, O, name):
    """-> {decade: [fused, cov]} over the finite vectors, and the list of non-finite vectors' (got, ref) pairs."""
    tab, nonfinite = {}, []
    for i in range(len(z["fuse_ok"])):
        f, c = FUSERS[name](O, z["fuse_prm"][i], int(z["fuse_ok"][i]), z["fuse_est"][i], z["fuse_H"][i], z["fuse_pred"][i],
                            z["fuse_motion"][i], z["fuse_last"][i], z["fuse_lastcov"][i], float(z["fuse_fitness"][i]),
                            int(z["fuse_converged"][i]), float(z["score_thre"]))
        if z["fuse_nonfinite"][i]:
            nonfinite.append((i, f, c, z["fuse_fused_ref"][i], z["fuse_cov_ref"][i]))
            continue
        ef, ec = fuse_errors(f, c, z["fuse_fused_ref"][i], z["fuse_cov_ref"][i])
        t = tab.setdefault(FB.decade(z["fuse_cond"][i]), [0.0, 0.0])
        t[0], t[1] = max(t[0], ef), max(t[1], ec)
    return tab, nonfinite


def chain_step(name, O, prm, ok, est, H, odo_cur, odo_prev, last, last_cov, fitness, score_thre):
    if name == "oracle":
        mo, pr = O.predict(odo_cur, odo_prev, last)
    else:
        m = replay.calMotion(Pose2D(*odo_cur), Pose2D(*odo_prev))
        mo, pr = pose3(m), pose3(replay.calPredPose(m, Pose2D(*last)))
    return FUSERS[name](O, prm, ok, est, H, pr, mo, last, last_cov, fitness, 1, score_thre)


def measure_chain(z, O, name):
    """The 60 steps with the restatement's OWN fused pose and covariance fed back -> [[fused, cov] per step]."""
    odo, last, last_cov, out = z["chain_odo"], z["chain_odo"][0].copy(), np.zeros(9), []
    for k in range(len(z["chain_ok"])):
        f, c = chain_step(name, O, z["chain_prm"], int(z["chain_ok"][k]), z["chain_est"][k], z["chain_H"][k], odo[k + 1], odo[k],
                          last, last_cov, float(z["chain_fitness"][k]), float(z["score_thre"]))
        out.append(list(fuse_errors(f, c, z["chain_fused_ref"][k], z["chain_cov_ref"][k])))
        last, last_cov = f, c
    return out


@pytest.mark.parametrize("name", RESTATEMENTS)
def test_fusion_against_the_references_posefuser(z, oracle, name):
    """PoseFuser::fusePose / calOdometryCovariance (src/PoseFuser.cpp:3-61) behind the accept test: per condition-number
    decade of the Hessian, `fused` and `cov` within 4 x the measured difference ("front-end pins";
    tests/front_ref_bounds.py).  Where the reference's output is not finite (Qmat + cov_hat singular) the restatement's
    is not either, entry by entry for the oracle; numpy's inverse refuses or fills the whole matrix."""
    tab, nonfinite = measure_fusion(z, oracle, name)
    assert sorted(tab) == sorted(FB.FUSION[name]), (sorted(tab), sorted(FB.FUSION[name]))
    for dec in sorted(tab):
        bf, bc = FB.fusion_bound(name, dec)
        print("fusion %-6s decade %2d: fused %.3g (bound %.3g)  cov %.3g (bound %.3g)" % (name, dec, tab[dec][0], bf, tab[dec][1], bc))
    for dec in sorted(tab):
        bf, bc = FB.fusion_bound(name, dec)
        assert tab[dec][0] <= bf and tab[dec][1] <= bc, (name, dec, tab[dec], bf, bc)
    assert len(nonfinite) == int(z["fuse_nonfinite"].sum())
    for i, f, c, f_ref, c_ref in nonfinite:
        if name == "oracle":
            assert np.array_equal(np.isfinite(f), np.isfinite(f_ref)) and np.array_equal(np.isfinite(c), np.isfinite(c_ref)), i
        else:
            assert not np.isfinite(c).all() and not np.isfinite(f).all(), i


@pytest.mark.parametrize("name", RESTATEMENTS)
def test_chained_run_against_the_reference_step_by_step(z, oracle, name):
    """60 consecutive steps of ScanMatcher::matchScan's filter (src/ScanMatcher.cpp:27-32,50-67) with the restatement's
    own cov and fusedPose fed back as lastCov / lastPose: per step within 4 x the measured difference."""
    got = measure_chain(z, oracle, name)
    worst = np.array(got).max(0)
    print("chain %-6s: largest fused %.3g, cov %.3g over %d steps" % (name, worst[0], worst[1], len(got)))
    assert len(got) == len(FB.CHAIN[name]) == 60
    for k, (ef, ec) in enumerate(got):
        bf, bc = FB.chain_bound(name, k)
        assert ef <= bf and ec <= bc, (name, k, ef, bf, ec, bc)


# ---- the fixture is what the reference produces today -----------------------------------------------------------------
def _front_ref():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_front_ref_golden as G
    if not G.have_reference():
        pytest.skip("the reference tree is only in the build container")
    return G


def test_fixture_regenerates_from_the_reference_tree(z, tmp_path):
    """In the build container: build oracle/_ref/libfront_ref.so from the reference's sources again and regenerate
    every vector: the committed arrays, byte for byte -- and, built by the same compiler, the committed file."""
    G = _front_ref()
    arrays = G.generate()
    assert sorted(arrays) == sorted(z.files)
    same_build = all(str(arrays[k]) == str(z[k]) for k in ("built_compiler", "built_flags"))
    for k in z.files:
        if k.startswith("built_") and not same_build:
            continue
        a = np.asanyarray(arrays[k])
        assert a.dtype == z[k].dtype and a.shape == z[k].shape and a.tobytes() == z[k].tobytes(), k
    if same_build:
        G.write_npz(str(tmp_path / "again.npz"), arrays)
        assert open(tmp_path / "again.npz", "rb").read() == open(GOLD, "rb").read()


if __name__ == "__main__":
    from oracle import ndt_oracle as O_
    O_.build()
    z_ = np.load(GOLD)
    print("FUSION = {")
    for n_ in RESTATEMENTS:
        t_, _ = measure_fusion(z_, O_, n_)
        print("    %r: {%s}," % (n_, ", ".join("%d: (%.3g, %.3g)" % (d, t_[d][0], t_[d][1]) for d in sorted(t_))))
    print("}\nCHAIN = {")
    for n_ in RESTATEMENTS:
        c_ = measure_chain(z_, O_, n_)
        print("    %r: [%s]," % (n_, ", ".join("(%.3g, %.3g)" % (a, b) for a, b in c_)))
    print("}")
