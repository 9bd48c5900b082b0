#!/usr/bin/env python3
"""Generates tests/golden/front_ref_golden.npz: outputs of the reference's OWN front-end sources -- src/Pose2D.cpp,
src/MyUtil.cpp, src/PoseFuser.cpp and src/ScanPointResampler.cpp with their headers, compiled here with plain g++
(-O2 -ffp-contract=off, no -march: the reference's CMakeLists sets no optimisation or FMA flags) behind the driver
make_front_ref_golden.cpp -- for the rows either side of the match: odometry prediction and EKF fusion (SURVEY.md 8f
row f2), the scan resampler (f4) and growMap's scan-to-map transform.  Unlike front_golden.npz these ARE outputs of the
reference; tests/test_front_ref_pins.py holds every restatement in the tree against them and
tests/test_gpu_front_ref_pins.py the four device entry points.

Build-container only: the reference tree does not exist where the GPU tests run and nothing of it travels -- what is
committed are inputs and the reference's outputs (data), this script, the driver and its ros/ros.h stand-in (ours).

Three steps of the chain have their source in files that need PCL, so the DRIVER does them, one line each, with the
reference's vendored Eigen; they are NOT the reference's compiled code:
  * Qmat = (-H3).inverse() * coeNDTCov                                         (src/PoseEstimator.cpp:57-64)
  * fusePose, or calOdometryCovariance + fusedPose = predPose, by a `successful` flag passed in
                                                                                (src/ScanMatcher.cpp:50-66)
  * the double -> float conversion of a map-frame point                        (src/ScanMatcher.cpp:100-101, src/PointCloudMap.cpp:59-60)
and, since a match record carries the estimated yaw in radians, estPose.setPose(tx, ty, RAD2DEG(theta))
(src/PoseEstimator.cpp:36, with the reference's own macro).

Sections (inputs `*_in` or named, reference outputs `*_ref`):
  ang_*     MyUtil::add_angle / sub_angle: sums and differences at +-180 and one ulp either side, headings outside
            [-180, 180) (one wrap only), random pairs
  rmat_*    Pose2D::calRmat at the edge headings
  pt_*      Pose2D::globalPoint (both overloads) / relativePoint
  pred_*    calMotion + calPredPose chained (src/ScanMatcher.cpp:27-32), calGlobalMotion
  fuse_*    one step behind the match, both branches, three parameter sets, Hessians of condition number 1 .. 1e10,
            zero lastCov, zero motion, singular Qmat + cov_hat (non-finite outputs recorded), unsymmetric lastCov
  chain_*   60 consecutive steps with cov and fusedPose fed back, accepted and rejected steps mixed
  rs_*      resamplePoints: per vector the input points followed by the reference's output points in ONE array (kept
            points repeat their input bit for bit, which the file's compression then finds); 32 synthetic 1081-beam
            scans, inputs on a 2^-10 m grid stored as int16: full outputs of the first RS_SYN_FULL, counts and SHA-256
            of the float64 / float32 output bytes of all (the outputs are incompressible doubles; the file stays below
            the largest fixture of this directory)
  gm_*      growMap's transform of resampled scans at 24 poses, float64 and the map cloud's float32

resamplePoints does not terminate on some parameter sets (space == 0 < space_thre); none is in the fixture, and every
call runs in a child process under a time and memory cap, so the generator cannot hang.
"""
import ctypes as C
import hashlib
import io
import math
import multiprocessing
import os
import subprocess
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REF = "/root/reference"
SO = os.path.join(ROOT, "oracle", "_ref", "libfront_ref.so")
OUT = os.path.join(HERE, "front_ref_golden.npz")
EDGE_TH = [0.0, 90.0, -90.0, 180.0, -180.0, 179.999999, 1e-9, 359.5]
LAUNCH_FUSE = (0.5, 0.1, 0.5, 1.0)          # delTime, coeVel, coeOmega, coeNDTCov (ndt_mapping.launch)
FUSE_SETS = [LAUNCH_FUSE, (0.1, 0.3, 0.05, 0.7), (1.0, 0.02, 1.5, 2.5)]
SCORE_THRE = 0.5
RS_PAIRS = [(0.05, 0.25), (0.05, 0.05), (0.1, 0.05), (0.0, 0.0), (0.03, 0.2)]    # tests/test_gpu_resample.py: all end
RS_SYN, RS_SYN_FULL, RS_GRID = 32, 4, 1024.0
RS_CAP_SECONDS = 30


def have_reference():
    return os.path.isdir(os.path.join(REF, "include", "ndt_slam")) and os.path.isdir(os.path.join(REF, "src"))


def build_front_ref():
    """make -C oracle _ref/libfront_ref.so (output only into oracle/_ref/)."""
    if not have_reference():
        raise SystemExit("the reference tree is not here (%s): run this in the build container" % REF)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "_ref/libfront_ref.so"], stdout=subprocess.DEVNULL)
    return SO


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Ref:
    """ctypes face of oracle/_ref/libfront_ref.so."""

    def __init__(self, so=None):
        self.L = L = C.CDLL(so or build_front_ref())
        vp, d = C.c_void_p, C.c_double
        L.fr_add_angle.restype = L.fr_sub_angle.restype = d
        L.fr_add_angle.argtypes = L.fr_sub_angle.argtypes = [d, d]
        L.fr_cal_rmat.argtypes = [d, vp]
        for f in (L.fr_cal_motion, L.fr_cal_global_motion, L.fr_cal_pred_pose, L.fr_global_point, L.fr_global_point_out,
                  L.fr_relative_point):
            f.argtypes = [vp] * 3
        L.fr_predict.argtypes = [vp] * 5
        L.fr_odo_cov.argtypes = [vp] * 5
        L.fr_fuse_step.restype = C.c_int
        L.fr_fuse_step.argtypes = [vp, C.c_int] + [vp] * 8
        L.fr_resample.restype = C.c_long
        L.fr_resample.argtypes = [d, d, vp, C.c_long, vp, C.c_long]
        L.fr_grow_map.argtypes = [vp, vp, C.c_long, vp, vp]
        L.fr_build_info.argtypes = [vp, vp, vp]

    def build_info(self):
        v, c, f = (C.c_int * 3)(), C.c_char_p(), C.c_char_p()
        self.L.fr_build_info(v, C.byref(c), C.byref(f))
        return tuple(v), c.value.decode(), f.value.decode()

    def add_angle(self, a, b):
        return self.L.fr_add_angle(float(a), float(b))

    def sub_angle(self, a, b):
        return self.L.fr_sub_angle(float(a), float(b))

    def rmat(self, th):
        o = np.zeros(4)
        self.L.fr_cal_rmat(float(th), _p(o))
        return o

    def _3(self, fn, a, b, n=3):
        a, b, o = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64), np.zeros(n)
        fn(_p(a), _p(b), _p(o))
        return o

    def cal_motion(self, cur, prev):
        return self._3(self.L.fr_cal_motion, cur, prev)

    def cal_global_motion(self, cur, prev):
        return self._3(self.L.fr_cal_global_motion, cur, prev)

    def cal_pred_pose(self, motion, last):
        return self._3(self.L.fr_cal_pred_pose, motion, last)

    def global_point(self, pose, p):
        return self._3(self.L.fr_global_point, pose, p, 2)

    def global_point_out(self, pose, p):
        return self._3(self.L.fr_global_point_out, pose, p, 2)

    def relative_point(self, pose, p):
        return self._3(self.L.fr_relative_point, pose, p, 2)

    def predict(self, cur, prev, last):
        a = [np.ascontiguousarray(v, np.float64) for v in (cur, prev, last)]
        mo, pr = np.zeros(3), np.zeros(3)
        self.L.fr_predict(_p(a[0]), _p(a[1]), _p(a[2]), _p(mo), _p(pr))
        return mo, pr

    def odo_cov(self, prm, motion, last, last_cov):
        a = [np.ascontiguousarray(v, np.float64).ravel() for v in (prm, motion, last, last_cov)]
        o = np.zeros(9)
        self.L.fr_odo_cov(_p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(o))
        return o.reshape(3, 3)

    def fuse_step(self, prm, ok, est, H, pred, motion, last, last_cov):
        a = [np.ascontiguousarray(v, np.float64).ravel() for v in (prm, est, H, pred, motion, last, last_cov)]
        fused, cov = np.zeros(3), np.zeros(9)
        self.L.fr_fuse_step(_p(a[0]), int(ok), _p(a[1]), _p(a[2]), _p(a[3]), _p(a[4]), _p(a[5]), _p(a[6]), _p(fused), _p(cov))
        return fused, cov.reshape(3, 3)

    def resample_unguarded(self, xy, space, space_thre):
        xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        k_max = 1 if space_thre <= space else int(math.floor(space_thre / space)) + 2
        cap = len(xy) * k_max + 1
        out = np.zeros((cap, 2))
        m = self.L.fr_resample(float(space), float(space_thre), _p(xy), len(xy), _p(out), cap)
        assert m <= cap, (m, cap)
        return out[:m].copy()

    def grow_map(self, pose, xy):
        xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        pose = np.ascontiguousarray(pose, np.float64)
        o64, o32 = np.zeros((len(xy), 2)), np.zeros((len(xy), 2), np.float32)
        self.L.fr_grow_map(_p(pose), _p(xy), len(xy), _p(o64), _p(o32))
        return o64, o32


# ---- resamplePoints under a cap: a child process, a time limit per scan, an address-space limit -------------------
_WORKER_REF = None


def _worker_init(so):
    global _WORKER_REF
    import resource
    with open("/proc/self/statm") as f:                       # what the parent had mapped already, plus 4 GiB for the walk
        now = int(f.read().split()[0]) * resource.getpagesize()
    resource.setrlimit(resource.RLIMIT_AS, (now + (4 << 30), now + (4 << 30)))
    _WORKER_REF = Ref(so)


def _worker_resample(xy, space, space_thre):
    return _WORKER_REF.resample_unguarded(xy, space, space_thre)


class GuardedResampler:
    def __init__(self, so):
        self.pool = multiprocessing.get_context("fork").Pool(1, initializer=_worker_init, initargs=(so,))

    def __call__(self, xy, space, space_thre):
        if not (space > 0 or space_thre <= space):
            raise ValueError("resamplePoints never ends with space == 0 < space_thre: not a fixture vector")
        job = self.pool.apply_async(_worker_resample, (np.asarray(xy, np.float64), space, space_thre))
        try:
            return job.get(timeout=RS_CAP_SECONDS)
        except multiprocessing.TimeoutError:
            self.pool.terminate()
            raise SystemExit("resamplePoints did not end within %d s (space %r, space_thre %r)" % (RS_CAP_SECONDS, space, space_thre))

    def close(self):
        self.pool.terminate()
        self.pool.join()


# ---- the vectors ---------------------------------------------------------------------------------------------------
def angle_pairs(rng):
    up, dn = lambda v: np.nextafter(v, np.inf), lambda v: np.nextafter(v, -np.inf)
    p = []
    for s in (180.0, -180.0):
        for t in (s, up(s), dn(s)):
            for a in (0.0, 35.25, -170.0, 179.5, 90.0):
                p.append((a, t - a))          # add: a + (t - a); sub sees the same pair as a difference
                p.append((t + a, a))          # sub: (t + a) - a
                p.append((t, 0.0))
    p += [(540.0, 0.0), (-725.0, 0.0), (540.0, 10.0), (-725.0, -10.0), (359.5, 0.5), (359.5, -0.5), (720.0, 720.0),
          (-180.0, -180.0), (180.0, 180.0), (179.999999, 1e-6), (179.999999, 1e-9), (-180.0, 1e-9), (-180.0, -1e-9),
          (0.0, 0.0), (-0.0, 0.0), (1e-9, -1e-9), (90.0, 90.0), (-90.0, -90.0), (90.0, -270.0), (170.0, 10.0), (-170.0, -10.0)]
    p += [(a, b) for a in EDGE_TH for b in EDGE_TH]
    p += [tuple(v) for v in rng.uniform(-400, 400, (64, 2))]
    return np.array(p, dtype=np.float64)


def predict_inputs(rng):
    """[N, 9]: cur, prev, last."""
    B = 200
    prev = np.column_stack([rng.uniform(-50, 50, (B, 2)), rng.uniform(-180, 180, B)])
    cur = np.column_stack([prev[:, :2] + rng.uniform(-1, 1, (B, 2)), rng.uniform(-180, 180, B)])
    last = np.column_stack([rng.uniform(-50, 50, (B, 2)), rng.uniform(-180, 180, B)])
    last[:4, 2] = [179.9, -180.0, 170.0, -179.5]; cur[:4, 2] = [-179.0, 179.0, 10.0, 0.0]; prev[:4, 2] = [179.0, -179.0, 0.0, 0.4]   # tests/test_gpu_fuse.py:32
    rows = [np.column_stack([cur, prev, last])]
    extra = []

    def pose(th=None, scale=50.0):
        return np.array([*rng.uniform(-scale, scale, 2), rng.uniform(-180, 180) if th is None else th])
    for _ in range(4):                                        # zero motion
        q = pose()
        extra.append(np.concatenate([q, q, pose()]))
    for _ in range(4):                                        # pure rotation
        q = pose()
        c = q.copy(); c[2] = rng.uniform(-180, 180)
        extra.append(np.concatenate([c, q, pose()]))
    for step in (1e-9, 1e4):                                  # cancellation in cur - prev and in cp*dx + sp*dy
        for _ in range(4):
            q = pose(scale=50.0 if step < 1 else 1e4)
            c = q + np.array([*(rng.uniform(-1, 1, 2) * step), rng.uniform(-5, 5)])
            extra.append(np.concatenate([c, q, pose(scale=50.0 if step < 1 else 1e4)]))
    for th in EDGE_TH:                                        # edge headings of the previous odometry pose and of the last pose
        q = pose(th)
        c = q + np.array([*rng.uniform(-1, 1, 2), rng.uniform(-3, 3)])
        extra.append(np.concatenate([c, q, pose()]))
        q2 = pose()
        c2 = q2 + np.array([*rng.uniform(-1, 1, 2), rng.uniform(-3, 3)])
        extra.append(np.concatenate([c2, q2, pose(th)]))
    for th_c, th_p, th_l in ((540.0, 10.0, 0.0), (-725.0, 0.0, 30.0), (10.0, 540.0, -170.0), (0.0, -725.0, 179.0),
                             (179.0, -179.0, 540.0), (-179.0, 179.0, -725.0), (180.0, 0.0, 0.0), (0.0, 180.0, 0.0),
                             (0.0, 0.0, 180.0), (-180.0, 0.0, -180.0), (90.0, -90.0, 90.0), (-90.0, 90.0, 90.0)):
        q = pose(th_p)
        c = q + np.array([*rng.uniform(-1, 1, 2), 0.0]); c[2] = th_c
        extra.append(np.concatenate([c, q, pose(th_l)]))
    rows.append(np.array(extra))
    return np.concatenate(rows)


def spd(rng, scale=1.0):
    A = rng.normal(size=(3, 3))
    return (A @ A.T + 0.1 * np.eye(3)) * scale


def hessian_with_condition(rng, cond, scale):
    """-(V diag(1, sqrt(cond), cond) V^T) * scale: the match's Hessian is negative definite at a maximum."""
    V, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return -((V * np.array([1.0, math.sqrt(cond), cond])) @ V.T) * scale


def wrap_rad(a):
    return (a + math.pi) % (2 * math.pi) - math.pi


def fusion_vectors(R, rng):
    rows = []

    def add(prm, ok, cur, prev, last, last_cov, H, kind, est=None, reject_by=0):
        mo, pr = R.predict(cur, prev, last)
        if est is None:
            est = np.array([pr[0] + rng.normal(0, 0.05), pr[1] + rng.normal(0, 0.05), wrap_rad(math.radians(pr[2] + rng.normal(0, 1.0)))])
        # how the record tells the accept test of src/ScanMatcher.cpp:50: cost <= SCORE_THRE, or above it, or not converged
        fitness, conv = (0.1, 1) if ok else ((0.7, 1) if reject_by == 0 else (0.1, 0))
        rows.append(dict(prm=prm, ok=ok, est=est, H=np.asarray(H, float).ravel(), pred=pr, motion=mo, last=np.asarray(last, float),
                         last_cov=np.asarray(last_cov, float).ravel(), fitness=fitness, converged=conv, kind=kind))

    def poses(th_last=None, zero=False):
        prev = np.array([*rng.uniform(-50, 50, 2), rng.uniform(-180, 180)])
        cur = prev.copy() if zero else prev + np.array([*rng.uniform(-0.6, 0.6, 2), rng.uniform(-6, 6)])
        last = np.array([*rng.uniform(-50, 50, 2), rng.uniform(-180, 180) if th_last is None else th_last])
        return cur, prev, last
    for s, prm in enumerate(FUSE_SETS):                                   # kind 0: random, both branches, every set
        for k in range(28):
            cur, prev, last = poses()
            add(prm, int(k < 20), cur, prev, last, spd(rng, 1e-3), -spd(rng, rng.uniform(1, 1e4)), 0, reject_by=k % 2)
    for dec in range(11):                                                 # kind 1: condition number 10^dec
        for k in range(3):
            cur, prev, last = poses()
            add(LAUNCH_FUSE, 1, cur, prev, last, spd(rng, 1e-3), hessian_with_condition(rng, 10.0 ** dec, 10.0 ** rng.uniform(0, 3)), 1)
    for k in range(4):                                                    # kind 2: lastCov all zeros (the second scan of a run)
        cur, prev, last = poses()
        add(LAUNCH_FUSE, int(k < 2), cur, prev, last, np.zeros((3, 3)), -spd(rng, 100.0), 2)
    for k in range(4):                                                    # kind 3: zero motion: Mmat == 0, cov_hat == lastCov
        cur, prev, last = poses(zero=True)
        add(LAUNCH_FUSE, int(k < 2), cur, prev, last, spd(rng, 1e-3), -spd(rng, 100.0), 3)
    for k in range(4):                                                    # kind 4: an unsymmetric lastCov
        cur, prev, last = poses()
        add(FUSE_SETS[k % 3], int(k < 3), cur, prev, last, spd(rng, 1e-3) + np.triu(rng.normal(size=(3, 3)), 1) * 1e-4, -spd(rng, 100.0), 4)
    for th in EDGE_TH:                                                    # kind 5: edge headings of the last pose
        cur, prev, last = poses(th_last=th)
        add(LAUNCH_FUSE, 1, cur, prev, last, spd(rng, 1e-3), -spd(rng, 100.0), 5)
    for th_l, d_est in ((179.9, 0.3), (-179.9, -0.3)):                    # kind 6: estimate and prediction either side of +-180
        prev = np.array([1.0, 2.0, 10.0]); cur = np.array([1.2, 2.1, 10.0]); last = np.array([-3.0, 4.0, th_l])
        mo, pr = R.predict(cur, prev, last)
        est = np.array([pr[0] + 0.02, pr[1] - 0.01, wrap_rad(math.radians(pr[2] + d_est))])
        add(LAUNCH_FUSE, 1, cur, prev, last, spd(rng, 1e-3), -spd(rng, 100.0), 6, est=est)
    # kind 7: Qmat + cov_hat singular -> inf / nan in the reference.  (a) zero motion, lastCov = diag(a, a, 1/2) and
    # -H = diag(1, 1, -2): Qmat = diag(1, 1, -1/2) exactly and the sum has a zero on its diagonal; (b) a singular H.
    q = np.array([3.0, -2.0, 40.0])
    add(LAUNCH_FUSE, 1, q, q, np.array([1.0, 1.0, 20.0]), np.diag([0.25, 0.25, 0.5]), np.diag([-1.0, -1.0, 2.0]), 7)
    cur, prev, last = poses()
    add(LAUNCH_FUSE, 1, cur, prev, last, spd(rng, 1e-3), -np.ones((3, 3)), 7)
    return rows


def chain_inputs(rng, n=60):
    """Odometry of a drive on an arc that crosses +-180, the accept flags and the match of every step."""
    odo = np.zeros((n + 1, 3))
    odo[0] = (2.0, -1.0, 168.0)
    for k in range(1, n + 1):
        a = math.radians(odo[k - 1, 2])
        step = 0.3 + 0.05 * math.sin(k)
        odo[k] = (odo[k - 1, 0] + step * math.cos(a), odo[k - 1, 1] + step * math.sin(a), odo[k - 1, 2] + 3.0 + 0.2 * math.cos(k))
        if odo[k, 2] >= 180.0:
            odo[k, 2] -= 360.0
    ok = np.array([0 if (k % 5 == 3 or k in (10, 11, 12)) else 1 for k in range(n)], np.int32)
    noise = np.column_stack([rng.normal(0, 0.02, (n, 2)), rng.normal(0, 0.3, n)])
    H = np.array([-spd(rng, 10.0 ** rng.uniform(2, 5)) for _ in range(n)]).reshape(n, 9)
    return odo, ok, noise, H


def resample_vectors(rng):
    """-> list of (space, space_thre, scan[n,2], tag).  Ordered by scan, then by parameter pair: the random walks are
    the same for every pair, and lie next to each other in the file."""
    from ndt_slam_amd import synth
    from test_resample_capacity import adversarial_scans
    per_pair = [adversarial_scans(sp, th, np.random.default_rng(11)) for sp, th in RS_PAIRS]
    vec = []
    for i in range(len(per_pair[0])):
        for (sp, th), scans in zip(RS_PAIRS, per_pair):
            vec.append((sp, th, np.asarray(scans[i], np.float64), 0))
    for sp, th in ((0.05, 0.25), (0.1, 0.05), (0.05, 0.05)):                 # hand-made edges, tag 1
        r = max(sp, th)                                                      # the device's resync length
        below = np.nextafter(r, 0.0)
        edge = [
            np.zeros((0, 2)), np.array([[1.0, 2.0]]), np.array([[0.0, 0.0], [0.3, 0.0]]), np.array([[0.0, 0.0], [0.01, 0.0]]),
            np.repeat(np.array([[0.5, -0.25], [0.5, -0.2], [0.9, -0.2]]), 5, axis=0),                  # repeated points: L == 0
            np.column_stack([np.zeros(40), np.arange(40) * sp]),                                      # steps exactly `space`
            np.column_stack([np.arange(40) * th, np.zeros(40)]),                                      # steps exactly `space_thre`
            np.array([[0.0, 0.0], [0.02, 0.0], [0.02, r], [0.04, r], [0.04, r + below], [0.06, r + below],
                      [0.06 + r, r + below], [0.06 + r + below, r + below], [0.06 + r + below, 2 * r + below]]),   # a step of exactly max(space, space_thre), one an ulp below it, with dis > 0 in front
            np.array([[0.0, 0.0], [0.0, below], [0.0, below + r], [0.01, below + r], [0.01, below + r + below]]),
            np.column_stack([1000.0 + np.arange(120) * 0.013, -1000.0 + 0.4 * np.sin(np.arange(120) * 0.1)]),   # near 1e3 m
            np.column_stack([-999.5 + rng.normal(0, 0.02, 150).cumsum(), 1000.25 + rng.normal(0, 0.02, 150).cumsum()]),
        ]
        vec += [(sp, th, e, 1) for e in edge]
    recs, _ = synth.replay_records(n_frames=RS_SYN, n_beams=1081)
    for r in recs:                                                           # tag 2: on the 2^-10 m grid (int16 in the file)
        g = np.round(np.asarray(r["front"], np.float64) * RS_GRID)
        assert np.abs(g).max() < 32767
        vec.append((0.05, 0.25, g / RS_GRID, 2))
    return vec


def generate(R=None):
    """-> dict of arrays: the whole fixture (no file is written)."""
    R = R or Ref()
    ev, comp, flags = R.build_info()
    out = {"eigen_version": np.array(ev), "built_compiler": np.array(comp), "built_flags": np.array(flags),
           "score_thre": np.float64(SCORE_THRE)}
    rng = np.random.Generator(np.random.Philox(2024))

    ap = angle_pairs(rng)
    out.update(ang_in=ap, ang_add_ref=np.array([R.add_angle(a, b) for a, b in ap]), ang_sub_ref=np.array([R.sub_angle(a, b) for a, b in ap]))
    rth = np.array(EDGE_TH + [-179.999999, 45.0, -135.0, 540.0, -725.0, 30.0, 1e-300])
    out.update(rmat_in=rth, rmat_ref=np.array([R.rmat(t) for t in rth]))

    pp = [np.array([*rng.uniform(-30, 30, 2), th]) for th in EDGE_TH for _ in range(4)]
    pp += [np.array([*rng.uniform(-1e3, 1e3, 2), rng.uniform(-180, 180)]) for _ in range(32)]
    pp = np.array(pp)
    pts = rng.uniform(-30, 30, (len(pp), 2))
    pts[::4] = rng.uniform(-1e3, 1e3, (len(pts[::4]), 2))
    out.update(pt_pose_in=pp, pt_in=pts, pt_global_ref=np.array([R.global_point(a, b) for a, b in zip(pp, pts)]),
               pt_global_out_ref=np.array([R.global_point_out(a, b) for a, b in zip(pp, pts)]),
               pt_relative_ref=np.array([R.relative_point(a, b) for a, b in zip(pp, pts)]))

    pi = predict_inputs(rng)
    mo, pr = zip(*[R.predict(v[0:3], v[3:6], v[6:9]) for v in pi])
    mo, pr = np.array(mo), np.array(pr)
    for v, m_, p_ in zip(pi, mo, pr):                 # the chained call is the two calls one after the other
        assert R.cal_motion(v[0:3], v[3:6]).tobytes() == m_.tobytes() and R.cal_pred_pose(m_, v[6:9]).tobytes() == p_.tobytes()
    out.update(pred_in=pi, pred_motion_ref=mo, pred_pred_ref=pr,
               pred_gmotion_ref=np.array([R.cal_global_motion(v[0:3], v[3:6]) for v in pi]))

    fv = fusion_vectors(R, rng)
    fused, cov = zip(*[R.fuse_step(v["prm"], v["ok"], v["est"], v["H"], v["pred"], v["motion"], v["last"], v["last_cov"]) for v in fv])
    fused, cov = np.array(fused), np.array(cov).reshape(-1, 9)
    for v, c in zip(fv, cov):                         # the rejected branch is calOdometryCovariance alone
        if not v["ok"]:
            assert R.odo_cov(v["prm"][:3], v["motion"], v["last"], v["last_cov"]).tobytes() == c.tobytes()
    nonfinite = ~(np.isfinite(fused).all(1) & np.isfinite(cov).all(1))
    assert 0 < nonfinite.sum() < 0.02 * len(fv), (nonfinite.sum(), len(fv))
    assert set(np.nonzero(nonfinite)[0]) == {i for i, v in enumerate(fv) if v["kind"] == 7}
    Hs = np.array([v["H"] for v in fv])
    out.update(fuse_prm=np.array([v["prm"] for v in fv]), fuse_ok=np.array([v["ok"] for v in fv], np.int32),
               fuse_est=np.array([v["est"] for v in fv]), fuse_H=Hs, fuse_pred=np.array([v["pred"] for v in fv]),
               fuse_motion=np.array([v["motion"] for v in fv]), fuse_last=np.array([v["last"] for v in fv]),
               fuse_lastcov=np.array([v["last_cov"] for v in fv]), fuse_fitness=np.array([v["fitness"] for v in fv]),
               fuse_converged=np.array([v["converged"] for v in fv], np.int32), fuse_kind=np.array([v["kind"] for v in fv], np.int32),
               fuse_cond=np.array([np.linalg.cond(h.reshape(3, 3)) for h in Hs]), fuse_fused_ref=fused, fuse_cov_ref=cov,
               fuse_nonfinite=nonfinite)

    odo, cok, noise, cH = chain_inputs(rng)
    n = len(cok)
    last, last_cov = odo[0].copy(), np.zeros((3, 3))      # the first scan: its odometry pose, zero covariance (src/ScanMatcher.cpp:11-17)
    c_mo, c_pr, c_est, c_fu, c_cov = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 9))
    for k in range(n):
        c_mo[k], c_pr[k] = R.predict(odo[k + 1], odo[k], last)
        c_est[k] = (c_pr[k, 0] + noise[k, 0], c_pr[k, 1] + noise[k, 1], wrap_rad(math.radians(c_pr[k, 2] + noise[k, 2])))
        f, cv = R.fuse_step(LAUNCH_FUSE, cok[k], c_est[k], cH[k], c_pr[k], c_mo[k], last, last_cov)
        c_fu[k], c_cov[k] = f, cv.ravel()
        last, last_cov = f, cv
    assert np.isfinite(c_fu).all() and np.isfinite(c_cov).all()
    out.update(chain_prm=np.array(LAUNCH_FUSE), chain_odo=odo, chain_ok=cok, chain_est=c_est, chain_H=cH,
               chain_fitness=np.where(cok == 1, 0.1, 0.7), chain_motion_ref=c_mo, chain_pred_ref=c_pr, chain_fused_ref=c_fu,
               chain_cov_ref=c_cov)

    rs = GuardedResampler(SO)
    try:
        vec = resample_vectors(rng)
        outs = [rs(xy, sp, th) for sp, th, xy, _ in vec]
    finally:
        rs.close()
    small = [i for i, v in enumerate(vec) if v[3] != 2]
    syn = [i for i, v in enumerate(vec) if v[3] == 2]
    xy, off = [], [0]
    for i in small:                                    # per vector: input points, then the reference's output points
        xy += [vec[i][2].reshape(-1, 2), outs[i]]
        off += [off[-1] + len(vec[i][2]), off[-1] + len(vec[i][2]) + len(outs[i])]
    out.update(rs_xy=np.concatenate(xy), rs_off=np.array(off, np.int64),
               rs_space=np.array([vec[i][0] for i in small]), rs_thre=np.array([vec[i][1] for i in small]),
               rs_tag=np.array([vec[i][3] for i in small], np.int32))
    syn_in = np.concatenate([vec[i][2] for i in syn])
    out.update(rs_syn_in_i16=np.round(syn_in * RS_GRID).astype(np.int16), rs_syn_grid=np.float64(RS_GRID),
               rs_syn_in_off=np.concatenate([[0], np.cumsum([len(vec[i][2]) for i in syn])]).astype(np.int64),
               rs_syn_count_ref=np.array([len(outs[i]) for i in syn], np.int64),
               rs_syn_sha64_ref=np.array([hashlib.sha256(outs[i].tobytes()).hexdigest() for i in syn]),
               rs_syn_sha32_ref=np.array([hashlib.sha256(outs[i].astype(np.float32).tobytes()).hexdigest() for i in syn]),
               rs_syn_full_ref=np.concatenate([outs[i] for i in syn[:RS_SYN_FULL]]))
    assert np.array_equal(out["rs_syn_in_i16"].astype(np.float64) / RS_GRID, syn_in)

    # growMap: slices of resampled scans (the reference's own outputs) at 24 poses
    src = [outs[i] for i in syn[:8]] + [outs[i] for i in small if len(outs[i]) >= 40][:16]
    gp = np.column_stack([rng.uniform(-30, 30, (24, 2)), rng.uniform(-180, 180, 24)])
    gp[0] = (0.0, 0.0, 0.0); gp[1] = (1.5, -2.0, 90.0); gp[2] = (0.0, 0.0, -180.0); gp[3] = (1000.0, -1000.0, 33.0)
    gp[4] = (-999.75, 1e3, -90.0); gp[5] = (3.0, 4.0, 180.0); gp[6] = (250.0, -750.5, 179.999999); gp[7] = (-5.0, 5.0, 359.5)
    gin = [s[:: max(1, len(s) // 96)][:96] for s in src]
    g64, g32 = zip(*[R.grow_map(p, s) for p, s in zip(gp, gin)])
    out.update(gm_pose_in=gp, gm_xy_in=np.concatenate(gin), gm_off=np.concatenate([[0], np.cumsum([len(s) for s in gin])]).astype(np.int64),
               gm_out64_ref=np.concatenate(g64), gm_out32_ref=np.concatenate(g32))
    return out


def write_npz(path, arrays):
    """A .npz (numpy.load reads it) whose bytes depend on the arrays alone: fixed member dates, sorted names."""
    with zipfile.ZipFile(path, "w") as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    arrays = generate()
    write_npz(OUT, arrays)
    size = os.path.getsize(OUT)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith(".npz") and f != "front_ref_golden.npz")
    print("wrote", OUT, size, "bytes (largest other fixture %d); %s, %s, Eigen %s" %
          (largest, arrays["built_compiler"], arrays["built_flags"], tuple(arrays["eigen_version"])))
    print("  %d angle pairs, %d predictions, %d fusion vectors (%d non-finite), %d chained steps, %d + %d resampler vectors, %d growMap poses"
          % (len(arrays["ang_in"]), len(arrays["pred_in"]), len(arrays["fuse_ok"]), int(arrays["fuse_nonfinite"].sum()),
             len(arrays["chain_ok"]), len(arrays["rs_space"]), len(arrays["rs_syn_count_ref"]), len(arrays["gm_pose_in"])))
    assert size <= largest, "the fixture outgrew the largest one of tests/golden"


if __name__ == "__main__":
    main()
