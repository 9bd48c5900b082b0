// make_front_ref_golden.cpp -- the reference's OWN front-end sources run on chosen vectors, to pin this project's
// restatements of them and the device kernels behind them (rows f2 and f4 of SURVEY.md 8f and growMap's transform).
//
// TEST INFRASTRUCTURE, build container only (oracle/Makefile, rule _ref/libfront_ref.so):
//     g++ -O2 -std=c++14 -ffp-contract=off -fPIC -shared -Itests/golden/front_ref_stubs -Itests/shim_stubs -I$(REF_INC) \
//         tests/golden/make_front_ref_golden.cpp $(REF_SRC)/Pose2D.cpp $(REF_SRC)/MyUtil.cpp $(REF_SRC)/PoseFuser.cpp \
//         $(REF_SRC)/ScanPointResampler.cpp -o oracle/_ref/libfront_ref.so
// The four source files and their headers are reached by those paths only; nothing of them is copied into this
// repository and the library never travels in git (oracle/_ref/ is ignored).  What is committed are its OUTPUTS,
// tests/golden/front_ref_golden.npz (written by make_front_ref_golden.py).
//
// Every function below marshals plain arrays into the reference's types and calls the reference's compiled code:
//   fr_add_angle / fr_sub_angle     MyUtil::add_angle / sub_angle                      (src/MyUtil.cpp:4-23)
//   fr_cal_rmat                     Pose2D::calRmat                                    (include/ndt_slam/Pose2D.h:43-48)
//   fr_cal_motion / fr_cal_global_motion / fr_cal_pred_pose                            (src/Pose2D.cpp:5-37)
//   fr_predict                      calMotion then calPredPose on the same objects, as src/ScanMatcher.cpp:27-32 chains them
//   fr_global_point / fr_global_point_out / fr_relative_point                          (src/Pose2D.cpp:40-59)
//   fr_odo_cov                      PoseFuser::calOdometryCovariance                   (src/PoseFuser.cpp:38-61)
//   fr_fuse_step                    PoseFuser::fusePose or calOdometryCovariance       (src/PoseFuser.cpp:3-61)
//   fr_resample                     ScanPointResampler::resamplePoints                 (src/ScanPointResampler.cpp:4-62)
//   fr_grow_map                     Pose2D::globalPoint on every point of a scan       (src/Pose2D.cpp:55-59)
// Three steps around them have their source in files that need PCL, so they are written HERE, one line each, with the
// vendored Eigen; they are NOT the reference's compiled code (marked "ours" where they stand).
#include <ros/ros.h>              // tests/golden/front_ref_stubs: ros::param::get served from front_ref_params()
#include <iostream>
#include <streambuf>
#include <vector>

#include "ndt_slam/MyUtil.h"
#include "ndt_slam/Pose2D.h"
#include "ndt_slam/PoseFuser.h"
#include "ndt_slam/Scan2D.h"
#include "ndt_slam/ScanPointResampler.h"

#ifndef FRONT_REF_FLAGS
#define FRONT_REF_FLAGS "unknown"
#endif

namespace {

// fusePose prints cov_hat and cov to std::cout on every call (src/PoseFuser.cpp:14-15,27-28): sent nowhere meanwhile.
struct NullBuf : std::streambuf { int overflow(int c) override { return c; } };
struct QuietCout {
  NullBuf nb; std::streambuf *old;
  QuietCout() : old(std::cout.rdbuf(&nb)) {}
  ~QuietCout() { std::cout.rdbuf(old); }
};

Pose2D pose_of(const double *p) { return Pose2D(p[0], p[1], p[2]); }
void put(const Pose2D &p, double *o) { o[0] = p.tx; o[1] = p.ty; o[2] = p.th; }
Eigen::Matrix3d mat_of(const double *m) {
  Eigen::Matrix3d M;
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) M(i, j) = m[3 * i + j];
  return M;
}
void put(const Eigen::Matrix3d &M, double *o) { for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) o[3 * i + j] = M(i, j); }

PoseFuser make_fuser(const double *prm) {          // prm = delTime, coeVel, coeOmega (PoseFuser.h:19-23 reads them)
  std::map<std::string, double> &t = front_ref_params();
  t.clear();
  t["delTime"] = prm[0]; t["coeVel"] = prm[1]; t["coeOmega"] = prm[2];
  return PoseFuser();
}

}  // namespace

extern "C" {

void fr_build_info(int eigen_version[3], const char **compiler, const char **flags) {
  eigen_version[0] = EIGEN_WORLD_VERSION; eigen_version[1] = EIGEN_MAJOR_VERSION; eigen_version[2] = EIGEN_MINOR_VERSION;
  *compiler = __VERSION__;
  *flags = FRONT_REF_FLAGS;
}

double fr_add_angle(double a1, double a2) { return MyUtil::add_angle(a1, a2); }
double fr_sub_angle(double a1, double a2) { return MyUtil::sub_angle(a1, a2); }

void fr_cal_rmat(double th, double *rmat4) {       // row-major Rmat[2][2]
  Pose2D p(0.0, 0.0, th);
  rmat4[0] = p.Rmat[0][0]; rmat4[1] = p.Rmat[0][1]; rmat4[2] = p.Rmat[1][0]; rmat4[3] = p.Rmat[1][1];
}

void fr_cal_motion(const double *cur, const double *prev, double *motion) {
  Pose2D m;
  Pose2D::calMotion(pose_of(cur), pose_of(prev), m);
  put(m, motion);
}

void fr_cal_global_motion(const double *cur, const double *prev, double *motion) {
  Pose2D m;
  Pose2D::calGlobalMotion(pose_of(cur), pose_of(prev), m);
  put(m, motion);
}

void fr_cal_pred_pose(const double *motion, const double *last, double *pred) {
  Pose2D p;
  Pose2D::calPredPose(pose_of(motion), pose_of(last), p);
  put(p, pred);
}

void fr_predict(const double *cur, const double *prev, const double *last, double *motion, double *pred) {
  Pose2D odoMotion, predPose;
  Pose2D::calMotion(pose_of(cur), pose_of(prev), odoMotion);
  Pose2D::calPredPose(odoMotion, pose_of(last), predPose);
  put(odoMotion, motion);
  put(predPose, pred);
}

void fr_global_point(const double *pose, const double *in, double *out) {
  LPoint2D r = pose_of(pose).globalPoint(LPoint2D(0, in[0], in[1]));
  out[0] = r.x; out[1] = r.y;
}

void fr_global_point_out(const double *pose, const double *in, double *out) {
  LPoint2D pi(0, in[0], in[1]), po;
  pose_of(pose).globalPoint(pi, po);
  out[0] = po.x; out[1] = po.y;
}

void fr_relative_point(const double *pose, const double *in, double *out) {
  LPoint2D r = pose_of(pose).relativePoint(LPoint2D(0, in[0], in[1]));
  out[0] = r.x; out[1] = r.y;
}

void fr_odo_cov(const double *prm, const double *motion, const double *last, const double *last_cov, double *cov) {
  PoseFuser pfu = make_fuser(prm);
  Eigen::Matrix3d c;
  pfu.calOdometryCovariance(pose_of(motion), pose_of(last), mat_of(last_cov), c);
  put(c, cov);
}

// One step of ScanMatcher::matchScan behind the match.  prm = delTime, coeVel, coeOmega, coeNDTCov; est = the match's
// (tx, ty, theta in RADIANS) and H3 its 3x3 Hessian over (tx, ty, yaw) (row-major), as a match record carries them.
// Returns `successful`.
int fr_fuse_step(const double *prm, int successful, const double *est, const double *H3, const double *pred,
                 const double *motion, const double *last, const double *last_cov, double *fused, double *cov_out) {
  PoseFuser pfu = make_fuser(prm);
  Pose2D predPose = pose_of(pred), odoMotion = pose_of(motion), lastPose = pose_of(last), estPose, fusedPose;
  estPose.setPose(est[0], est[1], RAD2DEG(est[2]));               // ours: src/PoseEstimator.cpp:36 (RAD2DEG is MyUtil.h:23)
  Eigen::Matrix3d lastCov = mat_of(last_cov), cov;
  if (successful) {                                               // ours: the branch of src/ScanMatcher.cpp:50-66
    Eigen::Matrix3d Qmat = (-mat_of(H3)).inverse() * prm[3];      // ours: src/PoseEstimator.cpp:57-64
    QuietCout quiet;
    pfu.fusePose(predPose, estPose, odoMotion, lastPose, lastCov, Qmat, fusedPose, cov);
  } else {
    pfu.calOdometryCovariance(odoMotion, lastPose, lastCov, cov);
    fusedPose = predPose;
  }
  put(fusedPose, fused);
  put(cov, cov_out);
  return successful;
}

// resamplePoints on n points (x, y pairs).  Returns the number of points the reference left in the scan; at most `cap`
// of them are copied out.  (Some parameter sets never end, space == 0 < space_thre for one: the caller runs this in a
// child process under a time limit.)
long fr_resample(double space, double space_thre, const double *xy, long n, double *out, long cap) {
  std::map<std::string, double> &t = front_ref_params();
  t.clear();
  t["space"] = space; t["space_thre"] = space_thre;
  ScanPointResampler spres;
  Scan2D scan;
  scan.lps.reserve(n);
  for (long i = 0; i < n; ++i) scan.lps.push_back(LPoint2D(0, xy[2 * i], xy[2 * i + 1]));
  spres.resamplePoints(&scan);
  const long m = static_cast<long>(scan.lps.size());
  for (long i = 0; i < m && i < cap; ++i) { out[2 * i] = scan.lps[i].x; out[2 * i + 1] = scan.lps[i].y; }
  return m;
}

// growMap's transform of a scan: Pose2D::globalPoint computes the expression of src/ScanMatcher.cpp:100-101
// (src/Pose2D.cpp:56-57 is the same two lines); out32 is the map cloud's float.
void fr_grow_map(const double *pose, const double *xy, long n, double *out64, float *out32) {
  const Pose2D p = pose_of(pose);
  for (long i = 0; i < n; ++i) {
    LPoint2D g = p.globalPoint(LPoint2D(0, xy[2 * i], xy[2 * i + 1]));
    out64[2 * i] = g.x; out64[2 * i + 1] = g.y;
    out32[2 * i] = static_cast<float>(g.x); out32[2 * i + 1] = static_cast<float>(g.y);   // ours: src/ScanMatcher.cpp:100-101 -> src/PointCloudMap.cpp:59-60
  }
}

}  // extern "C"
