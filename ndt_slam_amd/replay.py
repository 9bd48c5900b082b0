"""Replay harness: the reference's log-driven pipeline around the match, so that a recorded
(or synthetic) log goes in and the poses file and PCD maps of the reference come out, with every heavy step on
the device through the C ABI.

Host-side mirrors, same names and argument meaning as the reference:
  * SlamLauncher   -- text-log reader (src/SlamLauncher.cpp:37-105, 4 header lines: SlamLauncher.h:91-101),
                      pose dump (src/SlamLauncher.cpp:30-35), loop (:107-141)
  * ScanPointResampler (src/ScanPointResampler.cpp:4-62)
  * ScanMatcher    -- matchScan / growMap (src/ScanMatcher.cpp:4-116)
  * PoseFuser      -- fusePose / calOdometryCovariance (src/PoseFuser.cpp:3-61), Pose2D::calMotion / calPredPose
                      (src/Pose2D.cpp:5-37), MyUtil::add_angle / sub_angle (src/MyUtil.cpp:4-23)
  * Submap / PointCloudMap (include/ndt_slam/PointCloudMap.h:22-151, src/PointCloudMap.cpp:4-134) with PCD ASCII
                      output (PointCloudMap.h:124-136), and remakeMaps (src/PointCloudMap.cpp:136-170, commented out
                      there) as ndt_sessions_correct applies a pose adjustment: over ops.repose_points
  * FrontEnd::process (src/FrontEnd.cpp:4-47)

What runs on the MI355X: the source pre-filter and NDT match (PoseEstimator -> ndt_prefilter, ndt_map_build,
ndt_align), Submap::makeMap (ndt_make_map: octree change detection + moving-object removal) and
Submap::filterPoints (ndt_prefilter) -- in run_sessions both for all sessions at once (ndt_local_map_batch); with SlamLauncher(device_resample=True) also ScanPointResampler (ndt_resample,
bit-identical to resample_points).  `ops` is the object that provides them (capi.Context); the bookkeeping and the
3x3 filter algebra stay on the host as in the reference.  ROS publishing (tf, PoseArray, RViz clouds)
is left out: it does not feed back into the estimate.
"""
import collections
import math
import os

import numpy as np

from .pose_estimator import DEG2RAD, RAD2DEG, Pose2D, PoseEstimator, Scan2D, estimate_poses

# launch-file parameters (ndt_mapping.launch:8-36); constructor defaults differ and are noted at their classes
LAUNCH_PARAMS = dict(
    draw_skip=5, start_frame=0, end_frame=690, keyframe_skip=5, score_thre=0.5, space=0.05, space_thre=0.25,
    sepThre=10.0, removeMoving=True, resol=0.05, thre_neighbor=0.2, sidelidar=False, delTime=0.5, coeVel=0.1,
    coeOmega=0.5, coeNDTCov=1.0, TransformationEpsilon=0.01, StepSize=0.1, Resolution=0.3, MaximumIterations=35,
    LeafSize=0.05)


# ---------------------------------------------------------------------------------------------------------
# log file (SlamLauncher)
# ---------------------------------------------------------------------------------------------------------
def write_log(path, records, header=("# ndt_slam log", "# stamp x y theta[deg] image", "# n_front x y ...",
                                     "# n_left ... / n_right ...")):
    """records: iterable of dict(stamp, x, y, th, image, front[n,2], left[n,2], right[n,2]) -> the text format
    SlamLauncher::input_file_line reads: four free header lines, then per scan one line `stamp x y th image` and
    three groups `count x y x y ... ` (front, left, right lidar), every token followed by one space."""
    with open(path, "w") as f:
        for h in header:
            f.write(h + "\n")
        for r in records:
            f.write("%d %.9g %.9g %.9g %s\n" % (r["stamp"], r["x"], r["y"], r["th"], r.get("image", "none")))
            for key in ("front", "left", "right"):
                pts = np.asarray(r.get(key, np.zeros((0, 2))), dtype=np.float64).reshape(-1, 2)
                f.write("%d " % len(pts))
                f.write("".join("%.9g %.9g " % (p[0], p[1]) for p in pts))
                f.write("\n")


def read_log(path, sidelidar=True):
    """-> list of Scan2D (sid = stamp, pose = odometry in degrees, lps = front (+ left + right when sidelidar),
    SlamLauncher.cpp:37-93).  Every complete record is returned; the reference itself stops at end_frame and
    either drops or trips over the record that meets the end of the file (:95-98)."""
    with open(path) as f:
        for _ in range(4):                                   # readFormat(): four header lines
            f.readline()
        text = f.read()
    scans, pos = [], 0
    n = len(text)

    def token():
        nonlocal pos
        while pos < n and text[pos].isspace():
            pos += 1
        a = pos
        while pos < n and not text[pos].isspace():
            pos += 1
        return text[a:pos]

    while True:
        t = token()
        if not t:
            break
        stamp = int(t)
        x, y, th = float(token()), float(token()), float(token())
        eol = text.find("\n", pos)                           # image name: the rest of the line
        pos = n if eol < 0 else eol + 1
        groups = []
        ok = True
        for _ in range(3):
            c = token()
            if not c:
                ok = False
                break
            pts = np.empty((int(c), 2), dtype=np.float64)
            for i in range(int(c)):
                a, b = token(), token()
                if not b:
                    ok = False
                    break
                pts[i] = (float(a), float(b))
            if not ok:
                break
            groups.append(pts)
        if not ok:
            break                                            # truncated record at the end of the file
        lps = groups[0] if not sidelidar else np.concatenate(groups)
        scans.append(Scan2D(lps, sid=stamp, pose=Pose2D(x, y, th)))
    return scans


def write_poses(path, poses):
    """SlamLauncher::output_file_poses (:30-35): the count, then every 10th pose as `tx ty th ` (th in degrees),
    numbers as operator<< prints doubles (6 significant digits)."""
    with open(path, "w") as f:
        f.write("%d\n" % len(poses))
        for i in range(0, len(poses), 10):
            f.write("%s %s %s \n" % tuple(_cout(v) for v in (poses[i].tx, poses[i].ty, poses[i].th)))


def _cout(v):
    return "%g" % v          # std::ostream default: precision 6, general format


def save_pcd_ascii(path, xy):
    """pcl::io::savePCDFileASCII of a PointXYZ cloud with z = 0 (PointCloudMap.h:124-136): PCD v0.7 header,
    one `x y z` line per point, 8 significant digits (PCL's default precision)."""
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    with open(path, "w") as f:
        f.write("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\n"
                "COUNT 1 1 1\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA ascii\n" % (len(xy), len(xy)))
        for p in xy:
            f.write("%.8g %.8g 0\n" % (p[0], p[1]))


def load_pcd_ascii(path):
    with open(path) as f:
        lines = f.read().split("\n")
    i = next(k for k, l in enumerate(lines) if l.startswith("DATA"))
    rows = [l.split() for l in lines[i + 1:] if l.strip()]
    return np.array([[float(r[0]), float(r[1])] for r in rows], dtype=np.float32).reshape(-1, 2)


# ---------------------------------------------------------------------------------------------------------
# ScanPointResampler
# ---------------------------------------------------------------------------------------------------------
def resample_points(lps, space, space_thre):
    """ScanPointResampler::resamplePoints (src/ScanPointResampler.cpp:4-62): walk the scan, drop points until the
    accumulated distance reaches `space`, interpolate a point at exactly `space` (and look at the same input
    point again), keep the point itself across gaps of `space_thre` or more.  lps: [n,2] doubles."""
    lps = np.asarray(lps, dtype=np.float64).reshape(-1, 2)
    if len(lps) == 0:
        return lps
    out = [(lps[0, 0], lps[0, 1])]
    dis = 0.0
    prev = (lps[0, 0], lps[0, 1])
    i = 1
    n = len(lps)
    while i < n:
        cx, cy = lps[i, 0], lps[i, 1]
        dx, dy = cx - prev[0], cy - prev[1]
        L = math.sqrt(dx * dx + dy * dy)
        if dis + L < space:                                   # findInterpolatePoint: too close, dropped
            dis += L
            prev = (cx, cy)
        elif dis + L >= space_thre:                           # a gap: the point is kept as it is
            out.append((cx, cy))
            prev = (cx, cy)
            dis = 0.0
        else:                                                 # interpolate at `space` along prev -> current
            ratio = (space - dis) / L
            npt = (dx * ratio + prev[0], dy * ratio + prev[1])
            out.append(npt)
            prev = npt
            dis = 0.0
            continue                                          # inserted before lp: lp is looked at again (i--)
        i += 1
    return np.array(out, dtype=np.float64).reshape(-1, 2)


# ---------------------------------------------------------------------------------------------------------
# Pose2D helpers and PoseFuser
# ---------------------------------------------------------------------------------------------------------
def add_angle(a1, a2):                                        # src/MyUtil.cpp:4-12
    s = a1 + a2
    if s < -180:
        s += 360
    elif s >= 180:
        s -= 360
    return s


def sub_angle(a1, a2):                                        # src/MyUtil.cpp:15-23
    d = a1 - a2
    if d < -180:
        d += 360
    elif d >= 180:
        d -= 360
    return d


def calMotion(cur, prev):                                     # src/Pose2D.cpp:5-16
    dx, dy = cur.tx - prev.tx, cur.ty - prev.ty
    return Pose2D(prev.Rmat[0][0] * dx + prev.Rmat[1][0] * dy, prev.Rmat[0][1] * dx + prev.Rmat[1][1] * dy,
                  sub_angle(cur.th, prev.th))


def calPredPose(motion, last):                                # src/Pose2D.cpp:28-37
    return Pose2D(last.Rmat[0][0] * motion.tx + last.Rmat[0][1] * motion.ty + last.tx,
                  last.Rmat[1][0] * motion.tx + last.Rmat[1][1] * motion.ty + last.ty,
                  add_angle(last.th, motion.th))


class PoseFuser:
    """src/PoseFuser.cpp; constructor defaults include/ndt_slam/PoseFuser.h:19 (0.1, 0.1, 0.5)."""

    def __init__(self, coeVel=0.1, coeOmega=0.1, delTime=0.5):
        self.coeVel, self.coeOmega, self.delTime = coeVel, coeOmega, delTime

    def calOdometryCovariance(self, odoMotion, lastPose, lastCov):           # :39-61
        dt = self.delTime
        v = math.sqrt(odoMotion.tx * odoMotion.tx + odoMotion.ty * odoMotion.ty) / dt
        omega = DEG2RAD(odoMotion.th / dt)
        M = np.array([[self.coeVel * v * v, 0.0], [0.0, self.coeOmega * omega * omega]])
        c, s = math.cos(DEG2RAD(lastPose.th)), math.sin(DEG2RAD(lastPose.th))
        A = np.array([[dt * c, 0.0], [dt * s, 0.0], [0.0, dt]])
        F = np.array([[1.0, 0.0, -v * dt * s], [0.0, 1.0, v * dt * c], [0.0, 0.0, 1.0]])
        return F @ lastCov @ F.T + A @ M @ A.T

    def fusePose(self, predPose, estPose, odoMotion, lastPose, lastCov, Qmat):  # :3-37
        cov_hat = self.calOdometryCovariance(odoMotion, lastPose, lastCov)
        mu_hat = np.array([predPose.tx, predPose.ty, DEG2RAD(predPose.th)])
        K = cov_hat @ np.linalg.inv(Qmat + cov_hat)
        cov = (np.eye(3) - K) @ cov_hat
        zh = np.array([estPose.tx - predPose.tx, estPose.ty - predPose.ty, DEG2RAD(sub_angle(estPose.th, predPose.th))])
        mu = K @ zh + mu_hat
        return Pose2D(mu[0], mu[1], RAD2DEG(mu[2])), cov


# ---------------------------------------------------------------------------------------------------------
# Submap / PointCloudMap
# ---------------------------------------------------------------------------------------------------------
_EMPTY = np.zeros((0, 2), dtype=np.float32)


class Submap:
    """include/ndt_slam/PointCloudMap.h:22-69; constructor defaults LeafSize 0.2, removeMoving false."""

    def __init__(self, ops, atdS=0.0, cntS=0, removeMoving=False, LeafSize=0.2, resol=0.05, thre_neighbor=0.1):
        self.ops = ops
        self.atdS, self.cntS, self.cntE, self.newest = atdS, cntS, -1, True
        self.removeMoving, self.LeafSize = removeMoving, LeafSize
        self.resol, self.thre_neighbor = resol, thre_neighbor          # PCFilter.h:20-23
        self.scans = []
        self.p_cloud = _EMPTY
        self.filtered = None            # filterPoints() of the current p_cloud, when a batched call has already made it

    def addPoints(self, cloud):
        self.scans.append(cloud)

    def filterPoints(self):                                             # src/PointCloudMap.cpp:4-13
        if self.filtered is not None:
            return self.filtered
        if len(self.p_cloud) == 0:
            return _EMPTY
        return self.ops.prefilter(self.p_cloud, self.LeafSize)

    def makeMapArgs(self):
        """makeMap's arguments, as ops.make_map takes them and as an item of ops.local_maps starts."""
        return (self.scans, self.cntS == 0, self.newest, self.removeMoving, self.resol, self.thre_neighbor)

    def makeMap(self):                                                  # src/PointCloudMap.cpp:15-39
        self.p_cloud = self.ops.make_map(*self.makeMapArgs())
        self.filtered = None

    def setMap(self, p_cloud, filtered):
        """What makeMap and the filterPoints calls behind it give, from one batched call (ops.local_maps)."""
        self.p_cloud, self.filtered = p_cloud, filtered


class PointCloudMap:
    """include/ndt_slam/PointCloudMap.h:72-151, src/PointCloudMap.cpp:44-134; default sepThre 30."""

    def __init__(self, ops, sepThre=30.0, **submap_kw):
        self.ops, self.sepThre, self.submap_kw = ops, sepThre, submap_kw
        self.poses = []
        self.lastPose = Pose2D()
        self.lastScan = None
        self.atd = 0.0
        self.globalMap_cloud = _EMPTY
        self.localMap_cloud = _EMPTY
        self.maps = []
        self.submaps = [Submap(ops, **submap_kw)]
        # run_sessions' batched path: addPoints does its bookkeeping only, and the makeMap it ends in and makeLocalMap
        # are left to ONE ops.local_maps call over every session of the step (localMapItem / setLocalMap)
        self.deferred = False

    def setLastPose(self, p):
        self.lastPose = p

    def getLastPose(self):
        return self.lastPose

    def setLastScan(self, s):
        self.lastScan = s

    def addPose(self, p):                                               # :44-56
        if self.poses:
            pp = self.poses[-1]
            self.atd += math.sqrt((p.tx - pp.tx) * (p.tx - pp.tx) + (p.ty - pp.ty) * (p.ty - pp.ty))
        else:
            self.atd = 0.0
        self.poses.append(p)

    def addPoints(self, lps):                                           # :59-96
        sub = self.addPointsBookkeeping(lps)
        if not self.deferred:
            sub.makeMap()

    def addPointsBookkeeping(self, lps):
        """addPoints without the makeMap it ends in: the scan goes to the current submap, or -- past sepThre of travelled
        distance -- the current submap closes (:72-90) and a new one takes it.  Returns the submap whose map is to be made."""
        cloud = np.ascontiguousarray(lps, dtype=np.float32).reshape(-1, 2)   # double -> PointXYZ floats, z = 0
        cur = self.submaps[-1]
        if self.atd - cur.atdS >= self.sepThre:
            size = len(self.poses)
            cur.cntE = size - 2
            cur.p_cloud = cur.filterPoints()                            # (p_cloud has not changed since the last step's filter)
            cur.filtered = None
            cur.newest = False
            sub = Submap(self.ops, self.atd, size - 1, **self.submap_kw)
            if len(cur.scans) >= 2:                                     # two scans of overlap for the triple test
                sub.addPoints(cur.scans[-2])
                sub.addPoints(cur.scans[-1])
            sub.addPoints(cloud)
            self.submaps.append(sub)
            return sub
        cur.addPoints(cloud)
        return cur

    def makeGlobalMap(self):                                            # :101-117
        self.maps = [s.p_cloud for s in self.submaps[:-1]]
        self.maps.append(self.submaps[-1].filterPoints())
        self.globalMap_cloud = np.concatenate(self.maps) if self.maps else _EMPTY

    def makeLocalMap(self):                                             # :119-134
        if self.deferred:
            return
        parts = []
        if len(self.submaps) >= 2:
            parts.append(self.submaps[-2].p_cloud)
        parts.append(self.submaps[-1].filterPoints())
        self.localMap_cloud = np.concatenate(parts)

    def localMapItem(self):
        """The current submap's makeMap + makeLocalMap as an item of ops.local_maps."""
        prev = self.submaps[-2].p_cloud if len(self.submaps) >= 2 else None
        return self.submaps[-1].makeMapArgs() + (prev,)

    def setLocalMap(self, p_cloud, target, n_prev):
        """The result of that item: the submap's cloud, and the local map = previous submap's cloud + filtered cloud."""
        self.submaps[-1].setMap(p_cloud, target[n_prev:])
        self.localMap_cloud = target

    def storeFirst(self):
        """Index in `poses` of the first scan the current submap holds: its scans are the tail of the stepped scans, the two
        carried over at a split first (:80-83)."""
        return len(self.poses) - len(self.submaps[-1].scans)

    def anchorScan(self, m):
        """The scan whose (old, new) pose pair moves submap m's closed cloud in remakeMaps: the middle one of the submap's own
        scans, cntS + (cntE - cntS) / 2 -- the current submap's cntE is the newest scan; a submap that closed without a scan of
        its own (cntE < cntS) takes cntS."""
        sub = self.submaps[m]
        cntE = sub.cntE if m < len(self.submaps) - 1 else len(self.poses) - 1
        return sub.cntS + (cntE - sub.cntS) // 2 if cntE > sub.cntS else sub.cntS

    def remakeMaps(self, newPoses):                                     # :138-170 (commented out in the reference)
        """The maps after a pose adjustment, as ndt_sessions_correct makes them on the device: every scan the current submap
        holds moves from its own old pose to its new one and the submap's cloud is made again from them (the reference moves
        the points of the cloud by their scan ids; recomputing keeps the cloud what makeMap gives for the scans held); a closed
        submap's cloud -- voxel centroids without a scan id -- moves as a whole by the pair of its anchor scan (anchorScan).
        ops.repose_points does the moves.  poses and lastPose are replaced; atd is left as it is (:166-169).  deferred: the
        makeMap and makeLocalMap are the caller's (localMapItem / setLocalMap), as in addPoints."""
        newPoses = list(newPoses)
        if len(newPoses) != len(self.poses):
            raise ValueError("remakeMaps: %d new poses for %d scans" % (len(newPoses), len(self.poses)))
        if not newPoses:
            return
        cur = self.submaps[-1]
        first = self.storeFirst()
        idx = [self.anchorScan(m) for m in range(len(self.submaps) - 1)] + [first + k for k in range(len(cur.scans))]
        clouds = [s.p_cloud for s in self.submaps[:-1]] + list(cur.scans)
        moved = self.ops.repose_points(clouds, [(self.poses[i].tx, self.poses[i].ty, self.poses[i].th) for i in idx],
                                       [(newPoses[i].tx, newPoses[i].ty, newPoses[i].th) for i in idx])
        n_closed = len(self.submaps) - 1
        for m in range(n_closed):
            self.submaps[m].p_cloud = moved[m]
        cur.scans = list(moved[n_closed:])
        self.poses = newPoses
        self.lastPose = newPoses[-1]
        if not self.deferred:
            cur.makeMap()
            self.makeGlobalMap()
            self.makeLocalMap()

    def saveGlobalMap(self, map_name, separated_map_name):              # PointCloudMap.h:124-136
        save_pcd_ascii(map_name, self.globalMap_cloud)
        for i, m in enumerate(self.maps):
            save_pcd_ascii("%s%d.pcd" % (separated_map_name, i), m)


# ---------------------------------------------------------------------------------------------------------
# ScanMatcher / FrontEnd / SlamLauncher
# ---------------------------------------------------------------------------------------------------------
class ScanMatcher:
    """src/ScanMatcher.cpp:4-116; default score threshold 0.0 (ScanMatcher.h:49)."""

    def __init__(self, estim, pcmap, pfu, scthre=0.0, space=0.0, space_thre=0.0, resample=resample_points):
        self.estim, self.pcmap, self.pfu = estim, pcmap, pfu
        self.resample = resample             # resample_points, or a device resampler with its arguments (ops.resample)
        self.scthre, self.space, self.space_thre = scthre, space, space_thre
        self.cnt = 0
        self.prevScan = None
        self.poses, self.Covs = [], []
        self.lastCov = np.zeros((3, 3))      # (the reference reads it uninitialised on the second scan, ScanMatcher.h:42)
        self.costs, self.accepted = [], []

    def matchScan(self, curScan):
        predPose = self.matchScanBegin(curScan)
        if predPose is None:
            return True
        cost, estPose, Qmat = self.estim.estimatePose(predPose)                         # :45
        return self.matchScanEnd(cost, estPose, Qmat)

    def matchScanBegin(self, curScan):
        """matchScan up to setScanPair.  Returns the predicted pose the match starts from, or None when the scan is the
        first one (taken as it is: nothing to match)."""
        curScan.lps = self.resample(curScan.lps, self.space, self.space_thre)           # :6
        if self.cnt == 0:                                                               # :9-22
            self.growMap(curScan, curScan.pose)
            self.savePose(curScan.pose, np.zeros((3, 3)))
            self.prevScan = curScan
            self.cnt += 1
            return None
        odoMotion = calMotion(curScan.pose, self.prevScan.pose)                         # :27-28
        lastPose = self.pcmap.getLastPose()
        predPose = calPredPose(odoMotion, lastPose)                                     # :30-32
        self.estim.setScanPair(curScan, self.pcmap.localMap_cloud)                      # :40
        self._pending = (curScan, odoMotion, lastPose, predPose)
        return predPose

    def matchScanEnd(self, cost, estPose, Qmat):
        """matchScan from the accept test on, with the estimate of the scan matchScanBegin set up."""
        curScan, odoMotion, lastPose, predPose = self._pending
        self._pending = None
        successful = cost <= self.scthre                                                # :49-53
        if successful:                                                                  # :58-65
            fusedPose, cov = self.pfu.fusePose(predPose, estPose, odoMotion, lastPose, self.lastCov, Qmat)
        else:
            cov = self.pfu.calOdometryCovariance(odoMotion, lastPose, self.lastCov)
            fusedPose = predPose
        self.lastCov = cov
        self.growMap(curScan, fusedPose)                                                # :71
        self.prevScan = curScan
        self.savePose(fusedPose, cov)
        self.costs.append(cost)
        self.accepted.append(bool(successful))
        self.cnt += 1
        return successful

    def savePose(self, pose, cov):
        self.poses.append(pose)
        self.Covs.append(cov)

    def growMap(self, scan, pose):                                                      # :92-116
        R = pose.Rmat
        x = R[0][0] * scan.lps[:, 0] + R[0][1] * scan.lps[:, 1] + pose.tx
        y = R[1][0] * scan.lps[:, 0] + R[1][1] * scan.lps[:, 1] + pose.ty
        self.pcmap.addPose(pose)
        self.pcmap.addPoints(np.stack([x, y], axis=1))
        self.pcmap.setLastPose(pose)
        self.pcmap.setLastScan(scan)
        self.pcmap.makeLocalMap()


class FrontEnd:
    """src/FrontEnd.cpp:4-47 (the pose-graph and loop-closure parts are commented out in the reference)."""

    def __init__(self, smat, pcmap, keyframeSkip=5, startFrame=0):
        self.smat, self.pcmap = smat, pcmap
        self.keyframeSkip, self.startFrame = keyframeSkip, startFrame
        self.cnt = 0

    def process(self, scan):
        if scan.sid < self.startFrame:
            return
        self.smat.matchScan(scan)
        self.processEnd()

    def processEnd(self):
        """process() behind the match: the keyframe bookkeeping."""
        if self.cnt % self.keyframeSkip == 0:
            self.pcmap.makeGlobalMap()
        self.cnt += 1

    def get_poses(self):
        return self.smat.poses


class SlamLauncher:
    """Wires the pipeline as SlamLauncher::init does (src/SlamLauncher.cpp:7-28) and runs the replay loop
    (:107-141).  `ops` provides prefilter / make_map (a capi.Context); `estim` defaults to the device
    PoseEstimator on the same context.  device_resample: the scans are resampled by ops.resample (on the device)
    instead of the host mirror resample_points -- the same points, bit for bit."""

    def __init__(self, ops, estim=None, device_resample=False, **params):
        p = dict(LAUNCH_PARAMS)
        p.update(params)
        self.p = p
        self.estim = estim if estim is not None else PoseEstimator(
            ctx=ops, coeNDTCov=p["coeNDTCov"], TransformationEpsilon=p["TransformationEpsilon"], StepSize=p["StepSize"],
            Resolution=p["Resolution"], MaximumIterations=p["MaximumIterations"], LeafSize=p["LeafSize"])
        self.pcmap = PointCloudMap(ops, sepThre=p["sepThre"], removeMoving=p["removeMoving"], LeafSize=p["LeafSize"],
                                   resol=p["resol"], thre_neighbor=p["thre_neighbor"])
        self.pfu = PoseFuser(p["coeVel"], p["coeOmega"], p["delTime"])
        self.smat = ScanMatcher(self.estim, self.pcmap, self.pfu, scthre=p["score_thre"], space=p["space"],
                                space_thre=p["space_thre"], resample=ops.resample if device_resample else resample_points)
        self.frontEnd = FrontEnd(self.smat, self.pcmap, keyframeSkip=p["keyframe_skip"], startFrame=p["start_frame"])

    def run(self, scans, poses_name=None, map_name=None, separated_map_name=None):
        """scans: list of Scan2D (read_log).  Processes at most end_frame scans, then writes what the reference
        writes: the poses file and, when names are given, the PCD maps.  Returns the list of fused poses."""
        for cnt, scan in enumerate(scans, start=1):
            if cnt > self.p["end_frame"]:
                break
            self.frontEnd.process(scan)
        poses = self.frontEnd.get_poses()
        if poses_name:
            write_poses(poses_name, poses)
        if map_name:
            self.pcmap.saveGlobalMap(map_name, separated_map_name or (map_name + "_sep"))
        return poses


def run_sessions(ops, logs, poses_names=None, map_names=None, separated_map_names=None, estimate=estimate_poses,
                 launchers=None, **params):
    """Independent SLAM sessions in lockstep: one SlamLauncher stack per log (`launchers`, or built from ops and
    params), all stepped together.  At step k every session that still has a scan (at most end_frame of them) runs
    matchScan's first half; the sessions that need a match are estimated together by ONE call of
    `estimate(estimators, initPoses)` -- estimate_poses: one multi-map launch over the sessions' local maps -- then
    each session runs the second half and FrontEnd's bookkeeping (start_frame, keyframe_skip).  A session that has
    run out of scans drops out of the batch.  Writes per session what SlamLauncher.run writes (names may be None)
    and returns the list of every session's fused poses; each is the same as its own SlamLauncher.run.
    When all sessions share one `ops` object that provides local_maps (a capi.Context), the map part of every growMap
    of a step -- Submap::makeMap, filterPoints and makeLocalMap -- is done by ONE ops.local_maps call per step (one per
    distinct LeafSize), between the second halves of matchScan and the bookkeeping; the sessions then make no
    ops.make_map and no ops.prefilter call.  Otherwise every session makes its own calls, as SlamLauncher.run does."""
    logs = [list(l) for l in logs]
    S = len(logs)
    if launchers is None:
        launchers = [SlamLauncher(ops, **params) for _ in range(S)]
    if len(launchers) != S:
        raise ValueError("run_sessions: one launcher per log")
    lengths = [min(len(l), L.p["end_frame"]) for l, L in zip(logs, launchers)]
    ops0 = launchers[0].pcmap.ops if launchers else None
    batched = ops0 is not None and hasattr(ops0, "local_maps") and all(L.pcmap.ops is ops0 for L in launchers)
    for L in launchers:
        L.pcmap.deferred = batched
    try:
        for k in range(max(lengths, default=0)):
            stepped, need = [], []
            for i in range(S):
                if k >= lengths[i]:
                    continue
                fe, scan = launchers[i].frontEnd, logs[i][k]
                if scan.sid < fe.startFrame:
                    continue
                stepped.append(i)
                pred = fe.smat.matchScanBegin(scan)
                if pred is not None:
                    need.append((i, pred))
            if need:
                res = estimate([launchers[i].smat.estim for i, _ in need], [p for _, p in need])
                for (i, _), (cost, est, cov) in zip(need, res):
                    launchers[i].smat.matchScanEnd(cost, est, cov)
            if batched and stepped:
                # every stepped session has grown its map by one scan (matchScanBegin for a first scan, matchScanEnd for the
                # others): their local maps in one call per LeafSize
                by_leaf = {}
                for i in stepped:
                    by_leaf.setdefault(launchers[i].pcmap.submaps[-1].LeafSize, []).append(i)
                for leaf, idx in by_leaf.items():
                    res = ops0.local_maps([launchers[i].pcmap.localMapItem() for i in idx], leaf)
                    for i, (p_cloud, target, n_prev) in zip(idx, res):
                        launchers[i].pcmap.setLocalMap(p_cloud, target, n_prev)
            for i in stepped:
                launchers[i].frontEnd.processEnd()
    finally:
        for L in launchers:
            L.pcmap.deferred = False
    out = []
    for i, L in enumerate(launchers):
        poses = L.frontEnd.get_poses()
        if poses_names and poses_names[i]:
            write_poses(poses_names[i], poses)
        if map_names and map_names[i]:
            sep = separated_map_names[i] if separated_map_names and separated_map_names[i] else None
            L.pcmap.saveGlobalMap(map_names[i], sep or (map_names[i] + "_sep"))
        out.append(poses)
    return out


def save_occupancy(stem, values, geometry, occupied_thresh=0.65, free_thresh=0.196):
    """An occupancy grid in map_server's format: `stem`.pgm and `stem`.yaml.  values: [ny, nx] int8 as OccGrid.render gives
    them (-1 unknown, else 0 .. 100), row iy at y0 + iy res; geometry: anything with x0, y0, res.  The PGM is P5 with row 0
    the LARGEST y; a pixel is 0 for value / 100 > occupied_thresh, 254 for value / 100 < free_thresh, 205 otherwise (unknown
    included).  The YAML holds image, resolution, origin [x0, y0, 0.0], negate 0 and the two thresholds."""
    v = np.asarray(values, dtype=np.int8)
    if v.ndim != 2:
        raise ValueError("save_occupancy: values must be [ny, nx]")
    known = v >= 0
    p = v.astype(np.float64) / 100.0
    pix = np.full(v.shape, 205, dtype=np.uint8)
    pix[known & (p > occupied_thresh)] = 0
    pix[known & (p < free_thresh)] = 254
    stem = str(stem)
    with open(stem + ".pgm", "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (v.shape[1], v.shape[0]))
        f.write(np.ascontiguousarray(pix[::-1]).tobytes())
    with open(stem + ".yaml", "w") as f:
        f.write("image: %s\nresolution: %r\norigin: [%r, %r, 0.0]\nnegate: 0\noccupied_thresh: %r\nfree_thresh: %r\n"
                % (os.path.basename(stem) + ".pgm", float(geometry.res), float(geometry.x0), float(geometry.y0),
                   float(occupied_thresh), float(free_thresh)))


def load_occupancy(stem):
    """The inverse of save_occupancy, for tests -> (pixels [ny, nx] uint8 with row 0 the SMALLEST y again, dict of the YAML:
    image, resolution, origin [x0, y0, 0.0], negate, occupied_thresh, free_thresh)."""
    stem = str(stem)
    with open(stem + ".pgm", "rb") as f:
        raw = f.read()
    magic, dims, maxv, body = raw.split(b"\n", 3)
    if magic != b"P5" or maxv != b"255":
        raise ValueError("load_occupancy: not a P5 image of 8 bits")
    nx, ny = (int(t) for t in dims.split())
    pix = np.frombuffer(body, dtype=np.uint8, count=nx * ny).reshape(ny, nx)[::-1].copy()
    meta = {}
    with open(stem + ".yaml") as f:
        for line in f:
            key, _, val = line.strip().partition(": ")
            if key == "image":
                meta[key] = val
            elif key == "origin":
                meta[key] = [float(t) for t in val.strip("[]").split(",")]
            elif key == "negate":
                meta[key] = int(val)
            elif key:
                meta[key] = float(val)
    return pix, meta


# run_sessions_resident's loop closure: loop = a capi.LoopParams, pg = pose-graph parameters (None: the defaults), odo_info =
# the six numbers of every odometry arc's information matrix, every = the lockstep steps between two searches, cooldown = the
# steps a corrected session is not searched again, remake_closed = behind correct() every corrected session's closed submaps
# are computed again from the scan archive (sessions.remake_closed) instead of staying rigidly moved, multi = None or a
# capi.LoopMultiParams: the search is then sessions.find_loops_multi with it (several old submaps per session, accepted on
# ranged fitness; its `loop` part replaces `loop`) and every edge found for a session goes into that session's one graph,
# cross = None or a capi.LoopMultiParams: behind the closing inside the sessions comes one sessions.find_cross_loops with it
# (the sessions must share a map frame), one joint graph per group of sessions that its edges tie together, and one correct(),
# robust = None or an object with `params` (a capi.PgRobustParams, None: the defaults) and `phi` (the chi-square beyond which a
# loop or cross arc counts as rejected): the graphs then go through capi.optimize_pose_graphs_robust with phi on the loop and
# cross arcs and 0 on the odometry arcs, `pg` is not used, and a graph's sessions are corrected only when robust_keep says so,
# consistency = None or a chi-square bound (11.34: 99 % at 3 degrees of freedom): a loop edge found inside a session whose
# loop_consistency against that session's odometry is above the bound is dropped before the graph is built (cross edges, which
# no single trajectory's odometry spans, are not gated)
class LoopClosure(collections.namedtuple("LoopClosure", "loop pg odo_info every cooldown")):
    """The five fields above as a tuple, as before (its _fields, its length and its unpacking are unchanged), and the
    attributes remake_closed (default False), multi (default None), cross (default None), robust (default None) and
    consistency (default None) beside them."""

    def __new__(cls, loop, pg, odo_info, every, cooldown, remake_closed=False, multi=None, cross=None, robust=None,
                consistency=None):
        self = super().__new__(cls, loop, pg, odo_info, every, cooldown)
        self.remake_closed = bool(remake_closed)
        self.multi = multi
        self.cross = cross
        self.robust = robust
        self.consistency = consistency
        return self


RobustClosure = collections.namedtuple("RobustClosure", "params phi")      # what LoopClosure.robust is set to


def robust_keep(records, chi2, phi, edge_offsets):
    """Which graphs of a robust batch may correct their sessions (host only): graph g when its record ends with status 0 and
    converged and at least one of its robust arcs (phi > 0) is kept, that is has chi2 <= phi.  records: PG_ROBUST_RESULT_DTYPE
    (or anything with ["pg"]["status"] and ["pg"]["converged"] per graph); chi2 and phi one number per arc; edge_offsets the
    batch's.  -> a bool array, one per graph."""
    chi2, phi = np.asarray(chi2, dtype=np.float64).reshape(-1), np.asarray(phi, dtype=np.float64).reshape(-1)
    if len(chi2) != len(phi) or len(edge_offsets) != len(records) + 1:
        raise ValueError("robust_keep needs one chi2 and one phi per arc and one more edge offset than graphs")
    keep = np.zeros(len(records), dtype=bool)
    for g in range(len(records)):
        a, b = int(edge_offsets[g]), int(edge_offsets[g + 1])
        kept = (phi[a:b] > 0) & (chi2[a:b] <= phi[a:b])
        keep[g] = int(records[g]["pg"]["status"]) == 0 and bool(records[g]["pg"]["converged"]) and bool(kept.any())
    return keep


def _optimize_closing(ctx, lc, poses, node_offsets, edges, edge_offsets, n_loop_arcs):
    """The batch of a closing through the optimiser lc asks for -> (new poses, one flag per graph: correct its sessions).
    n_loop_arcs[g]: the loop or cross arcs of graph g, which lie at the END of its arc list (loops_graph, cross_graph without
    loops inside the trajectories)."""
    from . import capi
    robust = getattr(lc, "robust", None)
    if robust is None:
        new, res = capi.optimize_pose_graphs(ctx, poses, node_offsets, edges, edge_offsets, lc.pg)
        return new, np.array([r["status"] == 0 and bool(r["converged"]) for r in res], dtype=bool)
    phi = np.zeros(len(edges), dtype=np.float64)
    for g, k in enumerate(n_loop_arcs):
        phi[int(edge_offsets[g + 1]) - k:int(edge_offsets[g + 1])] = float(robust.phi)
    new, res, _, chi2 = capi.optimize_pose_graphs_robust(ctx, poses, node_offsets, edges, edge_offsets, phi, robust.params)
    return new, robust_keep(res, chi2, phi, edge_offsets)


def closed_scan_ranges(sub_first, n_closed):
    """The scans every closed submap held when it closed, as [first, last] index ranges of the stepped scans (host only):
    sub_first = every submap's first own scan (sessions.trajectory(i)[1]: n_closed + 1 entries, the current submap's last),
    submap m owns [sub_first[m], sub_first[m + 1] - 1] and held, in front of them, the last two scans of what submap m - 1
    held -- none when that held fewer than two (addPointsBookkeeping's split rule).  An empty range has last = first - 1."""
    sub_first = [int(v) for v in sub_first]
    if n_closed < 0 or n_closed + 1 > len(sub_first):
        raise ValueError("closed_scan_ranges: %d closed submaps need %d entries of sub_first" % (n_closed, n_closed + 1))
    out, held = [], 0
    for m in range(n_closed):
        first, last = sub_first[m] - (2 if m >= 1 and held >= 2 else 0), sub_first[m + 1] - 1
        held = last - first + 1
        out.append([first, last])
    return out


def loops_graph(poses, loop_edges, odo_info):
    """The pose graph of one trajectory with any number of loops (host only): one odometry arc per consecutive pair of
    `poses` ([n, 3], (tx, ty, th[deg])) -- rel by capi.pg_edge_between, info = odo_info (6 numbers) -- then every loop's arc
    as given and in the given order (records with from / from_, to, rel, info: ndt_loop.edge) -> the n - 1 + len(loop_edges)
    arcs as capi.PG_EDGE_DTYPE."""
    from . import capi
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    n = len(poses)
    edges = np.zeros(n - 1 + len(loop_edges), dtype=capi.PG_EDGE_DTYPE)
    for j in range(n - 1):
        edges[j]["from"], edges[j]["to"] = j, j + 1
        edges[j]["rel"] = capi.pg_edge_between(poses[j], poses[j + 1])
        edges[j]["info"] = np.asarray(odo_info, dtype=np.float64).reshape(6)
    for k, loop_edge in enumerate(loop_edges):
        names = getattr(getattr(loop_edge, "dtype", None), "names", None) or ()
        e = edges[n - 1 + k]
        e["from"] = loop_edge["from" if "from" in names else "from_"]
        e["to"] = loop_edge["to"]
        e["rel"], e["info"] = loop_edge["rel"], loop_edge["info"]
    return edges


def loop_consistency(ctx, poses, odo_info, loop_edges):
    """How far every candidate loop arc of one trajectory lies from what the odometry in between allows -> d2[], one squared
    Mahalanobis distance per arc (chi-square with 3 degrees of freedom for a true one).  The graph is the odometry alone,
    loops_graph(poses, [], odo_info); one query (0, from, to) per arc in one capi.pose_graph_marginals call, then
    capi.pg_relative_cov and capi.pg_edge_chi2 at the trajectory's poses."""
    from . import capi
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    if not len(loop_edges):
        return np.zeros(0, dtype=np.float64)
    ends = []
    for e in loop_edges:
        names = getattr(getattr(e, "dtype", None), "names", None) or ()
        ends.append((int(e["from" if "from" in names else "from_"]), int(e["to"])))
    odo = loops_graph(poses, [], odo_info)
    marg = capi.pose_graph_marginals(ctx, poses, [0, len(poses)], odo, [0, len(odo)], [(0, a, b) for a, b in ends])
    d2 = np.zeros(len(ends), dtype=np.float64)
    for k, ((a, b), e) in enumerate(zip(ends, loop_edges)):
        if marg[k]["status"] != 0 or not marg[k]["converged"]:
            raise capi.NdtError("loop_consistency: no covariance for the arc %d -> %d (status %d, converged %d)"
                                % (a, b, marg[k]["status"], marg[k]["converged"]))
        d2[k] = capi.pg_edge_chi2(poses[a], poses[b], e, capi.pg_relative_cov(poses[a], poses[b], marg[k]))
    return d2


def loop_graph(poses, loop_edge, odo_info):
    """loops_graph with one loop: the n arcs of a trajectory of n poses."""
    return loops_graph(poses, [loop_edge], odo_info)


def cross_graph(trajs, loop_edges_per_session, cross_edges, odo_info):
    """The joint pose graph of a group of sessions (host only).  The nodes are the trajectories `trajs` ([n_i, 3] each, in
    ascending session order) back to back: node offset[i] + k is scan k of trajectory i.  The arcs: per trajectory, in order,
    what loops_graph(trajs[i], loop_edges_per_session[i], odo_info) makes, its indices shifted by offset[i]; then every cross
    edge (a, b, edge) -- `edge` found by a searcher that is trajectory b in a closed submap of trajectory a (ndt_cross_loop:
    edge.from a scan of a, edge.to a scan of b) -- with from shifted by offset[a] and to by offset[b], in the given order.
    -> (the nodes [sum n_i, 3], the arcs as capi.PG_EDGE_DTYPE, offset)."""
    from . import capi
    trajs = [np.ascontiguousarray(t, dtype=np.float64).reshape(-1, 3) for t in trajs]
    if len(loop_edges_per_session) != len(trajs):
        raise ValueError("cross_graph needs one list of loop edges per trajectory")
    offset = np.concatenate([[0], np.cumsum([len(t) for t in trajs])]).astype(np.int64)
    parts = []
    for i, t in enumerate(trajs):
        g = loops_graph(t, loop_edges_per_session[i], odo_info)
        g["from"] += int(offset[i])
        g["to"] += int(offset[i])
        parts.append(g)
    tail = np.zeros(len(cross_edges), dtype=capi.PG_EDGE_DTYPE)
    for k, (a, b, edge) in enumerate(cross_edges):
        if not (0 <= a < len(trajs) and 0 <= b < len(trajs)) or a == b:
            raise ValueError("cross_graph: cross edge %d does not tie two trajectories of the group" % k)
        names = getattr(getattr(edge, "dtype", None), "names", None) or ()
        tail[k]["from"] = int(edge["from" if "from" in names else "from_"]) + int(offset[a])
        tail[k]["to"] = int(edge["to"]) + int(offset[b])
        tail[k]["rel"], tail[k]["info"] = edge["rel"], edge["info"]
    return np.concatenate(trajs), np.concatenate(parts + [tail]), offset


def place_verify(ctx, sessions, candidates, loop_params):
    """Sessions.place_candidates' `candidates` through the stages of the multi-submap loop search, made of public calls: a map
    of every candidate's closed cloud (capi.build_maps), the searcher's newest scan -- from the set's archive, robot frame,
    pre-filtered at the set's leaf --, a lattice of loop_params.loop's steps and half extents around the candidate's guess (wide
    enough when the half extents cover one ring width and one sector, +-3 deg), then ndt_score_lattice_multi_dev ->
    ndt_lattice_select_multi_dev -> ndt_align_batch_multi_dev -> ndt_fit_points_multi_dev over all candidates at once.  A
    candidate is accepted by ndt_sessions_find_loops_multi's rule (include/ndt_mi355x.h: a pick is usable when it converged with
    n_in >= 1 and n_in >= min_overlap * n_points, its cost the ranged fitness; the best pick is the accepted one of largest n_in,
    then lowest cost; accepted when its cost <= max_cost).  -> [(candidate index, edge)] of the accepted candidates: edge a
    capi.PG_EDGE_DTYPE record from the candidate's centre scan in map_session's trajectory to the searcher's newest scan, rel =
    ndt_pg_edge_between(that scan's pose, the matched pose), info = loop_params.loop.info."""
    import torch

    from . import capi
    lp, K = loop_params.loop, loop_params.loop.top_k
    cands = list(candidates)
    if not cands:
        return []
    dev = torch.device("cuda", ctx.device)
    trajs = {i: sessions.trajectory(i)[0] for c in cands for i in (int(c["session"]), int(c["map_session"]))}
    closed = {i: sessions.global_map(i)[1] for i in {int(c["map_session"]) for c in cands}}
    searchers = sorted({int(c["session"]) for c in cands})
    leaf = sessions.params.leaf
    scans = [ctx.prefilter(np.asarray(sessions.archive_scans(i, len(trajs[i]) - 1, 1)[0], np.float32), leaf) for i in searchers]
    if any(len(s) == 0 for s in scans):
        raise ValueError("place_verify: a searcher's newest scan is empty")
    maps = capi.build_maps(ctx, [closed[int(c["map_session"])][int(c["submap"])] for c in cands], sessions.params.match)
    try:
        jobs = []
        for j, c in enumerate(cands):
            g = c["guess"]
            lat = capi.PoseLattice(x0=g[0] - lp.half_x * lp.step_xy, y0=g[1] - lp.half_y * lp.step_xy,
                                   yaw0=DEG2RAD(g[2]) - lp.half_yaw * lp.step_yaw, step_x=lp.step_xy, step_y=lp.step_xy,
                                   step_yaw=lp.step_yaw, nx=2 * lp.half_x + 1, ny=2 * lp.half_y + 1, nyaw=2 * lp.half_yaw + 1)
            jobs.append((j, searchers.index(int(c["session"])), lat))
        pts, off = capi.pack_scans(scans)
        d_pts, d_off = torch.from_numpy(pts).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev)
        total = sum(lat.size for _, _, lat in jobs)
        d_score = torch.zeros(total, dtype=torch.float64, device=dev)
        d_pairs = torch.zeros(total, dtype=torch.int32, device=dev)
        d_cand = torch.zeros(len(jobs) * K, dtype=torch.int64, device=dev)
        d_n = torch.zeros(len(jobs), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        ctx.score_lattice_multi_dev(maps, d_pts.data_ptr(), d_off.data_ptr(), len(scans), len(pts), jobs, d_score.data_ptr(), d_pairs.data_ptr())
        ctx.lattice_select_multi_dev(jobs, d_score.data_ptr(), d_pairs.data_ptr(), K, lp.local_max, d_cand.data_ptr(), d_n.data_ptr())
        torch.cuda.synchronize(dev)
        picks, n_pick = d_cand.cpu().numpy().reshape(len(jobs), K), d_n.cpu().numpy()
        rows = [(j, int(q)) for j in range(len(jobs)) for q in picks[j, :n_pick[j]]]
        if not rows:
            return []
        inits = np.array([jobs[j][2].pose(q) for j, q in rows], np.float64).reshape(-1, 3)
        m_pts, m_off = capi.pack_scans([scans[jobs[j][1]] for j, _ in rows])
        d_mp, d_mo = torch.from_numpy(m_pts).to(dev), torch.from_numpy(m_off.astype(np.int64)).to(dev)
        d_map_of = torch.tensor([j for j, _ in rows], dtype=torch.int32, device=dev)
        d_init = torch.from_numpy(inits).to(dev)
        d_res = torch.zeros(len(rows) * capi.RESULT_BYTES, dtype=torch.uint8, device=dev)
        d_fit = torch.zeros(len(rows) * capi.FIT_STATS_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        ctx.align_batch_multi_dev(maps, d_map_of.data_ptr(), d_mp.data_ptr(), d_mo.data_ptr(), len(rows), len(m_pts), d_init.data_ptr(),
                                  d_res.data_ptr())
        ctx.fit_points_multi_dev(maps, d_map_of.data_ptr(), d_mp.data_ptr(), d_mo.data_ptr(), len(rows), len(m_pts),
                                 d_res.data_ptr() + capi.RESULT_DTYPE.fields["T00"][1], capi.RESULT_BYTES, loop_params.max_d2, None, d_fit.data_ptr())
        torch.cuda.synchronize(dev)
        res = d_res.cpu().numpy().view(capi.RESULT_DTYPE)
        fit = d_fit.cpu().numpy().view(capi.FIT_STATS_DTYPE)
    finally:
        for m in maps:
            m.close()
    out = []
    for j, c in enumerate(cands):
        best, best_key = -1, None
        for r, (jj, _) in enumerate(rows):
            if jj != j:
                continue
            usable = bool(res[r]["converged"]) and fit[r]["n_in"] >= 1 and float(fit[r]["n_in"]) >= loop_params.min_overlap * float(fit[r]["n_points"])
            cost = float(fit[r]["fitness"]) if usable else 1e7
            key = (not cost <= lp.max_cost, -(int(fit[r]["n_in"]) if usable else 0), cost)
            if best_key is None or key < best_key:
                best, best_key = r, key
        if best < 0 or best_key[0]:
            continue
        pose = np.array([res[best]["pose"][0], res[best]["pose"][1], RAD2DEG(res[best]["pose"][2])])
        edge = np.zeros(1, dtype=capi.PG_EDGE_DTYPE)[0]
        edge["from"], edge["to"] = int(c["centre_scan"]), len(trajs[int(c["session"])]) - 1
        edge["rel"] = capi.pg_edge_between(trajs[int(c["map_session"])][int(c["centre_scan"])], pose)
        edge["info"] = lp.info[:]
        out.append((j, edge))
    return out


def align_frames(traj_b, edge, traj_a):
    """B's trajectory expressed in A's frame from one accepted place edge (edge.from a scan of A, edge.to a scan of B, rel the
    pose of B's scan seen from A's): the rigid motion that carries traj_b[edge.to] onto traj_a[edge.from] (+) rel, applied to
    every pose of B -> [n, 3] (tx, ty, th[deg], headings wrapped as Pose2D does).  A usable start for cross_graph."""
    traj_a = np.asarray(traj_a, np.float64).reshape(-1, 3)
    traj_b = np.asarray(traj_b, np.float64).reshape(-1, 3)
    names = getattr(getattr(edge, "dtype", None), "names", None) or ()
    a = traj_a[int(edge["from" if "from" in names else "from_"])]
    b = traj_b[int(edge["to"])]
    rel = np.asarray(edge["rel"], np.float64)
    ca, sa = math.cos(DEG2RAD(a[2])), math.sin(DEG2RAD(a[2]))
    want = np.array([a[0] + ca * rel[0] - sa * rel[1], a[1] + sa * rel[0] + ca * rel[1], add_angle(a[2], rel[2])])     # (calPredPose's composition)
    dth = sub_angle(want[2], b[2])
    c, s = math.cos(DEG2RAD(dth)), math.sin(DEG2RAD(dth))
    out = np.empty_like(traj_b)
    dx, dy = traj_b[:, 0] - b[0], traj_b[:, 1] - b[1]
    out[:, 0] = want[0] + c * dx - s * dy
    out[:, 1] = want[1] + s * dx + c * dy
    out[:, 2] = [add_angle(t, dth) for t in traj_b[:, 2]]
    return out


def _close_cross(ctx, sessions, lc, which):
    """One cross search of the sessions `which` against all, the sessions grouped by the edges found, one batch with a joint
    graph per group, correct() for every session of a group whose graph converged -> the corrected sessions' flags."""
    from . import capi
    S = len(which)
    corrected = np.zeros(S, dtype=np.uint8)
    found = [l for l in sessions.find_cross_loops(lc.cross, which) if l["m"]["loop"]["status"] == 0 and l["m"]["loop"]["found"]]
    if not found:
        return corrected
    root = list(range(S))

    def find(i):
        while root[i] != i:
            root[i] = root[root[i]]
            i = root[i]
        return i
    for l in found:
        a, b = find(int(l["map_session"])), find(int(l["m"]["loop"]["cand"]["session"]))
        root[max(a, b)] = min(a, b)
    groups = collections.OrderedDict()
    for i in sorted({int(l["map_session"]) for l in found} | {int(l["m"]["loop"]["cand"]["session"]) for l in found}):
        groups.setdefault(find(i), []).append(i)
    nodes, arcs, noff, eoff, offsets, n_cross = [], [], [0], [0], [], []
    for members in groups.values():
        place = {i: k for k, i in enumerate(members)}
        cross = [(place[int(l["map_session"])], place[int(l["m"]["loop"]["cand"]["session"])], l["m"]["loop"]["edge"])
                 for l in found if int(l["map_session"]) in place]
        n, e, off = cross_graph([sessions.trajectory(i)[0] for i in members], [[] for _ in members], cross, lc.odo_info)
        nodes.append(n); arcs.append(e); offsets.append(off); n_cross.append(len(cross))
        noff.append(noff[-1] + len(n)); eoff.append(eoff[-1] + len(e))
    new, good = _optimize_closing(ctx, lc, np.concatenate(nodes), np.array(noff, dtype=np.uint64), np.concatenate(arcs),
                                  np.array(eoff, dtype=np.uint64), n_cross)
    fix = {}
    for g, members in enumerate(groups.values()):
        if good[g]:
            for k, i in enumerate(members):
                fix[i] = new[noff[g] + int(offsets[g][k]):noff[g] + int(offsets[g][k + 1])]
    if fix:
        for i in sessions.correct(fix):
            corrected[i] = 1
    return corrected


def _close_loops(ctx, sessions, lc, which):
    """One search over the sessions `which`, one batch of pose graphs for the loops found -- a graph per session, with every
    edge found for it (lc.multi: several) --, correct() for the graphs that converged -> the corrected sessions' flags."""
    from . import capi
    S = len(which)
    corrected = np.zeros(S, dtype=np.uint8)
    multi = getattr(lc, "multi", None)
    loops = sessions.find_loops(lc.loop, which) if multi is None else sessions.find_loops_multi(multi, which)["loop"]
    by_session = collections.OrderedDict()
    for l in loops:
        if l["status"] == 0 and l["found"]:
            by_session.setdefault(int(l["cand"]["session"]), []).append(l["edge"])
    bound = getattr(lc, "consistency", None)
    if bound is not None:                              # the gate: an edge the odometry in between contradicts never reaches a graph
        for i in list(by_session):
            d2 = loop_consistency(ctx, sessions.trajectory(i)[0], lc.odo_info, by_session[i])
            by_session[i] = [e for e, d in zip(by_session[i], d2) if d <= bound]
            if not by_session[i]:
                del by_session[i]
    if not by_session:
        return corrected
    who = list(by_session)
    trajs = [sessions.trajectory(i)[0] for i in who]
    graphs = [loops_graph(t, by_session[i], lc.odo_info) for t, i in zip(trajs, who)]
    off = np.concatenate([[0], np.cumsum([len(t) for t in trajs])]).astype(np.uint64)
    eoff = np.concatenate([[0], np.cumsum([len(g) for g in graphs])]).astype(np.uint64)
    new, good = _optimize_closing(ctx, lc, np.concatenate(trajs), off, np.concatenate(graphs), eoff, [len(by_session[i]) for i in who])
    fix = {i: new[int(off[g]):int(off[g + 1])] for g, i in enumerate(who) if good[g]}
    if fix:
        for i in sessions.correct(fix):
            corrected[i] = 1
    return corrected


def run_sessions_resident(ctx, logs, poses_names=None, map_names=None, separated_map_names=None, sessions=None,
                          occupancy=None, occupancy_names=None, loop_closure=None, **params):
    """run_sessions with every session's state resident on the device: one capi.Sessions set (ndt_sessions_*) over all
    logs, one `step` per lockstep step -- the raw scans and odometry go up, the fused poses come down; scans, submap
    clouds, local maps and NDT maps never leave the device.  The same files and return value as run_sessions
    (start_frame and end_frame reach the set through `active`); the global map is read from the device once per session,
    at its last keyframe step (cnt % keyframe_skip == 0: what saveGlobalMap writes).  One parameter set for all sessions
    (a sweep makes one call per set).  `sessions`: an object with capi.Sessions' interface to use instead of a new
    capi.Sessions(ctx, len(logs), ...) (tests: a host stand-in).
    occupancy: a geometry (x0, y0, res, nx, ny: capi.OccGeometry), or one per log -- one occupancy grid per log
    (capi.OccGrid, or sessions.occ_grid(geometry) where the stand-in has one), every step's scans ray-cast into them
    (sessions.occ_integrate with the records' `stepped` flags), rendered at min_obs = 1 and written with save_occupancy to
    occupancy_names[i] at the end.  None: no grids, nothing else changes.
    loop_closure: None, or an object with LoopClosure's fields.  The set is then created with the scan archive, and behind
    every `every`-th lockstep step come find_loops over the sessions outside their cooldown, one optimize_pose_graphs batch
    for the loops found, correct() for the graphs that end with status 0 and converged, with loop_closure.remake_closed set
    remake_closed(corrected) -- the corrected sessions' closed submaps again from the archive -- and, when grids are in use,
    occ_rebuild(grids, which = corrected, clear = True).  The returned and written poses are then the final trajectories
    (sessions.trajectory(i)), not the poses as the steps gave them.  With loop_closure.cross set, behind that closing of every
    search comes one find_cross_loops (the searched sessions against all; the logs must then share a map frame), one
    optimize_pose_graphs batch with a joint graph (cross_graph) per group of sessions its edges tie together and one correct()
    for every session of a converged group; remake_closed and occ_rebuild then take the sessions either closing corrected.
    A `sessions` object given by the caller must have
    find_loops (else ValueError) and, for the grids, its archive on."""
    from . import capi
    if loop_closure is not None and sessions is not None and not hasattr(sessions, "find_loops"):
        raise ValueError("run_sessions_resident: loop_closure needs a sessions object with find_loops")
    p = dict(LAUNCH_PARAMS)
    p.update(params)
    logs = [list(l) for l in logs]
    S = len(logs)
    if S == 0:
        return []
    own = sessions is None
    if own:
        sessions = capi.Sessions(ctx, S, capi.session_params_from_launch(p), archive=loop_closure is not None)
    lengths = [min(len(l), p["end_frame"]) for l in logs]
    steps_of = [[k for k in range(lengths[i]) if logs[i][k].sid >= p["start_frame"]] for i in range(S)]
    # FrontEnd::process makes the global map when cnt % keyframe_skip == 0 (cnt: scans processed so far): the last such step
    last_key = [(st[((len(st) - 1) // p["keyframe_skip"]) * p["keyframe_skip"]] if st else -1) for st in steps_of]
    poses = [[] for _ in range(S)]
    exported = [(_EMPTY, []) for _ in range(S)]
    empty = np.zeros((0, 2))
    grids, rendered = None, None
    n_steps, quiet_until = 0, [0] * S
    try:
        if occupancy is not None:
            geoms = [occupancy] * S if hasattr(occupancy, "res") else list(occupancy)
            if len(geoms) != S:
                raise ValueError("run_sessions_resident: occupancy needs one geometry, or one per log")
            make = getattr(sessions, "occ_grid", None) or (lambda g: capi.OccGrid(ctx, g))
            grids = []
            for g in geoms:
                grids.append(make(g))
        for k in range(max(lengths, default=0)):
            active = np.array([k < lengths[i] and logs[i][k].sid >= p["start_frame"] for i in range(S)], dtype=np.uint8)
            if not active.any():
                continue
            scans = [logs[i][k].lps if active[i] else empty for i in range(S)]
            odo = [((logs[i][k].pose.tx, logs[i][k].pose.ty, logs[i][k].pose.th) if active[i] else (0.0, 0.0, 0.0))
                   for i in range(S)]
            recs = sessions.step(scans, odo, active)
            if grids is not None:
                sessions.occ_integrate(grids, np.ascontiguousarray(recs["stepped"], dtype=np.uint8))
            for i in range(S):
                if not active[i]:
                    continue
                if not recs[i]["stepped"]:
                    raise capi.NdtError("run_sessions_resident: session %d, scan %d: status %d (a non-finite coordinate)"
                                        % (i, k, int(recs[i]["status"])))
                poses[i].append(Pose2D(*[float(v) for v in recs[i]["pose"]]))
                if k == last_key[i]:
                    g, parts = sessions.global_map(i)
                    exported[i] = (g.copy(), [m.copy() for m in parts])
            n_steps += 1
            if loop_closure is not None and n_steps % loop_closure.every == 0:
                search = np.array([bool(poses[i]) and n_steps >= quiet_until[i] for i in range(S)], dtype=np.uint8)
                corrected = _close_loops(ctx, sessions, loop_closure, search) if search.any() else search
                if getattr(loop_closure, "cross", None) is not None and search.any():
                    corrected = corrected | _close_cross(ctx, sessions, loop_closure, search)
                for i in np.nonzero(corrected)[0]:
                    quiet_until[i] = n_steps + loop_closure.cooldown
                if getattr(loop_closure, "remake_closed", False) and corrected.any():
                    sessions.remake_closed([int(i) for i in np.nonzero(corrected)[0]])
                if grids is not None and corrected.any():
                    sessions.occ_rebuild(grids, corrected, True)
        if loop_closure is not None:
            poses = [[Pose2D(*[float(v) for v in q]) for q in sessions.trajectory(i)[0]] for i in range(S)]
        if grids is not None:
            rendered = [g.render(1) for g in grids]
    finally:
        for g in grids or []:
            g.close()
        if own:
            sessions.close()
    for i in range(S):
        if rendered is not None and occupancy_names and occupancy_names[i]:
            save_occupancy(occupancy_names[i], rendered[i], geoms[i])
        if poses_names and poses_names[i]:
            write_poses(poses_names[i], poses[i])
        if map_names and map_names[i]:
            sep = separated_map_names[i] if separated_map_names and separated_map_names[i] else None
            save_pcd_ascii(map_names[i], exported[i][0])
            for j, m in enumerate(exported[i][1]):
                save_pcd_ascii("%s%d.pcd" % (sep or (map_names[i] + "_sep"), j), m)
    return poses
