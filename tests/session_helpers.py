"""Stand-ins and comparison chains for the device-resident session set (ndt_sessions_*; tests only).

OracleSessions   capi.Sessions' interface on the host: the oracle's match, prediction and fusion around replay's own
                 PointCloudMap -- what drives replay.run_sessions_resident without a GPU.
ComposedChain    the same lockstep step made of the existing *_dev entry points (full recomputation of every scan triple,
                 replay.PointCloudMap's bookkeeping on the host): what ndt_sessions_step must reproduce byte for byte.
DevForm          ndt_sessions_step_dev's arguments from the host form's: the raw scans and the odometry as device tensors at
                 a chosen stride behind a non-zero first offset, sentinels wherever the step must not read.

Both stand-ins take allow_item_failures (default off: a refused item is an assertion failure, as before).  On, they follow
ndt_session_step's per-session rules (include/ndt_mi355x.h): a local-map item whose status is non-zero gives that session
status NDT_E_ARG with empty clouds and its map kept; a refused map build gives the session the build's code and keeps its
previous map, possibly none.
"""
import ctypes

import numpy as np

from ndt_slam_amd import replay
from ndt_slam_amd.pose_estimator import DEG2RAD, Pose2D
from replay_helpers import OracleOps


def step_records(capi, n):
    return np.zeros(n, dtype=capi.SESSION_STEP_DTYPE)


def to_map_frame(lps, pose):
    """ScanMatcher::growMap's transform (replay.ScanMatcher.growMap)."""
    R = Pose2D(*pose).Rmat
    x = R[0][0] * lps[:, 0] + R[0][1] * lps[:, 1] + pose[0]
    y = R[1][0] * lps[:, 0] + R[1][1] * lps[:, 1] + pose[1]
    return np.stack([x, y], axis=1)


class OracleSessions:
    """n sessions with the interface of capi.Sessions (step, global_map, close), on the host."""

    def __init__(self, oracle, capi, n, p, arith="oracle", allow_item_failures=False):
        """arith: "oracle" -- prediction and fusion by oracle.predict / oracle.fuse (C, the reference's expression order,
        what the device kernels restate); "replay" -- by replay's numpy mirrors calMotion / calPredPose / PoseFuser, the
        arithmetic of SlamLauncher itself (the two differ in the last bits of a 3x3 product)."""
        self.o, self.capi, self.n, self.p, self.arith = oracle, capi, n, p, arith
        self.tolerant = allow_item_failures
        self.maps = [None] * n                          # (tolerant: the map a session keeps across a refused step)
        self.pcmaps = [replay.PointCloudMap(OracleOps(oracle), sepThre=p["sepThre"], removeMoving=p["removeMoving"],
                                            LeafSize=p["LeafSize"], resol=p["resol"], thre_neighbor=p["thre_neighbor"])
                       for _ in range(n)]
        self.last_cov = [np.zeros((3, 3)) for _ in range(n)]
        self.prev_odo = [None] * n
        self.prm = oracle.default_params(resolution=p["Resolution"], step_size=p["StepSize"],
                                         trans_eps=p["TransformationEpsilon"], max_iter=p["MaximumIterations"])
        self.fprm = oracle.default_fuse_params(coe_ndt_cov=p["coeNDTCov"], coe_vel=p["coeVel"], coe_omega=p["coeOmega"],
                                               del_time=p["delTime"], score_thre=p["score_thre"])
        self.steps = 0

    def step(self, scans, odo, active=None):
        o, p = self.o, self.p
        out = step_records(self.capi, self.n)
        self.steps += 1
        for i in range(self.n):
            pm = self.pcmaps[i]
            out[i]["submap"] = len(pm.submaps) - 1
            if active is not None and not active[i]:
                continue
            raw = np.asarray(scans[i], np.float64).reshape(-1, 2)
            if not np.isfinite(raw).all():
                out[i]["status"] = -1
                continue
            lps = replay.resample_points(raw, p["space"], p["space_thre"])
            cur = np.asarray(odo[i], np.float64)
            if self.prev_odo[i] is None:
                pose, cov, cost, matched, ok = cur.copy(), np.zeros((3, 3)), 0.0, 0, 1
            else:
                last = pm.getLastPose()
                motion, pred = o.predict(cur, self.prev_odo[i], (last.tx, last.ty, last.th))
                filt = o.approx_voxel_filter(lps.astype(np.float32), p["LeafSize"])
                if not self.tolerant:
                    r = o.Map(np.ascontiguousarray(pm.localMap_cloud, np.float32), self.prm).align(
                        filt, [pred[0], pred[1], DEG2RAD(pred[2])])
                elif self.maps[i] is None or not len(filt):
                    r = np.zeros(1, o.RESULT_DTYPE)[0]          # (no map yet, or no points: nothing converged)
                else:
                    r = self.maps[i].align(filt, [pred[0], pred[1], DEG2RAD(pred[2])])
                cost, matched = (float(r["fitness"]) if r["converged"] and r["status"] == 0 else 1e7), 1
                if self.arith == "oracle":
                    ok, pose, cov = o.fuse(r, pred, motion, (last.tx, last.ty, last.th), self.last_cov[i], self.fprm)
                    cov = np.asarray(cov, np.float64).reshape(3, 3)
                else:
                    pose, cov, ok = self._replay_fuse(r, cur, self.prev_odo[i], last, self.last_cov[i], cost)
            self.last_cov[i], self.prev_odo[i] = cov, cur
            n_sub = len(pm.submaps)
            q = Pose2D(*pose)
            pm.addPose(q)
            if not self.tolerant:
                pm.addPoints(to_map_frame(lps, pose))
                pm.setLastPose(q)
                pm.makeLocalMap()
            else:
                out[i]["status"] = self._tolerant_local_map(pm, i, to_map_frame(lps, pose))
                pm.setLastPose(q)
            out[i]["pose"], out[i]["cov"], out[i]["cost"] = pose, cov.ravel(), cost
            out[i]["stepped"], out[i]["matched"], out[i]["successful"] = 1, matched, int(ok)
            out[i]["submap"], out[i]["split"] = len(pm.submaps) - 1, int(len(pm.submaps) > n_sub)
        return out

    def _tolerant_local_map(self, pm, i, cloud):
        """addPoints + makeLocalMap + the map of the new local map, by the per-session rules -> the record's status."""
        empty = np.zeros((0, 2), np.float32)
        try:
            pm.addPoints(cloud)
        except ValueError:                               # a triple beyond 2^30 voxels: empty clouds, the map kept
            pm.submaps[-1].setMap(empty, empty)
            pm.localMap_cloud = empty
            return self.capi.NDT_E_ARG
        pm.makeLocalMap()
        if len(pm.localMap_cloud):
            try:
                self.maps[i] = self.o.Map(np.ascontiguousarray(pm.localMap_cloud, np.float32), self.prm)
            except RuntimeError:                         # a grid beyond 2^28 cells: the map kept
                return self.capi.NDT_E_GRID
        return self.capi.NDT_OK

    def has_map(self, i):
        return self.maps[i] is not None if self.tolerant else len(self.pcmaps[i].localMap_cloud) > 0

    def _replay_fuse(self, r, cur, prev, last, last_cov, cost):
        """ScanMatcher.matchScanBegin / matchScanEnd's arithmetic on the record of OracleEstimator's match."""
        from ndt_slam_amd.pose_estimator import RAD2DEG
        p = self.p
        motion = replay.calMotion(Pose2D(*cur), Pose2D(*prev))
        pred = replay.calPredPose(motion, last)
        pfu = replay.PoseFuser(p["coeVel"], p["coeOmega"], p["delTime"])
        ok = cost <= p["score_thre"]
        if ok:
            est = Pose2D(float(r["pose"][0]), float(r["pose"][1]), RAD2DEG(float(r["pose"][2])))
            with np.errstate(all="ignore"):
                Q = np.linalg.inv(-np.array(r["H"], float).reshape(3, 3)) * p["coeNDTCov"]
            fused, cov = pfu.fusePose(pred, est, motion, last, last_cov, Q)
        else:
            fused, cov = pred, pfu.calOdometryCovariance(motion, last, last_cov)
        return np.array([fused.tx, fused.ty, fused.th]), cov, int(ok)

    def global_map(self, i):
        pm = self.pcmaps[i]
        pm.makeGlobalMap()
        return pm.globalMap_cloud, list(pm.maps)

    def close(self):
        pass


# ---- the GPU side ----

_HIP = None


def read_device(ptr, nbytes):
    """nbytes at a device address -> bytes (after a device-wide synchronisation)."""
    global _HIP
    import torch
    torch.cuda.synchronize()
    if not nbytes:
        return b""
    if _HIP is None:
        from ndt_slam_amd import capi
        _HIP = capi.lib()                              # (dlsym on the library reaches the HIP runtime it is linked with)
        _HIP.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    buf = ctypes.create_string_buffer(nbytes)
    rc = _HIP.hipMemcpy(buf, ctypes.c_void_p(ptr), nbytes, 2)
    assert rc == 0, rc
    return buf.raw


def device_cloud(ptr, n):
    return np.frombuffer(read_device(ptr, n * 8), dtype=np.float32).reshape(-1, 2).copy()


class _NoOps:
    """PointCloudMap's bookkeeping alone: the chain makes every cloud itself."""


class ComposedChain:
    """S sessions stepped through the existing batched *_dev entry points, the arrays in torch tensors."""

    def __init__(self, capi, ctx, S, p, allow_item_failures=False):
        import torch
        self.torch, self.capi, self.ctx, self.S, self.p = torch, capi, ctx, S, p
        self.tolerant = allow_item_failures
        self.dev = torch.device("cuda", 0)
        self.pcmaps = []
        for _ in range(S):
            pm = replay.PointCloudMap(_NoOps(), sepThre=p["sepThre"], removeMoving=p["removeMoving"], LeafSize=p["LeafSize"],
                                      resol=p["resol"], thre_neighbor=p["thre_neighbor"])
            pm.deferred = True
            self.pcmaps.append(pm)
        self.started = [False] * S
        self.last_pose, self.last_cov, self.prev_odo = np.zeros((S, 3)), np.zeros((S, 9)), np.zeros((S, 3))
        self.maps = [None] * S
        self.params = capi.default_params(resolution=p["Resolution"], step_size=p["StepSize"],
                                          trans_eps=p["TransformationEpsilon"], max_iter=p["MaximumIterations"], grid_margin=8)
        self.fprm = capi.default_fuse_params(coe_ndt_cov=p["coeNDTCov"], coe_vel=p["coeVel"], coe_omega=p["coeOmega"],
                                             del_time=p["delTime"], score_thre=p["score_thre"])
        self.p_cloud = [np.zeros((0, 2), np.float32)] * S
        self.target = [np.zeros((0, 2), np.float32)] * S

    def _t(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def step(self, scans, odo, active=None):
        torch, capi, ctx, S, p = self.torch, self.capi, self.ctx, self.S, self.p
        out = step_records(capi, S)
        act = [True] * S if active is None else [bool(a) for a in active]
        raw, off = capi.pack_scans(scans, np.float64, offsets_dtype=np.int64)
        N = int(off[-1])
        odo = np.ascontiguousarray(odo, np.float64).reshape(S, 3)
        mode = [0 if not act[i] else (2 if self.started[i] else 1) for i in range(S)]
        live = [i for i in range(S) if mode[i] == 2 and self.maps[i] is not None]
        map_of = np.full(S, -1, np.int32)
        for k, i in enumerate(live):
            map_of[i] = k
        cap = capi.resample_capacity(max(N, 1), p["space"], p["space_thre"])
        d_rs64 = torch.zeros((cap, 2), dtype=torch.float64, device=self.dev)
        d_rs32 = torch.zeros((cap, 2), dtype=torch.float32, device=self.dev)
        d_src = torch.zeros((cap, 2), dtype=torch.float32, device=self.dev)
        d_rsoff = torch.zeros(S + 1, dtype=torch.int64, device=self.dev)
        d_srcoff = torch.zeros(S + 1, dtype=torch.int64, device=self.dev)
        d_stat = torch.zeros(S, dtype=torch.int32, device=self.dev)
        d_odo, d_prev, d_last, d_lcov = self._t(odo), self._t(self.prev_odo), self._t(self.last_pose), self._t(self.last_cov)
        d_motion, d_pred, d_init, d_fused = (torch.zeros((S, 3), dtype=torch.float64, device=self.dev) for _ in range(4))
        d_cov = torch.zeros((S, 9), dtype=torch.float64, device=self.dev)
        d_succ = torch.zeros(S, dtype=torch.int32, device=self.dev)
        d_res = torch.zeros(S * capi.RESULT_BYTES, dtype=torch.uint8, device=self.dev)
        d_mapof = self._t(map_of)
        d_mapxy = torch.zeros((cap, 2), dtype=torch.float32, device=self.dev)
        if N:
            d_raw, d_off = self._t(raw), self._t(off)
        torch.cuda.synchronize()                      # (the context works on a stream of its own)
        if N:
            ctx.resample_batch_dev(d_raw.data_ptr(), 16, d_off.data_ptr(), S, N, p["space"], p["space_thre"], d_rs64.data_ptr(),
                                   d_rs32.data_ptr(), d_rsoff.data_ptr(), d_stat.data_ptr())
            ctx.prefilter_batch_dev(d_rs32.data_ptr(), 8, d_rsoff.data_ptr(), S, cap, p["LeafSize"], d_src.data_ptr(),
                                    d_srcoff.data_ptr())
        ctx.predict_batch_dev(d_odo.data_ptr(), d_prev.data_ptr(), d_last.data_ptr(), S, d_motion.data_ptr(), d_pred.data_ptr(),
                              d_init.data_ptr())
        if live and N:
            ctx.align_batch_multi_dev([self.maps[i] for i in live], d_mapof.data_ptr(), d_src.data_ptr(), d_srcoff.data_ptr(), S,
                                      cap, d_init.data_ptr(), d_res.data_ptr())
        ctx.fuse_batch_dev(d_res.data_ptr(), d_pred.data_ptr(), d_motion.data_ptr(), d_last.data_ptr(), d_lcov.data_ptr(), S,
                           self.fprm, d_fused.data_ptr(), d_cov.data_ptr(), d_succ.data_ptr())
        torch.cuda.synchronize()
        res = np.frombuffer(d_res.cpu().numpy().tobytes(), dtype=capi.RESULT_DTYPE)
        fused, cov, succ, stat = d_fused.cpu().numpy(), d_cov.cpu().numpy(), d_succ.cpu().numpy(), d_stat.cpu().numpy()
        rsoff = d_rsoff.cpu().numpy()
        stepped = []
        for i in range(S):
            out[i]["submap"] = len(self.pcmaps[i].submaps) - 1
            if mode[i] == 0:
                continue
            if stat[i] != 0:
                out[i]["status"] = -1
                continue
            if mode[i] == 1:
                out[i]["pose"], out[i]["successful"] = odo[i], 1
            else:
                out[i]["pose"], out[i]["cov"], out[i]["matched"], out[i]["successful"] = fused[i], cov[i], 1, succ[i]
                out[i]["cost"] = res[i]["fitness"] if res[i]["status"] == 0 and res[i]["converged"] else 1e7
            out[i]["stepped"] = 1
            self.last_pose[i], self.last_cov[i], self.prev_odo[i] = out[i]["pose"], out[i]["cov"], odo[i]
            self.started[i] = True
            stepped.append(i)
        if not stepped:
            return out
        # growMap's transform, then PointCloudMap's bookkeeping on the host
        if int(rsoff[S]):
            d_poses = self._t(self.last_pose)
            torch.cuda.synchronize()
            ctx.scan_to_map_batch_dev(d_rs64.data_ptr(), 16, d_rsoff.data_ptr(), S, int(rsoff[S]), d_poses.data_ptr(),
                                      d_mapxy.data_ptr())
        torch.cuda.synchronize()
        mapxy = d_mapxy.cpu().numpy()
        items = []
        for i in stepped:
            pm = self.pcmaps[i]
            n_sub = len(pm.submaps)
            q = Pose2D(*out[i]["pose"])
            pm.addPose(q)
            pm.addPoints(mapxy[int(rsoff[i]):int(rsoff[i + 1])].copy())
            pm.setLastPose(q)
            out[i]["submap"], out[i]["split"] = len(pm.submaps) - 1, int(len(pm.submaps) > n_sub)
            items.append(pm.localMapItem())
        # every triple of every submap again (ndt_local_map_batch_dev), then the maps of the new local maps
        from local_map_helpers import DevCall
        call = DevCall(capi, items)
        call.run(ctx, p["LeafSize"])
        torch.cuda.synchronize()
        clouds, targets, status = call.results()
        if not self.tolerant:
            assert not status.any()
        toff = call.toff.cpu().numpy()
        ptrs, ns, who = [], [], []
        empty = np.zeros((0, 2), np.float32)
        for k, i in enumerate(stepped):
            if status[k]:                                  # this session alone: empty clouds, its map kept
                out[i]["status"] = capi.NDT_E_ARG
                self.pcmaps[i].setLocalMap(empty, empty, 0)
                self.p_cloud[i], self.target[i] = empty, empty
                continue
            n_prev = 0 if items[k][6] is None else len(items[k][6])
            self.pcmaps[i].setLocalMap(clouds[k], targets[k], n_prev)
            self.p_cloud[i], self.target[i] = clouds[k], targets[k]
            if len(targets[k]):
                ptrs.append(call.target.data_ptr() + 8 * int(toff[k])); ns.append(len(targets[k])); who.append(i)
        if who:
            try:
                built = ctx.build_maps_dev(ptrs, ns, self.params, [self.maps[i] for i in who])
            except capi.NdtError:
                if not self.tolerant:
                    raise
                built = []
                for ptr, n, i in zip(ptrs, ns, who):     # the batch is all-or-nothing: each map alone, by the same entry point
                    rc, m = self._build_alone(ptr, n, self.maps[i])
                    out[i]["status"] = rc
                    built.append(m)
            for i, m in zip(who, built):
                self.maps[i] = m
        torch.cuda.synchronize()
        return out

    def _build_alone(self, ptr, n, m):
        """ndt_map_build_batch_dev on one map -> (its code, the map: rebuilt, new, or on a refusal the one given)."""
        capi = self.capi
        xy, nn, P = (ctypes.c_void_p * 1)(ptr), (ctypes.c_size_t * 1)(n), (capi.Params * 1)(self.params)
        mp = (ctypes.c_void_p * 1)(m.h if m is not None else None)
        rc = capi.lib().ndt_map_build_batch_dev(self.ctx.h, xy, nn, 8, 1, P, mp)
        if rc or m is not None:
            return rc, m
        return rc, capi.Map.adopt(self.ctx, mp[0], self.params)

    def has_map(self, i):
        return self.maps[i] is not None

    def global_map(self, i):
        pm = self.pcmaps[i]
        pm.makeGlobalMap()
        return pm.globalMap_cloud, list(pm.maps)

    def close(self):
        for m in self.maps:
            if m is not None:
                m.close()
        self.maps = [None] * self.S


class DevForm:
    """The arguments of ndt_sessions_step_dev for one step: every scan's points as rows of stride / 8 doubles in one device
    tensor, `lead` sentinel rows in front (raw_offsets[0] = lead), a sentinel in every pad column, and sentinel rows in the
    range of every inactive session; the odometry as a device tensor.  The sentinel is finite and far off (a row read by
    mistake moves a cloud, a box or a match; it does not just raise a status)."""
    SENTINEL = 4321.0

    def __init__(self, scans, odo, active, stride=24, lead=5, idle_rows=3):
        import torch
        assert stride in (16, 24, 32) and lead > 0
        S, w = len(scans), stride // 8
        act = [True] * S if active is None else [bool(a) for a in active]
        rows = [np.full((lead, w), self.SENTINEL)]
        off = [lead]
        for i in range(S):
            pts = np.asarray(scans[i], np.float64).reshape(-1, 2) if act[i] else np.full((idle_rows, 2), self.SENTINEL)
            r = np.full((len(pts), w), self.SENTINEL)
            r[:, :2] = pts
            rows.append(r)
            off.append(off[-1] + len(pts))
        rows.append(np.full((2, w), self.SENTINEL))
        dev = torch.device("cuda", 0)
        self.stride, self.offsets = stride, np.array(off, np.uint64)
        self.raw = torch.from_numpy(np.ascontiguousarray(np.concatenate(rows))).to(dev)
        self.odo = torch.from_numpy(np.ascontiguousarray(odo, np.float64).reshape(S, 3)).to(dev)
        torch.cuda.synchronize()

    def step(self, ses, active=None):
        return ses.step_dev(self.raw.data_ptr(), self.stride, self.offsets, self.odo.data_ptr(), active)


RECORD_FIELDS = ("pose", "cov", "cost", "stepped", "matched", "successful", "status", "submap", "split")


def same_records(a, b):
    return all(np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes() for f in RECORD_FIELDS)


def session_logs(specs, n_beams=181, step=0.6):
    """[(seed, n_frames)] -> per session (list of raw scans [n, 2] float64, odometry [n, 3]) from synth.replay_records."""
    from ndt_slam_amd import synth
    logs = []
    for seed, n in specs:
        recs, _ = synth.replay_records(n_frames=n, n_beams=n_beams, step=step, seed=seed)
        logs.append(([np.asarray(r["front"], np.float64).reshape(-1, 2) for r in recs],
                     np.array([[r["x"], r["y"], r["th"]] for r in recs], np.float64)))
    return logs


def lockstep(logs, starts=None):
    """Per step k: (scans, odo, active) over the sessions; session i takes part in steps [starts[i], starts[i] + len)."""
    S = len(logs)
    starts = starts or [0] * S
    empty = np.zeros((0, 2))
    for k in range(max(s + len(l[0]) for s, l in zip(starts, logs))):
        act = np.array([starts[i] <= k < starts[i] + len(logs[i][0]) for i in range(S)], np.uint8)
        scans = [logs[i][0][k - starts[i]] if act[i] else empty for i in range(S)]
        odo = np.array([logs[i][1][k - starts[i]] if act[i] else (0.0, 0.0, 0.0) for i in range(S)])
        yield k, scans, odo, act
