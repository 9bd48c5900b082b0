"""The comparison chain of ndt_sessions_correct (tests only): session_helpers.ComposedChain with the correction made of the
existing entry points -- ndt_repose_points for the moves, ndt_local_map_batch_dev for the current submap's cloud and the local
map, ndt_map_build_batch_dev for the map.  Nothing here calls ndt_sessions_trajectory or ndt_sessions_correct."""
import numpy as np

from ndt_slam_amd.pose_estimator import Pose2D
from session_helpers import ComposedChain


def anchor_scan(cntS, cntE):
    """The scan whose pose pair moves a submap's closed cloud: the middle one of its own scans [cntS, cntE]; cntS for a submap
    that closed without a scan of its own."""
    return cntS + (cntE - cntS) // 2 if cntE > cntS else cntS


def layout(pm):
    """(sub_first, sub_anchor, store_first) of a replay.PointCloudMap, from its own bookkeeping: cntS per submap, the anchor
    rule with the newest scan as the current submap's cntE, and where the current submap's scans start among the poses."""
    n = len(pm.poses)
    firsts = [s.cntS for s in pm.submaps]
    lasts = [s.cntE for s in pm.submaps[:-1]] + [n - 1]
    return firsts, [anchor_scan(a, e) for a, e in zip(firsts, lasts)], n - len(pm.submaps[-1].scans)


def smooth_adjustment(poses, scale=1.0, start=0):
    """A pose adjustment as a closed loop spreads it: pose k >= start moved by (k - start + 1) x (1.5 cm, -1 cm, 0.12 deg) x
    scale, the poses before `start` left bit-equal."""
    out = np.array(poses, np.float64).reshape(-1, 3).copy()
    for k in range(start, len(out)):
        g = (k - start + 1) * scale
        out[k] += (0.015 * g, -0.010 * g, 0.12 * g)
    return out


class CorrectedChain(ComposedChain):
    def correct(self, i, new_poses):
        """Session i's state after its trajectory became new_poses ([n, 3]) -> the status the session gets."""
        capi, ctx, pm = self.capi, self.ctx, self.pcmaps[i]
        new_poses = np.ascontiguousarray(new_poses, np.float64).reshape(-1, 3)
        old = np.array([(q.tx, q.ty, q.th) for q in pm.poses], np.float64).reshape(-1, 3)
        assert len(new_poses) == len(old) >= 1
        firsts, anchors, store_first = layout(pm)
        for m, sub in enumerate(pm.submaps[:-1]):
            a = anchors[m]
            sub.p_cloud = capi.repose_points(ctx, np.ascontiguousarray(sub.p_cloud, np.float32).reshape(-1, 2), [0, len(sub.p_cloud)],
                                             old[a:a + 1], new_poses[a:a + 1])
        cur = pm.submaps[-1]
        cur.scans = [capi.repose_points(ctx, np.ascontiguousarray(x, np.float32).reshape(-1, 2), [0, len(x)],
                                        old[store_first + k:store_first + k + 1], new_poses[store_first + k:store_first + k + 1])
                     for k, x in enumerate(cur.scans)]
        pm.poses = [Pose2D(*row) for row in new_poses]
        pm.lastPose = pm.poses[-1]
        self.last_pose[i] = new_poses[-1]
        from local_map_helpers import DevCall
        item = pm.localMapItem()
        call = DevCall(capi, [item])
        call.run(ctx, self.p["LeafSize"])
        self.torch.cuda.synchronize()
        clouds, targets, status = call.results()
        empty = np.zeros((0, 2), np.float32)
        if status[0]:
            pm.setLocalMap(empty, empty, 0)
            self.p_cloud[i], self.target[i] = empty, empty
            return capi.NDT_E_ARG
        n_prev = 0 if item[6] is None else len(item[6])
        pm.setLocalMap(clouds[0], targets[0], n_prev)
        self.p_cloud[i], self.target[i] = clouds[0], targets[0]
        if len(targets[0]):
            self.maps[i] = ctx.build_maps_dev([call.target.data_ptr()], [len(targets[0])], self.params, [self.maps[i]])[0]
        self.torch.cuda.synchronize()
        return capi.NDT_OK
