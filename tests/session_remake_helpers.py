"""The comparison chain of ndt_sessions_remake_closed (tests only): session_correct_helpers.CorrectedChain that also keeps every
stepped scan as the resampler gives it (ndt_resample on the raw scan: what a set's archive holds, tests/test_gpu_occ_rebuild.py)
and remakes the closed submaps by the header's Definition out of ndt_scan_to_map_batch_dev and ndt_local_map_batch_dev.
Nothing here calls ndt_sessions_remake_closed or replay.closed_scan_ranges."""
import numpy as np

from local_map_helpers import DevCall
from occ_rebuild_helpers import to_map_dev
from session_correct_helpers import CorrectedChain

EMPTY = np.zeros((0, 2), np.float32)


def scan_lists(cntS, n_scans_total):
    """The Definition's L_m of every closed submap as (first, last) scan indices: cntS = every submap's first own scan (the
    current submap's last), submap m owns [cntS[m], cntS[m + 1] - 1] and holds the last two scans of L_(m-1) in front of
    them, none when that has fewer than two."""
    out, held = [], 0
    for m in range(len(cntS) - 1):
        first = cntS[m] - (2 if m >= 1 and held >= 2 else 0)
        last = cntS[m + 1] - 1
        assert 0 <= first and last < n_scans_total and last >= first - 1
        held = last - first + 1
        out.append((first, last))
    return out


class RemadeChain(CorrectedChain):
    def __init__(self, capi, ctx, S, p, **kw):
        super().__init__(capi, ctx, S, p, **kw)
        self.archive = [[] for _ in range(S)]

    def step(self, scans, odo, active=None):
        out = super().step(scans, odo, active)
        for i in range(self.S):
            if out[i]["stepped"]:
                self.archive[i].append(self.ctx.resample(np.asarray(scans[i], np.float64).reshape(-1, 2), self.p["space"],
                                                         self.p["space_thre"]))
        return out

    def closed_clouds(self, i):
        """(status, the Definition's cloud of every closed submap of session i) at the poses the chain holds now."""
        pm, p = self.pcmaps[i], self.p
        poses = np.array([(q.tx, q.ty, q.th) for q in pm.poses], np.float64).reshape(-1, 3)
        assert len(self.archive[i]) == len(poses)
        cntS = [s.cntS for s in pm.submaps]
        items, where = [], []
        for m, (first, last) in enumerate(scan_lists(cntS, len(poses))):
            if last < first:
                continue
            scans = to_map_dev(self.ctx, self.archive[i][first:last + 1], poses[first:last + 1])
            items.append((scans, cntS[m] == 0, True, p["removeMoving"], p["resol"], p["thre_neighbor"], None))
            where.append(m)
        clouds = [EMPTY] * (len(cntS) - 1)
        if not items:
            return 0, clouds
        call = DevCall(self.capi, items)
        call.run(self.ctx, p["LeafSize"])
        self.torch.cuda.synchronize()
        _, targets, status = call.results()
        if status.any():
            return self.capi.NDT_E_ARG, None
        for m, t in zip(where, targets):
            clouds[m] = t
        return 0, clouds

    def remake(self, i):
        """Session i's closed submaps remade by the Definition, its local map and map behind them -> the session's status."""
        pm = self.pcmaps[i]
        if len(pm.submaps) < 2:
            return self.capi.NDT_OK
        status, clouds = self.closed_clouds(i)
        if status:
            return status                                   # (all or nothing: the session keeps what it had)
        for sub, cloud in zip(pm.submaps[:-1], clouds):
            sub.p_cloud = cloud
        if not len(self.p_cloud[i]):                        # no local map at the moment (a failed step or correction): none now
            return self.capi.NDT_OK
        tail = pm.submaps[-1].filterPoints()                # (the filtered form the last local map was made of: kept)
        target = np.ascontiguousarray(np.concatenate([clouds[-1], tail]), np.float32).reshape(-1, 2)
        pm.setLocalMap(self.p_cloud[i], target, len(clouds[-1]))
        self.target[i] = target
        if len(target):
            d = self.torch.from_numpy(target.copy()).to(self.dev)
            self.torch.cuda.synchronize()
            self.maps[i] = self.ctx.build_maps_dev([d.data_ptr()], [len(target)], self.params, [self.maps[i]])[0]
            self.torch.cuda.synchronize()
        return self.capi.NDT_OK
