"""replay.PointCloudMap.remakeMaps -- the host mirror of ndt_sessions_correct -- over a numpy `ops`, without a GPU: which scan
and which closed cloud moves by which pose pair, the anchor indices, the replaced poses, the untouched travelled distance, and
the `deferred` form run_sessions uses.  The point move is pg_helpers.repose_ref: fp64, one rounding to float32."""
import math

import numpy as np
import pytest

from ndt_slam_amd import replay
from ndt_slam_amd.pose_estimator import Pose2D
from pg_helpers import repose_ref


class NumpyOps:
    """prefilter / make_map / repose_points on the host.  make_map: Submap::makeMap's removeMoving-off branches; prefilter: the
    cloud as it is (a filter that drops nothing keeps every point traceable).  `moves` logs every repose_points call."""

    def __init__(self):
        self.moves = []

    def prefilter(self, xy, leaf):
        return np.ascontiguousarray(xy, np.float32).copy()

    def make_map(self, scans, first, newest, remove, resol, thre):
        assert not remove
        parts = list(scans) if first else list(scans[2:])
        return np.concatenate(parts) if parts else np.zeros((0, 2), np.float32)

    def repose_points(self, clouds, old_poses, new_poses):
        self.moves.append(([np.array(c, np.float32) for c in clouds], np.array(old_poses, np.float64), np.array(new_poses, np.float64)))
        return [repose_ref(np.ascontiguousarray(c, np.float32).reshape(-1, 2), [0, len(c)], [o], [n])
                for c, o, n in zip(clouds, old_poses, new_poses)]


def drive(n, sepThre, deferred, seed=5):
    """n scans of 7 points along a line, 1 m of travel per scan -> (pcmap, ops, the scans in the map frame)."""
    rng = np.random.default_rng(seed)
    ops = NumpyOps()
    pm = replay.PointCloudMap(ops, sepThre=sepThre, removeMoving=False, LeafSize=0.05)
    pm.deferred = deferred
    scans = []
    for k in range(n):
        pose = Pose2D(1.0 * k, 0.1 * k, 2.0 * k)
        cloud = (rng.normal(size=(7, 2)) + (k, 0.0)).astype(np.float32)
        scans.append(cloud)
        pm.addPose(pose)
        pm.addPoints(cloud)
        pm.setLastPose(pose)
        if deferred:
            run_item(pm, ops)
        pm.makeLocalMap()
    return pm, ops, scans


def run_item(pm, ops):
    """What ops.local_maps does with pm.localMapItem(), on the host."""
    scans, first, newest, remove, resol, thre, prev = pm.localMapItem()
    cloud = ops.make_map(scans, first, newest, remove, resol, thre)
    filt = ops.prefilter(cloud, pm.submaps[-1].LeafSize) if len(cloud) else np.zeros((0, 2), np.float32)
    target = filt if prev is None else np.concatenate([prev, filt])
    pm.setLocalMap(cloud, target, 0 if prev is None else len(prev))


def adjusted(pm, start=0):
    out = []
    for k, q in enumerate(pm.poses):
        g = max(k - start + 1, 0)
        out.append(Pose2D(q.tx + 0.02 * g, q.ty - 0.01 * g, q.th + 0.3 * g) if g else q)
    return out


def triple(q):
    return (q.tx, q.ty, q.th)


def moved(cloud, old, new):
    return repose_ref(np.ascontiguousarray(cloud, np.float32), [0, len(cloud)], [triple(old)], [triple(new)])


# (scans, sepThre): no split; splits that carry two scans (every closing submap holds >= 2); splits of one-scan submaps, where
# nothing is carried
CASES = {"no_split": (6, 1e9), "split_with_carry": (8, 2.5), "split_without_carry": (5, 0.5)}


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_remake_maps_moves_each_cloud_by_its_own_pair(case, deferred):
    n, sep = CASES[case]
    pm, ops, scans = drive(n, sep, deferred)
    n_sub = len(pm.submaps)
    assert (n_sub == 1) == (case == "no_split")
    held = len(pm.submaps[-1].scans)
    first = pm.storeFirst()
    assert first == n - held
    if case == "split_with_carry":
        assert n_sub >= 3 and first == pm.submaps[-1].cntS - 2          # the two carried scans come first
    if case == "split_without_carry":
        assert n_sub >= 3 and held == 1 and first == pm.submaps[-1].cntS
    # the store is the tail of the stepped scans
    assert all(pm.submaps[-1].scans[k].tobytes() == scans[first + k].tobytes() for k in range(held))
    old = list(pm.poses)
    new = adjusted(pm)
    atd, closed_before = pm.atd, [s.p_cloud.copy() for s in pm.submaps[:-1]]
    anchors = [pm.anchorScan(m) for m in range(n_sub)]
    for m, sub in enumerate(pm.submaps):
        cntE = sub.cntE if m < n_sub - 1 else n - 1
        assert sub.cntS <= anchors[m] <= cntE and anchors[m] == sub.cntS + (cntE - sub.cntS) // 2
    ops.moves.clear()
    pm.remakeMaps(new)
    # one call: the closed clouds by their anchors' pairs, then every held scan by its own
    assert len(ops.moves) == 1
    clouds, po, pn = ops.moves[0]
    idx = anchors[:-1] + [first + k for k in range(held)]
    assert len(clouds) == len(idx)
    assert po.tobytes() == np.array([triple(old[i]) for i in idx]).tobytes()
    assert pn.tobytes() == np.array([triple(new[i]) for i in idx]).tobytes()
    for m in range(n_sub - 1):
        assert pm.submaps[m].p_cloud.tobytes() == moved(closed_before[m], old[anchors[m]], new[anchors[m]]).tobytes()
    for k in range(held):
        assert pm.submaps[-1].scans[k].tobytes() == moved(scans[first + k], old[first + k], new[first + k]).tobytes()
    # the state around the points
    assert pm.poses == new and pm.lastPose is new[-1] and pm.atd == atd
    if deferred:
        run_item(pm, ops)
    want_cloud = ops.make_map(pm.submaps[-1].scans, pm.submaps[-1].cntS == 0, True, False, 0.05, 0.1)
    assert pm.submaps[-1].p_cloud.tobytes() == want_cloud.tobytes()
    parts = ([pm.submaps[-2].p_cloud] if n_sub >= 2 else []) + [want_cloud]
    assert pm.localMap_cloud.tobytes() == np.concatenate(parts).tobytes()
    # the next addPose measures from the new last pose
    nxt = Pose2D(new[-1].tx + 3.0, new[-1].ty + 4.0, 0.0)
    pm.addPose(nxt)
    assert pm.atd == atd + math.sqrt(3.0 * 3.0 + 4.0 * 4.0)


def test_a_pair_that_does_not_change_keeps_its_bytes():
    pm, ops, scans = drive(8, 2.5, False)
    first_closed = pm.submaps[0]
    start = first_closed.cntE + 1
    before = first_closed.p_cloud.copy()
    other = pm.submaps[1].p_cloud.copy()
    old = list(pm.poses)
    new = adjusted(pm, start=start)
    assert all(new[k] is old[k] for k in range(start)) and pm.anchorScan(0) < start <= pm.anchorScan(1)
    pm.remakeMaps(new)
    assert pm.submaps[0].p_cloud.tobytes() == before.tobytes()
    assert pm.submaps[1].p_cloud.tobytes() != other.tobytes()


def test_a_stale_trajectory_is_refused():
    pm, ops, _ = drive(4, 1e9, False)
    with pytest.raises(ValueError, match="3 new poses for 4 scans"):
        pm.remakeMaps(list(pm.poses)[:-1])
    assert not ops.moves
