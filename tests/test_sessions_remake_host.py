"""replay.closed_scan_ranges (host only): the scan list of every closed submap, against the scans the host mirror
replay.PointCloudMap really held in each submap when it closed -- the very arrays, by identity -- and LoopClosure's new field."""
import numpy as np
import pytest

from ndt_slam_amd import replay
from ndt_slam_amd.pose_estimator import Pose2D


class _NoOps:
    """PointCloudMap's bookkeeping alone."""


def drive(sep_thre, steps):
    """A PointCloudMap stepped along x by `steps` metres per scan (the first scan at 0) -> (the map, every scan's array)."""
    pm = replay.PointCloudMap(_NoOps(), sepThre=sep_thre, removeMoving=True, LeafSize=0.05, resol=0.05, thre_neighbor=0.2)
    pm.deferred = True
    scans, x = [], 0.0
    for k, d in enumerate([0.0] + list(steps)):
        x += d
        cloud = np.full((3, 2), float(k), np.float32)
        scans.append(cloud)
        pm.addPose(Pose2D(x, 0.0, 0.0))
        sub = pm.addPointsBookkeeping(cloud)
        assert sub.scans[-1].tobytes() == cloud.tobytes()
        scans[-1] = sub.scans[-1]                          # (the array the map keeps: addPointsBookkeeping converts)
    return pm, scans


def check(pm, scans):
    n_closed = len(pm.submaps) - 1
    sub_first = [s.cntS for s in pm.submaps]
    ranges = replay.closed_scan_ranges(sub_first, n_closed)
    assert len(ranges) == n_closed
    for m, (first, last) in enumerate(ranges):
        held = pm.submaps[m].scans
        assert last == pm.submaps[m].cntE and last - first + 1 == len(held), (m, first, last, len(held))
        assert all(held[j] is scans[first + j] for j in range(len(held))), m
    return ranges


def test_sep_thre_1_5_carries_two_scans_into_every_later_submap():
    pm, scans = drive(1.5, [0.609] * 11)
    ranges = check(pm, scans)
    assert ranges == [[0, 2], [1, 5], [4, 8]] and len(pm.submaps[-1].scans) == 5


@pytest.mark.parametrize("sep", [0.0, -1.0])
def test_the_empty_first_submap_and_submaps_of_one_scan(sep):
    pm, scans = drive(sep, [0.609] * 4)
    ranges = check(pm, scans)
    # submap 0 closes before it holds a scan; every later one closes with its one own scan and hands nothing on
    assert ranges == [[0, -1], [0, 0], [1, 1], [2, 2], [3, 3]]


def test_a_submap_that_closes_with_exactly_one_scan_hands_none_on():
    pm, scans = drive(0.6, [0.609] * 4)
    assert check(pm, scans) == [[0, 0], [1, 1], [2, 2], [3, 3]]
    # mixed: one scan, then two (carried into the next), then one again behind a long step
    pm, scans = drive(1.0, [1.2, 0.5, 0.6, 0.3, 0.3, 0.5, 2.0, 2.0, 0.1])
    ranges = check(pm, scans)
    assert [b - a + 1 for a, b in ranges] == [len(s.scans) for s in pm.submaps[:-1]]
    assert 1 in [len(s.scans) for s in pm.submaps[:-1]] and max(len(s.scans) for s in pm.submaps[:-1]) >= 4


def test_arguments_and_the_loop_closure_field():
    assert replay.closed_scan_ranges([0], 0) == []
    assert replay.closed_scan_ranges(np.array([0, 3, 6], np.int32), 1) == [[0, 2]]
    with pytest.raises(ValueError):
        replay.closed_scan_ranges([0, 3], 2)
    lc = replay.LoopClosure(loop=None, pg=None, odo_info=None, every=1, cooldown=2)
    assert lc.remake_closed is False
    assert replay.LoopClosure(None, None, None, 1, 2, remake_closed=True).remake_closed is True
