"""ndt_align_batch_multi{,_dev} and the lockstep replay without a GPU: the declarations and exports, the refusals that
need no device, and replay.run_sessions with the oracle standing in for the device operations."""
import ctypes
import os
import re

import numpy as np
import pytest

from ndt_slam_amd import replay, synth
from replay_helpers import OracleEstimator, OracleOps
from multimap_helpers import OracleBatchEstimate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ndt_align_batch_multi", "ndt_align_batch_multi_dev")


@pytest.fixture(scope="module")
def lib():
    from ndt_slam_amd import build, capi
    build.build()
    return capi.lib()


def test_header_declares_and_capi_exports_the_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ndt_mi355x.h")).read(), flags=re.S)
    from ndt_slam_amd import capi
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in capi.EXPORTS


def test_refusals_without_a_device(lib):
    """Without a device only the NULL-context refusal is reachable: it comes first, before the maps are looked at (the
    n_maps < 1 and maps == NULL refusals with a real context: tests/test_gpu_multimap.py)."""
    scans = np.zeros((4, 2), np.float32)
    off = np.array([0, 4], np.uint64)
    inits = np.zeros((1, 3))
    out = np.zeros(4096, np.uint8)
    one_map = (ctypes.c_void_p * 1)(None)
    for maps, n in ((one_map, 1), (one_map, 0), (None, 1)):
        assert lib.ndt_align_batch_multi(None, maps, n, None, scans.ctypes.data, off.ctypes.data, 1, 0,
                                         inits.ctypes.data, out.ctypes.data) == -1
        assert lib.ndt_align_batch_multi_dev(None, maps, n, None, scans.ctypes.data, off.ctypes.data, 1, 4, 0,
                                             inits.ctypes.data, out.ctypes.data, None) == -1
        assert lib.ndt_last_error(None).decode() == "null context"


def _logs(tmp_path):
    logs = []
    for i, (seed, n) in enumerate(((33, 10), (41, 6), (52, 8))):
        recs, _ = synth.replay_records(n_frames=n, n_beams=121, step=0.6, seed=seed)
        replay.write_log(tmp_path / ("log%d.txt" % i), recs)
        logs.append(tmp_path / ("log%d.txt" % i))
    return logs


def test_lockstep_driver_writes_what_separate_runs_write(oracle, tmp_path):
    """3 sessions of different lengths, one of them with start_frame > 0: run_sessions writes the same pose lists and
    PCD files as 3 separate SlamLauncher.run, and estimates every step's matches in one batch call."""
    logs = _logs(tmp_path)
    base = dict(replay.LAUNCH_PARAMS, end_frame=20, keyframe_skip=3, sepThre=4.0)
    per = [dict(base), dict(base, start_frame=2), dict(base)]

    def launcher(p):
        return replay.SlamLauncher(OracleOps(oracle), estim=OracleEstimator(oracle, p), **p)

    solo_poses = []
    for i, p in enumerate(per):
        solo_poses.append(launcher(p).run(replay.read_log(logs[i], sidelidar=False),
                                          poses_name=tmp_path / ("solo%d.txt" % i),
                                          map_name=str(tmp_path / ("solo%d.pcd" % i))))
    est = OracleBatchEstimate()
    multi_poses = replay.run_sessions(None, [replay.read_log(l, sidelidar=False) for l in logs],
                                      poses_names=[tmp_path / ("multi%d.txt" % i) for i in range(3)],
                                      map_names=[str(tmp_path / ("multi%d.pcd" % i)) for i in range(3)],
                                      estimate=est, launchers=[launcher(p) for p in per])
    for i in range(3):
        assert [(q.tx, q.ty, q.th) for q in multi_poses[i]] == [(q.tx, q.ty, q.th) for q in solo_poses[i]]
        assert open(tmp_path / ("multi%d.txt" % i)).read() == open(tmp_path / ("solo%d.txt" % i)).read()
        assert open(tmp_path / ("multi%d.pcd" % i)).read() == open(tmp_path / ("solo%d.pcd" % i)).read()
        k = 0
        while os.path.exists(tmp_path / ("solo%d.pcd_sep%d.pcd" % (i, k))):
            assert open(tmp_path / ("multi%d.pcd_sep%d.pcd" % (i, k))).read() == \
                open(tmp_path / ("solo%d.pcd_sep%d.pcd" % (i, k))).read()
            k += 1
    assert [len(p) for p in multi_poses] == [10, 4, 8]
    # one batch per step from step 1 on, over the sessions still running; session 1 takes its frame 2 as it is (its first
    # scan) and matches from frame 3 on
    first = [0, 2, 0]
    assert est.calls == [sum(1 for n, f in zip((10, 6, 8), first) if f < k < n) for k in range(1, 10)]
