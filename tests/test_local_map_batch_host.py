"""ndt_local_map_batch{,_dev}, ndt_prefilter_batch and the batched lockstep replay without a GPU: the declarations and
exports, the refusal that needs no device, replay.run_sessions with the oracle standing in for the batched call, and
estimate_poses' one pre-filter call per leaf size."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from ndt_slam_amd import replay, synth
from replay_helpers import OracleEstimator, OracleOps
from multimap_helpers import OracleBatchEstimate
from local_map_helpers import OracleBatchOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ndt_local_map_batch", "ndt_local_map_batch_dev", "ndt_prefilter_batch")


@pytest.fixture(scope="module")
def lib():
    from ndt_slam_amd import build, capi
    build.build()
    return capi.lib()


def test_header_declares_capi_lists_and_the_library_exports_the_entry_points(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ndt_mi355x.h")).read(), flags=re.S)
    from ndt_slam_amd import capi
    syms = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if l.strip()}
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in capi.EXPORTS
        assert name in exported
        assert getattr(lib, name) is not None
    assert re.search(r"\bndt_submap_desc\b", src)
    # the descriptor binds the header's fields, in order
    body = re.search(r"typedef\s+struct\s+ndt_submap_desc\s*\{(.*?)\}\s*ndt_submap_desc\s*;", src, flags=re.S).group(1)
    fields = [f for decl in body.split(";") for f in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.split(None, 1)[-1] if decl.strip() else "")]
    assert [n for n, _ in capi.SubmapDesc._fields_] == [f for f in fields if f]


def test_null_context_is_refused_first(lib):
    """Every other argument is bad too: the NULL context is what the refusal names."""
    for fn, args in (
            (lib.ndt_local_map_batch, (None, None, 0, 3, ctypes.c_float(-1.0), None, None, None, None, None)),
            (lib.ndt_local_map_batch_dev, (None, None, 0, 3, ctypes.c_float(-1.0), None, None, None, None, None, None)),
            (lib.ndt_prefilter_batch, (None, None, 3, None, 0, ctypes.c_float(-1.0), None, None))):
        lib.ndt_last_error.restype = ctypes.c_char_p
        assert fn(*args) == -1
        assert lib.ndt_last_error(None).decode() == "null context"


def _logs(tmp_path):
    logs = []
    for i, (seed, n) in enumerate(((33, 10), (41, 6), (52, 8))):
        recs, _ = synth.replay_records(n_frames=n, n_beams=121, step=0.6, seed=seed)
        replay.write_log(tmp_path / ("log%d.txt" % i), recs)
        logs.append(tmp_path / ("log%d.txt" % i))
    return logs


def test_batched_lockstep_driver_writes_what_separate_runs_write(oracle, tmp_path):
    """3 sessions of different lengths (one with start_frame = 2) sharing one ops object that provides local_maps:
    run_sessions writes the same pose lists, poses files, global and per-submap PCD files as 3 separate
    SlamLauncher.run with plain OracleOps, with ONE local_maps call per step and no make_map / prefilter call.
    Sessions 0 and 2 close their first submap within these frames (a closing submap, a new one with two carried-over
    scans and a previous cloud); keyframe_skip = 3 gives keyframes; session 1's first scan is taken in matchScanBegin at
    step 2; sessions 1 and 2 drop out before session 0 ends."""
    logs = _logs(tmp_path)
    base = dict(replay.LAUNCH_PARAMS, end_frame=20, keyframe_skip=3, sepThre=4.0)
    per = [dict(base), dict(base, start_frame=2), dict(base)]

    solo_poses, solo = [], []
    for i, p in enumerate(per):
        L = replay.SlamLauncher(OracleOps(oracle), estim=OracleEstimator(oracle, p), **p)
        solo_poses.append(L.run(replay.read_log(logs[i], sidelidar=False), poses_name=tmp_path / ("solo%d.txt" % i),
                                map_name=str(tmp_path / ("solo%d.pcd" % i))))
        solo.append(L)
    ops = OracleBatchOps(oracle)
    est = OracleBatchEstimate()
    multi = [replay.SlamLauncher(ops, estim=OracleEstimator(oracle, p), **p) for p in per]
    multi_poses = replay.run_sessions(ops, [replay.read_log(l, sidelidar=False) for l in logs],
                                      poses_names=[tmp_path / ("multi%d.txt" % i) for i in range(3)],
                                      map_names=[str(tmp_path / ("multi%d.pcd" % i)) for i in range(3)],
                                      estimate=est, launchers=multi)
    for i in range(3):
        assert [(q.tx, q.ty, q.th) for q in multi_poses[i]] == [(q.tx, q.ty, q.th) for q in solo_poses[i]]
        assert open(tmp_path / ("multi%d.txt" % i)).read() == open(tmp_path / ("solo%d.txt" % i)).read()
        assert open(tmp_path / ("multi%d.pcd" % i)).read() == open(tmp_path / ("solo%d.pcd" % i)).read()
        n_sep = len(solo[i].pcmap.maps)
        assert n_sep == len(multi[i].pcmap.maps) and len(solo[i].pcmap.submaps) == len(multi[i].pcmap.submaps)   # (maps: as of the last keyframe)
        for k in range(n_sep):
            assert open(tmp_path / ("multi%d.pcd_sep%d.pcd" % (i, k))).read() == \
                open(tmp_path / ("solo%d.pcd_sep%d.pcd" % (i, k))).read()
        assert not os.path.exists(tmp_path / ("solo%d.pcd_sep%d.pcd" % (i, n_sep)))
        assert multi[i].pcmap.localMap_cloud.tobytes() == solo[i].pcmap.localMap_cloud.tobytes()
        assert all(a.p_cloud.tobytes() == b.p_cloud.tobytes() for a, b in zip(multi[i].pcmap.submaps, solo[i].pcmap.submaps))
        assert all(multi[i].smat.accepted)
    assert [len(p) for p in multi_poses] == [10, 4, 8]
    assert [len(L.pcmap.submaps) for L in multi] == [2, 1, 2]
    assert max(len(L.pcmap.submaps) for L in multi) == 2
    # one local_maps call per step in which a session stepped, over exactly the sessions that stepped
    first, n = [0, 2, 0], (10, 6, 8)
    stepped = [sum(1 for f, m in zip(first, n) if f <= k < m) for k in range(10)]
    assert ops.calls == [c for c in stepped if c]
    assert len(ops.calls) == sum(1 for c in stepped if c)
    assert set(ops.leaves) == {base["LeafSize"]}


def test_sessions_with_different_leaf_sizes_go_in_one_call_per_value(oracle, tmp_path):
    logs = _logs(tmp_path)[:2]
    base = dict(replay.LAUNCH_PARAMS, end_frame=4, keyframe_skip=3, sepThre=4.0)
    per = [dict(base), dict(base, LeafSize=0.06)]
    ops = OracleBatchOps(oracle)
    multi = [replay.SlamLauncher(ops, estim=OracleEstimator(oracle, p), **p) for p in per]
    got = replay.run_sessions(ops, [replay.read_log(l, sidelidar=False) for l in logs], estimate=OracleBatchEstimate(),
                              launchers=multi)
    for i, p in enumerate(per):
        want = replay.SlamLauncher(OracleOps(oracle), estim=OracleEstimator(oracle, p), **p).run(
            replay.read_log(logs[i], sidelidar=False))
        assert [(q.tx, q.ty, q.th) for q in got[i]] == [(q.tx, q.ty, q.th) for q in want]
    assert ops.calls == [1] * 8 and sorted(set(ops.leaves)) == [0.05, 0.06]


def test_add_points_is_bookkeeping_plus_make_map(oracle):
    """PointCloudMap.addPoints = addPointsBookkeeping + the returned submap's makeMap."""
    from ndt_slam_amd.pose_estimator import Pose2D
    scans = synth.submap_scans(6, 300, seed=5)
    a, b = replay.PointCloudMap(OracleOps(oracle), sepThre=1.0, removeMoving=True), \
        replay.PointCloudMap(OracleOps(oracle), sepThre=1.0, removeMoving=True)
    for k, sc in enumerate(scans):
        for m in (a, b):
            m.addPose(Pose2D(0.4 * k, 0.0, 0.0))
        a.addPoints(sc)
        b.addPointsBookkeeping(sc).makeMap()
        assert len(a.submaps) == len(b.submaps)
        assert all(x.p_cloud.tobytes() == y.p_cloud.tobytes() and x.cntS == y.cntS and x.cntE == y.cntE and
                   len(x.scans) == len(y.scans) for x, y in zip(a.submaps, b.submaps))
    assert len(a.submaps) >= 2


class _CountingCtx:
    def __init__(self, oracle):
        self.o = oracle
        self.batch_calls = []           # (leaf, number of scans) of every prefilter_batch call
        self.single_calls = 0

    def prefilter_batch(self, scans, leaf):
        scans = list(scans)
        self.batch_calls.append((leaf, len(scans)))
        return [self.o.approx_voxel_filter(np.ascontiguousarray(s, np.float32), leaf) for s in scans]

    def prefilter(self, xy, leaf):
        self.single_calls += 1
        return self.o.approx_voxel_filter(np.ascontiguousarray(xy, np.float32), leaf)


def test_estimate_poses_prefilters_once_per_leaf_size(oracle, monkeypatch):
    from ndt_slam_amd import capi, pose_estimator
    from ndt_slam_amd.pose_estimator import Pose2D, PoseEstimator, Scan2D, estimate_poses
    ctx = _CountingCtx(oracle)
    monkeypatch.setattr(capi, "default_params", lambda *a, **k: object())
    seen = {}

    def build_maps(c, clouds, params, maps=None):
        return [object() for _ in clouds]

    def align_batch_multi(c, maps, scans, offsets, inits, map_of=None, shared_scan=False):
        seen["scans"], seen["offsets"] = np.array(scans), np.array(offsets)
        r = np.zeros(len(inits), dtype=capi.RESULT_DTYPE)
        r["T00"] = 1.0
        r["H"][:] = -np.eye(3).ravel()
        return r

    monkeypatch.setattr(capi, "build_maps", build_maps)
    monkeypatch.setattr(capi, "align_batch_multi", align_batch_multi)
    leaves = [0.05, 0.1, 0.05, 0.05, 0.1]
    es, clouds = [], []
    for k, leaf in enumerate(leaves):
        e = PoseEstimator(ctx=ctx, LeafSize=leaf)
        sc = synth.submap_scans(1, 400 + 50 * k, seed=70 + k)[0]
        e.setScanPair(Scan2D(sc.astype(np.float64)), sc)
        es.append(e); clouds.append(sc)
    out = estimate_poses(es, [Pose2D()] * len(es))
    assert len(out) == len(es)
    assert sorted(ctx.batch_calls) == [(0.05, 3), (0.1, 2)] and ctx.single_calls == 0
    want = [oracle.approx_voxel_filter(np.ascontiguousarray(c, np.float32), l) for c, l in zip(clouds, leaves)]
    assert seen["scans"].tobytes() == np.concatenate(want).tobytes()
    assert list(seen["offsets"]) == list(np.concatenate([[0], np.cumsum([len(w) for w in want])]))
    # the same exception for the same bad input as before: an estimator without a scan pair raises what prefilterSource raises
    bad = PoseEstimator(ctx=ctx, LeafSize=0.05)
    with pytest.raises(Exception) as one:
        bad.prefilterSource()
    with pytest.raises(type(one.value)):
        estimate_poses([es[0], bad], [Pose2D()] * 2)
