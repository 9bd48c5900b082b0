"""ndt_sessions_* and replay.run_sessions_resident without a GPU: the declarations and exports, the bindings' layouts, the
refusals that need no device, the default parameters, and the resident lockstep driver with the oracle standing in for
capi.Sessions."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from ndt_slam_amd import replay, synth
from replay_helpers import OracleEstimator, OracleOps
from session_helpers import OracleSessions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ndt_session_default_params", "ndt_sessions_create", "ndt_sessions_destroy", "ndt_sessions_step",
         "ndt_sessions_step_dev", "ndt_sessions_local_map", "ndt_sessions_submap_cloud", "ndt_sessions_global_map",
         "ndt_sessions_get_stats")


@pytest.fixture(scope="module")
def lib():
    from ndt_slam_amd import build, capi
    build.build()
    return capi.lib()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ndt_mi355x.h")).read(), flags=re.S)


def _fields(src, name):
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), src, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        if not decl.strip():
            continue
        for f in decl.split(None, 1)[-1].split(","):               # (the type is one word in these structs)
            out.append(re.match(r"\s*\*?\s*(\w+)", f).group(1))
    return out


def test_header_declares_capi_lists_and_the_library_exports_the_entry_points(lib):
    src = _header()
    from ndt_slam_amd import capi
    syms = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if l.strip()}
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in capi.EXPORTS
        assert name in exported
        assert getattr(lib, name) is not None
    for struct in ("ndt_session_params", "ndt_session_step", "ndt_sessions_stats", "ndt_sessions"):
        assert re.search(r"\b%s\b" % struct, src)


def test_bindings_have_the_headers_fields_in_order(lib):
    from ndt_slam_amd import capi
    src = _header()
    for struct, cls in (("ndt_session_params", capi.SessionParams), ("ndt_session_step", capi.SessionStep),
                        ("ndt_sessions_stats", capi.SessionsStats)):
        assert [n for n, _ in cls._fields_] == _fields(src, struct), struct
    assert capi.SESSION_STEP_DTYPE.itemsize == ctypes.sizeof(capi.SessionStep)
    assert [capi.SESSION_STEP_DTYPE.fields[n][1] for n, _ in capi.SessionStep._fields_] == \
        [getattr(capi.SessionStep, n).offset for n, _ in capi.SessionStep._fields_]


def test_null_set_and_null_context_are_refused_first(lib):
    """Every other argument is bad too: the NULL set (or context) is what the refusal names."""
    lib.ndt_last_error.restype = ctypes.c_char_p
    vp = ctypes.c_void_p
    assert lib.ndt_sessions_create(None, 0, None, None) == -1
    assert lib.ndt_last_error(None).decode() == "null context"
    for fn, args in ((lib.ndt_sessions_step, (None, None, 3, None, None, None, None)),
                     (lib.ndt_sessions_step_dev, (None, None, 3, None, None, None, None)),
                     (lib.ndt_sessions_local_map, (None, -1, None, None, None)),
                     (lib.ndt_sessions_submap_cloud, (None, -1, None, None)),
                     (lib.ndt_sessions_global_map, (None, -1, None, 0, None, None, None)),
                     (lib.ndt_sessions_get_stats, (None, None)),
                     (lib.ndt_sessions_destroy, (None,))):
        assert fn(*args) == -1, fn
        assert lib.ndt_last_error(None).decode() == "null session set"


def test_default_params_are_the_launch_files(lib):
    from ndt_slam_amd import capi
    p, q = capi.default_session_params(), replay.LAUNCH_PARAMS
    assert p.match.resolution == np.float32(q["Resolution"]) and p.match.step_size == q["StepSize"]
    assert p.match.trans_eps == q["TransformationEpsilon"] and p.match.max_iter == q["MaximumIterations"]
    assert (p.fuse.coe_ndt_cov, p.fuse.coe_vel, p.fuse.coe_omega, p.fuse.del_time, p.fuse.score_thre) == \
        (q["coeNDTCov"], q["coeVel"], q["coeOmega"], q["delTime"], q["score_thre"])
    assert (p.space, p.space_thre, p.resol, p.thre_neighbor, p.sep_thre) == \
        (q["space"], q["space_thre"], q["resol"], q["thre_neighbor"], q["sepThre"])
    assert p.leaf == np.float32(q["LeafSize"]) and p.remove_moving == int(q["removeMoving"])
    # everything else of the match parameters is ndt_default_params, with the shims' grid margin
    d = capi.default_params(resolution=q["Resolution"], step_size=q["StepSize"], trans_eps=q["TransformationEpsilon"],
                            max_iter=q["MaximumIterations"], grid_margin=8)
    assert bytes(p.match) == bytes(d)
    assert bytes(capi.session_params_from_launch(q)) == bytes(p)


def _logs(tmp_path):
    logs = []
    for i, (seed, n) in enumerate(((33, 10), (41, 6), (52, 8))):
        recs, _ = synth.replay_records(n_frames=n, n_beams=121, step=0.6, seed=seed)
        replay.write_log(tmp_path / ("log%d.txt" % i), recs)
        logs.append(tmp_path / ("log%d.txt" % i))
    return logs


def test_resident_lockstep_driver_writes_what_separate_runs_write(oracle, tmp_path):
    """The three logs of test_local_map_batch_host.py (a closing submap, two carried-over scans, keyframe_skip = 3,
    sessions dropping out), all with start_frame = 2 (one parameter set per session set): run_sessions_resident over an
    oracle-backed stand-in for capi.Sessions returns the pose lists and writes the poses, global and per-submap PCD files
    of three separate SlamLauncher.run on the same oracle operations.
    With the stand-in on SlamLauncher's own arithmetic (replay's numpy prediction and fusion) everything is equal to the
    last bit.  With the stand-in on oracle.predict / oracle.fuse -- the reference's expression order in C, which the
    device kernels restate -- the two fusions differ in the last bits of their 3x3 products (fp64, values of order 10,
    fewer than 10 steps: far below 1e-9), so the poses are held to 1e-9 and the files (6 and 8 significant digits) to
    equality."""
    from ndt_slam_amd import capi
    logs = _logs(tmp_path)
    p = dict(replay.LAUNCH_PARAMS, end_frame=20, keyframe_skip=3, sepThre=4.0, start_frame=2)
    solo_poses, solo = [], []
    for i in range(3):
        L = replay.SlamLauncher(OracleOps(oracle), estim=OracleEstimator(oracle, p), **p)
        solo_poses.append(L.run(replay.read_log(logs[i], sidelidar=False), poses_name=tmp_path / ("solo%d.txt" % i),
                                map_name=str(tmp_path / ("solo%d.pcd" % i))))
        solo.append(L)
    assert max(len(L.pcmap.submaps) for L in solo) >= 2          # a submap closed within these frames
    for arith in ("replay", "oracle"):
        stand_in = OracleSessions(oracle, capi, 3, p, arith=arith)
        got = replay.run_sessions_resident(None, [replay.read_log(l, sidelidar=False) for l in logs],
                                           poses_names=[tmp_path / ("res%d.txt" % i) for i in range(3)],
                                           map_names=[str(tmp_path / ("res%d.pcd" % i)) for i in range(3)],
                                           sessions=stand_in, **p)
        # stamps run from 0: start_frame = 2 drops the first two scans of each log
        assert [len(q) for q in got] == [8, 4, 6] == [len(q) for q in solo_poses]
        assert stand_in.steps == 8                                  # steps 2 .. 9: one call each
        for i in range(3):
            a = np.array([(q.tx, q.ty, q.th) for q in got[i]])
            b = np.array([(q.tx, q.ty, q.th) for q in solo_poses[i]])
            if arith == "replay":
                assert a.tobytes() == b.tobytes()
            else:
                assert np.abs(a - b).max() < 1e-9
            assert open(tmp_path / ("res%d.txt" % i)).read() == open(tmp_path / ("solo%d.txt" % i)).read()
            assert open(tmp_path / ("res%d.pcd" % i)).read() == open(tmp_path / ("solo%d.pcd" % i)).read()
            n_sep = len(solo[i].pcmap.maps)
            for k in range(n_sep):
                assert open(tmp_path / ("res%d.pcd_sep%d.pcd" % (i, k))).read() == \
                    open(tmp_path / ("solo%d.pcd_sep%d.pcd" % (i, k))).read()
                os.remove(tmp_path / ("res%d.pcd_sep%d.pcd" % (i, k)))
            assert not os.path.exists(tmp_path / ("res%d.pcd_sep%d.pcd" % (i, n_sep)))
            assert len(stand_in.pcmaps[i].submaps) == len(solo[i].pcmap.submaps)


def test_resident_driver_refuses_a_scan_the_set_skipped(oracle, tmp_path):
    """A record that comes back not stepped for an active session (a non-finite coordinate) is raised, as run_sessions
    raises the resampler's refusal."""
    from ndt_slam_amd import capi
    log = replay.read_log(_logs(tmp_path)[1], sidelidar=False)
    log[2].lps[3, 0] = np.nan
    p = dict(replay.LAUNCH_PARAMS, end_frame=6, sepThre=4.0)
    with pytest.raises(capi.NdtError):
        replay.run_sessions_resident(None, [log], sessions=OracleSessions(oracle, capi, 1, p), **p)


def test_costs_of_the_device_comparison_keep_clear_of_the_accept_threshold(oracle):
    """tests/test_gpu_sessions.py compares the resident path with run_sessions on the four logs of
    test_lockstep_replay_on_the_device and asks for identical accepted lists: on the oracle pipeline every match's cost on
    those logs is below a quarter of score_thre, so no accept decision hangs on the last bits of a fitness score."""
    from ndt_slam_amd import capi
    from session_helpers import lockstep, session_logs
    p = dict(replay.LAUNCH_PARAMS, end_frame=20, sepThre=5.0)
    logs = session_logs(((33, 14), (34, 9), (35, 12), (36, 6)))
    ses = OracleSessions(oracle, capi, 4, p)
    costs = []
    for _, scans, odo, act in lockstep(logs):
        costs += [float(r["cost"]) for r in ses.step(scans, odo, act) if r["matched"]]
    assert len(costs) == 14 + 9 + 12 + 6 - 4
    assert max(costs) < p["score_thre"] / 4, max(costs)
