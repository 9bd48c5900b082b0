"""ndt_align_batch_multi{,_dev}: one launch, one map per match (independent SLAM sessions, or one scan against several
candidate submaps).  Every record equals the one ndt_align_batch_dev gives for the same scan, init and map, byte for byte."""
import math

import numpy as np
import pytest

from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu


def wrap(a):
    return (a + math.pi) % (2 * math.pi) - math.pi


def multi_dev(capi, ctx, maps, scans, off, inits, map_of=None, shared_scan=False, stream=None):
    """One ndt_align_batch_multi_dev launch from torch buffers; the records, read back."""
    import torch
    dev = torch.device("cuda", 0)
    d_sc = torch.from_numpy(np.ascontiguousarray(scans, np.float32)).to(dev)
    d_of = torch.from_numpy(np.ascontiguousarray(off, np.uint64).astype(np.int64)).to(dev)
    d_in = torch.from_numpy(np.ascontiguousarray(inits, np.float64).reshape(-1, 3)).to(dev)
    B = len(d_in)
    d_mo = None if map_of is None else torch.from_numpy(np.ascontiguousarray(map_of, np.int32)).to(dev)
    out = torch.zeros(B * capi.RESULT_BYTES, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.align_batch_multi_dev(maps, None if d_mo is None else d_mo.data_ptr(), d_sc.data_ptr(), d_of.data_ptr(), B,
                              len(d_sc), d_in.data_ptr(), out.data_ptr(), shared_scan=shared_scan, stream=stream)
    lib_sync(ctx)
    return np.frombuffer(out.cpu().numpy().tobytes(), dtype=capi.RESULT_DTYPE).copy()


def lib_sync(ctx):
    """Wait on the host for the context's stream (its last launch included: ctx.wait_launch orders the stream behind it)."""
    import torch
    ctx.wait_launch(0, None)
    torch.cuda.ExternalStream(ctx.stream).synchronize()


def single_dev(capi, ctx, gm, scan, init):
    """ndt_align_batch_dev of one scan on one map (B = 1)."""
    import torch
    dev = torch.device("cuda", 0)
    d_sc = torch.from_numpy(np.ascontiguousarray(scan, np.float32)).to(dev)
    d_of = torch.tensor([0, len(scan)], dtype=torch.int64, device=dev)
    d_in = torch.from_numpy(np.ascontiguousarray(init, np.float64).reshape(1, 3)).to(dev)
    out = torch.zeros(capi.RESULT_BYTES, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    gm.align_batch_dev(d_sc.data_ptr(), d_of.data_ptr(), 1, len(scan), d_in.data_ptr(), out.data_ptr(), ctx=ctx)
    lib_sync(ctx)
    return np.frombuffer(out.cpu().numpy().tobytes(), dtype=capi.RESULT_DTYPE).copy()[0]


def per_map(capi, maps, scans, off, inits, map_of):
    """The records of per-map launches (host ndt_align_batch: the same launch as ndt_align_batch_dev), in batch order."""
    B = len(inits)
    out = np.zeros(B, dtype=capi.RESULT_DTYPE)
    for k in sorted(set(int(x) for x in map_of)):
        idx = [b for b in range(B) if int(map_of[b]) == k]
        parts = [scans[int(off[b]):int(off[b + 1])] for b in idx]
        out[idx] = maps[k].align_batch(*capi.pack_scans(parts), inits[idx])
    return out


def test_two_far_apart_maps(gpu):
    capi, ctx = gpu
    from ndt_slam_amd import synth
    cfg = synth.CONFIGS["C1"]
    m = synth.make_map(cfg["n_map"], cfg["half"])
    shifted = np.ascontiguousarray(m + np.float32([50.0, 0.0]), dtype=np.float32)
    prm = capi.default_params(resolution=cfg["resolution"])
    maps = [capi.Map(ctx, m, prm), capi.Map(ctx, shifted, prm)]
    sf = synth.ScanFactory(m, cfg["half"], cfg["n_scan"])
    scans, off, truths, inits = sf.batch(0, 16)
    inits = inits.copy()
    map_of = np.array([b % 2 for b in range(16)], np.int32)
    inits[1::2, 0] += 50.0                                     # the scans of map 1 start at the shifted place
    res = multi_dev(capi, ctx, maps, scans, off, inits, map_of)
    assert np.all(res["status"] == 0)
    for b in range(16):
        one = single_dev(capi, ctx, maps[map_of[b]], scans[int(off[b]):int(off[b + 1])], inits[b])
        assert res[b].tobytes() == one.tobytes(), b
        wrong = single_dev(capi, ctx, maps[1 - map_of[b]], scans[int(off[b]):int(off[b + 1])], inits[b])
        assert res[b].tobytes() != wrong.tobytes(), b
    assert res.tobytes() == capi.align_batch_multi(ctx, maps, scans, off, inits, map_of=map_of).tobytes()


def test_mixed_sizes_in_one_launch(gpu, oracle):
    """64 C1-shaped maps (5k points) and one 1M-point map with wide 10k-point scans (the window is clipped), one resolution."""
    capi, ctx = gpu
    from ndt_slam_amd import synth
    res_m = 0.5
    prm = capi.default_params(resolution=res_m)
    small, factories = [], []
    for k in range(64):
        mk = synth.make_map(5000, 24.0, seed=1000 + k)
        small.append(mk)
        factories.append(synth.ScanFactory(mk, 24.0, 360))
    c2 = synth.CONFIGS["C2"]
    big = synth.make_map(c2["n_map"], c2["half"])
    maps = [capi.Map(ctx, mk, prm) for mk in small] + [capi.Map(ctx, big, prm)]
    wide = synth.ScanFactory(big, c2["half"], c2["n_scan"], radius=48.0)
    parts, inits, map_of = [], [], []
    for b in range(72):
        if b % 9 == 4:
            scan, truth, init = wide.make(b)
            k = 64
        else:
            k = (b * 7) % 64
            scan, truth, init = factories[k].make(b)
        parts.append(scan); inits.append(init); map_of.append(k)
    scans, off = capi.pack_scans(parts)
    inits, map_of = np.array(inits), np.array(map_of, np.int32)
    res = multi_dev(capi, ctx, maps, scans, off, inits, map_of)
    assert np.all(res["status"] == 0)
    ref = per_map(capi, maps, scans, off, inits, map_of)
    assert res.tobytes() == ref.tobytes()
    flagged = (res["flags"] & (capi.FLAG_WINDOW_SPILL | capi.FLAG_REGION_CLIPPED)) != 0
    assert flagged.any(), "no record took the HBM fall-back path"
    for b in (0, 4, 17, 40):
        om = oracle.Map(small[map_of[b]] if map_of[b] < 64 else big, oracle.default_params(resolution=res_m))
        r = om.align(parts[b], inits[b], run_stats=True)
        d = res[b]["pose"] - r["pose"]
        assert int(res[b]["converged"]) == int(r["converged"])
        assert abs(d[0]) <= 1e-4 and abs(d[1]) <= 1e-4 and abs(wrap(d[2])) <= 1e-4


def test_work_sharing_across_maps(gpu):
    """B = 8 scans on 8 maps: helpers join scans of other maps than the one they last read."""
    capi, _ = gpu
    from ndt_slam_amd import synth
    cfg = synth.CONFIGS["C1"]
    prm = capi.default_params(resolution=cfg["resolution"])
    clouds = [synth.make_map(cfg["n_map"], cfg["half"], seed=77 + k) for k in range(8)]
    parts, inits = [], []
    for k in range(8):
        scan, truth, init = synth.ScanFactory(clouds[k], cfg["half"], cfg["n_scan"]).make(k)
        parts.append(scan); inits.append(init)
    scans, off = capi.pack_scans(parts)
    inits = np.array(inits)
    got = []
    for helpers in (0, None, 15):
        ctx = capi.Context(0)
        if helpers is not None:
            ctx.set_option(capi.OPT_MAX_HELPERS, helpers)
        maps = [capi.Map(ctx, c, prm) for c in clouds]
        got.append(multi_dev(capi, ctx, maps, scans, off, inits))          # map_of NULL: scan b on map b
        if helpers == 0:
            ref = per_map(capi, maps, scans, off, inits, np.arange(8))
            assert got[-1].tobytes() == ref.tobytes()
    assert np.all(got[0]["status"] == 0)
    assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes()


def test_shared_scan_against_four_maps(gpu):
    """One scan, 4 candidate maps x 64 seeds: equal to 4 single-map shared_scan launches (far-phase fitness included)."""
    capi, ctx = gpu
    from ndt_slam_amd import synth
    cfg = synth.CONFIGS["C1"]
    prm = capi.default_params(resolution=cfg["resolution"])
    clouds = [synth.make_map(cfg["n_map"], cfg["half"], seed=300 + k) for k in range(4)]
    maps = [capi.Map(ctx, c, prm) for c in clouds]
    scan, truth, _ = synth.ScanFactory(clouds[0], cfg["half"], cfg["n_scan"]).make(0)
    seeds = synth.hypothesis_seeds(truth, count=64, pitch=0.3, yaw_deg=10.0)
    seeds[::5, :2] += 200.0                                    # seeds far off every map: the far phase of the fitness
    off = np.array([0, len(scan)], np.uint64)
    inits = np.concatenate([seeds] * 4)
    map_of = np.repeat(np.arange(4, dtype=np.int32), 64)
    res = multi_dev(capi, ctx, maps, scan, off, inits, map_of, shared_scan=True)
    assert np.all(res["status"] == 0)
    for k in range(4):
        one = maps[k].align_batch(scan, off, seeds, shared_scan=True)
        assert res[64 * k:64 * (k + 1)].tobytes() == one.tobytes(), k
    host = capi.align_batch_multi(ctx, maps, scan, off, inits, map_of=map_of, shared_scan=True)
    assert host.tobytes() == res.tobytes()


def test_bad_map_index_marks_only_its_record(gpu):
    capi, ctx = gpu
    from ndt_slam_amd import synth
    cfg = synth.CONFIGS["C1"]
    prm = capi.default_params(resolution=cfg["resolution"])
    clouds = [synth.make_map(cfg["n_map"], cfg["half"], seed=500 + k) for k in range(3)]
    maps = [capi.Map(ctx, c, prm) for c in clouds]
    parts, inits = [], []
    map_of = np.array([0, 1, -1, 2, 0, 3, 1, 2], np.int32)
    for b in range(8):
        k = int(map_of[b]) if 0 <= map_of[b] < 3 else 0
        scan, truth, init = synth.ScanFactory(clouds[k], cfg["half"], cfg["n_scan"]).make(b)
        parts.append(scan); inits.append(init)
    scans, off = capi.pack_scans(parts)
    inits = np.array(inits)
    for shared in (False, True):
        o = np.array([0, len(parts[0])], np.uint64) if shared else off
        sc = parts[0] if shared else scans
        res = multi_dev(capi, ctx, maps, sc, o, inits, map_of, shared_scan=shared)
        zero = np.zeros(1, dtype=capi.RESULT_DTYPE)[0]
        zero["status"] = -1; zero["fitness"] = np.finfo(np.float64).max
        for b in (2, 5):
            assert int(res[b]["status"]) == -1 and int(res[b]["converged"]) == 0
            assert res[b]["fitness"] == np.finfo(np.float64).max
            assert res[b].tobytes() == zero.tobytes()
        good = [b for b in range(8) if b not in (2, 5)]
        assert np.all(res["status"][good] == 0)
        for b in good:
            if shared:
                one = maps[map_of[b]].align_batch(parts[0], o, inits[b:b + 1], shared_scan=True)[0]
            else:
                one = single_dev(capi, ctx, maps[map_of[b]], parts[b], inits[b])
            assert res[b].tobytes() == one.tobytes(), (shared, b)


def test_mismatched_parameters_are_refused(gpu):
    capi, ctx = gpu
    from ndt_slam_amd import synth
    cfg = synth.CONFIGS["C1"]
    m = synth.make_map(cfg["n_map"], cfg["half"])
    base = capi.Map(ctx, m, capi.default_params(resolution=cfg["resolution"]))
    scan, truth, init = synth.ScanFactory(m, cfg["half"], cfg["n_scan"]).make(0)
    off = np.array([0, len(scan)], np.uint64)
    inits = np.array([init, init])
    ok = capi.Map(ctx, m, capi.default_params(resolution=cfg["resolution"], grid_margin=8))   # build-only: allowed
    assert np.all(capi.align_batch_multi(ctx, [base, ok], scan, off, inits, shared_scan=True)["status"] == 0)
    for other in (capi.default_params(resolution=0.5), capi.default_params("pcl18", resolution=cfg["resolution"])):
        if other.transform_sse == base.params.transform_sse and other.resolution == base.params.resolution:
            continue
        bad = capi.Map(ctx, m, other)
        with pytest.raises(capi.NdtError, match="map 1"):
            capi.align_batch_multi(ctx, [base, bad], scan, off, inits, shared_scan=True)
    with pytest.raises(capi.NdtError, match="n_maps == B"):
        capi.align_batch_multi(ctx, [base], scan, off, inits, shared_scan=True)


def test_refusals_with_a_context(gpu):
    """The argument refusals behind the context check: no maps, a NULL maps array, a NULL map, map_of NULL with
    n_maps != B -- NDT_E_ARG with the reason, nothing queued (the context stays usable)."""
    import ctypes
    capi, ctx = gpu
    from ndt_slam_amd import synth
    cfg = synth.CONFIGS["C1"]
    m = synth.make_map(cfg["n_map"], cfg["half"])
    gm = capi.Map(ctx, m, capi.default_params(resolution=cfg["resolution"]))
    scan, truth, init = synth.ScanFactory(m, cfg["half"], cfg["n_scan"]).make(0)
    off = np.array([0, len(scan)], np.uint64)
    inits = np.array([init, init])
    out = np.zeros(2, dtype=capi.RESULT_DTYPE)
    L = capi.lib()
    one = (ctypes.c_void_p * 1)(gm.h)
    null_one = (ctypes.c_void_p * 1)(None)
    # (maps, n_maps, B, reason); map_of is NULL throughout, so B == n_maps wherever the maps themselves are checked
    cases = ((one, 0, 2, "no maps"), (None, 1, 1, "no maps"), (null_one, 1, 1, "map 0 is NULL"), (one, 1, 2, "n_maps == B"))
    for maps, n, B, why in cases:
        rc = L.ndt_align_batch_multi(ctx.h, maps, n, None, scan.ctypes.data, off.ctypes.data, B, 1, inits.ctypes.data,
                                     out.ctypes.data)
        assert rc == -1 and why in L.ndt_last_error(ctx.h).decode(), (why, L.ndt_last_error(ctx.h))
        rc = L.ndt_align_batch_multi_dev(ctx.h, maps, n, None, scan.ctypes.data, off.ctypes.data, B, len(scan), 1,
                                         inits.ctypes.data, out.ctypes.data, None)
        assert rc == -1 and why in L.ndt_last_error(ctx.h).decode(), (why, L.ndt_last_error(ctx.h))
    res = capi.align_batch_multi(ctx, [gm, gm], scan, off, inits, shared_scan=True)
    assert np.all(res["status"] == 0)


def test_estimate_poses_equals_estimate_pose_and_raises_on_other_parameters(gpu):
    """pose_estimator.estimate_poses: one launch gives what estimatePose gives one estimator at a time; estimators whose
    maps have other match parameters (a Resolution sweep) get the launch's refusal raised, not a not-converged step."""
    capi, ctx = gpu
    from ndt_slam_amd import synth
    from ndt_slam_amd.pose_estimator import Pose2D, PoseEstimator, Scan2D, estimate_poses, RAD2DEG
    cfg = synth.CONFIGS["C1"]
    clouds = [synth.make_map(cfg["n_map"], cfg["half"], seed=1200 + k) for k in range(3)]
    setups = []
    for k, c in enumerate(clouds):
        scan, truth, init = synth.ScanFactory(c, cfg["half"], cfg["n_scan"]).make(k)
        setups.append((Scan2D(scan.astype(np.float64)), c, Pose2D(init[0], init[1], RAD2DEG(init[2]))))

    def estimators(resolutions):
        es = []
        for (sc, c, _), r in zip(setups, resolutions):
            e = PoseEstimator(ctx=ctx, Resolution=r, LeafSize=0.05)
            e.setScanPair(sc, c)
            es.append(e)
        return es

    es = estimators([cfg["resolution"]] * 3)
    got = estimate_poses(es, [p for _, _, p in setups])
    for e, (_, _, p), (cost, est, cov) in zip(es, setups, got):
        c1, e1, v1 = e.estimatePose(p)
        assert cost == c1 and (est.tx, est.ty, est.th) == (e1.tx, e1.ty, e1.th)
        assert np.array_equal(cov, v1, equal_nan=True)
    assert all(c < 0.5 for c, _, _ in got)
    with pytest.raises(capi.NdtError, match="map 1 has other match parameters"):
        estimate_poses(estimators([cfg["resolution"], 0.5, cfg["resolution"]]), [p for _, _, p in setups])


def test_deferred_fitness_and_a_rebuild_behind_the_launch(gpu):
    """NDT_OPT_DEFER_FITNESS: map 1 rebuilt in place right behind a multi-map launch; the records equal the plain launch's."""
    import torch
    capi, _ = gpu
    from ndt_slam_amd import synth
    cfg = synth.CONFIGS["C1"]
    prm = capi.default_params(resolution=cfg["resolution"])
    clouds = [synth.make_map(cfg["n_map"], cfg["half"], seed=900 + k) for k in range(3)]
    parts, inits = [], []
    map_of = np.array([b % 3 for b in range(48)], np.int32)
    for b in range(48):
        scan, truth, init = synth.ScanFactory(clouds[map_of[b]], cfg["half"], cfg["n_scan"]).make(b)
        parts.append(scan); inits.append(init)
    scans, off = capi.pack_scans(parts)
    inits = np.array(inits)
    dev = torch.device("cuda", 0)
    moved = torch.from_numpy(np.ascontiguousarray(clouds[1] + np.float32(0.7), dtype=np.float32)).to(dev)

    def run(defer):
        ctx = capi.Context(0)
        if defer:
            ctx.set_option(capi.OPT_DEFER_FITNESS, 1)
        maps = [capi.Map(ctx, c, prm) for c in clouds]
        d_sc = torch.from_numpy(scans).to(dev)
        d_of = torch.from_numpy(off.astype(np.int64)).to(dev)
        d_in = torch.from_numpy(inits).to(dev)
        d_mo = torch.from_numpy(map_of).to(dev)
        out = torch.zeros(48 * capi.RESULT_BYTES, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.align_batch_multi_dev(maps, d_mo.data_ptr(), d_sc.data_ptr(), d_of.data_ptr(), 48, len(scans),
                                  d_in.data_ptr(), out.data_ptr())
        maps[1].rebuild(dev_ptr=moved.data_ptr(), n=len(moved))            # at once, no wait: it waits for the launch
        lib_sync(ctx)
        return np.frombuffer(out.cpu().numpy().tobytes(), dtype=capi.RESULT_DTYPE).copy()

    plain, deferred = run(False), run(True)
    assert np.all(plain["status"] == 0)
    assert plain.tobytes() == deferred.tobytes()


def test_lockstep_replay_on_the_device(gpu, tmp_path, monkeypatch):
    """4 sessions of different lengths: run_sessions writes what 4 separate SlamLauncher runs write, with one multi-map
    launch per step."""
    capi, ctx = gpu
    from ndt_slam_amd import replay, synth, pose_estimator
    logs = []
    for i, (seed, n) in enumerate(((33, 14), (34, 9), (35, 12), (36, 6))):
        recs, _ = synth.replay_records(n_frames=n, n_beams=181, step=0.6, seed=seed)
        replay.write_log(tmp_path / ("log%d.txt" % i), recs)
        logs.append(replay.read_log(tmp_path / ("log%d.txt" % i), sidelidar=False))
    params = dict(replay.LAUNCH_PARAMS, end_frame=20, sepThre=5.0)
    for i, log in enumerate(logs):
        replay.SlamLauncher(ctx, **params).run(log, poses_name=tmp_path / ("solo%d.txt" % i),
                                               map_name=str(tmp_path / ("solo%d.pcd" % i)))
    logs = [replay.read_log(tmp_path / ("log%d.txt" % i), sidelidar=False) for i in range(4)]
    calls = []
    real = capi.align_batch_multi

    def counted(*a, **k):
        calls.append(len(a[1]))
        return real(*a, **k)

    monkeypatch.setattr(capi, "align_batch_multi", counted)
    replay.run_sessions(ctx, logs, poses_names=[tmp_path / ("multi%d.txt" % i) for i in range(4)],
                        map_names=[str(tmp_path / ("multi%d.pcd" % i)) for i in range(4)], **params)
    for i in range(4):
        assert open(tmp_path / ("multi%d.txt" % i)).read() == open(tmp_path / ("solo%d.txt" % i)).read()
        assert open(tmp_path / ("multi%d.pcd" % i)).read() == open(tmp_path / ("solo%d.pcd" % i)).read()
    # steps 1 .. 13 need a match (step 0 takes every first scan as it is): one launch each, over the sessions still running
    assert calls == [sum(1 for n in (14, 9, 12, 6) if k < n) for k in range(1, 14)]
