"""ndt_local_map_batch{,_dev} and ndt_prefilter_batch on the device: every submap of a call against the oracle
(oracle.make_map, oracle.approx_voxel_filter) and against the single calls (ctx.make_map, ctx.prefilter), byte for byte.
There is no tolerance in this file: the batch runs the same arithmetic on the same points in the same order."""
import ctypes

import numpy as np
import pytest

from local_map_helpers import CountingOps, DevCall, capacities, host_call, item_arrays, oracle_local_map, room_scans
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu
EMPTY = np.zeros((0, 2), np.float32)
LEAF = 0.05


def prev_cloud(rng, n):
    return (rng.normal(size=(n, 2)) * 5.0 + np.array([12.0, -3.0])).astype(np.float32)


def mixed_items():
    """13 submaps of mixed shape (see the module's first test)."""
    rng = np.random.default_rng(2024)
    sc = {n: room_scans(np.random.default_rng(n), n, w, m) for n, w, m in ((3, 500, 20), (5, 1500, 60), (12, 4000, 150), (30, 700, 30))}
    small = room_scans(np.random.default_rng(5), 4, 300, 15)
    return [
        (sc[3], True, True, True, 0.05, 0.1, None),
        (sc[5], False, True, True, 0.05, 0.1, prev_cloud(rng, 3000)),
        (sc[12], False, False, True, 0.05, 0.1, prev_cloud(rng, 5000)),
        (sc[30], True, True, True, 0.03, 0.06, None),
        (sc[5], True, True, False, 0.05, 0.1, None),                       # remove_moving off: all scans
        (sc[5], False, True, False, 0.05, 0.1, prev_cloud(rng, 700)),       # remove_moving off: scans 2..
        (small[:1], True, True, True, 0.05, 0.1, None),                    # a lone scan: appended twice
        (small[:2], True, True, True, 0.05, 0.1, prev_cloud(rng, 100)),     # two scans: no triple
        ([small[0], EMPTY, small[2], small[3]], True, True, True, 0.05, 0.1, None),   # an empty middle scan
        ([EMPTY, EMPTY, EMPTY], True, True, True, 0.05, 0.1, prev_cloud(rng, 250)),     # every scan empty
        (sc[5], True, True, True, 0.3, 0.6, None),
        (sc[12][:4], False, True, True, 0.03, 0.06, prev_cloud(rng, 1)),
        (room_scans(np.random.default_rng(77), 12, 900, 30), True, True, True, 0.05, 0.1, None),
    ]


def twins(oracle, ctx, items, leaf):
    """Per item (p_cloud, target, n_prev) from the oracle, checked against the single device calls."""
    out = []
    for it in items:
        p_cloud, target, n_prev = oracle_local_map(oracle, it, leaf)
        assert ctx.make_map(*it[:6]).tobytes() == p_cloud.tobytes()
        if len(p_cloud):
            assert ctx.prefilter(p_cloud, leaf).tobytes() == target[n_prev:].tobytes()
        else:
            assert len(target) == n_prev
        out.append((p_cloud, target, n_prev))
    return out


def assert_equal_to_twins(clouds, targets, want, what=""):
    for s, (p_cloud, target, n_prev) in enumerate(want):
        assert clouds[s].shape == p_cloud.shape and clouds[s].tobytes() == p_cloud.tobytes(), (what, s, "cloud")
        if targets is not None:
            assert targets[s][n_prev:].tobytes() == target[n_prev:].tobytes(), (what, s, "filtered tail")
            assert targets[s].shape == target.shape and targets[s].tobytes() == target.tobytes(), (what, s, "target")


@pytest.fixture(scope="module")
def mixed(gpu, oracle):
    capi, ctx = gpu
    items = mixed_items()
    return items, twins(oracle, ctx, items, LEAF)


def test_mixed_submaps_equal_their_twins(gpu, mixed):
    capi, ctx = gpu
    items, want = mixed
    assert len(items) >= 12
    rc, clouds, targets, status = host_call(capi, ctx, items, LEAF)
    assert rc == 0 and not status.any()
    assert_equal_to_twins(clouds, targets, want)
    checked = 0
    for it, c in zip(items, clouds):
        if it[3] and sum(1 for x in it[0] if len(x)) >= 3:
            assert 0 < len(c) < sum(len(x) for x in it[0])        # something was removed and something stayed
            checked += 1
    assert checked >= 7
    # Context.local_maps: the same, as (p_cloud, target, n_prev)
    for got, (p_cloud, target, n_prev) in zip(ctx.local_maps(items, LEAF), want):
        assert got[0].tobytes() == p_cloud.tobytes() and got[1].tobytes() == target.tobytes() and got[2] == n_prev


def test_both_batch_orders_give_the_same_bytes(gpu, mixed):
    capi, ctx = gpu
    items, want = mixed
    rc, clouds, targets, status = host_call(capi, ctx, items[::-1], LEAF)
    assert rc == 0 and not status.any()
    assert_equal_to_twins(clouds, targets, want[::-1], "reversed")


def test_a_submap_beyond_the_voxel_span_fails_alone(gpu, mixed):
    capi, ctx = gpu
    items, want = mixed
    scans = [x.copy() for x in items[1][0]]
    scans[2][len(scans[2]) // 2] = (1.0e9, 0.0)                  # a point 1e9 m away in a middle scan
    bad = (scans,) + items[1][1:]
    with pytest.raises(capi.NdtError):
        ctx.make_map(*bad[:6])
    k = 4
    call = items[:k] + [bad] + items[k:]
    rc, clouds, targets, status = host_call(capi, ctx, call, LEAF)
    assert rc == 0
    assert status[k] == capi.NDT_E_ARG and not np.delete(status, k).any()
    assert len(clouds[k]) == 0 and len(targets[k]) == 0
    assert_equal_to_twins(clouds[:k] + clouds[k + 1:], targets[:k] + targets[k + 1:], want, "beside the failed one")
    with pytest.raises(capi.NdtError, match="submap %d" % k):
        ctx.local_maps(call, LEAF)
    # the device form, where the failed submap has a previous cloud: empty in both outputs as well
    d = DevCall(capi, call)
    d.run(ctx, LEAF)
    import torch
    torch.cuda.ExternalStream(ctx.stream).synchronize()
    clouds, targets, status = d.results()
    assert status[k] == capi.NDT_E_ARG and len(clouds[k]) == 0 and len(targets[k]) == 0 and bad[6] is not None
    assert_equal_to_twins(clouds[:k] + clouds[k + 1:], targets[:k] + targets[k + 1:], want, "device, beside the failed one")


def test_without_a_target_the_call_is_a_batched_make_map(gpu, mixed):
    import torch
    capi, ctx = gpu
    items, want = mixed
    rc, clouds, targets, status = host_call(capi, ctx, items, -1.0, want_target=False)     # leaf is ignored
    assert rc == 0 and targets is None and not status.any()
    assert_equal_to_twins(clouds, None, want)
    d = DevCall(capi, items, want_target=False)
    d.run(ctx, 0.0)
    torch.cuda.ExternalStream(ctx.stream).synchronize()
    clouds, targets, status = d.results()                                                  # (checks the unused target buffers)
    assert targets is None and not status.any()
    assert_equal_to_twins(clouds, None, want, "device")


def test_device_form_on_a_callers_stream_feeds_the_batched_build(gpu, oracle, mixed):
    import torch
    capi, ctx = gpu
    items, want = mixed
    pick = [s for s, w in enumerate(want) if len(w[1]) > 50]
    items, want = [items[s] for s in pick], [want[s] for s in pick]
    for stride in (8, 16):
        d = DevCall(capi, items, stride=stride)
        stream = torch.cuda.Stream()
        d.run(ctx, LEAF, stream=stream.cuda_stream)
        with torch.cuda.stream(stream):
            toff = d.toff.cpu().numpy()                                    # the one read-back of the offsets
        stream.synchronize()
        prm = capi.default_params(resolution=0.5)
        maps = ctx.build_maps_dev([d.target.data_ptr() + 8 * int(toff[s]) for s in range(len(items))],
                                  [int(toff[s + 1] - toff[s]) for s in range(len(items))], prm)
        torch.cuda.ExternalStream(ctx.stream).synchronize()
        clouds, targets, status = d.results()
        assert not status.any()
        assert_equal_to_twins(clouds, targets, want, "stride %d" % stride)
        for s, (m, w) in enumerate(zip(maps, want)):
            twin = capi.Map(ctx, w[1], prm)
            ea, eb = m.export(), twin.export()
            assert bytes(m.info()) == bytes(twin.info())
            for key in ea:
                assert ea[key].tobytes() == eb[key].tobytes(), (s, key)
            twin.close(); m.close()


def test_calls_of_different_sizes_back_to_back(gpu, oracle, mixed):
    """Scratch grows and is reused, the pinned table of the previous call is waited for; a single make_map in between."""
    capi, ctx0 = gpu
    items, want = mixed
    ctx = capi.Context(0)                                                  # a fresh context: its scratch starts empty
    sets = [[0, 6], [2, 3, 12, 1, 5], [9], list(range(len(items))), [7, 8]]
    single = room_scans(np.random.default_rng(31), 6, 800, 30)
    single_ref = oracle.make_map(single, True, True, True, 0.05, 0.2)
    for rnd in range(2):
        for idx in sets:
            rc, clouds, targets, status = host_call(capi, ctx, [items[s] for s in idx], LEAF)
            assert rc == 0 and not status.any()
            assert_equal_to_twins(clouds, targets, [want[s] for s in idx], (rnd, idx))
            assert ctx.make_map(single, True, True, True, 0.05, 0.2).tobytes() == single_ref.tobytes()
    ctx.close()


def test_every_synchronous_refusal(gpu, mixed):
    capi, ctx = gpu
    L = capi.lib()
    items, _ = mixed
    items = items[:3]
    arrs = [item_arrays(it) for it in items]
    cc, tc = capacities(items)
    canary = np.float32(-4242.0)

    def attempt(code, text, n_subs=3, stride=8, leaf=LEAF, edit=None, null=()):
        descs = (capi.SubmapDesc * 3)()
        for s, (it, (allp, off, prev)) in enumerate(zip(items, arrs)):
            descs[s] = capi.SubmapDesc(allp.ctypes.data, off.ctypes.data, len(it[0]), int(it[1]), int(it[2]), int(it[3]),
                                       float(it[4]), float(it[5]), prev.ctypes.data if len(prev) else None, len(prev))
        hold = edit(descs) if edit else None
        for form in ("ndt_local_map_batch", "ndt_local_map_batch_dev"):
            cloud, target = np.full((cc + 1, 2), canary), np.full((tc + 1, 2), canary)
            coff, toff = np.full(4, 7, np.uint64), np.full(4, 7, np.uint64)
            status = np.full(3, 99, np.int32)
            ptr = dict(subs=descs, cloud=cloud.ctypes.data, coff=coff.ctypes.data, target=target.ctypes.data,
                       toff=toff.ctypes.data, status=status.ctypes.data)
            for k in null:
                ptr[k] = None
            args = [ctx.h, ptr["subs"], n_subs, stride, ctypes.c_float(leaf), ptr["cloud"], ptr["coff"], ptr["target"],
                    ptr["toff"], ptr["status"]]
            if form.endswith("_dev"):
                args.append(None)
            assert getattr(L, form)(*args) == code, (form, text)
            msg = L.ndt_last_error(ctx.h).decode()
            assert msg.startswith(form + ":") and text in msg, (form, text, msg)
            assert np.all(cloud == canary) and np.all(target == canary) and np.all(coff == 7) and np.all(toff == 7) \
                and np.all(status == 99), (form, text)
        del hold

    E = capi.NDT_E_ARG
    attempt(E, "n_subs < 1", n_subs=0)
    attempt(E, "n_subs < 1", n_subs=-3)
    for k in ("subs", "cloud", "coff", "status", "target", "toff"):
        attempt(E, "NULL array", null=(k,))

    def set_field(s, **kw):
        def edit(descs):
            for k, v in kw.items():
                setattr(descs[s], k, v)
        return edit

    attempt(E, "submap 1: n_scans < 1", edit=set_field(1, n_scans=0))
    attempt(E, "submap 2: NULL scans_xy or offsets", edit=set_field(2, scans_xy=None))
    attempt(E, "submap 0: NULL scans_xy or offsets", edit=set_field(0, offsets=None))
    down = arrs[1][1].copy(); down[2] = down[1] - 1
    attempt(E, "submap 1: offsets must be non-decreasing", edit=set_field(1, offsets=down.ctypes.data))
    huge = np.array([0, (1 << 29) + 1], np.uint64)
    attempt(E, "submap 2: offsets must be non-decreasing, scans below 2^29 points",
            edit=set_field(2, offsets=huge.ctypes.data, n_scans=1))
    for stride in (0, 4, 12):
        attempt(E, "bad stride", stride=stride)
    for r in (0.0, -0.05, float("nan"), float("inf")):
        attempt(E, "submap 1: remove_moving needs a positive finite resol", edit=set_field(1, resol=r))
    attempt(E, "submap 0: n_prev > 0 with NULL prev_xy", edit=set_field(0, n_prev=10, prev_xy=None))
    for leaf in (0.0, -1.0, float("nan")):
        attempt(E, "a target needs leaf > 0", leaf=leaf)
    # the first offending index is the one named
    def two(descs):
        descs[2].n_scans = 0
        descs[1].n_scans = -1
    attempt(E, "submap 1: n_scans < 1", edit=two)
    # ndt_prefilter_batch
    out, ooff = np.full((10, 2), canary), np.full(3, 7, np.uint64)
    raw, roff = np.zeros((8, 2), np.float32), np.array([0, 5, 8], np.uint64)
    for text, kw in (("B < 1", dict(B=0)), ("NULL array", dict(roff=None)), ("NULL array", dict(ooff=None)),
                     ("NULL array", dict(raw=None)), ("bad stride", dict(stride=12)), ("leaf <= 0", dict(leaf=0.0)),
                     ("scan 1: offsets decrease", dict(roff=np.array([0, 5, 3], np.uint64).ctypes.data))):
        a = dict(raw=raw.ctypes.data, stride=8, roff=roff.ctypes.data, B=2, leaf=LEAF, ooff=ooff.ctypes.data)
        a.update(kw)
        assert L.ndt_prefilter_batch(ctx.h, a["raw"], a["stride"], a["roff"], a["B"], ctypes.c_float(a["leaf"]),
                                     out.ctypes.data, a["ooff"]) == E, text
        assert text in L.ndt_last_error(ctx.h).decode(), text
        assert np.all(out == canary) and np.all(ooff == 7)
    # a call in which every submap is empty is valid: all-zero offsets
    rc, clouds, targets, status = host_call(capi, ctx, [([EMPTY], True, True, True, 0.05, 0.1, None),
                                                        ([EMPTY, EMPTY, EMPTY], False, False, False, 0.05, 0.1, None)], LEAF)
    assert rc == 0 and not status.any() and all(len(c) == 0 for c in clouds) and all(len(t) == 0 for t in targets)


def test_256_submaps_in_one_call(gpu):
    capi, ctx = gpu
    from ndt_slam_amd import synth
    rng = np.random.default_rng(256)
    items = []
    for s in range(256):
        prev = prev_cloud(rng, 400) if s % 3 == 0 else None
        items.append((synth.submap_scans(12, 1200, seed=21 + s), s % 2 == 0, s % 5 != 0, True, 0.05, 0.2, prev))
    res = ctx.local_maps(items, LEAF)
    for s, (it, (p_cloud, target, n_prev)) in enumerate(zip(items, res)):
        single = ctx.make_map(*it[:6])
        assert p_cloud.tobytes() == single.tobytes(), s
        assert target[n_prev:].tobytes() == ctx.prefilter(single, LEAF).tobytes(), s
        assert n_prev == (0 if it[6] is None else len(it[6])) and target[:n_prev].tobytes() == (EMPTY if it[6] is None else it[6]).tobytes()
        assert 0 < len(single) < 12 * 1200 + 1


def test_prefilter_batch_equals_prefilter_one_by_one(gpu, oracle):
    capi, ctx = gpu
    rng = np.random.default_rng(40)
    sizes = [0, 1, 30000, 0, 64, 513] + [int(v) for v in rng.integers(0, 30001, 34)]
    assert len(sizes) == 40
    scans = [(rng.normal(size=(n, 2)) * 6.0).astype(np.float32) for n in sizes]
    got = ctx.prefilter_batch(scans, LEAF)
    assert len(got) == 40
    for b, (x, g) in enumerate(zip(scans, got)):
        want = ctx.prefilter(x, LEAF) if len(x) else EMPTY
        assert g.shape == want.shape and g.tobytes() == want.tobytes(), b
        if len(x):
            assert g.tobytes() == oracle.approx_voxel_filter(x, LEAF).tobytes(), b
    assert [len(g) for g in ctx.prefilter_batch([EMPTY, EMPTY], LEAF)] == [0, 0]


def test_lockstep_replay_makes_one_local_map_call_per_step(gpu, tmp_path):
    capi, ctx = gpu
    from ndt_slam_amd import replay, synth
    from ndt_slam_amd.pose_estimator import Pose2D, PoseEstimator, Scan2D, estimate_poses, RAD2DEG
    n_frames = (14, 9, 12, 6)
    for i, (seed, n) in enumerate(zip((33, 34, 35, 36), n_frames)):
        recs, _ = synth.replay_records(n_frames=n, n_beams=181, step=0.6, seed=seed)
        replay.write_log(tmp_path / ("log%d.txt" % i), recs)
    read = lambda: [replay.read_log(tmp_path / ("log%d.txt" % i), sidelidar=False) for i in range(4)]
    params = dict(replay.LAUNCH_PARAMS, end_frame=20, sepThre=5.0)
    solo = []
    for i, log in enumerate(read()):
        L = replay.SlamLauncher(ctx, **params)
        L.run(log, poses_name=tmp_path / ("solo%d.txt" % i), map_name=str(tmp_path / ("solo%d.pcd" % i)))
        solo.append(L)
    ops = CountingOps(ctx)
    launchers = [replay.SlamLauncher(ops, **params) for _ in range(4)]
    replay.run_sessions(ops, read(), poses_names=[tmp_path / ("multi%d.txt" % i) for i in range(4)],
                        map_names=[str(tmp_path / ("multi%d.pcd" % i)) for i in range(4)], launchers=launchers)
    for i in range(4):
        assert open(tmp_path / ("multi%d.txt" % i)).read() == open(tmp_path / ("solo%d.txt" % i)).read()
        assert open(tmp_path / ("multi%d.pcd" % i)).read() == open(tmp_path / ("solo%d.pcd" % i)).read()
        assert len(solo[i].pcmap.maps) == len(launchers[i].pcmap.maps)
        for k in range(len(solo[i].pcmap.maps)):
            assert open(tmp_path / ("multi%d.pcd_sep%d.pcd" % (i, k))).read() == \
                open(tmp_path / ("solo%d.pcd_sep%d.pcd" % (i, k))).read()
        assert launchers[i].pcmap.localMap_cloud.tobytes() == solo[i].pcmap.localMap_cloud.tobytes()
    assert ops.local_maps_calls == [sum(1 for n in n_frames if k < n) for k in range(14)]
    assert ops.make_map_calls == 0 and ops.prefilter_calls == 0
    # estimate_poses (one prefilter_batch per leaf size) equals estimatePose one by one
    cfg = synth.CONFIGS["C1"]
    es, inits = [], []
    for k, leaf in enumerate((0.05, 0.08, 0.05)):
        c = synth.make_map(cfg["n_map"], cfg["half"], seed=1500 + k)
        scan, truth, init = synth.ScanFactory(c, cfg["half"], cfg["n_scan"]).make(k)
        e = PoseEstimator(ctx=ctx, Resolution=cfg["resolution"], LeafSize=leaf)
        e.setScanPair(Scan2D(np.repeat(scan, 3, axis=0).astype(np.float64)), c)
        es.append(e); inits.append(Pose2D(init[0], init[1], RAD2DEG(init[2])))
    for e, p, (cost, est, cov) in zip(es, inits, estimate_poses(es, inits)):
        c1, e1, v1 = e.estimatePose(p)
        assert cost == c1 and (est.tx, est.ty, est.th) == (e1.tx, e1.ty, e1.th) and np.array_equal(cov, v1, equal_nan=True)
