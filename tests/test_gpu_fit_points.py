"""ndt_fit_points_batch{,_dev} on the device: every query's float32 distance against brute force over ALL map points
(fitness_workloads.brute_sq) on the sixteen map families, ndt_fit_stats bit for bit against the numpy restatement
(fit_points_helpers.ref_stats) wherever the sums are exact, the shapes at which the reduction can go wrong, shared_scan against
the own-scan form, the launch's own fitness, the ordering against a rebuild, the re-ranked relocalisation and the refusals.
(Written with no MI355X at hand and not yet run on one: LOG.md R18.1.)"""
import math

import numpy as np
import pytest

import fitness_workloads as W
from ndt_slam_amd.capi import pack_scans
from fit_points_helpers import (DBL_MAX, HALF_SCENES, IDENT, describe, half_scene, narrow_pool, ranged_best, ref_stats, stats_tuple,
                                tf_of_pose)
from reloc_helpers import LAT, capi_lattice, pose_error, ref_best
from gpu_support import gpu, sync, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32
LEAVES = (0.05, 0.3, 2.0)
CASES = [(leaf, off) for leaf in LEAVES for off in W.OFFSETS]
STILL = dict(max_iter=0, min_pts=1 << 30)                   # (as tests/test_gpu_fitness_geometry.py: only the raw buckets matter)
SHAPES = (1, 63, 64, 65, 255, 256, 257, 4097, 16385)       # 4097: more than 64 chunks; 16385: more than 256


def sse_of(leaf, off):
    """transform_sse of the maps of one (leaf, offset), alternating as tests/test_gpu_fitness_geometry.py does."""
    return (W.GPU_LEAVES.index(leaf) + W.OFFSETS.index(off) + 1) % 2


def build(gpu, w, sse=1):
    capi, ctx = gpu
    return capi.Map(ctx, w.map, capi.default_params(resolution=w.leaf, transform_sse=sse, **STILL))


def ragged(parts):
    allp, off = pack_scans(parts)
    return (allp if len(allp) else np.zeros((1, 2), F)), off           # (an address for a batch without points)


def poses_of(w):
    b, L = W.lattice_base(w.leaf, w.offset)
    return [(0.0, 0.0, 0.0), (b[0] + 3.7 * L, b[1] - 1.9 * L, 0.6), (b[0] - 40.5 * L, b[1] + 27.25 * L, -2.2)]


_posed = {}


def posed(w, sse):
    """Per pose (the identity and two moved ones): (scan, the four floats passed as tf, queries, brute-force distances);
    computed once per session and workload."""
    key = (w.family, w.leaf, w.offset, sse)
    if key in _posed:
        return _posed[key]
    out = _posed[key] = []
    for k, p in enumerate(poses_of(w)):
        tf = IDENT if k == 0 else tf_of_pose(p)
        scan = w.queries if k == 0 else W.scan_for(w.queries, p)
        q = W.queries_of(scan, tf, sse)
        out.append((scan, tf, q, W.brute_sq(w.map, q)))
    return out


def same_d2(want, got):
    want, got = np.asarray(want, dtype=F), np.asarray(got, dtype=F)
    fin = np.isfinite(want)
    return bool(np.all(np.where(fin, want.view(np.uint32) == got.view(np.uint32), got == np.inf)))


# ------------------------------------------------------------------------------------------ 1: every query
@pytest.mark.parametrize("family", list(W.FAMILIES))
def test_every_query_equals_brute_force(gpu, family):
    """The whole query set of every (leaf, offset), at the identity and through two moved poses, in ONE ragged call: where
    brute force is finite d2 has the same bits, elsewhere it is +inf.  The uncut scans' stats at n 2^-53."""
    for leaf, off in CASES:
        w = W.make(family, leaf, off)
        sse = sse_of(leaf, off)
        gm = build(gpu, w, sse)
        P = posed(w, sse)
        scans, offs = ragged([p[0] for p in P])
        d2, st = gm.fit_points(scans, offs, np.array([p[1] for p in P], dtype=F))
        for k, (scan, tf, q, d) in enumerate(P):
            got = d2[int(offs[k]):int(offs[k + 1])]
            if not same_d2(d, got):
                pytest.fail(describe(w, q, d, got, what=str((family, leaf, off, "pose", k, "sse", sse))))
            fit, fit_all, n_in, n_dist, n = ref_stats(d, DBL_MAX)
            g = stats_tuple(st[k])
            assert g[2:] == (n_in, n_dist, n) and n_in == n_dist, (family, leaf, off, k)
            assert g[0] == g[1] == pytest.approx(fit_all, rel=W.loose_rel(n), abs=0.0), (family, leaf, off, k)
        gm.close()


# ------------------------------------------------------------------------------------------ 2: stats bit for bit
@pytest.mark.parametrize("family", list(W.FAMILIES))
def test_stats_equal_the_restatement_bit_for_bit(gpu, family):
    """The stratified cuts of the three poses' scans as one ragged batch, at five thresholds per workload: every field equal to
    the restatement.  With them a scan out of reach, a scan of NaN points and an empty scan."""
    for leaf, off in CASES:
        w = W.make(family, leaf, off)
        sse = sse_of(leaf, off)
        P = posed(w, sse)
        parts, tfs, dist = [], [], []
        for scan, tf, q, d in P:
            for cut in W.stratify(None, d, 900):
                assert W.sum_is_exact(d[cut])
                parts.append(scan[cut]); tfs.append(tf); dist.append(d[cut])
        n_cuts = len(parts)
        assert n_cuts >= 6, (family, leaf, off, n_cuts)        # (checked here, on the CPU, before the device is asked)
        gone, nan = W.out_of_reach(w.map[0], 70), np.full((3, 2), np.nan, dtype=F)
        for extra in (gone, nan, np.zeros((0, 2), F)):
            parts.append(extra); tfs.append(IDENT); dist.append(np.full(len(extra), np.inf, dtype=F))
        d0 = P[0][3]
        fin = d0[np.isfinite(d0)]
        present = float(fin[len(fin) // 3])
        scans, offs = ragged(parts)
        gm = build(gpu, w, sse)
        compared = 0
        for t in (float(np.median(fin.astype(np.float64))), 0.0, DBL_MAX, present, float(np.nextafter(present, 0.0))):
            _, st = gm.fit_points(scans, offs, np.array(tfs, dtype=F), max_d2=t, want_d2=False)
            for b in range(len(parts)):
                want, got = ref_stats(dist[b], t), stats_tuple(st[b])
                print(family, leaf, off, "threshold %r match %d:" % (t, b), got)
                assert got == want, (family, leaf, off, t, b, got, want)
            compared += n_cuts
            assert stats_tuple(st[n_cuts]) == (DBL_MAX, DBL_MAX, 0, 0, 70)
            assert stats_tuple(st[n_cuts + 1]) == (DBL_MAX, DBL_MAX, 0, 0, 3)
            assert stats_tuple(st[n_cuts + 2]) == (DBL_MAX, DBL_MAX, 0, 0, 0)
        assert compared >= 6 * 5
        gm.close()


# ------------------------------------------------------------------------------------------ 3: the shapes of the reduction
def test_reduction_shapes_batch_order_and_workgroups(gpu):
    """n = 1 .. 16385 on the `sparse` map with distances from one narrow window of binades (every sum exact): every match
    bit-equal to the restatement; the same scans in reversed batch order, each alone with B = 1, and all of it again with
    NDT_OPT_WORKGROUPS = 1, give identical bytes of d2 and stats."""
    capi, ctx = gpu
    w = W.make("sparse", 0.3, W.OFFSETS[0])
    scans, ds = narrow_pool(w, SHAPES)
    gm = build(gpu, w)
    t = float(np.median(np.concatenate(ds).astype(np.float64)))
    tf = np.tile(np.array(IDENT, dtype=F), (len(scans), 1))

    def run():
        allp, offs = ragged(scans)
        d2, st = gm.fit_points(allp, offs, tf, max_d2=t)
        rp, roffs = ragged(scans[::-1])
        d2r, str_ = gm.fit_points(rp, roffs, tf, max_d2=t)
        for b, (scan, d) in enumerate(zip(scans, ds)):
            got = d2[int(offs[b]):int(offs[b + 1])]
            assert got.tobytes() == d.tobytes(), describe(w, scan, d, got, what="n = %d" % len(scan))
            assert stats_tuple(st[b]) == ref_stats(d, t), (len(scan), stats_tuple(st[b]), ref_stats(d, t))
            rb = len(scans) - 1 - b
            assert d2r[int(roffs[rb]):int(roffs[rb + 1])].tobytes() == got.tobytes(), len(scan)
            assert str_[rb].tobytes() == st[b].tobytes(), len(scan)
            d1, s1 = gm.fit_points(scan, np.array([0, len(scan)], np.uint64), tf[:1], max_d2=t)
            assert d1.tobytes() == got.tobytes() and s1[0].tobytes() == st[b].tobytes(), len(scan)
        return d2.tobytes(), st.tobytes()

    first = run()
    assert 0 < ref_stats(ds[-1], t)[2] < len(ds[-1])            # the threshold cuts
    ctx.set_option(capi.OPT_WORKGROUPS, 1)
    try:
        again = run()
    finally:
        ctx.set_option(capi.OPT_WORKGROUPS, 0)
    assert again == first
    gm.close()


# ------------------------------------------------------------------------------------------ 4: shared_scan
def test_shared_scan_rows_equal_the_own_scan_form(gpu):
    """One scan, five transforms (the identity twice, three moved poses): rows 0 and 1 byte-equal, every row and its stats
    equal to the own-scan form of the same (scan, transform), and to brute force."""
    for leaf, off in ((0.3, W.OFFSETS[1]), (2.0, W.OFFSETS[3])):
        w = W.make("sparse", leaf, off)
        sse = sse_of(leaf, off)
        gm = build(gpu, w, sse)
        b, L = W.lattice_base(leaf, off)
        scan = W.scan_for(w.queries, (b[0], b[1], 0.0))          # the queries in a frame at the lattice base
        tfs = np.array([tf_of_pose(p) for p in [(b[0], b[1], 0.0), (b[0], b[1], 0.0), (b[0] + 2.3 * L, b[1] - 3.1 * L, 0.0),
                                                (b[0] + 20.5 * L, b[1] + 23.25 * L, 0.0), (b[0] - 0.4 * L, b[1] + 0.3 * L, 0.002)]], dtype=F)
        n = len(scan)
        t = float((1.5 * L) ** 2)
        d2, st = gm.fit_points(scan, np.array([0, n], np.uint64), tfs, max_d2=t, shared_scan=True)
        own_d2, own_st = gm.fit_points(np.tile(scan, (5, 1)), (np.arange(6) * n).astype(np.uint64), tfs, max_d2=t)
        assert d2.shape == (5 * n,) and d2[:n].tobytes() == d2[n:2 * n].tobytes() and st[0].tobytes() == st[1].tobytes()
        assert d2.tobytes() == own_d2.tobytes() and st.tobytes() == own_st.tobytes()
        for k in range(5):
            q = W.queries_of(scan, tfs[k], sse)
            d = W.brute_sq(w.map, q)
            assert same_d2(d, d2[k * n:(k + 1) * n]), describe(w, q, d, d2[k * n:(k + 1) * n], what=str((leaf, off, "row", k)))
            want, got = ref_stats(d, t), stats_tuple(st[k])
            assert got[2:] == want[2:] and got[0] == pytest.approx(want[0], rel=W.loose_rel(n), abs=0.0)
        gm.close()


# ------------------------------------------------------------------------------------------ 5: against the launch
def test_records_of_a_launch_as_transforms_where_they_lie(gpu, c1_world):
    """align_batch_dev on 8 scans of the C1 world, then fit_points_dev with tf = the address of record 0's T00 and the record
    stride: fitness_all within n 2^-53 of record.fitness, n_dist == n, and n_in at the 0.9 quantile as numpy counts it."""
    import torch
    capi, ctx = gpu
    m, sf, cfg = c1_world
    gm = capi.Map(ctx, m, capi.default_params(resolution=cfg["resolution"]))
    scans, offs, _, inits = sf.batch(0, 8)
    B, total = 8, len(scans)
    dev = torch.device("cuda", 0)
    d_sc, d_off, d_in = to_dev(scans), to_dev(offs.view(np.int64)), to_dev(inits)
    d_rec = torch.zeros(B * capi.RESULT_BYTES, dtype=torch.uint8, device=dev)
    d_d2 = torch.full((total,), -1.0, dtype=torch.float32, device=dev)
    d_st = torch.zeros(B * 32, dtype=torch.uint8, device=dev)
    sync()
    gm.align_batch_dev(d_sc.data_ptr(), d_off.data_ptr(), B, total, d_in.data_ptr(), d_rec.data_ptr())
    tf_ptr = d_rec.data_ptr() + capi.RESULT_DTYPE.fields["T00"][1]
    gm.fit_points_dev(d_sc.data_ptr(), d_off.data_ptr(), B, total, tf_ptr, capi.RESULT_BYTES, DBL_MAX, d_d2.data_ptr(), d_st.data_ptr())
    sync()
    rec = d_rec.cpu().numpy().view(capi.RESULT_DTYPE)
    d2 = d_d2.cpu().numpy()
    st = d_st.cpu().numpy().view(capi.FIT_STATS_DTYPE)
    assert np.all(rec["status"] == 0) and np.isfinite(d2).all()
    for b in range(B):
        n = int(offs[b + 1] - offs[b])
        assert int(st[b]["n_dist"]) == n == int(st[b]["n_points"]) == int(st[b]["n_in"])
        assert float(st[b]["fitness_all"]) == pytest.approx(float(rec[b]["fitness"]), rel=n * 2.0 ** -53, abs=0.0), b
        assert stats_tuple(st[b])[1] == pytest.approx(ref_stats(d2[int(offs[b]):int(offs[b + 1])], DBL_MAX)[1], rel=n * 2.0 ** -53, abs=0.0)
    # the host form with the records as `tf` gives the same bytes; the ranged count at the 0.9 quantile
    h_d2, h_st = gm.fit_points(scans, offs, rec)
    assert h_d2.tobytes() == d2.tobytes() and h_st.tobytes() == st.tobytes()
    t = float(np.quantile(d2.astype(np.float64), 0.9))
    gm.fit_points_dev(d_sc.data_ptr(), d_off.data_ptr(), B, total, tf_ptr, capi.RESULT_BYTES, t, None, d_st.data_ptr())
    sync()
    st = d_st.cpu().numpy().view(capi.FIT_STATS_DTYPE)
    for b in range(B):
        seg = d2[int(offs[b]):int(offs[b + 1])].astype(np.float64)
        assert int(st[b]["n_in"]) == int((seg <= t).sum()), b
        assert float(st[b]["fitness"]) == pytest.approx(ref_stats(seg, t)[0], rel=len(seg) * 2.0 ** -53, abs=0.0)
    assert 0 < int(st["n_in"].sum()) < total
    gm.close()


# ------------------------------------------------------------------------------------------ 6: ordering
def test_a_rebuild_queued_behind_a_call_waits_for_it(gpu, c1_world):
    """ndt_fit_points_batch_dev on another stream, a rebuild of the map on the context's stream right behind it: the call's
    results are those of the call made alone (it read the OLD map), and afterwards the map is the new one."""
    import torch
    capi, ctx = gpu
    m, sf, cfg = c1_world
    prm = capi.default_params(resolution=cfg["resolution"], grid_margin=8)
    old = m
    new = (m[:3000] + np.float32([0.45, -0.3])).astype(np.float32)        # another cloud on (nearly) the same grid
    d_old, d_new = to_dev(old), to_dev(new)
    sync()
    gm = capi.Map(ctx, params=prm, dev_ptr=d_old.data_ptr(), n=len(old))
    scan, truth, _ = sf.make(0)
    B, n = 2048, len(scan)
    rng = np.random.Generator(np.random.Philox(9))
    poses = np.array(truth)[None, :] + rng.uniform(-1, 1, (B, 3)) * np.array([2.0, 2.0, 0.3])
    tfs = np.array([tf_of_pose(p) for p in poses], dtype=F)
    dev = torch.device("cuda", 0)
    d_sc, d_off, d_tf = to_dev(scan), to_dev(np.array([0, n], np.int64)), to_dev(tfs)
    t = float((2 * cfg["resolution"]) ** 2)

    def call(stream=None):
        d_d2 = torch.full((B * n,), -1.0, dtype=torch.float32, device=dev)
        d_st = torch.zeros(B * 32, dtype=torch.uint8, device=dev)
        sync()
        gm.fit_points_dev(d_sc.data_ptr(), d_off.data_ptr(), B, n, d_tf.data_ptr(), 16, t, d_d2.data_ptr(), d_st.data_ptr(),
                          shared_scan=True, stream=stream)
        return d_d2, d_st

    ref_d2, ref_st = call()
    sync()
    ref_d2, ref_st = ref_d2.cpu().numpy(), ref_st.cpu().numpy()
    other = torch.cuda.Stream()
    got_d2, got_st = call(stream=other.cuda_stream)
    gm.rebuild_begin(d_new.data_ptr(), len(new))                           # on the context's stream, directly behind
    gm.rebuild_end()
    sync()
    assert got_d2.cpu().numpy().tobytes() == ref_d2.tobytes() and got_st.cpu().numpy().tobytes() == ref_st.tobytes()
    fresh = capi.Map(ctx, new, prm)                                        # afterwards the map is the new one
    a_d2, a_st = call()
    sync()
    f_d2, f_st = fresh.fit_points(scan, np.array([0, n], np.uint64), tfs, max_d2=t, shared_scan=True)
    assert a_d2.cpu().numpy().tobytes() == f_d2.tobytes() != ref_d2.tobytes()
    assert a_st.cpu().numpy().tobytes() == f_st.tobytes()
    gm.close(); fresh.close()


# ------------------------------------------------------------------------------------------ 7: re-ranked relocalisation
@pytest.mark.parametrize("k,axis,side", HALF_SCENES)
def test_relocalize_in_a_half_covered_map(gpu, c1_world, k, axis, side):
    """The scenes tests/test_fit_points_host.py settles on the oracle.  max_d2 = None: what a plain call returns, byte for byte;
    with max_d2 = (2 leaf)^2 the winner lies within 0.05 m of the truth, where the unbounded mean's lies metres away."""
    capi, ctx = gpu
    m, sf, cfg = c1_world
    leaf = cfg["resolution"]
    hm, scan, truth = half_scene(m, sf, k, axis, side)
    gm = capi.Map(ctx, hm, capi.default_params(resolution=leaf))
    L = capi_lattice(capi, LAT)
    plain = gm.relocalize(scan, L, top_k=16)
    none = gm.relocalize(scan, L, top_k=16, max_d2=None)
    assert sorted(none) == sorted(plain) and none["best"] == plain["best"] == ref_best(plain["records"])
    for key in ("cand_index", "cand_score", "records"):
        assert none[key].tobytes() == plain[key].tobytes(), key
    t = (2 * leaf) ** 2
    out = gm.relocalize(scan, L, top_k=16, max_d2=t)
    assert out["records"].tobytes() == plain["records"].tobytes() and out["best_unbounded"] == plain["best"]
    st = out["fit_stats"]
    assert out["best"] == ranged_best(out["records"], st["fitness"], st["n_in"])
    # the stats are those of one shared-scan call on the records
    _, again = gm.fit_points(scan, np.array([0, len(scan)], np.uint64), out["records"], max_d2=t, shared_scan=True, want_d2=False)
    assert again.tobytes() == st.tobytes()
    err_plain = pose_error(plain["records"][plain["best"]]["pose"], truth)[0]
    err = pose_error(out["records"][out["best"]]["pose"], truth)[0]
    print("scene %r: unbounded winner %.3f m off, ranged winner %.4f m off" % ((k, axis, side), err_plain, err))
    assert err <= 0.05 and out["records"][out["best"]]["converged"]
    assert err_plain > 1.0
    gm.close()
    # the estimator's form: the same ranking, the ranged fitness as the cost
    from ndt_slam_amd.pose_estimator import PoseEstimator, Scan2D
    pe = PoseEstimator(ctx=ctx, Resolution=leaf, LeafSize=1e-4)            # (a leaf that keeps every point)
    pe.setScanPair(Scan2D(scan.astype(np.float64)), hm)
    est, cost = pe.relocalize(L, top_k=16, max_d2=t)
    assert math.hypot(est.tx - truth[0], est.ty - truth[1]) <= 0.05 and cost <= t
    est0, cost0 = pe.relocalize(L, top_k=16)
    assert math.hypot(est0.tx - truth[0], est0.ty - truth[1]) > 1.0


# ------------------------------------------------------------------------------------------ 8: refusals
def test_refusals_return_e_arg_and_write_nothing(gpu, c1_world):
    """Every refusal a caller can provoke through the C ABI on one device, both forms: NDT_E_ARG, d2 and stats keep their
    pattern, and the context stays usable.  (A map that was never built cannot be made through the ABI -- every call that
    creates one builds it -- and a map of another device needs two devices.)"""
    import torch
    capi, ctx = gpu
    m, sf, cfg = c1_world
    lib = capi.lib()
    d_m = to_dev(m)
    sync()
    gm = capi.Map(ctx, params=capi.default_params(resolution=cfg["resolution"]), dev_ptr=d_m.data_ptr(), n=len(m))
    scan, truth, _ = sf.make(0)
    n = len(scan)
    off = np.array([0, n], np.uint64)
    tf = np.array([tf_of_pose(truth)], dtype=F)
    dev = torch.device("cuda", 0)
    d_sc, d_off, d_tf = to_dev(scan), to_dev(off.view(np.int64)), to_dev(tf)
    d_d2 = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
    d_st = torch.full((32,), 0x5a, dtype=torch.uint8, device=dev)
    h_d2 = np.full(n, -7.0, dtype=F)
    h_st = np.full(32, 0x5a, dtype=np.uint8)
    sync()
    sp, op, tp, dp, stp = d_sc.data_ptr(), d_off.data_ptr(), d_tf.data_ptr(), d_d2.data_ptr(), d_st.data_ptr()
    hs, ho, ht, hd, hst = scan.ctypes.data, off.ctypes.data, tf.ctypes.data, h_d2.ctypes.data, h_st.ctypes.data
    nan = float("nan")

    def dev_call(ctx_h=ctx.h, map_h=gm.h, s=sp, o=op, B=1, t=tp, stride=16, max_d2=1.0, d=dp, st=stp):
        return lib.ndt_fit_points_batch_dev(ctx_h, map_h, s, o, B, n, 0, t, stride, max_d2, d, st, None)

    def host_call(ctx_h=ctx.h, map_h=gm.h, s=hs, o=ho, B=1, t=ht, stride=16, max_d2=1.0, d=hd, st=hst):
        return lib.ndt_fit_points_batch(ctx_h, map_h, s, o, B, 0, t, stride, max_d2, d, st)

    def untouched():
        sync()
        return (bool((d_d2.cpu().numpy() == -7.0).all()) and bool((d_st.cpu().numpy() == 0x5a).all())
                and bool((h_d2 == -7.0).all()) and bool((h_st == 0x5a).all()))

    for call in (dev_call, host_call):
        assert call(ctx_h=None) == capi.NDT_E_ARG and lib.ndt_last_error(None) == b"null context"
        for kw in (dict(map_h=None), dict(s=None), dict(o=None), dict(t=None), dict(d=None, st=None), dict(B=0), dict(B=-3),
                   dict(stride=12), dict(stride=18), dict(stride=0), dict(max_d2=nan), dict(max_d2=-1e-300), dict(max_d2=-math.inf)):
            assert call(**kw) == capi.NDT_E_ARG, (call.__name__, kw)
            assert b"ndt_fit_points_batch" in lib.ndt_last_error(ctx.h), kw
        assert untouched()
    bad_off = np.array([5, 2], np.uint64)                                  # host form: offsets that decrease
    assert host_call(o=bad_off.ctypes.data) == capi.NDT_E_ARG and b"monotone" in lib.ndt_last_error(ctx.h)
    if torch.cuda.device_count() > 1:                                      # a map of another device, where there is one
        ctx1 = capi.Context(1)
        other = capi.Map(ctx1, m, capi.default_params(resolution=cfg["resolution"]))
        assert dev_call(map_h=other.h) == capi.NDT_E_ARG and b"another device" in lib.ndt_last_error(ctx.h)
        assert host_call(map_h=other.h) == capi.NDT_E_ARG
        other.close(); ctx1.close()
    # an open ndt_map_rebuild_begin on the context
    gm.rebuild_begin(d_m.data_ptr(), len(m))
    assert dev_call() == capi.NDT_E_ARG and b"ndt_map_rebuild_begin" in lib.ndt_last_error(ctx.h)
    assert host_call() == capi.NDT_E_ARG
    gm.rebuild_end()
    assert untouched()
    # the legal edges are accepted: max_d2 = 0.0, one output alone, a stride of 20; and the context is still usable
    assert dev_call(max_d2=0.0) == 0 and dev_call(d=None) == 0 and dev_call(st=None) == 0
    wide = np.zeros((1, 5), dtype=F); wide[0, :4] = tf[0]
    assert host_call(t=wide.ctypes.data, stride=20, max_d2=DBL_MAX) == 0
    sync()
    d = W.brute_sq(m, W.queries_of(scan, tf[0], bool(gm.params.transform_sse)))
    assert h_d2.tobytes() == d.tobytes() == d_d2.cpu().numpy().tobytes()
    assert stats_tuple(h_st.view(capi.FIT_STATS_DTYPE)[0])[2:] == (n, n, n)
    gm.close()
