"""Many (scan, map, lattice) jobs in one sweep and one pick (ndt_score_lattice_multi_dev, ndt_lattice_select_multi_dev):
every job's volume and candidate list bit for bit against the single-job calls on the same map, scan and lattice."""
import ctypes
import math

import numpy as np
import pytest

from reloc_helpers import crafted_volumes, ref_select
from gpu_support import gpu, sync, to_dev  # noqa: F401
from ndt_slam_amd import replay
from session_helpers import session_logs

pytestmark = pytest.mark.gpu

STAGE_LIMIT = 8000                                   # capi.SCORE_STAGE_POINTS
LENGTHS = (0, 1, 63, 64, 65, 181, STAGE_LIMIT, STAGE_LIMIT + 1)
# (nx, ny, nyaw): lattices of 1, 15, 16, 17 and 1025 poses -- below, at and above a tile of 16, and 64 tiles and one pose
DIMS = {1: (1, 1, 1), 15: (5, 3, 1), 16: (4, 2, 2), 17: (17, 1, 1), 1025: (41, 5, 5)}


class World:
    """Two maps, one scan cut (or tiled) to LENGTHS, and the single-job volumes, each computed once."""

    def __init__(self, capi, ctx, c1_world):
        self.capi, self.ctx = capi, ctx
        m, _, cfg = c1_world
        p = dict(replay.LAUNCH_PARAMS, sepThre=5.0)
        (frames, odo), = session_logs(((33, 12),), n_beams=181)
        ses = capi.Sessions(ctx, 1, capi.session_params_from_launch(p))
        for k in range(12):
            rec = ses.step([frames[k]], odo[k:k + 1])
        closed = ses.global_map(0)[1]
        assert len(closed) >= 2 and len(closed[0]) > 300             # the first submap has closed
        self.pose = (float(rec[0]["pose"][0]), float(rec[0]["pose"][1]), math.radians(float(rec[0]["pose"][2])))
        ses.close()
        prm = capi.default_params(resolution=cfg["resolution"])
        self.maps = [capi.Map(ctx, m, prm), capi.Map(ctx, np.ascontiguousarray(closed[0], np.float32), prm)]
        self.centre = [(0.0, 0.0, 0.3), self.pose]                    # where a job's lattice lies on each map
        scan0 = frames[11].astype(np.float32)
        assert len(scan0) == 181
        rng = np.random.default_rng(11)
        big = (np.tile(scan0, (45, 1)) + rng.normal(0.0, 0.01, (45 * 181, 2))).astype(np.float32)
        self.scans = {n: (scan0[:n] if n <= 181 else big[:n]).copy() for n in LENGTHS}
        self.cache = {}

    def lattice(self, mi, poses, shift=0.0):
        nx, ny, nk = DIMS[poses]
        cx, cy, cyaw = self.centre[mi]
        step = 0.6 if mi == 0 else 0.1
        return self.capi.PoseLattice(cx + shift - step * (nx // 2), cy - step * (ny // 2), cyaw - 0.02 * (nk // 2), step, step, 0.02,
                                     nx, ny, nk)

    def single(self, mi, n, poses, shift=0.0):
        """(score, pairs) of ndt_score_lattice_dev; an empty scan, which that call refuses: zeros."""
        key = (mi, n, poses, shift)
        if key not in self.cache:
            L = self.lattice(mi, poses, shift)
            if n == 0:
                out = np.zeros(L.size), np.zeros(L.size, np.uint32)
            else:
                out = score_single(self.maps[mi], self.scans[n], L)
            for a in out:
                a.setflags(write=False)
            self.cache[key] = out
        return self.cache[key]


@pytest.fixture(scope="module")
def world(gpu, c1_world):
    capi, ctx = gpu
    w = World(capi, ctx, c1_world)
    yield w
    for m in w.maps:
        m.close()


def score_single(gm, scan, L, stream=None):
    import torch
    d_sc = to_dev(scan)
    d_s = torch.full((L.size,), -1.0, dtype=torch.float64, device=d_sc.device)
    d_p = torch.full((L.size,), -1, dtype=torch.int32, device=d_sc.device)
    sync()
    gm.score_lattice(d_sc.data_ptr(), len(scan), L, d_s.data_ptr(), d_p.data_ptr(), stream=stream)
    sync()
    return d_s.cpu().numpy(), d_p.cpu().numpy().view(np.uint32)


class Multi:
    """One multi-job call's device buffers: the packed scans of `lengths`, the volumes, the candidate lists."""

    def __init__(self, w, lengths, jobs):
        """jobs: [(map index, position in `lengths`, poses, shift)]."""
        import torch
        self.w, self.spec = w, jobs
        pts, off = w.capi.pack_scans([w.scans[n] for n in lengths])
        self.lengths, self.total = lengths, len(pts)
        self.d_pts = to_dev(pts if len(pts) else np.zeros((1, 2), np.float32))
        self.d_off = to_dev(off.view(np.int64))
        self.jobs = [(mi, si, w.lattice(mi, poses, shift)) for mi, si, poses, shift in jobs]
        P = sum(L.size for _, _, L in self.jobs)
        dev = self.d_pts.device
        self.d_s = torch.full((P,), -1.0, dtype=torch.float64, device=dev)
        self.d_p = torch.full((P,), -1, dtype=torch.int32, device=dev)
        sync()

    def sweep(self, want_pairs=True, stream=None):
        self.vol = self.w.ctx.score_lattice_multi_dev(self.w.maps, self.d_pts.data_ptr(), self.d_off.data_ptr(), len(self.lengths),
                                                      self.total, self.jobs, self.d_s.data_ptr(),
                                                      self.d_p.data_ptr() if want_pairs else None, stream=stream)
        return self

    def volumes(self):
        sync()
        s, p = self.d_s.cpu().numpy(), self.d_p.cpu().numpy().view(np.uint32)
        v = [int(x) for x in self.vol]
        return [(s[v[j]:v[j + 1]], p[v[j]:v[j + 1]]) for j in range(len(self.jobs))]

    def pick(self, top_k, local_max):
        import torch
        J = len(self.jobs)
        d_c = torch.full((J * top_k,), -1, dtype=torch.int64, device=self.d_s.device)
        d_n = torch.full((J,), -1, dtype=torch.int32, device=self.d_s.device)
        sync()
        self.w.ctx.lattice_select_multi_dev(self.jobs, self.d_s.data_ptr(), self.d_p.data_ptr(), top_k, local_max, d_c.data_ptr(),
                                            d_n.data_ptr())
        sync()
        return d_c.cpu().numpy().reshape(J, top_k), d_n.cpu().numpy()

    def assert_single(self, hits=True):
        """Every job's volume is the single-job call's, to the bit; with `hits`, the call as a whole met the maps."""
        met = 0
        for (mi, si, poses, shift), (s, p) in zip(self.spec, self.volumes()):
            s0, p0 = self.w.single(mi, self.lengths[si], poses, shift)
            assert s.tobytes() == s0.tobytes() and p.tobytes() == p0.tobytes(), (mi, self.lengths[si], poses, shift)
            met += int((p > 0).sum())
        assert met > 0 or not hits


def test_scan_lengths_on_both_sides_of_a_wave_and_of_the_staging_limit(world):
    jobs = [(k % 2, k, 17, 0.0) for k in range(len(LENGTHS))] + [(1, LENGTHS.index(181), 1025, 0.0)]
    m = Multi(world, LENGTHS, jobs).sweep()
    assert m.total > STAGE_LIMIT                                     # 8000 points are staged, 8001 are not
    m.assert_single()
    vols = m.volumes()
    assert (vols[0][0] == 0.0).all() and (vols[0][1] == 0).all()     # the empty scan: 0 and 0 at every pose
    assert (vols[-1][1] > 0).sum() > 500                             # the scan on its own submap: most poses meet it


def test_lattice_sizes_a_one_pose_job_between_large_ones_and_shared_scans(world):
    lengths = (181, 65)
    jobs = [(1, 0, 1025, 0.0), (0, 1, 1, 0.0), (1, 0, 1025, 0.3)]    # one pose between two large jobs
    jobs += [(1, 0, n, 0.0) for n in (1, 15, 16, 17)] + [(0, 0, n, 0.0) for n in (15, 16, 17, 1025)]
    jobs += [(1, 0, 1025, 0.0), (1, 0, 17, 0.0)]                     # jobs that share a scan and a map, and the same job twice
    Multi(world, lengths, jobs).sweep().assert_single()


def test_one_job_and_no_pairs_array(world):
    m = Multi(world, (181,), [(1, 0, 1025, 0.0)]).sweep()
    m.assert_single()
    m = Multi(world, (181,), [(1, 0, 1025, 0.0)]).sweep(want_pairs=False)
    sync()
    assert m.d_s.cpu().numpy().tobytes() == world.single(1, 181, 1025)[0].tobytes()
    assert (m.d_p.cpu().numpy() == -1).all()


SEVEN = [(1, 0, 1025, 0.0), (0, 1, 17, 0.0), (1, 2, 16, 0.0), (0, 0, 1025, 0.0), (1, 1, 1, 0.0), (1, 0, 15, 0.3), (0, 2, 1025, 0.0)]


@pytest.mark.parametrize("workgroups", [1, 3])
def test_workgroups_that_cross_job_boundaries(world, workgroups):
    world.ctx.set_option(world.capi.OPT_WORKGROUPS, workgroups)
    try:
        m = Multi(world, (181, 64, 63), SEVEN).sweep()
        sync()
    finally:
        world.ctx.set_option(world.capi.OPT_WORKGROUPS, 0)
    m.assert_single()


def test_without_staging_and_in_reverse_order(world):
    world.ctx.set_option(world.capi.OPT_SCORE_STAGE, 0)
    try:
        m = Multi(world, (181, 64, 63), SEVEN).sweep()
        sync()
    finally:
        world.ctx.set_option(world.capi.OPT_SCORE_STAGE, 1)
    m.assert_single()
    Multi(world, (181, 64, 63), SEVEN[::-1]).sweep().assert_single()


def select_single(gm, L, d_s, d_p, at, top_k, local_max):
    import torch
    d_c = torch.full((top_k,), -1, dtype=torch.int64, device=d_s.device)
    d_n = torch.full((1,), -1, dtype=torch.int32, device=d_s.device)
    sync()
    gm.lattice_select(L, d_s.data_ptr() + 8 * at, d_p.data_ptr() + 4 * at, top_k, local_max, d_c.data_ptr(), d_n.data_ptr())
    sync()
    n = int(d_n.cpu()[0])
    return d_c.cpu().numpy()[:n], n


@pytest.mark.parametrize("top_k,local_max", [(1, 1), (4, 1), (16, 0), (16, 1)])
def test_pick_on_the_sweeps_volumes(world, top_k, local_max):
    m = Multi(world, (181, 64, 63), SEVEN).sweep()
    cand, n = m.pick(top_k, local_max)
    vols = m.volumes()
    assert n.max() == top_k or local_max
    for j, (mi, _, L) in enumerate(m.jobs):
        c0, n0 = select_single(world.maps[mi], L, m.d_s, m.d_p, int(m.vol[j]), top_k, local_max)
        assert n[j] == n0 and np.array_equal(cand[j, :n0], c0), j
        want = ref_select(vols[j][0], vols[j][1], (L.nx, L.ny, L.nyaw), top_k, local_max)
        assert np.array_equal(cand[j, :n0].astype(np.uint64), want), j
        assert (cand[j, n0:] == -1).all()                            # nothing written behind the list


@pytest.mark.parametrize("top_k", [1, 3, 16])
def test_pick_on_crafted_volumes(world, top_k):
    """Plateaus, fewer eligible poses than top_k, none eligible, ties across threads: every volume a job of one call."""
    import torch
    capi, ctx = world.capi, world.ctx
    vols = crafted_volumes()
    jobs = [(0, 0, capi.PoseLattice(0.0, 0.0, 0.0, 1.0, 1.0, 0.1, d[0], d[1], d[2])) for _, d, _, _ in vols]
    d_s = to_dev(np.concatenate([np.asarray(s, np.float64) for _, _, s, _ in vols]))
    d_p = to_dev(np.concatenate([np.asarray(p, np.uint32) for _, _, _, p in vols]).view(np.int32))
    for local_max in (0, 1):
        d_c = torch.full((len(vols) * top_k,), -1, dtype=torch.int64, device=d_s.device)
        d_n = torch.full((len(vols),), -1, dtype=torch.int32, device=d_s.device)
        sync()
        ctx.lattice_select_multi_dev(jobs, d_s.data_ptr(), d_p.data_ptr(), top_k, local_max, d_c.data_ptr(), d_n.data_ptr())
        sync()
        cand, n = d_c.cpu().numpy().reshape(len(vols), top_k), d_n.cpu().numpy()
        for j, (name, dims, s, p) in enumerate(vols):
            want = ref_select(s, p, dims, top_k, local_max)
            assert n[j] == len(want) and np.array_equal(cand[j, :n[j]].astype(np.uint64), want), (name, local_max)
            assert (cand[j, n[j]:] == -1).all(), name


def test_a_rebuild_queued_behind_the_sweep_waits_for_it(world, c1_world):
    import torch
    capi, ctx = world.capi, world.ctx
    cloud = c1_world[0]
    new = (cloud[:3000] + np.float32([0.45, -0.3])).astype(np.float32)    # another cloud on (nearly) the same grid
    d_old, d_new = to_dev(cloud), to_dev(new)
    sync()
    prm = capi.default_params(resolution=c1_world[2]["resolution"], grid_margin=8)
    own = capi.Map(ctx, params=prm, dev_ptr=d_old.data_ptr(), n=len(cloud))
    L = world.lattice(0, 1025)
    before = score_single(own, world.scans[181], L)
    assert (before[1] > 0).sum() > 100
    m = Multi(world, (181,), [(0, 0, 1025, 0.0), (1, 0, 17, 0.0)])
    other = torch.cuda.Stream()
    sync()
    maps, world.maps = world.maps, [own, world.maps[1]]
    try:
        m.sweep(stream=other.cuda_stream)
        own.rebuild_begin(d_new.data_ptr(), len(new))                 # on the context's stream, directly behind
        own.rebuild_end()
    finally:
        world.maps = maps
    s, p = m.volumes()[0]
    assert s.tobytes() == before[0].tobytes() and p.tobytes() == before[1].tobytes()   # the map from before the rebuild
    after = score_single(own, world.scans[181], L)
    assert after[0].tobytes() != before[0].tobytes()
    own.close()


def test_refusals_queue_and_write_nothing(world):
    import torch
    capi, ctx = world.capi, world.ctx
    lib = capi.lib()
    E = capi.NDT_E_ARG
    m = Multi(world, (181, 64), [(1, 0, 17, 0.0), (0, 1, 16, 0.0)])
    arr, vol = capi.score_jobs(m.jobs)
    mp, n_maps = capi._map_handles(world.maps)
    d_c = torch.full((2 * 16,), -1, dtype=torch.int64, device=m.d_s.device)
    d_n = torch.full((2,), -1, dtype=torch.int32, device=m.d_s.device)
    sync()
    err = lambda: lib.ndt_last_error(ctx.h).decode()

    def sweep(**kw):
        a = dict(ctx=ctx.h, maps=mp, n_maps=n_maps, scans=m.d_pts.data_ptr(), off=m.d_off.data_ptr(), n_scans=2, total=m.total,
                 jobs=arr, n_jobs=2, score=m.d_s.data_ptr(), pairs=m.d_p.data_ptr(), vol=vol.ctypes.data)
        a.update(kw)
        return lib.ndt_score_lattice_multi_dev(a["ctx"], a["maps"], a["n_maps"], a["scans"], a["off"], a["n_scans"], a["total"], a["jobs"],
                                               a["n_jobs"], a["score"], a["pairs"], a["vol"], None)

    def pick(**kw):
        a = dict(ctx=ctx.h, jobs=arr, n_jobs=2, score=m.d_s.data_ptr(), pairs=m.d_p.data_ptr(), vol=vol.ctypes.data, top_k=4,
                 cand=d_c.data_ptr(), n_cand=d_n.data_ptr())
        a.update(kw)
        return lib.ndt_lattice_select_multi_dev(a["ctx"], a["jobs"], a["n_jobs"], a["score"], a["pairs"], a["vol"], a["top_k"], 1,
                                                a["cand"], a["n_cand"], None)

    assert sweep(ctx=None) == E and lib.ndt_last_error(None).decode() == "null context"
    assert pick(ctx=None) == E and lib.ndt_last_error(None).decode() == "null context"
    for name in ("maps", "scans", "off", "jobs", "score", "vol"):
        assert sweep(**{name: None}) == E and "ndt_score_lattice_multi_dev: NULL" in err(), name
    for name in ("jobs", "score", "pairs", "vol", "cand", "n_cand"):
        assert pick(**{name: None}) == E and "ndt_lattice_select_multi_dev: NULL array" in err(), name
    for call in (sweep, pick):
        assert call(n_jobs=0) == E and "need n_jobs >= 1" in err()
        assert call(n_jobs=-2) == E and "need n_jobs >= 1" in err()
    assert sweep(n_scans=0) == E and "n_scans >= 1" in err()
    assert sweep(total=2 ** 31) == E and "total_points" in err()
    assert sweep(n_maps=0) == E and "job 0: map index out of range" in err()

    def raw(jobs):
        """The call's job arguments without the binding's own lattice check: (keep-alive, dict(jobs=, vol=))."""
        arr2 = (capi.ScoreJob * len(jobs))(*[capi.ScoreJob(mi, si, L) for mi, si, L in jobs])
        vol2 = np.zeros(len(jobs) + 1, np.uint64)
        vol2[1:] = np.cumsum([max(L.nx, 0) * max(L.ny, 0) * max(L.nyaw, 0) for _, _, L in jobs])
        return (arr2, vol2), dict(jobs=arr2, vol=vol2.ctypes.data)

    def edited(j, **kw):
        jobs = [[mi, si, capi.PoseLattice.from_buffer_copy(L)] for mi, si, L in m.jobs]
        for f, v in kw.items():
            if f == "map":
                jobs[j][0] = v
            elif f == "scan":
                jobs[j][1] = v
            else:
                setattr(jobs[j][2], f, v)
        return raw(jobs)

    for kw, text, both in ((dict(map=2), "job 1: map index out of range", False), (dict(map=-1), "job 1: map index out of range", False),
                           (dict(scan=2), "job 1: scan index out of range", False), (dict(scan=-1), "job 1: scan index out of range", False),
                           (dict(nx=0), "job 1: bad lattice", True), (dict(step_y=float("nan")), "job 1: bad lattice", True),
                           (dict(nx=65536, ny=32768), "job 1: bad lattice", True)):
        keep, a = edited(1, **kw)
        assert sweep(**a) == E and text in err(), kw
        if both:
            assert pick(**a) == E and text in err(), kw
    keep, a = edited(0, nx=4097, ny=4096, nyaw=1)                    # 2^24 + 4096 poses: the single call takes it, this pick does not
    assert pick(**a) == E and "job 0: a lattice of more than 2^24 poses" in err()
    keep, a = raw([(0, 0, capi.PoseLattice(0.0, 0.0, 0.0, 0.1, 0.1, 0.1, 32768, 32768, 1))] * 2)    # 2^30 poses are legal, twice as many are not
    assert sweep(**a) == E and "more than 2^31 - 1 poses in all (at job 1)" in err()
    for bad, text in ((np.array([0, 16, 33], np.uint64), "job 1: vol_offsets is not the running sum"),
                      (np.array([1, 18, 34], np.uint64), "job 0: vol_offsets is not the running sum"),
                      (np.array([0, 17, 34], np.uint64), "vol_offsets[n_jobs] is not the sum")):
        for call in (sweep, pick):
            assert call(vol=bad.ctypes.data) == E and text in err(), bad
    for top_k in (0, -1, 17):
        assert pick(top_k=top_k) == E and "top_k must be in 1 .. 16" in err()
    holes = (ctypes.c_void_p * 2)(world.maps[0].h, None)
    assert sweep(maps=holes) == E and "map 1 is NULL" in err()
    other = capi.Map(ctx, world.scans[181], capi.default_params(resolution=0.5))
    mixed = (ctypes.c_void_p * 2)(world.maps[0].h, other.h)
    assert sweep(maps=mixed) == E and "map 1 has other match parameters than map 0" in err()
    other.close()
    if torch.cuda.device_count() > 1:
        ctx1 = capi.Context(1)
        assert sweep(ctx=ctx1.h) == E and "built on another device" in lib.ndt_last_error(ctx1.h).decode()
        ctx1.close()
    cloud = to_dev(world.scans[STAGE_LIMIT])
    sync()
    own = capi.Map(ctx, params=capi.default_params(resolution=0.3, grid_margin=8), dev_ptr=cloud.data_ptr(), n=len(cloud))
    own.rebuild_begin(cloud.data_ptr(), len(cloud))
    try:
        assert sweep() == E and "ndt_map_rebuild_begin" in err()
        assert pick() == E and "ndt_map_rebuild_begin" in err()
    finally:
        own.rebuild_end()
    own.close()
    # nothing was queued, nothing written, and the context works
    sync()
    assert (m.d_s.cpu().numpy() == -1.0).all() and (m.d_p.cpu().numpy() == -1).all()
    assert (d_c.cpu().numpy() == -1).all() and (d_n.cpu().numpy() == -1).all()
    m.sweep().assert_single()
