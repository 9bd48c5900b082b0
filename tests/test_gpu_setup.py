"""The match kernel's set-up never changes a record: the optimiser's start, the scan's window and the voxel order of its points
come out the same whether the owner computes them inline, ndt_order_kernel computes them ahead of the launch
(ndt_align_batch_prepare_dev), or the order is found by counting (the repair of order_scan_regs).

Reference everywhere: the same batch launched WITHOUT a prepare call, on a freshly built map with the launch-time parameters.
Records are compared byte for byte."""
import ctypes
import ctypes.util
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def capi():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from ndt_slam_amd import capi
    return capi


@pytest.fixture(scope="module")
def world():
    """A C3-style world at half the extent (0.5 m voxels), 3000-point scans; 40 ragged scans with an empty one and one beyond
    kSortRegs = 10240 points (left to its owner's streaming set-up)."""
    from ndt_slam_amd import synth
    cfg = synth.CONFIGS["C3"]
    m = synth.make_map(200_000, cfg["half"] / 2)
    sf = synth.ScanFactory(m, cfg["half"] / 2, 3000)
    parts, inits = [], []
    for b in range(40):
        sc, _, ini = sf.make(b)
        if b == 7:
            sc = sc[:0]
        elif b == 11:
            sc = np.concatenate([sc] * 4)[:11000]
        else:
            sc = sc[:3000 - 61 * b]
        parts.append(sc); inits.append(ini)
    return dict(m=m, sf=sf, cfg=cfg, parts=parts, inits=np.array(inits))


class Batch:
    """A batch on the device (scans, offsets, inits) and its launch arguments."""

    def __init__(self, parts, inits, shared=False):
        import torch
        from ndt_slam_amd.capi import pack_scans
        dev = torch.device("cuda", 0)
        self.scans, off = pack_scans(parts, offsets_dtype=np.int64)
        self.inits = np.ascontiguousarray(inits, dtype=np.float64)
        self.d_sc = torch.from_numpy(self.scans).to(dev)
        self.d_off = torch.from_numpy(off).to(dev)
        self.d_in = torch.from_numpy(self.inits).to(dev)
        self.B, self.shared = len(self.inits), shared
        torch.cuda.synchronize()

    def args(self):
        return (self.d_sc.data_ptr(), self.d_off.data_ptr(), self.B, len(self.scans), self.d_in.data_ptr())

    def out(self):
        import torch
        return torch.zeros(self.B * RESULT_BYTES(), dtype=torch.uint8, device=self.d_sc.device)

    def prepare(self, gm, stream=None, ctx=None):
        gm.prepare_batch_dev(*self.args(), shared_scan=self.shared, stream=stream, ctx=ctx)

    def launch(self, gm, out, stream=None, ctx=None):
        gm.align_batch_dev(*self.args(), out.data_ptr(), shared_scan=self.shared, stream=stream, ctx=ctx)


def RESULT_BYTES():
    from ndt_slam_amd import capi
    return capi.RESULT_BYTES


def rec(t):
    import torch
    from ndt_slam_amd import capi
    torch.cuda.synchronize()
    return np.frombuffer(t.cpu().numpy().tobytes(), dtype=capi.RESULT_DTYPE).copy()


def plain(capi, cloud, prm, batch):
    """The reference: the batch, no prepare call, on a map freshly built from `cloud` with `prm`, in a context of its own."""
    ctx = capi.Context(0)
    gm = capi.Map(ctx, cloud, prm)
    o = batch.out()
    batch.launch(gm, o)
    r = rec(o)
    gm.close(); ctx.close()
    return r


def host_libm():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    for f in (libm.cosf, libm.sinf):
        f.restype = ctypes.c_float; f.argtypes = [ctypes.c_float]
    return libm


def yaws_where_libm_differs(ctx, yaws, width=0.05, tries=20000):
    """Per yaw, a float32 within +-width of it where cosf or sinf of the platform differ from the correctly rounded values:
    all candidates at once through ndt_selftest_libm_f32 (the device's restatement of glibc), the picks then on the host."""
    rng = np.random.default_rng(11)
    cand = (np.asarray(yaws)[:, None] + rng.uniform(-width, width, size=(len(yaws), tries))).astype(np.float32)
    c, s, _ = ctx.selftest_libm_f32(cand.ravel())
    flat = cand.ravel().astype(np.float64)
    differs = ((c != np.cos(flat).astype(np.float32)) | (s != np.sin(flat).astype(np.float32))).reshape(cand.shape)
    assert np.all(differs.any(axis=1))
    out = cand[np.arange(len(yaws)), np.argmax(differs, axis=1)]
    libm = host_libm()
    for v in out:
        plat = (np.float32(libm.cosf(float(v))), np.float32(libm.sinf(float(v))))
        assert plat != (np.float32(math.cos(float(v))), np.float32(math.sin(float(v)))), v
    return out.astype(np.float64)


def sse_sensitive(ctx, parts, inits, inv_leaf, per_scan=8, tries=1_500_000):
    """The scans with up to per_scan points replaced by points whose voxel at the first pose differs between the two float32
    transforms (transform_sse 1: a + (b + tx), 0: (a + b) + tx; tf_apply_t): points within an ulp of a voxel boundary.  The
    first pose's cos / sin are the device's (libm_f32 = 1); numpy's float32 arithmetic rounds as the device does."""
    rng = np.random.default_rng(12)
    c_all, s_all, _ = ctx.selftest_libm_f32(np.asarray(inits)[:, 2].astype(np.float32))
    L = np.float32(inv_leaf)
    out, moved = [], 0
    for sc, ini, c, s in zip(parts, inits, c_all, s_all):
        sc = sc.copy()
        tx, ty, ms = np.float32(ini[0]), np.float32(ini[1]), np.float32(-s)
        p = sc[rng.integers(0, len(sc), tries)] + rng.uniform(-0.25, 0.25, size=(tries, 2)).astype(np.float32)
        a, b, cc, d = c * p[:, 0], ms * p[:, 1], s * p[:, 0], c * p[:, 1]
        differs = (np.floor(((a + b) + tx) * L) != np.floor((a + (b + tx)) * L)) | \
                  (np.floor(((cc + d) + ty) * L) != np.floor((cc + (d + ty)) * L))
        pick = p[differs][:per_scan]
        sc[:len(pick)] = pick
        moved += len(pick)
        out.append(sc)
    return out, moved


def check_param_change(capi, w, batch, prm_a, prm_b):
    """Prepare under parameters A, rebuild the same cloud (same grid) under B, launch: the records of a fresh map under B.
    Also: the inputs separate A from B (plain records differ), else the case would test nothing."""
    ref_a, ref_b = plain(capi, w["m"], prm_a, batch), plain(capi, w["m"], prm_b, batch)
    assert ref_a.tobytes() != ref_b.tobytes(), "the workload does not separate the two parameter sets"
    ctx = capi.Context(0)
    gm = capi.Map(ctx, w["m"], prm_a)
    info_a = gm.info()
    o = batch.out()
    batch.prepare(gm)
    gm.rebuild(xy=w["m"], params=prm_b)
    info_b = gm.info()
    assert (info_a.min_bx, info_a.min_by, info_a.div_x, info_a.div_y) == (info_b.min_bx, info_b.min_by, info_b.div_x, info_b.div_y)
    batch.launch(gm, o)
    got = rec(o)
    gm.close(); ctx.close()
    assert got.tobytes() == ref_b.tobytes(), "a batch prepared under other parameters changed the records"
    return ref_b


def test_prepared_batch_after_libm_f32_changes(capi, world):
    """libm_f32 1 -> 0 between prepare and launch: the start matrix is glibc's cosf / sinf under 1 and the correctly rounded
    values under 0.  The guesses' yaws are moved to floats where the two differ on this host (and on the device:
    ndt_selftest_libm_f32), so the start of every scan depends on the switch."""
    w = world
    libm = host_libm()
    inits = w["inits"].copy()
    ctx = capi.Context(0)
    inits[:, 2] = yaws_where_libm_differs(ctx, inits[:, 2])
    y = inits[:, 2].astype(np.float32)
    c, s, _ = ctx.selftest_libm_f32(y)
    ctx.close()
    host = np.array([libm.cosf(float(v)) for v in y], np.float32), np.array([libm.sinf(float(v)) for v in y], np.float32)
    cr = np.array([math.cos(float(v)) for v in y], np.float32), np.array([math.sin(float(v)) for v in y], np.float32)
    assert c.tobytes() == host[0].tobytes() and s.tobytes() == host[1].tobytes()
    assert np.all((c != cr[0]) | (s != cr[1]))
    res = w["cfg"]["resolution"]
    check_param_change(capi, w, Batch(w["parts"], inits), capi.default_params(resolution=res, libm_f32=1),
                       capi.default_params(resolution=res, libm_f32=0))


def test_prepared_batch_after_snap_thresh_changes(capi, world):
    """snap_thresh 1e-4 -> 1e-2: guesses with 1e-4 <= |yaw| < 1e-2 start with exact angle terms under A and with (1, 0) under B."""
    w = world
    inits = w["inits"].copy()
    inits[:, 2] = np.where(np.arange(len(inits)) % 2 == 0, 1.0, -1.0) * np.linspace(2e-4, 9e-3, len(inits))
    res = w["cfg"]["resolution"]
    check_param_change(capi, w, Batch(w["parts"], inits), capi.default_params(resolution=res, snap_thresh=1e-4),
                       capi.default_params(resolution=res, snap_thresh=1e-2))


def test_prepared_batch_after_transform_sse_flips(capi, world):
    """transform_sse 1 -> 0: picks the other ndt_order_kernel instance, i.e. the cells the points are ordered by at the first
    pose.  A ragged batch of C2-sized scans (up to 10k points, 0.5 m voxels) in which a few points per scan lie within an ulp
    of a voxel boundary, so that the two transforms put them in different voxels at the first pose."""
    from ndt_slam_amd import synth
    cfg = synth.CONFIGS["C2"]
    w = dict(world)
    m = synth.make_map(400_000, cfg["half"])
    sf = synth.ScanFactory(m, cfg["half"], cfg["n_scan"])
    parts, inits = [], []
    for b in range(24):
        sc, _, ini = sf.make(b)
        parts.append(sc[:10240 - 211 * b]); inits.append(ini)
    ctx = capi.Context(0)
    parts, moved = sse_sensitive(ctx, parts, inits, 1.0 / cfg["resolution"])
    ctx.close()
    assert moved >= 8
    w["m"] = m
    check_param_change(capi, w, Batch(parts, np.array(inits)), capi.default_params(resolution=cfg["resolution"], transform_sse=1),
                       capi.default_params(resolution=cfg["resolution"], transform_sse=0))


def test_prepared_batch_against_a_new_map_at_the_old_address(capi, world):
    """The map destroyed after the prepare call and another one built from the same cloud (same grid) with other parameters,
    at the old address where the allocator gives it back: the launch with the prepared batch's pointers is not served by it."""
    w = world
    res = w["cfg"]["resolution"]
    inits = w["inits"].copy()
    ctx = capi.Context(0)
    inits[:, 2] = yaws_where_libm_differs(ctx, inits[:, 2])
    ctx.close()
    batch = Batch(w["parts"], inits)
    prm_a = capi.default_params(resolution=res, libm_f32=1, snap_thresh=1e-4)
    prm_b = capi.default_params(resolution=res, libm_f32=0, snap_thresh=2e-4, transform_sse=0)
    ref_b = plain(capi, w["m"], prm_b, batch)
    assert plain(capi, w["m"], prm_a, batch).tobytes() != ref_b.tobytes()
    ctx = capi.Context(0)
    gm = capi.Map(ctx, w["m"], prm_a)
    old = gm.h.value
    batch.prepare(gm)
    gm.close()
    keep = []
    for _ in range(4):                         # (the allocator usually hands the freed block back at once)
        nm = capi.Map(ctx, w["m"], prm_b)
        keep.append(nm)
        if nm.h.value == old:
            break
    o = batch.out()
    batch.launch(keep[-1], o)
    assert rec(o).tobytes() == ref_b.tobytes()
    for nm in keep:
        nm.close()
    ctx.close()


def test_prepared_batch_survives_a_rebuild_with_the_same_grid(capi, world):
    """The designed use: prepare, then rebuild the map from ANOTHER cloud with the same bounding box and parameters (bench.py
    prepares ahead of the step's rebuild).  The prepared set is used and the records are those of a fresh map of that cloud."""
    w = world
    prm = capi.default_params(resolution=w["cfg"]["resolution"])
    m = w["m"]
    m2 = m.copy()
    inner = np.ones(len(m), bool)
    inner[[int(np.argmin(m[:, 0])), int(np.argmax(m[:, 0])), int(np.argmin(m[:, 1])), int(np.argmax(m[:, 1]))]] = False
    rng = np.random.default_rng(3)
    m2[inner] += rng.normal(0.0, 0.01, size=(int(inner.sum()), 2)).astype(np.float32)
    m2 = np.clip(m2, m.min(axis=0), m.max(axis=0))
    batch = Batch(w["parts"], w["inits"])
    want = plain(capi, m2, prm, batch)
    assert want.tobytes() != plain(capi, m, prm, batch).tobytes()
    ctx = capi.Context(0)
    gm = capi.Map(ctx, m, prm)
    i0 = gm.info()
    assert ctx.prepare_timing() == 0.0
    batch.prepare(gm)
    gm.rebuild(xy=m2)
    i1 = gm.info()
    assert (i0.min_bx, i0.min_by, i0.div_x, i0.div_y) == (i1.min_bx, i1.min_by, i1.div_x, i1.div_y)
    o = batch.out()
    batch.launch(gm, o)
    assert rec(o).tobytes() == want.tobytes()
    assert ctx.prepare_timing() > 0.0                     # it was used
    gm.close(); ctx.close()


def test_prepared_shared_scan(capi, world):
    """64 seeds of one scan (shared_scan), prepared ahead and not."""
    w = world
    prm = capi.default_params(resolution=w["cfg"]["resolution"])
    base = w["inits"][3]
    seeds = base[None, :] + np.stack([np.linspace(-0.3, 0.3, 64), np.linspace(0.25, -0.25, 64),
                                      np.linspace(-0.06, 0.06, 64)], axis=1)
    batch = Batch([w["parts"][3]], seeds, shared=True)
    want = plain(capi, w["m"], prm, batch)
    assert np.all(want["status"] == 0) and len(set(want["pose"][:, 2].tolist())) > 1
    ctx = capi.Context(0)
    gm = capi.Map(ctx, w["m"], prm)
    o = batch.out()
    batch.prepare(gm)
    batch.launch(gm, o)
    assert rec(o).tobytes() == want.tobytes()
    assert ctx.prepare_timing() > 0.0
    gm.close(); ctx.close()


@pytest.mark.parametrize("opt", [("workgroups", 8), ("helpers", 0)])
def test_prepared_batch_under_launch_options(capi, world, opt):
    """OPT_WORKGROUPS = 8 with B = 40 (the order kernel's grid-stride loop takes five scans per workgroup) and OPT_MAX_HELPERS = 0."""
    w = world
    prm = capi.default_params(resolution=w["cfg"]["resolution"])
    batch = Batch(w["parts"], w["inits"])
    want = plain(capi, w["m"], prm, batch)
    ctx = capi.Context(0)
    ctx.set_option(capi.OPT_WORKGROUPS if opt[0] == "workgroups" else capi.OPT_MAX_HELPERS, opt[1])
    gm = capi.Map(ctx, w["m"], prm)
    o = batch.out()
    batch.launch(gm, o)
    assert rec(o).tobytes() == want.tobytes()             # (the option alone changes no record)
    batch.prepare(gm)
    batch.launch(gm, o)
    assert rec(o).tobytes() == want.tobytes()
    assert ctx.prepare_timing() > 0.0
    gm.close(); ctx.close()


def test_three_prepares_on_three_streams(capi, world):
    """Three batches prepared on three streams before any launch: the third prepare call reuses the first one's set (two per
    context) and must wait for that set's own order kernel.  Batches 3 and 2 are served and byte-equal; batch 1 is no longer
    prepared and is launched as without a prepare call."""
    import torch
    w = world
    prm = capi.default_params(resolution=w["cfg"]["resolution"])
    dev = torch.device("cuda", 0)
    batches = []
    for k in range(3):
        inits = w["inits"].copy()
        inits[:, 0] += 0.03 * k; inits[:, 2] -= 0.004 * k
        batches.append(Batch(w["parts"][k:] + w["parts"][:k], np.roll(inits, -k, axis=0)))
    want = [plain(capi, w["m"], prm, b) for b in batches]
    assert len({r.tobytes() for r in want}) == 3
    ctx = capi.Context(0)
    gm = capi.Map(ctx, w["m"], prm)
    streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
    for b, st in zip(batches, streams):
        b.prepare(gm, stream=st.cuda_stream)
    outs = [b.out() for b in batches]
    batches[2].launch(gm, outs[2])
    batches[1].launch(gm, outs[1])
    batches[0].launch(gm, outs[0])
    for k in (2, 1, 0):
        assert rec(outs[k]).tobytes() == want[k].tobytes(), k
    gm.close(); ctx.close()


def test_prepared_pipeline_with_deferred_fitness(capi, world):
    """OPT_DEFER_FITNESS on, a stream of batches as a caller would run it: step i prepares batch i + 1, then launches batch i,
    over two alternating sets of input buffers.  Six steps; every record equals the plain loop's."""
    import torch
    w = world
    prm = capi.default_params(resolution=w["cfg"]["resolution"])
    dev = torch.device("cuda", 0)
    steps = 6
    data = []
    for i in range(steps + 1):
        inits = w["inits"].copy()
        inits[:, 1] += 0.02 * i; inits[:, 2] += 0.003 * i
        data.append((w["parts"][i:] + w["parts"][:i], inits))
    want = [plain(capi, w["m"], prm, Batch(*data[i])) for i in range(steps)]
    ctx = capi.Context(0)
    st = torch.cuda.Stream(device=dev)
    ctx.set_stream(st.cuda_stream)
    ctx.set_option(capi.OPT_DEFER_FITNESS, 1)
    gm = capi.Map(ctx, w["m"], prm)
    bufs = [Batch(*data[0]), Batch(*data[1])]

    def load(i):                                            # batch i into its buffer set (nothing in flight reads it)
        b = bufs[i % 2]
        src = Batch(*data[i])
        assert src.d_sc.numel() == b.d_sc.numel() and src.B == b.B
        b.d_sc.copy_(src.d_sc); b.d_off.copy_(src.d_off); b.d_in.copy_(src.d_in)
        torch.cuda.synchronize()
    outs = [bufs[0].out(), bufs[0].out()]
    bufs[0].prepare(gm, stream=st.cuda_stream)
    got = []
    for i in range(steps):
        if i >= 1:
            load(i + 1)                                     # (its buffer set was batch i - 1's, whose launch has ended)
        bufs[(i + 1) % 2].prepare(gm, stream=st.cuda_stream)
        bufs[i % 2].launch(gm, outs[i % 2], stream=st.cuda_stream)
        ctx.wait_launch(0, st.cuda_stream)
        st.synchronize()
        got.append(rec(outs[i % 2]))
    assert ctx.prepare_timing() > 0.0
    for i in range(steps):
        assert got[i].tobytes() == want[i].tobytes(), i
    gm.close(); ctx.close()


def test_forced_order_repair_gives_the_same_records(capi, tmp_path):
    """The order repair of order_scan_regs (the places found by counting when the scatter's atomics did not come back in lane
    order) has to give the places the scatter gives.  The build with NDT_FORCE_ORDER_REPAIR takes the repair on every scan of
    the register-resident set-up, inline and in ndt_order_kernel: a fresh child process runs fixed workloads
    (tests/repair_workloads.py) on it, this process on the default library; the records must be byte-equal."""
    variant = os.path.join(ROOT, "ndt_slam_amd", "libndt_mi355x_force_repair.so")
    assert os.path.exists(variant), "%s is missing: __graft_entry__.build() builds it" % variant
    out = tmp_path / "repair.npz"
    env = dict(os.environ, NDT_LIB_PATH=variant)
    p = subprocess.run([sys.executable, os.path.join(HERE, "repair_workloads.py"), str(out)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, "child with the forced repair failed (%d):\n%s" % (p.returncode, p.stderr[-4000:])
    sys.path.insert(0, HERE)
    try:
        import repair_workloads as W
    finally:
        sys.path.remove(HERE)
    ctx = capi.Context(0)
    m, m2, sf, cfg = W.world()
    mine = W.records(capi, ctx, m, m2, sf, cfg)
    ctx.close()
    theirs = np.load(out)
    assert str(theirs["lib_path"]) == os.path.abspath(variant)
    assert os.path.abspath(capi.LIB_PATH) != os.path.abspath(variant)
    assert bool(mine["prepared_used"][0]) and bool(theirs["prepared_used"][0])
    assert np.all(mine["c3_64"]["status"] == 0) and np.all(mine["multi"]["status"] == 0)
    for name, r in mine.items():
        if name == "prepared_used":
            continue
        assert theirs[name].tobytes() == r.tobytes(), "records of workload %r differ with the forced repair" % name
