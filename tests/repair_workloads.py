"""Fixed match workloads for tests/test_gpu_setup.py::test_forced_order_repair_gives_the_same_records (tests only).

Both sides of that test import this module: the test's own process computes the records with the default library, and a
fresh child process runs it as a script with NDT_LIB_PATH pointing at the build with NDT_FORCE_ORDER_REPAIR (every scan of the
register-resident set-up puts its points in place by counting), writing the same records to an .npz:

    python tests/repair_workloads.py OUT.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# scan lengths of the ragged batch: both sides of every power of two the set-up's loops split on, up to kSortRegs = 10240
# (the largest scan the register-resident set-up takes), and an empty scan
RAGGED_LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 10239, 10240, 0)


def world():
    """The C3 world (1M-point map, 10k-point scans, 0.5 m voxels) and a second map of another cloud."""
    from ndt_slam_amd import synth
    cfg = synth.CONFIGS["C3"]
    m = synth.make_map(cfg["n_map"], cfg["half"])
    sf = synth.ScanFactory(m, cfg["half"], cfg["n_scan"])
    m2 = synth.make_map(cfg["n_map"] // 2, cfg["half"], seed=synth.MAP_SEED + 1)
    return m, m2, sf, cfg


def batches(sf):
    """name -> (scans, offsets, inits, shared_scan).  Inputs only: no device needed."""
    from ndt_slam_amd.capi import pack_scans
    scans, off, _, inits = sf.batch(0, 64)
    out = {"c3_64": (scans, off, inits, False)}
    # ragged: lengths at the set-up's edges, an empty scan, and a scan with NaN points among finite ones
    pool = [scans[int(off[b]):int(off[b + 1])] for b in range(64)]
    parts = []
    for k, n in enumerate(RAGGED_LENGTHS):
        src = np.concatenate([pool[k], pool[k + 20]])
        parts.append(src[:n])
    nan_scan = pool[40].copy()
    nan_scan[::97] = np.nan
    nan_scan[5, 1] = np.nan
    parts.append(nan_scan)
    rs, ro = pack_scans(parts)
    out["ragged"] = (rs, ro, inits[:len(parts)], False)
    # dense clusters: ~10k points packed into a handful of voxels (+-4 cm around 3..6 centres, at 0.5 m voxels), so that one
    # wave instruction of the scatter issues hundreds of atomics on the same cell counter
    rng = np.random.Generator(np.random.Philox(77))
    parts = []
    for b in range(6):
        base = pool[48 + b]
        k = 3 + b % 4
        centres = base[rng.choice(len(base), size=k, replace=False)]
        n = 10240 - 37 * b
        pts = centres[rng.integers(0, k, size=n)] + rng.uniform(-0.04, 0.04, size=(n, 2))
        parts.append(pts.astype(np.float32))
    ds, do = pack_scans(parts)
    out["dense"] = (ds, do, inits[48:54], False)
    # 24 scans, fewer than the launch's workgroups: the owners open their scans for joining from inside the set-up (open_ctl)
    s24, o24, _, i24 = sf.batch(100, 24)
    out["few_24"] = (s24, o24, i24, False)
    # 64 seeds of one scan
    one = pool[3]
    seeds = inits[3][None, :] + np.stack([np.linspace(-0.3, 0.3, 64), np.linspace(0.2, -0.2, 64),
                                          np.linspace(-0.05, 0.05, 64)], axis=1)
    out["shared_64"] = (one, np.array([0, len(one)], np.uint64), seeds, True)
    return out


def records(capi, ctx, m, m2, sf, cfg):
    """name -> ndt_result records (bytes) of every workload, computed with the library capi has loaded."""
    import torch
    prm = capi.default_params(resolution=cfg["resolution"])
    gm = capi.Map(ctx, m, prm)
    gm2 = capi.Map(ctx, m2, prm)
    out = {}
    for name, (scans, off, inits, shared) in batches(sf).items():
        out[name] = gm.align_batch(scans, off, inits, shared_scan=shared)
    # a prepared batch: the set-up in ndt_order_kernel ahead of the launch
    scans, off, inits, _ = batches(sf)["c3_64"]
    dev = torch.device("cuda", 0)
    d_sc = torch.from_numpy(scans).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_in = torch.from_numpy(np.ascontiguousarray(inits)).to(dev)
    res = torch.zeros(len(inits) * capi.RESULT_BYTES, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    args = (d_sc.data_ptr(), d_off.data_ptr(), len(inits), len(scans), d_in.data_ptr())
    gm.prepare_batch_dev(*args)
    gm.align_batch_dev(*args, res.data_ptr())
    torch.cuda.synchronize()
    out["prepared"] = np.frombuffer(res.cpu().numpy().tobytes(), dtype=capi.RESULT_DTYPE).copy()
    out["prepared_used"] = np.array([ctx.prepare_timing() > 0.0])
    # one launch over two maps, the matches alternating between them
    map_of = np.arange(len(inits), dtype=np.int32) % 2
    out["multi"] = capi.align_batch_multi(ctx, [gm, gm2], scans, off, inits, map_of=map_of)
    gm2.close()
    gm.close()
    return out


def main(path):
    import torch                                    # (the HIP runtime through torch first, as in the test process)
    assert torch.cuda.is_available()
    from ndt_slam_amd import capi
    ctx = capi.Context(0)
    m, m2, sf, cfg = world()
    out = records(capi, ctx, m, m2, sf, cfg)
    out = {k: np.frombuffer(v.tobytes(), np.uint8) if v.dtype == capi.RESULT_DTYPE else v for k, v in out.items()}
    np.savez(path, lib_path=np.array(os.path.abspath(capi.LIB_PATH)), **out)
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1])
