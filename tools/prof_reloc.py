"""Relocalisation (ndt_score_lattice_dev, ndt_lattice_select_dev, ndt_relocalize) against the parent's only way to rank P
poses on the device, ndt_align_batch(shared_scan) over the same P poses.

Workloads
  C5   configs[4]'s scene of tools/prof_c5.py (5M-point map, one 10k-point scan); lattice 65 x 65 translations at 0.5 m
       centred 5 m off the truth x 72 yaws at 5 degrees = 304 200 poses.
  C1   configs[0]'s world (tests/conftest.py::c1_world) with the tests' lattice LAT (81 x 81 x 36 = 236 196 poses).
Figures (each the median of --reps repeats after one warm-up, alternating sweep and alignment; device events):
  sweep_ms / sweep_us_per_pose / sweep_point_evals_per_s       the score kernel alone (the events on its dispatch)
  align_ms / align_us_per_seed / align_seeds_per_s             ndt_align_batch(shared_scan) over --align-seeds lattice poses
                                                               (the events around the launch, ndt_last_timing)
  ratio_align_over_sweep                                       per pose; the sweep must be the cheaper one
  eval_at_ms_per_call                                          host clock around ndt_eval_at (one pose, host pointers)
  reloc_ms {total, sweep, pick, refine}                        host clock around ndt_relocalize and around its three parts
                                                               issued one by one with a device synchronise behind each
  success                                                      scans 0 .. 15: winner within 0.05 m of the truth (a count)
--only sweep: the sweep alone, --reps times (for a counters-only rocprofv3 --pmc run of its own: bytes fetched per pose
against the algorithmic 8 B x 9 + 40 B x pairs per point).
Usage: python tools/prof_reloc.py [--world C5,C1] [--reps 5] [--align-seeds 4096] [--scans 16] [--only sweep] [--json PATH]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ndt_slam_amd import capi, synth      # noqa: E402


def world(name):
    cfg = synth.CONFIGS[name]
    m = synth.make_map(cfg["n_map"], cfg["half"])
    return m, synth.ScanFactory(m, cfg["half"], cfg["n_scan"]), cfg


def lattice_for(name, truth, cfg):
    if name == "C1":
        return capi.PoseLattice(-24.0, -24.0, -math.pi, 0.6, 0.6, 2.0 * math.pi / 36, 81, 81, 36)
    cx, cy = truth[0] + 5.0 / math.sqrt(2.0), truth[1] - 5.0 / math.sqrt(2.0)          # centred 5 m off the truth
    return capi.PoseLattice(cx - 32 * 0.5, cy - 32 * 0.5, -math.pi, 0.5, 0.5, math.radians(5.0), 65, 65, 72)


def med(x):
    return float(np.median(np.asarray(x, dtype=np.float64)))


def run(name, args):
    import torch
    dev = torch.device("cuda", 0)
    t0 = time.time()
    m, sf, cfg = world(name)
    scan, truth, _ = sf.make(0)
    ctx = capi.Context(0)
    gm = capi.Map(ctx, m, capi.default_params(resolution=cfg["resolution"]))
    L = lattice_for(name, truth, cfg)
    P, n = L.size, len(scan)
    print("[%s] inputs + map in %.1f s: %d cells, scan %d points, lattice %d poses" % (name, time.time() - t0, gm.info().n_cells, n, P))
    d_sc = torch.from_numpy(scan).to(dev)
    d_s = torch.zeros(P, dtype=torch.float64, device=dev)
    d_p = torch.zeros(P, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def sweep():
        gm.score_lattice(d_sc.data_ptr(), n, L, d_s.data_ptr(), d_p.data_ptr())
        torch.cuda.synchronize()
        return ctx.kernel_timing(0)[0]

    if args.only == "sweep":
        ms = [sweep() for _ in range(args.reps + 1)][1:]
        pairs = int(d_p.cpu().numpy().view(np.uint32).astype(np.int64).sum())
        return dict(world=name, poses=P, scan_points=n, sweep_ms=med(ms), pairs_total=pairs,
                    algorithmic_bytes_per_pose=(72.0 * n * P + 40.0 * pairs) / P)

    rng = np.random.default_rng(1)
    seeds = L.poses(rng.choice(P, min(args.align_seeds, P), replace=False))
    off = np.array([0, n], np.uint64)

    def align():
        gm.align_batch(scan, off, seeds, shared_scan=True)
        return ctx.last_timing()[1]

    sweep(); align()                                                       # warm-up of both
    sw, al = [], []
    for _ in range(args.reps):
        sw.append(sweep()); al.append(align())
    pairs = int(d_p.cpu().numpy().view(np.uint32).astype(np.int64).sum())
    out = dict(world=name, poses=P, scan_points=n, cells=int(gm.info().n_cells), sweep_ms=med(sw), sweep_ms_all=sw,
               sweep_us_per_pose=med(sw) * 1e3 / P, sweep_point_evals_per_s=P * n / (med(sw) * 1e-3),
               sweep_pairs_per_point=pairs / (float(P) * n), align_seeds=len(seeds), align_ms=med(al), align_ms_all=al,
               align_us_per_seed=med(al) * 1e3 / len(seeds), align_seeds_per_s=len(seeds) / (med(al) * 1e-3))
    out["ratio_align_over_sweep"] = out["align_us_per_seed"] / out["sweep_us_per_pose"]
    t = []
    for _ in range(20):
        a = time.perf_counter(); gm.eval_at(scan, truth); t.append((time.perf_counter() - a) * 1e3)
    out["eval_at_ms_per_call"] = med(t[2:])
    # the whole call, and its three parts one by one
    d_c = torch.zeros(args.top_k, dtype=torch.int64, device=dev); d_n = torch.zeros(1, dtype=torch.int32, device=dev)
    tot, part = [], []
    for _ in range(args.reps + 1):
        a = time.perf_counter(); r = gm.relocalize(scan, L, top_k=args.top_k); tot.append((time.perf_counter() - a) * 1e3)
        a = time.perf_counter()
        gm.score_lattice(d_sc.data_ptr(), n, L, d_s.data_ptr(), d_p.data_ptr()); torch.cuda.synchronize()
        b = time.perf_counter()
        gm.lattice_select(L, d_s.data_ptr(), d_p.data_ptr(), args.top_k, 1, d_c.data_ptr(), d_n.data_ptr()); torch.cuda.synchronize()
        c = time.perf_counter()
        k = int(d_n.cpu()[0])
        if k:
            gm.align_batch(scan, off, L.poses(d_c.cpu().numpy()[:k]), shared_scan=True)
        d = time.perf_counter()
        part.append(((b - a) * 1e3, (c - b) * 1e3, (d - c) * 1e3))
    part = np.array(part[1:])
    out["reloc_ms"] = dict(total=med(tot[1:]), sweep=med(part[:, 0]), pick=med(part[:, 1]), refine=med(part[:, 2]))
    ok, rows = 0, []
    for k in range(args.scans):
        sc, tr, _ = sf.make(k)
        r = gm.relocalize(sc, lattice_for(name, tr, cfg), top_k=args.top_k)
        e = float("inf")
        if r["best"] >= 0:
            w = r["records"][r["best"]]
            e = math.hypot(w["pose"][0] - tr[0], w["pose"][1] - tr[1])
        ok += e <= 0.05
        rows.append(dict(scan=k, best=int(r["best"]), err_m=e))
    out["success"] = dict(scans=args.scans, within_0_05_m=int(ok), rows=rows)
    gm.close(); ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", default="C5,C1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--align-seeds", type=int, default=4096)
    ap.add_argument("--scans", type=int, default=16)
    ap.add_argument("--top-k", type=int, default=16)
    ap.add_argument("--only", default="")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    res = [run(w, args) for w in args.world.split(",")]
    for r in res:
        print(json.dumps({k: v for k, v in r.items() if not k.endswith("_all") and k != "success"}))
        if "success" in r:
            print("success %d / %d" % (r["success"]["within_0_05_m"], r["success"]["scans"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(tool="tools/prof_reloc.py", results=res), f, indent=1)


if __name__ == "__main__":
    main()
