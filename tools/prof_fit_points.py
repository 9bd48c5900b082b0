"""ndt_fit_points_batch_dev beside the fitness kernels of the launch whose records it reads.

Workload: the benchmark's shape (configs[2]): 256 scans x 10k points against the 1M-point map, one ndt_align_batch_dev launch
from the scans' initial guesses; its device records are the call's `tf` (tf = &records[0].T00, stride sizeof(ndt_result)).
Figures (device events on the kernels' own dispatches, ndt_kernel_timing; median of --reps after one warm-up):
  launch_match_ms / launch_fitness_ms     the launch's match kernel and its fitness kernels (the ordered copy, chunk sums only)
  fit_points_ms {d2_and_stats, stats_only, d2_only}    fit_points_kernel, and behind it fit_points_close_kernel (close_ms)
  ratio_over_launch_fitness               (search + close, d2 and stats) / launch_fitness_ms: what reading the scan in input
                                          order instead of the launch's voxel-ordered copy, and writing d2, cost
  max_d2                                  the squared range of the stats (m^2); the times do not depend on it
Usage: python tools/prof_fit_points.py [--scans 256] [--reps 5] [--max-d2 1.0] [--json PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ndt_slam_amd import capi, synth      # noqa: E402


def med(x):
    return float(np.median(np.asarray(x, dtype=np.float64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", default="C3")
    ap.add_argument("--scans", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-d2", type=float, default=1.0)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    t0 = time.time()
    cfg = synth.CONFIGS[args.world]
    m = synth.make_map(cfg["n_map"], cfg["half"])
    sf = synth.ScanFactory(m, cfg["half"], cfg["n_scan"])
    scans, offs, _, inits = sf.batch(0, args.scans)
    B, total = args.scans, len(scans)
    ctx = capi.Context(0)
    gm = capi.Map(ctx, m, capi.default_params(resolution=cfg["resolution"]))
    print("inputs + map in %.1f s: %d scans, %d points, map %d points" % (time.time() - t0, B, total, len(m)))
    d_sc = torch.from_numpy(scans).to(dev)
    d_off = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    d_in = torch.from_numpy(inits).to(dev)
    d_rec = torch.zeros(B * capi.RESULT_BYTES, dtype=torch.uint8, device=dev)
    d_d2 = torch.zeros(total, dtype=torch.float32, device=dev)
    d_st = torch.zeros(B * 32, dtype=torch.uint8, device=dev)
    tf_ptr = d_rec.data_ptr() + capi.RESULT_DTYPE.fields["T00"][1]
    torch.cuda.synchronize()

    def launch():
        gm.align_batch_dev(d_sc.data_ptr(), d_off.data_ptr(), B, total, d_in.data_ptr(), d_rec.data_ptr())
        torch.cuda.synchronize()
        return ctx.kernel_timing(0)

    def fit(want_d2, want_stats):
        gm.fit_points_dev(d_sc.data_ptr(), d_off.data_ptr(), B, total, tf_ptr, capi.RESULT_BYTES, args.max_d2,
                          d_d2.data_ptr() if want_d2 else None, d_st.data_ptr() if want_stats else None)
        torch.cuda.synchronize()
        return ctx.kernel_timing(0)                        # (search kernel, what follows it up to the call's end)

    launch()
    la = [launch() for _ in range(args.reps)]
    out = dict(tool="tools/prof_fit_points.py", world=args.world, scans=B, points=total, map_points=len(m), max_d2=args.max_d2,
               launch_match_ms=med([a for a, _ in la]), launch_fitness_ms=med([f for _, f in la]), fit_points_ms={}, close_ms={})
    for name, wd, ws in (("d2_and_stats", True, True), ("stats_only", False, True), ("d2_only", True, False)):
        fit(wd, ws)
        r = [fit(wd, ws) for _ in range(args.reps)]
        out["fit_points_ms"][name] = med([a for a, _ in r])
        out["close_ms"][name] = med([f for _, f in r])
        out[name + "_ms_all"] = [a + f for a, f in r]
    out["ratio_over_launch_fitness"] = (out["fit_points_ms"]["d2_and_stats"] + out["close_ms"]["d2_and_stats"]) / out["launch_fitness_ms"]
    rec = d_rec.cpu().numpy().view(capi.RESULT_DTYPE)
    fit(True, True)
    st = d_st.cpu().numpy().view(capi.FIT_STATS_DTYPE)
    rel = np.abs(st["fitness_all"] - rec["fitness"]) / rec["fitness"]
    out["fitness_all_vs_record_max_rel"] = float(rel.max())
    out["share_in_range"] = float(st["n_in"].sum()) / float(st["n_dist"].sum())
    print(json.dumps({k: v for k, v in out.items() if not k.endswith("_all")}))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    gm.close(); ctx.close()


if __name__ == "__main__":
    main()
