"""Times Submap::makeMap on the device (ndt_make_map_dev) against the oracle on the host, or -- `rn` -- the neighbour
removal on its own (ndt_remove_neighbors_dev) and, alone, the one table upload it queues.
Usage: python tools/prof_localmap.py [n_scans] [points_per_scan]
       python tools/prof_localmap.py rn [n_base] [n_list]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ndt_slam_amd import capi, synth               # noqa: E402
from oracle import ndt_oracle as O                 # noqa: E402  (checker only)


def timed(stream, call, reps=8):
    """HIP events around `call` on `stream`: milliseconds of a warm-up and of `reps` runs"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(reps + 1):
        ev[0].record(stream)
        call()
        ev[1].record(stream)
        stream.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    return times


def remove_neighbors(n_base, n_list):
    rng = np.random.default_rng(1)
    base = rng.uniform(-20, 20, (n_base, 2)).astype(np.float32)
    lst = (base[rng.choice(n_base, n_list)] + rng.normal(0, 0.08, (n_list, 2))).astype(np.float32)
    ctx = capi.Context(0)
    d_base, d_list = torch.from_numpy(base).cuda(), torch.from_numpy(lst).cuda()
    out = torch.empty((n_base + 1, 2), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    t = timed(stream, lambda: ctx.check(capi.lib().ndt_remove_neighbors_dev(
        ctx.h, d_base.data_ptr(), 8, n_base, d_list.data_ptr(), 8, n_list, 0.1, out.data_ptr(), cnt.data_ptr(), stream.cuda_stream),
        "ndt_remove_neighbors_dev"))
    n = int(cnt.item())
    ref = O.remove_neighbors(base, lst, 0.1)
    same = n == len(ref) and out[:n].cpu().numpy().tobytes() == ref.tobytes()
    # the call's table: one job, a 24-byte unit per 256 base points, a submap, a previous cloud, a count word, each from a 64-byte line
    table = sum(-(-b // 64) * 64 for b in (88, 24 * -(-n_base // 256), 8, 16, 8))
    pinned, dst = torch.empty(table, dtype=torch.uint8).pin_memory(), torch.empty(table, dtype=torch.uint8, device="cuda")
    with torch.cuda.stream(stream):
        c = timed(stream, lambda: dst.copy_(pinned, non_blocking=True))
    print("remove_neighbors %d x %d: device %.4f ms (best of 8 after a warm-up of %.3f; all %s), a pinned-to-device copy of %d bytes "
          "alone %.4f ms (best of 8; all %s), kept %d, identical %s"
          % (n_base, n_list, min(t[1:]), t[0], " ".join("%.4f" % x for x in t[1:]), table, min(c[1:]),
             " ".join("%.4f" % x for x in c[1:]), n, same))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "rn":
        return remove_neighbors(int(sys.argv[2]) if len(sys.argv) > 2 else 10000, int(sys.argv[3]) if len(sys.argv) > 3 else 1000)
    n_scans = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    n_pts = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    scans = synth.submap_scans(n_scans, n_pts)
    off = np.zeros(n_scans + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in scans])
    ctx = capi.Context(0)
    allp = torch.from_numpy(np.concatenate(scans)).cuda()
    out = torch.empty((len(allp) + 1, 2), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    times = timed(stream, lambda: ctx.make_map_dev(allp.data_ptr(), 8, off, True, True, True, 0.05, 0.1, out.data_ptr(), cnt.data_ptr(),
                                                   stream=stream.cuda_stream), reps=7)
    n = int(cnt.item())
    t0 = time.perf_counter()
    ref = O.make_map(scans, True, True, True, 0.05, 0.1)
    cpu = time.perf_counter() - t0
    same = n == len(ref) and out[:n].cpu().numpy().tobytes() == ref.tobytes()
    print("make_map %d scans x %d pts: device %.3f ms (best of 8, first %.3f), oracle on 1 core %.1f ms, kept %d of %d, "
          "identical %s" % (n_scans, n_pts, min(times[1:]), times[0], cpu * 1e3, n, len(allp), same))


if __name__ == "__main__":
    main()
