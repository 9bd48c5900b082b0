"""Times of the pose-graph launch and of re-posing (LOG.md R23.1): HIP events on the stream the calls run on, two warm runs,
the median of the repeats.  python tools/pg_bench.py  ->  one line per case, and --json PATH for the figures."""
import sys, os, json
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import pg_helpers as H
from ndt_slam_amd import capi

ctx = capi.Context(0)
dev = torch.device("cuda", 0)
st = torch.cuda.Stream()                               # (a NULL stream would mean the context's own: the events must ride on the calls' stream)
torch.cuda.set_stream(st)
out = {}


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn(a, b)
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


for n_loops in (5, 40):
    poses, edges = H.figure_eight(2000, n_loops=n_loops)
    for G in (256, 1):
        P, no, E, eo = H.pack([(poses, edges)] * G)
        d_p0 = torch.from_numpy(P.reshape(-1).copy()).to(dev)
        d_p = d_p0.clone()
        d_e = torch.from_numpy(E.view(np.uint8).copy()).to(dev)
        d_r = torch.zeros(G * 32, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def run(a=None, b=None):
            d_p.copy_(d_p0)
            if a is not None:
                a.record(st)
            capi.optimize_pose_graphs_dev(ctx, d_p.data_ptr(), no, d_e.data_ptr(), eo, d_r.data_ptr(), stream=st.cuda_stream)
            if b is not None:
                b.record(st)
        med, lo, hi = timed(run, 5)
        res = np.frombuffer(d_r.cpu().numpy().tobytes(), dtype=capi.PG_RESULT_DTYPE)
        key = "solve N=2000 loops=%d G=%d" % (n_loops, G)
        out[key] = dict(ms_median=med, ms_min=lo, ms_max=hi, iterations=int(res[0]["iterations"]), cg=int(res[0]["cg_iterations"]),
                        converged=int(res["converged"].min()), cost=[float(res[0]["cost_initial"]), float(res[0]["cost_final"])])
        print(key, out[key], flush=True)

K, n_each = 256, 100000
rng = np.random.default_rng(1)
xy = torch.from_numpy((rng.uniform(-50, 50, (K * n_each, 2)) + np.array([-1003.3, 707.1])).astype(np.float32)).to(dev)
d_out = torch.zeros_like(xy)
off = torch.from_numpy((np.arange(K + 1) * n_each).astype(np.int64)).to(dev)
old = np.stack([rng.uniform(-1010, -990, K), rng.uniform(700, 715, K), rng.uniform(-180, 180, K)], axis=1)
new = old + rng.normal(0, 0.2, (K, 3))
d_old, d_new = torch.from_numpy(old).to(dev), torch.from_numpy(new).to(dev)
torch.cuda.synchronize()


def rp(a=None, b=None):
    if a is not None:
        a.record(st)
    capi.repose_points_dev(ctx, xy.data_ptr(), 8, off.data_ptr(), K, d_old.data_ptr(), d_new.data_ptr(), d_out.data_ptr(), 8, stream=st.cuda_stream)
    if b is not None:
        b.record(st)
med, lo, hi = timed(rp, 11, warm=3)
out["repose 256 x 100k"] = dict(ms_median=med, ms_min=lo, ms_max=hi, gb_per_s=K * n_each * 16 / med / 1e6)
print("repose", out["repose 256 x 100k"], flush=True)
if "--json" in sys.argv:
    json.dump(out, open(sys.argv[sys.argv.index("--json") + 1], "w"), indent=1)
