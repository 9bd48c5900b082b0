"""Times of ndt_pg_marginals_batch_dev beside the plain optimiser's (LOG.md R45.1): the pose-graph timing workload of
tools/pg_bench.py -- 256 figure-eights of 2000 nodes, 5 loop arcs --, one (anchor, last) query per graph (6 columns) and one
(last, last) query per graph (3 columns).  HIP events on the stream the calls run on, two warm runs, the median, minimum and
maximum of the repeats, the cases alternating.  python tools/pg_marginals_bench.py  ->  one line per case; --json PATH."""
import sys, os, json
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import pg_helpers as H
from ndt_slam_amd import capi

N, G, REPS = 2000, 256, 7
ctx = capi.Context(0)
dev = torch.device("cuda", 0)
st = torch.cuda.Stream()                               # (a NULL stream would mean the context's own: the events must ride on the calls' stream)
torch.cuda.set_stream(st)

poses, edges = H.figure_eight(N)
P, no, E, eo = H.pack([(poses, edges)] * G)
d_p0 = torch.from_numpy(P.reshape(-1).copy()).to(dev)
d_p = d_p0.clone()
d_e = torch.from_numpy(E.view(np.uint8).copy()).to(dev)
d_r = torch.zeros(G * capi.PG_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
d_m = torch.zeros(G * capi.PG_MARGINAL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
anchor, last = N // 4, N - 1                           # (3 N / 4, N / 4) is one of the loop arcs
queries = {"six columns (anchor, last)": [(g, anchor, last) for g in range(G)], "three columns (last, last)": [(g, last, last) for g in range(G)]}
torch.cuda.synchronize()


def solve(a=None, b=None):
    d_p.copy_(d_p0)
    if a is not None:
        a.record(st)
    capi.optimize_pose_graphs_dev(ctx, d_p.data_ptr(), no, d_e.data_ptr(), eo, d_r.data_ptr(), stream=st.cuda_stream)
    if b is not None:
        b.record(st)


def marginals(qs):
    def run(a=None, b=None):
        if a is not None:
            a.record(st)
        capi.pose_graph_marginals_dev(ctx, d_p0.data_ptr(), no, d_e.data_ptr(), eo, qs, d_m.data_ptr(), stream=st.cuda_stream)
        if b is not None:
            b.record(st)
    return run


cases = {"plain optimiser": solve}
cases.update({k: marginals(capi.pg_queries(v)) for k, v in queries.items()})
for fn in cases.values():
    fn(); fn()
torch.cuda.synchronize()
ms = {k: [] for k in cases}
info = {}
for _ in range(REPS):
    for k, fn in cases.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn(a, b)
        torch.cuda.synchronize()
        ms[k].append(a.elapsed_time(b))
        if k == "plain optimiser":
            res = np.frombuffer(d_r.cpu().numpy().tobytes(), dtype=capi.PG_RESULT_DTYPE)
            info[k] = dict(iterations=int(res[0]["iterations"]), cg=int(res[0]["cg_iterations"]), converged=int(res["converged"].min()))
        else:
            res = np.frombuffer(d_m.cpu().numpy().tobytes(), dtype=capi.PG_MARGINAL_DTYPE)
            info[k] = dict(cg=[int(res["cg_iterations"].min()), int(res["cg_iterations"].max())], converged=int(res["converged"].min()),
                           status=int(np.abs(res["status"]).max()), trace_Sbb=float(np.trace(res[0]["Sbb"].reshape(3, 3))))
out = {k: dict(ms_median=float(np.median(v)), ms_min=float(min(v)), ms_max=float(max(v)), **info[k]) for k, v in ms.items()}
for k, v in out.items():
    print("N=%d G=%d %s" % (N, G, k), v, flush=True)
six, three = out["six columns (anchor, last)"]["ms_median"], out["three columns (last, last)"]["ms_median"]
out["ratio six / three"] = six / three
print("six columns / three columns: %.3f" % (six / three), flush=True)
if "--json" in sys.argv:
    json.dump(out, open(sys.argv[sys.argv.index("--json") + 1], "w"), indent=1)
