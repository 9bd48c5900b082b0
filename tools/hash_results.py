"""Result records of fixed workloads as hashes, to compare library builds bit for bit (run once per build with
NDT_LIB_PATH): C3 batch of 256, a ragged batch of 301, 24 scans (helpers from the start), 512 seeds of one scan on the
5M-point map (shared_scan), C1 x 24.  Usage: python tools/hash_results.py [--c5]

--pg: the pose-graph kernels alone (seconds), one hash per output, once through the host-pointer entry points and once through
the _dev ones.  Plain solver: one batch of figure-eights on either side of the sweep's pieces of 64 nodes, dense graphs around
the key array's power of two, a far start that takes halvings, a graph without arcs and a faulted one.  Robust solver: drifted
graphs with and without phi -- poses, records, weights, chi-squares.  Marginals: three- and six-column queries over the tests'
query nodes, with and without weights, and bad queries."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ndt_slam_amd import capi, synth               # noqa: E402


def h(a):
    return hashlib.sha256(a.tobytes()).hexdigest()[:16]


def main():
    ctx = capi.Context(0)
    cfg = synth.CONFIGS["C3"]
    m = synth.make_map(cfg["n_map"], cfg["half"])
    sf = synth.ScanFactory(m, cfg["half"], cfg["n_scan"])
    gm = capi.Map(ctx, m, capi.default_params(resolution=cfg["resolution"]))
    scans, off, truths, inits = sf.batch(0, 301)
    r = gm.align_batch(scans[:int(off[256])], off[:257], inits[:256])
    print("C3x256", h(r), "evals %.3f T %s" % (r["evals"].mean(), h(np.stack([r["T00"], r["T10"], r["T03"], r["T13"]]))), "iters", h(r["iters"]))
    keep = np.ones(len(scans), bool)
    for b in range(0, 301, 3):
        keep[int(off[b]) + 7000:int(off[b + 1])] = False
    lens = np.array([keep[int(off[b]):int(off[b + 1])].sum() for b in range(301)])
    r = gm.align_batch(scans[keep], np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), inits)
    print("ragged301", h(r), "T", h(np.stack([r["T00"], r["T10"], r["T03"], r["T13"]])))
    r = gm.align_batch(scans[:int(off[24])], off[:25], inits[:24])
    print("C3x24", h(r), "T", h(np.stack([r["T00"], r["T10"], r["T03"], r["T13"]])))
    c1 = synth.CONFIGS["C1"]
    m1 = synth.make_map(c1["n_map"], c1["half"])
    s1 = synth.ScanFactory(m1, c1["half"], c1["n_scan"])
    g1 = capi.Map(ctx, m1, capi.default_params(resolution=c1["resolution"]))
    sc, of, tr, ini = s1.batch(0, 24)
    r = g1.align_batch(sc, of, ini)
    print("C1x24", h(r), "T", h(np.stack([r["T00"], r["T10"], r["T03"], r["T13"]])))
    if "--c5" in sys.argv:
        c5 = synth.CONFIGS["C5"]
        m5 = synth.make_map(c5["n_map"], c5["half"])
        s5 = synth.ScanFactory(m5, c5["half"], c5["n_scan"])
        scan, truth, _ = s5.make(0)
        seeds = synth.hypothesis_seeds(truth, c5["seeds"])[::8]
        g5 = capi.Map(ctx, m5, capi.default_params(resolution=c5["resolution"]))
        r = g5.align_batch(scan, np.array([0, len(scan)], np.uint64), seeds, shared_scan=True)
        print("C5x512", h(r), "T", h(np.stack([r["T00"], r["T10"], r["T03"], r["T13"]])), "iters", h(r["iters"]))


def pg_workloads():
    """-> (plain: [(name, poses, edges)], robust: [(name, poses, edges, phi or None)], marginals: [(name, poses, edges, queries)])"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import pg_helpers as H
    import pg_robust_helpers as R
    import pg_marginal_helpers as M
    plain = [("eight%d" % n,) + H.figure_eight(n) for n in (2, 24, 63, 64, 65, 129, 257)]
    plain += [("dense24_%d" % e,) + H.dense(24, e) for e in (127, 128, 129)]
    plain.append(("far24a",) + H.far_start(*H.FAR_STARTS["far24a"]))
    plain.append(("no_arcs", H.eight_truth(3), np.zeros(0, H.PG_EDGE_DTYPE)))
    poses, edges = H.figure_eight(24)
    edges = edges.copy()
    edges[7]["to"] = 24                                # (an arc end out of range)
    plain.append(("faulted", poses, edges))
    robust = []
    for name in ("d65a", "d65b", "p128"):
        fn, args = R.ROBUST_WORKLOADS[name]
        poses, edges, phi, _ = fn(*args)
        robust += [(name, poses, edges, phi), (name + "_no_phi", poses, edges, None)]
    marg = []
    for n in (4, 65, 66, 257):
        poses, edges = H.figure_eight(n)
        nodes = M.query_nodes(n)
        q = [(a, a) for a in nodes] + list(zip(nodes[:-1], nodes[1:])) + [(0, b) for b in nodes] + [(n, 1), (1, -1)]
        marg.append(("eight%d" % n, poses, edges, q))
    return H, plain, robust, marg


def pg_main():
    import torch
    H, plain, robust, marg = pg_workloads()
    ctx = capi.Context(0)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    down = lambda t, dtype: np.frombuffer(t.cpu().numpy().tobytes(), dtype=dtype)
    cut = lambda a, off, g: a[int(off[g]):int(off[g + 1])]
    for form in ("host", "dev"):
        P, no, E, eo = H.pack([(p, e) for _, p, e in plain])
        if form == "host":
            out, res = capi.optimize_pose_graphs(ctx, P, no, E, eo)
        else:
            d_p, d_e, d_r = up(P), up(E), up(np.zeros(len(plain), capi.PG_RESULT_DTYPE))
            capi.optimize_pose_graphs_dev(ctx, d_p.data_ptr(), no, d_e.data_ptr(), eo, d_r.data_ptr())
            torch.cuda.synchronize()
            out, res = down(d_p, np.float64).reshape(-1, 3), down(d_r, capi.PG_RESULT_DTYPE)
        for g, (name, _, _) in enumerate(plain):
            print("pg", form, "plain", name, "poses", h(cut(out, no, g)), "record", h(res[g:g + 1]),
                  "iters %d cg %d status %d" % (res[g]["iterations"], res[g]["cg_iterations"], res[g]["status"]))
        for name, poses, edges, phi in robust:
            P, no, E, eo = H.pack([(poses, edges)])
            if form == "host":
                out, res, w, c = capi.optimize_pose_graphs_robust(ctx, P, no, E, eo, phi=phi)
            else:
                d_p, d_e, d_r = up(P), up(E), up(np.zeros(1, capi.PG_ROBUST_RESULT_DTYPE))
                d_f, d_w, d_c = (up(phi) if phi is not None else None), up(np.zeros(len(E))), up(np.zeros(len(E)))
                capi.optimize_pose_graphs_robust_dev(ctx, d_p.data_ptr(), no, d_e.data_ptr(), eo, d_r.data_ptr(),
                                                     phi_ptr=d_f.data_ptr() if d_f is not None else None, weight_ptr=d_w.data_ptr(),
                                                     chi2_ptr=d_c.data_ptr())
                torch.cuda.synchronize()
                out, res = down(d_p, np.float64), down(d_r, capi.PG_ROBUST_RESULT_DTYPE)
                w, c = down(d_w, np.float64), down(d_c, np.float64)
            print("pg", form, "robust", name, "poses", h(out), "record", h(res), "weights", h(w), "chi2", h(c),
                  "iters %d levels %d rejected %d" % (res[0]["pg"]["iterations"], res[0]["levels"], res[0]["n_rejected"]))
        P, no, E, eo = H.pack([(p, e) for _, p, e, _ in marg])
        q = capi.pg_queries([(g, a, b) for g, (_, _, _, qs) in enumerate(marg) for a, b in qs] + [(len(marg), 0, 1)])
        weight = np.random.default_rng(5).uniform(0.5, 1.5, len(E))
        for wname, wt in (("unweighted", None), ("weighted", weight)):
            if form == "host":
                rec = capi.pose_graph_marginals(ctx, P, no, E, eo, q, weight=wt)
            else:
                d_p, d_e, d_m = up(P), up(E), up(np.zeros(len(q), capi.PG_MARGINAL_DTYPE))
                d_w = up(wt) if wt is not None else None
                capi.pose_graph_marginals_dev(ctx, d_p.data_ptr(), no, d_e.data_ptr(), eo, q, d_m.data_ptr(),
                                              weight_ptr=d_w.data_ptr() if d_w is not None else None)
                torch.cuda.synchronize()
                rec = down(d_m, capi.PG_MARGINAL_DTYPE)
            for g, (name, _, _, _) in enumerate(marg):
                mine = rec[q["graph"] == g]
                print("pg", form, "marginals", wname, name, "records", h(mine), "queries %d converged %d refused %d cg %d..%d" % (
                    len(mine), mine["converged"].sum(), (mine["status"] != 0).sum(), mine["cg_iterations"].min(), mine["cg_iterations"].max()))
            print("pg", form, "marginals", wname, "bad_graph", "records", h(rec[q["graph"] == len(marg)]))


if __name__ == "__main__":
    pg_main() if "--pg" in sys.argv else main()
