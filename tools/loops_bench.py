"""Time of one ndt_sessions_find_loops over S sessions that have closed the loop of tests/loops_helpers.loop_workload (the 5 m
circle, 56 frames of 181 beams, sepThre 5), against the same search made session by session of the single-job entry points
(ndt_repose_points_dev, ndt_prefilter_batch_dev with one scan, ndt_map_build_dev in place, ndt_relocalize_dev) on device
copies of the same scans and closed clouds; and, by device events, of the multi-job sweep against J ndt_score_lattice_dev
launches on the same jobs (LOG.md R34.1).  Host clock around calls that end in a device synchronise; two warm rounds, the
forms alternated, median and range of the repeats.
python tools/loops_bench.py [--sessions 256] [--reps 9] [--json PATH]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ndt_slam_amd import capi, replay, synth  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


S, REPS, FRAMES, N_LOGS = arg("--sessions", 256), arg("--reps", 9), 56, 8
p = dict(replay.LAUNCH_PARAMS, sepThre=5.0)
ctx = capi.Context(0)
dev = torch.device("cuda", 0)

logs = []
for seed in range(33, 33 + N_LOGS):
    recs, _ = synth.replay_records(n_frames=FRAMES, n_beams=181, step=0.6, seed=seed)
    logs.append(([np.asarray(r["front"], np.float64).reshape(-1, 2) for r in recs],
                 np.array([[r["x"], r["y"], r["th"]] for r in recs], np.float64)))
ses = capi.Sessions(ctx, S, capi.session_params_from_launch(p))
for k in range(FRAMES):
    recs = ses.step([logs[i % N_LOGS][0][k] for i in range(S)], np.array([logs[i % N_LOGS][1][k] for i in range(S)]))
    assert recs["stepped"].all() and not recs["status"].any()
lp = capi.default_loop_params()
cands = ses.loop_candidates(lp)
J = len(cands)
assert J == S, "every session has come back to its first submap"


# the per-session form's inputs: the newest scan in the map frame (resampled, at the pose of its record) and the candidate
# submap's closed cloud, on the device; a map per session, rebuilt in place by every search
def map_frame(lps, pose):
    a = np.radians(pose[2])
    c, s = np.cos(a), np.sin(a)
    return np.stack([c * lps[:, 0] - s * lps[:, 1] + pose[0], s * lps[:, 0] + c * lps[:, 1] + pose[1]], axis=1).astype(np.float32)


params = capi.default_params(resolution=p["Resolution"], step_size=p["StepSize"], trans_eps=p["TransformationEpsilon"],
                             max_iter=p["MaximumIterations"], grid_margin=8)
zero = torch.zeros((1, 3), dtype=torch.float64, device=dev)
per = []
for c in cands:
    i = int(c["session"])
    pose = ses.trajectory(i)[0][-1]
    scan = map_frame(replay.resample_points(logs[i % N_LOGS][0][FRAMES - 1], p["space"], p["space_thre"]), pose)
    cloud = ses.global_map(i)[1][int(c["submap"])]
    n = len(scan)
    per.append(dict(scan=torch.from_numpy(scan).to(dev), n=n, off=torch.tensor([0, n], dtype=torch.int64, device=dev),
                    pose=torch.from_numpy(pose.reshape(1, 3).copy()).to(dev), robot=torch.zeros((n, 2), dtype=torch.float32, device=dev),
                    filt=torch.zeros((n, 2), dtype=torch.float32, device=dev), foff=torch.zeros(2, dtype=torch.int64, device=dev),
                    cloud=torch.from_numpy(np.ascontiguousarray(cloud)).to(dev), n_cloud=len(cloud),
                    lattice=capi.PoseLattice.from_buffer_copy(c["lattice"].tobytes())))
torch.cuda.synchronize()
for d in per:
    d["map"] = capi.Map(ctx, params=params, dev_ptr=d["cloud"].data_ptr(), n=d["n_cloud"])
torch.cuda.synchronize()


def per_session():
    """robot frame -> pre-filter -> the old submap's map -> ndt_relocalize_dev, one session after the other."""
    found = 0
    for d in per:
        capi.repose_points_dev(ctx, d["scan"].data_ptr(), 8, d["off"].data_ptr(), 1, d["pose"].data_ptr(), zero.data_ptr(),
                               d["robot"].data_ptr(), 8)
        ctx.prefilter_batch_dev(d["robot"].data_ptr(), 8, d["off"].data_ptr(), 1, d["n"], p["LeafSize"], d["filt"].data_ptr(),
                                d["foff"].data_ptr())
        torch.cuda.synchronize()
        d["nf"] = int(d["foff"][1].item())
        d["map"].rebuild(dev_ptr=d["cloud"].data_ptr(), n=d["n_cloud"])
        out = d["map"].relocalize(None, d["lattice"], top_k=lp.top_k, local_max=bool(lp.local_max), dev_ptr=d["filt"].data_ptr(),
                                  n=d["nf"], stride=8)
        if out["best"] >= 0:
            r = out["records"][out["best"]]
            found += int((r["fitness"] if r["converged"] else 1e7) <= lp.max_cost)
    torch.cuda.synchronize()
    return found


def one_call():
    t0 = time.perf_counter()
    loops = ses.find_loops(lp)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, int(loops["found"].sum())


def looped():
    t0 = time.perf_counter()
    found = per_session()
    return (time.perf_counter() - t0) * 1e3, found


for _ in range(2):                                       # warm: both forms
    one_call()
    looped()
a, b = [], []
for _ in range(REPS):
    a.append(one_call())
    b.append(looped())
stats = ses.stats()

# the sweep alone, by device events on one stream: one multi-job launch against J single-job launches on the same jobs
st = torch.cuda.Stream()
pts = torch.cat([d["filt"][:d["nf"]] for d in per]).contiguous()
off = torch.tensor(np.concatenate([[0], np.cumsum([d["nf"] for d in per])]), dtype=torch.int64, device=dev)
jobs = [(j, j, d["lattice"]) for j, d in enumerate(per)]
P = per[0]["lattice"].size
score = torch.zeros(J * P, dtype=torch.float64, device=dev)
pairs = torch.zeros(J * P, dtype=torch.int32, device=dev)
torch.cuda.synchronize()


def sweep_multi():
    ctx.score_lattice_multi_dev([d["map"] for d in per], pts.data_ptr(), off.data_ptr(), J, len(pts), jobs, score.data_ptr(), pairs.data_ptr(),
                                stream=st.cuda_stream)


def sweep_single():
    for j, d in enumerate(per):
        d["map"].score_lattice(d["filt"].data_ptr(), d["nf"], d["lattice"], score.data_ptr() + 8 * j * P, pairs.data_ptr() + 4 * j * P,
                               stream=st.cuda_stream)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1)


for _ in range(2):
    timed(sweep_multi)
    timed(sweep_single)
m, s1 = [], []
for _ in range(REPS):
    m.append(timed(sweep_multi))
    s1.append(timed(sweep_single))


def summary(x):
    return dict(median=float(np.median(x)), min=float(min(x)), max=float(max(x)))


# ---- the search over several submaps (ndt_sessions_find_loops_multi; LOG.md R40.1): S sessions x 2 submaps in one call, against
# what a caller composes today -- ndt_sessions_find_loops for the nearest submap, then per extra submap and session a build,
# the single-job sweep, pick and match (ndt_relocalize_dev), and one ndt_fit_points_batch_dev per map (the nearest submaps' maps
# are the set's own, so the caller builds those again for its verification).  Beside them the one call at 1, 2 and 4 submaps
# and ndt_sessions_find_loops with the same gating.
MULTI = dict(radius=4.0, max_d2=0.09, min_overlap=0.5)
mp2 = capi.default_loop_multi_params(max_submaps=2, **MULTI)
cands2 = ses.loop_candidates_multi(mp2)
assert len(cands2) == 2 * S, "every session has two old submaps within 4 m"
extra = []
for c in cands2:
    i = int(c["session"])
    cloud = np.ascontiguousarray(ses.global_map(i)[1][int(c["submap"])])
    d = per[[int(x["session"]) for x in cands].index(i)]
    e = dict(base=d, session=i, cloud=torch.from_numpy(cloud).to(dev), n_cloud=len(cloud), lattice=capi.PoseLattice.from_buffer_copy(c["lattice"].tobytes()),
             nearest=int(c["submap"]) == int(cands2[cands2["session"] == i][0]["submap"]),
             stats=torch.zeros(capi.NDT_LOOP_MAX_CAND * 32, dtype=torch.uint8, device=dev))
    extra.append(e)
torch.cuda.synchronize()
for e in extra:
    e["map"] = capi.Map(ctx, params=params, dev_ptr=e["cloud"].data_ptr(), n=e["n_cloud"])
torch.cuda.synchronize()
TF_AT = capi.RESULT_DTYPE.fields["T00"][1]


def composed():
    t0 = time.perf_counter()
    loops, recs = ses.find_loops(mp2.loop, want_records=True)
    row = {int(l["cand"]["session"]): j for j, l in enumerate(loops)}
    for e in extra:
        d = e["base"]
        e["map"].rebuild(dev_ptr=e["cloud"].data_ptr(), n=e["n_cloud"])
        if e["nearest"]:
            j = row[e["session"]]
            rec = recs[j][:int(loops[j]["n_cand"])]
        else:
            rec = e["map"].relocalize(None, e["lattice"], top_k=lp.top_k, local_max=bool(lp.local_max), dev_ptr=d["filt"].data_ptr(),
                                      n=d["nf"], stride=8)["records"]
        if len(rec):
            d_rec = torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8)).to(dev)
            e["map"].fit_points_dev(d["filt"].data_ptr(), d["foff"].data_ptr(), len(rec), d["nf"], d_rec.data_ptr() + TF_AT, capi.RESULT_BYTES,
                                    mp2.max_d2, None, e["stats"].data_ptr(), shared_scan=True)
            e["st"] = e["stats"].cpu()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def multi_call(prm):
    t0 = time.perf_counter()
    loops = ses.find_loops_multi(prm)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, len(loops), int(loops["loop"]["found"].sum())


def single_call(prm):
    t0 = time.perf_counter()
    ses.find_loops(prm)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


forms = {"multi_x1": capi.default_loop_multi_params(max_submaps=1, **MULTI), "multi_x2": mp2,
         "multi_x4": capi.default_loop_multi_params(max_submaps=4, **dict(MULTI, radius=10.0))}
for _ in range(2):
    composed()
    single_call(mp2.loop)
    for prm in forms.values():
        multi_call(prm)
t_comp, t_single, t_multi = [], [], {k: [] for k in forms}
for _ in range(REPS):
    t_comp.append(composed())
    t_single.append(single_call(mp2.loop))
    for k, prm in forms.items():
        t_multi[k].append(multi_call(prm))
mstats = {}
for k, prm in forms.items():
    ses.find_loops_multi(prm)
    q = ses.stats()
    mstats[k] = dict(host_waits=q.host_waits, candidates=q.sessions_stepped, h2d_bytes=int(q.h2d_bytes), d2h_bytes=int(q.d2h_bytes))
multi_out = dict(composed_x2_ms=summary(t_comp), find_loops_radius4_ms=summary(t_single),
                 **{k + "_ms": summary([t for t, _, _ in v]) for k, v in t_multi.items()},
                 **{k + "_found": v[-1][2] for k, v in t_multi.items()}, stats=mstats)
for e in extra:
    e["map"].close()

out = dict(find_loops_multi=multi_out,
sessions=S, candidates=J, reps=REPS, lattice_poses=int(P), filtered_points=int(np.mean([d["nf"] for d in per])),
           cloud_points=int(np.mean([d["n_cloud"] for d in per])),
           find_loops_ms=summary([t for t, _ in a]), per_session_ms=summary([t for t, _ in b]),
           found=dict(find_loops=a[-1][1], per_session=b[-1][1]),
           sweep_multi_ms=summary(m), sweep_single_sum_ms=summary(s1),
           host_waits=stats.host_waits, h2d_bytes=int(stats.h2d_bytes), d2h_bytes=int(stats.d2h_bytes))
print(json.dumps(out), flush=True)
if "--json" in sys.argv:
    json.dump(out, open(sys.argv[sys.argv.index("--json") + 1], "w"), indent=1)
for d in per:
    d["map"].close()
ses.close()
