"""Times of the place-recognition calls (LOG.md R47.1): 256 searchers against 256 tracks x 40 items x 15 descriptors, 20 rings.
Clouds: walls of the 24 x 16 m hall, 1 500 points per closed submap, 3 000 per local map.  HIP events on the stream the calls run
on, two warm runs, the median, minimum and maximum of the repeats.  describe = ndt_place_describe_batch_dev over all 153 856
descriptors; match_and_pick = ndt_place_match_dev (its table upload and both launches); pick = the same call on items without
descriptors, where the match kernel only writes zeros -- the pick kernel's share, from above.  host = ndt_place_match_host on
one core for HOST_Q of the queries, scaled to all of them.  python tools/place_timing.py  ->  one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ndt_slam_amd import capi

N_Q, TRACKS, ITEMS, PER, REPS, HOST_Q = 256, 256, 40, 15, 7, 2
N_SUB, N_LOCAL = 1500, 3000
rng = np.random.default_rng(47)
ctx = capi.Context(0)
dev = torch.device("cuda", 0)
st = torch.cuda.Stream()                               # (a NULL stream would mean the context's own: the events must ride on the calls' stream)
torch.cuda.set_stream(st)
p = capi.default_place_params()
R = p.n_rings


def hall(n, around, reach):
    """n wall points of the hall within `reach` of a pose, as a submap or a local map sees them."""
    t = rng.uniform(0, 1, 4 * n)
    side = rng.integers(0, 4, 4 * n)
    x = np.where(side == 0, 24 * t, np.where(side == 1, 24 * t, np.where(side == 2, 0.0, 24.0)))
    y = np.where(side == 0, 0.0, np.where(side == 1, 16.0, 16 * t))
    xy = np.stack([x, y], axis=1) + rng.normal(0, 0.01, (4 * n, 2))
    near = xy[np.hypot(*(xy - around).T) < reach]
    return near[:n].astype(np.float32)


n_items = TRACKS * ITEMS
item_pose = rng.uniform([2, 2], [22, 14], (n_items, 2))
base = [hall(N_SUB, item_pose[i], 12.0) for i in range(64)]                 # 64 distinct clouds, dealt to the items in turn
clouds = [base[i % 64] for i in range(n_items)]
centres = np.repeat(item_pose, PER, axis=0) + rng.normal(0, 0.5, (n_items * PER, 2))
cloud_of = np.repeat(np.arange(n_items), PER)
q_pose = rng.uniform([2, 2], [22, 14], (N_Q, 2))
q_base = [hall(N_LOCAL, q_pose[i], 12.0) for i in range(N_Q)]
pts, off = capi.pack_scans(clouds + q_base)
all_centres = np.concatenate([centres, q_pose])
all_cloud_of = np.concatenate([cloud_of, n_items + np.arange(N_Q)])
n_desc = len(all_centres)
d_xy = torch.from_numpy(pts).to(dev)
d_desc = torch.zeros(n_desc * R, dtype=torch.int64, device=dev)
d_out = torch.zeros(N_Q * p.top_k * 8, dtype=torch.int32, device=dev)
d_n = torch.zeros(N_Q, dtype=torch.int32, device=dev)
d_table = torch.zeros(N_Q * n_items, dtype=torch.int64, device=dev)
item_first = np.arange(0, n_items * PER + 1, PER, dtype=np.int32)
item_group = np.repeat(np.arange(TRACKS, dtype=np.int32), ITEMS)
q_group = np.arange(N_Q, dtype=np.int32)
torch.cuda.synchronize()


def describe():
    capi.place_describe_batch_dev(ctx, d_xy.data_ptr(), 8, off, all_centres, all_cloud_of, p, d_desc.data_ptr(), stream=st.cuda_stream)


def match(first=item_first):
    capi.place_match_dev(ctx, d_desc.data_ptr() + n_items * PER * R * 8, q_group, d_desc.data_ptr(), first, item_group, p, d_out.data_ptr(),
                         d_n.data_ptr(), d_table.data_ptr(), stream=st.cuda_stream)


def timed(fn):
    ms = []
    for k in range(REPS + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st); fn(); b.record(st)
        torch.cuda.synchronize()
        if k >= 2:
            ms.append(a.elapsed_time(b))
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


out = dict(workload=dict(queries=N_Q, tracks=TRACKS, items=n_items, descriptors=n_items * PER, rings=R, points_per_submap=N_SUB,
                         points_per_local_map=N_LOCAL, described_points=int(sum(len(clouds[c]) for c in cloud_of) + sum(len(c) for c in q_base))))
out["describe_ms"] = timed(describe)
out["match_and_pick_ms"] = timed(match)
out["pick_ms"] = timed(lambda: match(np.zeros(n_items + 1, np.int32)))
describe(); match()
torch.cuda.synchronize()
desc = d_desc.cpu().numpy().view(np.uint64).reshape(n_desc, R)
hits = d_out.cpu().numpy().view(capi.PLACE_HIT_DTYPE).reshape(N_Q, p.top_k)
t0 = time.perf_counter()
h_hits, h_n, _ = capi.place_match_host(desc[n_items * PER:][:HOST_Q], q_group[:HOST_Q], desc[:n_items * PER], item_first, item_group, p)
dt = time.perf_counter() - t0
assert h_hits.tobytes() == hits[:HOST_Q].tobytes() and h_n.tobytes() == d_n.cpu().numpy()[:HOST_Q].tobytes()
out["host_match_ms"] = dict(measured_queries=HOST_Q, per_query=1e3 * dt / HOST_Q, all_queries_scaled=1e3 * dt / HOST_Q * N_Q)
out["mean_key_of_best_hit"] = float(hits[:, 0]["key"].mean())
print(json.dumps(out))
