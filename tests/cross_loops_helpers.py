"""What the cross-session loop tests share: the numpy restatement of the cross gate (ndt_cross_gate's rule in
include/ndt_mi355x.h, written from the rule and sharing no code with the library), crafted tracks, and the sets' read-outs as
tracks."""
import math

import numpy as np


def track(poses, per_submap, cloud=100):
    """(poses, sub_first, sub_anchor, sub_offsets) of a trajectory cut into submaps of `per_submap` scans, the last one open;
    every closed cloud has `cloud` points."""
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    first = np.arange(0, len(poses), per_submap, dtype=np.int32)
    ends = np.append(first[1:] - 1, len(poses) - 1)
    anchor = (first + (ends - first) // 2).astype(np.int32)
    off = (np.arange(len(first) + 1) * cloud).astype(np.uint64)
    return poses, first, anchor, off


def line(x0, y0, n, step=0.5, heading_deg=0.0):
    """n poses along a straight line."""
    a = math.radians(heading_deg)
    k = np.arange(n, dtype=np.float64)
    return np.stack([x0 + k * step * math.cos(a), y0 + k * step * math.sin(a), np.full(n, heading_deg)], axis=1)


def cross_gate_ref(capi, last_pose, newest_scan, own, tracks, p, session=0):
    """The rule, restated: CROSS_CANDIDATE_DTYPE records (zeroed first, so the padding is 0) of one searcher."""
    L = np.asarray(last_pose, np.float64).reshape(3)
    r2 = np.float64(p.loop.radius) * np.float64(p.loop.radius)
    hits = []
    for t, (poses, first, anchor, off) in enumerate(tracks):
        if t == own:
            continue
        T = np.asarray(poses, np.float64).reshape(-1, 3)
        for m in range(len(first) - 1):                                       # every closed submap
            a, e = int(first[m]), int(first[m + 1]) - 1
            if e < a or int(off[m + 1]) == int(off[m]):
                continue
            dx, dy = L[0] - T[a:e + 1, 0], L[1] - T[a:e + 1, 1]
            d2 = dx * dx + dy * dy                                            # elementwise: every operation rounded once
            k = int(np.argmin(d2))                                            # (the first index of the minimum)
            if d2[k] <= r2:
                hits.append((float(d2[k]), t, m, a + k, int(anchor[m])))
    hits.sort(key=lambda h: h[:3])
    hits = hits[:p.max_submaps]
    out = np.zeros(len(hits), dtype=capi.CROSS_CANDIDATE_DTYPE)
    lp = p.loop
    yaw = L[2] * np.float64(math.pi) / np.float64(180)
    for r, (d2, t, m, near, anc) in enumerate(hits):
        c = out[r]
        c["cand"]["session"], c["cand"]["submap"], c["cand"]["anchor_scan"] = session, m, anc
        c["cand"]["newest_scan"], c["cand"]["nearest_scan"] = newest_scan, near
        c["cand"]["dist"], c["cand"]["path"] = np.sqrt(np.float64(d2)), 0.0
        lat = c["cand"]["lattice"]
        lat["x0"] = L[0] - np.float64(lp.half_x) * np.float64(lp.step_xy)
        lat["y0"] = L[1] - np.float64(lp.half_y) * np.float64(lp.step_xy)
        lat["yaw0"] = yaw - np.float64(lp.half_yaw) * np.float64(lp.step_yaw)
        lat["step_x"], lat["step_y"], lat["step_yaw"] = lp.step_xy, lp.step_xy, lp.step_yaw
        lat["nx"], lat["ny"], lat["nyaw"] = 2 * lp.half_x + 1, 2 * lp.half_y + 1, 2 * lp.half_yaw + 1
        c["map_session"], c["rank"], c["d2"] = t, r, d2
    return out


def set_tracks(ses, against=None):
    """The tracks of a session set as ndt_sessions_find_cross_loops takes them: (the sessions that are tracks, their
    (poses, sub_first, sub_anchor, sub_offsets) from Sessions.trajectory and Sessions.global_map)."""
    who, tracks = [], []
    for i in range(ses.n):
        if against is not None and not against[i]:
            continue
        poses, first, anchor, _ = ses.trajectory(i)
        if len(poses) < 1 or len(first) < 2:
            continue
        who.append(i)
        off = np.concatenate([[0], np.cumsum([len(c) for c in ses.global_map(i)[1]])]).astype(np.uint64)
        tracks.append((poses, first, anchor, off))
    return who, tracks


def set_gate_ref(capi, ses, p, which=None, against=None):
    """The candidates of a set by the restated rule on its read-outs, with session indices: [(searcher, its records)] in
    ascending searcher order, the searchers without a candidate left out."""
    who, tracks = set_tracks(ses, against)
    out = []
    for i in range(ses.n):
        if which is not None and not which[i]:
            continue
        poses = ses.trajectory(i)[0]
        if len(poses) < 1 or not tracks:
            continue
        ref = cross_gate_ref(capi, poses[-1], len(poses) - 1, who.index(i) if i in who else -1, tracks, p, session=i)
        for c in ref:
            c["map_session"] = who[int(c["map_session"])]
        if len(ref):
            out.append((i, ref))
    return out


def assert_set_candidates(capi, ses, got, p, which=None, against=None):
    """Sessions.cross_candidates' records against set_gate_ref, byte for byte (slices of the library's own memory: a copy of
    a structured array does not carry the padding)."""
    at = 0
    for i, ref in set_gate_ref(capi, ses, p, which, against):
        mine = got[at:at + len(ref)]
        assert mine["cand"]["session"].tolist() == [i] * len(ref), (i, mine["cand"]["session"])
        assert mine.tobytes() == ref.tobytes(), i
        at += len(ref)
    assert at == len(got)

# ---- the cross search composed of public single-job calls on a comparison chain (needs the device) ----

def compose_cross(sc, a, b, cand, mp):
    """One cross candidate's search made of public calls: the map of session b's closed cloud cand["submap"], session a's newest
    scan in the robot frame and pre-filtered, the single-job sweep and pick on the candidate's lattice, one align per pick and
    Map.fit_points at the records' transforms -> (dict(status, n_cand, cand_index, cand_score), records, FIT_STATS records).
    A cloud whose map the single build refuses gives that code and nothing else; a scan that filters to no point picks nothing."""
    import re

    import torch

    from gpu_support import sync, to_dev
    from test_gpu_sessions_correct import chain_poses
    capi, ctx, chain = sc["capi"], sc["ctx"], sc["chain"]
    none, no_fit = np.zeros(0, capi.RESULT_DTYPE), np.zeros(0, capi.FIT_STATS_DTYPE)
    zero = dict(n_cand=0, cand_index=np.zeros(0, np.uint64), cand_score=np.zeros(0))
    cloud = np.ascontiguousarray(chain.pcmaps[b].submaps[int(cand["submap"])].p_cloud, np.float32).reshape(-1, 2)
    try:
        gm = capi.Map(ctx, cloud, chain.params)
    except capi.NdtError as e:
        return dict(zero, status=int(re.search(r"-> (-?\d+):", str(e)).group(1))), none, no_fit
    src = np.ascontiguousarray(chain.pcmaps[a].submaps[-1].scans[-1], np.float32).reshape(-1, 2)
    if len(src):
        robot = capi.repose_points(ctx, src, [0, len(src)], chain_poses(chain, a)[-1:], np.zeros((1, 3)))
        src = ctx.prefilter(robot, sc["p"]["LeafSize"])
    if not len(src):
        gm.close()
        return dict(zero, status=0), none, no_fit
    lp = mp.loop
    L = capi.PoseLattice.from_buffer_copy(cand["lattice"].tobytes())
    d_src = to_dev(src)
    d_s = torch.zeros(L.size, dtype=torch.float64, device=d_src.device)
    d_p = torch.zeros(L.size, dtype=torch.int32, device=d_src.device)
    d_c = torch.zeros(lp.top_k, dtype=torch.int64, device=d_src.device)
    d_n = torch.zeros(1, dtype=torch.int32, device=d_src.device)
    sync()
    gm.score_lattice(d_src.data_ptr(), len(src), L, d_s.data_ptr(), d_p.data_ptr())
    gm.lattice_select(L, d_s.data_ptr(), d_p.data_ptr(), lp.top_k, lp.local_max, d_c.data_ptr(), d_n.data_ptr())
    sync()
    n = int(d_n.cpu()[0])
    idx, score = d_c.cpu().numpy()[:n].astype(np.uint64), d_s.cpu().numpy()
    recs = np.concatenate([gm.align_batch(src, [0, len(src)], L.pose(int(q)).reshape(1, 3)) for q in idx]) if n else none
    fit = no_fit
    if n:
        _, fit = gm.fit_points(np.tile(src, (n, 1)), np.arange(n + 1) * len(src), recs, max_d2=mp.max_d2, want_d2=False)
    gm.close()
    return dict(status=0, n_cand=n, cand_index=idx, cand_score=score[idx.astype(np.int64)]), recs, fit
