"""What the tests of the scan archive and ndt_sessions_occ_rebuild share (tests only).

to_map_dev       archived scans at poses through ONE ndt_scan_to_map_batch_dev call: the float32 map-frame points whose bits
                 the rebuild's end points are defined by
restate          the rebuild of one session restated: to_map_dev, then occ_helpers.integrate from the poses' (tx, ty)
restate_numpy    the same with the transform in numpy (session_helpers.to_map_frame), for a grid compared as rendered
same_counts      a grid's counters against a (hit, pass) pair
views            (local map, p_cloud) of a session, read from the device
alternating_scan a raw scan whose points alternate between radii 3 m and 4 m: the resampler keeps every point
growths          how often an archive of these scan lengths outgrew its allocation (ss_grow's rule)
"""
import numpy as np

import occ_helpers as H
from gpu_support import sync, to_dev
from session_helpers import device_cloud, to_map_frame

STATS_FIELDS = ("h2d_bytes", "d2h_bytes", "host_waits", "triples_run", "sessions_stepped")


def to_map_dev(ctx, scans, poses):
    """scans: [n_k, 2] float64 robot-frame scans, poses [K, 3] -> the list of [n_k, 2] float32 map-frame scans."""
    import torch
    from ndt_slam_amd.capi import pack_scans
    xy, off = pack_scans(scans, dtype=np.float64)
    total = len(xy)
    if not total:
        return [np.zeros((0, 2), np.float32) for _ in scans]
    d_in, d_off = to_dev(xy), to_dev(off.astype(np.int64))
    d_pose = to_dev(np.ascontiguousarray(poses, np.float64).reshape(-1, 3))
    d_out = torch.zeros((total, 2), dtype=torch.float32, device=d_in.device)
    sync()
    ctx.scan_to_map_batch_dev(d_in.data_ptr(), 16, d_off.data_ptr(), len(scans), total, d_pose.data_ptr(), d_out.data_ptr())
    sync()
    out = d_out.cpu().numpy()
    return [out[int(off[k]):int(off[k + 1])].copy() for k in range(len(scans))]


def restate(ctx, geom, scans, poses, max_range2=H.DBL_MAX, counters=None):
    """-> ((hit, pass), stats dict) of every scan k cast from poses[k][:2] to its device-transformed points."""
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    assert len(scans) == len(poses)
    ends = to_map_dev(ctx, scans, poses)
    want, st = H.integrate([geom], ends, [q[:2] for q in poses], None, max_range2,
                           counters=None if counters is None else [counters])
    return want[0], st


def restate_numpy(geom, scans, poses, max_range2=H.DBL_MAX):
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    ends = [to_map_frame(np.asarray(s, np.float64).reshape(-1, 2), q).astype(np.float32) for s, q in zip(scans, poses)]
    want, st = H.integrate([geom], ends, [q[:2] for q in poses], None, max_range2)
    return want[0], st


def same_counts(grid, want):
    hit, pas = grid.counts()
    return np.array_equal(hit, want[0]) and np.array_equal(pas, want[1])


def grid_bytes(grid):
    return np.concatenate(grid.counts()).tobytes()


def views(ses, i):
    tp, tn, _ = ses.local_map(i)
    cp, cn = ses.submap_cloud(i)
    return device_cloud(tp, tn), device_cloud(cp, cn)


def stats_fields(st):
    return {f: int(getattr(st, f)) for f in STATS_FIELDS}


def table_b_moves_bytes(S):
    """What table B of a step gains with the archive: a fourth 24-byte move per session, the table's regions at multiples
    of 64 bytes (the moves' region starts at one)."""
    up = lambda v: (v + 63) // 64 * 64      # noqa: E731
    return up(4 * S * 24) - up(3 * S * 24)


def alternating_scan(n, phase=0.0):
    j = np.arange(n)
    r = np.where(j % 2 == 0, 3.0, 4.0)
    a = phase + 2.0 * np.pi * j / max(n, 1)
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=1).astype(np.float64)


def growths(lengths):
    """The growths of an archive that takes scans of these lengths behind its first allocation: a growth allocates
    max(2 x need, 1024) points."""
    cap, total, n = 0, 0, -1
    for m in lengths:
        total += m
        if cap == 0 or total > cap:
            cap, n = max(2 * total, 1024), n + 1
    return n
