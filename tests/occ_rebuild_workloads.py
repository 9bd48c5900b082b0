"""Crafted scan archives for ndt_sessions_occ_rebuild: the beam families of tests/test_gpu_occupancy.py, made reachable through
a session set (tests only, no GPU needed).

A session set created with space = space_thre = 0 archives every raw scan unchanged, a step with score_thre = -1 takes the
odometry and ndt_sessions_correct sets any trajectory, so a rebuild casts exactly the robot-frame points and poses named here;
the geometry is an argument of the rebuild, so one archive is cast into many grids.  A Session is a named archive:

  scans   raw robot-frame scans (float64 [n, 2]): the wanted float32 map-frame points through the inverse pose, in fp64
  poses   the pose of every scan (tx, ty, th[deg]); exact: every heading is one of 0, 90, 180, -90, where the numpy transform
          and the device's agree to the bit and the round trip gives back the wanted points (asserted below)
  start   the step of the set at which the session takes its first scan
  casts   the (Geometry, max_range2) pairs it is cast into; casts[0] is the one its own grid has in the sessions form

conditions(family) evaluates, on the reference alone (occ_helpers.classify / integrate), what makes a family what it claims
to be, and returns the values; tests/test_occ_rebuild_workloads_host.py asserts them.
"""
import math
from collections import namedtuple

import numpy as np

import occ_helpers as H
from ndt_slam_amd.pose_estimator import Pose2D
from session_helpers import to_map_frame

F = np.float32
EXACT_HEADINGS = (0.0, 90.0, 180.0, -90.0)
GENERIC_HEADING = 33.7
MAX_ROBOT_RANGE = 25.0

Session = namedtuple("Session", "name family scans poses start casts exact")

EXACT_GEOM = H.Geometry(0.0, 0.0, 0.25, 64, 48)
OFFSET_GEOM = H.Geometry(-1003.3, 707.1, 0.05, 64, 48)
BORDER_SHAPES = ((64, 48), (1, 1), (1, 37), (37, 1))
LEN_GEOM = H.Geometry(0.0, 0.0, 2.0 ** -14, 64, 8)             # 4 m are 65536 cells
INDEX_GEOM = H.Geometry(0.0, 0.0, 2.0 ** -28, 16, 16)          # 4 m are 2^30 cells
PREFIX_GEOM = H.Geometry(0.0, 0.0, 2.0 ** -6, 1200, 64)        # 1012 cells are 15.8 m
LONG_GEOM = H.Geometry(0.0, 0.0, 2.0 ** -8, 5400, 6)           # 5000 cells are 19.5 m
SIZES_GEOM = H.Geometry(0.0, 0.0, 0.25, 300, 300)
CIRCLE_GEOM = H.Geometry(-6.4, -6.4, 0.05, 256, 256)
ROUNDING_GEOM = H.Geometry(990.0, -710.0, 0.25, 80, 80)
PREFIX_TOTALS = (63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
SCAN_SIZES = (0, 1, 63, 64, 65, 0, 0, 255, 256, 257, 513, 1025, 0)      # empty at the front, in the middle, at the back
MANY_LATE = 5
# steps of the set -> the sessions named: 70 steps give 275 scans, one round boundary of the jobs kernel when all are named and
# none otherwise; 90 steps give 355, and every naming has the boundary in another row
MANY = {70: ([1, 1, 1, 1], [1, 0, 1, 1]), 90: ([1, 1, 1, 1], [1, 0, 1, 1], [1, 1, 0, 1])}
MANY_GEOMS = (H.Geometry(-12.0, -12.0, 0.25, 96, 96), H.Geometry(-10.0, -10.0, 0.125, 160, 160),
              H.Geometry(-1.0, -1.0, 0.25, 9, 7), H.Geometry(-12.05, -12.05, 0.05, 480, 480))
WORKGROUPS = (0, 1, 2, 5)


def centre(g, ix, iy):
    """The fp64 centre of cell (ix, iy) (arrays allowed) as float32 points [n, 2]."""
    ix, iy = np.asarray(ix, np.float64), np.asarray(iy, np.float64)
    return np.stack([g.x0 + (ix + 0.5) * g.res, g.y0 + (iy + 0.5) * g.res], axis=-1).astype(F).reshape(-1, 2)


def all_ends(g, ring=2):
    ix, iy = np.meshgrid(np.arange(-ring, g.nx + ring), np.arange(-ring, g.ny + ring))
    return centre(g, ix.ravel(), iy.ravel())


def to_robot(points, pose):
    """The inverse of session_helpers.to_map_frame in fp64: R^T (p - t), with the very cos / sin the forward transform uses."""
    R = Pose2D(*pose).Rmat
    p = np.asarray(points, np.float64).reshape(-1, 2)
    dx, dy = p[:, 0] - np.float64(pose[0]), p[:, 1] - np.float64(pose[1])
    return np.stack([R[0][0] * dx + R[1][0] * dy, R[0][1] * dx + R[1][1] * dy], axis=1)


def map_points(scan, pose):
    """The float32 map-frame points the rebuild's beams end in, by numpy."""
    return to_map_frame(np.asarray(scan, np.float64).reshape(-1, 2), np.asarray(pose, np.float64)).astype(F)


def aimed(wanted, pose):
    """The robot-frame scan whose float32 map-frame points at `pose` are `wanted` -- asserted by the round trip: an fp64
    transform is off by about 1e-13 m, a float32 point near 1000 m has neighbours 6e-5 m away."""
    wanted = np.asarray(wanted, F).reshape(-1, 2)
    scan = to_robot(wanted, pose)
    assert map_points(scan, pose).tobytes() == wanted.tobytes(), pose
    return scan


def _session(name, family, wanted, poses, casts, start=0):
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    assert len(wanted) == len(poses)
    scans = [aimed(w, q) for w, q in zip(wanted, poses)]
    return Session(name, family, scans, poses, start, list(casts), bool(np.isin(poses[:, 2], EXACT_HEADINGS).all()))


# ------------------------------------------------------------------------------------------ 1: octants
def _octants():
    out = []
    for tag, g in (("exact", EXACT_GEOM), ("offset", OFFSET_GEOM)):
        ends = all_ends(g)
        org = centre(g, 32, 24)[0].astype(np.float64)
        casts = [(g, H.DBL_MAX)]
        out.append(_session("octants-%s" % tag, "octants", [ends] * 4, [[org[0], org[1], h] for h in EXACT_HEADINGS], casts))
        out.append(_session("octants-%s-generic" % tag, "octants", [ends], [[org[0], org[1], GENERIC_HEADING]], casts))
    return out


def octant_conditions(g, origin, ends):
    """The counts of every tie and degenerate beam of one scan, per sign combination of (X1 - X0, Y1 - Y0)."""
    live, X1, Y1, X0, Y0 = H.classify(g, origin, ends)
    ddx, ddy = X1 - X0, Y1 - Y0
    dx, dy = np.abs(ddx), np.abs(ddy)
    L = np.maximum(dx, dy)
    out = {"all live": bool(live.all()), "L == 0": int((L == 0).sum()), "origin passes": int((L >= 1).sum())}
    for sx in (-1, 1):
        out["L == 1, sx %+d" % sx] = int(((L == 1) & (np.sign(ddx) == sx)).sum())
        out["horizontal, sx %+d" % sx] = int(((dy == 0) & (L > 1) & (np.sign(ddx) == sx)).sum())
        out["vertical, sy %+d" % sx] = int(((dx == 0) & (L > 1) & (np.sign(ddy) == sx)).sum())
        for sy in (-1, 1):
            q = (np.sign(ddx) == sx) & (np.sign(ddy) == sy)
            out["dx == dy > 1, %+d %+d" % (sx, sy)] = int(((dx == dy) & (L > 1) & q).sum())
            out["dx == dy + 1, %+d %+d" % (sx, sy)] = int(((dx == dy + 1) & q).sum())
            out["dy == dx + 1, %+d %+d" % (sx, sy)] = int(((dy == dx + 1) & q).sum())
    return out


# ------------------------------------------------------------------------------------------ 2: borders
def border_scans(shape):
    """The scans of test_borders_and_thin_grids for a grid of this shape, and three more origins: every side, two corners
    and the inside.  -> (geometry, scans, origin cells, the crossing and missing beams, their origin)."""
    g = H.Geometry(-1003.3, 707.1, 0.05, shape[0], shape[1])
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    ends = all_ends(g, ring=3)
    far = centre(g, rng.integers(-90, 160, size=400), rng.integers(-90, 140, size=400))
    j = np.arange(-2, 3)
    cross = centre(g, np.concatenate([shape[0] + 6 + j, -20 + j]), np.concatenate([shape[1] + 4 + j[::-1], -9 + j]))
    scans = [ends, far, np.concatenate([ends[::7], far]), far[::-1], cross, ends[::5], ends[::3], far[::2]]
    cells = [(-5, shape[1] + 9), (shape[0] + 40, -30), (shape[0] // 2, -70), (shape[0] // 2, shape[1] // 2), (-7, -5),
             (-9, shape[1] // 2), (shape[0] + 11, shape[1] // 2), (shape[0] // 2, shape[1] + 13)]
    return g, scans, cells, cross, cells[4]


def _borders():
    out = []
    for shape in BORDER_SHAPES:
        g, scans, cells, _, _ = border_scans(shape)
        poses = [list(centre(g, cx, cy)[0].astype(np.float64)) + [EXACT_HEADINGS[k % 4]] for k, (cx, cy) in enumerate(cells)]
        casts = [(g, H.DBL_MAX)]
        if shape == BORDER_SHAPES[0]:                   # the archive aimed at 64 x 48, into the thin grids as well
            casts += [(H.Geometry(g.x0, g.y0, g.res, s[0], s[1]), H.DBL_MAX) for s in BORDER_SHAPES[1:]]
        out.append(_session("borders-%dx%d" % shape, "borders", scans, poses, casts))
    return out


def border_conditions(shape):
    g, scans, cells, cross, oc = border_scans(shape)
    org = centre(g, *oc)[0].astype(np.float64)
    _, st_cross = H.integrate([g], [cross[:5]], [org])
    _, st_miss = H.integrate([g], [cross[5:]], [org])
    inside = [bool(0 <= cx < g.nx and 0 <= cy < g.ny) for cx, cy in cells]
    return {"crossing": H.stats_tuple(st_cross), "missing": H.stats_tuple(st_miss), "origins inside": inside}


# ------------------------------------------------------------------------------------------ 3: limits
E15, E14, E13 = 2.0 ** -15, 2.0 ** -14, 2.0 ** -13
LEN_ENDS = np.array([[4 + E15, E15], [4 + E14 + E15, E15], [E15 + E14 - 4, E15],
                     [E15, 4 + E15], [E15, 4 + E14 + E15], [4 + E15, 4 + E15]], np.float64)
LEN_LIVE = [True, False, True, True, False, True]             # L = 65536, 65537, 65535; the same upwards; the diagonal
INDEX_ENDS = np.array([[4.0, 0.0], [np.nextafter(F(4.0), F(8.0)), 0.0], [np.nextafter(F(4.0), F(0.0)), 0.0]], np.float64)
INDEX_CELLS = [1 << 30, (1 << 30) + 128, (1 << 30) - 64]
INDEX_LIVE = [True, False, True]
LIMIT_POSES = np.array([[E15, E15, 0.0], [4 - E13, 0.0, 0.0], [4.5, 0.0, 0.0]])      # (the last: the origin's cell is beyond 2^30)


def _limits():
    assert (LEN_ENDS.astype(F).astype(np.float64) == LEN_ENDS).all() and (INDEX_ENDS.astype(F).astype(np.float64) == INDEX_ENDS).all()
    return [_session("limits", "limits", [LEN_ENDS, INDEX_ENDS, INDEX_ENDS], LIMIT_POSES,
                     [(LEN_GEOM, H.DBL_MAX), (INDEX_GEOM, H.DBL_MAX)])]


def limit_conditions():
    s = by_name("limits")
    ends = [map_points(x, q) for x, q in zip(s.scans, s.poses)]
    live_len, _, _, X0, _ = H.classify(LEN_GEOM, s.poses[0][:2], ends[0])
    live_idx = H.classify(INDEX_GEOM, s.poses[1][:2], ends[1])[0]
    fx = np.floor(ends[1][:, 0].astype(np.float64) / INDEX_GEOM.res).astype(np.int64)
    return {"length live": live_len.tolist(), "length L on x": [int(abs(v - X0)) for v in H.cell_of(LEN_GEOM, ends[0][:3, 0], 0.0)[0]],
            "index live": live_idx.tolist(), "index cells": fx.tolist(),
            "origin beyond 2^30 live": H.classify(INDEX_GEOM, s.poses[2][:2], ends[2])[0].tolist()}


# ------------------------------------------------------------------------------------------ 4: range
def range_settings(s):
    """max_range2 at a squared length present among the session's beams (fp64 from the float32 end and the fp64 origin, as
    classify forms it), at the double just below it, and 0 -> ([three settings], beams at the value, beams with d2 > 0)."""
    d2 = []
    for x, q in zip(s.scans, s.poses):
        d = map_points(x, q).astype(np.float64) - q[:2]
        d2.append(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    d2 = np.sort(np.concatenate(d2))
    v = float(d2[len(d2) // 2])
    return [v, float(np.nextafter(v, 0.0)), 0.0], int((d2 == v).sum()), int((d2 > 0).sum())


def range_conditions():
    s = by_name("octants-exact")
    (v, below, zero), n_at, n_pos = range_settings(s)
    ends = [map_points(x, q) for x, q in zip(s.scans, s.poses)]
    skipped = [H.integrate([EXACT_GEOM], ends, [q[:2] for q in s.poses], None, r2)[1]["n_skipped"] for r2 in (v, below, zero)]
    return {"value": v, "beams at the value": n_at, "skipped": skipped, "beams with d2 > 0": n_pos}


# ------------------------------------------------------------------------------------------ 5: prefix
def _prefix():
    g, (ox, oy) = PREFIX_GEOM, (100, 32)
    pose = list(centre(g, ox, oy)[0].astype(np.float64)) + [0.0]
    runs = [centre(g, [ox + 2, ox - 2, ox, ox, ox + T - 13], [oy, oy, oy + 2, oy - 2, oy]) for T in PREFIX_TOTALS]
    runs += [np.repeat(centre(g, ox, oy), 256, axis=0), np.repeat(centre(g, ox, oy), 257, axis=0)]
    out = [_session("prefix-totals", "prefix", runs, [pose] * len(runs), [(g, H.DBL_MAX)])]
    # one beam with more items than all the others of its run together
    rng = np.random.default_rng(4)
    big = centre(LONG_GEOM, 200 + rng.integers(0, 4, size=256), 2 + rng.integers(-2, 3, size=256))
    big[100] = centre(LONG_GEOM, 200 + 5000, 3)[0]
    out.append(_session("prefix-long-beam", "prefix", [big], [list(centre(LONG_GEOM, 200, 2)[0].astype(np.float64)) + [0.0]],
                        [(LONG_GEOM, H.DBL_MAX)]))
    sized = [centre(SIZES_GEOM, 150 + rng.integers(-40, 41, size=n), 150 + rng.integers(-40, 41, size=n)) for n in SCAN_SIZES]
    poses = [[37.625, 37.625, EXACT_HEADINGS[k % 4]] for k in range(len(SCAN_SIZES))]
    out.append(_session("prefix-sizes", "prefix", sized, poses, [(SIZES_GEOM, H.DBL_MAX)]))
    return out


def items_of(g, origin, ends):
    """L + 1 of every live beam (0 for a skipped one)."""
    live, X1, Y1, X0, Y0 = H.classify(g, origin, ends)
    return np.where(live, np.maximum(np.abs(X1 - X0), np.abs(Y1 - Y0)) + 1, 0)


def prefix_conditions():
    s = by_name("prefix-totals")
    items = [items_of(PREFIX_GEOM, q[:2], map_points(x, q)) for x, q in zip(s.scans, s.poses)]
    b = by_name("prefix-long-beam")
    big = items_of(LONG_GEOM, b.poses[0][:2], map_points(b.scans[0], b.poses[0]))
    return {"totals": [int(x.sum()) for x in items], "beams": [x.tolist() for x in items[:len(PREFIX_TOTALS)]],
            "long beam": int(big[100]), "the rest of its run": int(big.sum() - big[100]),
            "scan sizes": [len(x) for x in by_name("prefix-sizes").scans]}


# ------------------------------------------------------------------------------------------ 6: contention
def _contention():
    a = np.arange(4096) * (2 * np.pi / 4096)
    r = np.where(np.arange(4096) % 64 == 0, 0.0, 5.0)                            # every 64th beam ends in the origin cell
    org = np.array([0.013, -0.021])
    ends = np.stack([org[0] + r * np.cos(a), org[1] + r * np.sin(a)], axis=1).astype(F)
    return [_session("contention", "contention", [ends], [[org[0], org[1], 0.0]], [(CIRCLE_GEOM, H.DBL_MAX)])]


def contention_conditions():
    s = by_name("contention")
    ends = map_points(s.scans[0], s.poses[0])
    want, _ = H.integrate([CIRCLE_GEOM], [ends], [s.poses[0][:2]])
    live, X1, Y1, X0, Y0 = H.classify(CIRCLE_GEOM, s.poses[0][:2], ends)
    L = np.maximum(np.abs(X1 - X0), np.abs(Y1 - Y0))
    return {"all live": bool(live.all()), "origin passes": int(want[0][1][Y0, X0]), "L >= 1": int((L >= 1).sum()),
            "origin hits": int(want[0][0][Y0, X0])}


# ------------------------------------------------------------------------------------------ 7: rounding
ROUNDING_POSE = np.array([1000.125, -700.125, 0.0])


def _rounding():
    """Map points 1e-6 .. 1e-5 m below a border of the 0.25 m grid, near 1000 m, where float32 numbers are 6.1e-5 m apart:
    the float32 point IS the border and lies in the next cell.  24 beams on x, 24 on y, 8 on both."""
    g, k = ROUNDING_GEOM, np.arange(24)
    below = 1e-6 * (1 + k % 10)
    bx, by = g.x0 + 0.25 * (44 + k), g.y0 + 0.25 * (28 + k)                      # borders (exact multiples of 0.25)
    cx, cy = g.x0 + 0.25 * (20.5 + 2 * k), g.y0 + 0.25 * (60.5 - 2 * k)          # cell centres
    pts = np.concatenate([np.stack([bx - below, cy], axis=1), np.stack([cx, by - below], axis=1),
                          np.stack([bx[:8] - below[:8], by[8:16] - below[:8]], axis=1)])
    scan = to_robot(pts, ROUNDING_POSE)                   # (NOT aimed(): the float32 point is not the fp64 one, on purpose)
    return [Session("rounding", "rounding", [scan], ROUNDING_POSE.reshape(1, 3), 0, [(ROUNDING_GEOM, H.DBL_MAX)], True)]


def rounding_cells():
    """-> (cells of the fp64 map points, cells of the float32 map points), (ix, iy) int64 arrays each."""
    s = by_name("rounding")
    m64 = to_map_frame(s.scans[0], s.poses[0])
    m32 = m64.astype(F).astype(np.float64)
    return H.cell_of(ROUNDING_GEOM, m64[:, 0], m64[:, 1]), H.cell_of(ROUNDING_GEOM, m32[:, 0], m32[:, 1])


# ------------------------------------------------------------------------------------------ the aimed set
_AIMED = None


def aimed_sessions():
    """The sessions of families 1 to 7, in the order of the set's rows."""
    global _AIMED
    if _AIMED is None:
        _AIMED = _octants() + _borders() + _limits() + _prefix() + _contention() + _rounding()
        for s in _AIMED:
            for x in s.scans:
                x.setflags(write=False)
    return _AIMED


def by_name(name):
    return next(s for s in aimed_sessions() if s.name == name)


def casts_of(s):
    """Every (tag, Geometry, max_range2) a session is cast with; the range family rides on the exact octants."""
    out = [("%dx%d@%g" % (g.nx, g.ny, g.res), g, r2) for g, r2 in s.casts]
    if s.name == "octants-exact":
        out += [("range-%s" % t, EXACT_GEOM, r2) for t, r2 in zip(("at", "below", "zero"), range_settings(s)[0])]
    return out


def aimed_cases():
    """(session name, cast tag) of every rebuild of the aimed set."""
    return [(s.name, tag) for s in aimed_sessions() for tag, _, _ in casts_of(s)]


def lockstep(sessions):
    """The steps of a set whose row i is sessions[i]: (scans, odo, active) per step; a session takes scan k at step
    start + k with the scan's pose as its odometry, and rests once its scans are used up."""
    n_steps = max(s.start + len(s.scans) for s in sessions)
    for k in range(n_steps):
        scans, odo, act = [], np.zeros((len(sessions), 3)), np.zeros(len(sessions), np.uint8)
        for i, s in enumerate(sessions):
            j = k - s.start
            if 0 <= j < len(s.scans):
                scans.append(s.scans[j]); odo[i] = s.poses[j]; act[i] = 1
            else:
                scans.append(np.zeros((0, 2)))
        yield scans, odo, act


# ------------------------------------------------------------------------------------------ 8: many scans
def many_sessions(steps=70):
    """Four sessions of one-to-three-beam scans over `steps` steps, session 2 five steps late.  70 steps: 275 scans, so that
    the jobs kernel's round of 256 scans ends inside the fourth session's rows when all are named."""
    rng = np.random.default_rng(steps + 8)
    out = []
    for i, g in enumerate(MANY_GEOMS):
        start = MANY_LATE if i == 2 else 0
        n = steps - start
        poses = np.stack([0.0625 * rng.integers(-16, 17, size=n), 0.0625 * rng.integers(-16, 17, size=n),
                          np.array(EXACT_HEADINGS)[rng.integers(0, 4, size=n)]], axis=1)
        wanted = [rng.uniform(-8.0, 8.0, size=(1 + (k + i) % 3, 2)).astype(F) for k in range(n)]
        out.append(_session("many-%d" % i, "many scans", wanted, poses, [(g, H.DBL_MAX)], start))
    return out


def many_conditions(steps):
    """Per naming: the scans named and the session whose rows hold scan 256, the first of the jobs kernel's second round
    (None: a single round)."""
    sessions = many_sessions(steps)
    lens = [len(s.scans) for s in sessions]
    named, row, starts = [], [], []
    for which in MANY[steps]:
        who = [i for i in range(4) if which[i]]
        first = np.concatenate([[0], np.cumsum([lens[i] for i in who])])
        named.append(int(first[-1])); starts.append(first[:-1].tolist())
        row.append(who[int(np.searchsorted(first, 256, side="right") - 1)] if first[-1] > 256 else None)
    return {"scans": lens, "scans named": named, "session of scan 256": row, "first scan of every row": starts,
            "beams": sorted({len(x) for s in sessions for x in s.scans})}


# ------------------------------------------------------------------------------------------ 9: dealing
DEAL_STAGES = (3, 4, 5, 6)                               # the runs session 2's archive holds when the set is rebuilt
DEAL_SUBSETS = ([1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1])


def dealing_sessions():
    """Archives of 1, 2 and (growing) 3 to 6 runs of 256 beams: one scan of 200 beams, one of 300, six of 100."""
    rng = np.random.default_rng(9)
    g = [H.Geometry(-8.0, -8.0, 0.25, 64, 64), H.Geometry(-8.0, -8.0, 0.125, 128, 128), H.Geometry(-6.0, -7.0, 0.25, 50, 60)]
    sizes = [[200], [300], [100] * 6]
    out = []
    for i in range(3):
        n = len(sizes[i])
        poses = np.stack([0.125 * rng.integers(-8, 9, size=n), 0.125 * rng.integers(-8, 9, size=n),
                          np.array(EXACT_HEADINGS)[rng.integers(0, 4, size=n)]], axis=1)
        wanted = [rng.uniform(-7.5, 7.5, size=(m, 2)).astype(F) for m in sizes[i]]
        out.append(_session("deal-%d" % i, "dealing", wanted, poses, [(g[i], H.DBL_MAX)]))
    return out


def deal_stride(n_runs, T):
    """The host's rule (ndt_sessions_occ_rebuild): about one session's runs, bumped until coprime -> (stride, bumps)."""
    stride = max(1, n_runs // T)
    bumps = 0
    while n_runs and math.gcd(stride, n_runs) != 1:
        stride += 1; bumps += 1
    return stride, bumps


def dealing_combinations():
    """(stage, subset, n_runs, T, stride, bumps) of every rebuild of the dealing set."""
    out = []
    for stage in DEAL_STAGES:
        runs = (1, 2, stage)
        for sub in DEAL_SUBSETS:
            n_runs, T = sum(r for r, w in zip(runs, sub) if w), sum(sub)
            out.append((stage, sub, n_runs, T) + deal_stride(n_runs, T))
    return out
