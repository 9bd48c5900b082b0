"""The numpy / plain-Python restatement of ndt_occ_* (include/ndt_mi355x.h; tests only).

cell_of       the cell of a coordinate: floor((x - x0) / res) in fp64 (numpy's subtraction and division round once each)
walk          the textbook all-octant integer Bresenham line as a loop, end cell excluded
closed_form   the visits by the header's formula: major start + s k, minor start + s floor((2 k m + L - 1) / (2 L))
integrate     hit and pass counters and the stats of a set of beams, by the rules of the header
render        100 hit / n rounded half up, -1 below min_obs
OccSessionsStandIn   session_helpers.OracleSessions with occ_grid / occ_integrate on the host
"""
from collections import namedtuple

import numpy as np

from ndt_slam_amd.capi import pack_scans as pack           # [scan] -> (packed float32 [N, 2], uint64 offsets)
from session_helpers import OracleSessions, to_map_frame

Geometry = namedtuple("Geometry", "x0 y0 res nx ny")
DBL_MAX = float(np.finfo(np.float64).max)
INDEX_MAX = 1 << 30
LEN_MAX = 65536
STATS = ("n_beams", "n_hit", "n_pass", "n_skipped")


def cell_of(g, x, y):
    """(ix, iy) as int64 arrays (or scalars) of fp64 coordinates: one subtraction, one division, floor."""
    with np.errstate(all="ignore"):
        fx = np.floor((np.asarray(x, np.float64) - np.float64(g.x0)) / np.float64(g.res))
        fy = np.floor((np.asarray(y, np.float64) - np.float64(g.y0)) / np.float64(g.res))
    lim = float(1 << 62)
    return np.clip(fx, -lim, lim).astype(np.int64), np.clip(fy, -lim, lim).astype(np.int64)


def walk(X0, Y0, X1, Y1):
    """Bresenham from (X0, Y0) to (X1, Y1), the end cell excluded -> (list of visited cells, where the last step arrived)."""
    dx, dy = abs(X1 - X0), abs(Y1 - Y0)
    sx, sy = (X1 > X0) - (X1 < X0), (Y1 > Y0) - (Y1 < Y0)
    x, y, out = X0, Y0, []
    if dx >= dy:
        e = 2 * dy - dx
        for _ in range(dx):
            out.append((x, y))
            if e > 0:
                y += sy
                e -= 2 * dx
            e += 2 * dy
            x += sx
    else:
        e = 2 * dx - dy
        for _ in range(dy):
            out.append((x, y))
            if e > 0:
                x += sx
                e -= 2 * dy
            e += 2 * dx
            y += sy
    return out, (x, y)


def closed_form(X0, Y0, X1, Y1):
    """The visits k = 0 .. L - 1 by the closed form -> (xs, ys) int64 arrays."""
    dx, dy = abs(X1 - X0), abs(Y1 - Y0)
    sx, sy = (X1 > X0) - (X1 < X0), (Y1 > Y0) - (Y1 < Y0)
    L, m = max(dx, dy), min(dx, dy)
    k = np.arange(L, dtype=np.int64)
    if L == 0:
        return k, k.copy()
    minor = (2 * k * m + L - 1) // (2 * L)
    if dx >= dy:
        return X0 + sx * k, Y0 + sy * minor
    return X0 + sx * minor, Y0 + sy * k


def classify(g, origin, ends, max_range2=DBL_MAX):
    """Per beam: live (bool), X1, Y1, and the origin's cell (X0, Y0) -- the skip rules of the header, in their order."""
    ends = np.asarray(ends, np.float32).reshape(-1, 2)
    ox, oy = np.float64(origin[0]), np.float64(origin[1])
    ex, ey = ends[:, 0].astype(np.float64), ends[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        live = np.isfinite(ex) & np.isfinite(ey) & bool(np.isfinite(ox) and np.isfinite(oy))
        dx, dy = ex - ox, ey - oy
        d2 = dx * dx + dy * dy
        live &= ~(d2 > np.float64(max_range2))
        fx1, fy1 = np.floor((ex - np.float64(g.x0)) / np.float64(g.res)), np.floor((ey - np.float64(g.y0)) / np.float64(g.res))
        fx0, fy0 = np.floor((ox - np.float64(g.x0)) / np.float64(g.res)), np.floor((oy - np.float64(g.y0)) / np.float64(g.res))
        for f in (fx1, fy1):
            live &= (f >= -INDEX_MAX) & (f <= INDEX_MAX)
        org_ok = bool(-INDEX_MAX <= fx0 <= INDEX_MAX and -INDEX_MAX <= fy0 <= INDEX_MAX)
        live &= org_ok
    X0, Y0 = (int(fx0), int(fy0)) if org_ok and np.isfinite(ox) and np.isfinite(oy) else (0, 0)
    X1 = np.where(live, fx1, 0).astype(np.int64)
    Y1 = np.where(live, fy1, 0).astype(np.int64)
    L = np.maximum(np.abs(X1 - X0), np.abs(Y1 - Y0))
    live &= L <= LEN_MAX
    return live, X1, Y1, X0, Y0


def integrate(geoms, scans, origins, grid_of=None, max_range2=DBL_MAX, counters=None):
    """Scans (float32 [n, 2] each) from origins[b][:2] into grid grid_of[b] (None: all into grid 0) ->
    (list of (hit, pass) uint32 [ny, nx] pairs, stats dict).  `counters`: pairs to add to instead of zeros (modified)."""
    if counters is None:
        counters = [(np.zeros((g.ny, g.nx), np.uint32), np.zeros((g.ny, g.nx), np.uint32)) for g in geoms]
    st = dict.fromkeys(STATS, 0)
    for b, scan in enumerate(scans):
        scan = np.asarray(scan, np.float32).reshape(-1, 2)
        st["n_beams"] += len(scan)
        gi = 0 if grid_of is None else int(grid_of[b])
        if gi < 0 or gi >= len(geoms):
            st["n_skipped"] += len(scan)
            continue
        g = geoms[gi]
        hit, pas = counters[gi]
        live, X1, Y1, X0, Y0 = classify(g, origins[b], scan, max_range2)
        st["n_skipped"] += int((~live).sum())
        for i in np.nonzero(live)[0]:
            x1, y1 = int(X1[i]), int(Y1[i])
            xs, ys = closed_form(X0, Y0, x1, y1)
            ins = (xs >= 0) & (xs < g.nx) & (ys >= 0) & (ys < g.ny)
            np.add.at(pas, (ys[ins], xs[ins]), np.uint32(1))
            st["n_pass"] += int(ins.sum())
            if 0 <= x1 < g.nx and 0 <= y1 < g.ny:
                hit[y1, x1] += np.uint32(1)
                st["n_hit"] += 1
    return counters, st


def render(hit, pas, min_obs=1):
    n = hit.astype(np.uint64) + pas.astype(np.uint64)
    v = (200 * hit.astype(np.uint64) + n) // np.maximum(2 * n, 1)
    return np.where(n < min_obs, -1, v.astype(np.int64)).astype(np.int8)


def stats_tuple(st):
    """A stats dict or a numpy OCC_STATS_DTYPE record as a tuple of ints."""
    return tuple(int(st[k]) for k in STATS)


def add_stats(a, b):
    return {k: int(a[k]) + int(b[k]) for k in STATS}


class HostGrid:
    """What capi.OccGrid is to run_sessions_resident, on the host."""

    def __init__(self, geometry):
        self.geometry = Geometry(geometry.x0, geometry.y0, geometry.res, geometry.nx, geometry.ny)
        self.hit = np.zeros((geometry.ny, geometry.nx), np.uint32)
        self.pas = np.zeros((geometry.ny, geometry.nx), np.uint32)
        self.closed = False

    def render(self, min_obs=1):
        return render(self.hit, self.pas, min_obs)

    def close(self):
        self.closed = True


class OccSessionsStandIn(OracleSessions):
    """OracleSessions that keeps every session's newest map-frame scan (float32, as the device stores it) and pose, with
    capi.Sessions.occ_integrate on the host; `beams` records (session, origin, scan) of everything integrated."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.newest = [None] * self.n
        self.beams = []

    def step(self, scans, odo, active=None):
        out = super().step(scans, odo, active)
        for i in range(self.n):
            if out[i]["stepped"]:
                lps = self._resampled(scans[i])
                pose = np.array(out[i]["pose"], np.float64)
                self.newest[i] = (pose[:2].copy(), to_map_frame(lps, pose).astype(np.float32))
        return out

    def _resampled(self, raw):
        from ndt_slam_amd import replay
        return replay.resample_points(np.asarray(raw, np.float64).reshape(-1, 2), self.p["space"], self.p["space_thre"])

    def occ_grid(self, geometry):
        return HostGrid(geometry)

    def occ_integrate(self, grids, which=None, max_range2=DBL_MAX):
        total = dict.fromkeys(STATS, 0)
        for i in range(self.n):
            if (which is not None and not which[i]) or self.newest[i] is None:
                continue
            org, scan = self.newest[i]
            g = grids[i]
            _, st = integrate([g.geometry], [scan], [org], None, max_range2, counters=[(g.hit, g.pas)])
            self.beams.append((i, org, scan))
            total = add_stats(total, st)
        return total


def beam_to_cell(g, ix, iy, fx=0.5, fy=0.5):
    """A float32 point inside cell (ix, iy) at the given fractions (for geometries whose arithmetic is exact)."""
    return np.float32(g.x0 + (ix + fx) * g.res), np.float32(g.y0 + (iy + fy) * g.res)
