"""ndt_occ_* without a device: the declared surface, the layouts, the NULL-context refusal from pedantic C99, ndt_occ_cell
against the numpy restatement (tests/occ_helpers.py), the loop Bresenham against the closed form, map_server's files, and
replay.run_sessions_resident(occupancy=...) over a host stand-in."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import occ_helpers as H
from ndt_slam_amd import replay, synth
from replay_helpers import OracleOps  # noqa: F401  (the stand-in's operations)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ndt_occ_cell", "ndt_occ_create", "ndt_occ_destroy", "ndt_occ_clear", "ndt_occ_geometry_get", "ndt_occ_view",
         "ndt_occ_integrate_dev", "ndt_occ_integrate", "ndt_occ_render_dev", "ndt_occ_render", "ndt_occ_counts",
         "ndt_sessions_occ_integrate")


@pytest.fixture(scope="module")
def capi():
    from ndt_slam_amd import build, capi
    build.build()
    return capi


# ------------------------------------------------------------------------------------------ the surface
def test_header_declares_library_exports_and_binding_lists_every_name(capi):
    src = open(os.path.join(ROOT, "include", "ndt_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    for t in ("ndt_occ_geometry", "ndt_occ_stats"):
        assert "typedef struct %s" % t in code
    for name in ("OccGeometry", "OccStats", "OCC_STATS_DTYPE", "OccGrid", "integrate_occ"):
        assert hasattr(capi, name), name
    for m in ("integrate", "integrate_dev", "render", "counts", "clear", "close"):
        assert callable(getattr(capi.OccGrid, m)), m
    assert callable(capi.Sessions.occ_integrate)


def test_layouts(capi):
    G, S = capi.OccGeometry, capi.OccStats
    assert ctypes.sizeof(S) == 32 and ctypes.sizeof(G) == 32
    assert [(n, getattr(G, n).offset) for n, _ in G._fields_] == [("x0", 0), ("y0", 8), ("res", 16), ("nx", 24), ("ny", 28)]
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("n_beams", 0), ("n_hit", 8), ("n_pass", 16), ("n_skipped", 24)]
    dt = capi.OCC_STATS_DTYPE
    assert dt.itemsize == 32 and dt.names == H.STATS and [dt.fields[n][1] for n in dt.names] == [0, 8, 16, 24]


C99 = r"""
#include <float.h>
#include <stdio.h>
#include <string.h>
#include "ndt_mi355x.h"
int main(void) {
  float xy[2] = {0.f, 0.f};
  double org[2] = {0.0, 0.0};
  uint64_t off[2] = {0, 1};
  ndt_occ_geometry g;
  ndt_occ_stats st;
  ndt_occ *occ = (ndt_occ *)&g, *list[1];
  int64_t ix = 0, iy = 0;
  int rc;
  g.x0 = -1.0; g.y0 = -1.0; g.res = 0.25; g.nx = 8; g.ny = 8;
  list[0] = NULL;
  memset(&st, 0x5a, sizeof st);
  if (sizeof(ndt_occ_stats) != 32 || sizeof(ndt_occ_geometry) != 32) return 10;
  rc = ndt_occ_integrate(NULL, list, 1, NULL, xy, off, 1, org, sizeof org, DBL_MAX, &st);
  if (rc != NDT_E_ARG || strcmp(ndt_last_error(NULL), "null context") != 0) return 11;
  rc = ndt_occ_create(NULL, &g, &occ);
  if (rc != NDT_E_ARG || strcmp(ndt_last_error(NULL), "null context") != 0) return 12;
  if (occ != (ndt_occ *)&g || st.n_beams != 0x5a5a5a5a5a5a5a5aull || st.n_skipped != 0x5a5a5a5a5a5a5a5aull) return 13;
  rc = ndt_occ_integrate_dev(NULL, list, 1, NULL, xy, off, 1, 1, org, sizeof org, DBL_MAX, &st, NULL);
  if (rc != NDT_E_ARG || strcmp(ndt_last_error(NULL), "null context") != 0) return 14;
  if (ndt_occ_cell(&g, 0.3, -0.8, &ix, &iy) != NDT_OK || ix != 5 || iy != 0) return 15;
  puts("ok");
  return 0;
}
"""


def test_pedantic_c99_compiles_the_header_and_a_null_context_is_refused(capi, tmp_path):
    src, exe = tmp_path / "occ_c99.c", tmp_path / "occ_c99"
    src.write_text(C99)
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["cc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", libdir, "-l:" + os.path.basename(capi.LIB_PATH), "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout)


# ------------------------------------------------------------------------------------------ the cell of a point
def _cells(capi, g, xs, ys):
    L = capi.lib()
    G = capi.OccGeometry(*g)
    ix, iy = ctypes.c_int64(), ctypes.c_int64()
    out = np.zeros((len(xs), 2), np.int64)
    for k in range(len(xs)):
        assert L.ndt_occ_cell(ctypes.byref(G), float(xs[k]), float(ys[k]), ctypes.byref(ix), ctypes.byref(iy)) == 0
        out[k] = ix.value, iy.value
    return out


@pytest.mark.parametrize("res", [0.25, 0.05])
@pytest.mark.parametrize("origin", [(0.0, 0.0), (-1003.3, 707.1), (8191.7, 8191.7)])
def test_occ_cell_is_the_restatement(capi, res, origin):
    """10^5 points over the 2 x 3 geometries: random ones (both signs), float32 values widened (what a scan holds), points
    exactly on cell edges as fp64 forms them (x0 + i res) and their two fp64 neighbours."""
    g = H.Geometry(origin[0], origin[1], res, 640, 480)
    rng = np.random.default_rng(int(res * 1000) + int(abs(origin[0])))
    n = 100000 // 6
    a, f = n // 5, n // 10
    i = rng.integers(-2000, 2000, size=(a, 2))
    edge = np.array(origin) + i * res
    pts = np.concatenate([
        np.array(origin) + rng.uniform(-120.0, 120.0, size=(a, 2)),
        (np.array(origin) + rng.uniform(-120.0, 120.0, size=(f, 2))).astype(np.float32).astype(np.float64),
        edge, np.nextafter(edge, -np.inf), np.nextafter(edge, np.inf),
        -rng.uniform(0.0, 30.0, size=(n - 4 * a - f, 2)),
    ])
    assert len(pts) == n
    got = _cells(capi, g, pts[:, 0], pts[:, 1])
    ex, ey = H.cell_of(g, pts[:, 0], pts[:, 1])
    assert np.array_equal(got[:, 0], ex) and np.array_equal(got[:, 1], ey)
    if res == 0.25 and origin == (0.0, 0.0):         # exact arithmetic: an edge point is the first point of its cell
        assert np.array_equal(got[a + f:2 * a + f], i)


def test_occ_cell_and_geometry_refusals(capi):
    L = capi.lib()
    ix, iy = ctypes.c_int64(7), ctypes.c_int64(7)

    def rc(g, x=0.0, y=0.0):
        G = capi.OccGeometry(*g)
        return L.ndt_occ_cell(ctypes.byref(G), x, y, ctypes.byref(ix), ctypes.byref(iy))
    ok = (0.0, 0.0, 0.05, 10, 10)
    assert rc(ok) == 0
    for bad in ((0.0, 0.0, 0.0, 10, 10), (0.0, 0.0, -0.05, 10, 10), (0.0, 0.0, np.inf, 10, 10), (0.0, 0.0, np.nan, 10, 10),
                (np.nan, 0.0, 0.05, 10, 10), (0.0, np.inf, 0.05, 10, 10), (0.0, 0.0, 0.05, 0, 10), (0.0, 0.0, 0.05, 10, -1)):
        ix.value = iy.value = 7
        assert rc(bad) == -1, bad
        assert ix.value == 7 and iy.value == 7
    assert rc((0.0, 0.0, 0.05, 1 << 14, 1 << 14)) == 0                     # 2^28 cells: the limit itself
    assert rc((0.0, 0.0, 0.05, (1 << 14) + 1, 1 << 14)) == -4               # NDT_E_GRID
    assert rc(ok, np.nan, 0.0) == -1 and rc(ok, 0.0, np.inf) == -1
    assert L.ndt_occ_cell(None, 0.0, 0.0, ctypes.byref(ix), ctypes.byref(iy)) == -1


# ------------------------------------------------------------------------------------------ the walk
def _same_walk(X0, Y0, X1, Y1):
    cells, arrived = H.walk(X0, Y0, X1, Y1)
    xs, ys = H.closed_form(X0, Y0, X1, Y1)
    L = max(abs(X1 - X0), abs(Y1 - Y0))
    assert len(cells) == L == len(xs)
    assert arrived == (X1, Y1)
    assert (X1, Y1) not in cells or L == 0
    assert cells == list(zip(xs.tolist(), ys.tolist()))


def test_loop_walk_equals_closed_form_for_every_end_cell_nearby():
    for X1 in range(-40, 41):
        for Y1 in range(-40, 41):
            _same_walk(0, 0, X1, Y1)
    _same_walk(5, -7, 5, -7)
    _same_walk(-3, 11, 9, 2)


def test_loop_walk_equals_closed_form_on_long_random_beams():
    rng = np.random.default_rng(19)
    ends = [(65536, 0), (0, -65536), (65536, 65536), (-65536, 65535), (65535, -65536), (65536, 1), (1, 65536), (-65536, 32768)]
    for _ in range(24):
        L = int(rng.integers(3000, 65537))
        m = int(rng.integers(0, L + 1))
        sx, sy = rng.choice([-1, 1], size=2)
        ends.append((int(sx) * L, int(sy) * m) if rng.integers(2) else (int(sx) * m, int(sy) * L))
    for X1, Y1 in ends:
        X0, Y0 = (int(v) for v in rng.integers(-3000, 3000, size=2))
        _same_walk(X0, Y0, X0 + X1, Y0 + Y1)


def test_restatement_on_hand_made_beams():
    g = H.Geometry(0.0, 0.0, 1.0, 4, 3)
    scan = np.array([[3.5, 0.5], [0.5, 0.5], [9.5, 0.5], [np.nan, 0.0], [2.5, 2.5]], np.float32)
    (c,), st = H.integrate([g], [scan], [(0.5, 0.5)])
    hit, pas = c
    # (3,0): pass 0,1,2; (0,0): a hit only; (9,0): pass 0..3 inside, the hit outside; NaN skipped; (2,2): x-major diagonal
    assert hit.tolist() == [[1, 0, 0, 1], [0, 0, 0, 0], [0, 0, 1, 0]]
    assert pas.tolist() == [[3, 2, 2, 1], [0, 1, 0, 0], [0, 0, 0, 0]]
    assert H.stats_tuple(st) == (5, 3, 9, 1)
    assert H.render(hit, pas, 1).tolist() == [[25, 0, 0, 50], [-1, 0, -1, -1], [-1, -1, 100, -1]]
    assert H.render(hit, pas, 3).tolist() == [[25, -1, -1, -1], [-1, -1, -1, -1], [-1, -1, -1, -1]]
    # the range cut is `>` on the squared length; a scan whose grid_of is out of range is skipped whole
    _, st = H.integrate([g], [scan[:1]], [(0.5, 0.5)], max_range2=9.0)
    assert H.stats_tuple(st) == (1, 1, 3, 0)
    _, st = H.integrate([g], [scan[:1]], [(0.5, 0.5)], max_range2=float(np.nextafter(9.0, 0.0)))
    assert H.stats_tuple(st) == (1, 0, 0, 1)
    _, st = H.integrate([g], [scan, scan], [(0.5, 0.5)] * 2, grid_of=[-1, 1])
    assert H.stats_tuple(st) == (10, 0, 0, 10)


# ------------------------------------------------------------------------------------------ map_server's files
def test_save_and_load_occupancy_round_trip_and_pixel_rule(tmp_path):
    g = H.Geometry(-1003.3, 707.1, 0.05, 7, 3)
    v = np.array([[-1, 0, 19, 20, 64, 65, 66],
                  [100, 50, -1, 1, 99, 19, 20],
                  [65, 66, 0, -1, 20, 19, 100]], np.int8)
    replay.save_occupancy(tmp_path / "m", v, g)
    raw = open(tmp_path / "m.pgm", "rb").read()
    assert raw.startswith(b"P5\n7 3\n255\n") and len(raw) == len(b"P5\n7 3\n255\n") + 21
    pix, meta = replay.load_occupancy(tmp_path / "m")
    # 19 / 100 < 0.196 is free, 20 / 100 is not; 65 / 100 > 0.65 is false, 66 / 100 is occupied; unknown is 205
    exp = np.array([[205, 254, 254, 205, 205, 205, 0],
                    [0, 205, 205, 254, 0, 254, 205],
                    [205, 0, 254, 205, 205, 254, 0]], np.uint8)
    assert np.array_equal(pix, exp)
    # row 0 of the file is the largest y
    assert np.frombuffer(raw[-21:], np.uint8).reshape(3, 7)[0].tolist() == exp[2].tolist()
    assert meta == {"image": "m.pgm", "resolution": 0.05, "origin": [-1003.3, 707.1, 0.0], "negate": 0, "occupied_thresh": 0.65,
                    "free_thresh": 0.196}
    # thresholds given: values exactly at them fall in the middle class
    replay.save_occupancy(tmp_path / "t", np.array([[50, 51, 25, 24]], np.int8), g, occupied_thresh=0.5, free_thresh=0.25)
    pix, meta = replay.load_occupancy(tmp_path / "t")
    assert pix.tolist() == [[205, 0, 205, 254]] and meta["occupied_thresh"] == 0.5 and meta["free_thresh"] == 0.25


# ------------------------------------------------------------------------------------------ the replay driver
def _logs(tmp_path):
    logs = []
    for i, (seed, n) in enumerate(((33, 7), (41, 5))):
        recs, _ = synth.replay_records(n_frames=n, n_beams=121, step=0.6, seed=seed)
        replay.write_log(tmp_path / ("log%d.txt" % i), recs)
        logs.append(tmp_path / ("log%d.txt" % i))
    return logs


def test_resident_driver_writes_the_occupancy_of_every_step_and_none_changes_nothing(oracle, tmp_path, capi):
    logs = _logs(tmp_path)
    p = dict(replay.LAUNCH_PARAMS, end_frame=20, sepThre=4.0, start_frame=1)
    geoms = [H.Geometry(-20.0, -20.0, 0.25, 160, 160), H.Geometry(-15.05, -15.05, 0.1, 301, 299)]

    def run(tag, **kw):
        ses = H.OccSessionsStandIn(oracle, capi, 2, p, arith="replay")
        poses = replay.run_sessions_resident(None, [replay.read_log(l, sidelidar=False) for l in logs],
                                             poses_names=[tmp_path / ("%s%d.txt" % (tag, i)) for i in range(2)],
                                             map_names=[str(tmp_path / ("%s%d.pcd" % (tag, i))) for i in range(2)], sessions=ses, **p,
                                             **kw)
        return ses, poses
    _, base = run("base")
    ses_none, none = run("none", occupancy=None)
    ses, occ = run("occ", occupancy=geoms, occupancy_names=[tmp_path / "occ0", None])
    assert not ses_none.beams and len(ses.beams) == 6 + 4                       # one scan per session and step taken
    for tag in ("none", "occ"):
        for i in range(2):
            for ext in (".txt", ".pcd", ".pcd_sep0.pcd"):
                assert open(tmp_path / ("%s%d%s" % (tag, i, ext)), "rb").read() == open(tmp_path / ("base%d%s" % (i, ext)), "rb").read()
    for a, b in zip(base, occ):
        assert [(q.tx, q.ty, q.th) for q in a] == [(q.tx, q.ty, q.th) for q in b]
    # the file of session 0 is the helper's render of the same beams; session 1 asked for no file
    mine = [b for b in ses.beams if b[0] == 0]
    (c,), st = H.integrate([geoms[0]], [b[2] for b in mine], [b[1] for b in mine])
    assert st["n_hit"] > 300 and st["n_pass"] > 10 * st["n_hit"]
    replay.save_occupancy(tmp_path / "expect", H.render(c[0], c[1], 1), geoms[0])
    assert open(tmp_path / "occ0.pgm", "rb").read() == open(tmp_path / "expect.pgm", "rb").read()
    pix, meta = replay.load_occupancy(tmp_path / "occ0")
    assert meta["resolution"] == 0.25 and meta["origin"] == [-20.0, -20.0, 0.0] and set(np.unique(pix)) == {0, 205, 254}
    assert not os.path.exists(tmp_path / "occ1.pgm")
    # one geometry for all logs is accepted as well; a list of the wrong length is not
    run("one", occupancy=geoms[0])
    with pytest.raises(ValueError):
        run("bad", occupancy=geoms[:1] * 3)
