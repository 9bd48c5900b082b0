"""Relocalisation without a GPU: the lattice's host functions, the numpy reference of the candidate pick, and the whole
coarse-to-fine chain on the CPU oracle (the prototype the device path is held to in tests/test_gpu_reloc.py)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from reloc_helpers import (LAT, crafted_volumes, edge_poses, lattice_poses, lattice_size, oracle_scores, pose_error, ref_best,
                           ref_select, relocalize_ref)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ndt_lattice_size", "ndt_lattice_pose", "ndt_score_poses", "ndt_score_poses_dev", "ndt_score_lattice_dev",
       "ndt_lattice_select_dev", "ndt_relocalize", "ndt_relocalize_dev")


@pytest.fixture(scope="module")
def capi():
    from ndt_slam_amd import build, capi
    build.build()
    return capi


def test_header_declares_and_library_exports_the_new_names(capi):
    src = open(os.path.join(ROOT, "include", "ndt_mi355x.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(ndt_[a-z_0-9]+)\s*\(", src))
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in capi.EXPORTS, name
    assert "ndt_pose_lattice" in src and "ndt_reloc_params" in src
    assert ctypes.sizeof(capi.PoseLattice) == 64 and ctypes.sizeof(capi.RelocParams) == 72


LATTICES = [
    dict(LAT),
    dict(x0=0.1, y0=-7.3, yaw0=0.7, step_x=0.37, step_y=1e-3, step_yaw=0.01, nx=1, ny=211, nyaw=97),          # a dimension of 1
    dict(x0=1e3 / 3, y0=5.0, yaw0=math.pi, step_x=-0.1, step_y=-1.0 / 3, step_yaw=-math.pi / 180, nx=301, ny=57, nyaw=360),
]


@pytest.mark.parametrize("lat", LATTICES, ids=["LAT", "dim1", "negative_steps"])
def test_lattice_pose_is_origin_plus_index_times_step_bit_for_bit(capi, lat):
    L = capi.PoseLattice(lat["x0"], lat["y0"], lat["yaw0"], lat["step_x"], lat["step_y"], lat["step_yaw"], lat["nx"], lat["ny"],
                         lat["nyaw"])
    n = lattice_size(lat)
    assert L.size == n
    rng = np.random.default_rng(11)
    idx = np.concatenate([[0, n - 1], rng.integers(0, n, 998)])
    got = L.poses(idx)
    want = lattice_poses(lat, idx)
    assert got.tobytes() == want.tobytes()
    # yaw-major, x fastest
    if lat["nx"] > 1:
        assert L.pose(1)[0] == lat["x0"] + 1.0 * lat["step_x"] and L.pose(1)[1] == lat["y0"]
    assert L.pose(lat["nx"])[1] == lat["y0"] + 1.0 * lat["step_y"]
    assert L.pose(lat["nx"] * lat["ny"])[2] == lat["yaw0"] + 1.0 * lat["step_yaw"]


def test_lattice_refusals(capi):
    lib = capi.lib()
    n = ctypes.c_uint64(77)
    p = (ctypes.c_double * 3)()
    good = capi.PoseLattice(0, 0, 0, 1, 1, 1, 2, 3, 4)
    assert lib.ndt_lattice_size(ctypes.byref(good), ctypes.byref(n)) == capi.NDT_OK and n.value == 24
    assert lib.ndt_lattice_pose(ctypes.byref(good), 23, p) == capi.NDT_OK
    assert lib.ndt_lattice_size(None, ctypes.byref(n)) == capi.NDT_E_ARG
    assert lib.ndt_lattice_size(ctypes.byref(good), None) == capi.NDT_E_ARG
    assert lib.ndt_lattice_pose(None, 0, p) == capi.NDT_E_ARG
    assert lib.ndt_lattice_pose(ctypes.byref(good), 0, None) == capi.NDT_E_ARG
    assert lib.ndt_lattice_pose(ctypes.byref(good), 24, p) == capi.NDT_E_ARG                 # index out of range
    assert lib.ndt_lattice_pose(ctypes.byref(good), 2 ** 40, p) == capi.NDT_E_ARG
    bad = []
    for field in ("nx", "ny", "nyaw"):
        for v in (0, -1):
            bad.append({field: v})
    for field in ("x0", "y0", "yaw0", "step_x", "step_y", "step_yaw"):
        for v in (float("nan"), float("inf"), -float("inf")):
            bad.append({field: v})
    bad += [dict(nx=65536, ny=32768, nyaw=1),                  # 2^31: one too many
            dict(nx=2 ** 31 - 1, ny=2, nyaw=1), dict(nx=2 ** 30, ny=2 ** 30, nyaw=2 ** 30), dict(nx=46341, ny=46341, nyaw=1)]
    for kw in bad:
        L = capi.PoseLattice(0, 0, 0, 1, 1, 1, 2, 3, 4)
        for k, v in kw.items():
            setattr(L, k, v)
        n.value = 77
        assert lib.ndt_lattice_size(ctypes.byref(L), ctypes.byref(n)) == capi.NDT_E_ARG, kw
        assert n.value == 77                                   # nothing written
        assert lib.ndt_lattice_pose(ctypes.byref(L), 0, p) == capi.NDT_E_ARG, kw
    # the largest lattice there is
    L = capi.PoseLattice(0, 0, 0, 1, 1, 1, 2 ** 31 - 1, 1, 1)
    assert lib.ndt_lattice_size(ctypes.byref(L), ctypes.byref(n)) == capi.NDT_OK and n.value == 2 ** 31 - 1
    assert lib.ndt_lattice_pose(ctypes.byref(L), 2 ** 31 - 2, p) == capi.NDT_OK and p[0] == float(2 ** 31 - 2)


# ------------------------------------------------------------------------------------------ the reference pick
def volume(name):
    return next(v for v in crafted_volumes() if v[0] == name)


def test_pick_all_equal_volume_gives_exactly_index_zero():
    _, dims, s, p = volume("all_equal")
    assert ref_select(s, p, dims, 16, True).tolist() == [0]
    assert ref_select(s, p, dims, 4, False).tolist() == [0, 1, 2, 3]          # without the local-maximum rule: ties by index


def test_pick_plateau_yields_its_lowest_index():
    _, dims, s, p = volume("plateau2")
    # (the zero background is a plateau of its own, cut in two by nothing: it yields its lowest index, 0)
    assert ref_select(s, p, dims, 16, True).tolist() == [40, 0]
    assert ref_select(s, p, dims, 2, False).tolist() == [40, 41]


def test_pick_maxima_on_faces_and_corners_and_top_k_beyond_their_number():
    _, dims, s, p = volume("faces_corners")
    peaks = [0, 6, 28, 34, 70, 76, 98, 104, 3, 52, 14]
    got = ref_select(s, p, dims, 1024, True).tolist()
    assert got[:len(peaks)] == sorted(peaks, reverse=True)               # their scores are 5 + index
    assert len(got) < 7 * 5 * 3 and len(set(got)) == len(got)
    assert ref_select(s, p, dims, 3, True).tolist() == [104, 98, 76]


def test_pick_degenerate_lattices():
    _, dims, s, p = volume("one")
    assert ref_select(s, p, dims, 5, True).tolist() == [0]
    _, dims, s, p = volume("one_empty")
    assert ref_select(s, p, dims, 5, True).tolist() == []
    for name in ("line_x", "line_y", "line_yaw"):
        _, dims, s, p = volume(name)
        got = ref_select(s, p, dims, 3, True).tolist()
        assert got == [13, 0, 39], name                                   # 4.0 (plateau 13, 14 -> 13), 3.0 at one end, 2.0 at the other


def test_pick_never_takes_a_pose_without_pairs():
    _, dims, s, p = volume("pairs_zero")
    for lm in (False, True):
        got = ref_select(s, p, dims, 1024, lm)
        assert (p[got.astype(np.int64)] > 0).all()
    order = np.argsort(-s)
    assert ref_select(s, p, dims, 3, False).tolist() == [order[1], order[3], order[5]]
    _, dims, s, p = volume("none_eligible")
    assert len(ref_select(s, p, dims, 16, False)) == 0


# ------------------------------------------------------------------------------------------ the prototype, on the oracle
@pytest.fixture(scope="module")
def world(oracle, c1_world):
    m, sf, cfg = c1_world
    return oracle.Map(m, oracle.default_params(resolution=cfg["resolution"])), sf


@pytest.mark.parametrize("k", [0, 2, 6])
def test_coarse_to_fine_recovers_the_pose_on_the_oracle(oracle, world, k):
    """Sweep LAT, refine the 16 best local maxima, take the lowest cost: within 0.05 m / 0.002 rad of the truth (measured on
    the oracle: 0.0231 m / 7.4e-4 rad at worst).  For scans 2 and 6 the winner is not the best-scoring candidate."""
    om, sf = world
    scan, truth, _ = sf.make(k)
    out = relocalize_ref(oracle, om, scan, LAT, 16)
    assert len(out["cand_index"]) == 16 and out["best"] >= 0
    assert (np.diff(out["cand_score"]) <= 0).all()
    win = out["records"][out["best"]]
    dm, dr = pose_error(win["pose"], truth)
    print("scan %d: winner = candidate %d, %.4f m, %.2e rad, cost %.3g" % (k, out["best"], dm, dr, win["fitness"]))
    assert win["converged"] and dm <= 0.05 and dr <= 0.002
    if k in (2, 6):
        assert out["best"] != 0
    assert out["best"] == ref_best(out["records"])


def test_oracle_agrees_with_itself_on_no_pairs_and_no_score(oracle, world):
    om, sf = world
    for k in range(2):
        scan, truth, _ = sf.make(k)
        s, p = oracle_scores(oracle, om, scan, edge_poses(truth))
        assert ((p == 0) == (s == 0.0)).all()
        assert p[0] > 0 and (p[5:8] == 0).all()                           # the truth meets the map; far poses meet nothing
