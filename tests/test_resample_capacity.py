"""The resampler's C ABI without a GPU: the four new entry points are declared, bound and exported, and
ndt_resample_capacity (which needs no device) bounds the output of ScanPointResampler::resamplePoints
(src/ScanPointResampler.cpp:4-62, mirrored by replay.resample_points) and refuses what the reference cannot do."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from ndt_slam_amd import replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ndt_resample_capacity", "ndt_resample_batch_dev", "ndt_resample", "ndt_scan_to_map_batch_dev")
PAIRS = [(0.05, 0.25), (0.05, 0.05), (0.1, 0.05), (0.0, 0.0)]


@pytest.fixture(scope="module")
def capi():
    from ndt_slam_amd import build
    build.build()
    from ndt_slam_amd import capi
    return capi


def adversarial_scans(space, space_thre, rng):
    """Inputs that stress the bound: random walks, collinear points at exact multiples of `space`, segments just below
    `space_thre`, duplicates, gaps exactly equal to `space_thre`."""
    out = [rng.normal(0, 0.03, (500, 2)).cumsum(0), rng.normal(0, 0.3, (300, 2)).cumsum(0)]
    step = space if space > 0 else 0.05
    out.append(np.column_stack([np.arange(200) * step, np.zeros(200)]))
    out.append(np.column_stack([np.arange(200) * step * 3, np.arange(200) * step * 4]))
    below = np.nextafter(space_thre, 0) if space_thre > 0 else 0.0
    out.append(np.column_stack([np.arange(100) * below, np.zeros(100)]))
    out.append(np.column_stack([np.zeros(100), np.arange(100) * below * 0.999]))
    out.append(np.repeat(rng.uniform(-5, 5, (60, 2)), 4, axis=0))
    out.append(np.zeros((50, 2)))
    out.append(np.column_stack([np.arange(100) * space_thre, np.zeros(100)]))
    out.append(np.column_stack([np.arange(100) * space_thre * 0.6, np.arange(100) * space_thre * 0.8]))
    mixed = rng.normal(0, 0.02, (400, 2)).cumsum(0)
    mixed[::37] += space_thre
    out.append(mixed)
    out.append(np.zeros((1, 2)))
    return out


def test_the_new_entry_points_are_declared_bound_and_exported(capi):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ndt_mi355x.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ndt_[a-z_0-9]+)\s*\(", src))
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in capi.EXPORTS, name
        assert hasattr(L, name), name


@pytest.mark.parametrize("space,space_thre", PAIRS)
def test_capacity_bounds_the_resampler(capi, space, space_thre):
    rng = np.random.default_rng(11)
    k_max = 1 if space_thre <= space else math.floor(space_thre / space) + 2
    for scan in adversarial_scans(space, space_thre, rng):
        n_out = len(replay.resample_points(scan, space, space_thre))
        cap = capi.resample_capacity(len(scan), space, space_thre)
        assert cap == len(scan) * k_max
        assert n_out <= cap, (len(scan), n_out, cap)
    assert capi.resample_capacity(0, space, space_thre) == 0


def test_capacity_bounds_the_synthetic_scans(capi):
    from ndt_slam_amd import synth
    recs, _ = synth.replay_records(n_frames=4, n_beams=1081)
    for r in recs:
        n_out = len(replay.resample_points(r["front"], 0.05, 0.25))
        assert n_out <= capi.resample_capacity(len(r["front"]), 0.05, 0.25)


@pytest.mark.parametrize("space,space_thre", [(-0.05, 0.25), (0.05, -0.25), (math.nan, 0.25), (0.05, math.nan),
                                              (math.inf, 0.25), (0.05, math.inf), (0.0, 0.25), (1e-300, 1e300)])
def test_capacity_refuses_what_the_reference_cannot_do(capi, space, space_thre):
    cap = ctypes.c_size_t(123)
    rc = capi.lib().ndt_resample_capacity(10, space, space_thre, ctypes.byref(cap))
    assert rc == capi.NDT_E_ARG and cap.value == 123
    with pytest.raises(capi.NdtError):
        capi.resample_capacity(10, space, space_thre)


def test_capacity_refuses_an_overflowing_product(capi):
    cap = ctypes.c_size_t()
    assert capi.lib().ndt_resample_capacity(2 ** 62, 0.05, 0.25, ctypes.byref(cap)) == capi.NDT_E_ARG
    assert capi.lib().ndt_resample_capacity(2 ** 61, 0.05, 0.05, ctypes.byref(cap)) == capi.NDT_OK
    assert cap.value == 2 ** 61
    assert capi.lib().ndt_resample_capacity(10, 0.05, 0.25, None) == capi.NDT_E_ARG
