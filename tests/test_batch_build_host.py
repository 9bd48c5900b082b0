"""ndt_map_build_batch{,_dev} without a device: the header declares both, the binding lists them, and a NULL context is
refused before anything else is looked at."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared():
    src = open(os.path.join(ROOT, "include", "ndt_mi355x.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(ndt_[a-z_0-9]+)\s*\(", src))


def test_header_and_binding_list_both_entry_points():
    from ndt_slam_amd import capi
    for name in ("ndt_map_build_batch", "ndt_map_build_batch_dev"):
        assert name in declared(), name
        assert name in capi.EXPORTS, name
    assert callable(capi.build_maps) and callable(capi.Context.build_maps_dev) and callable(capi.Map.adopt)


@pytest.mark.parametrize("fn", ["ndt_map_build_batch", "ndt_map_build_batch_dev"])
def test_null_context_is_refused_first(fn):
    from ndt_slam_amd import build, capi
    build.build()
    L = capi.lib()
    # every other argument is bad too: the context is checked first
    rc = getattr(L, fn)(None, None, None, 12, 0, None, None)
    assert rc == capi.NDT_E_ARG
    assert L.ndt_last_error(None).decode() == "null context"
    pts = (ctypes.c_float * 4)(0.0, 0.0, 1.0, 1.0)
    xy = (ctypes.c_void_p * 1)(ctypes.addressof(pts))
    n = (ctypes.c_size_t * 1)(2)
    prm = (capi.Params * 1)(capi.default_params())
    maps = (ctypes.c_void_p * 1)(None)
    assert getattr(L, fn)(None, xy, n, 8, 1, prm, maps) == capi.NDT_E_ARG
    assert L.ndt_last_error(None).decode() == "null context"
    assert maps[0] is None
