"""ndt_fit_points_batch{,_dev} without a device: the declared surface, the layout of ndt_fit_stats, the NULL-context refusal
from pedantic C99, the numpy restatement of the stats (tests/fit_points_helpers.py) on hand-made vectors, the exactness
the GPU test's bit-for-bit claim rests on, and the relocalisation scene of a half-covered map on the CPU oracle."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import fitness_workloads as W
from fit_points_helpers import (DBL_MAX, HALF_SCENES, half_scene, narrow_pool, ranged_best, ranged_of_records, ref_stats,
                                tf_of_pose)
from reloc_helpers import LAT, pose_error, ref_best, relocalize_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = ("ndt_fit_points_batch", "ndt_fit_points_batch_dev")


@pytest.fixture(scope="module")
def capi():
    from ndt_slam_amd import build, capi
    build.build()
    return capi


# ------------------------------------------------------------------------------------------ the surface
def test_header_declares_library_exports_and_binding_lists_both_names(capi):
    src = open(os.path.join(ROOT, "include", "ndt_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert "typedef struct ndt_fit_stats" in code
    # each entry's comment cites the reference's call and PCL's ranged form
    for name in NAMES + ("ndt_fit_stats",):
        at = src.index("typedef struct ndt_fit_stats" if name == "ndt_fit_stats" else "int %s(" % name)
        near = src[max(0, at - 1200):at + 1200]
        assert "src/PoseEstimator.cpp:43" in near and "getFitnessScore(max_range)" in near, name


def test_fit_stats_layout(capi):
    S = capi.FitStats
    assert ctypes.sizeof(S) == 32
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("fitness", 0), ("fitness_all", 8), ("n_in", 16), ("n_dist", 20),
                                                                 ("n_points", 24), ("reserved", 28)]
    dt = capi.FIT_STATS_DTYPE
    assert dt.itemsize == 32 and [dt.fields[n][1] for n in dt.names] == [0, 8, 16, 20, 24, 28]


C99 = r"""
#include <float.h>
#include <stdio.h>
#include <string.h>
#include "ndt_mi355x.h"
int main(void) {
  float xy[2] = {0.f, 0.f}, tf[4] = {1.f, 0.f, 0.f, 0.f}, d2[1] = {-1.f};
  uint64_t off[2] = {0, 1};
  ndt_fit_stats st;
  int rc;
  memset(&st, 0x5a, sizeof st);
  if (sizeof(ndt_fit_stats) != 32) return 10;
  rc = ndt_fit_points_batch(NULL, NULL, xy, off, 1, 0, tf, sizeof tf, DBL_MAX, d2, &st);
  if (rc != NDT_E_ARG || strcmp(ndt_last_error(NULL), "null context") != 0) return 11;
  rc = ndt_fit_points_batch_dev(NULL, NULL, xy, off, 1, 1, 0, tf, sizeof tf, 0.0, d2, &st, NULL);
  if (rc != NDT_E_ARG || strcmp(ndt_last_error(NULL), "null context") != 0) return 12;
  if (d2[0] != -1.f || st.n_points != 0x5a5a5a5au) return 13;
  puts("ok");
  return 0;
}
"""


def test_pedantic_c99_compiles_the_header_and_a_null_context_is_refused(capi, tmp_path):
    src, exe = tmp_path / "fit_points_c99.c", tmp_path / "fit_points_c99"
    src.write_text(C99)
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["cc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-l:" + os.path.basename(capi.LIB_PATH), "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout)


# ------------------------------------------------------------------------------------------ the restatement
def test_restatement_on_hand_made_vectors():
    d = np.array([0.25, 0.0, 1.5, np.inf, 0.0, 3.0, np.nan, 0.75], dtype=F)
    assert ref_stats(d, DBL_MAX) == (5.5 / 6, 5.5 / 6, 6, 6, 8)
    # a value equal to max_d2 is in; the double just below it as the threshold puts that value out
    assert ref_stats(d, 1.5) == (2.5 / 5, 5.5 / 6, 5, 6, 8)
    assert ref_stats(d, float(np.nextafter(1.5, 0.0))) == (1.0 / 4, 5.5 / 6, 4, 6, 8)
    # the comparison is made on the widened value: a float32 that is not a short double
    x = F(0.1)
    assert ref_stats(np.array([x], dtype=F), float(x)) == (float(x), float(x), 1, 1, 1)
    assert ref_stats(np.array([x], dtype=F), 0.1) == (DBL_MAX, float(x), 0, 1, 1)      # F(0.1) > 0.1
    assert ref_stats(np.array([x], dtype=F), float(np.nextafter(float(x), 0.0)))[2] == 0
    # all-inf gives DBL_MAX; max_d2 = 0.0 counts only zeros; an empty scan
    assert ref_stats(np.full(5, np.inf, dtype=F), DBL_MAX) == (DBL_MAX, DBL_MAX, 0, 0, 5)
    assert ref_stats(d, 0.0) == (0.0, 5.5 / 6, 2, 6, 8)
    assert ref_stats(np.array([0.5, 2.0], dtype=F), 0.0) == (DBL_MAX, 1.25, 0, 2, 2)
    assert ref_stats(np.zeros(0, dtype=F), DBL_MAX) == (DBL_MAX, DBL_MAX, 0, 0, 0)
    # the sum is taken over the WIDENED values (in float32 the small term would be lost)
    big = np.array([1.0] * 1000 + [2.0 ** -30], dtype=F)
    assert ref_stats(big, DBL_MAX)[0] == (1000.0 + 2.0 ** -30) / 1001


def test_rerank_rule(capi):
    rec = np.zeros(4, dtype=capi.RESULT_DTYPE)
    rec["converged"] = [1, 1, 0, 1]
    st = np.zeros(4, dtype=capi.FIT_STATS_DTYPE)
    st["fitness"] = [0.5, 0.25, 0.01, 0.25]
    st["n_in"] = [9, 3, 9, 7]
    assert capi.rerank(rec, st) == 3 == ranged_best(rec, st["fitness"], st["n_in"])      # tie in fitness: the higher n_in
    st["n_in"][3] = 3
    assert capi.rerank(rec, st) == 1 == ranged_best(rec, st["fitness"], st["n_in"])      # full tie: the lower index
    rec["converged"] = 0
    assert capi.rerank(rec, st) == 0                                                      # all 1e7, n_in 9 twice: index 0
    assert capi.rerank(rec[:0], st[:0]) == -1


# ------------------------------------------------------------------------------------------ what the GPU test relies on
@pytest.mark.parametrize("family", list(W.FAMILIES))
def test_in_range_subsets_of_stratified_scans_are_exact_and_there_are_six_cuts(family):
    """For the identity and the two moved poses of the GPU test: every stratified cut has an exact sum, and so has its
    in-range subset at every threshold the GPU test uses (a subset spans no more binades and has no more points); and the
    three poses give at least 6 cuts."""
    leaf, off = 0.3, W.OFFSETS[1]
    w = W.make(family, leaf, off)
    b, L = W.lattice_base(leaf, off)
    poses = [(0.0, 0.0, 0.0), (b[0] + 3.7 * L, b[1] - 1.9 * L, 0.6), (b[0] - 40.5 * L, b[1] + 27.25 * L, -2.2)]
    n_cuts = 0
    for k, p in enumerate(poses):
        scan = w.queries if k == 0 else W.scan_for(w.queries, p)
        d = W.brute_sq(w.map, W.queries_of(scan, tf_of_pose(p), True))
        fin = d[np.isfinite(d)].astype(np.float64)
        thresholds = [float(np.median(fin)), 0.0, DBL_MAX, float(fin[len(fin) // 3]), float(np.nextafter(fin[len(fin) // 3], 0.0))]
        for cut in W.stratify(None, d, 900):
            n_cuts += 1
            assert W.sum_is_exact(d[cut])
            for t in thresholds:
                sub = d[cut][np.isfinite(d[cut]) & (d[cut].astype(np.float64) <= t)]
                assert W.binades(sub) <= W.binades(d[cut]) and W.binades(sub) <= W.max_binades(max(len(sub), 1))
                # exact: the float64 running sum in any order equals fsum
                s64 = sub.astype(np.float64)
                assert float(np.sum(s64[::-1])) == math.fsum(s64.tolist()) == float(np.cumsum(s64)[-1] if len(s64) else 0.0)
    assert n_cuts >= 6


def test_narrow_pool_scans_are_exact():
    w = W.make("sparse", 0.3, W.OFFSETS[0])
    scans, ds = narrow_pool(w, (1, 63, 64, 65, 255, 256, 257, 4097, 16385))
    assert [len(s) for s in scans] == [1, 63, 64, 65, 255, 256, 257, 4097, 16385]
    for d in ds:
        assert W.sum_is_exact(d) and np.isfinite(d).all()
    assert sum(int((d == 0).sum()) for d in ds) >= 50 and len(set(np.frexp(ds[-1][ds[-1] > 0].astype(np.float64))[1])) >= 5


# ------------------------------------------------------------------------------------------ the half-covered map, on the oracle
@pytest.mark.parametrize("k,axis,side", HALF_SCENES)
def test_unbounded_mean_picks_a_wrong_pose_in_a_half_covered_map_and_the_ranged_one_the_truth(oracle, c1_world, k, axis, side):
    """The C1 map cut to the half-plane that holds about half of the scan at the true pose; sweep LAT, refine 16 candidates
    (the prototype of reloc_helpers on the oracle).  The candidate at the truth is among them; `converged ? fitness : 1e7`
    ranks another one first, metres away; the ranged mean with max_d2 = (2 leaf)^2 ranks the truth first."""
    m, sf, cfg = c1_world
    leaf = cfg["resolution"]
    hm, scan, truth = half_scene(m, sf, k, axis, side)
    prm = oracle.default_params(resolution=leaf)
    # about half of the scan has no map within two voxels at the truth
    d_true = W.brute_sq(hm, W.queries_of(scan, tf_of_pose(truth), bool(prm.transform_sse)))
    share = float((d_true.astype(np.float64) <= (2 * leaf) ** 2).mean())
    assert 0.35 <= share <= 0.65, share
    out = relocalize_ref(oracle, oracle.Map(hm, prm), scan, LAT, 16)
    rec = out["records"]
    err = np.array([pose_error(r["pose"], truth)[0] for r in rec])
    fit, n_in = ranged_of_records(hm, scan, rec, (2 * leaf) ** 2, bool(prm.transform_sse))
    best_r = ranged_best(rec, fit, n_in)
    print("scene %r: in range at the truth %.2f; unbounded best = candidate %d (%.3f m off, cost %.4g); ranged best = candidate %d "
          "(%.3f m off, ranged %.4g, n_in %d)" % ((k, axis, side), share, out["best"], err[out["best"]],
                                                 rec[out["best"]]["fitness"], best_r, err[best_r], fit[best_r], n_in[best_r]))
    assert (err <= 0.05).any()
    assert out["best"] == ref_best(rec) and err[out["best"]] > 1.0
    assert err[best_r] <= 0.05 and rec[best_r]["converged"]
