"""The derivative pass of the match kernel (eval_point driven by pass_units, its LDS window staged by region_from_bbox /
fill_window_plan / fill_window_fetch) across the window geometries of tests/match_window_workloads.py, held to the HBM
pass and to the C oracle row by row.  tests/test_match_window_host.py shows on the CPU that every family reaches the path
it is named after and that the census used here is right on hand-worked windows.

Per case one traced match (trace_cap 64).  A trace row that is bit-equal to the row before it is a pass that was counted
and not run (repeat_totals); the other rows are the executed passes and their number must be `evals`.  A trial row's
transform is a function of its three pose columns alone (trial_transforms forms the float32 matrix and the angle terms
from S.xt, which are those columns; ndt_eval_at and the oracle's eval_at form them from p by the same rules), so each
executed pass -- whose points went through the LDS window, the ring, the -inf sentinel or the spilled pool as the census
says -- is evaluated again at the same pose by the oracle and by ndt_eval_at, whose kernel has an empty window and reads
the dense grid in HBM for every point.  Row 0 comes from the guess matrix: init_matrix takes cos / sin of the float32 yaw
and (float) tx, ty, and init_rest reads p0 back from that matrix -- (double) T.tx, (double) T.ty and the yaw of (c, s); for
yaw 0 that is c = 1, s = 0, p0 = (T.tx, T.ty, 0), from which tf_from_p gives the same matrix and angle_cs the same (1, 0):
row 0 is included (the test asserts p0 is what this says).  `walk` starts from a yaw: its row 0 is held to the oracle's
own trace row 0, and its pair total to the oracle's count of the pairs the device path runs.

Tolerances, none of them measured on the device.  Pairs: equal.  Score: every term is >= 0, so any order of summation is
within (terms - 1) 2^-53 relative and exp_neg is about an ulp per term: rel (2 pairs + 8) 2^-53, never looser than the
1e-10 of test_c1_matches_oracle_with_same_step_sequence.  Gradient and Hessian: the rule of
test_single_evaluation_matches_oracle (rel 1e-9, abs 1e-10 max|.|).  Whether a family cancels harder than that rule
allows was measured on the REFERENCE alone: the oracle's eval_at with the scan in input order against reversed order at
every pose of its own traces differs, times 16, by at most 0.19 of what the rule allows (worst: row_phase[32]; typical
1e-5 .. 1e-4), so the rule stands as it is for every family.  `degenerate_records`: where the oracle's gradient or Hessian
is NaN (it poisons itself as PCL would) pairs and score are held and the device's sums must be finite.

The CHK instance.  launch_align picks <sse, !incl, CHK> when !(e_hi > 1 + 1e-6), i.e. when d2 is within 1e-6 of 1.  With
c1 = 10 (1 - o), c2 = o / res^3 (Magnusson eq 6.8) 1 - d2 = 0.39 c1 / c2 to first order.  The issue's route, resolution
0.005 at the default outlier ratio, reaches it (4e-7); so does outlier_ratio = 1 - 5e-8 / res^3 at any resolution (c1 / c2 =
5e-7, 1 - d2 = 2e-7; the constants' own rounding is 5e-8 there, which is why it is not pushed further), which
keeps the leaf -- hence every window, and radius_tie's exact ties -- as the other four instances have them.  The test
computes d2 on the host for both and asserts on which side of the rule each falls.
"""
import math
import time

import numpy as np
import pytest

import match_window_workloads as W
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

T0 = time.time()
NAMES = [c.name for c in W.cases()]
TRACE_CAP = 64


def distinct_rows(tr):
    return [k for k in range(len(tr)) if k == 0 or tr[k].tobytes() != tr[k - 1].tobytes()]


def score_rel(pairs):
    return min((2.0 * pairs + 8.0) * 2.0 ** -53, 1e-10)


def close(a, ref, rel, abs_):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool(np.all(np.abs(a - ref) <= np.maximum(rel * np.abs(ref), abs_)))


def grad_close(a, ref):
    """rel 1e-9, abs 1e-10 max|ref| (test_single_evaluation_matches_oracle)."""
    return close(a, ref, 1e-9, 1e-10 * (np.abs(ref).max() + 1e-300))


_MAPS = {}


def dev_map(gpu, c):
    """The device map of a case, built once and kept (a few thousand voxels each)."""
    capi, ctx = gpu
    if c.name not in _MAPS:
        _MAPS[c.name] = capi.Map(ctx, c.cloud, W.params_of(c, capi))
    return _MAPS[c.name]


def offsets_of(c):
    return np.array([0, len(c.scan)], dtype=np.uint64)


_ALONE = {}


def alone(gpu, c):
    """(record, trace) of the case matched alone with default options, once."""
    if c.name not in _ALONE:
        res, traces = dev_map(gpu, c).align_batch(c.scan, offsets_of(c), [c.init], trace_cap=TRACE_CAP)
        _ALONE[c.name] = (res[0].copy(), traces[0].copy())
    return _ALONE[c.name]


def hold_case(gpu, oracle, c):
    """Everything the module docstring says about one traced match."""
    capi, ctx = gpu
    gm = dev_map(gpu, c)
    om, grid, cs = W.census_of(c, oracle)
    r, tr = alone(gpu, c)
    n = len(c.scan)
    assert r["status"] == 0 and len(tr) < TRACE_CAP, (c.name, r["status"], len(tr))
    want = capi.FLAG_WINDOW_SPILL | capi.FLAG_REGION_CLIPPED
    assert (capi.FLAG_WINDOW_SPILL, capi.FLAG_REGION_CLIPPED) == (W.FLAG_WINDOW_SPILL, W.FLAG_REGION_CLIPPED)
    assert int(r["flags"]) & want == cs.flags, (c.name, int(r["flags"]), cs.flags, cs.kept, cs.skipped, cs.cap)
    rows = distinct_rows(tr)
    assert len(rows) == int(r["evals"]), (c.name, len(rows), int(r["evals"]), len(tr))
    yaw0 = c.init[2] == 0.0
    ref_tr = None
    if yaw0:
        assert tr[0][5] == float(np.float32(c.init[0])) and tr[0][6] == float(np.float32(c.init[1])) and tr[0][7] == 0.0, c.name
    else:
        ref, ref_tr = om.align(c.scan, c.init, trace_cap=TRACE_CAP, run_stats=True)
    total, last = 0, None
    for k in rows:
        row = tr[k]
        if k == 0 and not yaw0:                     # (held below, once the other rows have left row 0's share of the pairs)
            continue
        p = row[5:8]
        s0, g0, H0, pairs0 = om.eval_at(c.scan, p)
        s1, g1, H1, pairs1 = gm.eval_at(c.scan, p)
        print("  %s row %d: pairs %d score %.17g oracle %.17g hbm %.17g |g| %.3g" % (c.name, k, pairs0, row[1], s0, s1, np.abs(row[2:5]).max()))
        assert pairs1 == pairs0, (c.name, k, pairs1, pairs0)
        rel = score_rel(pairs0)
        assert close(row[1], s0, rel, 0.0) and close(row[1], s1, rel, 0.0), (c.name, k, "score", row[1], s0, s1, rel)
        assert np.isfinite(row[2:5]).all() and np.isfinite(g1).all() and np.isfinite(H1).all(), (c.name, k)
        if np.isfinite(g0).all() and np.isfinite(H0).all():
            assert grad_close(row[2:5], g0), (c.name, k, "gradient against the oracle", row[2:5], g0)
            assert grad_close(row[2:5], g1) and grad_close(g1, g0), (c.name, k, "gradient against the HBM pass", row[2:5], g1)
        else:
            assert c.family == "degenerate_records", (c.name, k, g0, H0)
        total += int(pairs0)
        last = (s0, g0, H0, pairs0, s1, H1)
    # the record: score and Hessian are the last executed pass's
    s0, g0, H0, pairs0, s1, H1 = last
    assert close(r["score"], s0, score_rel(pairs0), 0.0) and close(r["score"], s1, score_rel(pairs0), 0.0), (c.name, r["score"], s0, s1)
    H = np.asarray(r["H"]).reshape(3, 3)
    assert np.isfinite(H).all(), c.name
    if np.isfinite(H0).all():
        assert grad_close(H, H0) and grad_close(H, H1), (c.name, H, H0, H1)
    # pairs: kbar evals n is the integer the passes counted
    counted = float(r["kbar"]) * int(r["evals"]) * n
    assert abs(counted - round(counted)) < 1e-6, (c.name, counted)          # (kbar = pairs / (evals n): two roundings of 2^-53 pairs)
    if yaw0:
        assert int(round(counted)) == total, (c.name, counted, total)
    else:
        assert int(r["evals"]) == int(ref["evals_run"]) and int(round(counted)) == int(ref["pairs_run"]), (c.name, counted, ref["pairs_run"])
        pairs_row0 = int(ref["pairs_run"]) - total
        assert pairs_row0 > 0, (c.name, pairs_row0)
        assert close(tr[0][1], ref_tr[0][1], score_rel(pairs_row0), 0.0), (c.name, "row 0 score", tr[0][1], ref_tr[0][1])
        assert grad_close(tr[0][2:5], ref_tr[0][2:5]), (c.name, "row 0 gradient", tr[0][2:5], ref_tr[0][2:5])
    return r


@pytest.mark.parametrize("name", NAMES)
def test_every_pass_of_a_case_against_the_oracle_and_the_hbm_pass(gpu, oracle, name):
    hold_case(gpu, oracle, W.case(name))


def fillers():
    """One scan and initial guess per family: the company of a mixed batch."""
    return [W.cases(f)[0] for f in W.FAMILIES]


@pytest.mark.parametrize("name", NAMES)
def test_a_record_does_not_depend_on_company_helpers_or_workgroups(gpu, oracle, name):
    """Byte-identical records: alone with default options against (a) inside a batch of one scan of every family, in the
    middle, (b) NDT_OPT_MAX_HELPERS 0, 2 and 15, (c) NDT_OPT_WORKGROUPS 1 and 8, (d) ndt_align_batch_multi with the case's
    map between two others (the MULTI instance of the kernel)."""
    capi, ctx = gpu
    c = W.case(name)
    gm = dev_map(gpu, c)
    base = alone(gpu, c)[0].tobytes()
    one = (c.scan, offsets_of(c), [c.init])
    company = fillers()
    pos = len(company) // 2
    batch = company[:pos] + [c] + company[pos:]
    scans, off = capi.pack_scans([b.scan for b in batch])
    res = gm.align_batch(scans, off, [b.init for b in batch])
    assert res[pos].tobytes() == base, (name, "mixed batch")
    try:
        for h in (0, 2, 15):
            ctx.set_option(capi.OPT_MAX_HELPERS, h)
            assert gm.align_batch(*one)[0].tobytes() == base, (name, "helpers", h)
        ctx.set_option(capi.OPT_MAX_HELPERS, -1)
        for wg in (1, 8):
            ctx.set_option(capi.OPT_WORKGROUPS, wg)
            assert gm.align_batch(*one)[0].tobytes() == base, (name, "workgroups", wg)
            assert gm.align_batch(scans, off, [b.init for b in batch])[pos].tobytes() == base, (name, "workgroups", wg, "mixed batch")
    finally:
        ctx.set_option(capi.OPT_MAX_HELPERS, -1)
        ctx.set_option(capi.OPT_WORKGROUPS, 0)
    other = capi.Map(ctx, W.case("interior").cloud, W.params_of(c, capi))
    try:
        scans3, off3 = capi.pack_scans([c.scan, c.scan, c.scan])
        res = capi.align_batch_multi(ctx, [other, gm, other], scans3, off3, [c.init] * 3, map_of=[0, 1, 2])
        assert res[1].tobytes() == base, (name, "multi")
        res = capi.align_batch_multi(ctx, [other, gm], scans3, off3, [c.init] * 3, map_of=[1, 0, 1])
        assert res[0].tobytes() == base and res[2].tobytes() == base, (name, "multi, map_of")
    finally:
        other.close()


@pytest.mark.parametrize("side", W.GRID_EDGE_SIDES)
def test_grid_margin_changes_no_byte_of_a_record(gpu, oracle, side):
    """The header's promise: the same record with the grid widened by 8 voxels -- while ndt_map_info shows the wider grid."""
    c0, c8 = (W.case("grid_edge[%s,margin=%d]" % (side, m)) for m in (0, 8))
    i0, i8 = dev_map(gpu, c0).info(), dev_map(gpu, c8).info()
    assert (i8.min_bx, i8.min_by, i8.div_x, i8.div_y) == (i0.min_bx - 8, i0.min_by - 8, i0.div_x + 16, i0.div_y + 16)
    (r0, t0), (r8, t8) = alone(gpu, c0), alone(gpu, c8)
    assert r0.tobytes() == r8.tobytes() and t0.tobytes() == t8.tobytes()


# ------------------------------------------------------------------------------------------ the five kernel instances
def outlier_chk(resolution):
    """The outlier ratio that puts c1 / c2 at 5e-7, hence 1 - d2 near 2e-7, at this resolution."""
    return 1.0 - 5e-8 / float(resolution) ** 3


INSTANCES = (("sse,incl", dict(transform_sse=1, radius_inclusive=1)),
             ("sse", dict(transform_sse=1, radius_inclusive=0)),
             ("sse,chk", dict(transform_sse=1, radius_inclusive=0, outlier_ratio=None)),
             ("incl", dict(transform_sse=0, radius_inclusive=1)),
             ("plain", dict(transform_sse=0, radius_inclusive=0)))
INSTANCE_CASES = [c.name for f in ("ring", "pool_edge", "walk", "radius_tie") for c in W.cases(f) if c.prm.get("radius_inclusive", 0) == 0]


def d2_of(resolution, outlier_ratio):
    """The Gaussian constant d2 (Magnusson 2009 eq 6.8), on the host."""
    c1 = 10.0 * (1.0 - outlier_ratio)
    c2 = outlier_ratio / float(resolution) ** 3
    d3 = -math.log(c2)
    d1 = -math.log(c1 + c2) - d3
    return -2.0 * math.log((-math.log(c1 * math.exp(-0.5) + c2) - d3) / d1)


def test_which_parameters_reach_the_checked_instance(gpu):
    """e_hi is the largest double with d2 e_hi <= 1, i.e. 1 / d2 to an ulp: the default preset at 0.5 m and at 1 m is far on
    the unchecked side of launch_align's rule !(e_hi > 1 + 1e-6); resolution 0.005 and outlier_chk(res) are on the checked
    side with a margin no rounding of the constants can cross."""
    capi, ctx = gpu
    o = capi.default_params().outlier_ratio
    for res in (0.5, 1.0):
        assert 1.0 / d2_of(res, o) > 1.1
    assert 1.0 < 1.0 / d2_of(0.005, o) < 1.0 + 0.6e-6
    for res in (0.5, 1.0):
        assert 1.0 + 1e-7 < 1.0 / d2_of(res, outlier_chk(res)) < 1.0 + 4e-7


@pytest.mark.parametrize("inst", [i[0] for i in INSTANCES])
@pytest.mark.parametrize("name", INSTANCE_CASES)
def test_the_five_kernel_instances(gpu, oracle, name, inst):
    """ring, pool_edge, walk and radius_tie under each <SSE, INCL, CHK> instance launch_align can pick: the same row-by-row
    checks, against an oracle and a census with the instance's parameters."""
    c = W.case(name)
    over = dict(dict(INSTANCES)[inst])
    if "outlier_ratio" in over:
        over["outlier_ratio"] = outlier_chk(dict(W.DEFAULTS, **c.prm)["resolution"])
    v = c._replace(name="%s|%s" % (c.name, inst), prm=dict(c.prm, **over))
    try:
        hold_case(gpu, oracle, v)
    finally:
        m = _MAPS.pop(v.name, None)
        if m is not None:
            m.close()
        _ALONE.pop(v.name, None)
        W._CENSUS.pop(v.name, None)


def test_report_the_wall_time_of_this_module():
    for m in _MAPS.values():
        m.close()
    _MAPS.clear()
    print("\n  test_gpu_match_window_geometry.py: %.1f s from import to here" % (time.time() - T0))
