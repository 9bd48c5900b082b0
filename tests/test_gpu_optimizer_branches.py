"""The device's optimiser (ndt_slam_amd/csrc/ndt_optimizer.hip.h) against the oracle on the inputs of tests/optimizer_cases.py:
the unit rows through ndt_selftest_optimizer -- the device functions the match kernel calls, one lane per row -- and the
match list through ndt_align_batch_trace.  tests/test_optimizer_cases_host.py shows on the CPU that these inputs reach
every branch and that the oracle is right on them.

Why bit equality is the expectation for solve3 / mt_trial / mt_update: every branch is decided by exact comparisons of the
inputs or of values computed the same way, and both sides are built without contraction on correctly rounded fp64
+ - * / sqrt (fmax / fabs are exact).  Derived, then measured on an MI355X: LOG.md R20."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import optimizer_cases as OC      # noqa: E402
from gpu_support import gpu  # noqa: E402, F401

pytestmark = pytest.mark.gpu
EPS = OC.EPS


@pytest.fixture(scope="module")
def omaps(oracle, c1_world):
    m, _, cfg = c1_world
    return {k: oracle.Map(m, oracle.default_params(resolution=cfg["resolution"], **kw)) for k, kw in OC.PARAM_SETS.items()}


@pytest.fixture(scope="module")
def mt_all(oracle, c1_world, omaps):
    return OC.mt_rows(OC.harvest_mt_rows(oracle, c1_world, omaps))


@pytest.fixture(scope="module")
def device_rows(gpu, mt_all):
    """Every unit row through the device once: one launch, four parts."""
    capi, ctx = gpu
    s3, _ = OC.solve3_rows()
    mt, _ = mt_all
    out = ctx.selftest_optimizer(solve3=s3, mt_trial=mt, mt_update=mt, yaw=OC.yaw_rows())
    # a part alone gives what it gives in company (the parts are independent)
    alone = ctx.selftest_optimizer(mt_trial=mt[:100])
    assert OC.bits(alone["mt_trial"]).tobytes() == OC.bits(out["mt_trial"][:100]).tobytes() and set(alone) == {"mt_trial"}
    return out


def _group_of(groups, i):
    return next(k for k, sl in groups.items() if sl.start <= i < sl.stop)


def test_mt_update_equals_the_oracle_bit_for_bit(oracle, mt_all, device_rows):
    """It copies values and tests signs: the six interval values and the return value, every row."""
    rows, groups = mt_all
    dev = device_rows["mt_update"]
    want = np.zeros_like(dev)
    for i, r in enumerate(rows):
        rc, v = oracle.mt_update(*r)
        want[i, :6] = v; want[i, 6] = rc
    bad = np.nonzero((OC.bits(dev) != OC.bits(want)).any(axis=1))[0]
    assert len(bad) == 0, [(int(i), _group_of(groups, i), rows[i], dev[i], want[i]) for i in bad[:5]]
    assert set(np.unique(want[:, 6])) == {0.0, 1.0}


def test_mt_trial_equals_the_oracle_bit_for_bit(oracle, mt_all, device_rows):
    rows, groups = mt_all
    dev = device_rows["mt_trial"]
    want = np.array([oracle.mt_trial(*r) for r in rows])
    d = OC.ulp_distance(dev, want)
    print("mt_trial: %d rows, %d NaN on both sides, worst ulp distance to the oracle %d" % (len(rows), int(np.isnan(want).sum()), int(d.max())))
    bad = np.nonzero(OC.bits(dev) != OC.bits(want))[0]
    assert len(bad) == 0, [(int(i), _group_of(groups, i), rows[i], dev[i], want[i]) for i in bad[:5]]
    assert np.isnan(want).sum() >= 100 and np.isfinite(want).sum() >= 3000


def test_solve3_equals_the_oracle_bit_for_bit(oracle, device_rows):
    rows, groups = OC.solve3_rows()
    dev = device_rows["solve3"]
    want = np.array([oracle.solve3(*OC.rows_to_matrix(r)) for r in rows])
    d = OC.ulp_distance(dev, want)
    print("solve3: %d rows, worst ulp distance to the oracle %d" % (len(rows), int(d.max())))
    bad = np.nonzero((OC.bits(dev) != OC.bits(want)).any(axis=1))[0]
    assert len(bad) == 0, [(int(i), _group_of(groups, i), rows[i], dev[i], want[i]) for i in bad[:5]]
    assert np.isnan(want[groups["nan_entry"]]).all(axis=1).sum() >= 6


def test_solve3_against_jacobisvd_6x6(device_rows):
    """The device's solve3 on the fixture of the reference's vendored Eigen, at the bounds test_newton_solve_against_jacobisvd_6x6
    (tests/test_eigen_pins.py) holds the oracle to; the null direction of every rank-deficient row is dropped."""
    rows, groups = OC.solve3_rows()
    z = np.load(OC.GOLD)
    d, sv, n_real = z["svd6_dp3_eig"], z["svd6_sv_eig"], int(z["svd6_n_real"])
    dev = device_rows["solve3"][groups["svd6"]]
    n_deficient = 0
    for i in range(len(d)):
        rel = np.linalg.norm(dev[i] - d[i]) / np.linalg.norm(d[i])
        ratio = sv[i, 2] / sv[i, 0]
        if i < n_real:
            assert rel < 1e-12, (i, rel)
        elif ratio < 6 * EPS:
            assert rel < 1e-13, (i, rel, ratio)
            H, _ = OC.rows_to_matrix(rows[groups["svd6"]][i])
            w, V = np.linalg.eigh(H)
            null = V[:, np.argmin(np.abs(w))]
            assert abs(dev[i] @ null) <= 1e-9 * np.linalg.norm(dev[i]), (i, dev[i], null)      # (eigh's own null vector: 1e-9)
            n_deficient += 1
        else:
            assert rel < max(1e-13, 16 * EPS / ratio), (i, rel, ratio)
    assert n_deficient >= 10


def test_yaw_from_T_equals_the_oracle_bit_for_bit(oracle, device_rows):
    """As test_yaw_strata_near_90_and_180 demands for six matches, on 1e5 matrices.  A row that differs is judged by the
    50-digit value: the device must then be the one that is right."""
    T = OC.yaw_rows()
    dev = device_rows["yaw"]
    want = np.array([oracle.yaw_from_T(float(a), float(b)) for a, b in T])
    bad = np.nonzero(OC.bits(dev) != OC.bits(want))[0]
    print("yaw_from_T: %d rows, %d differ from the oracle" % (len(T), len(bad)))
    if len(bad):
        import mpmath as mp
        mp.mp.dps = 50
        for i in bad:
            t00, t10 = float(T[i, 0]), float(T[i, 1])
            v = mp.asin(mp.mpf(t10)) if t00 > 0 and t10 != 0 else mp.acos(mp.mpf(t00)) * (1 if (t00 < 0 and t10 > 0) else -1)
            assert dev[i] == float(np.float32(float(v))), (int(i), t00, t10, dev[i], want[i], float(v))


# ------------------------------------------------------------------------------------------------------------ the match list
def _batches(c1_world):
    """{parameter set: [(name, scan, init)]}: every MATCHES entry and every special scan, none left out."""
    out = {k: [] for k in OC.PARAM_SETS}
    for e in OC.MATCHES:
        scan, init = OC.match_inputs(c1_world, e)
        out[e[0]].append((e, scan, init))
    for name, pset, scan, init in OC.special_matches(c1_world):
        out[pset].append((name, scan, init))
    return out


def _same(a, b):
    """Equal, NaN for NaN."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def test_match_list_follows_the_oracle(gpu, oracle, c1_world, omaps):
    """One launch per parameter set (a map carries its parameters) with traces, plus ndt_align singly for every fifth."""
    from test_gpu_parity import assert_result_parity
    capi, ctx = gpu
    m, _, cfg = c1_world
    n_rows = n_matches = 0
    for pset, items in _batches(c1_world).items():
        gm = capi.Map(ctx, m, capi.default_params(resolution=cfg["resolution"], **OC.PARAM_SETS[pset]))
        scans, off = capi.pack_scans([it[1] for it in items])
        inits = np.array([it[2] for it in items])
        res, traces = gm.align_batch(scans, off, inits, trace_cap=512)
        for b, (name, scan, init) in enumerate(items):
            ref, tr = omaps[pset].align(scan, init, trace_cap=512, run_stats=True)
            r, t = res[b], traces[b]
            n_matches += 1; n_rows += len(tr)
            assert int(r["status"]) == 0, name
            if isinstance(name, str) and name in OC.SPECIAL_DEGENERATE:
                # no point with a finite image in reach of a voxel (include/ndt_mi355x.h): converged, iters and the pose as the oracle's
                assert (int(r["converged"]), int(r["iters"]), len(t)) == (int(ref["converged"]), int(ref["iters"]), len(tr)) == (1, 0, 1), name
                assert _same(r["pose"], ref["pose"]) and _same(r["p"], ref["p"]), (name, r["pose"], ref["pose"], r["p"], ref["p"])
                assert _same([r["T00"], r["T10"], r["T03"], r["T13"]], [ref["T00"], ref["T10"], ref["T03"], ref["T13"]]), name
                assert r["fitness"] == ref["fitness"] or r["fitness"] == pytest.approx(ref["fitness"], rel=1e-12), name
                assert r["score"] == 0.0 and np.all(r["H"] == 0.0), name
            else:
                assert_result_parity(r, ref)
                assert len(t) == len(tr), name
                assert t[:, 0] == pytest.approx(tr[:, 0], rel=1e-8, abs=1e-12), name              # step lengths
                nz = tr[:, 1] != 0
                assert t[nz, 1] == pytest.approx(tr[nz, 1], rel=1e-10), name                     # scores
                assert np.all(t[~nz, 1] == 0.0), name
                assert np.all(np.abs(t[:, 5:8] - tr[:, 5:8]) <= 1e-9), name                      # trial poses
            if b % 5 == 0 or isinstance(name, str):
                assert gm.align(scan, init).tobytes() == r.tobytes(), name                        # batch == single, byte for byte
        gm.close()
    assert n_matches == len(OC.MATCHES) + len(OC.special_matches(c1_world)) and n_rows >= 5 * len(OC.MATCHES)
