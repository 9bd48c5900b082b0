"""The robust pose-graph optimiser's oracle and workloads, without a device (tests/pg_robust_helpers.py): graduated
non-convexity keeps the true loops of a drifted chain and rejects the false one where a start at mu = 1 rejects a true one; every
decision of the workloads whose counts tests/test_gpu_pg_robust.py compares is far from a tie; without robust arcs the oracle is
pg_helpers' halving oracle; replay.robust_keep's rule on hand-made records."""
import numpy as np
import pytest

import pg_helpers as H
import pg_robust_helpers as R


@pytest.mark.parametrize("N, seed, loops, with_false", R.classification_cases())
def test_the_schedule_keeps_true_loops_and_rejects_the_false_one(N, seed, loops, with_false):
    """scale = 1.0: an end-of-chain drift of metres.  Automatic mu0 keeps every true arc (weight >= 0.9) and rejects every false
    one (weight below 1e-6); started at mu = 1 -- a plain Geman-McClure reweighting -- the same run rejects a true arc, which
    is what the schedule is for."""
    poses, edges, phi, bad = R.drifted(N, seed, 1.0, loops, [R.false_arc(N)] if with_false else [])
    rb = phi > 0
    ref = R.oracle_optimize_robust(poses, edges, phi)
    print("robust oracle N %d seed %d loops %d false %d: drift %.2f m | mu0 %.4g levels %d steps %d trips %d | weights %s"
          % (N, seed, len(loops), with_false, float(np.hypot(*(poses[-1, :2] - H.eight_truth(N)[-1, :2]))), ref["mu0"], ref["levels"],
             ref["iterations"], ref["trips"], np.round(ref["weights"][rb], 4)))
    assert ref["converged"] and ref["mu0"] > 100.0 and ref["levels"] > 10
    assert (ref["rejected"][rb] == bad[rb]).all()
    assert (ref["weights"][rb & ~bad] >= 0.9).all() and (ref["weights"][bad] < 1e-6).all()
    assert (ref["weights"][~rb] == 1.0).all()
    plain = R.oracle_optimize_robust(poses, edges, phi, mu0=1.0)
    assert plain["levels"] == 1 and plain["mu0"] == 1.0
    assert (plain["rejected"] & ~bad).any()


@pytest.mark.parametrize("name", sorted(R.ROBUST_WORKLOADS))
def test_every_compared_decision_is_far_from_a_tie(name):
    """A condition on the inputs of the GPU comparisons, not a tolerance: where a level ends on eps_level, whether a trial is
    accepted (against the change its step predicts), c > phi at the end and the step against eps_step at mu = 1 all have a
    relative margin of MARGIN_MIN and more, and every trial changes F_mu by TRIAL_F_MIN of itself and more."""
    poses, edges, phi, bad, ref = R.robust_workload(name)
    m = ref["margins"]
    print("robust workload %s: N %d E %d | mu0 %.6g levels %d steps %d trips %d converged %d | margins level %.3g trial %.3g (of F %.3g) "
          "reject %.3g step %.3g" % (name, len(poses), len(edges), ref["mu0"], ref["levels"], ref["iterations"], ref["trips"], ref["converged"],
                                     min(m["level"], default=np.inf), min(m["trial"]), min(m["trial_f"]), min(m["reject"]), min(m["step"])))
    assert ref["converged"] and ref["trips"] < 200
    assert R.smallest_margin(ref) >= R.MARGIN_MIN
    assert min(m["trial_f"]) >= R.TRIAL_F_MIN
    rb = phi > 0
    assert (ref["rejected"][rb] == bad[rb]).all()


def test_the_shapes_the_gpu_tests_need():
    """Two and four nodes, N = 24, 65 and 257, and arc lists of 127, 128 and 129 arcs around the key array's power of two."""
    sizes = {name: (len(R.robust_workload(name)[0]), len(R.robust_workload(name)[1])) for name in R.ROBUST_WORKLOADS}
    assert sizes["two"] == (2, 1) and sizes["four"] == (4, 5)
    assert {n for n, _ in sizes.values()} >= {24, 65, 257}
    assert [sizes[k][1] for k in ("p127", "p128", "p129")] == [127, 128, 129]


@pytest.mark.parametrize("name", ["far24a", "far65"])
def test_without_robust_arcs_it_is_the_halving_oracle(name):
    """The same iterates, bit for bit, over the steps whose decisions are not at the rounding of F (far_workload's compared
    steps: the two oracles sum F in different orders), and the same end within eps_step."""
    poses, edges, ref, n_cmp = H.far_workload(name)
    assert n_cmp >= 3
    for mu0 in (0.0, 1.0, 50.0):
        got = R.oracle_optimize_robust(poses, edges, np.zeros(len(edges)), mu0=mu0, eps_step=1e-12, max_iter=30)
        assert got["mu0"] == 1.0 and got["levels"] == 1 and got["mus"] == [1.0] * got["trips"]
        for k in range(n_cmp):
            assert got["iterates"][k].tobytes() == ref["iterates"][k].tobytes(), (name, k)
            assert got["steps"][k] == ref["steps"][k]
        assert H.pose_error(got["poses"], ref["poses"]) < (1e-9, 1e-9)
        assert abs(got["cost_initial"] - ref["costs"][0]) <= 1e-12 * ref["costs"][0] and (got["weights"] == 1.0).all()


def test_mu0_is_twice_the_largest_ratio_clipped():
    poses, edges, phi, bad = R.drifted(24, 2, 1.0, R.loop_sets(24)[1], [R.false_arc(24)])
    x = np.array(poses)
    x[:, 2] *= H.DEG
    c = R.arc_chi2(x, edges)
    assert R.auto_mu0(x, edges, phi) == 2.0 * (c[phi > 0] / phi[phi > 0]).max()
    assert R.auto_mu0(x, edges, np.where(phi > 0, 1e-12, 0.0)) == R.MU_MAX
    assert R.auto_mu0(x, edges, np.where(phi > 0, 1e12, 0.0)) == 1.0 and R.auto_mu0(x, edges, np.zeros(len(phi))) == 1.0


def records(rows):
    from ndt_slam_amd import capi
    rec = np.zeros(len(rows), dtype=capi.PG_ROBUST_RESULT_DTYPE)
    for k, (status, converged) in enumerate(rows):
        rec[k]["pg"]["status"], rec[k]["pg"]["converged"] = status, converged
    return rec


def test_robust_keep():
    from ndt_slam_amd import replay
    # four graphs of three arcs each (two odometry arcs, phi 0, then ... ) but the last, which has two loop arcs
    phi = np.array([0, 0, 9.0, 0, 0, 9.0, 0, 0, 9.0, 0, 9.0, 9.0])
    chi2 = np.array([50.0, 1, 100.0, 1, 1, 2.0, 1, 1, 2.0, 1, 400.0, 9.0])
    eoff = np.array([0, 3, 6, 9, 12], dtype=np.uint64)
    keep = replay.robust_keep(records([(0, 1), (0, 1), (-1, 0), (0, 1)]), chi2, phi, eoff)
    # all rejected (a large chi2 on a PLAIN arc does not count either way); one kept; a failed graph; one of two kept, at chi2 == phi
    assert keep.dtype == bool and keep.tolist() == [False, True, False, True]
    assert replay.robust_keep(records([(0, 0)]), [1.0, 1.0], [9.0, 9.0], [0, 2]).tolist() == [False]          # not converged
    assert replay.robust_keep(records([(0, 1)]), [1.0, 1.0], [0.0, 0.0], [0, 2]).tolist() == [False]          # no robust arc at all
    assert replay.robust_keep(records([(0, 1)]), [], [], [0, 0]).tolist() == [False]                          # no arc
    with pytest.raises(ValueError):
        replay.robust_keep(records([(0, 1)]), [1.0], [9.0, 9.0], [0, 2])
    with pytest.raises(ValueError):
        replay.robust_keep(records([(0, 1)]), [1.0], [9.0], [0, 1, 1])


def test_loop_closure_keeps_its_tuple_and_gains_robust():
    from ndt_slam_amd import replay
    lc = replay.LoopClosure(None, None, None, 1, 2)
    assert lc.robust is None and len(lc) == 5 and lc._fields == ("loop", "pg", "odo_info", "every", "cooldown")
    rc = replay.RobustClosure(params=None, phi=9.0)
    assert replay.LoopClosure(None, None, None, 1, 2, robust=rc).robust is rc and rc.phi == 9.0


def test_close_loops_gives_phi_to_the_loop_arcs_alone(monkeypatch):
    """_optimize_closing: phi on the last n_loop_arcs[g] arcs of every graph, 0 on the odometry arcs, the decision robust_keep's."""
    from ndt_slam_amd import capi, replay
    seen = {}

    def fake(ctx, poses, noff, edges, eoff, phi, params):
        seen["phi"], seen["params"] = np.array(phi), params
        chi2 = np.where(phi > 0, 1.0, 5.0)
        chi2[-1] = 100.0                                                  # graph 1's only loop arc is rejected
        return poses + 1.0, records([(0, 1), (0, 1)]), np.ones(len(edges)), chi2

    monkeypatch.setattr(capi, "optimize_pose_graphs_robust", fake)
    monkeypatch.setattr(capi, "optimize_pose_graphs", lambda *a: pytest.fail("the plain optimiser was called"))
    lc = replay.LoopClosure(None, "unused", None, 1, 2, robust=replay.RobustClosure(params="prm", phi=7.5))
    edges = np.zeros(9, dtype=capi.PG_EDGE_DTYPE)
    new, good = replay._optimize_closing(None, lc, np.zeros((6, 3)), np.array([0, 3, 6], dtype=np.uint64), edges,
                                         np.array([0, 5, 9], dtype=np.uint64), [2, 1])
    assert seen["phi"].tolist() == [0, 0, 0, 7.5, 7.5, 0, 0, 0, 7.5] and seen["params"] == "prm"
    assert good.tolist() == [True, False] and (new == 1.0).all()
