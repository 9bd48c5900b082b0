"""Resident session sets across maintenance schedules (tests/session_schedules.py): ndt_sessions_correct, _remake_closed,
_find_loops, _occ_integrate and _occ_rebuild called repeatedly, back to back and in every order a front end would, the set
held byte for byte to the composed chain behind every step and every call -- both views, the map's export, the global map
with its parts, the trajectory and its layout, the archive, the candidates, every ndt_loop and record, the grids' counters and
stats -- and the host waits of every call to two.  The header's claim that a remake depends on archive, trajectory and
parameters alone is held on two sets with different histories.  There is no tolerance in this module."""
import time

import numpy as np
import pytest

import occ_helpers as H
import occ_rebuild_helpers as R
import session_schedules as SS
from loops_helpers import FULL_LAP
from session_correct_helpers import smooth_adjustment
from session_helpers import lockstep, same_records
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = [(s.name, 1) for s in SS.SCHEDULES] + [(s.name, 0) for s in SS.SCHEDULES if s.rm_too]
_T0, _RUNS = [None], {}


def run_cached(gpu, name, rm=1):
    """The schedule's log; a schedule runs once per module however many tests read its log."""
    if _T0[0] is None:
        _T0[0] = time.perf_counter()
    if (name, rm) not in _RUNS:
        capi, ctx = gpu
        _RUNS[(name, rm)] = SS.run_lap(capi, ctx) if name == "lap" else SS.run(SS.BY_NAME[name], capi, ctx, rm)
    return _RUNS[(name, rm)]


def held_to_the_host_model(log, want, loose_from=None):
    """The run's log against session_schedules.simulate: the same steps, splits, ops, closed submaps and candidates."""
    assert [(e["kind"], e["k"]) for e in log] == [(e["kind"], e["k"]) for e in want]
    for got, ref in zip(log, want):
        tag = (got["kind"], got["k"])
        if got["kind"] == "step":
            assert got["split"] == ref["split"] and got["stepped"] == ref["stepped"], tag
            continue
        assert got["who"] == ref["who"], tag
        if "n_closed" in got:
            assert got["n_closed"] == ref["n_closed"], tag
        if got["kind"] in ("correct", "correct_to"):
            assert got["layout"] == ref["layout"] and got["n_scans"] == ref["n_scans"], tag
        if got["kind"] == "search":
            skip = set() if loose_from is None else {loose_from}
            assert sorted(got["cand"]) == sorted(set(ref["cand"]) - skip), tag
            assert all(got["cand"][i]["submap"] == ref["cand"][i]["submap"] for i in got["cand"]), tag


@pytest.mark.parametrize("name,rm", CASES)
def test_the_set_equals_the_chain_behind_every_step_and_every_call(gpu, name, rm):
    log = run_cached(gpu, name, rm)
    held_to_the_host_model(log, SS.simulate(SS.BY_NAME[name]), 0 if name == "failed_then_named_again" else None)
    ops = [e for e in log if e["kind"] != "step"]
    # no test passes by doing nothing (all of it on the chain: Runner.correct and Runner.remake assert the rest)
    for e in ops:
        if e["kind"] == "correct":
            assert all(any(e["moved"][i]) for i in e["who"] if e["n_closed"][i]), (name, e["k"])
    remakes = [e for e in ops if e["kind"] == "remake"]
    if name == "back_to_back":
        first, second = remakes
        assert all(any(first["changed"][i]) for i in (0, 2)) and not any(any(second["changed"][i]) for i in (0, 2))
    if name == "remake_then_correct":
        assert all(len(remakes[0]["changed"][i]) == 2 and len(remakes[1]["changed"][i]) == 3 for i in (0, 2))
        moved = [e for e in ops if e["kind"] == "correct"][1]["moved"]
        assert all(moved[i] == [False, True] for i in (0, 2))             # start = sub_first[1]: the first closed cloud keeps its bytes
    if name == "failed_then_named_again":
        capi, _ = gpu
        assert remakes[0]["status"] == {0: capi.NDT_E_ARG, 2: capi.NDT_OK}
        assert all(e["status"] == {2: capi.NDT_OK} and any(e["changed"][2]) for e in remakes[1:])
    if name == "grid_without_clear":
        beams = [e["stats"][0] for e in ops if e["kind"] == "occ_rebuild"]
        assert len(beams) == 2 and beams[1] > beams[0] > 0


def test_the_searches_of_workload_a_had_candidates_to_refine(gpu):
    """Over the searches of search_between, every_step and failed_then_named_again the composed reference picked at least one
    lattice pose (n_cand >= 1) three times or more: the sweeps, picks and matches ran on corrected and remade clouds."""
    n_cand = [n for name in ("search_between", "every_step", "failed_then_named_again")
              for e in run_cached(gpu, name) if e["kind"] == "search" for n in e["n_cand"].values()]
    print("workload A: %d searched candidates, n_cand %s" % (len(n_cand), sorted(set(n_cand))))
    assert sum(1 for n in n_cand if n >= 1) >= 3


def test_the_lap_searched_optimised_corrected_remade_and_rebuilt_behind_every_step(gpu):
    log = run_cached(gpu, "lap")
    steps = [e for e in log if e["kind"] == "step"]
    searches = [e for e in log if e["kind"] == "search"]
    corrections = [e for e in log if e["kind"] == "correct"]
    found_at = sorted({e["k"] for e in searches if any(e["found"].values())})
    print("the lap: loops found behind the steps %s, corrections behind %s, splits %s"
          % (found_at, [(e["k"], e["who"]) for e in corrections], [(e["k"], e["split"]) for e in steps if e["split"]]))
    assert [e["k"] for e in searches] == list(range(FULL_LAP - 1, SS.N_FRAMES_B))
    assert len(found_at) >= 2 and len(corrections) >= 2
    assert any(e["split"] for e in steps if e["k"] > corrections[0]["k"])          # a split follows the first correction
    assert any(e["kind"] == "remake" and any(any(c) for c in e["changed"].values()) for e in log)
    # a search whose candidate map is a remade cloud: a candidate behind the first remake
    first_remake = next(j for j, e in enumerate(log) if e["kind"] == "remake")
    assert any(e["kind"] == "search" and e["cand"] for e in log[first_remake:])
    # the same steps, splits and candidates as the host model (which leaves the corrections out)
    want = [e for e in SS.simulate_lap()]
    held_to_the_host_model([e for e in log if e["kind"] in ("step", "search")], want)


def test_a_remade_set_does_not_depend_on_its_history(gpu):
    """Two sets stepped to k = 8 together.  X: the trajectory C, a remake.  Y: a correction, a remake, another correction from
    scan 3 on, then C and a remake.  Closed clouds, the local maps' first parts, trajectories, layouts, archives, candidates and
    rebuilt grids are the same bytes; the current submap's float32 points were re-posed once in X and three times in Y, and
    nothing is claimed for them."""
    capi, ctx = gpu
    logs, p = SS.logs_a(), SS.params_a()
    S = len(logs)
    X, Y = (capi.Sessions(ctx, S, capi.session_params_from_launch(p), archive=True) for _ in range(2))
    for k, scans, odo, act in lockstep(logs, SS.STARTS_A):
        a, b = X.step(scans, odo, act), Y.step(scans, odo, act)
        assert all(same_records(x, y) for x, y in zip(a, b)), k
        if k == 8:
            break
    who, ok = [0, 2], {0: capi.NDT_OK, 2: capi.NDT_OK}
    common = {i: X.trajectory(i)[0] for i in who}
    assert all(common[i].tobytes() == Y.trajectory(i)[0].tobytes() for i in who)
    C = {i: smooth_adjustment(common[i], 1.0) for i in who}
    before = {i: [x.copy() for x in X.global_map(i)[1]] for i in who}
    assert X.correct(C) == ok and X.remake_closed(who) == ok
    assert Y.correct({i: smooth_adjustment(Y.trajectory(i)[0], 0.4) for i in who}) == ok and Y.remake_closed(who) == ok
    assert Y.correct({i: smooth_adjustment(Y.trajectory(i)[0], -0.2, 3) for i in who}) == ok
    assert Y.correct(C) == ok and Y.remake_closed(who) == ok
    lp = SS.loop_params_a(capi)
    flags = np.array([1, 0, 1], np.uint8)
    assert X.loop_candidates(lp, flags).tobytes() == Y.loop_candidates(lp, flags).tobytes() and len(X.loop_candidates(lp, flags)) == 2
    gx, gy = ([capi.OccGrid(ctx, SS.GEOM_A) for _ in range(S)] for _ in range(2))
    sx, sy = X.occ_rebuild(gx, flags, clear=True), Y.occ_rebuild(gy, flags, clear=True)
    assert H.stats_tuple(sx) == H.stats_tuple(sy) and sx["n_hit"] > 0
    for i in who:
        px, py = X.global_map(i)[1], Y.global_map(i)[1]
        assert len(px) == len(py) == 3 and all(len(x) for x in px[:-1])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(px[:-1], py[:-1])), i
        assert all(x.tobytes() != y.tobytes() for x, y in zip(px[:-1], before[i][:-1])), i          # (the remake was no no-op)
        n_prev = len(px[-2])
        tx, ty = R.views(X, i)[0], R.views(Y, i)[0]
        assert len(tx) > n_prev and tx[:n_prev].tobytes() == ty[:n_prev].tobytes() == px[-2].tobytes(), i
        a, b = X.trajectory(i), Y.trajectory(i)
        assert a[0].tobytes() == b[0].tobytes() == C[i].tobytes() and a[1].tolist() == b[1].tolist() and a[2].tolist() == b[2].tolist() and a[3] == b[3]
        assert X.archive_info(i) == Y.archive_info(i)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(X.archive_scans(i), Y.archive_scans(i)))
        assert R.grid_bytes(gx[i]) == R.grid_bytes(gy[i]), i
    for g in gx + gy:
        g.close()
    X.close(); Y.close()


def test_wall_time_of_the_module(gpu):
    """Prints the time from the module's first schedule to here (LOG.md keeps the figure measured on an MI355X)."""
    if _T0[0] is None:
        _T0[0] = time.perf_counter()
    print("tests/test_gpu_session_schedules.py: %.1f s from the first schedule to the last test, %d schedules run"
          % (time.perf_counter() - _T0[0], len(_RUNS)))
