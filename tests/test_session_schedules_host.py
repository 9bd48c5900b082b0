"""tests/session_schedules.py on the host: every schedule of the table reaches what its row says, on replay.PointCloudMap's
bookkeeping alone with the logs' odometry as the poses (the device run, tests/test_gpu_session_schedules.py, must show the same
closed submaps, splits and candidates on the composed chain).  These are conditions on the schedules, not measurements."""
import numpy as np
import pytest

import session_schedules as SS
from loops_helpers import FULL_LAP
from session_correct_helpers import smooth_adjustment
from session_remake_helpers import scan_lists

_EVENTS = {}


def events(name):
    if name not in _EVENTS:
        _EVENTS[name] = SS.simulate(SS.BY_NAME[name])
    return _EVENTS[name]


def ops(name, kind=None):
    return [e for e in events(name) if e["kind"] != "step" and (kind is None or e["kind"] == kind)]


def splits_between(name, a, b, i):
    """Whether session i splits at a step between the events a and b of the schedule."""
    ev = events(name)
    lo, hi = ev.index(a), ev.index(b)
    return any(e["kind"] == "step" and i in e["split"] for e in ev[lo:hi])


def no_step_between(name, a, b):
    ev = events(name)
    return not any(e["kind"] == "step" for e in ev[ev.index(a):ev.index(b)])


def own_closed(i, k):
    """Workload A without overrides: a session splits at its own steps 3, 6 and 9."""
    n = SS.SPECS_A[i][1]
    return min(max(min(k, SS.STARTS_A[i] + n - 1) - SS.STARTS_A[i], 0) // 3, 3)


@pytest.mark.parametrize("name", [s.name for s in SS.SCHEDULES if s.name != "idle_and_refused"])
def test_closed_submaps_layouts_and_candidates_at_every_op(name):
    seen = ops(name)
    assert seen and len(seen) == len([1 for k, _ in SS.BY_NAME[name].ops if k <= 11])
    for e in seen:
        for i in e["who"]:
            assert e["n_closed"][i] == own_closed(i, e["k"]), (name, e["k"], e["kind"], i)
            firsts, anchors, store_first = e["layout"][i]
            n, c = e["n_scans"][i], e["n_closed"][i]
            assert n == min(e["k"] - SS.STARTS_A[i] + 1, SS.SPECS_A[i][1])
            assert firsts == [0, 3, 6, 9][:c + 1]
            lasts = firsts[1:] + [n]
            assert anchors == [a + (b - 1 - a) // 2 for a, b in zip(firsts, lasts)]
            assert store_first == (firsts[-1] - 2 if c else 0)          # (the two carried scans lie in front of the submap's own)
        if e["kind"] == "search":
            assert sorted(e["cand"]) == [i for i in e["who"] if e["n_closed"][i] >= 2], (name, e["k"])
            assert all(c["submap"] <= e["n_closed"][i] - 2 for i, c in e["cand"].items())


def test_twice_has_a_split_and_a_second_closed_cloud_between_its_corrections():
    a, b = ops("twice", "correct")
    assert (a["k"], b["k"]) == (4, 8) and a["who"] == b["who"] == [0, 2]
    assert a["n_closed"] == {0: 1, 2: 1} and b["n_closed"] == {0: 2, 2: 2}
    assert all(splits_between("twice", a, b, i) for i in (0, 2))
    assert SS.BY_NAME["twice"].rm_too


def test_back_to_back_changes_arenas_five_times_without_a_step():
    seen = ops("back_to_back")
    assert [e["kind"] for e in seen] == ["correct", "correct", "correct", "remake", "remake", "correct"]
    assert [e["who"] for e in seen] == [[0], [2], [0, 1], [0, 2], [0, 2], [1]]
    assert no_step_between("back_to_back", seen[0], seen[-1])
    assert all(n == 2 for e in seen for n in e["n_closed"].values())
    # somebody is un-named at every call, and every session is un-named at one of them
    assert all(len(e["who"]) < 3 for e in seen) and set().union(*[set(range(3)) - set(e["who"]) for e in seen]) == {0, 1, 2}


def test_remake_then_correct_starts_behind_the_first_submap_and_remakes_three_after_two():
    c1, r1, c2, r2 = ops("remake_then_correct")
    assert [e["kind"] for e in (c1, r1, c2, r2)] == ["correct", "remake", "correct", "remake"]
    assert no_step_between("remake_then_correct", c1, r1) and r1["n_closed"] == {0: 2, 2: 2} and r2["n_closed"] == {0: 3, 2: 3}
    assert all(splits_between("remake_then_correct", c2, r2, i) for i in (0, 2))
    for i in (0, 2):
        firsts, _, _ = c2["layout"][i]
        start = c2["start"][i]
        assert start == firsts[1] == 3
        first, last = scan_lists(firsts, c2["n_scans"][i])[0]
        assert (first, last) == (0, start - 1)                           # every scan of L_0 lies in front of `start` ...
        old = np.arange(3.0 * c2["n_scans"][i]).reshape(-1, 3)
        new = smooth_adjustment(old, 1.0, start)
        assert new[:start].tobytes() == old[:start].tobytes() and (new[start:] != old[start:]).all()      # ... and keeps its pose
    assert SS.BY_NAME["remake_then_correct"].rm_too


def test_rotating_names_meets_every_session_in_another_phase():
    seen = ops("rotating_names")
    assert [(e["k"], e["kind"], e["who"]) for e in seen] == [(5, "correct", [0]), (6, "correct", [1]), (7, "remake", [0, 1, 2]),
                                                             (8, "correct", [2]), (8, "remake", [2]), (9, "correct", [0, 1, 2])]
    assert seen[2]["n_closed"] == {0: 2, 1: 2, 2: 2} and seen[-1]["n_closed"] == {0: 3, 1: 3, 2: 2}
    held = [e["n_scans"][i] - e["layout"][i][2] for e in seen[-1:] for i in e["who"]]
    assert len(set(held)) >= 2                                          # the late session holds another number of scans


def test_search_between_searches_a_moved_and_then_a_resized_cloud_twice():
    seen = ops("search_between")
    assert [e["kind"] for e in seen] == ["search", "correct", "search", "remake", "search"] * 2
    assert [e["k"] for e in seen] == [8] * 5 + [10] * 5
    assert all(sorted(e["cand"]) == [0, 1, 2] for e in seen if e["kind"] == "search")
    # the candidate is another submap at the second visit: the loop map is rebuilt over another cloud
    assert {c["submap"] for e in seen[:5] if e["kind"] == "search" for c in e["cand"].values()} == {0}
    assert {c["submap"] for e in seen[5:] if e["kind"] == "search" for c in e["cand"].values()} == {1}


def test_idle_and_refused_leaves_one_session_idle_and_one_a_scan_short():
    ev = events("idle_and_refused")
    steps = {e["k"]: e for e in ev if e["kind"] == "step"}
    assert all(1 not in steps[k]["stepped"] for k in (5, 6, 7)) and 1 in steps[4]["stepped"] and 1 in steps[8]["stepped"]
    assert 2 not in steps[6]["stepped"] and 2 in steps[5]["stepped"] and 2 in steps[7]["stepped"]
    c1, r1, g1, c2 = ops("idle_and_refused")
    assert (c1["k"], r1["k"], g1["k"], c2["k"]) == (7, 8, 8, 9) and g1["kind"] == "occ_rebuild"
    assert c1["n_closed"] == {0: 2, 1: 1, 2: 2} and r1["n_closed"] == {0: 2, 1: 2, 2: 2}
    # session 1 is corrected while idle (its views are carried ones); session 2 is one scan behind its steps
    assert c1["n_scans"] == {0: 8, 1: 5, 2: 6} and r1["n_scans"] == {0: 9, 1: 6, 2: 7}
    assert c1["layout"][2][0] == [0, 3, 5] and r1["layout"][1][0] == [0, 3, 5]


def test_every_step_refills_the_prefix_behind_every_step():
    seen = ops("every_step")
    assert [e["kind"] for e in seen] == ["occ_integrate", "correct", "remake", "occ_rebuild", "search"] * 11
    assert [e["k"] for e in seen[::5]] == list(range(1, 12))
    assert sum(len(e["cand"]) for e in seen if e["kind"] == "search") >= 3
    scales = [op.scale for _, op in SS.BY_NAME["every_step"].ops if op.kind == "correct"]
    assert all(a == -b and abs(a) == 0.3 for a, b in zip(scales, scales[1:]))


def test_grid_without_clear_integrates_at_every_step_and_rebuilds_twice_on_top():
    seen = ops("grid_without_clear")
    assert [e["k"] for e in seen if e["kind"] == "occ_integrate"] == list(range(12))
    assert [(e["k"], e["kind"]) for e in seen if e["kind"] != "occ_integrate"] == [(5, "correct"), (5, "occ_rebuild"), (9, "correct"), (9, "occ_rebuild")]
    assert all(op.clear == 0 for _, op in SS.BY_NAME["grid_without_clear"].ops if op.kind == "occ_rebuild")


def test_long_jump_moves_the_last_pose_far_enough_to_move_a_split_if_the_old_one_were_kept():
    """The travelled distance goes on from the corrected last pose, so the splits stay at the sessions' steps 3, 6 and 9 (the
    generic test above).  Measured from the pose the correction replaced, the next step alone would close the submap."""
    c, r = ops("long_jump")
    assert (c["kind"], c["k"], r["kind"], r["k"]) == ("correct", 4, "remake", 7)
    odo = SS.logs_a()[0][1]                                              # (session 2 stands at its own split step)
    n = c["n_scans"][0]
    new = smooth_adjustment(odo[:n], -8.0)
    jump, step = new[n - 1, :2] - odo[n - 1, :2], odo[n, :2] - odo[n - 1, :2]
    since_split = sum(np.hypot(*(odo[j + 1, :2] - odo[j, :2])) for j in range(3, n - 1))
    assert n == 5 and since_split + np.hypot(*step) < 1.5 <= since_split + np.hypot(*(step + jump))
    assert all(splits_between("long_jump", c, r, i) for i in (0, 2))


def test_failed_then_named_again_sends_a_scan_that_is_no_anchor_and_not_stored():
    seen = ops("failed_then_named_again")
    bad = seen[0]
    firsts, anchors, store_first = bad["layout"][0]
    assert bad["kind"] == "correct_to" and bad["n_closed"] == {0: 2} and 0 not in anchors and store_first > 0
    assert SS.far_first_scan(np.zeros((4, 3)))[:, 0].tolist() == [1e8, 0, 0, 0]
    assert all(0 not in e["who"] for e in seen[2:] if e["kind"] != "search")
    assert [e["k"] for e in seen if e["kind"] == "search"] == [8, 9] and all(2 in e["cand"] and 1 in e["cand"] for e in seen if e["kind"] == "search")


def test_the_lap_has_a_candidate_at_every_search_and_a_split_behind_the_first():
    ev = SS.simulate_lap()
    searches = [e for e in ev if e["kind"] == "search"]
    assert [e["k"] for e in searches] == list(range(FULL_LAP - 1, SS.N_FRAMES_B))
    assert all(sorted(e["cand"]) == [0, 1] for e in searches)
    assert any(e["kind"] == "step" and e["k"] > FULL_LAP - 1 and e["split"] == [0, 1] for e in ev)
    assert SS.N_FRAMES_B <= 80
