"""tests/session_workloads.py without a GPU: every family's certificate holds on the oracle stand-in (OracleSessions), so
the inputs alone -- not a device's arithmetic -- carry a run into the branches the family is named after; the census
itself is checked by hand on a tiny log; span_outlier's two CPU certificates."""
import numpy as np
import pytest

import session_workloads as W
from session_helpers import OracleSessions, to_map_frame


def _names(families):
    return [v["name"] for v in W.variants(families)]


@pytest.mark.parametrize("name", _names([f for f in W.FAMILIES]))
def test_family_reaches_its_branches_on_the_oracle(oracle, name):
    from ndt_slam_amd import capi
    v = W.variant(name)
    # (the stand-in's per-session rules throughout: its strict form builds a map of every local map, an empty one too)
    model = OracleSessions(oracle, capi, len(v["logs"]), v["p"], allow_item_failures=True)
    history, records = W.run_model(model, v["logs"], v["starts"])
    census = W.session_census(history, records)
    print(name, {k: {a: b for a, b in c.items() if b} for k, c in census.items()})
    assert len(v["logs"]) <= 4 and len(records) <= 12
    if not v["tolerant"]:                               # nothing is refused: the strict chain can run the family on the device
        assert all(census[i]["refused_builds"] == census[i]["refused_triples"] == 0 for i in range(len(v["logs"])))
    assert not W.certificate_misses(census, v["certificate"]), (W.certificate_misses(census, v["certificate"]), census)


def test_every_family_of_the_issue_is_in_the_table():
    assert set(W.FAMILIES) == {"split_at_first_pose", "split_without_carry", "split_every_other", "empty_first",
                               "empty_at_split", "empty_oldest_of_triple", "two_empties_running", "all_empty_step",
                               "no_map_yet", "bad_first_scan", "grid_outlier", "span_outlier"}
    for f in ("empty_first", "empty_at_split", "empty_oldest_of_triple", "two_empties_running", "grid_outlier"):
        assert {v["p"]["removeMoving"] for v in W.FAMILIES[f]} == {False, True}, f
    assert all(v["certificate"] for v in W.variants())
    logs, starts, cls = W.many_sessions()
    assert len(cls) == W.MANY_S > 1024 and set(cls) == set(range(len(logs))) and set(starts) == {0, 1}
    assert len({sum(len(x) for x in scans) for scans, _ in logs}) > 1        # class lengths differ
    assert len({c for c in cls[1024:]}) > 1 and max(len(s) + st for (s, _), st in zip(logs, starts)) == 4


def _rec(stepped=1, matched=1, status=0, split=0):
    r = np.zeros(1, dtype=[("stepped", "i4"), ("matched", "i4"), ("status", "i4"), ("split", "i4")])[0]
    r["stepped"], r["matched"], r["status"], r["split"] = stepped, matched, status, split
    return r


def _snap(scan_ns, closed_ns=(), t_n=5, had_map=True, rm=True):
    return dict(scan_ns=list(scan_ns), closed_ns=list(closed_ns), t_n=t_n, had_map=had_map, remove_moving=rm)


def test_census_by_hand():
    """One session and a neighbour, eight steps, removeMoving on, written down rather than run:

      k  record (session 0)              submap's scans after the step      what the census must count
      0  skipped, status -1              -                                  skipped_scans
      1  first scan, empty               [0]              t_n 0             first_scans, first_scan_after_skip, empty_scans,
                                                                            empty_first_scan, steps_t_n_0
      2  matched, had no map             [0, 7]                             matched_without_map
      3  matched                         [0, 7, 9]                          triples_run, triples_empty_oldest
      4  matched, empty scan             [0, 7, 9, 0]                       triples_run, triples_empty_newest, empty_scans
      5  matched, split (held 4)         [9, 0, 6]        closed [0]        splits, split_held_2plus, closed_empty,
                                                                            triples_empty_middle
      6  matched, status -4              [9, 0, 6, 8]                       triples_run, triples_empty_oldest, refused_builds,
                                                                            first_refused_step 6
      7  matched, OK                     [9, 0, 6, 8, 3]                    triples_run, recoveries, ok_after_recovery

    The neighbour steps at 1 (first scan, with points) and 2 (matched, with a map), and splits at step 2 holding one scan:
    step 1 is no all-empty step (its scan has points), step 2 is a mixed-map step; at step 4 session 0 steps alone with an
    empty scan: the one all-empty step."""
    s0 = [(_rec(0, 0, -1), _snap([], t_n=0, had_map=False)),
          (_rec(1, 0), _snap([0], t_n=0, had_map=False)),
          (_rec(), _snap([0, 7], had_map=False)),
          (_rec(), _snap([0, 7, 9])),
          (_rec(), _snap([0, 7, 9, 0])),
          (_rec(split=1), _snap([9, 0, 6], closed_ns=[0])),
          (_rec(status=-4), _snap([9, 0, 6, 8], closed_ns=[0])),
          (_rec(), _snap([9, 0, 6, 8, 3], closed_ns=[0]))]
    idle = (_rec(0, 0), _snap([4], closed_ns=[3]))
    s1 = [(_rec(0, 0), _snap([], had_map=False)), (_rec(1, 0), _snap([4], had_map=False)),
          (_rec(split=1), _snap([4], closed_ns=[3]))] + [idle] * 5
    records = [[a[0], b[0]] for a, b in zip(s0, s1)]
    history = [[a[1], b[1]] for a, b in zip(s0, s1)]
    c = W.session_census(history, records)
    want0 = dict(splits=1, split_held_0=0, split_held_1=0, split_held_2plus=1, closed_empty=1, triples_run=4,
                 triples_empty_middle=1, triples_empty_oldest=2, triples_empty_newest=1, empty_scans=2, empty_first_scan=1,
                 empty_at_split=0, steps_t_n_0=1, matched_without_map=1, first_scans=1, skipped_scans=1,
                 first_scan_after_skip=1, refused_builds=1, refused_triples=0, first_refused_step=6, recoveries=1,
                 ok_after_recovery=1)
    assert c[0] == want0, {k: (c[0][k], want0[k]) for k in want0 if c[0][k] != want0[k]}
    assert (c[1]["splits"], c[1]["split_held_1"], c[1]["first_scans"], c[1]["closed_empty"]) == (1, 1, 1, 0)
    assert c[1]["first_refused_step"] == -1 and c[1]["recoveries"] == 0
    assert c["set"] == dict(all_empty_steps=1, first_all_empty_step=4, mixed_map_steps=1, nomap_only_steps=0), c["set"]
    assert W.certificate_misses(c, {0: dict(splits=("==", 1), triples_run=4), "set": dict(mixed_map_steps=1)}) == []
    assert W.certificate_misses(c, {0: dict(splits=("==", 2), triples_run=5)}) == [(0, "splits", ("==", 2), 1),
                                                                                (0, "triples_run", 5, 4)]


def test_span_outlier_refuses_exactly_the_triples_that_hold_scan_j(oracle):
    """Under score_thre = -1 the poses are the odometry predictions (read from a clean oracle run).  Of the submap's triples
    (k - 2, k - 1, k), oracle.make_map refuses exactly k = j, j + 1, j + 2; and in the map frame the outlier stays within
    2^31 leaves of the origin, where the pre-filter's voxel index is defined."""
    from ndt_slam_amd import capi, replay
    v = W.variant("span_outlier")
    p, j = v["p"], W.SPAN_SCAN
    clean = W.span_outlier_clean_logs(v)
    model = OracleSessions(oracle, capi, 2, p, allow_item_failures=True)
    _, records = W.run_model(model, clean, v["starts"])
    assert all(r[0]["stepped"] and r[0]["status"] == 0 for r in records)
    scans, n = v["logs"][0][0], len(v["logs"][0][0])
    assert n >= j + 5
    cloud = [np.ascontiguousarray(to_map_frame(replay.resample_points(scans[k], p["space"], p["space_thre"]), records[k][0]["pose"]),
                                  np.float32) for k in range(n)]
    far = [k for k in range(n) if np.abs(cloud[k]).max() > 1e7]
    assert far == [j]                                   # the resampler keeps the point, and nothing is interpolated towards it
    assert np.abs(cloud[j].astype(np.float64) / np.float32(p["LeafSize"])).max() < 2.0 ** 31
    refused = []
    for k in range(2, n):
        try:
            oracle.make_map(cloud[k - 2:k + 1], False, True, True, p["resol"], p["thre_neighbor"])
        except ValueError:
            refused.append(k)
    assert refused == [j, j + 1, j + 2]
