"""Workloads that walk ndt_sessions_step through a submap's life cycle (tests only): named families of small logs with
starts, launch parameters and edits to single scans, the census that says which branches of the step's bookkeeping a run
reached (SsStep::book / front / behind / close, session_plan_kernel: ndt_slam_amd/csrc/ndt_sessions.hip.h), and per
family the counts it must reach -- its certificate.

The logs are synth.replay_records drives (a circle of radius 5 m, 0.6 m of arc per frame; the odometry scales it by
1.015: 0.609 m of travelled distance per step).  Families whose certificate depends on WHICH step splits run with
score_thre = -1: cost <= score_thre never holds, so the fused pose is the odometry prediction and neither a pose nor a
split step depends on a match.  With 0.609 m per step the split steps are then
    sepThre 0      every step, the first included (atd - atdS = 0 >= 0): an empty first submap closes at step 0
    sepThre 0.5    every step from step 1: every submap holds one scan, nothing is carried
    sepThre 1.0    steps 2, 4, 6, ...: every closing submap received two scans of its own (it holds two, or four with the
                   two carried into it), so every split carries and the reset and carry paths run back to back
    sepThre 2.5    steps 5, 10
Those families take 61-beam scans.  At 61 beams no voxel of a Resolution-0.3 map holds enough points for a covariance: a
match "converges" where it starts with H = 0, and fusing it inverts a singular matrix (NaN poses, in the reference's
arithmetic as in every restatement of it) -- so a family that is to accept its matches (score_thre as launched) takes the
181 beams of tests/test_gpu_sessions.py instead.
A variant is a dict: name, logs [(scans, odo)], starts, p (launch parameters), tolerant (run the stand-ins with
allow_item_failures), certificate {session index or "set": {census key: n (at least n) or ("==", n)}}.
"""
import numpy as np

from session_helpers import lockstep, session_logs

EMPTY = np.zeros((0, 2))
GRID_OUTLIER = (8000.0, 8000.0)          # one finite garbage beam: at Resolution 0.3 the local map's box is 5.35e8 cells
SPAN_OUTLIER = (1e8, 0.0)                # 2e9 voxels of resol 0.05 from everything else: beyond the triple's 2^30
SPAN_SCAN = 2                            # span_outlier's scan j
MATCH_BEAMS = 181                        # enough for matches that are accepted (see above)


def launch_params(**kw):
    from ndt_slam_amd import replay
    return dict(replay.LAUNCH_PARAMS, **kw)


def _logs(specs, n_beams=61):
    return [([x.copy() for x in scans], odo.copy()) for scans, odo in session_logs(specs, n_beams=n_beams)]


def _with_point(scan, xy):
    return np.concatenate([scan, np.array([xy], np.float64)])


def _variant(name, logs, p, certificate, starts=None, tolerant=False):
    return dict(name=name, logs=logs, starts=starts or [0] * len(logs), p=p, tolerant=tolerant, certificate=certificate)


def _both(name, make):
    """The variants of make(remove_moving) for removeMoving on and off."""
    return [make("%s[rm=%d]" % (name, rm), bool(rm)) for rm in (1, 0)]


def _split_at_first_pose(name, rm):
    return _variant(name, _logs(((33, 5), (34, 4))), launch_params(sepThre=0.0, score_thre=-1.0, removeMoving=rm),
                    {0: dict(split_held_0=("==", 1), split_held_1=("==", 4), split_held_2plus=("==", 0), closed_empty=1),
                     1: dict(split_held_0=("==", 1), split_held_1=("==", 3))}, starts=[0, 1])


def _split_without_carry(name, rm):
    # removeMoving off: a submap that is not the first and holds one scan has an empty cloud (Submap::makeMap skips what
    # would be the two carried scans), so every local map from step 2 on is empty: t_n == 0 with a map kept
    cert = dict(split_held_0=("==", 0), split_held_1=("==", 5), split_held_2plus=("==", 0))
    if not rm:
        cert.update(closed_empty=3, steps_t_n_0=3)
    return _variant(name, _logs(((33, 6), (35, 5))), launch_params(sepThre=0.5, score_thre=-1.0, removeMoving=rm),
                    {0: cert, 1: dict(split_held_1=("==", 4))})


def _split_every_other(name, rm):
    return _variant(name, _logs(((33, 9), (36, 8))), launch_params(sepThre=1.0, score_thre=-1.0, removeMoving=rm),
                    {0: dict(split_held_0=("==", 0), split_held_1=("==", 0), split_held_2plus=("==", 4)),
                     1: dict(split_held_2plus=("==", 3))}, starts=[0, 1])


def _empty_first(name, rm):
    logs = _logs(((33, 6), (34, 6)), MATCH_BEAMS)
    logs[1][0][0] = EMPTY
    return _variant(name, logs, launch_params(sepThre=2.5, removeMoving=rm),
                    {1: dict(empty_first_scan=("==", 1), matched_without_map=("==", 1), steps_t_n_0=("==", 1)),
                     0: dict(empty_scans=("==", 0), matched_without_map=("==", 0))})


def _empty_at_split(name, rm):
    logs = _logs(((33, 8), (34, 8)))
    logs[0][0][5] = EMPTY                               # sepThre 2.5: step 5 splits
    return _variant(name, logs, launch_params(sepThre=2.5, score_thre=-1.0, removeMoving=rm),
                    {0: dict(empty_at_split=("==", 1), split_held_2plus=("==", 1)), 1: dict(empty_at_split=("==", 0))})


def _empty_oldest_of_triple(name, rm):
    logs = _logs(((33, 6), (34, 6)), MATCH_BEAMS)
    logs[0][0][2] = EMPTY                               # newest at step 2, middle at step 3, oldest at step 4
    cert = dict(empty_scans=("==", 1), splits=("==", 0))
    if rm:
        cert.update(triples_empty_newest=("==", 1), triples_empty_middle=("==", 1), triples_empty_oldest=("==", 1), triples_run=3)
    return _variant(name, logs, launch_params(sepThre=1e9, removeMoving=rm), {0: cert})


def _two_empties_running(name, rm):
    logs = _logs(((33, 7), (34, 7)), MATCH_BEAMS)
    logs[0][0][2] = EMPTY
    logs[0][0][3] = EMPTY
    cert = dict(empty_scans=("==", 2), splits=("==", 0))
    if rm:                                              # steps 3 and 4 skip their triple, step 5's has an empty oldest scan
        cert.update(triples_empty_middle=("==", 2), triples_empty_oldest=("==", 1))
    return _variant(name, logs, launch_params(sepThre=1e9, removeMoving=rm), {0: cert})


def _all_empty_step(name, rm):
    logs = _logs(((33, 6), (34, 5)), MATCH_BEAMS)
    logs[0][0][3] = EMPTY
    logs[1][0][2] = EMPTY                               # (session 1 starts at step 1)
    return _variant(name, logs, launch_params(sepThre=2.5, removeMoving=rm),
                    {"set": dict(all_empty_steps=("==", 1), first_all_empty_step=("==", 3))}, starts=[0, 1])


def _no_map_yet(name, rm):
    logs = _logs(((33, 5), (34, 5), (35, 5)), MATCH_BEAMS)
    logs[1][0][0] = EMPTY
    beside = _variant(name.replace("[", "-beside["), logs, launch_params(sepThre=2.5, removeMoving=rm),
                      {"set": dict(mixed_map_steps=("==", 1)), 1: dict(matched_without_map=("==", 1))})
    alone = _variant(name.replace("[", "-alone["), [logs[1]], launch_params(sepThre=2.5, removeMoving=rm),
                     {"set": dict(nomap_only_steps=("==", 1)), 0: dict(matched_without_map=("==", 1))})
    return [beside, alone]


def _bad_first_scan(name, rm):
    logs = _logs(((33, 5), (34, 5)), MATCH_BEAMS)
    logs[1][0][0][7, 1] = np.inf
    return _variant(name, logs, launch_params(sepThre=2.5, removeMoving=rm),
                    {1: dict(skipped_scans=("==", 1), first_scan_after_skip=("==", 1), first_scans=("==", 1)),
                     0: dict(skipped_scans=("==", 0), first_scans=("==", 1))})


GRID_SESSION, GRID_SCAN = 1, 3


def _grid_outlier(name, rm):
    """sepThre 1.0: scan 3 is the current submap's own at step 3 (the newest scan, or with removeMoving off one of its
    pieces), and lies in the previous submap's closed cloud at steps 4 and 5; the triple (2, 3, 4) drops the lone point
    (removeMoving on) and Submap::makeMap skips the carried scans (off), so from step 6 the local map is free of it."""
    logs = _logs(((33, 10), (34, 10), (35, 8)))
    logs[GRID_SESSION][0][GRID_SCAN] = _with_point(logs[GRID_SESSION][0][GRID_SCAN], GRID_OUTLIER)
    clean = dict(refused_builds=("==", 0), refused_triples=("==", 0))
    v = _variant(name, logs, launch_params(sepThre=1.0, score_thre=-1.0, removeMoving=rm),
                 {GRID_SESSION: dict(refused_builds=("==", 3), first_refused_step=("==", 3), recoveries=("==", 1),
                                     ok_after_recovery=4, refused_triples=("==", 0), matched_without_map=("==", 0)),
                  0: clean, 2: clean}, tolerant=True)
    return dict(v, bad=GRID_SESSION, refused_steps=[3, 4, 5])


def _grid_outlier_first(name, rm, alone):
    """The point in a session's FIRST scan: the session has no map to keep.  Scans 0 and 1 make the first submap, whose
    cloud starts with scan 0 (steps 0, 1), and which is the previous submap at steps 2 and 3: four refused builds, four
    matches without a map (steps 1 .. 4), and at step 4 the session's first map.  `alone`: a set of that session only, so
    that EVERY map of the step's build is refused."""
    logs = _logs(((34, 7),) if alone else ((33, 7), (34, 7)))
    bad = 0 if alone else 1
    logs[bad][0][0] = _with_point(logs[bad][0][0], GRID_OUTLIER)
    cert = {bad: dict(refused_builds=("==", 4), first_refused_step=("==", 0), recoveries=("==", 1), ok_after_recovery=3,
                      matched_without_map=("==", 4))}
    if not alone:
        cert[0] = dict(refused_builds=("==", 0), matched_without_map=("==", 0))
        cert["set"] = dict(mixed_map_steps=("==", 4))
    else:
        cert["set"] = dict(nomap_only_steps=("==", 4))
    v = _variant(name, logs, launch_params(sepThre=1.0, score_thre=-1.0, removeMoving=rm), cert, tolerant=True)
    return dict(v, bad=bad, refused_steps=[0, 1, 2, 3])


def grid_outlier_clean_logs(variant):
    """A grid_outlier set without the outlier session: (logs, starts, original indices)."""
    keep = [i for i in range(len(variant["logs"])) if i != variant["bad"]]
    return [variant["logs"][i] for i in keep], [variant["starts"][i] for i in keep], keep


def _span_outlier():
    logs = _logs(((33, 8), (34, 8)))
    logs[0][0][SPAN_SCAN] = _with_point(logs[0][0][SPAN_SCAN], SPAN_OUTLIER)
    # the stand-ins recompute every triple of the submap, so they refuse every step from j on; the set computes the newest
    # triple alone: three refusals, then it recovers (tests/test_gpu_sessions_lifecycle.py asserts == 3 on its records)
    return _variant("span_outlier", logs, launch_params(sepThre=1e9, score_thre=-1.0, removeMoving=True),
                    {0: dict(refused_triples=3, first_refused_step=("==", SPAN_SCAN), refused_builds=("==", 0), splits=("==", 0)),
                     1: dict(refused_triples=("==", 0))}, tolerant=True)


def span_outlier_clean_logs(variant):
    """span_outlier's logs without the outlier point (under score_thre = -1: the same poses)."""
    logs = [([x.copy() for x in scans], odo.copy()) for scans, odo in variant["logs"]]
    logs[0][0][SPAN_SCAN] = logs[0][0][SPAN_SCAN][:-1]
    return logs


MANY_S = 1030
MANY_CLASSES = ((33, 4, 0), (34, 3, 1), (35, 4, 0), (36, 3, 1), (37, 4, 0), (38, 2, 1), (39, 4, 0), (40, 3, 0), (41, 4, 0),
                (42, 3, 1))                              # (seed, frames, start)


def many_sessions():
    """(class logs, class starts, class of each of the 1030 sessions): session_plan_kernel takes sessions 1024.. in its second
    round, where cloud_off carries the sum of the 1024 clouds before (clouds of ten different lengths)."""
    logs = _logs([(seed, n) for seed, n, _ in MANY_CLASSES], n_beams=31)
    return logs, [s for _, _, s in MANY_CLASSES], [(7 * i + 3) % len(MANY_CLASSES) for i in range(MANY_S)]


FAMILIES = {
    "split_at_first_pose": _both("split_at_first_pose", _split_at_first_pose),
    "split_without_carry": _both("split_without_carry", _split_without_carry),
    "split_every_other": _both("split_every_other", _split_every_other),
    "empty_first": _both("empty_first", _empty_first),
    "empty_at_split": _both("empty_at_split", _empty_at_split),
    "empty_oldest_of_triple": _both("empty_oldest_of_triple", _empty_oldest_of_triple),
    "two_empties_running": _both("two_empties_running", _two_empties_running),
    "all_empty_step": _both("all_empty_step", _all_empty_step),
    "no_map_yet": [v for pair in _both("no_map_yet", _no_map_yet) for v in pair],
    "bad_first_scan": _both("bad_first_scan", _bad_first_scan),
    "grid_outlier": _both("grid_outlier", _grid_outlier)
                    + [_grid_outlier_first("grid_outlier-first[rm=%d]" % rm, bool(rm), False) for rm in (1, 0)]
                    + [_grid_outlier_first("grid_outlier-first-alone[rm=1]", True, True)],
    "span_outlier": [_span_outlier()],
}
CHAIN_FAMILIES = tuple(f for f in FAMILIES if f not in ("grid_outlier", "span_outlier"))


def variants(families=None):
    return [v for f in (families or FAMILIES) for v in FAMILIES[f]]


def variant(name):
    return next(v for v in variants() if v["name"] == name)


# ---- the census ----

def snapshot(model, had_map):
    """PointCloudMap's bookkeeping of every session of a stand-in (OracleSessions, ComposedChain) after a step; had_map: which
    sessions had an NDT map before it."""
    snap = []
    for i, pm in enumerate(model.pcmaps):
        snap.append(dict(scan_ns=[len(x) for x in pm.submaps[-1].scans], closed_ns=[len(s.p_cloud) for s in pm.submaps[:-1]],
                         t_n=len(pm.localMap_cloud), had_map=bool(had_map[i]), remove_moving=bool(model.p["removeMoving"])))
    return snap


def run_model(model, logs, starts):
    """Steps a stand-in through the logs -> (pcmaps_history, records): per step the snapshot and the records."""
    history, records = [], []
    for _, scans, odo, act in lockstep(logs, starts):
        had = [model.has_map(i) for i in range(len(logs))]
        records.append(model.step(scans, odo, act).copy())
        history.append(snapshot(model, had))
    return history, records


PER_SESSION_KEYS = ("splits", "split_held_0", "split_held_1", "split_held_2plus", "closed_empty", "triples_run",
                    "triples_empty_middle", "triples_empty_oldest", "triples_empty_newest", "empty_scans", "empty_first_scan",
                    "empty_at_split", "steps_t_n_0", "matched_without_map", "first_scans", "skipped_scans", "first_scan_after_skip",
                    "refused_builds", "refused_triples", "first_refused_step", "recoveries", "ok_after_recovery")
SET_KEYS = ("all_empty_steps", "first_all_empty_step", "mixed_map_steps", "nomap_only_steps")


def session_census(pcmaps_history, records):
    """Which branches a run reached.  pcmaps_history[k][i]: snapshot() of session i after step k; records[k][i]: its
    ndt_session_step record.  -> {i: counts, "set": counts}.  Per session:
      splits, split_held_0 / _1 / _2plus   splits by the scans the closing submap held (>= 2: two are carried over)
      closed_empty                         splits that closed a submap with an empty cloud
      triples_run / triples_empty_middle   removeMoving: steps at which the submap held >= 3 scans, by whether the middle
                                           scan of the newest triple had points (empty: the triple is skipped)
      triples_empty_oldest / _newest       triples run whose oldest / newest scan was empty
      empty_scans, empty_first_scan, empty_at_split     stepped with a new scan of no points; ... as the first; ... at a split
      steps_t_n_0                          stepped with status OK and an empty local map (no map is built)
      matched_without_map                  matched while the session had no NDT map
      first_scans, skipped_scans, first_scan_after_skip   taken at the odometry pose; status != OK with stepped == 0; a first
                                           scan at a step after a skipped one
      refused_builds / refused_triples     stepped == 1 with status NDT_E_GRID / NDT_E_ARG; first_refused_step: the first (-1)
      recoveries, ok_after_recovery        OK steps right behind a refused one; OK steps behind the last refused one
    The set: all_empty_steps (somebody stepped and every stepped scan was empty; first_all_empty_step, -1: none),
    mixed_map_steps (a session matched without a map while another matched with one), nomap_only_steps (sessions matched,
    none with a map)."""
    S = len(records[0])
    out = {i: dict.fromkeys(PER_SESSION_KEYS, 0) for i in range(S)}
    out["set"] = dict.fromkeys(SET_KEYS, 0)
    out["set"]["first_all_empty_step"] = -1
    for i in range(S):
        c = out[i]
        c["first_refused_step"] = -1
        prev, seen_skip, last_refused, seen_step = None, False, False, False
        for k in range(len(records)):
            r, h = records[k][i], pcmaps_history[k][i]
            if not r["stepped"]:
                if r["status"] != 0:
                    c["skipped_scans"] += 1
                    seen_skip = True
                continue
            ns = h["scan_ns"]
            if r["split"]:
                held = len(prev["scan_ns"]) if prev is not None else 0
                c["splits"] += 1
                c["split_held_0" if held == 0 else "split_held_1" if held == 1 else "split_held_2plus"] += 1
                c["closed_empty"] += int(h["closed_ns"][-1] == 0)
            if h["remove_moving"] and len(ns) >= 3:
                if ns[-2] == 0:
                    c["triples_empty_middle"] += 1
                else:
                    c["triples_run"] += 1
                    c["triples_empty_oldest"] += int(ns[-3] == 0)
                    c["triples_empty_newest"] += int(ns[-1] == 0)
            if ns[-1] == 0:
                c["empty_scans"] += 1
                c["empty_first_scan"] += int(not seen_step)
                c["empty_at_split"] += int(r["split"])
            if not r["matched"]:
                c["first_scans"] += 1
                c["first_scan_after_skip"] += int(seen_skip)
            elif not h["had_map"]:
                c["matched_without_map"] += 1
            refused = r["status"] != 0
            if refused:
                c["refused_builds" if r["status"] == -4 else "refused_triples"] += 1
                if c["first_refused_step"] < 0:
                    c["first_refused_step"] = k
                c["ok_after_recovery"] = 0
            else:
                c["steps_t_n_0"] += int(h["t_n"] == 0)
                c["recoveries"] += int(last_refused)
                c["ok_after_recovery"] += int(c["first_refused_step"] >= 0)
            prev, last_refused, seen_step = h, refused, True
    for k in range(len(records)):
        stepped = [i for i in range(S) if records[k][i]["stepped"]]
        matched = [i for i in stepped if records[k][i]["matched"]]
        if stepped and all(pcmaps_history[k][i]["scan_ns"][-1] == 0 for i in stepped):
            out["set"]["all_empty_steps"] += 1
            if out["set"]["first_all_empty_step"] < 0:
                out["set"]["first_all_empty_step"] = k
        with_map = [i for i in matched if pcmaps_history[k][i]["had_map"]]
        if matched and len(with_map) < len(matched):
            out["set"]["mixed_map_steps" if with_map else "nomap_only_steps"] += 1
    return out


def certificate_misses(census, certificate):
    """The (who, key, wanted, got) of every count a census does not reach."""
    bad = []
    for who, wants in certificate.items():
        for key, want in wants.items():
            got = census[who][key]
            ok = got == want[1] if isinstance(want, tuple) else got >= want
            if not ok:
                bad.append((who, key, want, got))
    return bad
