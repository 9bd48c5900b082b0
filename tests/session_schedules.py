"""Maintenance schedules of a resident session set (tests only): ndt_sessions_correct, ndt_sessions_remake_closed,
ndt_sessions_find_loops, ndt_sessions_occ_integrate and ndt_sessions_occ_rebuild called again and again, in any order, with
and without steps between them, against the composed chain that makes every one of them out of public single-purpose calls.

ScheduleChain   session_remake_helpers.RemadeChain + the occupancy counters (occ_helpers.integrate, occ_rebuild_helpers.restate)
                and the loop search (loops_helpers.gate_ref + compose_loop).  Nothing in it calls ndt_sessions_correct,
                _remake_closed, _find_loops, _occ_integrate or _occ_rebuild.
Schedule        a name, a workload and a list of (step k, op): the ops are applied behind step k in list order.
SCHEDULES       the table of workload A (the three drives of tests/test_gpu_sessions_correct.py).
simulate        a schedule on replay.PointCloudMap's bookkeeping alone, the logs' odometry as the poses (host only): what
                tests/test_session_schedules_host.py holds every schedule's purpose to, and what the device run must meet.
Runner, run     the set and the chain side by side; every comparison is byte equality.
run_lap         workload B: the lap, searched, optimised, corrected, remade and rebuilt behind every step from FULL_LAP - 1 on.
"""
import collections
import math

import numpy as np

import occ_helpers as H
import occ_rebuild_helpers as R
from loops_helpers import FULL_LAP, gate_ref, loop_params_dict, same_candidate
from session_correct_helpers import layout, smooth_adjustment
from session_helpers import lockstep, same_records, session_logs
from session_remake_helpers import RemadeChain

SPECS_A, STARTS_A = ((33, 12), (34, 12), (35, 10)), [0, 0, 1]
GEOM_A = H.Geometry(-12.0, -6.0, 0.05, 400, 400)
LP_A = dict(min_path=1.0, radius=10.0, step_xy=0.1, step_yaw=math.radians(1.0), half=(2, 2, 1))      # 75 poses; top_k 2
TOP_K_A = 2
SPECS_B, N_FRAMES_B = (33, 34), 64
GEOM_B = H.Geometry(-25.0, -25.0, 0.25, 200, 200)
LP_B = dict(min_path=10.0, radius=2.0, step_xy=0.1, step_yaw=math.radians(1.0), half=(10, 10, 6))    # ndt_loop_default_params
_LOGS = {}


def logs_a():
    if "a" not in _LOGS:
        _LOGS["a"] = session_logs(SPECS_A)
    return _LOGS["a"]


def logs_b():
    if "b" not in _LOGS:
        _LOGS["b"] = session_logs(tuple((seed, N_FRAMES_B) for seed in SPECS_B), n_beams=181)
    return _LOGS["b"]


def params_a(rm=1):
    from ndt_slam_amd import replay
    return dict(replay.LAUNCH_PARAMS, sepThre=1.5, removeMoving=bool(rm))


def params_b():
    from ndt_slam_amd import replay
    return dict(replay.LAUNCH_PARAMS, sepThre=5.0)


# ---------------------------------------------------------------------------------------------- the ops and the table
Op = collections.namedtuple("Op", "kind who scale start key clear inert")
ALL = "started"                                            # `who`: every session that has started


def correct(who, scale=1.0, start=0):
    """smooth_adjustment of the poses as they are; start: a scan index, or "sub1" = the session's sub_first[1]."""
    return Op("correct", who, scale, start, None, None, False)


def correct_to(who, key, inert=False):
    """An explicit trajectory per session, kept under `key`; inert: it moves no anchor and no stored scan."""
    return Op("correct_to", who, None, None, key, None, inert)


def remake(who):
    return Op("remake", who, None, None, None, None, False)


def search(which=ALL):
    return Op("search", which, None, None, None, None, False)


def occ_integrate(which=ALL):
    return Op("occ_integrate", which, None, None, None, None, False)


def occ_rebuild(which=ALL, clear=1):
    return Op("occ_rebuild", which, None, None, None, clear, False)


class Schedule(collections.namedtuple("Schedule", "name ops idle bad rm_too")):
    """ops: [(k, Op)]; idle: {k: sessions inactive at step k}; bad: {k: sessions whose scan carries one NaN point at step k};
    rm_too: the schedule is also run with removeMoving = 0."""

    def behind(self, k):
        return [op for at, op in self.ops if at == k]


def _sched(name, ops, idle=None, bad=None, rm_too=False):
    return Schedule(name, ops, idle or {}, bad or {}, rm_too)


def far_first_scan(poses):
    """The span case of test_span_error_costs_its_session_alone: scan 0 sent to tx = 1e8."""
    out = np.array(poses, np.float64).reshape(-1, 3).copy()
    out[0, 0] = 1e8
    return out


def _every_step():
    ops = []
    for k in range(1, 13):
        ops += [(k, occ_integrate()), (k, correct(ALL, 0.3 if k % 2 else -0.3)), (k, remake(ALL)), (k, occ_rebuild(ALL, 1)), (k, search())]
    return ops


def _search_between():
    return [(k, op) for k in (8, 10) for op in (search(), correct([0, 2]), search(), remake([0, 2]), search())]


SCHEDULES = [
    _sched("twice", [(4, correct([0, 2])), (8, correct([0, 2], -0.7))], rm_too=True),
    _sched("back_to_back", [(7, correct([0])), (7, correct([2])), (7, correct([0, 1], 0.5)), (7, remake([0, 2])), (7, remake([0, 2])),
                            (7, correct([1]))]),
    _sched("remake_then_correct", [(7, correct([0, 2])), (7, remake([0, 2])), (8, correct([0, 2], 1.0, "sub1")), (10, remake([0, 2]))],
           rm_too=True),
    _sched("rotating_names", [(5, correct([0])), (6, correct([1])), (7, remake([0, 1, 2])), (8, correct([2])), (8, remake([2])),
                              (9, correct([0, 1, 2]))]),
    _sched("search_between", _search_between()),
    _sched("idle_and_refused", [(7, correct([0, 1, 2])), (8, remake([0, 1, 2])), (8, occ_rebuild(ALL, 1)), (9, correct([1]))],
           idle={5: [1], 6: [1], 7: [1]}, bad={6: [2]}),
    _sched("every_step", _every_step()),
    _sched("grid_without_clear", [(k, occ_integrate()) for k in range(13)] +
           [(k, op) for k in (5, 9) for op in (correct([0, 2]), occ_rebuild(ALL, 0))]),
    # (a correction that carries the last pose 0.7 m along the drive: the next split comes where the corrected pose puts it)
    _sched("long_jump", [(4, correct([0, 2], -8.0)), (7, remake([0, 2]))]),
    _sched("failed_then_named_again", [(7, correct_to([0], far_first_scan, inert=True)), (7, remake([0, 2])), (8, correct([2])),
                                       (8, remake([2])), (8, search()), (9, correct([2], -0.5)), (9, remake([2])), (9, search())]),
]
BY_NAME = {s.name: s for s in SCHEDULES}


def steps_of(schedule, logs, starts):
    """lockstep with the schedule's overrides: an idle session does not take part (its frame of that step is left out), a
    bad scan carries one NaN point."""
    for k, scans, odo, act in lockstep(logs, starts):
        act = act.copy()
        for i in schedule.idle.get(k, ()):
            act[i], scans[i], odo[i] = 0, np.zeros((0, 2)), (0.0, 0.0, 0.0)
        bad = [i for i in schedule.bad.get(k, ()) if act[i]]
        for i in bad:
            scans[i] = np.array(scans[i], np.float64).reshape(-1, 2).copy()
            scans[i][len(scans[i]) // 2, 1] = np.nan
        yield k, scans, odo, act, bad


# ---------------------------------------------------------------------------------------------- the host model
class _NoOps:
    """PointCloudMap's bookkeeping alone."""


def host_map(sep_thre):
    from ndt_slam_amd import replay
    pm = replay.PointCloudMap(_NoOps(), sepThre=sep_thre, removeMoving=True, LeafSize=0.05, resol=0.05, thre_neighbor=0.2)
    pm.deferred = True
    return pm


def host_add(pm, odo, prev_odo, mark):
    """One stepped scan at the pose the odometry predicts from the map's last pose (the first scan: at its odometry pose), as
    a step forms it before the match refines it -> whether the map split."""
    from ndt_slam_amd import replay
    from ndt_slam_amd.pose_estimator import Pose2D
    n_sub = len(pm.submaps)
    pose = Pose2D(*odo) if prev_odo is None else replay.calPredPose(replay.calMotion(Pose2D(*odo), Pose2D(*prev_odo)), pm.lastPose)
    pm.addPose(pose)
    pm.addPointsBookkeeping(np.full((3, 2), float(mark), np.float32))
    pm.setLastPose(pm.poses[-1])
    return len(pm.submaps) > n_sub


def host_poses(pm):
    return np.array([(q.tx, q.ty, q.th) for q in pm.poses], np.float64).reshape(-1, 3)


def host_set_poses(pm, new):
    from ndt_slam_amd.pose_estimator import Pose2D
    pm.poses = [Pose2D(*row) for row in np.asarray(new, np.float64).reshape(-1, 3)]
    pm.lastPose = pm.poses[-1]


def host_gate(pm, lp):
    """gate_ref on the model's layout; every closed submap that held a scan counts as a cloud with points."""
    firsts, anchors, _ = layout(pm)
    sizes = [1 if len(s.scans) else 0 for s in pm.submaps[:-1]]
    off = np.concatenate([[0], np.cumsum(sizes), [sum(sizes)]]).astype(np.uint64) if sizes else np.zeros(2, np.uint64)
    return gate_ref(host_poses(pm), firsts, anchors, off, **lp)


def resolve_start(start, pm):
    return int(layout(pm)[0][1]) if start == "sub1" else int(start)


def simulate(schedule, logs=None, starts=None, sep_thre=1.5, lp=None):
    """-> the events of the schedule on the host model, in order: dicts with kind = "step" (k, split: the sessions that split)
    or the op's kind (k, who, n_closed, sub_first, anchors, store_first, n_scans per named session; start for a correction;
    cand: the sessions gate_ref gives a candidate, for a search)."""
    logs, starts, lp = logs or logs_a(), starts or STARTS_A, lp or LP_A
    S = len(logs)
    pms, prev = [host_map(sep_thre) for _ in range(S)], [None] * S
    events = []
    for k, scans, odo, act, bad in steps_of(schedule, logs, starts):
        split = []
        for i in range(S):
            if act[i] and i not in bad:
                if host_add(pms[i], odo[i], prev[i], k):
                    split.append(i)
                prev[i] = odo[i].copy()
        events.append(dict(kind="step", k=k, split=split, stepped=[i for i in range(S) if act[i] and i not in bad]))
        for op in schedule.behind(k):
            who = [i for i in range(S) if pms[i].poses] if op.who == ALL else list(op.who)
            ev = dict(kind=op.kind, k=k, who=who, n_closed={i: len(pms[i].submaps) - 1 for i in who}, n_scans={i: len(pms[i].poses) for i in who},
                      layout={i: layout(pms[i]) for i in who})
            if op.kind == "correct":
                ev["start"] = {i: resolve_start(op.start, pms[i]) for i in who}
                for i in who:
                    host_set_poses(pms[i], smooth_adjustment(host_poses(pms[i]), op.scale, ev["start"][i]))
            elif op.kind == "correct_to":
                for i in who:
                    host_set_poses(pms[i], op.key(host_poses(pms[i])))
            elif op.kind == "search":
                ev["cand"] = {i: c for i in who for c in [host_gate(pms[i], lp)] if c is not None}
            events.append(ev)
    return events


def simulate_lap():
    """Workload B on the host model: a search behind every step from FULL_LAP - 1 on (the corrections, which come from the
    device's optimiser, are left out: they move a pose by centimetres)."""
    lap = _sched("lap", [(k, search()) for k in range(FULL_LAP - 1, N_FRAMES_B)])
    return simulate(lap, logs_b(), [0] * len(SPECS_B), 5.0, LP_B)


# ---------------------------------------------------------------------------------------------- the chain
class ScheduleChain(RemadeChain):
    """The composed chain with every maintenance call: step, correct(i, poses) and remake(i) are inherited."""

    def __init__(self, capi, ctx, S, p, geom, **kw):
        super().__init__(capi, ctx, S, p, **kw)
        self.geom = geom
        self.counters = [(np.zeros((geom.ny, geom.nx), np.uint32), np.zeros((geom.ny, geom.nx), np.uint32)) for _ in range(S)]

    def poses(self, i):
        return np.array([(q.tx, q.ty, q.th) for q in self.pcmaps[i].poses], np.float64).reshape(-1, 3)

    def occ_integrate(self, i):
        """The newest stored scan, as it lies after any re-posing, cast from the last pose's (tx, ty) -> the stats."""
        pm = self.pcmaps[i]
        scan = np.ascontiguousarray(pm.submaps[-1].scans[-1], np.float32).reshape(-1, 2)
        _, st = H.integrate([self.geom], [scan], [self.poses(i)[-1][:2]], None, H.DBL_MAX, counters=[self.counters[i]])
        return st

    def occ_rebuild(self, i, clear):
        """The whole archive at the poses the chain holds now, into the same counters -> the stats."""
        if clear:
            for a in self.counters[i]:
                a[...] = 0
        _, st = R.restate(self.ctx, self.geom, self.archive[i], self.poses(i), H.DBL_MAX, counters=self.counters[i])
        return st

    def candidate(self, i, lp):
        """gate_ref on the chain's layout -> its dict or None."""
        from loops_helpers import chain_layout
        pm = self.pcmaps[i]
        if not self.started[i] or len(pm.submaps) < 3:
            return None
        poses, first, anchor, off = chain_layout(self, i)
        return gate_ref(poses, first, anchor, off, **loop_params_dict(lp))

    def find_loop(self, i, lp):
        """gate_ref, then compose_loop on the chain's own data -> (the candidate's dict, its ndt_loop's fields, its records)
        or None."""
        from loops_helpers import compose_loop
        ref = self.candidate(i, lp)
        if ref is None:
            return None
        arr = np.zeros(1, self.capi.LOOP_CANDIDATE_DTYPE)
        arr["session"][0] = i
        for f in ("submap", "anchor_scan", "newest_scan", "nearest_scan", "dist", "path"):
            arr[f][0] = ref[f]
        for f, v in ref["lattice"].items():
            arr["lattice"][f][0] = v
        cand = arr[0]
        assert same_candidate(cand, ref)
        out, recs = compose_loop(dict(capi=self.capi, ctx=self.ctx, chain=self, p=self.p), i, cand, lp)
        return ref, out, recs


# ---------------------------------------------------------------------------------------------- the runner
def chain_bytes(chain, i):
    """(cloud, local map, every closed part) of the chain's session i as bytes."""
    _, parts = chain.global_map(i)
    return (chain.p_cloud[i].tobytes(), chain.target[i].tobytes(), [np.ascontiguousarray(x, np.float32).tobytes() for x in parts[:-1]])


class Runner:
    """A set with its archive, one grid per session and the chain, driven side by side.  `log` takes one dict per op: what
    the chain (never the set alone) showed -- the closed submaps, which closed parts changed, the reference's loops."""

    def __init__(self, capi, ctx, S, p, geom, tag):
        self.capi, self.ctx, self.S, self.p, self.geom, self.tag = capi, ctx, S, p, geom, tag
        self.ses = capi.Sessions(ctx, S, capi.session_params_from_launch(p), archive=True)
        self.chain = ScheduleChain(capi, ctx, S, p, geom)
        self.grids = [capi.OccGrid(ctx, geom) for _ in range(S)]
        self.loose = set()             # sessions a remake refused: held to their own snapshots, not to the chain
        self.dirty = [False] * S       # per session: corrected and not remade since
        self.remade = [False] * S      # per session: remade, and neither stepped nor corrected since
        self.log, self.k = [], -1

    def close(self):
        for g in self.grids:
            g.close()
        self.ses.close()
        self.chain.close()

    def started(self):
        return [i for i in range(self.S) if self.chain.started[i]]

    def held(self, tag):
        """Every session against the chain, and the archive against the chain's."""
        from test_gpu_sessions_correct import same_state
        ses, chain = self.ses, self.chain
        for i in range(self.S):
            if i not in self.loose:
                same_state(ses, chain, i, (self.tag, self.k, tag))
            n_scans, n_points = ses.archive_info(i)
            arch = ses.archive_scans(i)
            assert n_scans == len(ses.trajectory(i)[0]) == len(chain.archive[i]) == len(arch), (self.tag, self.k, tag, i)
            assert n_points == sum(len(x) for x in arch), (self.tag, self.k, tag, i)
            assert all(a.tobytes() == np.ascontiguousarray(b, np.float64).tobytes() for a, b in zip(arch, chain.archive[i])), (self.tag, self.k, tag, i)

    def step(self, k, scans, odo, act):
        self.k = k
        got, want = self.ses.step(scans, odo, act), self.chain.step(scans, odo, act)
        for i in range(self.S):
            if i not in self.loose:
                assert same_records(got[i], want[i]), (self.tag, k, i, got[i], want[i])
            if want[i]["stepped"]:
                self.remade[i] = False
        self.held("step")
        self.log.append(dict(kind="step", k=k, split=[i for i in range(self.S) if want[i]["split"]],
                             stepped=[i for i in range(self.S) if want[i]["stepped"]]))
        return want

    def _others(self, who):
        from test_gpu_sessions_correct import snapshot
        return {i: snapshot(self.ses, i) for i in self.loose if i not in who}

    def _others_kept(self, before, tag):
        from test_gpu_sessions_correct import same_snapshot, snapshot
        for i, snap in before.items():
            assert same_snapshot(snapshot(self.ses, i), snap), (self.tag, self.k, tag, i)

    def _waits(self, named, tag):
        st = self.ses.stats()
        assert st.host_waits <= 2 and st.sessions_stepped == named, (self.tag, self.k, tag, st.host_waits, st.sessions_stepped, named)

    def correct(self, new, inert=False, kind="correct"):
        """new: {session: its whole new trajectory}."""
        capi, chain, tag = self.capi, self.chain, kind
        who = list(new)
        before, others = {i: chain_bytes(chain, i) for i in who}, self._others(who)
        status = self.ses.correct(new)
        self._waits(len(who), tag)
        want = {i: chain.correct(i, new[i]) for i in who}
        assert status == want and all(v == capi.NDT_OK for v in want.values()), (self.tag, self.k, tag, status, want)
        moved = {}
        for i in who:
            assert self.ses.trajectory(i)[0].tobytes() == np.ascontiguousarray(new[i], np.float64).tobytes(), (self.tag, self.k, tag, i)
            after = chain_bytes(chain, i)
            moved[i] = [a != b for a, b in zip(after[2], before[i][2])]
            if not inert:                 # (no test passes by doing nothing: on the chain, the views and the closed parts moved)
                assert after[0] != before[i][0] and after[1] != before[i][1], (self.tag, self.k, tag, i)
                assert any(moved[i]) or not moved[i], (self.tag, self.k, tag, i)
                self.dirty[i], self.remade[i] = True, False
        self._others_kept(others, tag)
        self.held(tag)
        self.log.append(dict(kind=kind, k=self.k, who=who, n_closed={i: len(moved[i]) for i in who}, moved=moved,
                             layout={i: layout(chain.pcmaps[i]) for i in who}, n_scans={i: len(new[i]) for i in who}))

    def remake(self, who, tag="remake"):
        chain = self.chain
        from test_gpu_sessions_correct import same_snapshot, snapshot
        before, others = {i: chain_bytes(chain, i) for i in who}, self._others(who)
        snaps = {i: snapshot(self.ses, i) for i in who}                           # (a refused session keeps every byte)
        status = self.ses.remake_closed(who)
        self._waits(len(who), tag)
        want = {i: chain.remake(i) for i in who}
        assert status == want, (self.tag, self.k, tag, status, want)
        changed = {}
        for i in who:
            after = chain_bytes(chain, i)
            changed[i] = [a != b for a, b in zip(after[2], before[i][2])]
            if want[i] != self.capi.NDT_OK:
                self.loose.add(i)
                assert after == before[i] and same_snapshot(snapshot(self.ses, i), snaps[i]), (self.tag, self.k, tag, i)
                continue
            if self.dirty[i] and changed[i]:
                assert any(changed[i]), (self.tag, self.k, tag, i, "the first remake behind a correction changed no closed part")
            if self.remade[i]:
                assert after == before[i], (self.tag, self.k, tag, i, "a repeated remake changed a byte")
            self.dirty[i], self.remade[i] = False, True
        self._others_kept(others, tag)
        self.held(tag)
        self.log.append(dict(kind="remake", k=self.k, who=who, n_closed={i: len(changed[i]) for i in who}, changed=changed, status=want))

    def search(self, lp, which=None, tag="search"):
        """-> the set's loops of the sessions held to the chain."""
        from loops_helpers import assert_composed
        from test_gpu_sessions_correct import same_snapshot, snapshot
        ses, chain = self.ses, self.chain
        looked = list(range(self.S)) if which is None else list(which)
        flags = np.array([1 if i in looked else 0 for i in range(self.S)], np.uint8)
        before = [snapshot(ses, i) for i in range(self.S)]
        loops, recs = ses.find_loops(lp, flags, want_records=True)
        st = ses.stats()
        assert loops["cand"].tobytes() == ses.loop_candidates(lp, flags).tobytes(), (self.tag, self.k, tag)
        refs = {i: r for i in looked if i not in self.loose for r in [chain.find_loop(i, lp)] if r is not None}
        got = [j for j in range(len(loops)) if int(loops[j]["cand"]["session"]) not in self.loose]
        assert [int(loops[j]["cand"]["session"]) for j in got] == sorted(refs), (self.tag, self.k, tag, loops["cand"]["session"], sorted(refs))
        assert st.host_waits <= 2 and st.sessions_stepped == len(refs) + len(loops) - len(got), (self.tag, self.k, tag, st.host_waits,
                                                                                                 st.sessions_stepped, sorted(refs))
        sc = dict(capi=self.capi, ctx=self.ctx, chain=chain, p=self.p)
        for j in got:
            i = int(loops[j]["cand"]["session"])
            assert same_candidate(loops[j]["cand"], refs[i][0]), (self.tag, self.k, tag, i)
            assert_composed(sc, loops[j], recs[j], lp)
        for i in range(self.S):
            assert same_snapshot(before[i], snapshot(ses, i)), (self.tag, self.k, tag, i)
        self.held(tag)
        self.log.append(dict(kind="search", k=self.k, who=looked, loose=sorted(self.loose), cand={i: r[0] for i, r in refs.items()},
                             n_cand={i: int(r[1]["n_cand"]) for i, r in refs.items()}, found={i: int(r[1]["found"]) for i, r in refs.items()}))
        return {int(loops[j]["cand"]["session"]): loops[j] for j in got}

    def _occ(self, kind, which, clear, tag):
        flags = np.array([1 if i in which else 0 for i in range(self.S)], np.uint8)
        if kind == "occ_integrate":
            st = self.ses.occ_integrate(self.grids, flags)
        else:
            st = self.ses.occ_rebuild(self.grids, flags, clear=bool(clear))
        want = dict.fromkeys(H.STATS, 0)
        for i in which:
            if self.chain.started[i]:
                want = H.add_stats(want, self.chain.occ_integrate(i) if kind == "occ_integrate" else self.chain.occ_rebuild(i, clear))
        assert H.stats_tuple(st) == H.stats_tuple(want), (self.tag, self.k, tag, st, want)
        for i in range(self.S):
            assert R.same_counts(self.grids[i], self.chain.counters[i]), (self.tag, self.k, tag, i)
        self.held(tag)
        self.log.append(dict(kind=kind, k=self.k, who=list(which), stats=H.stats_tuple(want)))

    def occ_integrate(self, which, tag="occ_integrate"):
        self._occ("occ_integrate", which, 0, tag)

    def occ_rebuild(self, which, clear, tag="occ_rebuild"):
        self._occ("occ_rebuild", which, clear, tag)

    def apply(self, op, lp):
        chain = self.chain
        who = self.started() if op.who == ALL else list(op.who)
        if op.kind == "correct":
            self.correct({i: smooth_adjustment(chain.poses(i), op.scale, resolve_start(op.start, chain.pcmaps[i])) for i in who})
        elif op.kind == "correct_to":
            self.correct({i: op.key(chain.poses(i)) for i in who}, inert=op.inert, kind="correct_to")
        elif op.kind == "remake":
            self.remake(who)
        elif op.kind == "search":
            self.search(lp, who)
        elif op.kind == "occ_integrate":
            self.occ_integrate(who)
        else:
            self.occ_rebuild(who, op.clear)


def loop_params_a(capi):
    hx, hy, hk = LP_A["half"]
    return capi.default_loop_params(min_path=LP_A["min_path"], radius=LP_A["radius"], step_xy=LP_A["step_xy"], step_yaw=LP_A["step_yaw"],
                                    half_x=hx, half_y=hy, half_yaw=hk, top_k=TOP_K_A)


def run(schedule, capi, ctx, rm=1):
    """The schedule on workload A -> the runner's log."""
    logs, p = logs_a(), params_a(rm)
    r = Runner(capi, ctx, len(logs), p, GEOM_A, (schedule.name, rm))
    lp = loop_params_a(capi)
    try:
        for k, scans, odo, act, bad in steps_of(schedule, logs, STARTS_A):
            want = r.step(k, scans, odo, act)
            assert all(want[i]["stepped"] == 0 and want[i]["status"] != 0 for i in bad), (schedule.name, k, want)
            for op in schedule.behind(k):
                r.apply(op, lp)
        return r.log
    finally:
        r.close()


def run_lap(capi, ctx):
    """Workload B -> the runner's log.  From step FULL_LAP - 1 on, behind every step: search; the found loops' edges with the
    odometry arcs of ndt_sessions_trajectory into ndt_pg_optimize_batch; correct (the chain takes the same arrays), remake,
    occ_rebuild(clear = 1)."""
    from ndt_slam_amd import replay
    logs, p = logs_b(), params_b()
    S = len(logs)
    r = Runner(capi, ctx, S, p, GEOM_B, ("lap", 1))
    lp = capi.default_loop_params()
    assert loop_params_dict(lp) == LP_B
    info = np.array(lp.info[:]) / 100.0
    try:
        for k, scans, odo, act in lockstep(logs):
            r.step(k, scans, odo, act)
            if k < FULL_LAP - 1:
                continue
            loops = r.search(lp)
            found = [i for i, loop in loops.items() if loop["status"] == 0 and loop["found"]]
            new = {}
            if found:
                trajs = [r.ses.trajectory(i)[0] for i in found]
                graphs = [replay.loop_graph(t, loops[i]["edge"], info) for i, t in zip(found, trajs)]
                off = np.concatenate([[0], np.cumsum([len(t) for t in trajs])]).astype(np.uint64)
                out, res = capi.optimize_pose_graphs(ctx, np.concatenate(trajs), off, np.concatenate(graphs), off)
                new = {i: out[int(off[g]):int(off[g + 1])].copy() for g, i in enumerate(found) if res[g]["status"] == 0}
            if new:
                r.correct(new)
                r.remake(list(new))
                r.occ_rebuild(list(new), 1)
        return r.log
    finally:
        r.close()
