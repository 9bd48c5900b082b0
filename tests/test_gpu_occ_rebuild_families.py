"""ndt_sessions_occ_rebuild's cast kernel held to the beam families of ndt_occ_integrate (tests/occ_rebuild_workloads.py,
DESIGN.md 4.16): crafted archives -- sets with space = space_thre = 0 keep every raw scan to the byte, score_thre = -1 and
ndt_sessions_correct give exact poses -- rebuilt into the geometry each family needs.  Every rebuilt grid and the call's stats
equal (a) the restatement over the device's own float32 map points (occ_rebuild_helpers.to_map_dev + occ_helpers.integrate),
(b) at headings of 0, 90, 180 and -90 degrees the restatement over numpy's points, (c) the grid one ndt_occ_integrate_dev
call casts from the same points; (d) the sessions form of the first copy sees the same aimed beams step by step.  Integer
and byte equality throughout."""
import numpy as np
import pytest

import occ_helpers as H
import occ_rebuild_helpers as R
import occ_rebuild_workloads as W
from gpu_support import gpu, sync, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu


def explain(tag, geom, ends, origins, r2, got, want):
    """None when the counters are equal; else family / geometry, the first five differing cells with both values, and the
    reference's beams that touch the first one."""
    for name, a, b in (("hit", got[0], want[0]), ("pass", got[1], want[1])):
        bad = np.argwhere(a != b)
        if not len(bad):
            continue
        cy, cx = (int(v) for v in bad[0])
        touching = []
        for k, (e, o) in enumerate(zip(ends, origins)):
            live, X1, Y1, X0, Y0 = H.classify(geom, o, e, r2)
            for i in np.nonzero(live)[0]:
                x1, y1 = int(X1[i]), int(Y1[i])
                xs, ys = H.closed_form(X0, Y0, x1, y1)
                if ((x1, y1) == (cx, cy)) if name == "hit" else bool(((xs == cx) & (ys == cy)).any()):
                    touching.append({"scan": k, "beam": int(i), "from": (X0, Y0), "to": (x1, y1)})
            if len(touching) >= 8:
                break
        return ("%s into %s: %s counters differ in %d cells; (y, x, got, want) of the first five: %s; the reference's beams on "
                "cell (y %d, x %d): %s" % (tag, tuple(geom), name, len(bad), [(int(y), int(x), int(a[y, x]), int(b[y, x])) for y, x in bad[:5]],
                                           cy, cx, touching[:8]))
    return None


def first_copy(gpu, geom, ends, poses, r2):
    """One ndt_occ_integrate_dev call (batch form, grid_of) over the scans `ends` from the poses' (tx, ty) ->
    ((hit, pass), stats tuple)."""
    import torch
    capi, ctx = gpu
    xy, off = H.pack(ends)
    B, total = len(ends), len(xy)
    d_xy, d_off = to_dev(xy if total else np.zeros((1, 2), np.float32)), to_dev(off.astype(np.int64))
    d_org, d_gof = to_dev(np.ascontiguousarray(poses, np.float64).reshape(-1, 3)), to_dev(np.zeros(B, np.int32))
    d_st = torch.full((4,), 99, dtype=torch.int64, device=d_xy.device)
    sync()
    grid = capi.OccGrid(ctx, geom)
    capi.integrate_occ_dev(ctx, [grid], d_gof.data_ptr(), d_xy.data_ptr(), d_off.data_ptr(), B, total, d_org.data_ptr(), 24, r2, d_st.data_ptr())
    counts = grid.counts()                                                         # (waits for the context's stream)
    st = tuple(int(v) for v in d_st.cpu().numpy())
    grid.close()
    return counts, st


class CraftedSet:
    """A session set whose row i is sessions[i]: stepped to the end of every archive (odometry only), then corrected to the
    wanted poses.  `on_step(k, active)` runs behind every step."""

    def __init__(self, gpu, sessions, on_step=None):
        from ndt_slam_amd import replay
        capi, ctx = gpu
        self.gpu, self.sessions, self.S = gpu, sessions, len(sessions)
        p = dict(replay.LAUNCH_PARAMS, score_thre=-1.0, space=0.0, space_thre=0.0)
        self.ses = capi.Sessions(ctx, self.S, capi.session_params_from_launch(p), archive=True)
        self.step_poses = [[] for _ in sessions]
        self._ends, self._want = {}, {}
        for k, (scans, odo, act) in enumerate(W.lockstep(sessions)):
            recs = self.ses.step(scans, odo, act)
            assert recs["stepped"].tolist() == act.tolist(), (k, recs["stepped"], recs["status"])
            for i in np.nonzero(act)[0]:
                self.step_poses[i].append(np.array(recs[i]["pose"], np.float64))
            if on_step:
                on_step(self, k, act)

    def correct(self):
        """Every session to its wanted poses; -> the statuses (a map status other than NDT_OK does not keep the trajectory
        from being set: asserted here, to the byte)."""
        status = self.ses.correct({i: s.poses for i, s in enumerate(self.sessions)})
        for i, s in enumerate(self.sessions):
            assert self.ses.trajectory(i)[0].tobytes() == s.poses.tobytes(), s.name
        self.forget()
        return status

    def forget(self):
        """The archives or the poses have changed: the cached points and references go."""
        self._ends, self._want = {}, {}

    def ends(self, i):
        """Session i's archive at its trajectory through ONE ndt_scan_to_map_batch_dev call (cached)."""
        if i not in self._ends:
            self._ends[i] = R.to_map_dev(self.gpu[1], self.ses.archive_scans(i), self.ses.trajectory(i)[0])
        return self._ends[i]

    def rebuild(self, geoms, which=None, r2=H.DBL_MAX):
        """geoms: {session: Geometry} of the sessions to take -> ({session: (hit, pass)}, stats tuple)."""
        capi, ctx = self.gpu
        grids = [capi.OccGrid(ctx, geoms[i]) if i in geoms else None for i in range(self.S)]
        if which is None:
            which = np.array([i in geoms for i in range(self.S)], np.uint8)
        st = self.ses.occ_rebuild(grids, which, max_range2=r2)
        out = {i: grids[i].counts() for i in geoms}
        for g in grids:
            if g is not None:
                g.close()
        return out, H.stats_tuple(st)

    def close(self):
        self.ses.close()


def check_cast(cs, i, tag, geom, r2, got, got_st=None, numpy_too=True):
    """Session i's rebuilt counters (and, alone in its call, the stats) against (a), (b) and (c); the three references of a
    (session, geometry, range) are made once per state of the set."""
    s = cs.sessions[i]
    poses = cs.ses.trajectory(i)[0]
    origins = [q[:2] for q in poses]
    ends = cs.ends(i)
    key = (i, tuple(geom), r2)
    if key not in cs._want:
        want, wst = H.integrate([geom], ends, origins, None, r2)
        refs = [("the restatement", ends, want[0], H.stats_tuple(wst))]
        if s.exact:
            ends_np = [W.map_points(x, q) for x, q in zip(cs.ses.archive_scans(i), poses)]
            if all(a.tobytes() == b.tobytes() for a, b in zip(ends, ends_np)):      # the same points: the same restatement
                refs.append(("numpy", ends_np, want[0], H.stats_tuple(wst)))
            else:
                want_np, nst = H.integrate([geom], ends_np, origins, None, r2)
                refs.append(("numpy", ends_np, want_np[0], H.stats_tuple(nst)))
        one, ost = first_copy(cs.gpu, geom, ends, poses, r2)
        refs.append(("ndt_occ_integrate_dev", ends, one, ost))
        cs._want[key] = (refs, wst)
    refs, wst = cs._want[key]
    for what, e, want, st in refs:
        if what == "numpy" and not numpy_too:
            continue
        why = explain("%s (%s, %s) against %s" % (s.family, s.name, tag, what), geom, e, origins, r2, got, want)
        assert why is None, why
        assert got_st is None or got_st == st, (s.name, tag, what, got_st, st)
    return wst


# ------------------------------------------------------------------------------------------ the aimed set (families 1 to 7)
@pytest.fixture(scope="module")
def aimed(gpu):
    capi, ctx = gpu
    sessions = W.aimed_sessions()
    form = {"grids": [capi.OccGrid(ctx, s.casts[0][0]) for s in sessions], "total": np.zeros(4, np.uint64)}

    def newest_scans(cs, k, act):                                                 # (d): the sessions form, behind every step
        form["total"] += np.array(H.stats_tuple(cs.ses.occ_integrate(form["grids"], act)), np.uint64)
    cs = CraftedSet(gpu, sessions, on_step=newest_scans)
    cs.form_counts = [g.counts() for g in form["grids"]]
    cs.form_total = tuple(int(v) for v in form["total"])
    for g in form["grids"]:
        g.close()
    cs.statuses = cs.correct()
    yield cs
    cs.close()


def test_the_archive_is_the_raw_scans_and_the_poses_are_the_wanted_ones(aimed):
    print("map statuses of the correction:", aimed.statuses)
    for i, s in enumerate(aimed.sessions):
        arch = aimed.ses.archive_scans(i)
        assert len(arch) == len(s.scans) and aimed.ses.archive_info(i) == (len(s.scans), sum(len(x) for x in s.scans)), s.name
        assert all(a.tobytes() == np.ascontiguousarray(x).tobytes() for a, x in zip(arch, s.scans)), s.name
        assert aimed.ses.trajectory(i)[0].tobytes() == s.poses.tobytes(), s.name
        assert aimed.step_poses[i][0].tobytes() == s.poses[0].tobytes(), s.name      # a first step takes its odometry
        if s.exact and s.family != "rounding":                                    # the device's points are the wanted ones
            assert all(e.tobytes() == W.map_points(x, q).tobytes() for e, x, q in zip(aimed.ends(i), s.scans, s.poses)), s.name


@pytest.mark.parametrize("name,tag", W.aimed_cases(), ids=["%s-%s" % c for c in W.aimed_cases()])
def test_a_family_rebuilt_into_its_geometry(aimed, name, tag):
    i = [s.name for s in aimed.sessions].index(name)
    _, geom, r2 = next(c for c in W.casts_of(aimed.sessions[i]) if c[0] == tag)
    got, st = aimed.rebuild({i: geom}, r2=r2)
    wst = check_cast(aimed, i, tag, geom, r2, got[i], st)
    assert wst["n_beams"] == sum(len(x) for x in aimed.sessions[i].scans)


def test_every_aimed_session_in_one_call(aimed):
    """All fourteen rows in one table, each into its own geometry; with one and with five workgroups as well."""
    capi, ctx = aimed.gpu
    geoms = {i: s.casts[0][0] for i, s in enumerate(aimed.sessions)}
    total = dict.fromkeys(H.STATS, 0)
    for wg in (0, 1, 5):
        ctx.set_option(capi.OPT_WORKGROUPS, wg)
        try:
            got, st = aimed.rebuild(geoms)
        finally:
            ctx.set_option(capi.OPT_WORKGROUPS, 0)
        for i, s in enumerate(aimed.sessions):
            wst = check_cast(aimed, i, "all rows, %d workgroups" % wg, geoms[i], H.DBL_MAX, got[i], numpy_too=wg == 0)
            if wg == 0:
                total = H.add_stats(total, wst)
        assert st == H.stats_tuple(total), (wg, st, total)


def test_the_sessions_form_saw_the_same_beams_step_by_step(aimed):
    """(d) ndt_sessions_occ_integrate behind every step, into a grid of the session's first geometry: the newest scan at the
    step's pose.  A first step's pose is its odometry, so every session's first scan is cast exactly as aimed; the later ones
    at the pose the step gave -- for the prefix totals still a pose at which every scan has its total of items."""
    ctx = aimed.gpu[1]
    total = dict.fromkeys(H.STATS, 0)
    for i, s in enumerate(aimed.sessions):
        g, poses = s.casts[0][0], np.array(aimed.step_poses[i])
        origins = [q[:2] for q in poses]
        assert poses[0].tobytes() == s.poses[0].tobytes(), s.name
        ends = R.to_map_dev(ctx, s.scans, poses)
        want, wst = H.integrate([g], ends, origins)
        why = explain("%s (%s) in the sessions form" % (s.family, s.name), g, ends, origins, H.DBL_MAX, aimed.form_counts[i], want[0])
        assert why is None, why
        total = H.add_stats(total, wst)
        if s.name == "prefix-totals":
            items = [int(W.items_of(g, o, e).sum()) for o, e in zip(origins, ends)]
            assert items == list(W.PREFIX_TOTALS) + [256, 257], items
    assert aimed.form_total == H.stats_tuple(total)


# ------------------------------------------------------------------------------------------ 8: many scans
@pytest.mark.parametrize("steps", sorted(W.MANY))
def test_more_scans_than_the_jobs_kernel_has_threads(gpu, steps):
    capi, ctx = gpu
    sessions = W.many_sessions(steps)
    cs = CraftedSet(gpu, sessions)
    cs.correct()
    assert [cs.ses.archive_info(i)[0] for i in range(4)] == [steps, steps, steps - W.MANY_LATE, steps]
    alone = {}
    for which in W.MANY[steps]:
        geoms = {i: sessions[i].casts[0][0] for i in range(4) if which[i]}
        for wg in (0, 1):
            ctx.set_option(capi.OPT_WORKGROUPS, wg)
            try:
                got, st = cs.rebuild(geoms)
            finally:
                ctx.set_option(capi.OPT_WORKGROUPS, 0)
            total = dict.fromkeys(H.STATS, 0)
            for i in geoms:
                total = H.add_stats(total, check_cast(cs, i, "named %s, %d workgroups" % (which, wg), geoms[i], H.DBL_MAX, got[i], numpy_too=wg == 0))
                alone.setdefault(i, got[i])
                assert all(np.array_equal(a, b) for a, b in zip(alone[i], got[i])), (which, i)
            assert st == H.stats_tuple(total) and st[0] == sum(sum(len(x) for x in sessions[i].scans) for i in geoms), (which, st)
    cs.close()


# ------------------------------------------------------------------------------------------ 9: dealing
def test_the_dealing_order_visits_every_run_once(gpu):
    capi, ctx = gpu
    sessions = W.dealing_sessions()
    combos = W.dealing_combinations()
    seen = []

    def rebuild_subsets(cs, k, act):
        stage = k + 1
        if stage not in W.DEAL_STAGES:
            return
        cs.forget()
        runs = [sum(-(-len(x) // 256) for x in cs.ses.archive_scans(i)) for i in range(3)]
        assert runs == [1, 2, stage]
        for _, sub, n_runs, T, stride, bumps in [c for c in combos if c[0] == stage]:
            geoms = {i: sessions[i].casts[0][0] for i in range(3) if sub[i]}
            for wg in W.WORKGROUPS:
                ctx.set_option(capi.OPT_WORKGROUPS, wg)
                try:
                    got, st = cs.rebuild(geoms)
                finally:
                    ctx.set_option(capi.OPT_WORKGROUPS, 0)
                total = dict.fromkeys(H.STATS, 0)
                for i in geoms:
                    tag = "stage %d, named %s: %d runs in %d rows, stride %d; %d workgroups" % (stage, sub, n_runs, T, stride, wg)
                    total = H.add_stats(total, check_cast(cs, i, tag, geoms[i], H.DBL_MAX, got[i], numpy_too=False))
                assert st == H.stats_tuple(total), (stage, sub, wg, st, total)
            seen.append((n_runs, T))
    cs = CraftedSet(gpu, sessions, on_step=rebuild_subsets)
    assert len(seen) == len(combos) == 28 and {n for n, _ in seen} >= {1, 2, 3, 4, 6, 8, 9}
    cs.close()
