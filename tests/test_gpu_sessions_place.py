"""ndt_sessions_place_candidates on the device.  Composition: on a small set the candidates are ndt_place_describe_batch on the
set's own read-outs (closed clouds, trajectories, local maps) followed by ndt_place_match, byte for byte, and the numpy
restatement of tests/place_helpers.py on the same views; `which`, `against`, a set of one, a session that never started, the
stats, the untouched SLAM state."""
import ctypes

import numpy as np
import pytest

import place_helpers as H
import session_workloads as W
from session_helpers import device_cloud, lockstep, session_logs
from test_gpu_loops import run_lockstep
from test_gpu_sessions_correct import same_snapshot, snapshot
from gpu_support import gpu, sync, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

SPECS = ((33, 40), (34, 40), (35, 27), (36, 5))    # sepThre 3: a submap closes every five or six scans; session 3 never steps
STEPS = 40


@pytest.fixture(scope="module")
def scene(gpu):
    capi, ctx = gpu
    p = W.launch_params(sepThre=3.0)
    logs = session_logs(SPECS, n_beams=181)
    logs[3] = ([], np.zeros((0, 3)))
    ses, twin = (capi.Sessions(ctx, len(SPECS), capi.session_params_from_launch(p)) for _ in range(2))
    run_lockstep(logs, STEPS - 1, ses, twin)
    yield dict(capi=capi, ctx=ctx, logs=logs, p=p, ses=ses, twin=twin)
    ses.close(); twin.close()


def views(ses, pp, which=None, against=None):
    """The set's read-outs as the two public calls take them: (clouds, centres, cloud_of, centre scans, item_first, item_group,
    items as (session, submap), searchers, their last headings)."""
    clouds, centres, cloud_of, scans, item_first, item_group, items = [], [], [], [], [0], [], []
    for i in range(ses.n):
        poses, first, _, _ = ses.trajectory(i)
        if (against is not None and not against[i]) or len(poses) < 1 or len(first) < 2:
            continue
        closed = ses.global_map(i)[1][:len(first) - 1]
        for m in range(len(first) - 1):
            a, e = int(first[m]), int(first[m + 1]) - 1
            if not len(closed[m]) or e < a:
                continue
            clouds.append(closed[m])
            for k in range(a, e + 1, pp.centre_stride):
                centres.append(poses[k, :2]); cloud_of.append(len(clouds) - 1); scans.append(k)
            items.append((i, m)); item_group.append(i); item_first.append(len(centres))
    n_entries, who, heading = len(centres), [], []
    for i in range(ses.n):
        poses = ses.trajectory(i)[0]
        ptr, n, _ = ses.local_map(i)
        if (which is not None and not which[i]) or len(poses) < 1 or not n:
            continue
        clouds.append(device_cloud(ptr, n))
        centres.append(poses[-1, :2]); cloud_of.append(len(clouds) - 1)
        who.append(i); heading.append(poses[-1, 2])
    return dict(clouds=clouds, centres=np.array(centres).reshape(-1, 2), cloud_of=cloud_of, scans=scans, item_first=item_first, item_group=item_group,
                items=items, who=who, heading=heading, n_entries=n_entries)


def composed(capi, ctx, ses, pp, which=None, against=None, numpy_too=False):
    """The candidates made of ndt_place_describe_batch and ndt_place_match on the views: PLACE_CANDIDATE_DTYPE records."""
    v = views(ses, pp, which, against)
    if not v["who"] or not v["items"]:
        return np.zeros(0, capi.PLACE_CANDIDATE_DTYPE)
    desc = capi.place_describe_batch(ctx, v["clouds"], v["centres"], v["cloud_of"], pp)
    d, q = desc[:v["n_entries"]], desc[v["n_entries"]:]
    hits, n, table = capi.place_match(ctx, q, v["who"], d, v["item_first"], v["item_group"], pp)
    if numpy_too:
        ref = np.stack([H.describe_ref(v["clouds"][c], v["centres"][k], pp) for k, c in enumerate(v["cloud_of"])])
        assert desc.tobytes() == ref.tobytes()
        rh, rn, rt = H.match_ref(capi, q, v["who"], d, v["item_first"], v["item_group"], pp)
        assert hits.tobytes() == rh.tobytes() and n.tobytes() == rn.tobytes() and table.tobytes() == rt.tobytes()
    out = []
    for j, i in enumerate(v["who"]):
        for h in hits[j, :n[j]]:
            ses_t, m = v["items"][int(h["item"])]
            scan = v["scans"][int(h["desc"])]
            c = np.zeros(1, capi.PLACE_CANDIDATE_DTYPE)[0]
            c["session"], c["map_session"], c["submap"], c["centre_scan"] = i, ses_t, m, scan
            for f in ("shift", "key", "overlap", "n_query", "n_entry", "rank"):
                c[f] = h[f]
            centre = ses.trajectory(ses_t)[0][scan]
            c["guess"] = (centre[0], centre[1], np.float64(v["heading"][j]) - np.float64(int(h["shift"])) * np.float64(5.625))
            out.append(c)
    return np.array(out, capi.PLACE_CANDIDATE_DTYPE) if out else np.zeros(0, capi.PLACE_CANDIDATE_DTYPE)


def test_candidates_are_describe_and_match_on_the_views(scene):
    capi, ctx, ses = scene["capi"], scene["ctx"], scene["ses"]
    before = [snapshot(ses, i) for i in range(3)]
    assert all(len(ses.trajectory(i)[1]) >= 4 for i in range(3)) and len(ses.trajectory(3)[0]) == 0
    for kw in (dict(), dict(top_k=16), dict(top_k=1), dict(centre_stride=3), dict(n_rings=32, ring_width=0.3, min_pts=2), dict(min_key=30000)):
        pp = capi.default_place_params(**kw)
        got = ses.place_candidates(pp)
        st = ses.stats()
        want = composed(capi, ctx, ses, pp, numpy_too=not kw)
        assert got.tobytes() == want.tobytes(), kw
        assert (st.host_waits, st.sessions_stepped, st.triples_run) == (1, 0, 0) and st.h2d_bytes > 0 and st.d2h_bytes > 0
        print(kw, [(int(c["session"]), int(c["map_session"]), int(c["submap"]), int(c["centre_scan"]), int(c["shift"]), int(c["key"])) for c in got])
    pp = capi.default_place_params()
    got = ses.place_candidates(pp)
    assert sorted(set(got["session"].tolist())) == [0, 1, 2] and all(c["session"] != c["map_session"] for c in got)
    assert all(0 <= c["map_session"] < 3 for c in got)                                # the session that never started is nobody's track
    # top_k only truncates
    one, many = ses.place_candidates(capi.default_place_params(top_k=1)), ses.place_candidates(capi.default_place_params(top_k=16))
    for i in range(3):
        a, b = got[got["session"] == i], many[many["session"] == i]
        assert a.tobytes() == b[:len(a)].tobytes() and one[one["session"] == i].tobytes() == a[:1].tobytes()
    for i in range(3):
        assert same_snapshot(before[i], snapshot(ses, i)), i                         # nothing of the SLAM state moved


def test_which_against_and_the_sets_that_find_nothing(scene, gpu):
    capi, ctx, ses = scene["capi"], scene["ctx"], scene["ses"]
    pp = capi.default_place_params()
    every = ses.place_candidates(pp)
    for which, against in (([1, 0, 0, 0], None), (None, [0, 0, 1, 0]), ([1, 0, 1, 1], [1, 0, 1, 1]), ([0, 1, 0, 0], [1, 0, 1, 0])):
        sub = ses.place_candidates(pp, which, against)
        assert sub.tobytes() == composed(capi, ctx, ses, pp, which, against).tobytes(), (which, against)
        assert all(which is None or which[c["session"]] for c in sub) and all(against is None or against[c["map_session"]] for c in sub)
    # a searcher's candidates do not depend on the other searchers
    alone = ses.place_candidates(pp, [0, 1, 0, 0])
    assert alone.tobytes() == every[every["session"] == 1].tobytes()
    # the one track is the searcher's own; nobody searches; nobody is searched; the session that never started searches
    assert len(ses.place_candidates(pp, [0, 1, 0, 0], [0, 1, 0, 0])) == 0 and ses.stats().host_waits == 1
    for which, against in (([0, 0, 0, 0], None), (None, [0, 0, 0, 0]), ([0, 0, 0, 1], None), (None, [0, 0, 0, 1])):
        assert len(ses.place_candidates(pp, which, against)) == 0
        st = ses.stats()
        assert (st.host_waits, st.h2d_bytes, st.d2h_bytes) == (0, 0, 0)
    # a set of one session
    one = capi.Sessions(ctx, 1, capi.session_params_from_launch(scene["p"]))
    try:
        run_lockstep(scene["logs"][:1], 20, one)
        assert len(one.trajectory(0)[1]) >= 3 and len(one.place_candidates(pp)) == 0 and one.stats().host_waits == 1
    finally:
        one.close()
    # the refusals
    lib, E, n = capi.lib(), capi.NDT_E_ARG, ctypes.c_int(-7)
    out = np.zeros(16 * 4, capi.PLACE_CANDIDATE_DTYPE)
    err = lambda: lib.ndt_last_error(ctx.h).decode()
    assert lib.ndt_sessions_place_candidates(ses.h, None, None, None, out.ctypes.data, ctypes.byref(n)) == E and "NULL pointer" in err()
    assert lib.ndt_sessions_place_candidates(ses.h, None, None, ctypes.byref(pp), None, ctypes.byref(n)) == E and "NULL pointer" in err()
    for kw, word in ((dict(top_k=17), "top_k"), (dict(centre_stride=0), "centre_stride"), (dict(n_rings=33), "n_rings"), (dict(ring_width=0.0), "ring_width")):
        bad = capi.default_place_params(**kw)
        assert lib.ndt_sessions_place_candidates(ses.h, None, None, ctypes.byref(bad), out.ctypes.data, ctypes.byref(n)) == E
        assert err().startswith("ndt_sessions_place_candidates: ") and word in err()
    assert n.value == -7 and not out.tobytes().strip(b"\0")


def test_the_step_after_a_search_is_the_twins(scene):
    """Behind the searches above: the next step of the set and of the twin that never searched are the same bytes.  (The
    module's last test on the scene: it steps it.)"""
    ses, twin = scene["ses"], scene["twin"]
    ses.place_candidates(scene["capi"].default_place_params(top_k=16))
    for k, scans, odo, act in lockstep(scene["logs"]):
        if k < STEPS - 1:
            continue
        assert ses.step(scans, odo, act).tobytes() == twin.step(scans, odo, act).tobytes()
    for i in range(3):
        assert same_snapshot(snapshot(ses, i), snapshot(twin, i)), i


# ------------------------------------------------------------------------------------------ end to end
# Two sessions on the synthetic hall's lap (synth.replay_records: a circle of radius 5 m) with different seeds and steps.  A
# drives N_A scans of 0.3 m, B drives N_B scans of 0.27 m and ends where A's closed submaps have been.  B's odometry is
# rotated and shifted by an offset the library is not told.
N_A, N_B, STEP_A, STEP_B = 72, 60, 0.3, 0.27
SHIFT = (30.0, -12.0)


def lap(seed, n, step):
    from ndt_slam_amd import synth
    recs, truth = synth.replay_records(n_frames=n, n_beams=181, step=step, seed=seed)
    return ([np.asarray(r["front"], np.float64).reshape(-1, 2) for r in recs], np.array([[r["x"], r["y"], r["th"]] for r in recs], np.float64),
            np.asarray(truth, np.float64).reshape(-1, 3))


def moved(odo, phi_deg, shift):
    """The odometry as a robot that started in another frame reports it: rotated by phi, shifted, headings wrapped."""
    c, s = np.cos(np.radians(phi_deg)), np.sin(np.radians(phi_deg))
    out = odo.copy()
    out[:, 0] = c * odo[:, 0] - s * odo[:, 1] + shift[0]
    out[:, 1] = s * odo[:, 0] + c * odo[:, 1] + shift[1]
    out[:, 2] = (odo[:, 2] + phi_deg + 180.0) % 360.0 - 180.0
    return out


def pose_error(pose, truth):
    """(metres, radians) between a pose (tx, ty, th[deg]) and the truth."""
    return (float(np.hypot(pose[0] - truth[0], pose[1] - truth[1])), abs(np.radians((pose[2] - truth[2] + 180.0) % 360.0 - 180.0)))


@pytest.fixture(scope="module")
def laps(gpu):
    """The two logs, and the reference path's error: a twin set in which B's odometry is already in A's frame and the loop is
    found by ndt_sessions_find_cross_loops."""
    from loops_multi_helpers import MULTI
    from ndt_slam_amd import replay
    from test_gpu_loops import params
    capi, ctx = gpu
    a, b = lap(33, N_A, STEP_A), lap(77, N_B, STEP_B)
    p = params()
    twin = capi.Sessions(ctx, 2, capi.session_params_from_launch(p))
    try:
        run_lockstep([(a[0], a[1]), (b[0], b[1])], max(N_A, N_B), twin)
        mp = capi.default_loop_multi_params(**MULTI)
        found = [l for l in twin.find_cross_loops(mp, [0, 1], [1, 0]) if l["m"]["loop"]["status"] == 0 and l["m"]["loop"]["found"]]
        assert found, "the reference path finds no loop: the workload is wrong"
        ref_err = pose_error(found[0]["m"]["loop"]["pose"], b[2][-1])
    finally:
        twin.close()
    return dict(a=a, b=b, p=p, ref_err=ref_err)


@pytest.mark.parametrize("phi", [200.0, 70.0])
def test_two_sessions_without_a_shared_frame(gpu, laps, phi):
    """Condition (a cap, not a measurement): among B's at most 4 candidates one has a centre scan whose true position is
    within 1.0 m of B's true position and a shift within +-1 (mod 64) of the true rotation in sectors -- met by the numpy
    restatement on the set's read-out clouds alone; replay.place_verify accepts at least one candidate, and its edge, applied
    by replay.align_frames, places B's newest pose no worse than twice the reference path's error (floor 1e-3 m, 1e-3 rad)."""
    from loops_multi_helpers import MULTI
    from ndt_slam_amd import replay
    capi, ctx = gpu
    a, b = laps["a"], laps["b"]
    ses = capi.Sessions(ctx, 2, capi.session_params_from_launch(laps["p"]), archive=True)
    try:
        run_lockstep([(a[0], a[1]), (b[0], moved(b[1], phi, SHIFT))], max(N_A, N_B), ses)
        pp = capi.default_place_params()
        got = ses.place_candidates(pp, [0, 1], [1, 0])
        assert got.tobytes() == composed(capi, ctx, ses, pp, [0, 1], [1, 0], numpy_too=True).tobytes()
        true_shift = phi / 5.625
        good = []
        for k, c in enumerate(got):
            d = float(np.hypot(*(a[2][int(c["centre_scan"]), :2] - b[2][-1, :2])))
            off = (int(c["shift"]) - true_shift + 32.0) % 64.0 - 32.0
            print("phi %.0f: candidate %d: submap %d centre scan %d shift %d (true %.2f) key %d: %.2f m from B's true position"
                  % (phi, k, c["submap"], c["centre_scan"], c["shift"], true_shift, c["key"], d))
            if d <= 1.0 and abs(off) <= 1.0:
                good.append(k)
        assert 1 <= len(got) <= 4 and good
        vp = capi.default_loop_multi_params(**dict(MULTI, half_x=5, half_y=5, half_yaw=3))
        edges = replay.place_verify(ctx, ses, got, vp)
        print("phi %.0f: accepted candidates %s" % (phi, [k for k, _ in edges]))
        assert edges
        traj_a, traj_b = ses.trajectory(0)[0], ses.trajectory(1)[0]
        k, edge = edges[0]
        placed = replay.align_frames(traj_b, edge, traj_a)
        err, ref = pose_error(placed[-1], b[2][-1]), laps["ref_err"]
        print("phi %.0f: place path %.4f m %.5f rad; reference path %.4f m %.5f rad" % ((phi,) + err + ref))
        assert err[0] <= max(2 * ref[0], 1e-3) and err[1] <= max(2 * ref[1], 1e-3)
    finally:
        ses.close()
