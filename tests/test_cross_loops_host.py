"""Loops between sessions without a GPU: the header's prototypes in the binding, ndt_cross_gate held -- bytes and all --
against its numpy restatement (cross_loops_helpers.cross_gate_ref) on crafted tracks, its refusals, and replay.cross_graph's
indices against a hand-written case."""
import ctypes
import os
import re

import numpy as np
import pytest

from cross_loops_helpers import cross_gate_ref, line, track

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ndt_cross_gate", "ndt_cross_gate_batch", "ndt_sessions_cross_candidates", "ndt_sessions_find_cross_loops")


@pytest.fixture(scope="module")
def capi():
    from ndt_slam_amd import build, capi
    build.build()
    return capi


def check(capi, last, newest, own, tracks, p, want=None):
    """ndt_cross_gate against the restatement, byte for byte; want: the (map_session, submap) pairs expected."""
    got = capi.cross_gate(last, newest, own, tracks, p)
    ref = cross_gate_ref(capi, last, newest, own, tracks, p)
    assert [(int(g["map_session"]), int(g["cand"]["submap"])) for g in got] == [(int(r["map_session"]), int(r["cand"]["submap"])) for r in ref]
    assert got.tobytes() == ref.tobytes()
    if want is not None:
        assert [(int(g["map_session"]), int(g["cand"]["submap"])) for g in got] == list(want)
    keys = [(float(g["d2"]), int(g["map_session"]), int(g["cand"]["submap"])) for g in got]
    assert keys == sorted(keys) and got["rank"].tolist() == list(range(len(got)))
    assert all(int(g["cand"]["session"]) == 0 and int(g["cand"]["newest_scan"]) == newest and float(g["cand"]["path"]) == 0.0 for g in got)
    return got


def test_the_headers_prototypes_are_bound(capi):
    src = open(os.path.join(ROOT, "include", "ndt_mi355x.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, src), name
        assert name in capi.PROTOTYPES and hasattr(capi.lib(), name), name
    for word in ("ndt_cross_track;", "ndt_cross_candidate;", "ndt_cross_loop;"):
        assert word in src, word
    D = capi.CROSS_CANDIDATE_DTYPE
    assert D.names == ("cand", "map_session", "rank", "d2") and D.fields["cand"][0] == capi.LOOP_CANDIDATE_DTYPE
    assert D.itemsize == capi.LOOP_CANDIDATE_DTYPE.itemsize + 16
    E = capi.CROSS_LOOP_DTYPE
    assert E.names == ("m", "map_session", "reserved") and E.fields["m"][0] == capi.LOOP_MULTI_DTYPE
    assert E.itemsize == capi.LOOP_MULTI_DTYPE.itemsize + 8
    assert ctypes.sizeof(capi.CrossTrack) == 48
    assert "Out of scope: loops between sessions" not in src


def test_the_radius_is_inclusive_on_the_squared_distance(capi):
    M = capi.default_loop_multi_params
    r = 1.7
    r2 = np.float64(r) * np.float64(r)
    # a pose whose d2 is exactly radius * radius: (r, 0) from the origin; and one whose d2 is the next double above
    on = track(np.array([[r, 0.0, 0.0], [50.0, 0.0, 0.0], [60.0, 0.0, 0.0]]), 1)
    got = check(capi, (0.0, 0.0, 10.0), 7, -1, [on], M(radius=r, max_submaps=4), [(0, 0)])
    assert np.float64(got[0]["d2"]).tobytes() == r2.tobytes()
    # the next double above: r^2 + y^2 with y^2 about three quarters of r^2's last place rounds up by exactly one place
    up = np.nextafter(r2, np.inf)
    y = np.sqrt(np.float64(0.75) * (up - r2))
    assert np.float64(r) * np.float64(r) + y * y == up
    over = track(np.array([[r, y, 0.0], [50.0, 0.0, 0.0], [60.0, 0.0, 0.0]]), 1)
    check(capi, (0.0, 0.0, 10.0), 7, -1, [over], M(radius=r, max_submaps=4), [])
    check(capi, (0.0, 0.0, 10.0), 7, -1, [over, on], M(radius=r, max_submaps=4), [(1, 0)])


def test_ties_go_to_the_lower_track_submap_and_scan(capi):
    M = capi.default_loop_multi_params
    a = track(line(0.0, 0.5, 12), 4)                                          # three submaps, two closed
    # two identical tracks: the lower one first, then the same submap of the higher one
    got = check(capi, (0.75, 0.0, 0.0), 3, -1, [a, a], M(max_submaps=4))
    assert [(int(g["map_session"]), int(g["cand"]["submap"])) for g in got][:2] == [(0, 0), (1, 0)]
    check(capi, (0.75, 0.0, 0.0), 3, -1, [a, a], M(max_submaps=1), [(0, 0)])
    # two submaps of one track at the same distance: scans 3 (submap 0) and 4 (submap 1) lie 0.25 either side of x = 1.75
    got = check(capi, (1.75, 0.5, 0.0), 3, -1, [a], M(max_submaps=2), [(0, 0), (0, 1)])
    assert got["d2"].tolist() == [0.0625, 0.0625] and got["cand"]["nearest_scan"].tolist() == [3, 4]
    # two scans of one submap at the same distance: the lower k
    got = check(capi, (0.25, 0.5, 0.0), 3, -1, [a], M(max_submaps=1), [(0, 0)])
    assert int(got[0]["cand"]["nearest_scan"]) == 0 and float(got[0]["d2"]) == 0.0625
    # the anchor is the track's own
    assert int(got[0]["cand"]["anchor_scan"]) == int(a[2][0])


def test_own_track_empty_ranges_empty_clouds_and_open_tracks(capi):
    M = capi.default_loop_multi_params
    a, b = track(line(0.0, 0.0, 12), 4), track(line(0.0, 0.4, 12), 4)
    check(capi, (0.5, 0.0, 0.0), 11, 0, [a, b], M(max_submaps=4), [(1, 0), (1, 1)])      # own excluded: nothing of track 0
    check(capi, (0.5, 0.0, 0.0), 11, 0, [a], M(max_submaps=4), [])                       # one track, the searcher's own: none
    assert len(check(capi, (0.5, 0.0, 0.0), 11, -1, [a], M(max_submaps=4))) == 2
    # the newest CLOSED submap counts (submap 1 of three), the open one (2) never does
    got = check(capi, (3.8, 0.0, 0.0), 11, -1, [a], M(max_submaps=4, radius=1.2))        # (scan 8 of submap 2 is the nearest pose)
    assert got["cand"]["submap"].tolist() == [1]
    # an empty cloud
    poses, first, anchor, off = b
    hollow = off.copy(); hollow[1:] -= 100
    check(capi, (0.5, 0.0, 0.0), 11, 0, [a, (poses, first, anchor, hollow)], M(max_submaps=4), [(1, 1)])
    # an empty scan range: a submap 0 without a scan of its own in front
    f3, a3 = np.concatenate([[0], first]).astype(np.int32), np.concatenate([[0], anchor]).astype(np.int32)
    o3 = (np.arange(len(f3) + 1) * 100).astype(np.uint64)
    check(capi, (0.5, 0.0, 0.0), 11, 0, [a, (poses, f3, a3, o3)], M(max_submaps=4), [(1, 1), (1, 2)])
    # a track with no closed submap
    open_only = (poses[:3], first[:1], anchor[:1], off[:2])
    check(capi, (0.5, 0.0, 0.0), 11, -1, [open_only], M(max_submaps=4), [])
    check(capi, (0.5, 0.0, 0.0), 11, 0, [a, open_only, b], M(max_submaps=4), [(2, 0), (2, 1)])
    # min_path is not read
    assert check(capi, (0.5, 0.0, 0.0), 11, 0, [a, b], M(max_submaps=4, min_path=1e9)).tobytes() == \
        check(capi, (0.5, 0.0, 0.0), 11, 0, [a, b], M(max_submaps=4, min_path=0.0)).tobytes()


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_more_eligible_submaps_than_asked_for(capi, k):
    M = capi.default_loop_multi_params
    rng = np.random.default_rng(41)
    tracks = [track(line(0.0, 0.0, 24, step=0.3) + np.append(rng.normal(0, 0.2, 2), 0.0), 3) for _ in range(3)]
    p = M(max_submaps=k, radius=3.0)
    every = cross_gate_ref(capi, (2.0, 0.1, 30.0), 40, 1, tracks, M(max_submaps=4, radius=3.0))
    assert len(every) == 4                                                   # (more are eligible than any call may ask for)
    got = check(capi, (2.0, 0.1, 30.0), 40, 1, tracks, p)
    assert len(got) == k and got.tobytes() == every[:k].tobytes()
    assert len({g["cand"]["lattice"].tobytes() for g in got}) == 1


def test_refusals(capi):
    M = capi.default_loop_multi_params
    a, b = track(line(0.0, 0.0, 12), 4), track(line(0.0, 0.4, 12), 4)
    nan = float("nan")
    for kw, text in ((dict(max_submaps=0), "max_submaps must be in 1 .. 4"), (dict(max_submaps=5), "max_submaps must be in 1 .. 4"),
                     (dict(max_d2=nan), "max_d2 is NaN or negative"), (dict(min_overlap=1.5), "min_overlap is NaN or outside [0, 1]"),
                     (dict(radius=-1.0), "negative or not finite"), (dict(half_x=-1), "a negative half extent"),
                     (dict(half_x=2048, half_y=2048, half_yaw=0), "more than 2^24 poses"), (dict(top_k=9), "top_k must be in 1 .. 8"),
                     (dict(max_cost=nan), "max_cost is NaN")):
        with pytest.raises(capi.NdtError, match=re.escape("ndt_cross_gate: ") + ".*" + re.escape(text)):
            capi.cross_gate((0.0, 0.0, 0.0), 0, -1, [a, b], M(**kw))
    bad = b[0].copy(); bad[3, 1] = np.inf
    with pytest.raises(capi.NdtError, match=re.escape("ndt_cross_gate: track 1: scan 3: a pose is not finite")):
        capi.cross_gate((0.0, 0.0, 0.0), 0, -1, [a, (bad,) + b[1:]], M())
    with pytest.raises(capi.NdtError, match=re.escape("ndt_cross_gate: track 0: submap 0: ") + ".*is not a set's layout"):
        capi.cross_gate((0.0, 0.0, 0.0), 0, -1, [(a[0], a[1] + 1, a[2], a[3]), b], M())
    with pytest.raises(capi.NdtError, match=re.escape("ndt_cross_gate: track 1: need 1 <= n_scans")):
        capi.cross_gate((0.0, 0.0, 0.0), 0, -1, [a, (np.zeros((0, 3)), b[1][:1], b[2][:1], b[3][:2])], M())
    for last in ((nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -np.inf)):
        with pytest.raises(capi.NdtError, match="the last pose is not finite"):
            capi.cross_gate(last, 0, -1, [a, b], M())
    for own in (-2, 2, 1 << 30):
        with pytest.raises(capi.NdtError, match=re.escape("own is outside [-1, n_tracks)")):
            capi.cross_gate((0.0, 0.0, 0.0), 0, own, [a, b], M())
    with pytest.raises(capi.NdtError, match="n_tracks < 1"):
        capi.cross_gate((0.0, 0.0, 0.0), 0, -1, [], M())
    # (more than 2^28 pairs: tests/test_gpu_cross_gate.py, where many searchers make the product with small arrays)
    lib, k, p = capi.lib(), ctypes.c_int(), M()
    assert lib.ndt_cross_gate(None, 0, -1, None, 1, None, None, None) == capi.NDT_E_ARG
    assert lib.ndt_last_error(None).decode() == "ndt_cross_gate: NULL pointer"
    assert lib.ndt_cross_gate_batch(None, None, None, None, 0, None, 1, None, None, None) == capi.NDT_E_ARG
    assert lib.ndt_last_error(None).decode() == "null context"
    assert lib.ndt_sessions_cross_candidates(None, None, None, ctypes.byref(p), None, ctypes.byref(k)) == capi.NDT_E_ARG
    assert lib.ndt_last_error(None).decode() == "null session set"
    assert lib.ndt_sessions_find_cross_loops(None, None, None, ctypes.byref(p), None, ctypes.byref(k), None) == capi.NDT_E_ARG
    assert lib.ndt_last_error(None).decode() == "null session set"


def test_cross_graph_indices_against_a_hand_written_case(capi):
    from ndt_slam_amd import replay
    info = [10.0, 0.0, 0.0, 10.0, 0.0, 5.0]
    t0, t1, t2 = line(0.0, 0.0, 3, step=1.0), line(0.0, 1.0, 2, step=1.0), line(5.0, 0.0, 4, step=1.0)

    def edge(frm, to, rel):
        e = np.zeros(1, dtype=capi.PG_EDGE_DTYPE)[0]
        e["from"], e["to"], e["rel"], e["info"] = frm, to, rel, [1.0, 0.0, 0.0, 2.0, 0.0, 3.0]
        return e
    own_loop = edge(0, 3, (0.5, 0.0, 1.0))                                   # inside trajectory 2
    cross = [(0, 2, edge(1, 3, (0.1, 0.2, 0.3))), (2, 1, edge(2, 1, (0.4, 0.5, 0.6)))]
    nodes, arcs, off = replay.cross_graph([t0, t1, t2], [[], [], [own_loop]], cross, info)
    assert off.tolist() == [0, 3, 5, 9] and nodes.tobytes() == np.concatenate([t0, t1, t2]).tobytes()
    pairs = list(zip(arcs["from"].tolist(), arcs["to"].tolist()))
    assert pairs == [(0, 1), (1, 2),                  # trajectory 0's odometry
                     (3, 4),                          # trajectory 1's
                     (5, 6), (6, 7), (7, 8), (5, 8),  # trajectory 2's, then its own loop
                     (1, 8), (7, 4)]                  # the cross edges: from + offset of a, to + offset of b
    assert arcs["rel"][7].tolist() == [0.1, 0.2, 0.3] and arcs["rel"][8].tolist() == [0.4, 0.5, 0.6]
    assert arcs["info"][7].tolist() == [1.0, 0.0, 0.0, 2.0, 0.0, 3.0] and arcs["info"][0].tolist() == info
    # each trajectory's own arcs are loops_graph's, shifted
    g2 = replay.loops_graph(t2, [own_loop], info)
    assert arcs["rel"][3:7].tobytes() == g2["rel"].tobytes() and (arcs["from"][3:7] - 5).tolist() == g2["from"].tolist()
    with pytest.raises(ValueError, match="does not tie two trajectories"):
        replay.cross_graph([t0, t1], [[], []], [(0, 0, own_loop)], info)
    with pytest.raises(ValueError, match="one list of loop edges per trajectory"):
        replay.cross_graph([t0, t1], [[]], [], info)
