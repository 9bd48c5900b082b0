"""ndt_cross_gate_batch on the device against ndt_cross_gate on the host, searcher by searcher and byte for byte: numbers of
searchers around the workgroup's 256 threads and a wave's 64 lanes, rows around the 256 threads that stage them and the 1024
poses staged at a time, one row and 300 rows -- the same track 300 times, so that the best four come from ties between rows
of different threads and waves --, coordinates around (0, 0) and around (8191.7, 8191.7), where the squared distances round,
and every max_submaps."""
import re

import numpy as np
import pytest

from cross_loops_helpers import line, track
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu


def assert_batch_is_the_host_gate(capi, ctx, last, newest, own, tracks, p):
    got = capi.cross_gate_batch(ctx, last, newest, own, tracks, p)
    assert len(got) == len(last)
    n_cand = 0
    for i in range(len(last)):
        ref = capi.cross_gate(last[i], int(newest[i]), int(own[i]), tracks, p)          # (a fresh array: no copy, which would drop the padding)
        ref["cand"]["session"] = i
        assert len(got[i]) == len(ref), (i, len(got[i]), len(ref))
        assert np.ascontiguousarray(got[i]).tobytes() == ref.tobytes(), i
        n_cand += len(ref)
    return got, n_cand


def duplicated(origin, row_len, n_rows):
    """One track -- a closed submap of row_len scans along a gentle arc, and an open one -- n_rows times."""
    k = np.arange(row_len + 1, dtype=np.float64)
    poses = np.stack([origin[0] + 0.013 * k, origin[1] + 0.4 * np.sin(0.05 * k), 3.0 * k], axis=1)
    first = np.array([0, row_len], np.int32)
    one = (poses, first, np.array([row_len // 2, row_len], np.int32), np.array([0, 50, 60], np.uint64))
    return [one] * n_rows


def searchers(origin, n, n_tracks, span, seed):
    """n searchers scattered over the track's extent (a few far outside the radius), some of them owning a track."""
    rng = np.random.default_rng(seed)
    last = np.stack([origin[0] + rng.uniform(-1.0, span + 1.0, n), origin[1] + rng.uniform(-1.5, 1.5, n), rng.uniform(-180, 180, n)], axis=1)
    last[::7, 1] += 40.0
    own = np.where(rng.random(n) < 0.5, rng.integers(0, min(n_tracks, 6), n), -1).astype(np.int32)
    return last, rng.integers(0, 5000, n).astype(np.int32), own


@pytest.mark.parametrize("origin", [(0.0, 0.0), (8191.7, 8191.7)], ids=["origin", "far"])
@pytest.mark.parametrize("n_rows", [1, 300])
@pytest.mark.parametrize("row_len", [1, 255, 256, 257, 1000, 1024, 1025, 2500])
def test_rows_of_every_length_one_row_and_three_hundred(gpu, origin, n_rows, row_len):
    capi, ctx = gpu
    tracks = duplicated(origin, row_len, n_rows)
    last, newest, own = searchers(origin, 65, n_rows, 0.013 * row_len, seed=row_len)
    total = 0
    for k in (1, 2, 3, 4):
        p = capi.default_loop_multi_params(max_submaps=k, radius=1.0)
        got, n = assert_batch_is_the_host_gate(capi, ctx, last, newest, own, tracks, p)
        total += n
        if n_rows == 300:
            # all rows tie: a searcher with a candidate has max_submaps of them, the lowest tracks that are not its own
            for i, g in enumerate(got):
                if len(g):
                    assert g["map_session"].tolist() == [t for t in range(k + 1) if t != own[i]][:k], (i, own[i])
                    assert len({np.float64(v).tobytes() for v in g["d2"]}) == 1
    assert total > 0                                                         # (the scatter reaches the track)


@pytest.mark.parametrize("origin", [(0.0, 0.0), (8191.7, 8191.7)], ids=["origin", "far"])
@pytest.mark.parametrize("n_search", [1, 63, 64, 65, 257])
def test_numbers_of_searchers_around_a_wave_and_a_workgroup(gpu, origin, n_search):
    capi, ctx = gpu
    for n_rows in (1, 300):
        tracks = duplicated(origin, 257, n_rows)
        last, newest, own = searchers(origin, n_search, n_rows, 0.013 * 257, seed=n_search)
        last[0, :2] = tracks[0][0][100, :2]                                  # (searcher 0 stands on a pose: d2 = 0)
        own[0] = -1
        for k in ((1, 2, 3, 4) if n_rows == 1 else (1, 4)):
            got, _ = assert_batch_is_the_host_gate(capi, ctx, last, newest, own, tracks, capi.default_loop_multi_params(max_submaps=k, radius=1.0))
            assert len(got[0]) == min(k, n_rows) and float(got[0][0]["d2"]) == 0.0 and int(got[0][0]["cand"]["nearest_scan"]) == 100


@pytest.mark.parametrize("origin", [(0.0, 0.0), (8191.7, 8191.7)], ids=["origin", "far"])
def test_mixed_tracks_with_empty_ranges_empty_clouds_and_open_tracks(gpu, origin):
    """Tracks of different lengths and cuts, some rows that nobody may pick, several closed submaps per track."""
    capi, ctx = gpu
    rng = np.random.default_rng(77)
    tracks = []
    for t in range(23):
        n, per = int(rng.integers(3, 400)), int(rng.integers(1, 40))
        poses, first, anchor, off = track(line(origin[0] + rng.uniform(-3, 3), origin[1] + rng.uniform(-3, 3), n, step=0.05,
                                               heading_deg=float(rng.uniform(-180, 180))), per)
        off = off.copy()
        if t % 5 == 1 and len(first) > 2:
            off[2:] -= 100                                                   # submap 1's cloud is empty
        if t % 5 == 2:
            first, anchor = np.concatenate([[0], first]).astype(np.int32), np.concatenate([[0], anchor]).astype(np.int32)
            off = (np.arange(len(first) + 1) * 100).astype(np.uint64)        # submap 0 has no scan of its own
        if t % 5 == 3:
            poses, first, anchor, off = poses[:2], first[:1], np.zeros(1, np.int32), off[:2]      # no closed submap
        tracks.append((poses, first, anchor, off))
    last = np.stack([origin[0] + rng.uniform(-4, 4, 130), origin[1] + rng.uniform(-4, 4, 130), rng.uniform(-180, 180, 130)], axis=1)
    own = rng.integers(-1, len(tracks), 130).astype(np.int32)
    newest = rng.integers(0, 900, 130).astype(np.int32)
    sizes = set()
    for k in (1, 2, 3, 4):
        for radius in (0.3, 2.0):
            got, _ = assert_batch_is_the_host_gate(capi, ctx, last, newest, own, tracks, capi.default_loop_multi_params(max_submaps=k, radius=radius))
            sizes |= {len(g) for g in got}
    assert sizes == {0, 1, 2, 3, 4}                                          # searchers with none, with fewer than asked, with all
    # no closed submap anywhere, and no searcher: nothing is launched, nothing is found
    open_only = [t for i, t in enumerate(tracks) if i % 5 == 3]
    assert all(len(g) == 0 for g in capi.cross_gate_batch(ctx, last, newest, np.full(130, -1, np.int32), open_only, capi.default_loop_multi_params()))
    assert capi.cross_gate_batch(ctx, np.zeros((0, 3)), [], [], tracks, capi.default_loop_multi_params()) == []


def test_refusals(gpu):
    capi, ctx = gpu
    M = capi.default_loop_multi_params
    a = track(line(0.0, 0.0, 12), 4)
    last, newest, own = np.zeros((2, 3)), np.zeros(2, np.int32), np.full(2, -1, np.int32)
    with pytest.raises(capi.NdtError, match=re.escape("ndt_cross_gate_batch: ") + ".*max_submaps must be in 1 .. 4"):
        capi.cross_gate_batch(ctx, last, newest, own, [a], M(max_submaps=5))
    bad = last.copy(); bad[1, 0] = np.nan
    with pytest.raises(capi.NdtError, match="searcher 1: the last pose is not finite"):
        capi.cross_gate_batch(ctx, bad, newest, own, [a], M())
    with pytest.raises(capi.NdtError, match=re.escape("searcher 1: own is outside [-1, n_tracks)")):
        capi.cross_gate_batch(ctx, last, newest, np.array([0, 1], np.int32), [a], M())
    with pytest.raises(capi.NdtError, match=re.escape("ndt_cross_gate_batch: track 1: submap 0: ")):
        capi.cross_gate_batch(ctx, last, newest, own, [a, (a[0], a[1] + 1, a[2], a[3])], M())
    # more than 2^28 (searcher, closed submap) pairs: 2^15 searchers against 2^13 + 1 rows; refused before anything is queued
    many = track(line(0.0, 0.0, (1 << 13) + 2, step=0.01), 1)
    n = 1 << 15
    with pytest.raises(capi.NdtError, match=re.escape("more than 2^28 (searcher, closed submap) pairs")):
        capi.cross_gate_batch(ctx, np.zeros((n, 3)), np.zeros(n, np.int32), np.full(n, -1, np.int32), [many], M())
    # the context is as usable as before
    assert len(capi.cross_gate_batch(ctx, last, newest, own, [a], M(max_submaps=4))[0]) == 2
