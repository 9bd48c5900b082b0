"""tests/occ_rebuild_workloads.py without a GPU: every family is what it claims to be on the reference alone, the closed form
the device is held to equals the textbook Bresenham walk on the very beams of families 1 to 3, the exact-heading round trips
are bit-exact, the rounding family's two cell sets differ, the dealing rule is a permutation, and every raw scan is legal
session input."""
import math

import numpy as np
import pytest

import occ_helpers as H
import occ_rebuild_workloads as W


def sessions_of(family):
    return [s for s in W.aimed_sessions() if s.family == family]


def test_octants_hold_every_tie_and_degenerate_beam_in_every_sign_combination():
    for s in sessions_of("octants"):
        g = s.casts[0][0]
        for x, q in zip(s.scans, s.poses):
            c = W.octant_conditions(g, q[:2], W.map_points(x, q))
            print(s.name, q[2], c)
            assert c.pop("all live") and all(v >= 1 for v in c.values()), (s.name, q, c)
            assert c["L == 0"] == 1 and c["origin passes"] == 68 * 52 - 1
    assert [len(s.scans) for s in sessions_of("octants")] == [4, 1, 4, 1]
    assert [s.exact for s in sessions_of("octants")] == [True, False, True, False]


@pytest.mark.parametrize("shape", W.BORDER_SHAPES)
def test_borders_cross_and_miss_and_have_origins_on_every_side(shape):
    c = W.border_conditions(shape)
    print(shape, c)
    n, n_hit, n_pass, n_skip = c["crossing"]
    assert n == 5 and n_pass > 0 and n_hit == 0 and n_skip == 0 and c["missing"] == (5, 0, 0, 0)
    assert c["origins inside"] == [False, False, False, True, False, False, False, False]
    g, _, cells, _, _ = W.border_scans(shape)
    sides = {(int(np.sign(cx - min(max(cx, 0), g.nx - 1))), int(np.sign(cy - min(max(cy, 0), g.ny - 1)))) for cx, cy in cells}
    assert {(-1, 0), (1, 0), (0, -1), (0, 1), (0, 0)} <= sides and any(a and b for a, b in sides), sides


def test_limits_live_lists():
    c = W.limit_conditions()
    print(c)
    assert c["length live"] == W.LEN_LIVE and c["length L on x"] == [65536, 65537, 65535]
    assert c["index live"] == W.INDEX_LIVE and c["index cells"] == W.INDEX_CELLS
    assert c["origin beyond 2^30 live"] == [False, False, False]


def test_range_settings_differ_by_the_beams_at_the_value():
    c = W.range_conditions()
    print(c)
    at, below, zero = c["skipped"]
    assert below - at == c["beams at the value"] >= 1 and zero == c["beams with d2 > 0"] > below


def test_prefix_totals_and_scan_sizes():
    c = W.prefix_conditions()
    print({k: v for k, v in c.items() if k != "beams"})
    assert c["totals"] == list(W.PREFIX_TOTALS) + [256, 257]
    assert all(b == [3, 3, 3, 3, T - 12] for b, T in zip(c["beams"], W.PREFIX_TOTALS))
    assert c["long beam"] == 5001 > c["the rest of its run"] >= 255
    assert c["scan sizes"] == list(W.SCAN_SIZES) == [0, 1, 63, 64, 65, 0, 0, 255, 256, 257, 513, 1025, 0]


def test_contention_counts_on_the_origin_cell():
    c = W.contention_conditions()
    print(c)
    assert c == {"all live": True, "origin passes": 4096 - 64, "L >= 1": 4096 - 64, "origin hits": 64}


def test_rounding_moves_the_cell_on_both_axes():
    (x64, y64), (x32, y32) = W.rounding_cells()
    print("beams whose float32 cell differs on x: %d, on y: %d, of %d" % ((x64 != x32).sum(), (y64 != y32).sum(), len(x64)))
    assert (x64 != x32).sum() >= 16 and (y64 != y32).sum() >= 16 and ((x64 != x32) & (y64 != y32)).sum() >= 8
    assert (x32 - x64)[x64 != x32].tolist() == [1] * int((x64 != x32).sum()) and ((y32 - y64)[y64 != y32] == 1).all()
    g = W.ROUNDING_GEOM
    assert x32.min() >= 0 and x32.max() < g.nx and y32.min() >= 0 and y32.max() < g.ny


def test_exact_heading_round_trips_are_bit_exact():
    """aimed() asserts the round trip of every scan when the module builds it; here once more, from the finished sessions, with
    the wanted points made again."""
    n = 0
    for s in W.aimed_sessions() + W.many_sessions(70) + W.many_sessions(90) + W.dealing_sessions():
        assert s.exact == bool(np.isin(s.poses[:, 2], W.EXACT_HEADINGS).all())
        if not s.exact or s.family == "rounding":
            continue
        for x, q in zip(s.scans, s.poses):
            m = W.map_points(x, q)
            assert W.map_points(W.to_robot(m, q), q).tobytes() == m.tobytes(), (s.name, q)
            n += 1
    ends = W.all_ends(W.EXACT_GEOM)
    s = W.by_name("octants-exact")
    assert all(W.map_points(x, q).tobytes() == ends.tobytes() for x, q in zip(s.scans, s.poses)) and n > 300
    # at heading 0 the fp64 points are the wanted ones themselves; at the others sin or cos is 6e-17 or 1.2e-16, not 0
    assert s.poses[0][2] == 0.0 and np.array_equal(W.to_map_frame(s.scans[0], s.poses[0]), ends.astype(np.float64))


def test_the_closed_form_is_the_bresenham_walk_on_every_live_beam_of_families_1_to_3():
    seen, n_cells = set(), 0
    for s in W.aimed_sessions():
        if s.family not in ("octants", "borders", "limits"):
            continue
        for g, r2 in s.casts:
            for x, q in zip(s.scans, s.poses):
                live, X1, Y1, X0, Y0 = H.classify(g, q[:2], W.map_points(x, q), r2)
                for i in np.nonzero(live)[0]:
                    key = (int(X1[i]) - X0, int(Y1[i]) - Y0)      # (both forms are translation-invariant)
                    if key in seen:
                        continue
                    seen.add(key)
                    cells, end = H.walk(0, 0, *key)
                    xs, ys = H.closed_form(0, 0, *key)
                    assert end == key and cells == list(zip(xs.tolist(), ys.tolist())), (s.name, key)
                    n_cells += len(cells)
    print("distinct beams walked: %d, cells: %d" % (len(seen), n_cells))
    assert (65536, 0) in seen and (-65535, 0) in seen and (65536, 65536) in seen and (0, 0) in seen and len(seen) > 5000


def test_many_scans_put_the_round_of_256_inside_a_row():
    c = W.many_conditions(70)
    print(70, c)
    assert c["scans"] == [70, 70, 65, 70] and c["scans named"] == [275, 205] and c["session of scan 256"] == [3, None]
    assert c["beams"] == [1, 2, 3]
    c = W.many_conditions(90)                            # (every naming with a second round, its boundary in another row)
    print(90, c)
    assert c["scans"] == [90, 90, 85, 90] and c["scans named"] == [355, 265, 270] and c["session of scan 256"] == [2, 3, 3]
    assert all(256 not in f for f in c["first scan of every row"])      # ... and inside the row, not at its first scan


def test_the_dealing_rule_is_a_permutation_with_strides_other_than_one():
    combos = W.dealing_combinations()
    print([(n, T, stride, bumps) for _, _, n, T, stride, bumps in combos])
    assert {1, 2, 3, 4, 6, 8, 9} <= {c[2] for c in combos} and {c[3] for c in combos} == {1, 2, 3}
    for _, _, n, T, stride, bumps in combos:
        assert math.gcd(stride, n) == 1 and stride == max(1, n // T) + bumps
        assert sorted((v * stride) % n for v in range(n)) == list(range(n)), (n, T, stride)
    assert any(c[4] != 1 for c in combos) and any(c[5] == 2 for c in combos) and any(c[5] >= 2 and c[3] == 3 for c in combos)
    assert [len(s.scans) for s in W.dealing_sessions()] == [1, 1, 6]
    assert [[-(-len(x) // 256) for x in s.scans] for s in W.dealing_sessions()] == [[1], [2], [1] * 6]


def test_every_raw_scan_is_legal_session_input():
    for s in W.aimed_sessions() + W.many_sessions(70) + W.many_sessions(90) + W.dealing_sessions():
        assert len(s.scans) == len(s.poses) and np.isfinite(s.poses).all(), s.name
        for x in s.scans:
            assert x.dtype == np.float64 and x.ndim == 2 and x.shape[1] == 2 and np.isfinite(x).all(), s.name
            assert not len(x) or np.abs(x).max() <= W.MAX_ROBOT_RANGE, (s.name, np.abs(x).max())
    names = [s.name for s in W.aimed_sessions()]
    assert len(set(names)) == len(names) == 14 and len(W.aimed_cases()) == 21
