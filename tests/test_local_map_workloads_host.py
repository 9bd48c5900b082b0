"""The clouds of tests/local_map_workloads.py, on the CPU: the restated constants against the header, the census (every
family reaches the labels it is for, all of them every label, both sides of every constant, nothing left out), the
oracle's pointer octree against the replay on every case, and the teeth: wrong replays that each family tells apart."""
import os
import re

import numpy as np
import pytest

import local_map_workloads as W

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ndt_slam_amd", "csrc")


def labels(case):
    if "_labels" not in case:                      # (once per case: several tests ask)
        case["_labels"] = W.census(case["base"], case["test"], case["resol"], W.case_replay(case))
    return case["_labels"]


def test_restated_constants_are_the_headers():
    src = open(os.path.join(CSRC, "ndt_localmap.hip.h")).read()
    found = {}
    for line in re.findall(r"^constexpr int ([^;]+);", src, re.M):
        for name, value in re.findall(r"(\w+) = ([^,]+)", line):
            found[name] = value.strip()
    for name, value in W.HEADER_CONSTANTS.items():
        assert found[name] == str(value), name
    assert "lfill, 1) >= kMmLdsTab * 3 / 4" in src and W.LDS_LIMIT == 12288
    assert "for (int g0 = 0; g0 < N; g0 += kMmGroup * kMmBlock)" in src and W.GROUP_POINTS == 8192
    assert "c0 += kMmPer * kMmBlock" in src and W.CHUNK_POINTS == 4096
    assert "rem > res * 1e-6 && rem < res * (1.0 - 1e-6)" in src and W.CELL_BAND == 1e-6
    assert src.count("block_excl_offsets<1024>(") == 2 and src.count("__launch_bounds__(1024)") == 2 and W.SCAN_WIDTH == 1024
    host = open(os.path.join(CSRC, "ndt_mi355x.hip")).read()
    assert "prefilter_offsets_kernel<kTarget><<<1, 1024, 0, st>>>" in host
    assert "make_map_sub_scan_kernel<<<1, 1024, 0, st>>>" in host and "make_map_sub_offsets_kernel<<<(unsigned)ns, 1024, 0, st>>>" in host


# ---- census ----

@pytest.mark.parametrize("family", list(W.DIFF_FAMILIES))
def test_every_difference_family_reaches_its_labels(family):
    for resol, origin in W.family_grid(family):
        cases = W.DIFF_FAMILIES[family](resol, origin)
        got = set().union(*[labels(c) for c in cases])
        assert W.DIFF_FAMILY_LABELS[family] <= got, (resol, origin, sorted(W.DIFF_FAMILY_LABELS[family] - got))
        for c in cases:
            assert len(c["base"]) + len(c["test"]) <= 26500 and c["base"].dtype == c["test"].dtype == np.float32


@pytest.mark.parametrize("family", list(W.ASM_FAMILIES))
def test_every_assembly_family_reaches_its_labels(family):
    for resol, origin in W.GRID:
        cases = W.ASM_FAMILIES[family](resol, origin)
        got = set().union(*[W.assembly_census(c["items"], W.case_reference(c)) for c in cases])
        assert W.ASM_FAMILY_LABELS[family] <= got, (resol, origin)
        for c in cases:
            assert sum(len(x) for it in c["items"] for x in it[0]) <= 35000


def test_all_families_reach_every_label_and_nothing_is_left_out():
    got = set()
    for _, _, c in W.difference_cases():
        got |= labels(c)
    for _, _, c in W.assembly_cases():
        got |= W.assembly_census(c["items"], W.case_reference(c))
    assert got == W.ALL_LABELS, sorted(W.ALL_LABELS ^ got)
    # Every case built is a case compared: the GPU file and the oracle tests below walk these two lists whole, and a
    # case has a reference result or is refused by construction.
    ids = [cid for cid, _, _ in W.difference_cases() + W.assembly_cases()]
    assert len(ids) == len(set(ids))
    left_out = [cid for cid, _, c in W.difference_cases() if (W.case_replay(c).idx is None) != c["refused"]]
    left_out += [cid for cid, _, c in W.assembly_cases()
                 if [s for s, r in enumerate(W.case_reference(c)) if r is None] != c.get("refused", [])]
    assert left_out == []
    print("%d difference cases, %d assembly cases, 0 left out" % (len(W.difference_cases()), len(W.assembly_cases())))


def test_both_sides_of_every_constant():
    for resol, origin in W.GRID:
        # the LDS set's limit: 12287 .. 12290 distinct base keys, exactly
        for c in W.set_limit(resol, origin):
            assert len(W.case_replay(c).base_keys) == c["keys"]
        assert [c["keys"] for c in W.set_limit(resol, origin)] == [W.LDS_LIMIT - 1, W.LDS_LIMIT, W.LDS_LIMIT + 1, W.LDS_LIMIT + 2]
        # the growth replay's groups: doublings asked for by the last point of a group, the first and the second of the
        # next, the first of the third; by the last base point and the first test point
        singles = W.group_edges(resol, origin)[0]
        at = {i for i, _, _ in W.case_replay(singles).events}
        nA, G = len(singles["base"]), W.GROUP_POINTS
        assert {G - 1, G, G + 1, 2 * G, nA - 1, nA} <= at
        multi = W.case_replay(W.group_edges(resol, origin)[1])
        assert sum(1 for i, _, _ in multi.events if i == G) >= 5
        last = W.group_edges(resol, origin)[3]
        assert W.case_replay(last).events[-1][0] == len(last["base"]) + len(last["test"]) - 1 >= G
        # the 30 levels: the last accepted float and the next one, for both signs and three places of the far point
        for ok, no in zip(W.span_edge(resol, origin)[::2], W.span_edge(resol, origin)[1::2]):
            assert W.case_replay(ok).depth == W.K_MAX_DEPTH and W.case_replay(no).depth is None
            assert np.nextafter(np.float32(ok["far_x"]), np.float32(no["far_x"])) == np.float32(no["far_x"])
        assert [len(c["test"]) for c in W.chunks(resol, origin)] == [4095, 4096, 4097, 8193]
        assert [c["n_list"] for c in W.list_tiles(resol, origin)] == [1023, 1024, 1025, 2049]
        for c in W.list_tiles(resol, origin):
            assert W.case_reference(c)[0][1][1][2] == c["n_list"]           # the triple's new-voxel points, by the replay
        assert {255, 256, 257, 513} <= {len(x) for x in W.unit_tails(resol, origin)[0]["items"][0][0]}
        units = [len(W.unit_counts(W.case_reference(c)[0][1])) for c in W.long_submap(resol, origin)]
        assert units == [1024, 1024, 1100, 1100]
        assert [len(c["items"]) for c in W.many_submaps(resol, origin)] == [1025, 2050]
    # the band of mm_cell: keys taken inside it and just outside it
    border = [d for _, _, c in W.difference_cases() for _, d in W.case_replay(c).border]
    assert any(d <= W.CELL_BAND for d in border) and any(W.CELL_BAND < d < 1e-4 for d in border)
    # wave_runs: every run length asked for, starting on a multiple of 64 and off one
    runs = W.wave_runs(0.05, W.ORIGINS[0])[0]["runs"]
    starts = np.concatenate([[0], np.cumsum(runs)[:-1]])
    for n in (63, 64, 65, 129):
        assert {bool(s % 64) for s, m in zip(starts, runs) if m == n} == {False, True}, n
    assert 1 in runs


# ---- oracle against replay ----

@pytest.mark.parametrize("family", list(W.DIFF_FAMILIES))
def test_octree_equals_the_replay_on_every_difference_case(oracle, family):
    n = 0
    for resol, origin in W.family_grid(family):
        for c in W.DIFF_FAMILIES[family](resol, origin):
            R = W.case_replay(c)
            if c["refused"]:
                assert R.idx is None
                with pytest.raises(ValueError):
                    oracle.difference_indices(c["base"], c["test"], c["resol"])
                with pytest.raises(W.Refused):
                    W.replay_difference(c["base"], c["test"], c["resol"])
            else:
                idx = np.sort(oracle.difference_indices(c["base"], c["test"], c["resol"]))
                assert np.array_equal(idx, R.idx), (family, resol, origin, c["name"])
                # something is new, something is not -- but for a cloud that meets an empty set, and at the span's edge,
                # where base and test can lie in frames whose z keys differ throughout
                nd, nb = len(R.idx), len(c["test"])
                assert 0 < nd and (nd < nb or family == "span_edge" or c.get("free") == "most"), (family, resol, origin, c["name"])
            n += 1
    assert n == len(W.family_grid(family)) * len(W.DIFF_FAMILIES[family](*W.GRID[0]))


@pytest.mark.parametrize("family", list(W.ASM_FAMILIES))
def test_make_map_equals_assemble_on_every_assembly_case(oracle, family):
    for resol, origin in W.GRID:
        for c in W.ASM_FAMILIES[family](resol, origin):
            ref = W.case_reference(c)
            kept = total = removable = 0
            for s, (it, r) in enumerate(zip(c["items"], ref)):
                if r is None:
                    with pytest.raises(ValueError):
                        oracle.make_map(*it[:6])
                    continue
                assert oracle.make_map(*it[:6]).tobytes() == r[0].tobytes(), (family, resol, origin, c["name"], s)
                kept += len(r[0])
                if it[3]:
                    removable += sum(len(k) - int(k.sum()) for _, k, nd in r[1] if nd is not None)
                    total += 1
            assert kept > 0 and (removable > 0 or total == 0), (family, resol, origin, c["name"])      # keeps, and removes where asked


# ---- teeth ----

def test_a_lattice_in_x_and_y_alone_is_told_apart():
    """deep_split: with the z key left out the index set changes in `far_mid` everywhere (and in `snapped` nearly
    everywhere), never in the control; the shallow z cases of the other families likewise."""
    toothless = []
    for resol, origin in W.family_grid("deep_split"):
        mid, first, snapped = W.deep_split(resol, origin)
        assert not np.array_equal(W.indices_keyed_by_xy(mid), W.case_replay(mid).idx), (resol, origin)
        assert np.array_equal(W.indices_keyed_by_xy(first), W.case_replay(first).idx) and "z:split_deep" not in labels(first)
        if np.array_equal(W.indices_keyed_by_xy(snapped), W.case_replay(snapped).idx):
            toothless.append((resol, origin))
    assert len(toothless) <= 1
    shallow = [(cid, c) for cid, f, c in W.difference_cases() if not c["refused"] and "z:split_shallow" in labels(c)]
    differ = [cid for cid, c in shallow if not np.array_equal(W.indices_keyed_by_xy(c), W.case_replay(c).idx)]
    assert len(shallow) >= 40 and len(differ) >= 0.75 * len(shallow)
    print("snapped, toothless:", toothless, "| shallow z cases: %d of %d differ" % (len(differ), len(shallow)))


def test_keys_taken_in_the_final_frame_and_lost_group_carries():
    """Keying every point against the final box minimum moves no x or y key of these clouds, the lattice-snapped ones
    included: it differs from the replay exactly where the (x, y) lattice does (reported, not a tooth of its own).  What
    group_edges does tell apart is a growth replay that loses the doublings of the second and later groups."""
    same = [cid for cid, f, c in W.difference_cases() if not c["refused"] and f in ("deep_split", "group_edges")
            and np.array_equal(W.indices_keyed_in_final_frame(c), W.indices_keyed_by_xy(c))]
    total = sum(1 for _, f, c in W.difference_cases() if f in ("deep_split", "group_edges"))
    print("final-frame keys equal the x-y lattice's on %d of %d cases" % (len(same), total))
    toothless = []
    for resol, origin in W.GRID:
        for c in W.group_edges(resol, origin)[:3] + W.nonfinite(resol, origin)[2:]:
            if np.array_equal(W.indices_without_late_shifts(c), W.case_replay(c).idx):
                toothless.append((resol, origin, c["name"]))
        # the violator that ends the test cloud has nobody behind it to mis-key: what it holds is the event itself
        last = W.group_edges(resol, origin)[3]
        assert np.array_equal(W.indices_without_late_shifts(last), W.case_replay(last).idx)
    print("lost carries, toothless:", toothless)
    # at 0.05 no frame's z key deviates, so nothing can mask the lost shift; at the other leaf sizes a test cloud whose
    # frame deviates from the base cloud's is new throughout under either replay
    assert all(r != 0.05 for r, _, _ in toothless) and len(toothless) <= 8


def test_offsets_without_their_carry_misplace_kept_points():
    for resol, origin in W.GRID:
        for c in W.long_submap(resol, origin):
            counts = W.unit_counts(W.case_reference(c)[0][1])
            right, wrong = W.offsets(counts), W.offsets(counts, carry=False)
            moved = [u for u, (a, b) in enumerate(zip(right, wrong)) if a != b and counts[u]]
            assert bool(moved) == (len(counts) > W.SCAN_WIDTH), c["name"]
            if moved:
                assert sum(counts[:W.SCAN_WIDTH]) > 0 and sum(counts[W.SCAN_WIDTH:]) > 0      # kept points on both sides
        for c in W.many_submaps(resol, origin):
            totals = [0 if r is None else len(r[0]) for r in W.case_reference(c)]
            right, wrong = W.offsets(totals), W.offsets(totals, carry=False)
            # (1025 submaps: the one behind the first round is a refused one, so what the lost carry moves is the call's
            # total, cloud_off[1025]; 2050 submaps: clouds themselves)
            assert right[-1] + totals[-1] != wrong[-1] + totals[-1]
            assert len(totals) == W.SCAN_WIDTH + 1 or any(a != b and t for a, b, t in zip(right, wrong, totals))
            assert len(totals) == W.SCAN_WIDTH + 1 or (any(totals[W.SCAN_WIDTH + 1:]) and any(totals[2 * W.SCAN_WIDTH:]))      # (third round: 2048 and the refused last)
            assert len(totals) == W.SCAN_WIDTH + 1 or any(it[6] is not None for it in c["items"][W.SCAN_WIDTH:])
