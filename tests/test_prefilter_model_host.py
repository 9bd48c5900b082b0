"""The pre-filter's Python model (tests/prefilter_workloads.py) against the C oracle the whole suite leans on, the
certificates of the cloud families, and the seeded defects: every way a parallel replay goes wrong that the model can be
switched into changes the output bytes of a named family at the shape its GPU test uses
(tests/test_gpu_prefilter_families.py).  No GPU."""
import numpy as np
import pytest

import prefilter_workloads as W
from test_gpu_prefilter import lidar_like

HOST_LENGTHS = (1, 2, 63, 64, 65, 360, 8192, 8193, 16385, 20000)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("family", sorted(W.FAMILIES))
def test_model_equals_the_oracle_on_every_family(oracle, family):
    make, leaf = W.FAMILIES[family]
    for n in HOST_LENGTHS:
        cloud = make(n)
        assert cloud.shape == (n, 2) and same(W.model(cloud, leaf), oracle.approx_voxel_filter(cloud, leaf)), n


def test_model_equals_the_oracle_on_the_single_voxel_and_the_count_limits(oracle):
    for cloud in (W.no_flush(20000, V=1), W.count_limit(False), W.count_limit(True)):
        assert same(W.model(cloud, 0.05), oracle.approx_voxel_filter(cloud, 0.05))


@pytest.mark.parametrize("leaf", [0.05, 0.1, 0.5])
def test_model_equals_the_oracle_on_the_two_older_shapes(oracle, leaf):
    rng = np.random.default_rng(7)
    for n in (1, 2, 63, 64, 65, 360, 5000, 8192, 8193, 20000):
        for cloud in (lidar_like(rng, n), W.uniform_cloud(rng, n)):
            assert same(W.model(cloud, leaf), oracle.approx_voxel_filter(cloud, leaf)), n


def test_model_batch_is_the_scans_one_by_one():
    scans = [W.eight_slots(n) for n in (70, 0, 1, 300)]
    outs = W.replay_batch(scans, 0.5, 2)
    assert all(same(o, W.model(s, 0.5)) for o, s in zip(outs, scans)) and len(outs[1]) == 0


# ---- certificates (every generator also asserts its own on construction; here at every length the GPU tests use) ----
ALL_LENGTHS = W.SORTED_LENGTHS + W.EIGHT_WAVE_LENGTHS


def test_one_slot_certificate():
    for name, least in (("one_slot_round_robin", 63), ("one_slot_runs", 20)):
        make, leaf = W.FAMILIES[name]
        for n in ALL_LENGTHS + W.LONG_LENGTHS:
            lanes, changes = W.contention(make(n), leaf)
            assert np.all(lanes[:n // 64] == 64) and changes.max() >= least, (name, n)
            if least == 63:
                assert np.all(changes[:n // 64] == 63)                 # every point of every full step flushes


def test_one_wave_certificate():
    make, leaf = W.FAMILIES["one_wave"]
    for n in ALL_LENGTHS + W.LONG_LENGTHS:
        h = W.voxels(make(n), leaf)[2]
        assert len(np.unique(h & 7)) == 1 and len(np.unique(h)) >= 32, n
    lanes, changes = W.contention(make(66113), leaf)
    assert lanes.max() >= 4 and changes.max() >= 3                     # and the slots are contested inside a step


def test_eight_slots_certificate():
    make, leaf = W.FAMILIES["eight_slots"]
    for n in ALL_LENGTHS:
        cloud = make(n)
        ix, iy, h = W.voxels(cloud, leaf)
        assert sorted(np.unique(h)) == list(range(8)), n
        assert n < 8192 or len(set(zip(ix.tolist(), iy.tolist()))) == 24, n
        lanes, changes = W.contention(cloud, leaf)
        assert lanes.max() >= 8 and changes.max() >= 5, n            # 64 lanes in 8 slots; more changes than the older shapes


def test_no_flush_certificate():
    make, leaf = W.FAMILIES["no_flush"]
    for cloud in [make(n) for n in ALL_LENGTHS] + [W.no_flush(20000, V=1)]:
        ix, iy, h = W.voxels(cloud, leaf)
        nvox = len(set(zip(ix.tolist(), iy.tolist())))
        out, causes, _ = W.replay(cloud, leaf)
        assert causes == [] and len(out) == nvox == len(np.unique(h)) <= 512
    assert len(W.model(make(65535), leaf)) == 512 and len(W.model(W.no_flush(20000, V=1), leaf)) == 1


def test_tile_edges_certificate():
    make, leaf = W.FAMILIES["tile_edges"]
    for n in ALL_LENGTHS:
        causes = W.replay(make(n), leaf)[1]
        want = {t + i for t in range(0, n, 8192) for i in (0, 31, 32, 63, 64, 511, 512, 8191) if 0 < t + i < n}
        assert want <= set(causes), n
    assert {8191, 8192, 16383, 16384} <= set(W.replay(make(16385), leaf)[1])


def test_count_limit_certificate():
    parked, tail = W.count_limit(False), W.count_limit(True)
    assert len(parked) == len(tail) == 65535 == W.SORT_MAX
    for cloud, voxels_wanted in ((parked, 2), (tail, 1)):
        ix, iy, h = W.voxels(cloud, 0.05)
        assert len(np.unique(h)) == 1 and len(set(zip(ix.tolist(), iy.tolist()))) == voxels_wanted
    assert W.replay(parked, 0.05)[1] == [65534]                        # one flush, of the 65534 points in front of it


def test_second_round_batch_certificate():
    G = 2048
    scans = W.second_round_batch(G)
    assert len(scans) == G + 100
    later = [len(s) for s in scans[G:]]
    assert later.count(0) >= 5 and later.count(1) >= 5 and len(scans[5]) == len(scans[5 + G]) == 66113
    for b in range(100):
        if b == 5 or not len(scans[b + G]):
            continue
        (ax, ay, ah), (bx, by, bh) = W.voxels(scans[b], W.SECOND_ROUND_LEAF), W.voxels(scans[b + G], W.SECOND_ROUND_LEAF)
        assert set(bh.tolist()) <= set(ah.tolist())                                   # the same slots ...
        assert not set(zip(ax.tolist(), ay.tolist())) & set(zip(bx.tolist(), by.tolist()))    # ... in other voxels
    h5 = W.voxels(scans[5], W.SECOND_ROUND_LEAF)[2]
    assert int(h5[0]) in set(W.voxels(scans[5 + G], W.SECOND_ROUND_LEAF)[2].tolist())


# ---- seeded defects: switch -> the (family, length) pairs that must tell it apart ----
TELLS = {
    "a": [("one_slot_round_robin", 64), ("one_slot_runs", 8193), ("one_slot_round_robin", 66113)],
    "b": [("eight_slots", 64), ("one_wave", 65), ("one_wave", 66113)],
    "c": [("tile_edges", 8193), ("no_flush", 16385), ("one_voxel", 20000)],
    "d": [("one_slot_round_robin", 65), ("one_slot_round_robin", 8192), ("tile_edges", 16385)],
    "f": [("count_limit_parked", 65535)],
}


def family_cloud(name, n):
    if name == "one_voxel":
        return W.no_flush(n, V=1), 0.05
    if name == "count_limit_parked":
        return W.count_limit(False), 0.05
    make, leaf = W.FAMILIES[name]
    return make(n), leaf


@pytest.mark.parametrize("defect", sorted(TELLS))
def test_every_seeded_defect_is_told_apart_by_a_new_family(defect):
    for name, n in TELLS[defect]:
        cloud, leaf = family_cloud(name, n)
        assert not same(W.model(cloud, leaf, defect), W.model(cloud, leaf)), (defect, name, n)


def test_a_state_leak_between_rounds_is_told_apart_by_the_second_round_batch():
    G = 2048
    scans = W.second_round_batch(G)
    good, leaky = W.replay_batch(scans, W.SECOND_ROUND_LEAF, G), W.replay_batch(scans, W.SECOND_ROUND_LEAF, G, "e")
    assert all(same(a, b) for a, b in zip(good[:G], leaky[:G]))
    differ = [b for b in range(G, G + 100) if not same(good[b], leaky[b])]
    assert 5 + G in differ and len(differ) >= 90                       # the long pair, and nearly every tiny one
    assert any(len(scans[b]) == 0 for b in differ) and any(len(scans[b]) == 1 for b in differ)


def test_count_limit_tail_is_untouched_by_the_parked_count():
    """The tail divides by the slot's own 32-bit count: the 15-bit switch must not reach it (the model's, and so the test's,
    idea of where the 16-bit count travels)."""
    cloud = W.count_limit(True)
    assert same(W.model(cloud, 0.05, "f"), W.model(cloud, 0.05))
