"""The source pre-filter's sequential machine in plain Python, the cloud families that load its device replay where the
LiDAR-like and uniform clouds of tests/test_gpu_prefilter.py do not, and what certifies each family.

The machine (pcl::ApproximateVoxelGrid on a z = 0 cloud): 512 direct-mapped slots, slot (ix * 7171 + iy * 3079) & 511 with
ix = floor(x * (1f / leaf)) in float32; a point joins the voxel its slot holds (float32 sums, in cloud order) or flushes that
voxel's centroid to the output and takes the slot; what is left is flushed in slot order at the end.  `replay` is written
from that description alone, not from oracle/ndt_oracle.c: it is the second opinion on the C oracle
(tests/test_prefilter_model_host.py holds the two to each other byte for byte).

`replay` also carries switches for the ways a PARALLEL replay goes wrong (DEFECTS); a family earns its place by telling at
least one of them apart from the true machine.  The device kernels' geometry the switches and certificates speak of:
steps of 64 points (one wave), tiles of 8192 points split into eight wave parts (prefilter_sorted_kernel), read-ahead blocks
of 512 points and ownership of a slot by the wave numbered by the slot's low three bits (prefilter_mw_kernel)."""
import numpy as np

SLOTS = 512
STEP = 64
TILE = 8192
WAVES = 8
SORT_MAX = 65535            # the longest scan of prefilter_sorted_kernel
BITMAP_MAX = 1 << 18        # the longest scan of prefilter_mw_kernel's eight-wave path
F32 = np.float32

DEFECTS = {
    "a": "same-slot lanes of a step served in reverse order when a voxel change lies between them",
    "b": "a step's flushes emitted in slot order instead of point order",
    "c": "a slot's state dropped at a tile boundary",
    "d": "within a tile, a slot's points taken wave-part 1 before part 0",
    "e": "in a batch served by G workgroups, slot state leaks from scan b to scan b + G",
    "f": "the parked count truncated to 15 bits",
}


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
def voxels(xy, leaf):
    """(ix, iy, slot) of every point, as the filter computes them: float32 product with the float32 reciprocal of leaf."""
    xy = np.ascontiguousarray(xy, dtype=F32).reshape(-1, 2)
    inv = F32(1.0) / F32(leaf)
    q = np.floor(xy * inv)
    assert q.dtype == F32
    ix, iy = q[:, 0].astype(np.int64), q[:, 1].astype(np.int64)
    return ix, iy, (ix * 7171 + iy * 3079) & (SLOTS - 1)


def _serving_order(n, ix, iy, h, defect):
    """The order in which the points reach their slots (only the order inside a slot matters)."""
    order = list(range(n))
    if defect == "a":
        for base in range(0, n, STEP):
            groups = {}
            for i in range(base, min(base + STEP, n)):
                groups.setdefault(h[i], []).append(i)
            for g in groups.values():
                if any(ix[p] != ix[q] or iy[p] != iy[q] for p, q in zip(g, g[1:])):
                    for place, i in zip(g, reversed(g)):
                        order[place] = i
    elif defect == "d":
        for base in range(0, n, TILE):
            m = min(TILE, n - base)
            steps = (m + STEP - 1) // STEP
            part = STEP * ((steps + WAVES - 1) // WAVES)             # points of one wave's part
            p0 = list(range(base, base + min(part, m)))
            p1 = list(range(base + min(part, m), base + min(2 * part, m)))
            order[base:base + len(p0) + len(p1)] = p1 + p0
    return order


def replay(xy, leaf, defect=None, state=None):
    """The filter on one scan -> (out [m, 2] float32, causes, state).  causes: the indices of the points that caused a
    flush, in output order (what follows them in `out` is the slot-order tail).  state: the slots as the scan leaves them
    (a dict slot -> [ix, iy, count, sum x, sum y]); given as an argument it is the state the scan starts from (defect e)."""
    xy = np.ascontiguousarray(xy, dtype=F32).reshape(-1, 2)
    n = len(xy)
    vx, vy, vh = voxels(xy, leaf)
    ix, iy, h = vx.tolist(), vy.tolist(), vh.tolist()
    xs, ys = list(xy[:, 0]), list(xy[:, 1])                          # numpy float32 scalars: their sums round to float32
    slots = {} if state is None else {k: list(v) for k, v in state.items()}
    zero = F32(0.0)
    events = []                                                       # (cause, sum x, sum y, count)
    for i in _serving_order(n, ix, iy, h, defect):
        if defect == "c" and i and i % TILE == 0:
            slots.clear()
        e = slots.get(h[i])
        if e is None:
            e = slots[h[i]] = [0, 0, 0, zero, zero]
        if e[2] and (e[0] != ix[i] or e[1] != iy[i]):
            events.append((i, e[3], e[4], e[2]))
            e[2], e[3], e[4] = 0, zero, zero
        e[0], e[1] = ix[i], iy[i]
        e[2] += 1
        e[3] = e[3] + xs[i]
        e[4] = e[4] + ys[i]
    if defect == "b":
        events.sort(key=lambda ev: (ev[0] // STEP, h[ev[0]], ev[0]))
    else:
        events.sort(key=lambda ev: ev[0])                             # a flush stands where the point that caused it stood
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for _, sx, sy, c in events:
            c = F32(c & 0x7FFF if defect == "f" else c)
            out.append((sx / c, sy / c))
        for k in sorted(slots):
            e = slots[k]
            if e[2]:
                out.append((e[3] / F32(e[2]), e[4] / F32(e[2])))
    return np.array(out, dtype=F32).reshape(-1, 2), [ev[0] for ev in events], slots


def model(xy, leaf, defect=None):
    return replay(xy, leaf, defect)[0]


def replay_batch(scans, leaf, G, defect=None):
    """Every scan of a batch that G workgroups serve round robin -> the list of outputs."""
    outs, left = [], {}
    for b, s in enumerate(scans):
        out, _, state = replay(s, leaf, defect, left.get(b % G) if defect == "e" else None)
        left[b % G] = state
        outs.append(out)
    return outs


def contention(xy, leaf):
    """Per step of 64 points: (the most lanes that share a slot, the most voxel changes between neighbouring lanes of one
    slot) -- two int arrays of one entry per step."""
    ix, iy, h = voxels(xy, leaf)
    n = len(h)
    nsteps = (n + STEP - 1) // STEP
    key = (np.arange(n) // STEP) * SLOTS + h
    o = np.argsort(key, kind="stable")
    k, x, y = key[o], ix[o], iy[o]
    lanes = np.zeros(nsteps, np.int64)
    np.maximum.at(lanes, k // SLOTS, np.bincount(k, minlength=nsteps * SLOTS)[k])
    change = (k[1:] == k[:-1]) & ((x[1:] != x[:-1]) | (y[1:] != y[:-1]))
    per_group = np.bincount(k[1:][change], minlength=nsteps * SLOTS)
    return lanes, per_group.reshape(nsteps, SLOTS).max(axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# the families: points at voxel interiors, (index + u) * leaf with u in [0.2, 0.8]
# ---------------------------------------------------------------------------------------------------------------------
def ix_of_slot(h, iy=0, j=0):
    """A voxel column ix with slot(ix, iy) == h: 7171 = 3 and 3079 = 7 modulo 512, and 3 * 171 = 1 modulo 512."""
    return (171 * (np.asarray(h, np.int64) - 7 * np.asarray(iy, np.int64))) % SLOTS + SLOTS * np.asarray(j, np.int64)


def _points(ix, iy, leaf, rng):
    ix, iy = np.asarray(ix, np.int64), np.broadcast_to(np.asarray(iy, np.int64), np.shape(ix))
    u = rng.uniform(0.2, 0.8, (len(ix), 2))
    xy = ((np.stack([ix, iy], 1) + u) * leaf).astype(F32)
    vx, vy, _ = voxels(xy, leaf)
    assert np.array_equal(vx, ix) and np.array_equal(vy, iy), "a rounding of 1 / leaf moved a point out of its voxel"
    return xy


def one_slot(n, K=5, run=1, slot=43, iy=2, leaf=0.05, seed=1):
    """K voxels ix = c + 512 j of one row: every point in one slot.  run == 1: round robin, every point flushes; else random
    runs of 1..run points.  Certificate: 64 lanes of one slot in every full step, >= 20 voxel changes in some step."""
    rng = np.random.default_rng([seed, n, K, run])
    if run == 1:
        j = np.arange(n) % K
    else:
        j, last = [], -1
        while len(j) < n:
            v = int(rng.integers(K - 1))
            v += v >= last                                            # never the voxel of the run before
            j += [v] * int(rng.integers(1, run + 1))
            last = v
        j = np.array(j[:n])
    xy = _points(ix_of_slot(slot, iy, j), iy, leaf, rng)
    assert set(voxels(xy, leaf)[2].tolist()) == {slot}
    lanes, changes = contention(xy, leaf)
    assert np.all(lanes[:n // STEP] == STEP) and (n < STEP or changes.max() >= 20)
    return xy


def one_wave(n, r=3, leaf=0.1, seed=2):
    """The 64 slots whose low three bits are r, three voxels each, drawn at random: one wave of the eight-wave kernel gets
    every point, and its peer mask has to tell slots apart by bits 3-8 alone.  Certificate: slot & 7 constant, >= 32 slots."""
    rng = np.random.default_rng([seed, n])
    h = 8 * rng.integers(0, 64, n) + r
    iy = rng.integers(-2, 3, n)
    xy = _points(ix_of_slot(h, iy, rng.integers(0, 3, n)), iy, leaf, rng)
    got = voxels(xy, leaf)[2]
    assert np.all(got & 7 == r) and (n < STEP or len(np.unique(got)) >= 32)
    return xy


def eight_slots(n, leaf=0.5, seed=3):
    """Slots 0..7, three voxels each, drawn at random: every wave of the eight-wave kernel owns exactly one slot."""
    rng = np.random.default_rng([seed, n])
    h = rng.integers(0, 8, n)
    xy = _points(ix_of_slot(h, 0, rng.integers(0, 3, n)), 0, leaf, rng)
    got = voxels(xy, leaf)[2]
    assert np.all(got < 8) and (n < STEP or len(np.unique(got)) == 8)
    return xy


def no_flush(n, V=512, leaf=0.05, seed=4):
    """V <= 512 voxels in pairwise distinct slots, their points in random order: the whole output is the slot-order tail.
    Certificate: no flush, and as many output points as voxels.  V == 1: one float32 sum over the whole cloud."""
    rng = np.random.default_rng([seed, n, V])
    slots = rng.permutation(SLOTS)[:V]
    vy = rng.integers(-3, 4, V)
    vx = ix_of_slot(slots, vy, rng.integers(-2, 3, V))
    pick = rng.integers(0, V, n)
    xy = _points(vx[pick], vy[pick], leaf, rng)
    out, causes, _ = replay(xy, leaf)
    assert not causes and len(out) == len(np.unique(pick))
    return xy


def tile_edge_indices(n):
    """The indices tile_edges makes flush: first and last point of a tile, and both sides of a bitmap word (32), a step (64)
    and a read-ahead block (512), in every tile."""
    local = (0, 31, 32, 63, 64, 511, 512, TILE - 1)
    return [t + i for t in range(0, n, TILE) for i in local if 4 <= t + i < n]


def tile_edges(n, leaf=0.1, seed=5):
    """Point i lies in slot i % 4; a slot keeps its voxel until one of tile_edge_indices falls to it.  The voxels of slots 1
    and 2 run through every tile edge, those of slots 0 and 3 start on either side of one.  Certificate: the model's
    flush-causing indices are exactly tile_edge_indices(n)."""
    rng = np.random.default_rng([seed, n])
    j = np.zeros(n, np.int64)
    for s in tile_edge_indices(n):
        j[s::4] += 1                                                  # from s on, slot s % 4 holds its next voxel
    h = np.arange(n) % 4
    xy = _points(ix_of_slot(h, -1, j % 3), -1, leaf, rng)
    assert replay(xy, leaf)[1] == tile_edge_indices(n)
    return xy


def count_limit(tail, leaf=0.05, seed=6):
    """The largest counts the 16-bit parked count has to carry.  tail False: 65534 points of one voxel, then one point of a
    voxel in the same slot (a parked count of 65534); tail True: 65535 points of one voxel (a tail count of 65535)."""
    rng = np.random.default_rng([seed, int(tail)])
    j = np.zeros(SORT_MAX, np.int64)
    if not tail:
        j[-1] = 1
    xy = _points(ix_of_slot(100, 1, j), 1, leaf, rng)
    out, causes, _ = replay(xy, leaf)
    assert (causes, len(out)) == (([], 1) if tail else ([SORT_MAX - 1], 2))
    return xy


# name -> (generator of a cloud of n points, leaf)
FAMILIES = {
    "one_slot_round_robin": (lambda n: one_slot(n, K=5, run=1), 0.05),
    "one_slot_runs": (lambda n: one_slot(n, K=4, run=3), 0.05),
    "one_wave": (one_wave, 0.1),
    "eight_slots": (eight_slots, 0.5),
    "no_flush": (no_flush, 0.05),
    "tile_edges": (tile_edges, 0.1),
}
SORTED_LENGTHS = (64, 65, 8192, 8193, 16385, 65535)
EIGHT_WAVE_LENGTHS = (65536, 66113)
LONG_LENGTHS = (BITMAP_MAX, BITMAP_MAX + 1)          # the last length of the bitmap path, the first of the single wave
LONG_FAMILIES = ("one_slot_round_robin", "one_wave")


# ---------------------------------------------------------------------------------------------------------------------
# the batch whose workgroups each filter a second scan
# ---------------------------------------------------------------------------------------------------------------------
SECOND_ROUND_LEAF = 0.05
SECOND_ROUND_LONG = 66113


def second_round_batch(G, seed=7):
    """G + 100 scans of 0..130 points for G workgroups.  Scan b + G (b < 100) visits the slots scan b visits, in other
    voxels; every tenth of them is empty, every tenth has one point.  Scans 5 and 5 + G are long (one_slot, then one_wave
    over the wave that one_slot's slot belongs to): the second round of the step-by-step kernel."""
    rng = np.random.default_rng([seed, G])
    leaf = SECOND_ROUND_LEAF

    def tiny(m, hs, j0):
        h = hs[rng.integers(0, len(hs), m)]
        return _points(ix_of_slot(h, 0, j0 + rng.integers(0, 3, m)), 0, leaf, rng), h

    scans = [None] * (G + 100)
    for b in range(G):
        hs = rng.integers(0, SLOTS, 6)
        scans[b], h = tiny(0 if b >= 100 and b % 37 == 3 else int(rng.integers(1, 131)), hs, 0)
        if b < 100:
            m = 0 if b % 10 == 0 else 1 if b % 10 == 1 else int(rng.integers(1, 131))
            h2 = np.resize(h if len(h) else hs, m)
            scans[b + G] = _points(ix_of_slot(h2, 0, 3 + rng.integers(0, 3, m)), 0, leaf, rng)
    scans[5] = one_slot(SECOND_ROUND_LONG, K=5, run=1, slot=43, leaf=leaf)
    scans[5 + G] = one_wave(SECOND_ROUND_LONG, r=43 & 7, leaf=leaf)
    assert all(len(s) <= 130 for b, s in enumerate(scans) if b % G != 5)
    return scans


def uniform_cloud(rng, n):
    """The second cloud shape of tests/test_gpu_prefilter.py."""
    return rng.uniform(-40, 40, (n, 2)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# python tests/prefilter_workloads.py: the two tables of LOG.md (a record, not a test; about half a minute)
# ---------------------------------------------------------------------------------------------------------------------
def _older_inputs():
    """(name, cloud, leaf) of every cloud tests/test_gpu_prefilter.py filters, from its own generators and seeds."""
    from test_gpu_prefilter import lidar_like
    for leaf in (0.05, 0.1, 0.5):
        rng = np.random.default_rng(7)
        for n in (1, 2, 63, 64, 65, 360, 5000, 8192, 8193, 20000, 50000, 65535, 65536):
            yield "lidar_like", lidar_like(rng, n), leaf
            yield "uniform", uniform_cloud(rng, n), leaf
    yield "lidar_like", lidar_like(np.random.default_rng(17), 300_000, radius=60.0), 0.05
    rng = np.random.default_rng(23)
    for n in (100, 65535, 70000, 30000, 1, 65536, 8192):
        yield "lidar_like (batch)", lidar_like(rng, n), 0.05
    k = next(k for k in range(1, 4000) if (k * 7171) % 512 == 0)
    yield "two voxels alternating", np.array([[0.05 + 0.1 * k * (i % 2), 0.05] for i in range(257)], F32), 0.1


def _tables():
    def row(name, cloud, leaf):
        lanes, changes = contention(cloud, leaf)
        print("| %s | %d | %g | %d | %d |" % (name, len(cloud), leaf, lanes.max(), changes.max()))

    print("| input | points | leaf | lanes in one slot in a step | voxel changes in one slot in a step |\n|---|---|---|---|---|")
    for name, cloud, leaf in _older_inputs():
        if len(cloud) >= 5000 or name.startswith("two"):
            row(name, cloud, leaf)
    for name, (make, leaf) in FAMILIES.items():
        for n in (65535, 66113) + (LONG_LENGTHS if name in LONG_FAMILIES else ()):
            row(name, make(n), leaf)
    row("no_flush, one voxel", no_flush(20000, V=1), 0.05)
    row("count_limit, parked", count_limit(False), 0.05)
    told = {}
    for name, cloud, leaf in _older_inputs():
        good = model(cloud, leaf).tobytes()
        for d in "abcdf":
            if d in "cdf" and len(cloud) > SORT_MAX:                  # switches of the by-slot kernel: its scans only
                continue
            if model(cloud, leaf, d).tobytes() != good:
                told.setdefault((d, name), []).append("%d @ %g" % (len(cloud), leaf))
    print("\n| switch | older input | told apart at (points @ leaf) |\n|---|---|---|")
    for d in "abcdf":
        for name in ("lidar_like", "uniform", "lidar_like (batch)", "two voxels alternating"):
            print("| %s | %s | %s |" % (d, name, ", ".join(told.get((d, name), [])) or "never"))
    print("| e | every older input | never: no batch has more scans than workgroups |")


if __name__ == "__main__":
    _tables()
