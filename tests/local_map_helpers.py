"""The oracle standing in for a context that provides the batched local-map assembly (tests only)."""
import numpy as np

from ndt_slam_amd.capi import pack_scans

_EMPTY = np.zeros((0, 2), np.float32)


def oracle_local_map(oracle, item, leaf):
    """One item of Context.local_maps on the oracle -> (p_cloud, target, n_prev)."""
    scans, first, newest, remove, resol, thre, prev = item
    p_cloud = np.ascontiguousarray(oracle.make_map(scans, first, newest, remove, resol, thre), np.float32).reshape(-1, 2)
    filt = oracle.approx_voxel_filter(p_cloud, leaf).reshape(-1, 2) if len(p_cloud) else _EMPTY
    prev = _EMPTY if prev is None else np.ascontiguousarray(prev, np.float32).reshape(-1, 2)
    return p_cloud, np.concatenate([prev, filt]), len(prev)


class OracleBatchOps:
    """local_maps with the oracle, one item at a time, with the size of every call kept; the per-session operations
    raise: a lockstep replay on the batched path must not reach them."""

    def __init__(self, oracle):
        self.o = oracle
        self.calls = []                 # number of items of every local_maps call
        self.leaves = []

    def local_maps(self, items, leaf):
        items = list(items)
        self.calls.append(len(items))
        self.leaves.append(leaf)
        return [oracle_local_map(self.o, it, leaf) for it in items]

    def prefilter(self, xy, leaf):
        raise AssertionError("prefilter called on the batched path")

    def make_map(self, *a):
        raise AssertionError("make_map called on the batched path")


class CountingOps:
    """A wrapper around a context that counts local_maps / make_map / prefilter calls and passes everything on."""

    def __init__(self, ctx):
        self._ctx = ctx
        self.local_maps_calls, self.make_map_calls, self.prefilter_calls = [], 0, 0

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def local_maps(self, items, leaf):
        items = list(items)
        self.local_maps_calls.append(len(items))
        return self._ctx.local_maps(items, leaf)

    def make_map(self, *a, **k):
        self.make_map_calls += 1
        return self._ctx.make_map(*a, **k)

    def prefilter(self, *a, **k):
        self.prefilter_calls += 1
        return self._ctx.prefilter(*a, **k)


# ---- ndt_local_map_batch{,_dev} through the raw C ABI (GPU tests) ----

def room_scans(rng, n_scans, n_wall, n_mover, jitter=0.003):
    """Scans of one submap in the map frame: static walls re-observed with noise + an object that moves (the scenes of
    tests/test_gpu_local_map.py)."""
    th = np.linspace(0, 2 * np.pi, n_wall, endpoint=False)
    room = np.stack([8 * np.cos(th) / np.maximum(abs(np.cos(th)), abs(np.sin(th))),
                     6 * np.sin(th) / np.maximum(abs(np.cos(th)), abs(np.sin(th)))], 1)
    scans = []
    for k in range(n_scans):
        m = int(n_mover * (0.5 + rng.random()))
        mover = np.stack([rng.normal(-3 + 0.6 * k, 0.1, m), rng.normal(0.5, 0.15, m)], 1)
        keep = rng.random(n_wall) > 0.1
        scans.append((np.concatenate([room[keep], mover]) + rng.normal(size=(keep.sum() + m, 2)) * jitter)
                     .astype(np.float32))
    return scans


def item_arrays(item):
    """(all points [n, 2] float32, offsets uint64, previous cloud [m, 2] float32) of an item."""
    allp, off = pack_scans(item[0])
    prev = _EMPTY if item[6] is None else np.ascontiguousarray(item[6], np.float32).reshape(-1, 2)
    return allp, off, prev


def capacities(items):
    """The header's rule: (cloud capacity, target capacity) in points."""
    cloud = sum((2 if len(it[0]) == 1 else 1) * sum(len(x) for x in it[0]) for it in items)
    return cloud, cloud + sum(0 if it[6] is None else len(it[6]) for it in items)


def host_call(capi, ctx, items, leaf, want_target=True, offsets=False):
    """ndt_local_map_batch on host arrays -> (rc, clouds, targets or None, status); offsets: then (cloud_off, target_off) too."""
    S = len(items)
    descs = (capi.SubmapDesc * S)()
    keep = []
    for s, it in enumerate(items):
        allp, off, prev = item_arrays(it)
        if len(allp) == 0:
            allp = np.zeros((1, 2), np.float32)
        keep.append((allp, off, prev))
        descs[s] = capi.SubmapDesc(allp.ctypes.data, off.ctypes.data, len(it[0]), int(it[1]), int(it[2]), int(it[3]),
                                   float(it[4]), float(it[5]), prev.ctypes.data if len(prev) else None, len(prev))
    cc, tc = capacities(items)
    cloud = np.full((cc + 1, 2), np.float32(-777.0))
    target = np.full((tc + 1, 2), np.float32(-777.0))
    coff, toff = np.zeros(S + 1, np.uint64), np.zeros(S + 1, np.uint64)
    status = np.full(S, 99, np.int32)
    rc = capi.lib().ndt_local_map_batch(ctx.h, descs, S, 8, leaf, cloud.ctypes.data, coff.ctypes.data,
                                        target.ctypes.data if want_target else None,
                                        toff.ctypes.data if want_target else None, status.ctypes.data)
    if rc:
        return rc, None, None, status
    assert np.all(cloud[int(coff[S]):] == np.float32(-777.0)) and int(coff[S]) <= cc
    clouds = [cloud[int(coff[s]):int(coff[s + 1])].copy() for s in range(S)]
    targets = None
    if want_target:
        assert np.all(target[int(toff[S]):] == np.float32(-777.0)) and int(toff[S]) <= tc
        targets = [target[int(toff[s]):int(toff[s + 1])].copy() for s in range(S)]
    if offsets:
        return rc, clouds, targets, status, (coff, toff)
    return rc, clouds, targets, status


class DevCall:
    """ndt_local_map_batch_dev with torch tensors: the items uploaded, the outputs allocated by the header's rule."""

    def __init__(self, capi, items, want_target=True, stride=8):
        import torch
        self.capi, self.items, self.S, self.want_target = capi, items, len(items), want_target
        dev = torch.device("cuda", 0)
        self.keep, descs = [], []
        for it in items:
            allp, off, prev = item_arrays(it)
            if stride == 16:                                   # pcl::PointXYZ: x y z pad
                allp = np.concatenate([allp, np.zeros_like(allp)], axis=1)
                prev = np.concatenate([prev, np.zeros_like(prev)], axis=1)
            d_all = torch.from_numpy(allp if len(allp) else np.zeros((1, stride // 4), np.float32)).to(dev)
            d_prev = torch.from_numpy(prev).to(dev) if len(prev) else None
            self.keep.append((d_all, off, d_prev))
            descs.append(capi.SubmapDesc(d_all.data_ptr(), off.ctypes.data, len(it[0]), int(it[1]), int(it[2]), int(it[3]),
                                         float(it[4]), float(it[5]), d_prev.data_ptr() if d_prev is not None else None,
                                         len(prev)))
        self.descs = descs
        self.stride = stride
        cc, tc = capacities(items)
        self.cloud = torch.full((cc + 1, 2), -777.0, dtype=torch.float32, device=dev)
        self.target = torch.full((tc + 1, 2), -777.0, dtype=torch.float32, device=dev)
        self.coff = torch.zeros(self.S + 1, dtype=torch.int64, device=dev)
        self.toff = torch.zeros(self.S + 1, dtype=torch.int64, device=dev)
        self.status = torch.full((self.S,), 99, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

    def run(self, ctx, leaf, stream=None):
        t = self.want_target
        ctx.local_maps_dev(self.descs, leaf, self.cloud.data_ptr(), self.coff.data_ptr(),
                           self.target.data_ptr() if t else None, self.toff.data_ptr() if t else None,
                           self.status.data_ptr(), stride=self.stride, stream=stream)

    def results(self):
        """(clouds, targets or None, status) on the host (after the caller has synchronised the stream)."""
        coff, toff = self.coff.cpu().numpy(), self.toff.cpu().numpy()
        cloud, target = self.cloud.cpu().numpy(), self.target.cpu().numpy()
        S = self.S
        assert np.all(cloud[int(coff[S]):] == np.float32(-777.0))
        clouds = [cloud[int(coff[s]):int(coff[s + 1])].copy() for s in range(S)]
        if not self.want_target:
            assert np.all(target == np.float32(-777.0)) and not toff.any()
            return clouds, None, self.status.cpu().numpy()
        assert np.all(target[int(toff[S]):] == np.float32(-777.0))
        return clouds, [target[int(toff[s]):int(toff[s + 1])].copy() for s in range(S)], self.status.cpu().numpy()
