"""The older entry-point families across two streams: pre-filter, resampler, neighbour removal, difference extraction and
local-map assembly, whose device forms run on a second stream while their host forms -- and ndt_eval_at / ndt_fitness_at
against a map that another context owns and rebuilds -- run on the context's own.  All of them share the context's
scratch, so every call has to be ordered behind the one before it by the call frame, and the two map readers behind the
map's build.

A reference pass runs each call alone with a device synchronise behind it.  A chained pass then issues the same sequence
five times with nothing between the calls, alternating the two streams, and must reproduce every output byte for byte.

The test is one-sided: a difference proves an ordering break, equality proves nothing about the order (two calls that
overlap may still happen to give the right bytes).  It provokes nothing: every call is a valid one."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEAF, SPACE, SPACE_THRE, RESOL, THRE = 0.05, 0.05, 0.25, 0.05, 0.2
ROUNDS = 5


class Outputs:
    """The device outputs of one round of device-form calls."""

    def __init__(self, torch, dev, B, n_raw, cap_rs, n_cloud, n_test):
        z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
        self.rs64, self.rs32 = z(2 * cap_rs, torch.float64), z(2 * cap_rs, torch.float32)
        self.rs_off, self.rs_status = z(B + 1, torch.int64), z(B, torch.int32)
        self.pf, self.pf_off = z(2 * n_raw, torch.float32), z(B + 1, torch.int64)
        self.rn, self.rn_n = z(2 * n_cloud, torch.float32), z(1, torch.int64)
        self.de, self.de_n = z(2 * n_test + 2, torch.float32), z(1, torch.int64)
        self.mm, self.mm_n = z(2 * n_raw + 2, torch.float32), z(1, torch.int64)

    def snapshot(self):
        """Every output's defined part as bytes (after a synchronise)."""
        h = lambda t: t.cpu().numpy()
        rs_off, pf_off = h(self.rs_off), h(self.pf_off)
        rn_n, de_n, mm_n = int(h(self.rn_n)[0]), int(h(self.de_n)[0]), int(h(self.mm_n)[0])
        parts = [rs_off, h(self.rs_status), h(self.rs64)[:2 * int(rs_off[-1])], h(self.rs32)[:2 * int(rs_off[-1])],
                 pf_off, h(self.pf)[:2 * int(pf_off[-1])], np.array([rn_n, de_n, mm_n]), h(self.rn)[:2 * rn_n],
                 h(self.de)[:2 * de_n], h(self.mm)[:2 * mm_n]]
        return [p.tobytes() for p in parts]


def test_older_families_chained_across_two_streams_match_their_runs_alone():
    import torch
    from ndt_slam_amd import capi, synth
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    dev = torch.device("cuda", 0)
    L = capi.lib()

    lens = [2000, 2571, 3143, 3714, 4286, 4857, 5429, 6000]
    B = len(lens)
    scans = [synth.submap_scans(B, n, seed=21)[k] for k, n in enumerate(lens)]       # one room, seen eight times
    raw32 = np.ascontiguousarray(np.concatenate(scans))
    raw64 = raw32.astype(np.float64)
    off = np.zeros(B + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    n_raw = int(off[-1])
    cloud = synth.submap_scans(1, 20_000, seed=5)[0]
    map_xy = synth.make_map(200_000, 24.0)
    probe = np.ascontiguousarray(map_xy[::50] + np.float32(0.03))                    # 4 000 points beside the map's walls
    pose = np.array([0.01, -0.02, 0.003])
    cap_rs = capi.resample_capacity(n_raw, SPACE, SPACE_THRE)

    ctx, ctx2 = capi.Context(0), capi.Context(0)
    s2 = torch.cuda.Stream(device=dev)
    d_raw32, d_raw64 = torch.from_numpy(raw32).to(dev), torch.from_numpy(raw64).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_cloud, d_map = torch.from_numpy(cloud).to(dev), torch.from_numpy(map_xy).to(dev)
    d_list = d_raw32[:lens[0]]                                                        # scan 0
    d_test = d_raw32[lens[0]:lens[0] + lens[1]]                                       # scan 1
    sets = [Outputs(torch, dev, B, n_raw, cap_rs, len(cloud), lens[1]) for _ in range(ROUNDS + 1)]
    torch.cuda.synchronize()
    gm2 = capi.Map(ctx2, params=capi.default_params(resolution=0.5), dev_ptr=d_map.data_ptr(), n=len(map_xy), stride=8)
    torch.cuda.synchronize()

    def eval_at():                                        # on ctx, against ctx2's map
        s, pr, g, H = C.c_double(), C.c_double(), np.zeros(3), np.zeros(9)
        ctx.check(L.ndt_eval_at(ctx.h, gm2.h, probe.ctypes.data, len(probe), 8, pose.ctypes.data, C.addressof(s), g.ctypes.data,
                                H.ctypes.data, C.addressof(pr)), "ndt_eval_at")
        return np.concatenate([[s.value, pr.value], g, H])

    def fitness_at():
        f = C.c_double()
        ctx.check(L.ndt_fitness_at(ctx.h, gm2.h, probe.ctypes.data, len(probe), 8, 1.0, 0.0, 0.01, -0.02, C.addressof(f)), "ndt_fitness_at")
        return np.array([f.value])

    def rebuild_then_eval():
        gm2.rebuild_begin(d_map.data_ptr(), len(map_xy))
        gm2.rebuild_end()
        return eval_at()

    def calls(D):
        """The sequence: (name, call); a device form (on s2) returns None, a host form (on ctx's stream) its result."""
        st = s2.cuda_stream
        return [
            ("resample_batch_dev", lambda: ctx.resample_batch_dev(d_raw64.data_ptr(), 16, d_off.data_ptr(), B, n_raw, SPACE, SPACE_THRE,
                                                                  D.rs64.data_ptr(), D.rs32.data_ptr(), D.rs_off.data_ptr(),
                                                                  D.rs_status.data_ptr(), stream=st)),
            ("prefilter_batch", lambda: np.concatenate(ctx.prefilter_batch(scans, LEAF))),
            ("prefilter_batch_dev", lambda: ctx.prefilter_batch_dev(d_raw32.data_ptr(), 8, d_off.data_ptr(), B, n_raw, LEAF, D.pf.data_ptr(),
                                                                    D.pf_off.data_ptr(), stream=st)),
            ("resample", lambda: ctx.resample(raw64[:lens[0]], SPACE, SPACE_THRE)),
            ("remove_neighbors_dev", lambda: ctx.check(L.ndt_remove_neighbors_dev(ctx.h, d_cloud.data_ptr(), 8, len(cloud), d_list.data_ptr(), 8,
                                                                                  lens[0], THRE, D.rn.data_ptr(), D.rn_n.data_ptr(), st),
                                                       "ndt_remove_neighbors_dev")),
            ("make_map", lambda: ctx.make_map(scans, True, True, True, RESOL, THRE)),
            ("difference_extraction_dev", lambda: ctx.check(L.ndt_difference_extraction_dev(ctx.h, d_cloud.data_ptr(), 8, len(cloud),
                                                                                            d_test.data_ptr(), 8, lens[1], RESOL, D.de.data_ptr(),
                                                                                            D.de_n.data_ptr(), st),
                                                            "ndt_difference_extraction_dev")),
            ("remove_neighbors", lambda: ctx.remove_neighbors(cloud, scans[0], THRE)),
            ("make_map_dev", lambda: ctx.make_map_dev(d_raw32.data_ptr(), 8, off, True, True, True, RESOL, THRE, D.mm.data_ptr(),
                                                      D.mm_n.data_ptr(), stream=st)),
            ("difference_extraction", lambda: ctx.difference_extraction(cloud, scans[1], RESOL)),
            ("rebuild + eval_at", rebuild_then_eval),
            ("prefilter", lambda: ctx.prefilter(scans[2], LEAF)),
            ("fitness_at", fitness_at),
        ]

    # reference pass: each call alone
    ref_host = {}
    for name, call in calls(sets[0]):
        r = call()
        torch.cuda.synchronize()
        if r is not None:
            ref_host[name] = np.asarray(r).tobytes()
    ref_dev = sets[0].snapshot()
    assert all(len(b) for b in ref_dev) and all(len(b) for b in ref_host.values()), "an output of the reference pass is empty"

    # chained pass: nothing between the calls
    for rnd in range(ROUNDS):
        for name, call in calls(sets[1 + rnd]):
            r = call()
            if r is not None:
                assert np.asarray(r).tobytes() == ref_host[name], "round %d: %s differs from its run alone" % (rnd, name)
    torch.cuda.synchronize()
    for rnd in range(ROUNDS):
        got = sets[1 + rnd].snapshot()
        for k, (a, b) in enumerate(zip(got, ref_dev)):
            assert a == b, "round %d: device output %d differs from its run alone" % (rnd, k)
    gm2.close(); ctx2.close(); ctx.close()
