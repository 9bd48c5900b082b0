"""SURVEY.md 8f row f3 on the device, on the path-aimed clouds of tests/local_map_workloads.py: every difference case
and every assembly case against the oracle's pointer octree (which tests/test_local_map_workloads_host.py holds to the
independent replay on the same cases), through the host forms, the device forms and the batch.  No tolerance: every
comparison is of bytes, counts or status words.  Which path a case takes is proven by the census on the CPU."""
import numpy as np
import pytest

import local_map_workloads as W
from gpu_support import gpu  # noqa: F401
from local_map_helpers import DevCall as BatchDevCall, host_call, oracle_local_map

pytestmark = pytest.mark.gpu
CANARY = np.float32(-4242.0)
WORD = 0x5a5a5a5a5a5a            # what a count word holds before a call
EMPTY = np.zeros((0, 2), np.float32)


def grid_id(p):
    return "%s-%g-%s" % (p[0], p[1], "o0" if p[2][0] == 0 else "o1")


DIFF_PARAMS = [(f, r, o) for f in W.DIFF_FAMILIES for r, o in W.family_grid(f)]
ASM_PARAMS = [(f, r, o) for f in ("long_submap", "list_tiles", "unit_tails") for r, o in W.GRID]


def expect_difference(oracle, c):
    return c["test"][np.sort(oracle.difference_indices(c["base"], c["test"], c["resol"]))]


class DevDiff:
    """Device buffers of one ndt_difference_extraction_dev call at `stride` bytes per point: canaries between the points,
    behind the result and in the count word."""

    def __init__(self, capi, ctx, c, stride):
        import torch

        def up(points):
            host = np.full((max(len(points), 1), stride // 4), CANARY)
            host[:len(points), :2] = points
            return torch.from_numpy(host).cuda()
        base, test = up(c["base"]), up(c["test"])
        self.out = torch.full((len(c["test"]) + 1, 2), float(CANARY), dtype=torch.float32, device="cuda")
        self.cnt = torch.full((1,), WORD, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.check(capi.lib().ndt_difference_extraction_dev(ctx.h, base.data_ptr(), stride, len(c["base"]), test.data_ptr(), stride,
                                                           len(c["test"]), c["resol"], self.out.data_ptr(), self.cnt.data_ptr(), None),
                  "ndt_difference_extraction_dev")
        torch.cuda.synchronize()
        self.n, out = int(self.cnt.item()), self.out.cpu().numpy()             # UINT64_MAX reads -1
        assert (out[max(self.n, 0):] == CANARY).all()
        self.points = out[:max(self.n, 0)]


@pytest.mark.parametrize("family,resol,origin", DIFF_PARAMS, ids=[grid_id(p) for p in DIFF_PARAMS])
def test_difference_extraction_on_every_case(gpu, oracle, family, resol, origin):
    capi, ctx = gpu
    cases = W.DIFF_FAMILIES[family](resol, origin)
    accepted = [c for c in cases if not c["refused"]]
    for c in accepted:
        ref = expect_difference(oracle, c)
        got = ctx.difference_extraction(c["base"], c["test"], c["resol"])
        assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), c["name"]
    # one case of the family through the device form at the stride of pcl::PointXYZ
    c = accepted[0]
    d = DevDiff(capi, ctx, c, 16)
    ref = expect_difference(oracle, c)
    assert d.n == len(ref) and d.points.tobytes() == ref.tobytes()
    # the refused ones: the host form raises, the device form writes UINT64_MAX and nothing else, the next call is exact
    for c, nxt in zip([c for c in cases if c["refused"]], accepted):
        with pytest.raises(RuntimeError):
            ctx.difference_extraction(c["base"], c["test"], c["resol"])
        d = DevDiff(capi, ctx, c, 8)
        assert d.n == -1 and len(d.points) == 0
        assert ctx.difference_extraction(nxt["base"], nxt["test"], nxt["resol"]).tobytes() == expect_difference(oracle, nxt).tobytes()


def ordinary_item(resol, origin):
    scans = W.unit_tails(resol, origin)[0]["items"][0][0]
    return ([x[:120] for x in scans[:4]], True, True, True, resol, 2.0 * resol, None)


@pytest.mark.parametrize("family,resol,origin", ASM_PARAMS, ids=[grid_id(p) for p in ASM_PARAMS])
def test_make_map_on_every_single_submap_case(gpu, oracle, family, resol, origin):
    capi, ctx = gpu
    for c in W.ASM_FAMILIES[family](resol, origin):
        (it,) = c["items"]
        ref = oracle.make_map(*it[:6])
        got = ctx.make_map(*it[:6])
        assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), c["name"]
        assert 0 < len(ref) and (not it[3] or len(ref) < sum(len(x) for x in it[0]))
        if family == "list_tiles":            # the all-pairs step alone, on the case's own list
            scans = it[0]
            lst = oracle.difference_extraction(np.concatenate([scans[0], scans[2]]), scans[1], resol)
            assert len(lst) == c["n_list"]
            got, ref = ctx.remove_neighbors(scans[1], lst, it[5]), oracle.remove_neighbors(scans[1], lst, it[5])
            assert got.tobytes() == ref.tobytes() and len(ref) == len(scans[1]) - c["n_list"] - (c["n_cand"] + 2) // 3
        if family == "long_submap":           # one item of a batch, between two ordinary ones
            items = [ordinary_item(resol, origin), it, ordinary_item(resol, origin)]
            want = [oracle_local_map(oracle, x, resol) for x in items]
            rc, clouds, targets, status = host_call(capi, ctx, items, resol)
            assert rc == 0 and not status.any()
            for s in range(3):
                assert clouds[s].tobytes() == want[s][0].tobytes() and targets[s].tobytes() == want[s][1].tobytes(), (c["name"], s)


def batch_twins(oracle, items, leaf):
    """Per item (cloud, target) as the batch must give them; a refused submap is empty in both."""
    out = []
    for it in items:
        try:
            p_cloud, target, _ = oracle_local_map(oracle, it, leaf)
            out.append((p_cloud, target))
        except ValueError:
            out.append(None)
    return out


def assert_batch(capi, clouds, targets, status, coff, toff, want, what):
    bad = [s for s, w in enumerate(want) if w is None]
    assert [s for s in range(len(want)) if status[s] == capi.NDT_E_ARG] == bad and not np.delete(status, bad).any(), what
    lens_c = [0 if w is None else len(w[0]) for w in want]
    lens_t = [0 if w is None else len(w[1]) for w in want]
    assert np.array_equal(np.asarray(coff, np.int64), np.concatenate([[0], np.cumsum(lens_c)])), what
    assert np.array_equal(np.asarray(toff, np.int64), np.concatenate([[0], np.cumsum(lens_t)])), what
    for s, w in enumerate(want):
        c, t = (EMPTY, EMPTY) if w is None else w
        assert clouds[s].tobytes() == c.tobytes() and targets[s].tobytes() == t.tobytes(), (what, s)


MANY_PARAMS = [(r, o, k) for r, o in W.GRID for k in (0, 1)]


@pytest.mark.parametrize("resol,origin,k", MANY_PARAMS, ids=["%g-%s-%d" % (r, "o0" if o[0] == 0 else "o1", (1025, 2050)[k])
                                                             for r, o, k in MANY_PARAMS])
def test_many_submaps_in_one_call(gpu, oracle, resol, origin, k):
    import torch
    capi, ctx = gpu
    c = W.many_submaps(resol, origin)[k]
    items, leaf = c["items"], resol
    want = batch_twins(oracle, items, leaf)
    assert [s for s, w in enumerate(want) if w is None] == c["refused"]
    for it, w in zip(items, want):                       # every submap on its own
        if w is None:
            with pytest.raises(capi.NdtError):
                ctx.make_map(*it[:6])
        else:
            assert ctx.make_map(*it[:6]).tobytes() == w[0].tobytes()
    rc, clouds, targets, status, (coff, toff) = host_call(capi, ctx, items, leaf, offsets=True)      # (checks behind the totals)
    assert rc == 0
    assert_batch(capi, clouds, targets, status, coff, toff, want, "host form")
    d = BatchDevCall(capi, items, stride=(8, 16)[k])
    d.run(ctx, leaf)
    torch.cuda.ExternalStream(ctx.stream).synchronize()
    clouds, targets, status = d.results()                                                          # (checks behind the totals)
    assert_batch(capi, clouds, targets, status, d.coff.cpu().numpy(), d.toff.cpu().numpy(), want, "device form")
    rc, clouds, targets, status, (coff, toff) = host_call(capi, ctx, items[::-1], leaf, offsets=True)
    assert rc == 0
    assert_batch(capi, clouds, targets, status, coff, toff, want[::-1], "reversed")
