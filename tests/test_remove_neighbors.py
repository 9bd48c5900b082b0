"""Row f3 (part): PCFilter::remove_neighborPoint (include/ndt_slam/PCFilter.h:29-56) -- oracle against a
numpy evaluation of the same rule (CPU) and the device version against the oracle (GPU, exact)."""
import numpy as np
import pytest


def clouds(rng, nb, nl):
    base = rng.uniform(-20, 20, (nb, 2)).astype(np.float32)
    lst = base[rng.choice(nb, nl, replace=nl > nb)] + rng.normal(0, 0.08, (nl, 2)).astype(np.float32) if nl else np.zeros((0, 2), np.float32)
    return base, lst.astype(np.float32)


def test_oracle_follows_the_all_pairs_rule(oracle):
    rng = np.random.default_rng(4)
    base, lst = clouds(rng, 700, 90)
    d = np.sqrt(((base[:, None, :] - lst[None, :, :]) ** 2).sum(-1, dtype=np.float32), dtype=np.float32)
    keep = ~(d.astype(np.float64) < 0.1).any(1)
    out = oracle.remove_neighbors(base, lst, 0.1)
    assert out.tobytes() == base[keep].tobytes() and 0 < len(out) < len(base)
    assert oracle.remove_neighbors(base, np.zeros((0, 2), np.float32), 0.1).tobytes() == base.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("nb,nl", [(1, 1), (255, 3), (256, 0), (257, 1025), (10000, 700), (40000, 5000)])
def test_device_version_is_exact(oracle, nb, nl):
    import torch
    assert torch.cuda.is_available()
    from ndt_slam_amd import capi
    ctx = capi.Context(0)
    rng = np.random.default_rng(nb + nl)
    base, lst = clouds(rng, nb, nl)
    if nl:       # a pair exactly at the threshold distance and one just inside it
        base[0] = (1.0, 1.0); lst[0] = (1.0, np.float32(1.1)); base[-1] = lst[-1] + np.float32(0.0999)
    got, ref = ctx.remove_neighbors(base, lst, 0.1), oracle.remove_neighbors(base, lst, 0.1)
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("bs,ls", [(16, 24), (24, 16), (8, 8)])
def test_device_form_with_its_own_strides(oracle, bs, ls):
    """ndt_remove_neighbors_dev with base and list at strides of their own: 513 base points (two full 256-point units
    and a unit of one), 1025 list points (one full LDS tile and a tile of one), the threshold pair in the first unit
    and the just-inside pair in the last.  Equal to the oracle and to the host form; nothing behind the count is
    written; with no list (NULL) every point is kept."""
    import torch
    assert torch.cuda.is_available()
    from ndt_slam_amd import capi
    ctx = capi.Context(0)
    canary = np.float32(-4242.0)
    rng = np.random.default_rng(bs + ls)
    base, lst = clouds(rng, 513, 1025)
    base[0] = (1.0, 1.0); lst[0] = (1.0, np.float32(1.1)); base[-1] = lst[-1] + np.float32(0.0999)
    ref = oracle.remove_neighbors(base, lst, 0.1)
    assert ctx.remove_neighbors(base, lst, 0.1).tobytes() == ref.tobytes() and 0 < len(ref) < len(base)

    def strided(p, stride):
        host = np.full((len(p), stride // 4), canary)
        host[:, :2] = p
        return torch.from_numpy(host).cuda()
    d_base, d_list = strided(base, bs), strided(lst, ls)
    for n_list, want in ((len(lst), ref), (0, base)):
        out = torch.full((len(base) + 1, 2), float(canary), dtype=torch.float32, device="cuda")
        cnt = torch.full((1,), 0x5a5a5a5a5a5a, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.check(capi.lib().ndt_remove_neighbors_dev(ctx.h, d_base.data_ptr(), bs, len(base), d_list.data_ptr() if n_list else None,
                                                      ls, n_list, 0.1, out.data_ptr(), cnt.data_ptr(), None),
                  "ndt_remove_neighbors_dev")
        torch.cuda.synchronize()
        n, got = int(cnt.item()), out.cpu().numpy()
        assert n == len(want) and got[:n].tobytes() == want.tobytes() and (got[n:] == canary).all()
