"""What the GPU test modules share: the module-scoped context fixture and the torch plumbing around device buffers."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def gpu():
    """(capi, a Context on device 0).  A module imports this fixture by name and so gets a context of its own."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    from ndt_slam_amd import capi
    return capi, capi.Context(0)


def to_dev(a):
    """A numpy array as a contiguous torch tensor on device 0 (a read-only array is copied first: torch wants it writeable)."""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(torch.device("cuda", 0))


def sync():
    import torch
    torch.cuda.synchronize()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
