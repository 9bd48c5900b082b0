"""The scan archive and ndt_sessions_occ_rebuild without a GPU: the symbols and their prototypes, the refusals that need no
device, replay.loop_graph against a graph made by hand, and the replay driver's refusal of a stand-in that cannot search."""
import ctypes as C

import numpy as np
import pytest

from ndt_slam_amd import replay

NEW = ("ndt_sessions_archive_enable", "ndt_sessions_archive_info", "ndt_sessions_archive_scans", "ndt_sessions_archive_view",
       "ndt_sessions_occ_rebuild")


@pytest.fixture(scope="module")
def capi():
    from ndt_slam_amd import build, capi
    build.build()
    return capi


def test_the_new_symbols_are_exported_and_prototyped(capi):
    L = capi.lib()
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    want = {"ndt_sessions_archive_enable": [vp],
            "ndt_sessions_archive_info": [vp, i, C.POINTER(sz), C.POINTER(sz)],
            "ndt_sessions_archive_scans": [vp, i, sz, sz, vp, sz, vp, C.POINTER(sz)],
            "ndt_sessions_archive_view": [vp, i, C.POINTER(vp), C.POINTER(sz)],
            "ndt_sessions_occ_rebuild": [vp, vp, vp, i, C.c_double, vp]}
    assert tuple(want) == NEW
    for name in NEW:
        assert name in capi.EXPORTS and capi.PROTOTYPES[name] == want[name]
        fn = getattr(L, name)
        assert fn.argtypes == want[name] and fn.restype is C.c_int
    for method in ("archive_info", "archive_scans", "archive_view", "occ_rebuild"):
        assert callable(getattr(capi.Sessions, method))


def test_a_null_set_is_refused_by_every_new_call(capi):
    L = capi.lib()
    n, m, p = C.c_size_t(7), C.c_size_t(7), C.c_void_p(7)
    st, off = np.full(4, 9, np.uint64), np.full(3, 9, np.uint64)
    grids = (C.c_void_p * 1)(None)
    for rc in (L.ndt_sessions_archive_enable(None),
               L.ndt_sessions_archive_info(None, 0, C.byref(n), C.byref(m)),
               L.ndt_sessions_archive_scans(None, 0, 0, 1, None, 0, off.ctypes.data, C.byref(n)),
               L.ndt_sessions_archive_view(None, 0, C.byref(p), C.byref(n)),
               L.ndt_sessions_occ_rebuild(None, grids, None, 1, 1.0, st.ctypes.data)):
        assert rc == capi.NDT_E_ARG and L.ndt_last_error(None).decode() == "null session set"
    assert (n.value, m.value, p.value) == (7, 7, 7) and (st == 9).all() and (off == 9).all()


def test_loop_graph_is_the_graph_made_by_hand(capi):
    poses = np.array([[0.25, -1.0, 0.0], [1.25, -0.5, 0.0], [1.75, 1.0, 90.0]])      # (headings whose cos / sin are exact)
    info = np.array([100.0, 1.0, 2.0, 90.0, 3.0, 400.0])
    loop = np.zeros(1, dtype=capi.LOOP_DTYPE)[0]
    loop["edge"]["from_"], loop["edge"]["to"] = 0, 2
    loop["edge"]["rel"], loop["edge"]["info"] = (1.4, 2.1, 89.0), (50.0, 0.0, 0.0, 50.0, 0.0, 200.0)
    got = replay.loop_graph(poses, loop["edge"], info)
    # Pose2D::calMotion(to, from): the displacement in the frame of `from`, the heading's difference
    want = np.zeros(3, dtype=capi.PG_EDGE_DTYPE)
    want[0] = (0, 1, (1.0, 0.5, 0.0), info)
    want[1] = (1, 2, (0.5, 1.5, 90.0), info)
    want[2] = (0, 2, (1.4, 2.1, 89.0), (50.0, 0.0, 0.0, 50.0, 0.0, 200.0))
    assert got.dtype == capi.PG_EDGE_DTYPE and got.tobytes() == want.tobytes(), (got, want)
    # an arc given as a PG_EDGE_DTYPE record (field `from`) is taken as well; a single pose has the loop's arc alone
    assert replay.loop_graph(poses, want[2], info).tobytes() == got.tobytes()
    assert len(replay.loop_graph(poses[:1], want[2], info)) == 1


def test_the_driver_refuses_loop_closure_on_a_stand_in_that_cannot_search(capi):
    class StandIn:
        def step(self, *a):
            raise AssertionError("refused before the first step")

    lp = capi.default_loop_params()
    lc = replay.LoopClosure(loop=lp, pg=None, odo_info=np.array(lp.info[:]) / 100.0, every=1, cooldown=5)
    log = [replay.Scan2D(np.zeros((3, 2)), 0)]
    with pytest.raises(ValueError, match="find_loops"):
        replay.run_sessions_resident(None, [log], sessions=StandIn(), loop_closure=lc)
    assert lc._fields == ("loop", "pg", "odo_info", "every", "cooldown")
