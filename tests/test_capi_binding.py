"""The ctypes binding's own rules, without a GPU: every prototype of capi.PROTOTYPES held to its declaration in
include/ndt_mi355x.h, the ragged packer, the dtypes derived from Structures, the handle base and the error path."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_VALUE = {"int": C.c_int, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double, "uint32_t": C.c_uint32,
            "uint64_t": C.c_uint64, "long long": C.c_longlong}


@pytest.fixture(scope="module")
def capi():
    from ndt_slam_amd import build, capi
    build.build()
    return capi


def declarations():
    """[(return type, name, [parameter text])] of every function the header declares, in its order."""
    src = open(os.path.join(ROOT, "include", "ndt_mi355x.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r"^\s*#.*$", " ", src, flags=re.M)
    out = []
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(ndt_\w+)\s*\(([^;{}()]*)\)\s*;", src):
        params = [" ".join(a.split()) for a in args.split(",")]
        out.append((" ".join(ret.split()), name, [] if params in ([""], ["void"]) else params))
    return out


def is_pointer_type(t):
    return t in (C.c_void_p, C.c_char_p) or issubclass(t, (C._Pointer, C.Array))


def test_every_prototype_agrees_with_the_header(capi):
    decls = declarations()
    assert [d[1] for d in decls] == capi.EXPORTS == list(capi.PROTOTYPES)            # every function once, in the header's order
    assert len(decls) >= 92
    L = capi.lib()
    for ret, name, params in decls:
        fn = getattr(L, name)
        assert len(fn.argtypes) == len(params), (name, params)
        for t, p in zip(fn.argtypes, params):
            if "*" in p or "[" in p:
                assert is_pointer_type(t), (name, p, t)
                continue
            base = re.sub(r"\bconst\b", "", p).rsplit(None, 1)[0].strip()           # (the last word is the parameter's name)
            assert base in BY_VALUE, "%s: no rule for the by-value parameter %r" % (name, p)
            assert t is BY_VALUE[base], (name, p, t)
        want = {"const char *": C.c_char_p, "void *": C.c_void_p}.get(ret, C.c_int)
        assert ret in ("int", "const char *", "void *"), (name, ret)
        assert fn.restype is want, (name, ret, fn.restype)
    assert sorted(n for n in capi.PROTOTYPES if capi.RESTYPES.get(n, C.c_int) is not C.c_int) == ["ndt_ctx_stream", "ndt_last_error"]


def check_packed(capi, scans, **kw):
    pts, off = capi.pack_scans(scans, **kw)
    dtype, width = kw.get("dtype", np.float32), kw.get("width", 2)
    assert pts.dtype == dtype and off.dtype == kw.get("offsets_dtype", np.uint64)
    assert pts.shape == (sum(len(s) for s in scans), width) and pts.flags.c_contiguous
    if scans:
        assert np.array_equal(pts, np.concatenate([np.asarray(s).reshape(-1, width) for s in scans]).astype(dtype))
    assert off.tolist() == [sum(len(s) for s in scans[:i]) for i in range(len(scans) + 1)]
    return pts, off


def test_pack_scans(capi):
    rng = np.random.default_rng(3)
    pts, off = check_packed(capi, [])
    assert pts.shape == (0, 2) and off.tolist() == [0]
    empty = np.zeros((0, 2), np.float32)
    a, b = rng.normal(size=(5, 2)).astype(np.float32), rng.normal(size=(3, 2)).astype(np.float32)
    check_packed(capi, [empty, a, empty, b, empty])
    d = rng.normal(size=(4, 2))
    pts, _ = check_packed(capi, [d, np.zeros((0, 2)), d[:1]], dtype=np.float64)           # the Sessions.step case
    assert pts.tobytes() == np.concatenate([d, d[:1]]).tobytes()
    check_packed(capi, [a, b], offsets_dtype=np.int64)
    wide = rng.normal(size=(6, 4)).astype(np.float32)
    view = wide[::2, 1:3]                                                                  # neither row- nor column-contiguous
    assert not view.flags.c_contiguous
    check_packed(capi, [view, a])
    check_packed(capi, [wide], width=4)


def test_dtypes_derived_from_the_structures(capi):
    """The literals the module held before it derived them, with each field's offset as a number."""
    for dtype, struct, fields, size in (
            (capi.SESSION_STEP_DTYPE, capi.SessionStep,
             [("pose", "f8", 3, 0), ("cov", "f8", 9, 24), ("cost", "f8", None, 96), ("stepped", "i4", None, 104), ("matched", "i4", None, 108),
              ("successful", "i4", None, 112), ("status", "i4", None, 116), ("submap", "i4", None, 120), ("split", "i4", None, 124)], 128),
            (capi.FIT_STATS_DTYPE, capi.FitStats,
             [("fitness", "f8", None, 0), ("fitness_all", "f8", None, 8), ("n_in", "u4", None, 16), ("n_dist", "u4", None, 20),
              ("n_points", "u4", None, 24), ("reserved", "u4", None, 28)], 32),
            (capi.OCC_STATS_DTYPE, capi.OccStats,
             [("n_beams", "u8", None, 0), ("n_hit", "u8", None, 8), ("n_pass", "u8", None, 16), ("n_skipped", "u8", None, 24)], 32)):
        literal = np.dtype([(n, t) if k is None else (n, t, k) for n, t, k, _ in fields], align=True)
        assert dtype == literal and dtype.itemsize == literal.itemsize == size == C.sizeof(struct)
        assert dtype.isalignedstruct and dtype.names == literal.names
        for n, _, _, at in fields:
            assert dtype.fields[n][1] == literal.fields[n][1] == at == getattr(struct, n).offset, n
    # the one that stays hand-written: the C field `from` is from_ in the Structure
    assert np.dtype(capi.PgEdge) != capi.PG_EDGE_DTYPE and capi.PG_EDGE_DTYPE.itemsize == C.sizeof(capi.PgEdge)


def test_handle_destroys_once_and_never_what_it_gave_up(capi, monkeypatch):
    freed = []

    class Fake:
        @staticmethod
        def fake_destroy(h):
            freed.append(h.value)
            return 0
        ndt_map_destroy = fake_destroy

    class Thing(capi._Handle):
        _destroy = "fake_destroy"

        def __init__(self, value):
            self.h = C.c_void_p(value)

    monkeypatch.setattr(capi, "lib", lambda: Fake)
    t = Thing(0x1234)
    t.close()
    assert freed == [0x1234] and not t.h
    t.close()
    del t
    assert freed == [0x1234]
    u = Thing(0x5678)
    del u                                              # the guarded __del__ closes
    assert freed == [0x1234, 0x5678]
    view = Thing(0x9abc)                               # adopted, then given up: Sessions.map_export's view of a map it does not own
    view.h = C.c_void_p()
    view.close()
    del view
    assert freed == [0x1234, 0x5678]
    for cls, fn in ((capi.Context, "ndt_ctx_destroy"), (capi.Sessions, "ndt_sessions_destroy"), (capi.Map, "ndt_map_destroy"),
                    (capi.OccGrid, "ndt_occ_destroy")):
        assert issubclass(cls, capi._Handle) and cls._destroy == fn and "close" not in vars(cls) and "__del__" not in vars(cls)
    m = capi.Map.adopt(None, 0x4321, None)
    assert m.h.value == 0x4321
    m.close()
    assert freed[-1] == 0x4321 and not m.h


def test_errors_without_a_context_carry_the_code_and_the_library_text(capi):
    with pytest.raises(capi.NdtError) as e:
        capi.resample_capacity(100, -1.0, 0.25)
    assert str(e.value).startswith("ndt_resample_capacity -> %d: " % capi.NDT_E_ARG) and "ndt_resample_capacity: bad arguments" in str(e.value)
    lat = capi.PoseLattice(x0=0.0, y0=0.0, yaw0=0.0, step_x=0.1, step_y=0.1, step_yaw=0.1, nx=0, ny=3, nyaw=3)
    with pytest.raises(capi.NdtError) as e:
        lat.size
    assert str(e.value).startswith("ndt_lattice_size -> %d: ndt_lattice_size: " % capi.NDT_E_ARG) and "a dimension below 1" in str(e.value)
    with pytest.raises(capi.NdtError) as e:
        capi.OccGeometry(0.0, 0.0, -1.0, 4, 4).cell(0.0, 0.0)
    assert str(e.value).startswith("ndt_occ_cell -> %d: ndt_occ_cell: " % capi.NDT_E_ARG)
    # the same function behind Context.check, with a context handle (None here: the thread's last error)
    assert str(capi._error(-1, "what")).startswith("what -> -1: ")


def test_default_params_overrides(capi):
    p = capi.default_session_params(match_resolution=0.5, fuse_score_thre=1.25, space_thre=0.3, remove_moving=0)
    assert (p.match.resolution, p.fuse.score_thre, p.space_thre, p.remove_moving) == (0.5, 1.25, 0.3, 0)
    for bad in ("match", "fuse", "match_nope", "fuse_nope", "nope"):
        with pytest.raises(AttributeError, match=bad):
            capi.default_session_params(**{bad: 1})
    for fn in (capi.default_params, capi.default_fuse_params, capi.default_pg_params):
        with pytest.raises(AttributeError, match="nope"):
            fn(nope=1)
    assert capi.default_params("pcl18", max_iter=7).max_iter == 7 and capi.default_pg_params(max_iter=3).max_iter == 3
    assert capi.default_fuse_params(coe_vel=3.0).coe_vel == 3.0
