"""ndt_sessions_find_loops across candidate shapes (tests/loop_shape_workloads.py): every family on a capi.Sessions set beside
the composed chain.  Every candidate is held to the numpy gating on the chain's layout, every ndt_loop and every written record
byte for byte to the composition of public single-job calls (loops_helpers.compose_loop) on the chain's own scans and closed
clouds; the tails behind n_cand, the record slots behind n_cand (through the raw call, on a buffer pre-filled with a sentinel
byte), the host waits and the independence of a candidate from who else is named are checked at every search, the set's
snapshots around the searches behind a step.  The certificates that are statements about picks are checked here, on the composed reference.  There is no tolerance
in this module."""
import ctypes
import time

import numpy as np
import pytest

import loop_shape_workloads as L
from loops_helpers import assert_loop_is, chain_layout, compose_loop, gate_ref, same_candidate
from session_correct_helpers import CorrectedChain
from session_helpers import lockstep, same_records
from test_gpu_sessions_correct import same_snapshot, snapshot
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
_T0, _RUNS = [None], {}


def raw_find(capi, ses, lp, which):
    """ndt_sessions_find_loops through ctypes on buffers pre-filled with the sentinel byte: NDT_LOOP_MAX_CAND record slots per
    session of the set -> (the J loops, the J rows of record slots, the stats).  Nothing behind the J candidates is written."""
    S = ses.n
    out = np.frombuffer(bytearray([SENTINEL]) * (S * capi.LOOP_DTYPE.itemsize), dtype=capi.LOOP_DTYPE)
    rec = np.frombuffer(bytearray([SENTINEL]) * (S * capi.NDT_LOOP_MAX_CAND * capi.RESULT_BYTES), dtype=capi.RESULT_DTYPE)
    rec = rec.reshape(S, capi.NDT_LOOP_MAX_CAND)
    n = ctypes.c_int(-1)
    w = np.ascontiguousarray(which, np.uint8)
    assert len(w) == S
    rc = capi.lib().ndt_sessions_find_loops(ses.h, w.ctypes.data, ctypes.byref(lp), out.ctypes.data, ctypes.byref(n), rec.ctypes.data)
    assert rc == 0, (rc, capi.lib().ndt_last_error(ses.ctx.h).decode())
    J = n.value
    assert 0 <= J <= S and untouched(out[J:]) and untouched(rec[J:])
    return out[:J], rec[:J], ses.stats()      # (views: a copy of a structured array does not carry its padding)


def raw(a):
    """The memory of a C-contiguous structured array, one row of bytes per first index (numpy copies structured elements field
    by field, so bytes are compared on the memory the library wrote)."""
    assert a.flags.c_contiguous
    return a.view(np.uint8).reshape(len(a), -1) if a.size else np.zeros((0, 0), np.uint8)


def untouched(a):
    return bool((raw(a) == SENTINEL).all())


def whole(capi, loops, recs, j):
    """Candidate j's whole ndt_loop and its written records as bytes (loops_helpers.loop_bytes on the call's own memory)."""
    return raw(loops)[j].tobytes() + raw(recs)[j][:int(loops[j]["n_cand"]) * capi.RESULT_BYTES].tobytes()


def cand_bytes(capi, loops):
    assert capi.LOOP_DTYPE.fields["cand"][1] == 0
    return raw(loops)[:, :capi.LOOP_CANDIDATE_DTYPE.itemsize].tobytes()


def zero_loop(capi, loops, j, status, lp):
    """The bytes of the whole ndt_loop of a candidate that made no record: everything 0 but cand (candidate j's own bytes),
    status, best and the edge's ends and info."""
    want = np.zeros(1, capi.LOOP_DTYPE)
    n = capi.LOOP_CANDIDATE_DTYPE.itemsize
    raw(want)[0, :n] = np.frombuffer(cand_bytes(capi, loops[j:j + 1]), np.uint8)
    want["status"][0], want["best"][0] = status, -1
    want["edge"]["from_"][0], want["edge"]["to"][0] = loops[j]["cand"]["anchor_scan"], loops[j]["cand"]["newest_scan"]
    want["edge"]["info"][0] = np.array(lp.info[:])
    return raw(want)[0].tobytes()


def expected_waits(chain, cls, loops, refs):
    """host_waits of a call from the chain's data: 0 without a candidate or when every newest scan is empty (nothing is queued),
    1 when no map could be built, 2 otherwise."""
    if not len(loops):
        return 0
    if all(len(chain.pcmaps[cls[int(s)]].submaps[-1].scans[-1]) == 0 for s in loops["cand"]["session"]):
        return 0
    return 2 if any(refs[cls[int(s)]][0]["status"] == 0 for s in loops["cand"]["session"]) else 1


def search(sc, ses, fam, call):
    """One search of a family, with every check that holds for any family -> dict(loops, recs, refs: per class compose_loop's
    pair, stats)."""
    capi, chain, cls = sc["capi"], sc["chain"], fam["cls"]
    S, tag = len(cls), (fam["name"], call["tag"])
    lp, which = L.loop_params(capi, call["lp"]), np.array(call["which"], np.uint8)
    loops, recs, st = raw_find(capi, ses, lp, which)
    assert cand_bytes(capi, loops) == raw(ses.loop_candidates(lp, which)).tobytes(), tag
    gates = {c: gate_ref(*chain_layout(chain, c), **L.gate_of(call["lp"])) for c in sorted({cls[i] for i in range(S) if which[i]})}
    assert loops["cand"]["session"].tolist() == [i for i in range(S) if which[i] and gates[cls[i]] is not None], tag
    refs = {}
    for j, (loop, rec) in enumerate(zip(loops, recs)):
        i = int(loop["cand"]["session"])
        c = cls[i]
        assert same_candidate(loop["cand"], gates[c]), (tag, i)
        if c not in refs:
            refs[c] = compose_loop(sc, c, loop["cand"], lp)
        ref, want = refs[c]
        assert_loop_is(loop, rec, ref, want, lp)
        n = int(loop["n_cand"])
        assert 0 <= n <= lp.top_k and untouched(rec[n:]), (tag, i, n)          # no record slot behind n_cand is written
        assert all(not loop[f][n:].any() for f in ("cand_index", "cand_score", "cand_cost")), (tag, i)
        if n == 0:
            assert raw(loops)[j].tobytes() == zero_loop(capi, loops, j, ref["status"], lp), (tag, i)
    waits = expected_waits(chain, cls, loops, refs)
    assert (st.host_waits, st.sessions_stepped) == (waits, len(loops)), (tag, st.host_waits, st.sessions_stepped)
    if waits == 0:
        assert (st.h2d_bytes, st.d2h_bytes) == (0, 0), tag
    # naming a subset of the sessions leaves each remaining candidate's bytes unchanged
    subsets = [[int(s)] for s in loops["cand"]["session"]] if S <= 8 else [[i for i in range(S) if i % 3 == 0]]
    for keep in subsets:
        sub = np.array([1 if (i in keep and which[i]) else 0 for i in range(S)], np.uint8)
        l2, r2, st2 = raw_find(capi, ses, lp, sub)
        js = [j for j in range(len(loops)) if int(loops[j]["cand"]["session"]) in keep]
        assert len(l2) == len(js) >= 1, (tag, keep)
        for a, j in enumerate(js):
            assert whole(capi, l2, r2, a) == whole(capi, loops, recs, j) and untouched(r2[a][int(l2[a]["n_cand"]):]), (tag, keep, j)
        assert (st2.host_waits, st2.sessions_stepped) == (expected_waits(chain, cls, l2, refs), len(js)), (tag, keep, st2.host_waits)
    print("%s %s: n_src %s n_cand %s best %s found %s status %s" % (
        fam["name"], call["tag"], [refs[cls[int(s)]][0]["n_src"] for s in loops["cand"]["session"]][:8], loops["n_cand"].tolist()[:8],
        loops["best"].tolist()[:8], loops["found"].tolist()[:8], loops["status"].tolist()[:8]))
    return dict(loops=loops, recs=recs, refs=refs, stats=st, clouds={
        c: len(chain.pcmaps[c].submaps[int(gates[c]["submap"])].p_cloud) for c in gates if gates[c] is not None})


def run_family(capi, ctx, fam, search=None):
    """The family's set beside the chain (one chain session per class), a twin set that never searches where the family asks
    for one -> the result of every call.  search: another search(sc, ses, fam, call) than this module's
    (tests/test_gpu_loop_multi_shapes.py)."""
    search = search or globals()["search"]
    cls, p = fam["cls"], fam["p"]
    S = len(cls)
    ses = capi.Sessions(ctx, S, capi.session_params_from_launch(p))
    twin = capi.Sessions(ctx, S, capi.session_params_from_launch(p)) if fam.get("twin") else None
    chain = CorrectedChain(capi, ctx, len(fam["logs"]), p, allow_item_failures=fam["tolerant"])
    sc = dict(capi=capi, ctx=ctx, chain=chain, p=p, ses=ses)
    out, steps_behind = [], 0
    try:
        for k, scans, odo, act in lockstep(fam["logs"], fam["starts"]):
            got = ses.step([scans[c] for c in cls], odo[cls], act[cls])
            want = chain.step(scans, odo, act)
            assert all(same_records(got[i], want[cls[i]]) for i in range(S)), (fam["name"], k)
            if twin is not None:                                            # the step behind a search is the step of a set that never searched
                assert got.tobytes() == twin.step([scans[c] for c in cls], odo[cls], act[cls]).tobytes(), (fam["name"], k)
                steps_behind += int(bool(out))
            calls = [call for call in fam["calls"] if call["k"] == k]
            if calls:                                                       # the searches behind a step change nothing a caller can read
                watch = list(range(S)) if S <= 8 else [0, 31, 63, 64]
                before = {i: snapshot(ses, i) for i in watch}
                out += [search(sc, ses, fam, call) for call in calls]
                assert all(same_snapshot(before[i], snapshot(ses, i)) for i in watch), (fam["name"], k)
        if twin is not None:
            assert steps_behind >= 1 and all(same_snapshot(snapshot(ses, i), snapshot(twin, i)) for i in range(S)), fam["name"]
        assert len(out) == len(fam["calls"])
        if "zero" in fam:
            z = fam["zero"]
            last = ses.trajectory(z)[0][-1]
            newest = np.ascontiguousarray(chain.pcmaps[z].submaps[-1].scans[-1], np.float32).reshape(-1, 2)
            robot = capi.repose_points(ctx, newest, [0, len(newest)], last.reshape(1, 3), np.zeros((1, 3)))
            out[0]["zero"] = (last.tobytes(), len(newest), robot.tobytes() == newest.tobytes())
        return out
    finally:
        ses.close(); chain.close()
        if twin is not None:
            twin.close()


def run_cached(gpu, name):
    if _T0[0] is None:
        _T0[0] = time.perf_counter()
    if name not in _RUNS:
        capi, ctx = gpu
        _RUNS[name] = run_family(capi, ctx, L.family(name))
    return _RUNS[name]


def session_results(capi, res):
    """{session: (its ndt_loop, its whole result as bytes)}"""
    return {int(loop["cand"]["session"]): (loop, whole(capi, res["loops"], res["recs"], j)) for j, loop in enumerate(res["loops"])}


def check_ragged(capi, fam, out):
    (res,) = out
    n_src = [res["refs"][c][0]["n_src"] for c in range(len(L.RAGGED))]
    assert len(res["loops"]) == len(L.RAGGED) and len(set(n_src)) == len(n_src) and min(n_src) == 1, n_src
    # picks in later slots (c >= 1) of at least three candidates of different lengths: c * len(j) is told apart from c * anything else
    assert sum(1 for loop in res["loops"] if loop["n_cand"] >= 2) >= 3, res["loops"]["n_cand"]


def check_dead_slots(capi, fam, out):
    nine, one = out
    assert all(0 < n < 8 for n in nine["loops"]["n_cand"]) and len(nine["loops"]) == 2, nine["loops"]["n_cand"]
    assert all(n <= 1 for n in one["loops"]["n_cand"]) and len(one["loops"]) == 2, one["loops"]["n_cand"]


def check_nothing_picked(capi, fam, out):
    both, neighbours = (session_results(capi, r) for r in out)
    far = both[fam["far"]][0]
    assert (far["status"], far["n_cand"], far["best"], far["found"]) == (capi.NDT_OK, 0, -1, 0)
    assert not far["pose"].any() and not far["edge"]["rel"].any()
    assert sorted(neighbours) == [0, 2] and all(neighbours[i][1] == both[i][1] for i in (0, 2))
    assert all(both[i][0]["n_cand"] >= 1 for i in (0, 2))


def check_empty_newest(capi, fam, out):
    mixed, only = out
    got = session_results(capi, mixed)
    for i in range(4):
        loop = got[i][0]
        if i in fam["empty"]:
            assert (loop["status"], loop["n_cand"], loop["best"], loop["found"]) == (capi.NDT_OK, 0, -1, 0) and mixed["refs"][i][0]["n_src"] == 0
        else:
            assert loop["n_cand"] >= 1
    assert mixed["stats"].host_waits == 2
    # every candidate's newest scan is empty: nothing is queued, every ndt_loop is the zero record (search() compared all of it)
    st = only["stats"]
    assert only["loops"]["cand"]["session"].tolist() == fam["empty"]
    assert (st.host_waits, st.sessions_stepped, st.h2d_bytes, st.d2h_bytes) == (0, 2, 0, 0)
    assert all((l["status"], l["n_cand"], l["best"], l["found"]) == (capi.NDT_OK, 0, -1, 0) for l in only["loops"])


def check_later_submap(capi, fam, out):
    (res,) = out
    assert res["loops"]["cand"]["submap"].tolist() == fam["submaps"] and sum(1 for n in res["loops"]["n_cand"] if n >= 1) >= 3


def check_refused(capi, fam, out):
    (res,) = out
    bad = fam["bad"]
    assert res["loops"]["status"].tolist() == [capi.NDT_E_GRID if i == bad else capi.NDT_OK for i in range(3)]
    assert all(res["loops"][i]["n_cand"] >= 1 for i in range(3) if i != bad)     # the others picked, from maps of their own
    l = res["loops"][bad]
    assert (l["n_cand"], l["best"], l["found"]) == (0, -1, 0) and untouched(res["recs"][bad])


def check_map_reuse(capi, fam, out):
    assert [int(r["loops"][0]["cand"]["submap"]) for r in out] == fam["submaps"]
    sizes = [r["clouds"][0] for r in out]
    print("map_reuse: candidate clouds of %s points" % sizes)
    assert len(set(sizes)) == 3 and sizes[1] < sizes[0] and sizes[2] > sizes[1]
    assert any(r["loops"][0]["n_cand"] >= 1 for r in out)


def check_picks_and_costs(capi, fam, out):
    converged = []
    for call, res in zip(fam["calls"], out):
        q = call["lp"]
        for loop, rec in zip(res["loops"], res["recs"]):
            assert 1 <= loop["n_cand"] <= q["top_k"], call["tag"]
            if q["max_cost"] == -L.INF:
                assert loop["found"] == 0, call["tag"]
            else:
                assert loop["found"] == int(loop["best"] >= 0) == 1, call["tag"]
            converged += rec[:int(loop["n_cand"])]["converged"].tolist()
    print("picks_and_costs: %d records, %d converged" % (len(converged), sum(converged)))
    assert any(converged)
    assert any(res["loops"][0]["n_cand"] == 8 for res in out) and any(res["loops"][0]["n_cand"] == 1 for res in out)


def check_many(capi, fam, out):
    (res,) = out
    cls = fam["cls"]
    assert len(res["loops"]) == L.MANY_S == 65 and res["loops"]["cand"]["session"].tolist() == list(range(65))
    first = {}
    assert capi.LOOP_CANDIDATE_DTYPE.fields["session"][1] == 0
    for j in range(len(res["loops"])):
        anon = whole(capi, res["loops"], res["recs"], j)[4:]                  # (cand.session is the first four bytes)
        first.setdefault(cls[j], anon)
        assert anon == first[cls[j]], j                                       # a class's bytes apart from cand.session
    assert len(set(first.values())) == len(L.MANY_CLASSES)
    assert [int(res["loops"][cls.index(c)]["cand"]["submap"]) for c in range(5)] == fam["submaps"]
    assert sum(1 for n in res["loops"]["n_cand"] if n >= 2) >= 33


def check_zero_pose(capi, fam, out):
    (res,) = out
    last, n, same = res["zero"]
    assert last == np.zeros(3).tobytes() and n > 0 and same
    assert res["loops"][0]["n_cand"] >= 1                                     # records were made from that scan: its bytes count
    assert res["loops"]["cand"]["session"].tolist() == [0, 1] and res["loops"][0]["cand"]["submap"] == 0 and res["loops"][0]["cand"]["dist"] == 0.0


CHECKS = {"ragged": check_ragged, "dead_slots": check_dead_slots, "nothing_picked": check_nothing_picked,
          "empty_newest": check_empty_newest, "later_submap": check_later_submap, "refused_first": check_refused,
          "refused_middle": check_refused, "map_reuse": check_map_reuse, "picks_and_costs": check_picks_and_costs, "many": check_many,
          "zero_pose": check_zero_pose}


@pytest.mark.parametrize("name", sorted(L.FAMILIES))
def test_the_search_equals_the_composed_chain_on_every_family(gpu, name):
    assert sorted(CHECKS) == sorted(L.FAMILIES)
    t0 = time.perf_counter()
    out = run_cached(gpu, name)
    CHECKS[name](gpu[0], L.family(name), out)
    print("%s: %.1f s" % (name, time.perf_counter() - t0))


def test_wall_time_of_the_module(gpu):
    """Prints the time from the module's first family to here (LOG.md keeps the figure measured on an MI355X)."""
    if _T0[0] is None:
        _T0[0] = time.perf_counter()
    print("tests/test_gpu_loop_shapes.py: %.1f s from the first family to the last test, %d families run" % (time.perf_counter() - _T0[0], len(_RUNS)))
