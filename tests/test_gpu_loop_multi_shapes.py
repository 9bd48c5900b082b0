"""ndt_sessions_find_loops_multi and ndt_sessions_find_cross_loops across candidate shapes (tests/loop_multi_shape_workloads.py):
every family on a capi.Sessions set beside the composed chain, as tests/test_gpu_loop_shapes.py holds the single search.  At
every search, through the raw call on buffers pre-filled with a sentinel byte: the candidates are the library's own candidate
call and the numpy gate on the chain's layout (multi) or on the set's read-outs (cross); status, n_cand, cand_index, cand_score
and the written records are byte for byte the composition of public single-job calls (guarantee a: loops_helpers.compose_loop,
cross_loops_helpers.compose_cross) on the searcher's scan and the OWNER's closed cloud; fit is Map.fit_points of a fresh map of
that cloud at the records' transforms (guarantee b); cand_cost, best, found, pose and edge follow the rule restated
(loops_multi_helpers.decide_ref) and pg_edge_between at the owner's anchor pose; nothing behind n_out, behind n_cand or in a
candidate without a record is written; host_waits is derived from the chain's data; a candidate's bytes do not depend on who
else is named or on max_submaps; the set's snapshots around the searches of a step are equal.  The certificates that are
statements about picks and decisions are checked here, on the composed reference.  There is no tolerance in this module."""
import ctypes
import time

import numpy as np
import pytest

import loop_multi_shape_workloads as M
import test_gpu_loop_shapes as T
from cross_loops_helpers import assert_set_candidates, compose_cross
from loops_helpers import chain_layout, compose_loop, same_candidate
from loops_multi_helpers import NOT_USABLE_COST, gate_multi_ref
from test_gpu_loop_shapes import SENTINEL, raw, untouched
from test_gpu_loops_multi import assert_decision, field_rows, filtered_newest
from test_gpu_sessions_correct import chain_poses
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

_T0, _RUNS, _TIMES = [None], {}, {}


def sentinel_array(dtype, shape):
    n = int(np.prod(shape))
    return np.frombuffer(bytearray([SENTINEL]) * (n * dtype.itemsize), dtype=dtype).reshape(shape)


def raw_ranked(capi, ses, kind, mp, which, against=None):
    """ndt_sessions_find_loops_multi or ndt_sessions_find_cross_loops through ctypes on buffers pre-filled with the sentinel
    byte, NDT_LOOP_MAX_SUBMAPS records per session of the set -> (the J records, the J rows of record slots, the stats).
    Nothing behind the J candidates is written."""
    room = ses.n * capi.NDT_LOOP_MAX_SUBMAPS
    out = sentinel_array(capi.CROSS_LOOP_DTYPE if kind == "cross" else capi.LOOP_MULTI_DTYPE, (room,))
    rec = sentinel_array(capi.RESULT_DTYPE, (room, capi.NDT_LOOP_MAX_CAND))
    n = ctypes.c_int(-1)
    w = np.ascontiguousarray(which, np.uint8)
    assert len(w) == ses.n
    if kind == "cross":
        a = None if against is None else np.ascontiguousarray(against, np.uint8)
        rc = capi.lib().ndt_sessions_find_cross_loops(ses.h, w.ctypes.data, None if a is None else a.ctypes.data, ctypes.byref(mp),
                                                      out.ctypes.data, ctypes.byref(n), rec.ctypes.data)
    else:
        rc = capi.lib().ndt_sessions_find_loops_multi(ses.h, w.ctypes.data, ctypes.byref(mp), out.ctypes.data, ctypes.byref(n), rec.ctypes.data)
    assert rc == 0, (rc, capi.lib().ndt_last_error(ses.ctx.h).decode())
    J = n.value
    assert 0 <= J <= room and untouched(out[J:]) and untouched(rec[J:])
    return out[:J], rec[:J], ses.stats()


def multi_of(kind, out):
    """The ndt_loop_multi records of a call's output (views of the memory the library wrote)."""
    return out["m"] if kind == "cross" else out


def keys_of(kind, out):
    """[(searcher, rank, owner, submap)] of a call's records."""
    lm = multi_of(kind, out)
    owner = out["map_session"] if kind == "cross" else lm["loop"]["cand"]["session"]
    return [(int(s), int(r), int(o), int(m)) for s, r, o, m in zip(lm["loop"]["cand"]["session"], lm["rank"], owner, lm["loop"]["cand"]["submap"])]


def whole(out, recs, j):
    """Candidate j's whole record (ndt_loop_multi or ndt_cross_loop, padding and reserved fields included) and its written
    match records, from the memory the library wrote."""
    lm = out["m"] if "m" in out.dtype.names else out
    return raw(out)[j].tobytes() + raw(recs)[j][:int(lm[j]["loop"]["n_cand"]) * recs.dtype.itemsize].tobytes()


def zero_record(capi, kind, out, j, status, mp):
    """The bytes of the whole record of a candidate that made no match record: everything 0 but cand, status, best, the
    edge's ends and info, rank and (cross) map_session."""
    want = np.zeros(1, out.dtype)
    lm, got = multi_of(kind, want), multi_of(kind, out)
    path = ("m", "loop", "cand") if kind == "cross" else ("loop", "cand")
    field_rows(want, *path)[0, :] = field_rows(out, *path)[j]
    L = lm["loop"]
    L["status"][0], L["best"][0] = status, -1
    L["edge"]["from_"][0], L["edge"]["to"][0] = got[j]["loop"]["cand"]["anchor_scan"], got[j]["loop"]["cand"]["newest_scan"]
    L["edge"]["info"][0] = np.array(mp.loop.info[:])
    lm["rank"][0] = got[j]["rank"]
    if kind == "cross":
        want["map_session"][0] = out[j]["map_session"]
    return raw(want)[0].tobytes()


def composed(sc, kind, k, a, b, cand, mp):
    """Candidate (searcher class a, owner class b, cand.submap) composed of public single-job calls on the chain behind step k
    -> (dict(status, n_cand, cand_index, cand_score, n_src), records, FIT_STATS records).  Made once per class pair, submap,
    lattice and pick parameters; the statistics once more per max_d2."""
    capi, ctx, chain = sc["capi"], sc["ctx"], sc["chain"]
    cache = sc.setdefault("composed", {})
    m = int(cand["submap"])
    key = (kind, k, a, b, m, cand["lattice"].tobytes(), mp.loop.top_k, mp.loop.local_max)
    if key not in cache:
        if kind == "cross":
            ref, recs, _ = compose_cross(sc, a, b, cand, mp)
        else:
            assert a == b
            ref, recs = compose_loop(sc, a, cand, mp.loop)
        cache[key] = (ref, recs, {})
    ref, recs, fits = cache[key]
    n = int(ref["n_cand"])
    if mp.max_d2 not in fits:
        fit = np.zeros(0, capi.FIT_STATS_DTYPE)
        if n:
            src = filtered_newest(sc, a)
            gm = capi.Map(ctx, np.ascontiguousarray(chain.pcmaps[b].submaps[m].p_cloud, np.float32).reshape(-1, 2), chain.params)
            _, fit = gm.fit_points(np.tile(src, (n, 1)), np.arange(n + 1) * len(src), recs, max_d2=mp.max_d2, want_d2=False)
            gm.close()
            assert all(int(s["n_points"]) == len(src) for s in fit)
        fits[mp.max_d2] = fit
    return ref, recs, fits[mp.max_d2]


def expected_waits(chain, cls, kind, gated, keys, status):
    """host_waits of a call from the chain's data: the cross gate's wait where it ran; nothing more without a candidate or when
    every searcher's newest scan is empty (nothing is queued); then the bounding boxes' wait, and the read-back's when any map
    could be built."""
    waits = int(gated)
    if not keys or all(len(chain.pcmaps[cls[s]].submaps[-1].scans[-1]) == 0 for s, _, _, _ in keys):
        return waits
    return waits + (2 if any(st == 0 for st in status) else 1)


def search_ranked(sc, ses, fam, call):
    """One multi or cross search of a family, with every check that holds for any family -> dict(kind, loops, recs, keys, refs:
    per candidate composed()'s triple, stats, clouds: per candidate the points of its closed cloud)."""
    capi, chain, cls, kind = sc["capi"], sc["chain"], fam["cls"], M.kind_of(call)
    S, tag = len(cls), (fam["name"], call["tag"])
    mp, which, against = M.multi_params(capi, call), np.array(call["which"], np.uint8), call.get("against")
    out, recs, st = raw_ranked(capi, ses, kind, mp, which, against)
    lm, keys, J = multi_of(kind, out), keys_of(kind, out), len(out)
    # the candidates: the library's own candidate call, and the numpy gate
    if kind == "cross":
        cc = ses.cross_candidates(mp, which, against)
        assert len(cc) == J and field_rows(out, "m", "loop", "cand").tobytes() == field_rows(cc, "cand").tobytes(), tag
        assert out["map_session"].tolist() == cc["map_session"].tolist() and lm["rank"].tolist() == cc["rank"].tolist(), tag
        assert_set_candidates(capi, ses, cc, mp, which, against)
        tracks = [i for i in range(S) if (against is None or against[i]) and len(chain.pcmaps[cls[i]].submaps) >= 2]
        gated = bool(tracks) and any(which[i] and len(chain.pcmaps[cls[i]].poses) for i in range(S))
        assert all(s != o and o in tracks for s, _, o, _ in keys), tag
    else:
        assert field_rows(out, "loop", "cand").tobytes() == raw(ses.loop_candidates_multi(mp, which)).tobytes(), tag
        want = [(i, r, g) for i in range(S) if which[i] and len(chain.pcmaps[cls[i]].poses)
                for r, g in enumerate(gate_multi_ref(*chain_layout(chain, cls[i]), mp.max_submaps, **M.gate_of(call["lp"])))]
        assert [(s, r) for s, r, _, _ in keys] == [(i, r) for i, r, _ in want], tag
        assert all(same_candidate(lm[j]["loop"]["cand"], g) for j, (_, _, g) in enumerate(want)), tag
        gated = False
    assert all(r == (keys[j - 1][1] + 1 if j and keys[j - 1][0] == s else 0) for j, (s, r, _, _) in enumerate(keys)), tag
    refs = []
    for j, (s, r, o, m) in enumerate(keys):
        loop, rec = lm[j]["loop"], recs[j]
        ref, want, fit = composed(sc, kind, call["k"], cls[s], cls[o], loop["cand"], mp)
        refs.append((ref, want, fit))
        n = int(ref["n_cand"])
        # (a) the single search's part, (b) the ranged statistics, byte for byte
        assert loop["status"] == ref["status"] and loop["n_cand"] == n and 0 <= n <= mp.loop.top_k, (tag, keys[j], loop["status"], loop["n_cand"], n)
        for f in ("cand_index", "cand_score"):
            assert loop[f][:n].tobytes() == ref[f].tobytes() and not loop[f][n:].any(), (tag, keys[j], f)
        assert raw(recs)[j][:n * capi.RESULT_BYTES].tobytes() == want.tobytes(), (tag, keys[j])
        assert untouched(rec[n:]), (tag, keys[j])                           # no record slot behind n_cand is written
        assert lm[j]["fit"][:n].tobytes() == fit.tobytes() and not lm[j]["fit"][n:].tobytes().strip(b"\0"), (tag, keys[j], lm[j]["fit"][:n], fit)
        assert lm[j]["reserved"] == 0 and (kind != "cross" or out[j]["reserved"] == 0), (tag, keys[j])
        # the decision, the edge from the OWNER's anchor pose
        assert_decision(capi, lm[j], rec, chain_poses(chain, cls[o]), mp)
        if n == 0:
            assert raw(out)[j].tobytes() == zero_record(capi, kind, out, j, ref["status"], mp), (tag, keys[j])
    status = [ref["status"] for ref, _, _ in refs]
    waits = expected_waits(chain, cls, kind, gated, keys, status)
    assert (st.host_waits, st.sessions_stepped) == (waits, J), (tag, st.host_waits, waits, st.sessions_stepped, J)
    if waits == 0:
        assert (st.h2d_bytes, st.d2h_bytes) == (0, 0), tag
    # independence: every searcher alone (a large set: every third session); for multi, max_submaps lowered to rank + 1
    searchers = sorted({s for s, _, _, _ in keys})
    subsets = [[s] for s in searchers] if S <= 16 else [[i for i in range(S) if i % 3 == 0]]
    for keep in subsets:
        sub = np.array([1 if (i in keep and which[i]) else 0 for i in range(S)], np.uint8)
        o2, r2, st2 = raw_ranked(capi, ses, kind, mp, sub, against)
        js = [j for j in range(J) if keys[j][0] in keep]
        assert keys_of(kind, o2) == [keys[j] for j in js] and len(js) >= 1, (tag, keep)
        for a, j in enumerate(js):
            assert whole(o2, r2, a) == whole(out, recs, j) and untouched(r2[a][int(lm[j]["loop"]["n_cand"]):]), (tag, keep, keys[j])
        w2 = expected_waits(chain, cls, kind, gated, [keys[j] for j in js], [status[j] for j in js])
        assert (st2.host_waits, st2.sessions_stepped) == (w2, len(js)), (tag, keep, st2.host_waits, w2)
    if kind == "multi":
        for top in sorted({r + 1 for _, r, _, _ in keys if r + 1 < mp.max_submaps}):
            narrow = M.multi_params(capi, dict(call, mp=dict(call["mp"], max_submaps=top)))
            o2, r2, _ = raw_ranked(capi, ses, kind, narrow, which)
            js = [j for j in range(J) if keys[j][1] < top]
            assert keys_of(kind, o2) == [keys[j] for j in js], (tag, top)
            assert all(whole(o2, r2, a) == whole(out, recs, j) for a, j in enumerate(js)), (tag, top)
    L = lm["loop"]
    print("%s %s: J %d keys %s n_cand %s best %s found %s status %s waits %d" % (
        fam["name"], call["tag"], J, keys[:6], L["n_cand"].tolist()[:12], L["best"].tolist()[:12], L["found"].tolist()[:12],
        L["status"].tolist()[:12], st.host_waits))
    return dict(kind=kind, loops=out, recs=recs, keys=keys, refs=refs, stats=st,
                clouds=[len(chain.pcmaps[cls[o]].submaps[m].p_cloud) for _, _, o, m in keys])


def search(sc, ses, fam, call):
    if M.kind_of(call) == "single":
        res = T.search(sc, ses, fam, call)
        cls = fam["cls"]
        res.update(kind="single", keys=[(int(s), 0, int(s), int(m)) for s, m in zip(res["loops"]["cand"]["session"], res["loops"]["cand"]["submap"])])
        res["clouds"] = [res["clouds"][cls[s]] for s, _, _, _ in res["keys"]]
        return res
    return search_ranked(sc, ses, fam, call)


def run_cached(gpu, name):
    if _T0[0] is None:
        _T0[0] = time.perf_counter()
    if name not in _RUNS:
        capi, ctx = gpu
        t0 = time.perf_counter()
        _RUNS[name] = T.run_family(capi, ctx, M.family(name), search)
        _TIMES[name] = time.perf_counter() - t0
    return _RUNS[name]


def results(res):
    """{(searcher, rank, owner, submap): (its ndt_loop_multi, its whole result as bytes)}"""
    lm = multi_of(res["kind"], res["loops"])
    return {key: (lm[j], whole(res["loops"], res["recs"], j)) for j, key in enumerate(res["keys"])}


# ---------------------------------------------------------------------------------------------- the certificates on the composed reference
def check_ragged_ranks(capi, fam, out):
    (res,) = out
    per = [sum(1 for s, _, _, _ in res["keys"] if s == i) for i in range(4)]
    assert per == fam["per_session"] == [1, 2, 3, 4]
    assert [[m for s, _, _, m in res["keys"] if s == i] for i in range(4)] == fam["submaps"]
    n_src = [res["refs"][[s for s, _, _, _ in res["keys"]].index(i)][0]["n_src"] for i in range(4)]
    print("ragged_ranks: filtered lengths %s" % n_src)
    assert len(set(n_src)) == 4 and min(n_src) == 1, n_src
    # picks in later slots (c >= 1) of candidates of at least three different lengths, behind candidates of a shared scan
    L = multi_of("multi", res["loops"])["loop"]
    assert len({n_src[s] for j, (s, _, _, _) in enumerate(res["keys"]) if L[j]["n_cand"] >= 2}) >= 3, L["n_cand"]


def check_many_ranks(capi, fam, out):
    (res,) = out
    cls = fam["cls"]
    assert len(res["loops"]) == 260 > 256 and [k[:2] for k in res["keys"]] == [(i, r) for i in range(65) for r in range(4)]
    first = {}
    assert capi.LOOP_CANDIDATE_DTYPE.fields["session"][1] == 0 and capi.LOOP_MULTI_DTYPE.fields["loop"][1] == 0 and capi.LOOP_DTYPE.fields["cand"][1] == 0
    for j, (s, r, _, m) in enumerate(res["keys"]):
        anon = whole(res["loops"], res["recs"], j)[4:]                        # (cand.session is the first four bytes)
        first.setdefault((cls[s], m), anon)
        assert anon == first[(cls[s], m)], (j, s, r)                          # a class's bytes apart from cand.session
    assert len(first) == len(set(first.values())) == 20
    L = multi_of("multi", res["loops"])["loop"]
    assert sum(1 for n in L["n_cand"] if n >= 2) >= 130 and sum(1 for n in L["n_cand"][256:] if n >= 2) >= 2


def check_refused_ranks(capi, fam, out):
    every, without = (results(r) for r in out[:2])
    bad, rank = fam["bad"], fam["bad_rank"]
    lm = multi_of("multi", out[0]["loops"])
    refused = [key[:2] for j, key in enumerate(out[0]["keys"]) if lm[j]["loop"]["status"] != capi.NDT_OK]
    assert refused == [(bad, rank)] and len(out[0]["keys"]) == 12, refused
    assert every[[k for k in every if k[:2] == (bad, rank)][0]][0]["loop"]["status"] == capi.NDT_E_GRID
    assert sorted(without) == sorted(k for k in every if k[0] != bad) and all(without[k][1] == every[k][1] for k in without)
    assert sum(1 for k in every if every[k][0]["loop"]["n_cand"] >= 1) >= 9
    if rank == 0:
        # the refused candidate is the call's first: the stand-in map of every refused slot is a map of rank >= 1
        assert out[0]["keys"][0][:2] == (bad, 0) and bad == 0
        alone = out[2]
        assert alone["keys"] == [out[0]["keys"][0]] and alone["stats"].host_waits == 1
        assert multi_of("multi", alone["loops"])[0]["loop"]["status"] == capi.NDT_E_GRID


def slot_sequence(fam, out):
    """{(session, rank): [(call index, owner, submap, points of the cloud)]}: what every map slot met over the family's calls."""
    seq = {}
    for q, res in enumerate(out):
        for (s, r, o, m), n in zip(res["keys"], res["clouds"]):
            seq.setdefault((s, r), []).append((q, o, m, n))
    return seq


def check_slot_history(capi, fam, out):
    kinds = [r["kind"] for r in out]
    assert {"single", "multi", "cross"} == set(kinds) and len({c["k"] for c in fam["calls"]}) == 3
    assert all(a != b for a, b in zip(kinds, kinds[1:]) if "single" in (a, b))
    seq = slot_sequence(fam, out)
    shrinks_and_grows = [k for k, v in seq.items() if k[1] >= 1 and len({n for _, _, _, n in v}) >= 3 and
                         any(v[i][3] > v[i + 1][3] < v[i + 2][3] for i in range(len(v) - 2))]
    foreign_then_own = [k for k, v in seq.items() if any(v[i][1] != k[0] and v[i + 1][1] == k[0] for i in range(len(v) - 1))]
    print("slot_history: slots of rank >= 1 whose cloud shrinks and grows %s; slots with another session's cloud, then their own %s"
          % (shrinks_and_grows, foreign_then_own))
    print("slot_history: session 1, rank 2 met %s" % seq.get((1, 2)))
    assert shrinks_and_grows and foreign_then_own
    L = [multi_of(r["kind"], r["loops"])["loop"] if r["kind"] != "single" else r["loops"] for r in out]
    assert all((l["n_cand"] >= 1).any() for l in L)


def check_cross_owners(capi, fam, out):
    pair, every = out
    B, C = fam["not_a_track"], fam["silent_track"]
    for res in out:
        assert any(s == B for s, _, _, _ in res["keys"]) and all(o != B for _, _, o, _ in res["keys"])
    assert all(s != C for s, _, _, _ in every["keys"]) and any(o == C for _, _, o, _ in every["keys"])
    counts = lambda res: sorted({sum(1 for s, _, _, _ in res["keys"] if s == i) for i in range(4)} - {0})
    assert counts(pair) == [1, 2, 3] and counts(every) == [4]
    for res in out:
        got, lm = results(res), multi_of("cross", res["loops"])
        shared = {}
        for (s, r, o, m), (rec, b) in got.items():
            shared.setdefault((o, m), []).append((s, rec, b))
        twice = {k: v for k, v in shared.items() if len(v) >= 2}
        assert twice, res["keys"]
        # the same cloud under different scans: the results differ behind the candidate (each equals its own composition)
        picked = [k for k, v in twice.items() if all(rec["loop"]["n_cand"] >= 1 for _, rec, _ in v)]
        behind = capi.LOOP_CANDIDATE_DTYPE.itemsize
        assert picked and all(len({b[behind:] for _, _, b in twice[k]}) == len(twice[k]) for k in picked), twice.keys()
    lm = multi_of("cross", every["loops"])
    assert any(int(l["loop"]["cand"]["anchor_scan"]) > int(l["loop"]["cand"]["newest_scan"]) for l in lm)
    assert sum(1 for l in lm if l["loop"]["n_cand"] >= 1) >= 6


def check_cross_refused_empty(capi, fam, out):
    every, without, only = out
    bad, m = fam["bad"], fam["bad_submap"]
    got, rest, lm = results(every), results(without), multi_of("cross", every["loops"])
    on_bad = [k for k in got if k[2:] == (bad, m)]
    assert len(on_bad) == 2 and len({k[0] for k in on_bad}) == 2 and all(got[k][0]["loop"]["status"] == capi.NDT_E_GRID for k in on_bad)
    assert [k for k in got if got[k][0]["loop"]["status"] != capi.NDT_OK] == on_bad
    # a call without that track: the remaining (searcher, owner, submap) results are the same apart from the rank
    assert capi.CROSS_LOOP_DTYPE.fields["m"][1] == 0 and capi.LOOP_MULTI_DTYPE.fields["loop"][1] == 0
    n_loop = capi.LOOP_DTYPE.itemsize + capi.LOOP_MULTI_DTYPE.fields["fit"][0].itemsize
    by_pair = {(k[0], k[2], k[3]): v for k, v in got.items()}
    assert all(o != bad for _, _, o, _ in rest) and len(rest) == 8
    for (s, r, o, sub), (rec, b) in rest.items():
        a = by_pair[(s, o, sub)][1]
        assert b[:n_loop] == a[:n_loop] and b[capi.CROSS_LOOP_DTYPE.itemsize:] == a[capi.CROSS_LOOP_DTYPE.itemsize:], (s, r, o, sub)
    e = fam["empty"]
    mine = [k for k in got if k[0] == e]
    assert len(mine) == 4 and all((got[k][0]["loop"]["status"], got[k][0]["loop"]["n_cand"], got[k][0]["loop"]["best"]) == (0, 0, -1) for k in mine)
    assert sum(1 for l in lm if l["loop"]["n_cand"] >= 1) >= 4 and every["stats"].host_waits == 3
    st = only["stats"]
    assert [k[0] for k in only["keys"]] == [e] * 4 and (st.host_waits, st.sessions_stepped) == (1, 4)
    assert all(results(only)[k][1] == got[k][1] for k in only["keys"])


def check_cross_zero_pose(capi, fam, out):
    (res,) = out
    last, n, same = res["zero"]
    assert last == np.zeros(3).tobytes() and n > 0 and same
    lm = multi_of("cross", res["loops"])
    mine = [l for l, k in zip(lm, res["keys"]) if k[0] == fam["zero"]]
    assert mine and any(l["loop"]["n_cand"] >= 1 for l in mine) and all(k[2] == 1 - k[0] for k in res["keys"])


def check_decisions(capi, fam, out):
    mixed = not_argmin = later_best = 0
    n_rec = n_conv = 0
    wide_mixed = []
    for call, res in zip(fam["calls"], out):
        q, lm = call["lp"], multi_of("multi", res["loops"])
        assert len(lm) == 5, call["tag"]
        for j, l in enumerate(lm):
            loop, n = l["loop"], int(l["loop"]["n_cand"])
            assert 1 <= n <= q["top_k"], call["tag"]
            cost = loop["cand_cost"][:n]
            assert (cost <= NOT_USABLE_COST).all()
            usable = cost != NOT_USABLE_COST
            mixed += int(usable.any() and not usable.all())
            if "wide" in call["tag"]:
                wide_mixed.append((call["mp"]["min_overlap"], int(usable.sum()), n, [round(float(f["n_in"]) / max(int(f["n_points"]), 1), 2) for f in l["fit"][:n]]))
            not_argmin += int(int(loop["best"]) != int(np.argmin(cost)))
            later_best += int(loop["best"] > 0)
            conv = res["recs"][j][:n]["converged"]
            n_rec, n_conv = n_rec + n, n_conv + int(conv.sum())
            if q["max_cost"] == -M.INF:
                assert loop["found"] == 0, call["tag"]                       # (iv)
            if q["max_cost"] == M.INF:
                assert loop["found"] == 1, call["tag"]                       # an unusable record's cost 1e7 is <= +inf
    print("decisions: %d calls; candidates with usable and unusable slots %d, best != argmin(cand_cost) %d, best > 0 %d; %d records, %d converged"
          % (len(out), mixed, not_argmin, later_best, n_rec, n_conv))
    print("decisions: wide calls (min_overlap, usable, n, n_in / n_points per slot): %s" % wide_mixed)
    assert mixed >= 1                                                        # (i)
    assert not_argmin >= 1                                                   # (ii)
    assert later_best >= 1                                                   # (iii)


CHECKS = {"ragged_ranks": check_ragged_ranks, "many_ranks": check_many_ranks, "refused_rank3": check_refused_ranks,
          "refused_rank0_first": check_refused_ranks, "slot_history": check_slot_history, "cross_owners": check_cross_owners,
          "cross_refused_empty": check_cross_refused_empty, "cross_zero_pose": check_cross_zero_pose, "decisions": check_decisions}


@pytest.mark.parametrize("name", sorted(M.FAMILIES))
def test_both_searches_equal_the_composed_chain_on_every_family(gpu, name):
    assert sorted(CHECKS) == sorted(M.FAMILIES)
    out = run_cached(gpu, name)
    CHECKS[name](gpu[0], M.family(name), out)
    print("%s: %.1f s" % (name, _TIMES[name]))


def test_wall_time_of_the_module(gpu):
    """Prints the time from the module's first family to here (LOG.md keeps the figure measured on an MI355X)."""
    if _T0[0] is None:
        _T0[0] = time.perf_counter()
    print("tests/test_gpu_loop_multi_shapes.py: %.1f s from the first family to the last test, %d families run: %s"
          % (time.perf_counter() - _T0[0], len(_RUNS), {k: round(v, 1) for k, v in _TIMES.items()}))
