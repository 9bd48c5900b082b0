"""ndt_sessions_step across submap life cycles (tests/session_workloads.py): splits with nothing, one scan or two scans
to carry, empty and non-finite scans at every place of a submap, sessions without a map, a local map too wide for a voxel
grid, a scan triple too wide for the moving-object filter, the device form of the call, and more sessions than
session_plan_kernel has lanes.  Every comparison is byte equality: with session_helpers.ComposedChain (the step made of
the batched *_dev entry points, every triple recomputed), with a run of the same session in another set, or with clouds put
together from such runs.  Each family's certificate -- the branches it must reach -- is asserted on the chain's own
bookkeeping of the run on the device."""
import numpy as np
import pytest

import session_workloads as W
from session_helpers import ComposedChain, DevForm, device_cloud, lockstep, same_records
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu


def views(ses, i):
    """(local map, p_cloud) of session i, read from the device."""
    tp, tn, _ = ses.local_map(i)
    cp, cn = ses.submap_cloud(i)
    return device_cloud(tp, tn), device_cloud(cp, cn)


def same_export(a, b):
    return (a is None) == (b is None) and (a is None or all(a[f].tobytes() == b[f].tobytes() for f in b))


def run_set(capi, ctx, logs, starts, p):
    """Steps one capi.Sessions set -> per step [(record, local map, p_cloud, map export)] over the sessions."""
    ses = capi.Sessions(ctx, len(logs), capi.session_params_from_launch(p))
    hist = []
    for _, scans, odo, act in lockstep(logs, starts):
        recs = ses.step(scans, odo, act)
        hist.append([(recs[i].copy(),) + views(ses, i) + (ses.map_export(i),) for i in range(len(logs))])
    ses.close()
    return hist


def against_the_chain(capi, ctx, v, on_step=None):
    """Steps variant v through a set and the chain: per step and session the record, both views and the map's export (none
    where the chain has no map) are the chain's bytes, the stats describe the step; at the end the global map and its parts.
    on_step(k, ses, got, exports): the caller's own checks.  -> the census of the chain's bookkeeping."""
    logs, starts, p = v["logs"], v["starts"], v["p"]
    S = len(logs)
    ses = capi.Sessions(ctx, S, capi.session_params_from_launch(p))
    chain = ComposedChain(capi, ctx, S, p, allow_item_failures=v["tolerant"])
    history, records = [], []
    for k, scans, odo, act in lockstep(logs, starts):
        had = [chain.has_map(i) for i in range(S)]
        got = ses.step(scans, odo, act)                 # (a step that does not return NDT_OK raises)
        want = chain.step(scans, odo, act)
        exports = []
        for i in range(S):
            assert same_records(got[i], want[i]), (v["name"], k, i, got[i], want[i])
            target, cloud = views(ses, i)
            assert cloud.tobytes() == chain.p_cloud[i].tobytes(), (v["name"], k, i, len(cloud), len(chain.p_cloud[i]))
            assert target.tobytes() == chain.target[i].tobytes(), (v["name"], k, i, len(target), len(chain.target[i]))
            exports.append(ses.map_export(i))
            assert same_export(exports[i], chain.maps[i].export() if chain.maps[i] is not None else None), (v["name"], k, i)
        st = ses.stats()
        assert st.sessions_stepped == int(got["stepped"].sum()) and st.triples_run <= st.sessions_stepped
        assert act.any() and st.host_waits == 3, (k, st.host_waits)
        if on_step:
            on_step(k, ses, got, exports)
        records.append(want.copy())
        history.append(W.snapshot(chain, had))
    for i in range(S):
        g, parts = ses.global_map(i)
        wg, wparts = chain.global_map(i)
        assert g.tobytes() == np.ascontiguousarray(wg, np.float32).tobytes(), (v["name"], i)
        assert len(parts) == len(wparts) and all(x.tobytes() == np.ascontiguousarray(y, np.float32).tobytes()
                                                  for x, y in zip(parts, wparts)), (v["name"], i)
    ses.close()
    chain.close()
    census = W.session_census(history, records)
    print(v["name"], {k: {a: b for a, b in c.items() if b} for k, c in census.items()})
    return census


@pytest.mark.parametrize("name", [v["name"] for v in W.variants(W.CHAIN_FAMILIES)])
def test_family_equals_the_composed_chain(gpu, name):
    """Every family that refuses nothing, against the strict chain (an item it refuses is an assertion failure)."""
    capi, ctx = gpu
    v = W.variant(name)
    assert not v["tolerant"]
    census = against_the_chain(capi, ctx, v)
    assert not W.certificate_misses(census, v["certificate"]), (W.certificate_misses(census, v["certificate"]), census)


@pytest.mark.parametrize("name", [v["name"] for v in W.FAMILIES["grid_outlier"]])
def test_grid_outlier_costs_its_session_alone(gpu, name):
    """One raw point at (8000, 8000) m in one scan of one session: while that scan is in its local map, the map's box
    exceeds 2^28 cells (scan 3: steps 3, 4, 5; `first`, scan 0: steps 0 .. 3, a session that has no map to keep; `alone`:
    no other map in the step's build).  Every step returns NDT_OK; on the refused steps the session's record has
    stepped = 1 and status = NDT_E_GRID, its clouds are the computed ones (the tolerant chain's) and its map exports what
    it exported the step before -- nothing, if it had none; afterwards its map is the chain's again.  The sessions beside
    it are, at every step, what they are in a set without it."""
    capi, ctx = gpu
    v = W.variant(name)
    bad = v["bad"]
    refused, last = [], {"exports": [None] * len(v["logs"])}

    def on_step(k, ses, got, exports):
        if got[bad]["status"] != 0:
            assert got[bad]["stepped"] == 1 and got[bad]["status"] == capi.NDT_E_GRID
            assert same_export(exports[bad], last["exports"][bad]), k
            assert (exports[bad] is None) == (v["refused_steps"][0] == 0), k
            refused.append(k)
        last["exports"] = exports

    census = against_the_chain(capi, ctx, v, on_step)
    assert refused == v["refused_steps"], refused
    assert not W.certificate_misses(census, v["certificate"]), (W.certificate_misses(census, v["certificate"]), census)
    # the neighbours, in a set of their own
    logs, starts, keep = W.grid_outlier_clean_logs(v)
    if not keep:
        return
    with_it, without = run_set(capi, ctx, v["logs"], v["starts"], v["p"]), run_set(capi, ctx, logs, starts, v["p"])
    assert len(with_it) == len(without)
    for k in range(len(without)):
        for j, i in enumerate(keep):
            a, b = with_it[k][i], without[k][j]
            assert same_records(a[0], b[0]), (k, i)
            assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and same_export(a[3], b[3]), (k, i)


def test_span_outlier_skips_three_triples_and_recovers(gpu):
    """One raw point at (1e8, 0) in scan j = 2 of session 0, no split: the triples of steps j, j + 1 and j + 2 span more
    than 2^30 voxels.  On those steps the session has status NDT_E_ARG with stepped = 1, both views are empty and the map
    exports what it did at step j - 1; the neighbour equals its solo run throughout.  From step j + 3 the cloud is: the first
    scan, the survivors of every triple that does not hold scan j, the newest scan -- the survivors taken from a run of the
    same log without the point (under score_thre = -1: the same poses) as the growth of (p_cloud minus the newest scan)
    from one step to the next.  The local map is that cloud through the pre-filter."""
    capi, ctx = gpu
    from ndt_slam_amd import replay
    v = W.variant("span_outlier")
    p, j = v["p"], W.SPAN_SCAN
    got = run_set(capi, ctx, v["logs"], v["starts"], p)
    clean_logs = W.span_outlier_clean_logs(v)
    clean = run_set(capi, ctx, clean_logs, v["starts"], p)
    solo = run_set(capi, ctx, [v["logs"][1]], [0], p)
    n = len(got)
    assert n >= j + 5
    n_new = [len(replay.resample_points(clean_logs[0][0][k], p["space"], p["space_thre"])) for k in range(n)]
    prefix = [clean[k][0][2][:len(clean[k][0][2]) - n_new[k]] for k in range(n)]
    assert prefix[0].tobytes() == clean[0][0][2][n_new[0]:].tobytes() and len(prefix[0]) == n_new[0]   # one scan: twice
    survivors = {k: prefix[k][len(prefix[k - 1]):] for k in range(2, n)}
    assert all(prefix[k][:len(prefix[k - 1])].tobytes() == prefix[k - 1].tobytes() for k in range(1, n))
    assert len(prefix[1]) == len(prefix[0]) and all(len(survivors[k]) for k in survivors)
    statuses = []
    for k in range(n):
        rec, target, cloud, export = got[k][0]
        statuses.append(int(rec["status"]))
        assert rec["stepped"] == 1, k
        assert same_records(got[k][1][0], solo[k][0][0]), k
        assert all(got[k][1][f].tobytes() == solo[k][0][f].tobytes() for f in (1, 2)) and same_export(got[k][1][3], solo[k][0][3]), k
        if j <= k <= j + 2:
            assert rec["status"] == capi.NDT_E_ARG
            assert len(target) == 0 and len(cloud) == 0
            assert same_export(export, got[j - 1][0][3]) and export is not None
        # (the poses do not depend on a match; the cost does, and the maps of the two runs differ from step j on)
        assert all(rec[f].tobytes() == clean[k][0][0][f].tobytes() for f in ("pose", "cov", "matched", "successful", "submap", "split")), k
        if j <= k <= j + 2:
            pass
        elif k < j:
            assert same_records(rec, clean[k][0][0]) and cloud.tobytes() == clean[k][0][2].tobytes()
        else:
            assert rec["status"] == 0
            want = np.concatenate([prefix[0]] + [survivors[t] for t in range(2, k + 1) if not j <= t <= j + 2]
                                  + [clean[k][0][2][len(clean[k][0][2]) - n_new[k]:]])
            assert cloud.tobytes() == want.tobytes(), (k, len(cloud), len(want))
            assert target.tobytes() == ctx.prefilter(want, p["LeafSize"]).tobytes(), k
            assert not same_export(export, got[j - 1][0][3])
    assert statuses == [0] * j + [capi.NDT_E_ARG] * 3 + [0] * (n - j - 3), statuses


def test_device_form_equals_the_host_form(gpu):
    """split_every_other once more through ndt_sessions_step_dev: the raw scans at stride 24 behind five sentinel rows
    (raw_offsets[0] = 5), a sentinel in every pad column and in the rows of the session that is not active, the odometry in
    device memory.  Records, views and map exports are those of the host form at stride 16."""
    capi, ctx = gpu
    v = W.variant("split_every_other[rm=1]")
    logs, starts, p = v["logs"], v["starts"], v["p"]
    S = len(logs)
    host = run_set(capi, ctx, logs, starts, p)
    ses = capi.Sessions(ctx, S, capi.session_params_from_launch(p))
    idle = 0
    for k, scans, odo, act in lockstep(logs, starts):
        form = DevForm(scans, odo, act, stride=24, lead=5)
        assert form.offsets[0] == 5
        idle += int(not act.all())
        recs = form.step(ses, act)
        for i in range(S):
            assert same_records(recs[i], host[k][i][0]), (k, i, recs[i], host[k][i][0])
            target, cloud = views(ses, i)
            assert target.tobytes() == host[k][i][1].tobytes() and cloud.tobytes() == host[k][i][2].tobytes(), (k, i)
            assert same_export(ses.map_export(i), host[k][i][3]), (k, i)
    assert idle >= 1 and sum(int(h[0][0]["split"]) for h in host) >= 3
    ses.close()


def test_many_sessions_equal_their_class_twins(gpu):
    """1030 sessions, each a copy of one of ten (log, start) classes: session_plan_kernel takes sessions 1024.. in a second
    round that carries the first round's total.  Every session's record and both views, at every step, are those of its
    class in a set of ten; the map exports are compared at the last step."""
    capi, ctx = gpu
    logs, starts, cls = W.many_sessions()
    p = W.launch_params(sepThre=1e9, score_thre=-1.0)
    twins = run_set(capi, ctx, logs, starts, p)
    ses = capi.Sessions(ctx, len(cls), capi.session_params_from_launch(p))
    for k, scans, odo, act in lockstep([logs[c] for c in cls], [starts[c] for c in cls]):
        recs = ses.step(scans, odo, act)
        assert recs["stepped"].tolist() == [int(twins[k][c][0]["stepped"]) for c in cls]
        for i, c in enumerate(cls):
            assert same_records(recs[i], twins[k][c][0]), (k, i, c)
            target, cloud = views(ses, i)
            assert target.tobytes() == twins[k][c][1].tobytes() and cloud.tobytes() == twins[k][c][2].tobytes(), (k, i, c)
        assert ses.stats().sessions_stepped == int(recs["stepped"].sum())
    tri = {c for c in range(len(logs)) if starts[c] + len(logs[c][0]) == 4 and len(logs[c][0]) >= 3}
    assert k == 3 and ses.stats().triples_run == sum(1 for c in cls if c in tri)
    assert any(c in tri for c in cls[1024:]) and any(c not in tri for c in cls[1024:])      # (the second round runs both kinds)
    for i, c in enumerate(cls):
        assert same_export(ses.map_export(i), twins[-1][c][3]), (i, c)
    ses.close()
