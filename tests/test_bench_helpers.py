"""CPU checks of bench.py's bookkeeping (the bench itself needs a GPU)."""
import json
import os

import numpy as np

import bench


def test_algorithmic_bytes_follow_survey_8d():
    res = np.zeros(2, dtype=[("evals", "i4"), ("kbar", "f8")])
    res["evals"] = [10, 20]; res["kbar"] = [2.0, 3.0]
    n = 1000
    want = 10 * n * (8 + 20 * 2.0) + 16 * n + 20 * n * (8 + 20 * 3.0) + 16 * n
    assert bench.algorithmic_bytes(res, n) == want


def test_traffic_summary_is_consistent_with_the_pmc_files():
    traffic, src = bench.measured_traffic()
    root = os.path.dirname(os.path.abspath(bench.__file__))
    if traffic is None:
        assert not os.path.isdir(os.path.join(root, "profiles")) or not [f for f in os.listdir(os.path.join(root, "profiles")) if f.endswith("_traffic.json")]
        return
    t = json.load(open(os.path.join(root, src)))
    # rocprofv3 reports KB; FETCH_SIZE counts half the bytes fetched on gfx950 (calibrated for this kernel's access
    # widths: profiles/r02_calib_fetch.txt), WRITE_SIZE is exact (MI355X_MICROARCH.md, HBM section)
    fetch_factor = 2.0 if src.endswith("r02_traffic.json") or "calib_fetch" in t.get("note", "") else 1.0
    assert traffic == (fetch_factor * t["fetch_size_kb"] + t["write_size_kb"]) * 1024.0
    assert 1e6 < traffic < 1e11


def test_gpus_n_without_a_launcher_starts_the_ranks_itself(monkeypatch, capsys):
    """`python bench.py --gpus 8` is one command (the form the driver uses at N = 1): without WORLD_SIZE the process becomes
    the launcher -- a child `python -m torch.distributed.run`, one rank per GPU on 127.0.0.1 -- relays rank 0's JSON line,
    passes everything else to stderr and exits with the ranks' status; it never reaches the rank code (no GPU here)."""
    import subprocess
    import sys
    import pytest
    seen = {}

    class FakeProc:
        def __init__(self, cmd, **kw):
            seen["cmd"], seen["kw"] = cmd, kw
            self.stdout = iter(["noise from a rank\n", '{"metric": "m", "n_gpus": 8}\n'])

        def wait(self):
            return 3

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(subprocess, "Popen", FakeProc)
    with pytest.raises(SystemExit) as e:
        bench.main(["--gpus", "8", "--steps", "2", "--warmup", "1"])
    assert e.value.code == 3                                         # a failing rank fails the command
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"] and "--nproc-per-node" in cmd
    assert cmd[cmd.index("--nproc-per-node") + 1] == "8" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == ["--gpus", "8", "--steps", "2", "--warmup", "1"] and cmd[-7].endswith("bench.py")
    assert seen["kw"]["env"]["MASTER_ADDR"] == "127.0.0.1" and seen["kw"]["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    out = capsys.readouterr()
    assert out.out == '{"metric": "m", "n_gpus": 8}\n' and "noise from a rank" in out.err


def test_a_rank_under_a_launcher_of_the_wrong_size_says_so(monkeypatch):
    import pytest
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        bench.init_env(bench.parse_args(["--gpus", "4"]))
    assert "WORLD_SIZE 2 != --gpus 4" in str(e.value)


def test_plain_run_is_the_default_and_dumps_are_off():
    a = bench.parse_args(["--gpus", "1", "--steps", "4", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 4 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_writes_every_record_field_as_float(tmp_path):
    from ndt_slam_amd import capi
    res = np.zeros(5, dtype=capi.RESULT_DTYPE)
    res["pose"] = np.arange(15.0).reshape(5, 3); res["T00"] = 0.5; res["iters"] = [1, 2, 3, 4, 5]; res["H"][:, 4] = -1.0
    assert bench.dump_outputs(str(tmp_path / "d"), res, {"best_seed": np.array([17.0])}) == 5
    got = {f.name[:-4]: np.load(f) for f in (tmp_path / "d").iterdir()}
    assert set(got) == set(capi.RESULT_DTYPE.names) | {"best_seed"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["T00"].dtype == np.float32 and got["iters"].dtype == np.float64
    assert got["pose"].tobytes() == res["pose"].tobytes() and got["iters"].tolist() == [1, 2, 3, 4, 5]
    assert got["H"].shape == (5, 9) and got["best_seed"].tolist() == [17.0]


def test_dump_outputs_samples_a_fixed_subset_above_the_size_cap(tmp_path):
    from ndt_slam_amd import capi
    res = np.zeros(1000, dtype=capi.RESULT_DTYPE)
    res["iters"] = np.arange(1000)
    cap = 100 * 256
    written = [bench.dump_outputs(str(tmp_path / run), res, {}, max_bytes=cap) for run in ("a", "b")]
    a = {f.name: np.load(f) for f in (tmp_path / "a").iterdir()}
    b = {f.name: np.load(f) for f in (tmp_path / "b").iterdir()}
    assert sum(x.nbytes for x in a.values()) <= cap
    idx = a["record_index.npy"]
    assert 0 < len(idx) < 1000 and np.all(np.diff(idx) > 0) and a["iters.npy"].tolist() == idx.tolist()
    assert written == [len(idx), len(idx)]
    assert all(a[n].tobytes() == b[n].tobytes() for n in a)
