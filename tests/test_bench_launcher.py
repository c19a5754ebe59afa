"""`python3 bench.py --gpus N` as a plain command (no torch.distributed.run around it) starts its own ranks as child
processes and ALWAYS ends with one JSON line: here without a GPU — both ranks say so, the launcher
reports it, nothing hangs, nothing is left running; on the GPU box with two ranks on the ONE device RCCL refuses, which is the
failure path of a real multi-GPU node (a rank that cannot make its communicator) exercised on hardware."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra, timeout, env_extra=None):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    env.pop("LOCAL_RANK", None)
    env.update(env_extra or {})
    t0 = time.time()
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py")] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env,
                         start_new_session=True)
    try:
        out, err = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, 9)
        raise
    return p.returncode, out.decode(), err.decode(), time.time() - t0


def _json_lines(out):
    return [json.loads(t) for t in out.splitlines() if t.strip().startswith("{")]


def _no_child_left(pgid):
    """no process of the launcher's group is alive any more (the group was the launcher's own session)"""
    try:
        os.killpg(pgid, 0)
        return False
    except ProcessLookupError:
        return True
    except PermissionError:
        return False


def test_launcher_without_a_gpu_reports_and_returns():
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("a GPU is visible: the no-GPU path is the CPU container's")
    rc, out, err, dt = _run(["--gpus", "2", "--steps", "20", "--warmup", "5"], timeout=120)
    assert rc != 0
    assert dt < 90, dt
    for r in (0, 1):
        assert f"rank {r}: no GPU visible" in err, err[-2000:]
    lines = _json_lines(out)
    assert len(lines) == 1, out
    line = lines[0]
    assert line["value"] is None and line["n_gpus"] == 2 and "error" in line
    assert line["steps"] == 20 and line["warmup"] == 5 and line["unit"] == "reads/s"


def test_one_rank_needs_no_launcher_and_fails_loudly_without_gpu():
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("a GPU is visible")
    rc, out, err, dt = _run(["--steps", "20", "--warmup", "5"], timeout=120)
    assert rc != 0 and "no GPU visible" in err and not _json_lines(out)


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_end_with_an_error_line():
    """Two ranks, one device: ncclCommInitRank refuses (or the run dies some other way) — either way ONE line comes out, it names
    the failure, the exit code is not 0 and the ranks are gone within the bound."""
    import torch
    if torch.cuda.device_count() != 1:
        pytest.skip("needs exactly one visible GPU")
    rc, out, err, dt = _run(["--gpus", "2", "--steps", "16", "--warmup", "8", "--no-config3", "--no-once-through", "--no-cpu-baseline",
                             "--run-timeout", "150"], timeout=400)
    lines = _json_lines(out)
    assert len(lines) == 1, (out, err[-3000:])
    line = lines[0]
    assert line["n_gpus"] == 2
    if rc == 0:      # (an RCCL that accepts two ranks on a device: then the run must be a complete one)
        assert line["value"] and line["config"]["rccl_ranks"] == 2
    else:
        assert "error" in line, line
    assert dt < 380


@pytest.mark.gpu
def test_whole_run_watchdog_writes_the_line_and_exits_3():
    """One rank driving the N > 1 path (JL_BENCH_FORCE_DIST=1) with a --run-timeout that expires inside the --full legs: the line
    holds what was measured so far (the headline figure) plus "error", the exit code is 3."""
    rc, out, err, dt = _run(["--steps", "64", "--warmup", "16", "--full", "--no-cpu-baseline", "--run-timeout", "2"], timeout=300,
                            env_extra={"JL_BENCH_FORCE_DIST": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29671", "RANK": "0",
                                       "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
    lines = _json_lines(out)
    assert len(lines) == 1, (out, err[-3000:])
    line = lines[0]
    if rc == 0:
        pytest.skip(f"the whole run took less than the time-out ({dt:.1f} s)")
    assert rc == 3 and "error" in line and "run-timeout" in line["error"], line
    assert "config3_strong" in line


def test_dump_outputs_writes_float_arrays_within_the_bound(tmp_path, monkeypatch):
    """`--dump-outputs`: every array of a step's result as float64 / float32 .npy; the per-read ids become a fixed sample when the
    whole would exceed the bound (here made small), the same sample every time."""
    import numpy as np
    # (importing bench.py sets a default queue count for the HIP runtime of its process: not for this one's)
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", os.environ.get("GPU_MAX_HW_QUEUES", "4"))

    import bench
    from minorseq_amd import capi
    v = np.zeros(3, dtype=capi.VARIANT)
    v["count"], v["p_value"] = [5, 6, 7], [1e-300, 0.5, 1.0]
    ph = dict(summary={k: i for i, k in enumerate(capi.SUMMARY_FIELDS)}, pos_cols=np.arange(2, dtype=np.uint32),
              hap_count=np.array([9, 4], np.uint32), hap_pattern=np.zeros((2, 2), np.uint8), hit=np.ones((3, 2), np.uint8), cooc=None,
              read_hap=np.arange(5000, dtype=np.uint16))
    bench.dump_outputs(str(tmp_path / "all"), dict(variants=v, phase=ph))
    got = {f[:-4]: np.load(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all")}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert (got["variants_count"] == [5, 6, 7]).all() and got["variants_p_value"][0] == 1e-300
    assert (got["phase_summary"] == np.arange(len(capi.SUMMARY_FIELDS))).all()
    assert (got["phase_read_hap"] == np.arange(5000)).all() and "phase_read_hap_index" not in got
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8000)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), dict(variants=v, phase=ph))
        assert sum(os.path.getsize(tmp_path / d / f) - 128 for f in os.listdir(tmp_path / d)) <= 8000
    idx = np.load(tmp_path / "s1" / "phase_read_hap_index.npy")
    assert 0 < len(idx) < 5000 and (np.diff(idx) > 0).all()
    assert (np.load(tmp_path / "s1" / "phase_read_hap.npy") == idx).all()
    assert (np.load(tmp_path / "s2" / "phase_read_hap_index.npy") == idx).all()


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    """A plain run: the headline fields and the configuration, none of the --full legs; --dump-outputs writes the last timed
    step's results, and a second run with the same arguments writes the same arrays."""
    import numpy as np
    dumps = []
    for rep in range(2):
        d = tmp_path / f"out{rep}"
        rc, out, err, dt = _run(["--steps", "20", "--warmup", "5", "--dump-outputs", str(d)], timeout=300)
        lines = _json_lines(out)
        assert rc == 0 and len(lines) == 1, (out, err[-3000:])
        line = lines[0]
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert line.get(k) is not None, k
        assert line["steps"] == 20 and line["value"] > 0 and line["ms_per_step"] > 0
        for k in ("roofline", "end_to_end", "once_through", "once_through_qv", "config3_strong", "config4_strong", "cpu_baseline"):
            assert k not in line, k
        got = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
        assert len(got["variants_count"]) == line["config"]["variants_called"] > 0
        assert got["phase_summary"][-1] == line["config"]["haplotypes"]
        assert len(got["phase_read_hap"]) == line["config"]["reads_per_gpu"]
        dumps.append(got)
    assert dumps[0].keys() == dumps[1].keys()
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k
