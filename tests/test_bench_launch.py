"""`python bench.py --gpus N` started plainly (the way the driver runs it) must start its own N ranks: the parent spawns
`python -m torch.distributed.run ... bench.py --gpus N` as a child BEFORE it touches a device and relays output and return code.
Rehearsed here on the CPU with MTTS_BENCH_DRYRUN=1 (ranks rendezvous over gloo, no product code runs)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def _run(args, extra_env=None):
    env = dict(os.environ, MTTS_BENCH_DRYRUN="1", OMP_NUM_THREADS="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(extra_env or {})
    return subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], env=env, capture_output=True, text=True, timeout=300)


def test_plain_launch_spawns_its_ranks():
    res = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout                      # exactly one JSON line, from rank 0
    d = json.loads(lines[0])
    assert d == {"dryrun": True, "n_gpus": 2, "max_rank": 1, "gpus_arg": 2}


def test_single_process_default_does_not_spawn():
    res = _run([])
    assert res.returncode == 0, res.stderr[-2000:]
    assert json.loads(res.stdout.strip().splitlines()[-1])["n_gpus"] == 1


def test_child_failure_is_relayed():
    res = _run(["--gpus", "2", "--no-such-flag"])
    assert res.returncode != 0


def test_full_is_accepted_alone_and_with_its_skip_options():
    for extra in (["--full"], ["--full", "--no-cpu-baseline", "--no-events"]):
        res = _run(["--gpus", "1", "--steps", "1", "--warmup", "0", *extra])
        assert res.returncode == 0, res.stderr[-2000:]


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)             # importing does not launch anything: the self-launch sits under __main__
    return mod


def test_dump_outputs_dtypes_and_budget(tmp_path, monkeypatch):
    """--dump-outputs: one .npy per output, float32 / float64 only, integers exact, and an array beyond its share of the
    budget stored as the same seeded sample in every call."""
    import numpy as np
    import torch
    bench = _bench_module()
    g = torch.Generator().manual_seed(0)
    mel = torch.randn(3, 5, 7, generator=g)
    half = torch.randn(4, 6, generator=g).to(torch.bfloat16)
    lens = torch.tensor([7, 5, 2 ** 40 + 1], dtype=torch.int64)
    bench.dump_outputs(tmp_path / "a", {"mel": mel, "half": half, "mel_lengths": lens})
    got = {f.stem: np.load(f) for f in (tmp_path / "a").iterdir()}
    assert sorted(got) == ["half", "mel", "mel_lengths"]
    assert got["mel"].dtype == np.float32 and np.array_equal(got["mel"], mel.numpy())
    assert got["half"].dtype == np.float32 and np.array_equal(got["half"], half.float().numpy())
    assert got["mel_lengths"].dtype == np.float64 and got["mel_lengths"].astype(np.int64).tolist() == lens.tolist()

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * 40 * 4)      # a share of 40 floats per array
    big = torch.arange(1000, dtype=torch.float32).reshape(10, 100)
    for d in ("b", "c"):
        bench.dump_outputs(tmp_path / d, {"big": big, "small": mel[0, 0]})
    b, c = np.load(tmp_path / "b" / "big.npy"), np.load(tmp_path / "c" / "big.npy")
    assert b.shape == (40,) and np.array_equal(b, c)                 # the same sample both times
    assert np.all(np.diff(b) > 0) and set(b.tolist()) <= set(range(1000))   # sorted, distinct elements of the array
    assert np.array_equal(np.load(tmp_path / "b" / "small.npy"), mel[0, 0].numpy())
    assert sum(f.stat().st_size - 128 for f in (tmp_path / "b").iterdir()) <= bench.DUMP_BUDGET_BYTES


@pytest.mark.gpu
def test_dump_outputs_of_the_timed_path_repeat(tmp_path):
    """Two runs of the same bench command write the same arrays: what synthesise() returned in the last timed step, from
    seeded weights, ids and noise (small batch; the JSON line reports the timed step count it was given)."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MTTS_BENCH_DRYRUN")}
    outs = []
    for d in ("a", "b"):
        res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2",
                              "--no-cpu-baseline", "--no-events", "--dump-outputs", str(tmp_path / d)],
                             env=env, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == 2 and line["config"]["per_gpu_batch"] == 2
        outs.append({f.stem: np.load(f) for f in (tmp_path / d).iterdir()})
    a, b = outs
    assert sorted(a) == sorted(b) == ["mel", "mel_lengths"]
    assert a["mel"].dtype == np.float32 and a["mel"].ndim == 3 and a["mel"].shape[:2] == (2, 100)
    assert a["mel_lengths"].dtype == np.float64 and a["mel_lengths"].max() == a["mel"].shape[-1]
    assert np.isfinite(a["mel"]).all() and a["mel"].std() > 0
    assert np.array_equal(a["mel"], b["mel"]) and np.array_equal(a["mel_lengths"], b["mel_lengths"])


@pytest.mark.gpu
def test_plain_run_measures_the_headline_only_and_full_adds_the_rest(tmp_path):
    """A plain run leaves `roofline` and `cpu_baseline` null (no pass of the model beyond warm-up and the timed steps); --full
    fills `roofline` from the per-kernel event pass, after the dump: same headline keys and the same arrays as the plain run."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MTTS_BENCH_DRYRUN")}
    lines, outs = {}, {}
    for kind, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline"])):
        res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2",
                              "--dump-outputs", str(tmp_path / kind), *extra], env=env, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        lines[kind] = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
        outs[kind] = {f.stem: np.load(f) for f in (tmp_path / kind).iterdir()}
    plain, full = lines["plain"], lines["full"]
    assert plain["roofline"] is None and plain["cpu_baseline"] is None and "precision" not in plain
    assert full["roofline"]["launches_per_step"] > 0 and full["roofline"]["gemm_ms_per_step"] > 0 and full["cpu_baseline"] is None
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert plain[k] == full[k]
    for line in (plain, full):
        assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 2 and line["warmup"] == 1
    assert sorted(outs["plain"]) == sorted(outs["full"]) == ["mel", "mel_lengths"]
    assert all(np.array_equal(outs["plain"][n], outs["full"][n]) for n in outs["plain"])
