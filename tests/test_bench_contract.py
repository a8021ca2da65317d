"""bench.py contract tests: the driver runs
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N
 --master-addr 127.0.0.1 bench.py --gpus N ...` — verify that exact
invocation works (CPU device here; RCCL path shares all code but the
backend)."""

import json
import os
import socket
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_bench(extra, env=None):
    out = subprocess.run(
        [sys.executable] + extra,
        cwd=REPO, env=dict(os.environ, PYTHONPATH=REPO, **(env or {})),
        capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)


def run_torchrun_bench(nproc, bench_args):
    """torchrun rendezvous can transiently fail under suite load (the
    probed free port may be reclaimed, or an N-rank gloo full-mesh can
    time out on a loaded box) — retry with fresh ports; measured ~1 in
    10 suite runs for the 8-rank canary with a single retry."""
    last = None
    for _ in range(3):
        port = free_port()
        try:
            return run_bench([
                "-m", "torch.distributed.run", "--nnodes=1",
                "--nproc-per-node", str(nproc),
                "--master-addr", "127.0.0.1", "--master-port", str(port),
                "bench.py"] + bench_args)
        except (AssertionError,
                subprocess.TimeoutExpired) as e:  # pragma: no cover
            last = e
    raise last


def test_bench_single_process_contract():
    d = run_bench(["bench.py", "--steps", "2", "--warmup", "1",
                   "--words", "20000", "--splits", "4", "--vocab", "500",
                   "--device", "cpu"])
    assert d["metric"] == "words/sec"
    assert d["n_gpus"] == 1
    assert d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["vs_baseline"] == pytest.approx(
        d["value"] / (49_158_635 / 49.23))
    assert d["config"]["parallelism"] == "dp1"


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last timed step's delivered results as
    float .npy files, identical from run to run (same arguments -> same
    inputs), and they are the word count of the corpus; --full is
    accepted and keeps the headline line intact."""
    import numpy as np

    args = ["bench.py", "--steps", "2", "--warmup", "1",
            "--words", "20000", "--splits", "4", "--vocab", "500",
            "--device", "cpu"]
    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        out = tmp_path / name
        d = run_bench(args + ["--dump-outputs", str(out)] + extra)
        assert d["metric"] == "words/sec" and d["ms_per_step"] > 0
        assert d["steps"] == 2
        dumps.append({f[:-4]: np.load(out / f)
                      for f in sorted(os.listdir(out))})
    a, b = dumps
    assert set(a) == {"keys_hi", "keys_lo", "counts", "word_lens",
                      "word_bytes", "nwords"}
    for k in a:
        assert a[k].dtype in (np.float32, np.float64)
        assert np.array_equal(a[k], b[k]), k
    assert a["nwords"].tolist() == [20000.0]
    assert a["counts"].sum() == 20000
    n = a["counts"].size
    assert 0 < n <= 500
    assert a["keys_hi"].size == a["keys_lo"].size == a["word_lens"].size == n
    assert a["word_bytes"].size == a["word_lens"].sum()
    # the dumped words are the corpus' words with their true counts
    sys.path.insert(0, REPO)
    import collections

    from mapreduce_amd.gpu.corpus import make_corpus
    corpus = make_corpus("cpu", nwords=20000, nsplits=4, vocab_size=500,
                         seed=1234)
    exp = collections.Counter(corpus.text.numpy().tobytes().split())
    raw = a["word_bytes"].astype(np.uint8).tobytes()
    got, off = {}, 0
    for L, c in zip(a["word_lens"].astype(int), a["counts"].astype(int)):
        got[raw[off:off + L]] = int(c)
        off += L
    assert got == dict(exp)


@pytest.mark.timeout(500)
def test_bench_torchrun_ws4_contract():
    """4-rank canary for the driver's N=4/8 scaling runs."""
    d = run_torchrun_bench(4, [
        "--gpus", "4", "--steps", "2", "--warmup", "1",
        "--words", "12000", "--splits", "3", "--vocab", "400",
        "--device", "cpu"])
    assert d["n_gpus"] == 4
    assert d["config"]["global_batch"] == 48000


@pytest.mark.timeout(500)
def test_bench_torchrun_ws8_contract():
    """8-rank canary — the driver's exact N=8 scaling invocation shape
    (gloo on CPU here; RCCL on the node shares every line of code)."""
    d = run_torchrun_bench(8, [
        "--gpus", "8", "--steps", "1", "--warmup", "1",
        "--words", "6000", "--splits", "2", "--vocab", "300",
        "--device", "cpu"])
    assert d["n_gpus"] == 8
    assert d["config"]["parallelism"] == "dp8"
    assert d["config"]["global_batch"] == 48000


@pytest.mark.timeout(500)
def test_bench_torchrun_ws2_contract():
    d = run_torchrun_bench(2, [
        "--gpus", "2", "--steps", "2", "--warmup", "1",
        "--words", "20000", "--splits", "4", "--vocab", "500",
        "--device", "cpu"])
    assert d["n_gpus"] == 2
    assert d["config"]["parallelism"] == "dp2"
    # whole-job aggregate: words per step = words x world
    assert d["config"]["global_batch"] == 40000


@pytest.mark.timeout(500)
def test_bench_self_launch_gpus2():
    """`bench.py --gpus 2` with NO torchrun env must launch 2 real ranks
    itself (round 1 parsed the flag and silently measured 1 rank)."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK",
                        "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "2", "--steps", "2",
         "--warmup", "1", "--words", "20000", "--splits", "4",
         "--vocab", "500", "--device", "cpu"],
        cwd=REPO, env=dict(env, PYTHONPATH=REPO),
        capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2
    assert d["config"]["parallelism"] == "dp2"


def test_bench_world_mismatch_fails_loudly():
    """--gpus N disagreeing with an existing WORLD_SIZE must abort, not
    silently measure the wrong world."""
    env = dict(os.environ, PYTHONPATH=REPO, WORLD_SIZE="1", RANK="0",
               LOCAL_RANK="0")
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "4", "--steps", "1",
         "--warmup", "0", "--words", "2000", "--splits", "2",
         "--vocab", "100", "--device", "cpu"],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0
    assert "WORLD_SIZE" in out.stderr


@pytest.mark.timeout(500)
def test_bench_from_disk_ws2_contract():
    """--from-disk composes with multi-rank launch (per-rank corpus
    files, both timed regions bracketed by collectives)."""
    d = run_torchrun_bench(2, [
        "--gpus", "2", "--steps", "2", "--warmup", "1",
        "--words", "20000", "--splits", "4", "--vocab", "500",
        "--device", "cpu", "--from-disk"])
    assert d["n_gpus"] == 2
    assert d["config"]["ingestion"] == "streamed-from-disk"
    assert d["resident_value"] > 0
    assert d["streamed_over_resident"] > 0
