"""Flagship benchmark: Europarl-shape word count on MI355X.

Measures the BASELINE.json headline metric — words/sec, whole-job wall
clock — on synthetic text of the named shape (49,158,635 words, 197 splits
per GPU; weak scaling: each rank owns one Europarl-size corpus).

  python bench.py --gpus 1 --steps 20 --warmup 5
  python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 \
      --master-addr 127.0.0.1 bench.py --gpus 8 ...

One step = one complete MapReduce job over the corpus: fused
tokenize+combine kernels, unique extraction + radix sort, RCCL all-to-all
shuffle, sort+segmented reduce, per-rank sorted results materialized
(counts ready for the finalfn boundary).  Back-to-back steps run under
the depth-2 two-stream job pipeline (gpu/pipeline.py) by default — every
job still executes completely and exactly one job's work falls in each
timed step (steady state); MR_PIPELINE=0 forces sequential steps.
Reference headline to beat: 49.23 s / ~1.0 M words/s on 4 CPU workers
(BASELINE.md).

A plain run does only what the headline figure needs: set up, warm up,
time --steps steps, optionally --dump-outputs, print one JSON line.
Secondary measurements belong behind --full (off by default); today the
benchmark has none that run unasked (--from-disk and --timing are
explicit options), so --full adds nothing to a plain run.
"""

from __future__ import annotations

import argparse
import json
import sys
import time

import torch

BASELINE_WORDS_PER_SEC = 49_158_635 / 49.23  # BASELINE.md README.md:73

# --dump-outputs: total size ceiling, shared evenly by the arrays written
DUMP_BUDGET_BYTES = 60 << 20
DUMP_SAMPLE_SEED = 20240229


def _capped(arr, max_bytes):
    """`arr` itself when it fits in max_bytes, else a fixed seeded sample
    of its elements (same indices every run for the same length)."""
    import numpy as np

    k = max_bytes // arr.itemsize
    if arr.size <= k:
        return arr
    rng = np.random.default_rng(DUMP_SAMPLE_SEED)
    idx = np.unique(rng.integers(0, arr.size, size=k))
    return arr[idx]


def dump_outputs(res, out_dir, rank=0, world=1):
    """Write what the timed path's last step delivered — the arrays
    WordCountResult.materialize() hands a caller (hash-ordered keys,
    counts, exemplar word lengths, packed exemplar bytes) plus the job's
    word total — as <name>.npy (rank 0 / single rank) or
    <name>_rank<r>.npy.  u64 hash keys are split into exact 32-bit halves
    (keys_hi, keys_lo) because float64 holds 53 bits; counts/lens are
    exact in float64; word bytes go out as float32."""
    import os

    import numpy as np

    keys, counts, lens, blob = res.materialize(blocking=True)
    ku = keys.numpy().view(np.uint64)
    arrays = {
        "keys_hi": (ku >> np.uint64(32)).astype(np.float64),
        "keys_lo": (ku & np.uint64(0xFFFFFFFF)).astype(np.float64),
        "counts": counts.numpy().astype(np.float64),
        "word_lens": lens.numpy().astype(np.float64),
        "word_bytes": blob.numpy().astype(np.float32),
        "nwords": np.array([res.nwords], dtype=np.float64),
    }
    os.makedirs(out_dir, exist_ok=True)
    suffix = "" if world == 1 else f"_rank{rank}"
    per = DUMP_BUDGET_BYTES // len(arrays)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"),
                _capped(np.ascontiguousarray(a), per))


def _self_launch(n: int) -> int:
    """`bench.py --gpus N` run directly (no torchrun env): re-exec under
    torch.distributed.run with one rank per GPU so the flag is real —
    round-1 parsed it and silently measured 1 rank."""
    import os
    import socket
    import subprocess

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run",
           "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr=127.0.0.1", f"--master-port={port}",
           os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    # defaults give a ~1 s timed window (~1.6 ms/step on MI355X) so SMI
    # utilization sampling and box-to-box variance are meaningful
    # (VERDICT r1 "weak #3"); still finishes in seconds
    p.add_argument("--steps", type=int, default=600)
    p.add_argument("--warmup", type=int, default=50)
    p.add_argument("--words", type=int, default=49_158_635,
                   help="words per GPU (Europarl v7 English size)")
    p.add_argument("--splits", type=int, default=197)
    p.add_argument("--vocab", type=int, default=130_000)
    p.add_argument("--device", default=None)
    p.add_argument("--mode", default="auto",
                   choices=["auto", "streaming", "fused"])
    p.add_argument("--from-disk", action="store_true",
                   help="include ingestion in the timed job: each step "
                        "re-stages the corpus from a file (page cache -> "
                        "registered-DMA H2D overlapped with tokenize); "
                        "reports the resident number alongside")
    p.add_argument("--disk-chunks", type=int, default=8)
    p.add_argument("--uncoordinated", action="store_true",
                   help="bypass the control plane (engine-only timing)")
    p.add_argument("--timing", action="store_true",
                   help="print per-phase HIP-event times to stderr")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write the last timed "
                        "step's delivered results as DIR/<name>.npy")
    p.add_argument("--full", action="store_true",
                   help="also run the secondary measurements (none today: "
                        "a plain run already measures only the headline)")
    args = p.parse_args()

    import os
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return _self_launch(args.gpus)

    from mapreduce_amd import ops
    from mapreduce_amd.gpu import dist as dx
    from mapreduce_amd.gpu.corpus import make_corpus
    from mapreduce_amd.gpu.wordcount import WordCountJob

    rank, world, device = dx.init_from_env(args.device)
    assert world == args.gpus, (
        f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with "
        f"torchrun --nproc-per-node {args.gpus} (or drop WORLD_SIZE to "
        "let bench.py self-launch)")
    if device.type == "cuda":
        ops.require_gpu_ext()  # HIP kernels are mandatory on GPU

    corpus = make_corpus(device, nwords=args.words, nsplits=args.splits,
                         vocab_size=args.vocab, seed=1234 + rank)
    splits = corpus.splits()
    vocab_est = max(args.vocab, 1 << 12)
    # depth-2 job pipeline (default): job k+1's tokenize is issued before
    # job k's drain sync, hiding the host gaps (spill-count D2H, control
    # plane, launch latency) behind queued device work.  Steady state:
    # exactly one full job of work per timed step (the warmup lookahead
    # that precedes t0 is balanced by the in-flight lookahead the closing
    # synchronize waits for).  MR_PIPELINE=0 (or --timing, which needs
    # per-phase events of a single instance) restores sequential steps.
    import os
    use_pipe = os.environ.get("MR_PIPELINE", "1") != "0" and not args.timing
    if use_pipe and device.type == "cuda":
        # two engine instances double the spill allocation (~8 bytes per
        # corpus byte each); at giant corpora that exceeds HBM — fall
        # back to sequential (measured: 64x Europarl = 19.6 GB corpus,
        # 2 x 157 GB spill > 288 GB)
        n = corpus.text.numel()
        total = torch.cuda.get_device_properties(device).total_memory
        if n + 2 * 8.2 * n > 0.85 * total:
            use_pipe = False
    job = WordCountJob(device, vocab_estimate=vocab_est,
                       mode=args.mode, timing=args.timing)
    pipe = None
    runner = None
    if use_pipe:
        from mapreduce_amd.gpu.pipeline import PipelinedWordCount

        pipe = PipelinedWordCount(device, vocab_estimate=vocab_est,
                                  mode=args.mode,
                                  use_runner=not args.uncoordinated)
    elif not args.uncoordinated:
        from mapreduce_amd.gpu.runner import GpuClusterRunner

        runner = GpuClusterRunner(job, claim_mode="batch")

    def sync():
        if device.type == "cuda":
            torch.cuda.synchronize(device)

    def one_step():
        # full-framework step: map jobs tracked + claimed through the
        # control plane, engine executes, collective shuffle+reduce;
        # results land in host memory every step (C7/C8) — non-blocking
        # D2H overlaps the next job, and the timing bracket's synchronize
        # guarantees completion before the clock stops.  The pipelined
        # driver delivers internally (on the producing stream — a
        # default-stream materialize of side-stream tensors measured
        # 20x slower).
        if pipe is not None:
            return pipe.step(corpus.text, splits)
        if runner is not None:
            res = runner.run(corpus.text, splits)
        else:
            res = job.run(corpus.text, splits)
        res.materialize(blocking=False)
        return res

    # --from-disk: the timed job includes INGESTION — every step
    # re-stages the corpus bytes from a file through the OS page cache
    # into HBM (RegisteredFile: mmap + hipHostRegister once, then
    # chunked DMA overlapped with the tokenize launches), matching what
    # the reference's 49.23 s actually contains (197 GridFS file reads,
    # server.lua:348-385).  The resident number is measured first and
    # reported alongside.
    # Shape: double-buffered whole-corpus staging — job k+1's PCIe DMA
    # (one big copy from the hipHostRegistered page-cache pages, measured
    # 57.4 GB/s = link speed) runs on the side stream while job k
    # computes, so the steady-state step cadence is max(PCIe copy,
    # compute) ~= the host-link floor.  Per-chunk tokenize overlap was
    # measured WORSE: each extra map_split launch multiplies the spill
    # allocator's padded chunk tails (finish_map 0.6 -> 4.2 ms at 8
    # launches, benchmarks/fromdisk_probe.py).
    stream_ctx = None
    if args.from_disk:
        import os as _os
        import tempfile

        d = tempfile.mkdtemp(prefix="mr_bench_corpus_")
        path = _os.path.join(d, f"corpus_r{rank}.txt")
        with open(path, "wb") as fh:
            fh.write(corpus.text.cpu().numpy().tobytes())
        from mapreduce_amd.gpu.input import RegisteredFile

        rf = RegisteredFile(path, device, nchunks=args.disk_chunks)
        bufs = [rf.dtext, torch.empty_like(rf.dtext)]
        stream_ctx = {"rf": rf, "bufs": bufs, "stage_ev": [None, None],
                      "done_ev": [None, None], "i": 0, "primed": False}

    def one_step_disk():
        sc = stream_ctx
        rf = sc["rf"]
        i = sc["i"]
        sc["i"] += 1
        b = i & 1
        cur = (torch.cuda.current_stream(device)
               if device.type == "cuda" else None)
        if not sc["primed"]:
            # prologue: stage this buffer now, next buffer right after
            _, sc["stage_ev"][b] = rf.stage_async(sc["bufs"][b])
            _, sc["stage_ev"][1 - b] = rf.stage_async(sc["bufs"][1 - b])
            sc["primed"] = True
        if cur is not None and sc["stage_ev"][b] is not None:
            cur.wait_event(sc["stage_ev"][b])
        sc["stage_ev"][b] = None
        job.begin_map(sc["bufs"][b])
        job.map_split(splits[0][0], splits[-1][1])
        nwords = job.finish_map()
        res = job.shuffle_reduce(nwords)
        res.materialize(blocking=False)
        if cur is not None:
            done = torch.cuda.Event()
            done.record(cur)
        else:
            done = None
        # prefetch: re-stage THIS buffer for step i+2, after its last
        # reader (this step's queued kernels/D2H)
        _, sc["stage_ev"][b] = rf.stage_async(sc["bufs"][b],
                                              after_event=done)
        return res

    # warmup (untimed)
    res = None
    for _ in range(args.warmup):
        res = one_step()
    sync()
    dx.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = one_step()
    sync()
    dx.barrier()
    sync()
    elapsed = time.perf_counter() - t0

    streamed_elapsed = None
    if args.from_disk:
        if pipe is not None:
            pipe.flush()  # no lookahead crosses into the streamed timing
        for _ in range(max(2, args.warmup // 4)):
            res = one_step_disk()
        sync()
        dx.barrier()
        sync()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            res = one_step_disk()
        sync()
        dx.barrier()
        sync()
        streamed_elapsed = time.perf_counter() - t1

    # MAX over ranks (the slowest rank defines job wall-clock)
    el_t = torch.tensor([elapsed, streamed_elapsed or 0.0],
                        dtype=torch.float64,
                        device=device if device.type == "cuda" else "cpu")
    if world > 1:
        import torch.distributed as td
        td.all_reduce(el_t, op=td.ReduceOp.MAX)
    elapsed = float(el_t[0].item())
    if streamed_elapsed is not None:
        streamed_elapsed = float(el_t[1].item())

    total_words_per_step = args.words * world
    assert res is not None and res.nwords == args.words, \
        f"word count mismatch: {res.nwords} != {args.words}"
    if args.dump_outputs:
        dump_outputs(res, args.dump_outputs, rank=rank, world=world)
    resident_value = total_words_per_step * args.steps / elapsed
    if streamed_elapsed is not None:
        # the headline becomes the ingestion-inclusive number; the
        # resident number rides along for comparison
        value = total_words_per_step * args.steps / streamed_elapsed
        ms_per_step = streamed_elapsed / args.steps * 1000.0
    else:
        value = resident_value
        ms_per_step = elapsed / args.steps * 1000.0

    if args.timing and job.last_phase_ms:
        print(f"[rank {rank}] phase_ms: "
              + " ".join(f"{k}={v:.3f}" for k, v in
                         job.last_phase_ms.items()),
              file=sys.stderr, flush=True)
    if rank == 0:
        out = {
            "metric": "words/sec",
            "metric_detail": "words/sec (whole node) Europarl word-count "
                             "at N MI355X; job wall-clock (BASELINE.json)",
            "value": value,
            "unit": "words/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": value / BASELINE_WORDS_PER_SEC,
            "dtype": "u8-text/i64-counts",
            "data": ("synthetic (Europarl v7 shape: 49,158,635 words x N "
                     "GPUs, 197 splits/GPU, Zipf vocab 130k)"
                     + (", streamed from disk each step (page-cache DMA)"
                        if args.from_disk else "")),
            "config": {
                "model": "europarl-wordcount",
                "global_batch": total_words_per_step,
                "seq_len": args.words,
                "parallelism": f"dp{world}",
                "splits_per_gpu": args.splits,
                "partitions": world,
                "partitioner": "hash-mulhi",
                "ingestion": ("streamed-from-disk" if args.from_disk
                              else "resident-hbm"),
            },
        }
        if args.from_disk:
            out["resident_value"] = resident_value
            out["streamed_over_resident"] = (
                streamed_elapsed / (elapsed or 1e-12))
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
