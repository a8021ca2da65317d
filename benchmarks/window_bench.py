"""Running sums within every key on one device: the segmented scan kernels
against the same contract composed from torch ops, and the job end to end,
at three shapes of 2^24 rows.

    uniform   2^20 uniform keys: segments of ~16 rows, a head in every tile
    zipf      Zipf(0.7) over 2^20 keys: the hot keys span many tiles
    few_keys  2^8 keys: every segment is longer than a tile, most tiles
              hold no head and only pass the carry on

Per shape, on the same device and the same seeded inputs (keys sorted, one
random i64 value per row):
  (a) "scan": ops.scan_by_key_sorted, i64 sum (three launches);
  (b) "torch": the same contract from torch ops: cumsum(vals) minus the
      exclusive total at each segment's head, spread over the segment with
      repeat_interleave; exact in wrapping i64;
  (c) "job": WindowJob.run(keys, order, vals).scan("sum") end to end
      (unsorted keys).
(a) and (b) are checked equal before anything is timed and all are timed
alternately; each figure is the median of device-event times.  The three
scan kernels are also timed alone.  The op moves 40 B per row (keys and
values read twice, one write); that over its time gives the achieved
bytes/s.  Needs a GPU; there is no CPU form.  Prints one JSON line."""

import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # bytes/s, MI355X specification
ROW_BYTES = 40


def zipf_keys(n, nkeys, s, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.arange(1, nkeys + 1, dtype=torch.float64).pow(-s)
    cdf = torch.cumsum(w / w.sum(), 0)
    u = torch.rand(n, generator=g, dtype=torch.float64)
    return torch.searchsorted(cdf, u).clamp(max=nkeys - 1)


def spread(ids):
    """small ints -> u64 bit patterns on both halves of the sign bit"""
    return ids * -7046029254386353131  # 0x9E3779B97F4A7C15, odd: injective


def shapes(scale):
    g = torch.Generator().manual_seed(7)
    n = (1 << 24) >> scale
    n20 = (1 << 20) >> scale
    return {
        "uniform": spread(torch.randint(0, n20, (n,), dtype=torch.int64,
                                        generator=g)),
        "zipf": spread(zipf_keys(n, n20, 0.7, 1)),
        "few_keys": spread(torch.randint(0, 1 << 8, (n,), dtype=torch.int64,
                                         generator=g)),
    }


def torch_scan(keys, vals):
    """(b): inclusive running i64 sum within runs of equal keys."""
    n = keys.numel()
    head = torch.ones(n, dtype=torch.bool, device=keys.device)
    head[1:] = keys[1:] != keys[:-1]
    heads = torch.nonzero(head).squeeze(1)
    c = torch.cumsum(vals, 0)
    base = c.index_select(0, heads) - vals.index_select(0, heads)
    lens = torch.diff(heads, append=heads.new_tensor([n]))
    return c - torch.repeat_interleave(base, lens, output_size=n)


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def med(xs):
    return round(statistics.median(xs), 4)


def main():
    if not torch.cuda.is_available():
        print("window_bench needs a GPU", file=sys.stderr)
        return 1
    from mapreduce_amd import ops
    from mapreduce_amd.gpu.window import WindowJob

    ops.require_gpu_ext()
    dev = torch.device("cuda", 0)
    reps = int(os.environ.get("WINDOW_REPS", 9))
    warm = int(os.environ.get("WINDOW_WARMUP", 2))
    scale = int(os.environ.get("WINDOW_SCALE", 0))  # rehearsal: halvings
    tile, chunk = ops.seg_scan_caps()
    result = {"metric": "scan_by_key_sorted i64 sum ms (median)",
              "unit": "ms", "higher_is_better": False, "reps": reps,
              "warmup": warm, "tile": tile, "carry_chunk": chunk,
              "row_bytes": ROW_BYTES, "hbm_peak_bytes_per_s": HBM_PEAK,
              "shapes": {}}
    e = ops.ext()
    g = torch.Generator().manual_seed(11)
    for name, raw in shapes(scale).items():
        n = raw.numel()
        raw = raw.to(dev)
        rval = torch.randint(-2 ** 62, 2 ** 62, (n,), dtype=torch.int64,
                             generator=g).to(dev)
        rord = torch.randint(0, 1 << 40, (n,), dtype=torch.int64,
                             generator=g).to(dev)
        keys, vals = ops.sort_by_key(raw, rval)
        a = ops.scan_by_key_sorted(keys, vals, "sum")
        b = torch_scan(keys, vals)
        assert torch.equal(a, b), name
        del a, b
        nseg = int(e.head_flags(keys).sum().item())
        tf, ta = e.seg_scan_reduce(keys, vals, 0, False)
        cf, ca = e.seg_scan_carry(tf, ta, 0, False)
        headless = int(((tf & 1) == 0).sum().item())
        job = WindowJob(dev)
        runs = {
            "scan": lambda: ops.scan_by_key_sorted(keys, vals, "sum"),
            "torch": lambda: torch_scan(keys, vals),
            "job": lambda: job.run(raw, rord, rval).scan("sum"),
            "reduce_kernel": lambda: e.seg_scan_reduce(keys, vals, 0, False),
            "carry_kernel": lambda: e.seg_scan_carry(tf, ta, 0, False),
            "apply_kernel": lambda: e.seg_scan_apply(keys, vals, cf, ca, 0,
                                                     False),
        }
        times = {k: [] for k in runs}
        for it in range(warm + reps):
            for k, fn in runs.items():  # alternated within the one call
                t = timed(fn)
                if it >= warm:
                    times[k].append(t)
        torch.cuda.empty_cache()
        s_ms = statistics.median(times["scan"])
        result["shapes"][name] = {
            "rows": n, "segments": nseg, "tiles": tf.numel(),
            "headless_tiles": headless,
            "scan_ms": med(times["scan"]),
            "torch_ms": med(times["torch"]),
            "scan_over_torch": round(
                s_ms / statistics.median(times["torch"]), 4),
            "job_ms": med(times["job"]),
            "reduce_kernel_ms": med(times["reduce_kernel"]),
            "carry_kernel_ms": med(times["carry_kernel"]),
            "apply_kernel_ms": med(times["apply_kernel"]),
            "scan_bytes_per_s": round(ROW_BYTES * n / (s_ms * 1e-3)),
            "scan_share_of_hbm_peak": round(
                ROW_BYTES * n / (s_ms * 1e-3) / HBM_PEAK, 4),
            "scan_ms_min_max": [round(min(times["scan"]), 4),
                                round(max(times["scan"]), 4)],
            "torch_ms_min_max": [round(min(times["torch"]), 4),
                                 round(max(times["torch"]), 4)],
        }
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
