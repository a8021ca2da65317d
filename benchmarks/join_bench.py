"""Equi-join on one device: the HIP op against the plain-torch composition
of the same contract, and the job end to end, at three shapes.

    foreign_key    2^24 left rows referencing 2^20 unique right keys
    many_to_many   Zipf(0.7) keys on both sides, 2^20 rows each, ~2^26 rows
    hot_key        2^12 left x 2^12 right rows of one key (a 2^24-row run)
                   on top of 2^20 unique keys matched 1:1

Per shape, on the same device and the same seeded inputs:
  (a) ops.join_sorted on the two sorted key columns;
  (b) the same contract in plain torch: sign flip, two searchsorted,
      cumsum, repeat_interleave, arange arithmetic;
  (c) JoinJob.run end to end (unsorted keys, one i64 value per row).
(a) and (b) are checked equal before anything is timed and are timed
alternately; each figure is the median of device-event times.  The
kernels are also timed on their own (both variants of the bounds pass; the
op runs the windowed one); the expand kernel's bytes (two i64
stores per output row; off, lo and cnt read once per left row) over its
time give the achieved bytes/s.  Needs a GPU; there is no CPU form.
Prints one JSON line."""

import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # bytes/s, MI355X specification
SIGN = -1 << 63


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
    n24, n20, n12 = (1 << 24) >> scale, (1 << 20) >> scale, (1 << 12) >> (
        scale // 2)
    out = {}
    right = torch.arange(n20, dtype=torch.int64)
    out["foreign_key"] = (
        spread(torch.randint(0, n20, (n24,), dtype=torch.int64,
                             generator=g)), spread(right))
    out["many_to_many"] = (spread(zipf_keys(n20, n20, 0.7, 1)),
                           spread(zipf_keys(n20, n20, 0.7, 2)))
    hot = torch.full((n12,), n20 + 5, dtype=torch.int64)
    side = torch.cat([right, hot])
    out["hot_key"] = (spread(side[torch.randperm(side.numel(),
                                                 generator=g)]),
                      spread(side[torch.randperm(side.numel(),
                                                 generator=g)]))
    return out


def torch_join(lk, rk):
    """(b): inner join of two u64-sorted columns in plain torch."""
    ls, rs = lk ^ SIGN, rk ^ SIGN
    lo = torch.searchsorted(rs, ls, right=False)
    cnt = torch.searchsorted(rs, ls, right=True) - lo
    ends = torch.cumsum(cnt, 0)
    total = int(ends[-1].item()) if ends.numel() else 0
    li = torch.repeat_interleave(
        torch.arange(lk.numel(), device=lk.device), cnt, output_size=total)
    ri = lo[li] + (torch.arange(total, device=lk.device) - (ends - cnt)[li])
    return li, ri


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
        print("join_bench needs a GPU", file=sys.stderr)
        return 1
    from mapreduce_amd import ops
    from mapreduce_amd.gpu.join import JoinJob

    ops.require_gpu_ext()
    dev = torch.device("cuda", 0)
    reps = int(os.environ.get("JOIN_REPS", 9))
    warm = int(os.environ.get("JOIN_WARMUP", 2))
    scale = int(os.environ.get("JOIN_SCALE", 0))  # rehearsal: halvings
    result = {"metric": "join_sorted ms (median)", "unit": "ms",
              "higher_is_better": False, "reps": reps, "warmup": warm,
              "hbm_peak_bytes_per_s": HBM_PEAK, "shapes": {}}
    for name, (lraw, rraw) in shapes(scale).items():
        lraw, rraw = lraw.to(dev), rraw.to(dev)
        lval = torch.arange(lraw.numel(), device=dev)
        rval = torch.arange(rraw.numel(), device=dev)
        (lk,) = ops.sort_by_key(lraw)
        (rk,) = ops.sort_by_key(rraw)
        a = ops.join_sorted(lk, rk)
        b = torch_join(lk, rk)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name
        total = a[0].numel()
        del a, b
        # the pieces of (a), for the kernels' own times
        lo, cnt = ops.join_bounds(lk, rk)
        off = torch.zeros(cnt.numel() + 1, dtype=torch.int64, device=dev)
        torch.cumsum(cnt, 0, out=off[1:])
        job = JoinJob(dev, how="inner")
        runs = {
            "op": lambda: ops.join_sorted(lk, rk),
            "torch": lambda: torch_join(lk, rk),
            "job": lambda: job.run(lraw, lval, rraw, rval),
            "bounds_window_kernel": lambda: ops.ext().join_bounds(lk, rk,
                                                                  True),
            "bounds_row_kernel": lambda: ops.ext().join_bounds(lk, rk,
                                                               False),
            "expand_kernel": lambda: ops.ext().join_expand(off, lo, cnt,
                                                           total),
        }
        times = {k: [] for k in runs}
        for it in range(warm + reps):
            for k, fn in runs.items():  # alternated within the one call
                t = timed(fn)
                if it >= warm:
                    times[k].append(t)
        torch.cuda.empty_cache()
        nl = lk.numel()
        expand_bytes = 16 * total + 24 * nl
        ex_ms = statistics.median(times["expand_kernel"])
        result["shapes"][name] = {
            "left_rows": nl, "right_rows": rk.numel(), "output_rows": total,
            "op_ms": med(times["op"]), "torch_ms": med(times["torch"]),
            "op_over_torch": round(statistics.median(times["op"])
                                   / statistics.median(times["torch"]), 4),
            "job_ms": med(times["job"]),
            "bounds_window_kernel_ms": med(times["bounds_window_kernel"]),
            "bounds_row_kernel_ms": med(times["bounds_row_kernel"]),
            "expand_kernel_ms": med(times["expand_kernel"]),
            "expand_bytes": expand_bytes,
            "expand_bytes_per_s": round(expand_bytes / (ex_ms * 1e-3)),
            "expand_share_of_hbm_peak": round(
                expand_bytes / (ex_ms * 1e-3) / HBM_PEAK, 4),
            "op_ms_min_max": [round(min(times["op"]), 4),
                              round(max(times["op"]), 4)],
            "torch_ms_min_max": [round(min(times["torch"]), 4),
                                 round(max(times["torch"]), 4)],
        }
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
