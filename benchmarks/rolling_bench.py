"""Rolling aggregates within every key on one device: the frame kernels
against the same contracts composed from the project's own ops, the two
bounds kernels against each other, and OrderedRows.rolling end to end, at
three key shapes of 2^24 rows and two frame widths each.

    uniform   2^20 uniform keys: ~16 rows per key, no frame leaves its key
    zipf      Zipf(0.7) over 2^20 keys: the hot keys span many tiles
    few_keys  2^8 keys: 65 536 rows per key

Times are uniform i64 in [0, 2^30), values random i64.  Per shape a narrow
frame (about 8 rows: on the hottest key for zipf) and a wide one (every
earlier row of the key for uniform; thousands of rows, several reduce tiles,
on the long keys of zipf and few_keys): `preceding` ticks back, following = 0.  The measured
mean and longest frame and the share of frames that leave their reduce tile
are reported with every figure.

Per shape and width, on the same device and the same seeded inputs (rows
sorted on (key, time)):
  bounds   (a) ops.frame_bounds, row kernel;  (b) the window kernel;
           (c) composed: two ops.asof_sorted calls of the relation against
           itself, forward at t - preceding and backward at t + following;
  sum      (d) ops.frame_reduce "sum";  (e) composed: ops.scan_by_key_sorted
           and the difference of two gathers (exact for i64, which is why it
           can be checked equal; not the shipped path, see README);
  min/max  (f), (g) ops.frame_reduce; no composition exists, so the figure
           is the time and the achieved bytes/s;
  job      (h) WindowJob.run from the unsorted columns, then
           .rolling("sum", preceding).
(a) = (b) = (c) and (d) = (e) are checked before anything is timed; all are
timed alternately and each figure is the median of device-event times.
Byte models, for achieved bytes/s against the 8 TB/s HBM specification:
bounds 16 B read (key, time) + 16 B stored (lo, hi) per row; reduce 24 B read
(value, lo, hi) + 8 B stored per row, the least any implementation moves (the
three passes move more: pre and suf are written and gathered).
ROLLING_REPS (9) and ROLLING_WARMUP (2) set the timed and the warm-up
repetitions; ROLLING_SCALE=s shrinks rows and keys by 2^s for a rehearsal.
Needs a GPU; there is no CPU form.  Prints one JSON line."""

import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # bytes/s, MI355X specification
BOUNDS_BYTES = 32
REDUCE_BYTES = 32
TIME_BITS = 30


def zipf_keys(n, nkeys, s, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.arange(1, nkeys + 1, dtype=torch.float64).pow(-s)
    cdf = torch.cumsum(w / w.sum(), 0)
    u = torch.rand(n, generator=g, dtype=torch.float64)
    return torch.searchsorted(cdf, u).clamp(max=nkeys - 1)


def spread(ids):
    """small ints -> u64 bit patterns on both halves of the sign bit"""
    return ids * -7046029254386353131  # 0x9E3779B97F4A7C15, odd: injective


def shapes(scale=0):
    """name -> (keys, times, vals, narrow preceding, wide preceding)"""
    g = torch.Generator().manual_seed(13)
    n = (1 << 24) >> scale
    n20 = (1 << 20) >> scale
    full = 1 << TIME_BITS

    def cols(ids):
        times = torch.randint(0, full, (n,), dtype=torch.int64, generator=g)
        vals = torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), dtype=torch.int64,
                             generator=g)
        return spread(ids), times, vals

    return {
        "uniform": cols(torch.randint(0, n20, (n,), dtype=torch.int64,
                                      generator=g)) + (full >> 1, full),
        "zipf": cols(zipf_keys(n, n20, 0.7, 1)) + (full >> 13, full >> 3),
        "few_keys": cols(torch.randint(0, 1 << 8, (n,), dtype=torch.int64,
                                       generator=g))
        + ((full >> 13) << scale, full >> 3),
    }


def composed_bounds(ops, keys, times, pre, fol):
    """(c): P(k, t - pre) is the forward match of (k, t - pre), Q(k, t +
    fol) - 1 the backward match of (k, t + fol); row i itself qualifies for
    both, so neither is ever -1.  No saturation: the times are small."""
    lo = ops.asof_sorted(keys, times - pre, keys, times, "forward")
    hi = ops.asof_sorted(keys, times + fol, keys, times, "backward") + 1
    return lo, hi


def composed_sum(ops, keys, vals, lo, hi):
    """(e): the running sum of the key at the frame's last row minus the one
    in front of its first row"""
    run = ops.scan_by_key_sorted(keys, vals, "sum")
    return (run.index_select(0, hi - 1) - run.index_select(0, lo)
            + vals.index_select(0, lo))


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(ops, dev, raw, pre, reps, warm, clock=timed):
    from mapreduce_amd.gpu.window import WindowJob

    rk, rt, rv = (c.to(dev) for c in raw)
    R = ops.frame_caps()[2]
    # sorted on (key, time); the values ride along
    _, k, t, v = ops.sort_by_key(ops.group_order_keys(rt), rk, rt, rv)
    k, t, v = ops.sort_by_key(k, t, v)
    n = k.numel()
    fb = ops.ext().frame_bounds if dev.type == "cuda" else None

    def bounds(row):
        if fb is None:
            return ops.frame_bounds(k, t, pre, 0)
        return fb(k, t, pre, 0, row)

    lo, hi = bounds(True)
    for other in (bounds(False), composed_bounds(ops, k, t, pre, 0)):
        assert torch.equal(lo, other[0]) and torch.equal(hi, other[1])
    assert torch.equal(ops.frame_reduce(v, lo, hi, "sum"),
                       composed_sum(ops, k, v, lo, hi))
    rows = (hi - lo)
    info = {
        "rows": n, "preceding": pre,
        "frame_rows_mean": round(rows.double().mean().item(), 2),
        "frame_rows_max": int(rows.max().item()),
        "frames_leaving_their_tile": round(
            (lo // R != (hi - 1) // R).double().mean().item(), 4),
    }
    job = WindowJob(dev)
    runs = {
        "bounds_row": lambda: bounds(True),
        "bounds_window": lambda: bounds(False),
        "bounds_composed": lambda: composed_bounds(ops, k, t, pre, 0),
        "sum": lambda: ops.frame_reduce(v, lo, hi, "sum"),
        "sum_composed": lambda: composed_sum(ops, k, v, lo, hi),
        "min": lambda: ops.frame_reduce(v, lo, hi, "min"),
        "max": lambda: ops.frame_reduce(v, lo, hi, "max"),
        "job": lambda: job.run(rk, rt, rv).rolling("sum", pre),
    }
    times = {name: [] for name in runs}
    for it in range(warm + reps):
        for name, fn in runs.items():  # alternated within the one call
            ms = clock(fn)
            if it >= warm:
                times[name].append(ms)
    m = {name: statistics.median(x) for name, x in times.items()}
    for name, x in times.items():
        info[name + "_ms"] = round(m[name], 4)
        info[name + "_ms_min_max"] = [round(min(x), 4), round(max(x), 4)]
    info["bounds_row_over_window"] = round(
        m["bounds_row"] / m["bounds_window"], 4)
    info["bounds_row_over_composed"] = round(
        m["bounds_row"] / m["bounds_composed"], 4)
    info["bounds_window_over_composed"] = round(
        m["bounds_window"] / m["bounds_composed"], 4)
    info["sum_over_composed"] = round(m["sum"] / m["sum_composed"], 4)
    for name, per_row in (("bounds_row", BOUNDS_BYTES),
                          ("bounds_window", BOUNDS_BYTES),
                          ("sum", REDUCE_BYTES), ("min", REDUCE_BYTES),
                          ("max", REDUCE_BYTES)):
        rate = per_row * n / (m[name] * 1e-3)
        info[name + "_bytes_per_s"] = round(rate)
        info[name + "_share_of_hbm_peak"] = round(rate / HBM_PEAK, 4)
    return info


def main():
    if not torch.cuda.is_available():
        print("rolling_bench needs a GPU", file=sys.stderr)
        return 1
    from mapreduce_amd import ops

    ops.require_gpu_ext()
    dev = torch.device("cuda", 0)
    reps = int(os.environ.get("ROLLING_REPS", 9))
    warm = int(os.environ.get("ROLLING_WARMUP", 2))
    scale = int(os.environ.get("ROLLING_SCALE", 0))
    T, W, R = ops.frame_caps()
    result = {"metric": "frame_bounds / frame_reduce ms (median)",
              "unit": "ms", "higher_is_better": False, "reps": reps,
              "warmup": warm, "scale": scale,
              "hbm_peak_bytes_per_s": HBM_PEAK, "frame_tile": T,
              "frame_win": W, "frame_rtile": R,
              "bounds_model_bytes_per_row": BOUNDS_BYTES,
              "reduce_model_bytes_per_row": REDUCE_BYTES, "shapes": {}}
    for name, (keys, times, vals, narrow, wide) in shapes(scale).items():
        for width, pre in (("narrow", narrow), ("wide", wide)):
            result["shapes"][f"{name}_{width}"] = measure(
                ops, dev, (keys, times, vals), pre, reps, warm)
            torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
