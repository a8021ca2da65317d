"""As-of join on one device: the HIP op against the same contract composed
from the project's own ops, against its thread-per-row partner kernel, and
the job end to end, at three shapes.

    long_runs    2^24 x 2^24 rows over 2^12 keys (4096 rows per key a side)
    short_runs   2^24 left x 2^22 right rows over 2^20 keys (16 and 4)
    hot_key      2^24 x 2^24 rows, half of each side under ONE key, the
                 other half over 2^20 keys

Per shape, on the same device and the same seeded inputs (backward, exact
matches allowed, no tolerance):
  (a) ops.asof_sorted on the two sorted sides (asof_window_kernel);
  (b) the same contract from sort_by_key and scan_by_key_sorted: the sides
      concatenated right first, sorted by the time's order key and then
      stably by key, a running max of the right rows' indices within each
      key, read at the left rows;
  (c) asof_row_kernel, the thread-per-row partner of (a);
  (d) AsofJoinJob.run end to end (unsorted rows, one i64 value per row).
(a), (b) and (c) are checked equal before anything is timed and are timed
alternately; each figure is the median of device-event times.  The byte
model of the op, for achieved bytes/s: 16 B read per row of each side (key
and time) plus 8 B stored per left row.  ASOF_REPS (9) and ASOF_WARMUP (2)
set the timed and the warm-up repetitions per shape.  Needs a GPU; there is
no CPU form.  Prints one JSON line."""

import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # bytes/s, MI355X specification


def spread(ids):
    """small ints -> u64 bit patterns on both halves of the sign bit"""
    return ids * -7046029254386353131  # 0x9E3779B97F4A7C15, odd: injective


def shapes():
    g = torch.Generator().manual_seed(11)
    n24, n22, n20, n12 = (1 << b for b in (24, 22, 20, 12))

    def side(n, nkeys, hot=0):
        ids = torch.randint(0, nkeys, (n,), dtype=torch.int64, generator=g)
        if hot:
            ids[torch.randperm(n, generator=g)[:hot]] = nkeys + 5
        # times: seconds over ~35 years, signed
        times = torch.randint(-(1 << 29), 1 << 30, (n,), dtype=torch.int64,
                              generator=g)
        return spread(ids), times

    return {
        "long_runs": side(n24, n12) + side(n24, n12),
        "short_runs": side(n24, n20) + side(n22, n20),
        "hot_key": (side(n24, n20, n24 // 2) + side(n24, n20, n24 // 2)),
    }


def arrange(ops, keys, times):
    """one side sorted on (key, order key of the time)"""
    _, k, t = ops.sort_by_key(ops.group_order_keys(times), keys, times)
    return ops.sort_by_key(k, t)


def composed(ops, lk, lt, rk, rt):
    """(b): backward as-of join of two sorted sides from the project's ops"""
    nl, nr = lk.numel(), rk.numel()
    keys = torch.cat([rk, lk])
    okeys = torch.cat([ops.group_order_keys(rt), ops.group_order_keys(lt)])
    origin = torch.arange(nr + nl, device=lk.device)
    # right rows first and both sorts stable: among equal (key, time) the
    # right rows stay ahead of the left ones, each side in its own order
    _, keys, origin = ops.sort_by_key(okeys, keys, origin)
    keys, origin = ops.sort_by_key(keys, origin)
    idx = torch.where(origin < nr, origin, torch.full_like(origin, -1))
    run = ops.scan_by_key_sorted(keys, idx, "max")
    return torch.empty_like(run).scatter_(0, origin, run)[nr:]


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
        print("asof_bench needs a GPU", file=sys.stderr)
        return 1
    from mapreduce_amd import ops
    from mapreduce_amd.gpu.asof import AsofJoinJob

    ops.require_gpu_ext()
    dev = torch.device("cuda", 0)
    reps = int(os.environ.get("ASOF_REPS", 9))
    warm = int(os.environ.get("ASOF_WARMUP", 2))
    T, W = ops.asof_caps()
    result = {"metric": "asof_sorted ms (median)", "unit": "ms",
              "higher_is_better": False, "reps": reps, "warmup": warm,
              "hbm_peak_bytes_per_s": HBM_PEAK, "asof_tile": T,
              "asof_win": W, "shapes": {}}
    ext = ops.ext().asof_sorted
    for name, raw in shapes().items():
        lkr, ltr, rkr, rtr = (c.to(dev) for c in raw)
        lval = torch.arange(lkr.numel(), device=dev)
        rval = torch.arange(rkr.numel(), device=dev)
        lk, lt = arrange(ops, lkr, ltr)
        rk, rt = arrange(ops, rkr, rtr)
        a = ext(lk, lt, rk, rt)
        b = composed(ops, lk, lt, rk, rt)
        c = ext(lk, lt, rk, rt, row=True)
        assert torch.equal(a, b) and torch.equal(a, c), name
        matched = int((a >= 0).sum().item())
        del a, b, c
        job = AsofJoinJob(dev)
        runs = {
            "op": lambda: ext(lk, lt, rk, rt),
            "composed": lambda: composed(ops, lk, lt, rk, rt),
            "row_kernel": lambda: ext(lk, lt, rk, rt, row=True),
            "job": lambda: job.run(lkr, ltr, lval, rkr, rtr, rval),
        }
        times = {k: [] for k in runs}
        for it in range(warm + reps):
            for k, fn in runs.items():  # alternated within the one call
                t = timed(fn)
                if it >= warm:
                    times[k].append(t)
        torch.cuda.empty_cache()
        nl, nr = lk.numel(), rk.numel()
        nbytes = 16 * (nl + nr) + 8 * nl
        m = {k: statistics.median(v) for k, v in times.items()}
        result["shapes"][name] = {
            "left_rows": nl, "right_rows": nr, "matched_rows": matched,
            "op_ms": med(times["op"]),
            "composed_ms": med(times["composed"]),
            "row_kernel_ms": med(times["row_kernel"]),
            "job_ms": med(times["job"]),
            "op_over_composed": round(m["op"] / m["composed"], 4),
            "op_over_row_kernel": round(m["op"] / m["row_kernel"], 4),
            "model_bytes": nbytes,
            "op_bytes_per_s": round(nbytes / (m["op"] * 1e-3)),
            "op_share_of_hbm_peak": round(
                nbytes / (m["op"] * 1e-3) / HBM_PEAK, 4),
            "row_kernel_share_of_hbm_peak": round(
                nbytes / (m["row_kernel"] * 1e-3) / HBM_PEAK, 4),
            "op_ms_min_max": [round(min(times["op"]), 4),
                              round(max(times["op"]), 4)],
            "row_kernel_ms_min_max": [round(min(times["row_kernel"]), 4),
                                      round(max(times["row_kernel"]), 4)],
            "composed_ms_min_max": [round(min(times["composed"]), 4),
                                    round(max(times["composed"]), 4)],
        }
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
