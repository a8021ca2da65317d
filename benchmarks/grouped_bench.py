"""Values ordered within every key on one device: the LDS tile sort plus the
straddler re-sort against the two-sort composition of the same contract,
and the job end to end, at three shapes of 2^24 rows.

    uniform   2^20 uniform keys: groups of ~16 rows, nearly all finished in
              tiles
    zipf      Zipf(0.7) over 2^20 keys: the hot keys go through the
              straddler path
    few_keys  2^8 keys: every group is longer than a tile, all rows are
              straddlers

Per shape, on the same device and the same seeded inputs (keys sorted, one
random i64 value per row):
  (a) "tile": ops.sort_values_in_groups, the default path (LDS tile sort,
      then the straddlers re-sorted);
  (b) "two_sort": the same op under MR_GROUP_TWO_SORT=1, sort by order key
      and then stably by key;
  (c) "job": GroupedValuesJob.run end to end (unsorted keys).
(a) and (b) are checked equal before anything is timed and all three are
timed alternately; each figure is the median of device-event times.  The
tile kernel is also timed on its own; its bytes (8 B segment id and 8 B
value read, 8 B written per row) over its time give the achieved bytes/s.
Needs a GPU; there is no CPU form.  Prints one JSON line."""

import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # bytes/s, MI355X specification


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
        print("grouped_bench needs a GPU", file=sys.stderr)
        return 1
    from mapreduce_amd import ops
    from mapreduce_amd.gpu.grouped import GroupedValuesJob

    ops.require_gpu_ext()
    dev = torch.device("cuda", 0)
    reps = int(os.environ.get("GROUP_REPS", 9))
    warm = int(os.environ.get("GROUP_WARMUP", 2))
    scale = int(os.environ.get("GROUP_SCALE", 0))  # rehearsal: halvings
    tile = ops.group_caps()[0]
    result = {"metric": "sort_values_in_groups ms (median)", "unit": "ms",
              "higher_is_better": False, "reps": reps, "warmup": warm,
              "tile": tile,
              "hbm_peak_bytes_per_s": HBM_PEAK, "shapes": {}}

    def two_sort(keys, vals):
        os.environ["MR_GROUP_TWO_SORT"] = "1"
        try:
            return ops.sort_values_in_groups(keys, vals)
        finally:
            del os.environ["MR_GROUP_TWO_SORT"]

    g = torch.Generator().manual_seed(11)
    for name, raw in shapes(scale).items():
        n = raw.numel()
        raw = raw.to(dev)
        rval = torch.randint(-2 ** 62, 2 ** 62, (n,), dtype=torch.int64,
                             generator=g).to(dev)
        keys, vals = ops.sort_by_key(raw, rval)
        uk, off = ops.group_by_key_sorted(keys)
        _, srows = ops.group_straddlers(off, tile)
        a = ops.sort_values_in_groups(keys, vals, off)
        b = two_sort(keys, vals)
        assert torch.equal(a, b), name
        del a, b
        seg = torch.cumsum(ops.ext().head_flags(keys), 0)
        job = GroupedValuesJob(dev)
        runs = {
            "tile": lambda: ops.sort_values_in_groups(keys, vals),
            "two_sort": lambda: two_sort(keys, vals),
            "job": lambda: job.run(raw, rval),
            "tile_kernel": lambda: ops.ext().group_tile_sort(seg, vals,
                                                             False),
        }
        times = {k: [] for k in runs}
        for it in range(warm + reps):
            for k, fn in runs.items():  # alternated within the one call
                t = timed(fn)
                if it >= warm:
                    times[k].append(t)
        torch.cuda.empty_cache()
        tk_ms = statistics.median(times["tile_kernel"])
        result["shapes"][name] = {
            "rows": n, "keys": uk.numel(), "straddler_rows": srows,
            "straddler_share": round(srows / n, 5),
            "tile_ms": med(times["tile"]),
            "two_sort_ms": med(times["two_sort"]),
            "tile_over_two_sort": round(
                statistics.median(times["tile"])
                / statistics.median(times["two_sort"]), 4),
            "job_ms": med(times["job"]),
            "tile_kernel_ms": med(times["tile_kernel"]),
            "tile_kernel_bytes_per_s": round(24 * n / (tk_ms * 1e-3)),
            "tile_kernel_share_of_hbm_peak": round(
                24 * n / (tk_ms * 1e-3) / HBM_PEAK, 4),
            "tile_ms_min_max": [round(min(times["tile"]), 4),
                                round(max(times["tile"]), 4)],
            "two_sort_ms_min_max": [round(min(times["two_sort"]), 4),
                                    round(max(times["two_sort"]), 4)],
        }
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
