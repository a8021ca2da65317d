"""Resident-graph propagation on one device: ops.graph_propagate against the
same contract composed from the project's own ops, one full PageRank, and
the build of the resident graph, at three shapes of 2^20 nodes and 2^24
edges.

    uniform  both endpoints uniform: in-degrees near 16
    zipf     Zipf(0.9) destinations: the hot rows span many tiles (the
             maximum in-degree is reported)
    hub      one node receives half of all edges, the rest are uniform

Sources are uniform in all three; x is random f64.  Per shape, on the same
device and the same seeded inputs (the CSR GraphJob.run builds):
  (a) ops.graph_propagate f64 "sum";
  (b) composed: x.index_select(0, src), ops.reduce_by_key_sorted on the
      sorted destination column (kept resident, like the CSR), a scatter of
      the rows that have edges into the dense vector;
  (c) ops.pagerank_update against (d) the same update as plain torch ops;
  (e) Graph.pagerank(iters=20, tol=0) and (f) the same with a tol that is
      never met, which adds one 8-byte readback per iteration;
  (g) GraphJob.run from the unsorted columns.
The i64 sums of (a) and (b) are checked equal and the f64 ones close before
anything is timed; (a) is checked to return the same bits twice.  All are
timed alternately and each figure is the median of device-event times (the
jobs, which synchronise, by a host clock around a device synchronise).
Byte model for (a), against the 8 TB/s HBM specification: 4 B of src and
8 B gathered per edge, 16 B per node (offsets read, out stored), the least
any implementation moves when every gather misses.
GRAPH_REPS (9) and GRAPH_WARMUP (2) set the timed and the warm-up
repetitions; GRAPH_SCALE=s shrinks nodes and edges by 2^s for a rehearsal.
Needs a GPU; there is no CPU form.  Prints one JSON line."""

import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # bytes/s, MI355X specification
EDGE_BYTES = 12
NODE_BYTES = 16
PR_ITERS = 20


def zipf_ids(m, n, s, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.arange(1, n + 1, dtype=torch.float64).pow(-s)
    cdf = torch.cumsum(w / w.sum(), 0)
    u = torch.rand(m, generator=g, dtype=torch.float64)
    ids = torch.searchsorted(cdf, u).clamp(max=n - 1)
    # the hot destinations spread over the id range (n is a power of two
    # and the factor odd, so this permutes the ids)
    return (ids * 40503) % n


def spread(ids):
    """small ints -> u64 bit patterns on both halves of the sign bit"""
    return ids * -7046029254386353131  # 0x9E3779B97F4A7C15, odd: injective


def shapes(scale=0):
    """name -> (src_keys, dst_keys)"""
    g = torch.Generator().manual_seed(17)
    n = (1 << 20) >> scale
    m = (1 << 24) >> scale

    def uni():
        return torch.randint(0, n, (m,), dtype=torch.int64, generator=g)

    hub = uni()
    hub[torch.randperm(m, generator=g)[:m // 2]] = n // 3
    return {"uniform": (spread(uni()), spread(uni())),
            "zipf": (spread(uni()), spread(zipf_ids(m, n, 0.9, 3))),
            "hub": (spread(uni()), spread(hub))}


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def torch_update(sums, old, inv_out, damping, dangling):
    """(d): pagerank_update as plain torch ops"""
    n = sums.numel()
    new = (1.0 - damping) / n + damping * (sums + dangling / n)
    contrib = new * inv_out
    delta = (new - old).abs().sum()
    held = torch.where(inv_out == 0, new, torch.zeros_like(new)).sum()
    return new, contrib, torch.stack([delta, held]).reshape(1, 2)


def measure(ops, dev, raw, reps, warm, clock=timed, host_clock=host_timed):
    from mapreduce_amd.gpu.graph import GraphJob

    sk, dk = (c.to(dev) for c in raw)
    job = GraphJob(dev)
    g = job.run(sk, dk)
    n, m = g.n, g.m
    deg = g.offsets[1:] - g.offsets[:-1]
    dst = torch.repeat_interleave(torch.arange(n, device=dev), deg,
                                  output_size=m)
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(n, generator=gen, dtype=torch.float64).to(dev)
    xi = torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), dtype=torch.int64,
                       generator=gen).to(dev)
    composed = ops._graph_propagate_composed
    for op in ("sum", "min", "max"):
        assert torch.equal(ops.graph_propagate(g.offsets, g.src, xi, op),
                           composed(g.offsets, g.src, xi, op, dst))
    a = ops.graph_propagate(g.offsets, g.src, x, "sum")
    assert torch.equal(a.view(torch.int64), ops.graph_propagate(
        g.offsets, g.src, x, "sum").view(torch.int64))
    b = composed(g.offsets, g.src, x, "sum", dst)
    # non-negative terms: each sum errs by at most deg * 2^-53 of itself
    assert bool(((a - b).abs() <= deg.double() * 2.0 ** -52 * a).all())
    dang = torch.tensor(0.1, dtype=torch.float64, device=dev)
    old = torch.full_like(x, 1.0 / n)
    u = ops.pagerank_update(a / n, old, g.inv_out, 0.85, dang)
    w = torch_update(a / n, old, g.inv_out, 0.85, dang)
    assert torch.allclose(u[0], w[0], rtol=1e-14, atol=0)
    assert torch.allclose(u[2].sum(0), w[2].sum(0), rtol=1e-9, atol=0)
    info = {"nodes": n, "edges": m, "max_in_degree": int(deg.max().item()),
            "empty_rows": int((deg == 0).sum().item()),
            "tiles": -(-m // ops.graph_caps()[0])}
    runs = {
        "propagate": lambda: ops.graph_propagate(g.offsets, g.src, x, "sum"),
        "composed": lambda: composed(g.offsets, g.src, x, "sum", dst),
        "propagate_i64_min": lambda: ops.graph_propagate(
            g.offsets, g.src, xi, "min"),
        "update": lambda: ops.pagerank_update(a, old, g.inv_out, 0.85, dang),
        "update_torch": lambda: torch_update(a, old, g.inv_out, 0.85, dang),
    }
    jobs = {
        "pagerank20": lambda: g.pagerank(0.85, PR_ITERS, 0.0),
        "pagerank20_tol": lambda: g.pagerank(0.85, PR_ITERS, 1e-300),
        "build": lambda: job.run(sk, dk),
    }
    times = {name: [] for name in list(runs) + list(jobs)}
    for it in range(warm + reps):
        for name, fn in runs.items():  # alternated within the one call
            ms = clock(fn)
            if it >= warm:
                times[name].append(ms)
        for name, fn in jobs.items():
            ms = host_clock(fn)
            if it >= warm:
                times[name].append(ms)
    med = {name: statistics.median(t) for name, t in times.items()}
    for name, t in times.items():
        info[name + "_ms"] = round(med[name], 4)
        info[name + "_ms_min_max"] = [round(min(t), 4), round(max(t), 4)]
    info["propagate_over_composed"] = round(
        med["propagate"] / med["composed"], 4)
    info["update_over_torch"] = round(med["update"] / med["update_torch"], 4)
    info["tol_readback_ms_per_iteration"] = round(
        (med["pagerank20_tol"] - med["pagerank20"]) / PR_ITERS, 4)
    model = EDGE_BYTES * m + NODE_BYTES * n
    for name in ("propagate", "propagate_i64_min"):
        rate = model / (med[name] * 1e-3)
        info[name + "_bytes_per_s"] = round(rate)
        info[name + "_share_of_hbm_peak"] = round(rate / HBM_PEAK, 4)
    return info


def main():
    if not torch.cuda.is_available():
        print("graph_bench needs a GPU", file=sys.stderr)
        return 1
    from mapreduce_amd import ops

    ops.require_gpu_ext()
    dev = torch.device("cuda", 0)
    reps = int(os.environ.get("GRAPH_REPS", 9))
    warm = int(os.environ.get("GRAPH_WARMUP", 2))
    scale = int(os.environ.get("GRAPH_SCALE", 0))
    result = {"metric": "graph_propagate f64 sum ms (median)", "unit": "ms",
              "higher_is_better": False, "reps": reps, "warmup": warm,
              "scale": scale, "hbm_peak_bytes_per_s": HBM_PEAK,
              "graph_tile": ops.graph_caps()[0],
              "model_bytes_per_edge": EDGE_BYTES,
              "model_bytes_per_node": NODE_BYTES, "shapes": {}}
    for name, raw in shapes(scale).items():
        result["shapes"][name] = measure(ops, dev, raw, reps, warm)
        torch.cuda.empty_cache()
    s = result["shapes"]
    result["hub_over_uniform"] = round(
        s["hub"]["propagate_ms"] / s["uniform"]["propagate_ms"], 4)
    result["zipf_over_uniform"] = round(
        s["zipf"]["propagate_ms"] / s["uniform"]["propagate_ms"], 4)
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
