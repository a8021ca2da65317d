"""Cases and oracles shared by the graph tests (no torch device use: the
CPU suite checks the generators, the GPU suite runs them on the device).

Kernel cases are CSRs by destination, sized by E, the edges per tile of
ops/hip/graph.hip: (offsets int64[n + 1], src int32[m]).  Job cases are edge
lists over arbitrary i64 keys.  The oracles are plain Python: ints modulo
2^64, math.fsum, dicts, union-find."""

import math
import random

import numpy as np

M64 = (1 << 64) - 1
I64_MAX = (1 << 63) - 1
I64_MIN = -(1 << 63)
IDENT = {"sum": 0, "min": I64_MAX, "max": I64_MIN}


def _signed(u):
    return u - (1 << 64) if u >> 63 else u


def _csr(degrees, seed):
    """degrees -> (offsets, src): sources seeded in [0, n), the first and
    the last edge pinned to 0 and n - 1, each row's sources ascending (the
    order GraphJob builds)."""
    n = len(degrees)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.asarray(degrees, dtype=np.int64), out=off[1:])
    m = int(off[-1])
    rng = np.random.default_rng(seed)
    src = rng.integers(0, max(n, 1), size=m).astype(np.int32)
    if m:
        src[0] = 0
        src[-1] = n - 1
    for v in range(n):
        a, b = off[v], off[v + 1]
        if b - a > 1:
            src[a:b].sort()
    if m > 1:  # the pins survive the sort of their rows
        assert src.min() == 0 and src.max() == n - 1
    return off, src


def _degrees_to(m, rng, top=12):
    """Seeded degrees in [0, top] that sum to exactly m."""
    deg = []
    left = m
    while left:
        d = min(rng.randrange(top + 1), left)
        deg.append(d)
        left -= d
    deg += [0, 0]
    return deg or [0]


def kernel_cases(E):
    """name -> (offsets, src).  Sizes, a hub across tiles in three
    alignments, runs of empty rows, rows of one edge, a mix."""
    rng = random.Random(1234)
    cases = {}
    for m in (0, 1, 63, 64, 65, E - 1, E, E + 1, 3 * E + 17):
        cases[f"m{m}"] = _csr(_degrees_to(m, rng), 100 + m)
    cases["n1_selfloops"] = _csr([5], 1)
    cases["n0"] = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32))
    hub = 5 * E + 3
    # hub between short rows: mid-tile, its first edge on a tile start, its
    # last edge on a tile end
    for name, before in (("hub_mid", 100), ("hub_head_on_tile", E),
                         ("hub_tail_on_tile", E - 3)):
        lead = [3] * (before // 3) + ([before % 3] if before % 3 else [])
        cases[name] = _csr(lead + [hub] + [2, 0, 5, 1, 4] * 7, 200 + before)
    # n = 40 E rows, m = E + 1 edges: leading, trailing and interior runs of
    # empty rows, one of them 31 E rows long
    n = 40 * E
    rows = sorted(rng.sample(range(1000, 5 * E), 300)
                  + rng.sample(range(36 * E, n - 1000), 300))
    deg = [0] * n
    for r in rows:
        deg[r] = 1
    left = E + 1 - len(rows)
    while left:
        deg[rng.choice(rows)] += 1
        left -= 1
    cases["empties"] = _csr(deg, 300)
    cases["singles"] = _csr([1] * (2 * E + 5), 400)
    deg = []
    while sum(deg) < 5 * E:
        deg.append(0 if rng.random() < 0.2 else rng.randrange(401))
    deg.insert(rng.randrange(len(deg)), 3 * E)
    cases["mixed"] = _csr(deg, 500)
    return cases


def check_case(off, src):
    n = len(off) - 1
    assert off[0] == 0 and off[-1] == len(src) and (np.diff(off) >= 0).all()
    if len(src):
        assert 0 <= src.min() and src.max() < n


# ------------------------------------------------------------------- values

def values_i64(n):
    """Distinct per node and large: row sums wrap."""
    return np.array([_signed(((v + 1) * 0x9E3779B97F4A7C15) & M64)
                     for v in range(n)], dtype=np.int64)


def values_dyadic(n, seed):
    """Multiples of 2^-20 below 2^10: any sum of fewer than 2^22 of them is
    below 2^32 and exact in f64 in every association."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 30, size=n).astype(np.float64) / (1 << 20)


def values_general(n, seed):
    """Both signs over twelve decades, so sums cancel."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, size=n)


def propagate_oracle(off, src, x, op):
    """The exact answer as a list of Python numbers: i64 sums modulo 2^64
    (signed), f64 sums by math.fsum, min / max of the gathered values.  A
    src outside [0, n) contributes the identity."""
    n = len(off) - 1
    f64 = np.asarray(x).dtype == np.float64
    xs = np.asarray(x).tolist()
    ss = np.asarray(src).tolist()
    o = np.asarray(off).tolist()
    ident = 0.0 if f64 else IDENT[op]
    out = []
    for v in range(n):
        g = [xs[s] if 0 <= s < n else ident for s in ss[o[v]:o[v + 1]]]
        if not g:
            out.append(ident)
        elif op == "sum" and f64:
            out.append(math.fsum(g) if all(map(math.isfinite, g))
                       else float(np.sum(np.array(g))))
        elif op == "sum":
            out.append(_signed(sum(g) & M64))
        else:
            out.append(min(g) if op == "min" else max(g))
    return out


def row_abs_sums(off, src, x):
    """Per row (degree, sum |x[src]|), for the f64 error bound."""
    ax = np.abs(np.asarray(x))
    o = np.asarray(off).tolist()
    return [(o[v + 1] - o[v], math.fsum(ax[src[o[v]:o[v + 1]]].tolist()))
            for v in range(len(o) - 1)]


# ----------------------------------------------------------------- job cases

def u64_order(k):
    return k & M64


def multigraph(seed, n, m, keyed=True):
    """(src_keys, dst_keys) as lists: a seeded multigraph with a hub (a
    third of the edges point to it), dangling nodes, source-only nodes,
    parallel edges and self-loops; keyed=True maps the nodes to distinct
    i64 keys of both signs."""
    rng = random.Random(seed)
    tenth = max(n // 10, 1)
    sink0, quiet0 = n - tenth, n - 2 * tenth
    edges = []
    for _ in range(m):
        s = rng.randrange(sink0)
        r = rng.random()
        if r < 0.33:
            d = 0
        elif r < 0.38:
            d = s
        elif r < 0.45 and edges:
            s, d = rng.choice(edges)
        else:
            d = rng.randrange(n - tenth)
            if d >= quiet0:
                d += tenth
        edges.append((s, d))
    if keyed:
        keys = rng.sample(range(-(1 << 61), 1 << 61), n)
        edges = [(keys[s], keys[d]) for s, d in edges]
    return [s for s, _ in edges], [d for _, d in edges]


def graph_features(src, dst):
    """What the PageRank cases must contain."""
    nodes = set(src) | set(dst)
    srcs, dsts = set(src), set(dst)
    pairs = list(zip(src, dst))
    indeg = {}
    for d in dst:
        indeg[d] = indeg.get(d, 0) + 1
    return {"dangling": len(nodes - srcs), "source_only": len(nodes - dsts),
            "parallel": len(pairs) - len(set(pairs)),
            "self_loops": sum(s == d for s, d in pairs),
            "max_indeg": max(indeg.values()), "n": len(nodes)}


def pagerank_step(ranks, nodes, inn, outdeg, damping):
    n = len(nodes)
    dangling = math.fsum(ranks[v] for v in nodes if not outdeg[v])
    return {v: (1.0 - damping) / n + damping * (
        math.fsum(ranks[s] / outdeg[s] for s in inn[v]) + dangling / n)
        for v in nodes}


def pagerank_oracle(src, dst, damping=0.85, iters=20, tol=0.0, start=None):
    """-> (ranks dict, iterations, deltas): dicts and math.fsum; stops after
    iters iterations or the first whose |r' - r|_1 <= tol."""
    nodes = sorted(set(src) | set(dst), key=u64_order)
    outdeg = dict.fromkeys(nodes, 0)
    inn = {v: [] for v in nodes}
    for s, d in zip(src, dst):
        outdeg[s] += 1
        inn[d].append(s)
    r = dict(start) if start else dict.fromkeys(nodes, 1.0 / len(nodes))
    deltas = []
    for _ in range(iters):
        new = pagerank_step(r, nodes, inn, outdeg, damping)
        deltas.append(math.fsum(abs(new[v] - r[v]) for v in nodes))
        r = new
        if tol > 0 and deltas[-1] <= tol:
            break
    return r, len(deltas), deltas


def pagerank_residual(ranks, src, dst, damping):
    """|P(r) - r|_1, P one step of the oracle."""
    new, _, deltas = pagerank_oracle(src, dst, damping, 1, 0.0, ranks)
    return deltas[0]


def pagerank_bound(src, dst, iters):
    """The asserted relative error per node: every term is non-negative, so
    an iteration adds at most (max(max in-degree, dangling nodes) + 8) *
    2^-53 to first order; twice that, times the iterations."""
    f = graph_features(src, dst)
    return iters * (max(f["max_indeg"], f["dangling"]) + 8) * 2.0 ** -52


# damping of the early-stop case: the deltas shrink by at least 1 / damping
# per iteration, so with 0.002 consecutive deltas lie 500x apart and a tol
# halfway between two of them (in the exponent) is over 10x from both
EARLY_DAMPING = 0.002


def early_stop_tol(deltas, k=2):
    """A tol between deltas[k - 1] and deltas[k] (geometric mean): the run
    stops after k + 1 iterations."""
    return math.sqrt(deltas[k - 1] * deltas[k])


def component_oracle(src, dst):
    """node -> the smallest key (u64 order) of its component: union-find."""
    parent = {}

    def find(a):
        root = a
        while parent[root] != root:
            root = parent[root]
        while parent[a] != root:
            parent[a], a = root, parent[a]
        return root

    for s, d in zip(src, dst):
        parent.setdefault(s, s)
        parent.setdefault(d, d)
        a, b = find(s), find(d)
        if a != b:
            if u64_order(a) < u64_order(b):
                parent[b] = a
            else:
                parent[a] = b
    return {v: find(v) for v in parent}


def component_cases():
    """name -> (src, dst) lists."""
    rng = random.Random(77)
    n = 1 << 12
    cases = {}
    cases["path_sorted"] = (list(range(n - 1)), list(range(1, n)))
    zig = [i // 2 if i % 2 == 0 else n - 1 - i // 2 for i in range(n)]
    cases["path_zigzag"] = (zig[:-1], zig[1:])
    perm = list(range(n))
    rng.shuffle(perm)
    cases["path_random"] = (perm[:-1], perm[1:])
    # n / 2 edges over n ids: many components; endpoints that appear once
    s = [rng.randrange(n) for _ in range(n // 2)]
    d = [rng.randrange(n) for _ in range(n // 2)]
    cases["sparse_random"] = (s, d)
    cases["star"] = ([700] * 999, [i for i in range(1000) if i != 700])
    a = [(i, j) for i in range(40) for j in range(i)]
    b = [(100 + i, 100 + j) for i in range(40) for j in range(i)]
    cl = a + b + [(39, 100)]
    rng.shuffle(cl)
    cases["two_cliques"] = ([x for x, _ in cl], [y for _, y in cl])
    # negative keys are large u64 patterns: the label of a component of
    # both signs is its smallest NON-negative key
    keys = rng.sample(range(-(1 << 61), 1 << 61), 600)
    s = [keys[rng.randrange(600)] for _ in range(450)]
    d = [keys[rng.randrange(600)] for _ in range(450)]
    cases["negative_keys"] = (s + [-5, -5], d + [3, -9])
    return cases


def rounds_bound(n):
    return 2 * math.ceil(math.log2(max(n, 2))) + 4


# ------------------------------------------- job-level checks, either tier
# the device is the caller's: "cpu" in the CPU suite, "cuda:0" in the GPU one

def build(device, src, dst, symmetric=False):
    import torch

    from mapreduce_amd.gpu.graph import GraphJob
    g = GraphJob(device).run(torch.tensor(src, dtype=torch.int64),
                             torch.tensor(dst, dtype=torch.int64),
                             symmetric=symmetric)
    assert g.nodes.cpu().tolist() == sorted(set(src) | set(dst),
                                            key=u64_order)
    return g


def check_pagerank(device, src, dst, iters=20):
    """tol = 0 and fixed iterations against the oracle, within
    pagerank_bound per node; the ranks sum to 1 within n iters 2^-52."""
    g = build(device, src, dst)
    pr = g.pagerank(0.85, iters)
    exp, _, deltas = pagerank_oracle(src, dst, 0.85, iters)
    got = dict(zip(g.nodes.cpu().tolist(), pr.ranks.cpu().tolist()))
    bound = pagerank_bound(src, dst, iters)
    worst = max(abs(got[v] - exp[v]) / exp[v] for v in exp)
    print(f"pagerank n={g.n} m={g.m}: worst relative error / bound = "
          f"{worst / bound:.4f}")
    assert pr.iterations == iters
    assert worst <= bound
    assert abs(math.fsum(got.values()) - 1.0) <= g.n * iters * 2.0 ** -52
    assert abs(pr.delta - deltas[-1]) <= 1e-6 * deltas[-1]
    return g, pr


def check_early_stop(device, src, dst):
    g = build(device, src, dst)
    _, _, deltas = pagerank_oracle(src, dst, EARLY_DAMPING, 8)
    tol = early_stop_tol(deltas)
    _, iters, _ = pagerank_oracle(src, dst, EARLY_DAMPING, 8, tol)
    pr = g.pagerank(EARLY_DAMPING, 8, tol)
    assert pr.iterations == iters == 3
    assert pr.delta <= tol


def check_more(device, src, dst, j=7, k=13):
    import torch
    g = build(device, src, dst)
    whole = g.pagerank(0.85, j + k)
    part = g.pagerank(0.85, j)
    assert part.iterations == j
    cont = part.more(k)
    assert cont.iterations == j + k
    assert torch.equal(cont.ranks.view(torch.int64),
                       whole.ranks.view(torch.int64))
    assert cont.delta == whole.delta
    # the first run's result is left as it was
    assert part.iterations == j and not torch.equal(part.ranks, cont.ranks)


def check_components(device, src, dst):
    g = build(device, src, dst, symmetric=True)
    labels, rounds = g.components()
    exp = component_oracle(src, dst)
    got = dict(zip(g.nodes.cpu().tolist(), labels.cpu().tolist()))
    assert got == exp
    print(f"components n={g.n}: {rounds} rounds, bound {rounds_bound(g.n)}")
    assert rounds <= rounds_bound(g.n)
    return rounds
