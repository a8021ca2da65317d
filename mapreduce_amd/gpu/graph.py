"""Iterative jobs over keyed data: a graph kept resident on the device as a
CSR by destination, and PageRank and connected components run over it with
one gather-reduce pass (ops.graph_propagate) per iteration.

    g = GraphJob(device).run(src_keys, dst_keys)      # Graph
    pr = g.pagerank(damping=0.85, iters=100, tol=1e-9)
    pr.ranks, pr.iterations, pr.delta
    pr = pr.more(20)                                  # continue the state
    labels, rounds = GraphJob(device).run(a, b, symmetric=True).components()

Keys are i64 tensors holding u64 bit patterns.  The node dictionary `nodes`
(i64[n], ascending in u64 order) is the distinct keys of both columns; every
array of the graph is indexed by the dense id of a node, its position in the
dictionary.  Parallel edges count with their multiplicity and self-loops are
kept.  symmetric=True appends every edge reversed.

Build, all torch and existing ops: one sort of the keys for the dictionary,
a search for the dense ids, a count for the out-degrees, ONE ops.sort_pairs
of the packed key (dst << b | src, b = the bits n needs, so 2 b radix bits
and not 64) that orders the edges by (dst, src), and a search of the sorted
destinations for the row offsets (what a count and a cumsum give, without
atomics on a hub's counter).  Ordering a row's in-edges by source is the one locality lever
the gather has.

PageRank: r0 = 1 / n (or `start`),
r'[v] = (1 - d) / n + d * (sum over u -> v of r[u] / outdeg[u] + D / n), D the
rank held by nodes without out-edges; no renormalisation.  Every iteration
is ops.graph_propagate over contrib = r / outdeg and ops.pagerank_update,
chained on the device: with tol == 0 nothing is read back until the end,
with tol > 0 the 8 bytes of |r' - r|_1 per iteration.

Components (symmetric graphs): the FastSV scheme on dense ids from
f = arange(n).  A round takes gp = f[f], mn = the minimum of gp over every
node's neighbours (graph_propagate "min"), hooks the parent
(f[f_old[v]] = min(.., mn[v])) and sets f = min(f, mn, gp); it stops when f
no longer changes (one sync per round, about log2 n rounds).  A component's
label is its smallest node key in dictionary order.

Multi-rank: vertex-replicated, edge-partitioned; no edge moves.  Every rank
keeps the edges it staged, the dictionary is the distinct keys of the
all-gathered local dictionaries, the out-degrees and every iteration's sums
take one all_reduce(SUM) of an n-vector and mn one all_reduce(MIN): n * 8
bytes per iteration per rank.  The PageRank stop decision is rank 0's and
is broadcast, since an f64 all-reduce need not leave the same bits on every
rank and ranks that disagree on "converged" would deadlock the next
collective.  Graph.owned() is the contiguous slice of the nodes rank r
emits."""

from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.distributed as dist

from .. import ops
from . import dist as dx

_SIGN = -(1 << 63)


def _distinct(keys: torch.Tensor) -> torch.Tensor:
    """The distinct keys, ascending in u64 order."""
    if keys.numel() == 0:
        return keys.clone()
    k, _ = ops.sort_pairs(keys)
    return ops.group_by_key_sorted(k)[0]


def _gather_distinct(local: torch.Tensor, group, world: int) -> torch.Tensor:
    """The distinct keys of every rank's dictionary."""
    cnt = torch.tensor([local.numel()], dtype=torch.int64,
                       device=local.device)
    cnts = [torch.zeros_like(cnt) for _ in range(world)]
    dist.all_gather(cnts, cnt, group=group)
    sizes = [int(c) for c in cnts]
    pad = torch.zeros(max(max(sizes), 1), dtype=torch.int64,
                      device=local.device)
    pad[:local.numel()] = local
    bufs = [torch.zeros_like(pad) for _ in range(world)]
    dist.all_gather(bufs, pad, group=group)
    return _distinct(torch.cat([b[:s] for b, s in zip(bufs, sizes)]))


class PageRankResult:
    """ranks f64[n] by dense id (Graph.nodes holds the keys), the iterations
    run so far and the last iteration's |r' - r|_1.  It keeps the state:
    more(iters) continues from it, and a run of j iterations continued by k
    equals one run of j + k bit for bit."""

    def __init__(self, graph, ranks, contrib, dangling, iterations, delta,
                 damping, tol):
        self.graph = graph
        self.ranks = ranks
        self.iterations = iterations
        self.delta = delta
        self.damping = damping
        self.tol = tol
        self._contrib = contrib
        self._dangling = dangling

    def more(self, iters: int, tol: Optional[float] = None):
        return self.graph._pagerank_run(
            self.ranks, self._contrib, self._dangling, self.iterations,
            self.delta, self.damping, iters, self.tol if tol is None else tol)


class Graph:
    def __init__(self, nodes, offsets, src, outdeg, symmetric, group=None):
        self.nodes = nodes      # i64[n], ascending in u64 order
        self.offsets = offsets  # i64[n + 1]: in-edges of v at o[v]:o[v + 1]
        self.src = src          # int32[m]: dense source ids, by (dst, src)
        self.outdeg = outdeg    # i64[n], over every rank's edges
        self.symmetric = symmetric
        self.group = group
        self.rank, self.world = dx.world_info(group)
        od = outdeg.to(torch.float64)
        self.inv_out = torch.where(outdeg > 0, 1.0 / od.clamp(min=1.0),
                                   torch.zeros_like(od))

    @property
    def n(self) -> int:
        return self.nodes.numel()

    @property
    def m(self) -> int:
        return self.src.numel()

    def _collective(self) -> bool:
        return self.world > 1 or dx.force_collectives()

    def owned(self) -> Tuple[int, int]:
        """[a, b): the dense ids whose results this rank emits."""
        return (self.n * self.rank // self.world,
                self.n * (self.rank + 1) // self.world)

    # ------------------------------------------------------------ PageRank
    def pagerank(self, damping: float = 0.85, iters: int = 100,
                 tol: float = 0.0, start: Optional[torch.Tensor] = None
                 ) -> PageRankResult:
        if not 0.0 <= damping <= 1.0:
            raise ValueError(f"damping must be in [0, 1], got {damping}")
        if tol < 0:
            raise ValueError(f"tol must not be negative, got {tol}")
        n = self.n
        if start is None:
            r = torch.full((n,), 1.0 / max(n, 1), dtype=torch.float64,
                           device=self.nodes.device)
        else:
            if start.dtype != torch.float64 or start.numel() != n:
                raise ValueError(f"start must be float64[{n}]")
            r = start.to(self.nodes.device).clone()
        contrib = r * self.inv_out
        dangling = r[self.outdeg == 0].sum()
        return self._pagerank_run(r, contrib, dangling, 0, float("inf"),
                                  float(damping), iters, float(tol))

    def _pagerank_run(self, r, contrib, dangling, done, delta, damping,
                      iters, tol):
        if isinstance(iters, bool) or not isinstance(iters, int) or iters < 0:
            raise ValueError(f"iters must be a non-negative int, got {iters}")
        dl = None
        for _ in range(iters if self.n else 0):
            sums = ops.graph_propagate(self.offsets, self.src, contrib, "sum")
            if self._collective():
                dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=self.group)
            r, contrib, partials = ops.pagerank_update(
                sums, r, self.inv_out, damping, dangling)
            p = partials.sum(0)
            dl, dangling = p[0], p[1]
            done += 1
            if tol > 0:
                stop = (dl <= tol).to(torch.int64).reshape(1)
                if self._collective():
                    dist.broadcast(stop, src=0, group=self.group)
                if int(stop):
                    break
        if dl is not None:
            delta = float(dl)
        return PageRankResult(self, r, contrib, dangling, done, delta,
                              damping, tol)

    # ---------------------------------------------------------- components
    def components(self) -> Tuple[torch.Tensor, int]:
        """-> (labels i64[n]: the smallest node key of every node's
        component, rounds)."""
        if not self.symmetric:
            raise ValueError(
                "components needs a graph built with symmetric=True")
        n = self.n
        f = torch.arange(n, dtype=torch.int64, device=self.nodes.device)
        rounds = 0
        while n:
            gp = f.index_select(0, f)
            mn = ops.graph_propagate(self.offsets, self.src, gp, "min")
            if self._collective():
                dist.all_reduce(mn, op=dist.ReduceOp.MIN, group=self.group)
            new = f.scatter_reduce(0, f, mn, "amin", include_self=True)
            new = torch.minimum(torch.minimum(new, mn), gp)
            rounds += 1
            # integers: every rank holds the same f, so all agree
            same = torch.equal(new, f)
            f = new
            if same:
                break
        return self.nodes.index_select(0, f), rounds


class GraphJob:
    def __init__(self, device, group=None):
        self.device = torch.device(device)
        self.group = group
        self.rank, self.world = dx.world_info(group)

    def run(self, src_keys: torch.Tensor, dst_keys: torch.Tensor,
            symmetric: bool = False) -> Graph:
        """Two unsorted i64 columns, one edge src -> dst per row (this
        rank's edges).  The inputs are never written."""
        if src_keys.dtype != torch.int64 or dst_keys.dtype != torch.int64:
            raise TypeError("src_keys and dst_keys must be int64")
        if src_keys.numel() != dst_keys.numel():
            raise ValueError("one destination per source required")
        s = src_keys.to(self.device).reshape(-1)
        d = dst_keys.to(self.device).reshape(-1)
        if symmetric:
            s, d = torch.cat([s, d]), torch.cat([d, s])
        collective = self.world > 1 or dx.force_collectives()
        nodes = _distinct(torch.cat([s, d]))
        if collective:
            nodes = _gather_distinct(nodes, self.group, self.world)
        n, m = nodes.numel(), s.numel()
        ops._group_check_rows(n)
        ops._group_check_rows(m)
        order = nodes ^ _SIGN  # ascending as signed values
        sid = torch.searchsorted(order, s ^ _SIGN)
        did = torch.searchsorted(order, d ^ _SIGN)
        outdeg = torch.bincount(sid, minlength=n)
        if collective:
            dist.all_reduce(outdeg, op=dist.ReduceOp.SUM, group=self.group)
        b = max(1, (max(n, 1) - 1).bit_length())
        packed, _ = ops.sort_pairs((did << b) | sid, None, bits=2 * b)
        src = (packed & ((1 << b) - 1)).to(torch.int32)
        # offsets[v] = the edges whose destination is below v: a search of
        # the sorted column gives what a count and a cumsum give, without
        # the count's atomics, which a hub destination serialises
        offsets = torch.searchsorted(
            packed >> b, torch.arange(n + 1, device=self.device))
        return Graph(nodes, offsets, src, outdeg, symmetric, self.group)
