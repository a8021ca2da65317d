"""PageRank — the classic iterative MapReduce job over keyed data: every
round each node hands its rank, split evenly over its out-edges, to the
nodes it links to, and the round repeats (finalfn -> "loop") until the ranks
stop moving.

    r'[v] = (1 - d) / n + d * (sum over u -> v of r[u] / outdeg[u] + D / n)

with D the rank held by the nodes without out-edges (it is spread over all
nodes), n the number of nodes of either column, parallel edges counted with
their multiplicity and self-loops kept.  No renormalisation.

Host tier, one round per iteration: mapfn emits (dst, RANKS[src] /
outdeg[src]) for every edge of its slice and (node, 0.0) for every node of
its slice, so that nodes nobody links to exist; reducefn emits
(1 - d) / n + d * (fsum(values) + D / n), D taken from RANKS as the round
began; finalfn stores the new ranks and returns "loop" while
|new - RANKS|_1 > TOL.  The reducer needs its whole value list (math.fsum,
exactly rounded, so the order of the values does not matter) and declares no
property flags.  RANKS lives in the module: the host tier of this example
is the threaded local mode.

GPU tier (Server GPU dispatch, kind="graph": gpu/graph.py): the hooks at the
bottom stage the edges once and name the reducer; the engine iterates on the
device until |r' - r|_1 <= TOL and hands finalfn the ranks.  The same
finalfn ends that run in two rounds: after the first RANKS still holds the
start, so it loops; the second continues the resident state by one
iteration, which moves the ranks by at most d * TOL.

init_args: {"edges": [(src, dst), ...]} with explicit edges, or {"seed",
"n", "m"} for a synthetic graph; "splits" map jobs, "parts" host-tier
partitions.
"""

from __future__ import annotations

import math
import random

DAMPING = 0.85
TOL = 1e-6
MAX_ITERS = 200  # device iterations per round, should TOL not be met

_CFG = {"seed": 0, "n": 60, "m": 400, "splits": 3, "parts": 4, "edges": None}
_EDGES = []   # [(src, dst)]
_NODES = []   # the nodes of either column, ascending
_OUTDEG = {}  # node -> out-edges
_STATE = {"dangling": 0.0, "rounds": 0}
RANKS = {}    # node -> rank as the current round began
RESULTS = {}  # finalfn: node -> rank

reducefn_gpu = f"pagerank:d={DAMPING},iters={MAX_ITERS},tol={TOL}"


def make_edges(seed: int, n: int, m: int):
    """A skewed multigraph on nodes 0 .. n - 1: a hub that a third of the
    edges point to, nodes without out-edges (the last tenth), nodes nobody
    links to (the tenth before), parallel edges and self-loops."""
    rng = random.Random(seed)
    sink0, quiet0 = n - max(n // 10, 1), n - 2 * max(n // 10, 1)
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
            d = rng.randrange(n - (sink0 - quiet0))
            if d >= quiet0:
                d += sink0 - quiet0
        edges.append((s, d))
    return edges


def step(ranks, edges, damping=DAMPING):
    """The reference rule, one iteration on a plain dict node -> rank."""
    nodes = sorted({x for e in edges for x in e})
    n = len(nodes)
    outdeg = dict.fromkeys(nodes, 0)
    for s, _ in edges:
        outdeg[s] += 1
    dangling = math.fsum(ranks[v] for v in nodes if not outdeg[v])
    inn = {v: [] for v in nodes}
    for s, d in edges:
        inn[d].append(ranks[s] / outdeg[s])
    return {v: (1.0 - damping) / n
            + damping * (math.fsum(inn[v]) + dangling / n) for v in nodes}


def init(arg):
    if arg:
        _CFG.update({k: v for k, v in arg.items() if k in _CFG})
    edges = _CFG["edges"]
    if edges is None:
        edges = make_edges(_CFG["seed"], _CFG["n"], _CFG["m"])
    _EDGES[:] = [tuple(e) for e in edges]
    _NODES[:] = sorted({x for e in _EDGES for x in e})
    _OUTDEG.clear()
    _OUTDEG.update(dict.fromkeys(_NODES, 0))
    for s, _ in _EDGES:
        _OUTDEG[s] += 1
    RANKS.clear()
    RANKS.update(dict.fromkeys(_NODES, 1.0 / max(len(_NODES), 1)))
    RESULTS.clear()
    _STATE.update(dangling=0.0, rounds=0)


def taskfn(emit):
    # the round begins here: fix the dangling mass its reducers use
    _STATE["dangling"] = math.fsum(
        RANKS[v] for v in _NODES if not _OUTDEG[v])
    for p in range(_CFG["splits"]):
        emit(f"edges{p}", p)


def mapfn(key, value, emit):
    for s, d in _EDGES[value::_CFG["splits"]]:
        emit(d, RANKS[s] / _OUTDEG[s])
    for v in _NODES[value::_CFG["splits"]]:
        emit(v, 0.0)


def partitionfn(key):
    return key % _CFG["parts"]


def reducefn(key, values, emit):
    n = len(_NODES)
    emit((1.0 - DAMPING) / n
         + DAMPING * (math.fsum(values) + _STATE["dangling"] / n))


def finalfn(pairs):
    new = {node: vals[0] for node, vals in pairs}
    delta = math.fsum(abs(new[v] - RANKS[v]) for v in _NODES)
    RANKS.clear()
    RANKS.update(new)
    RESULTS.clear()
    RESULTS.update(new)
    _STATE["rounds"] += 1
    return "loop" if delta > TOL else True


# ---- GPU-tier hooks: mapfn_gpu_pairs stages one map job's edges as (src,
# dst) columns; reducefn_gpu (top of the file) names the iteration.  Nodes
# are their own i64 bit patterns, so no gpu_key_decode.

def mapfn_gpu_pairs(key, value):
    edges = _EDGES[value::_CFG["splits"]]
    return [s for s, _ in edges], [d for _, d in edges]
