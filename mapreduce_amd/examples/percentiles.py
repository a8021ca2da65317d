"""Latency percentiles per endpoint — a reducer that needs the whole value
list of its key, so it is neither associative nor commutative and declares
no property flags (job.lua:264-284, the general reduce).

mapfn emits (endpoint, latency) for one slice of the request log; reducefn
orders the key's values and picks the p50, p90 and p99 by the exact index
rule of ops.group_quantiles: the value at (N * (len - 1)) // D of the
ordered list for the fraction N/D.  No interpolation, so both tiers pick the
same stored value and leave identical RESULTS.

The GPU hooks at the bottom route the task onto the order-statistics engine
(Server GPU dispatch, kind="group": gpu/grouped.py).

init_args: {"rows": [(endpoint, latency), ...]} with explicit rows, or
{"seed", "n", "nendpoints"} for a synthetic log; "splits" map jobs, "parts"
host-tier partitions.
"""

from __future__ import annotations

import random

FRACS = ((1, 2), (9, 10), (99, 100))

_CFG = {"seed": 0, "n": 4000, "nendpoints": 24, "splits": 4, "parts": 4,
        "rows": None}
_ROWS = []    # [(endpoint, latency)]
RESULTS = {}  # finalfn: endpoint -> (p50, p90, p99)

reducefn_gpu = "quantile:" + ",".join(f"{n}/{d}" for n, d in FRACS)


def make_rows(seed: int, n: int, nendpoints: int):
    """A skewed request log: a few endpoints take most of the traffic,
    latencies are log-normal milliseconds with a slow tail."""
    rng = random.Random(seed)
    rows = []
    for _ in range(n):
        e = min(int(rng.paretovariate(1.2)) - 1, nendpoints - 1)
        ms = rng.lognormvariate(3.0 + 0.1 * (e % 5), 0.6)
        if rng.random() < 0.01:
            ms *= 20.0
        rows.append((e, round(ms, 3)))
    return rows


def pick(values, fracs=FRACS):
    """The reference rule, on a plain Python list."""
    s = sorted(values)
    return tuple(s[(n * (len(s) - 1)) // d] for n, d in fracs)


def init(arg):
    if arg:
        _CFG.update({k: v for k, v in arg.items() if k in _CFG})
    rows = _CFG["rows"]
    if rows is None:
        rows = make_rows(_CFG["seed"], _CFG["n"], _CFG["nendpoints"])
    _ROWS[:] = [tuple(r) for r in rows]
    RESULTS.clear()


def _slice(part):
    return _ROWS[part::_CFG["splits"]]


def taskfn(emit):
    for p in range(_CFG["splits"]):
        emit(f"log{p}", p)


def mapfn(key, value, emit):
    for endpoint, ms in _slice(value):
        emit(endpoint, ms)


def partitionfn(key):
    return key % _CFG["parts"]


def reducefn(key, values, emit):
    emit(pick(values))


def finalfn(pairs):
    RESULTS.clear()
    for endpoint, values in pairs:
        (row,) = values
        RESULTS[endpoint] = tuple(row)
    return True


# ---- GPU-tier hooks: mapfn_gpu_pairs stages one map job's rows as (key,
# value) columns; reducefn_gpu names the three quantiles.  Endpoints are
# their own i64 bit patterns, so no gpu_key_decode.

def mapfn_gpu_pairs(key, value):
    rows = _slice(value)
    return [e for e, _ in rows], [ms for _, ms in rows]
