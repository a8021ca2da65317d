"""Spend over the trailing hour — per user, the amount spent in the hour up
to and including every purchase: a rolling aggregate, a reducer that needs
the whole value list of its key in order and answers with a list as long as
its input, so it declares no property flags (job.lua:264-284, the general
reduce).

mapfn emits (user, (timestamp, amount)) for one slice of the log; reducefn
orders the user's purchases and gives every one the sum of the amounts whose
time lies in [timestamp - WINDOW, timestamp], both ends inclusive, so
purchases made in the same second count for each other.  The rule is that of
ops.frame_bounds and ops.frame_reduce, and amounts are integers (cents), so
both tiers leave identical RESULTS.

The GPU hooks at the bottom route the task onto the running-aggregate
engine (Server GPU dispatch, kind="window": gpu/window.py).

init_args: {"rows": [(user, timestamp, amount), ...]} with explicit rows,
or {"seed", "n", "nusers"} for a synthetic log; "splits" map jobs, "parts"
host-tier partitions.
"""

from __future__ import annotations

import bisect
import random

WINDOW = 3600  # seconds a purchase stays in the trailing sum

_CFG = {"seed": 0, "n": 4000, "nusers": 40, "splits": 4, "parts": 4,
        "rows": None}
_ROWS = []    # [(user, timestamp, amount)]
RESULTS = {}  # finalfn: user -> [(timestamp, spend over the hour), ...]

reducefn_gpu = f"rolling:sum:{WINDOW}"


def make_rows(seed: int, n: int, nusers: int):
    """A skewed purchase log: a few users buy most; purchases come seconds
    to minutes apart with longer pauses between, some in the same second as
    the one before, and some exactly WINDOW and WINDOW + 1 seconds after
    it."""
    rng = random.Random(seed)
    clock = [1_700_000_000 + rng.randrange(86_400) for _ in range(nusers)]
    rows = []
    for _ in range(n):
        u = min(int(rng.paretovariate(1.1)) - 1, nusers - 1)
        r = rng.random()
        if r < 0.05:
            step = 0
        elif r < 0.08:
            step = WINDOW
        elif r < 0.11:
            step = WINDOW + 1
        elif r < 0.16:
            step = rng.randrange(WINDOW + 2, 8 * 3600)
        else:
            step = rng.randrange(1, 900)
        clock[u] += step
        rows.append((u, clock[u], rng.randrange(1, 50_000)))
    rng.shuffle(rows)
    return rows


def window(rows, width=WINDOW):
    """The reference rule, on a plain Python list of (timestamp, amount):
    -> [(timestamp, spend), ...] ascending, spend = the amounts of the rows
    with timestamp - width <= their time <= timestamp."""
    rows = sorted(rows)
    times = [t for t, _ in rows]
    run = [0]
    for _, a in rows:
        run.append(run[-1] + a)
    return [(t, run[bisect.bisect_right(times, t)]
             - run[bisect.bisect_left(times, t - width)]) for t in times]


def init(arg):
    if arg:
        _CFG.update({k: v for k, v in arg.items() if k in _CFG})
    rows = _CFG["rows"]
    if rows is None:
        rows = make_rows(_CFG["seed"], _CFG["n"], _CFG["nusers"])
    _ROWS[:] = [tuple(r) for r in rows]
    RESULTS.clear()


def _slice(part):
    return _ROWS[part::_CFG["splits"]]


def taskfn(emit):
    for p in range(_CFG["splits"]):
        emit(f"log{p}", p)


def mapfn(key, value, emit):
    for user, ts, amount in _slice(value):
        emit(user, (ts, amount))


def partitionfn(key):
    return key % _CFG["parts"]


def reducefn(key, values, emit):
    for row in window([tuple(v) for v in values]):
        emit(row)


def finalfn(pairs):
    RESULTS.clear()
    for user, rows in pairs:
        RESULTS[user] = [tuple(r) for r in rows]
    return True


# ---- GPU-tier hooks: mapfn_gpu_pairs stages one map job's rows as (key,
# time, amount) columns; reducefn_gpu names the aggregate and the window.
# Users are their own i64 bit patterns, so no gpu_key_decode.

def mapfn_gpu_pairs(key, value):
    rows = _slice(value)
    return ([u for u, _, _ in rows], [ts for _, ts, _ in rows],
            [a for _, _, a in rows])
