"""Sessions of a click log — gap-based sessionization, a reducer that needs
the whole value list of its key in order and answers with a list of its
own, so it declares no property flags (job.lua:264-284, the general reduce).

mapfn emits (user, timestamp) for one slice of the log; reducefn orders the
user's timestamps and splits them wherever one exceeds the previous by more
than GAP seconds, emitting (start, end, count) per session.  The rule is
that of ops.session_flags, so both tiers leave identical RESULTS.

The GPU hooks at the bottom route the task onto the running-aggregate
engine (Server GPU dispatch, kind="window": gpu/window.py).

init_args: {"rows": [(user, timestamp), ...]} with explicit rows, or
{"seed", "n", "nusers"} for a synthetic log; "splits" map jobs, "parts"
host-tier partitions.
"""

from __future__ import annotations

import random

GAP = 1800  # seconds of silence that end a session

_CFG = {"seed": 0, "n": 4000, "nusers": 40, "splits": 4, "parts": 4,
        "rows": None}
_ROWS = []    # [(user, timestamp)]
RESULTS = {}  # finalfn: user -> [(start, end, count), ...]

reducefn_gpu = f"sessions:{GAP}"


def make_rows(seed: int, n: int, nusers: int):
    """A skewed click log: a few users click most; every user's clicks come
    in bursts a few seconds to minutes apart, the bursts hours apart, and
    some gaps are exactly GAP and GAP + 1."""
    rng = random.Random(seed)
    clock = [1_700_000_000 + rng.randrange(86_400) for _ in range(nusers)]
    rows = []
    for _ in range(n):
        u = min(int(rng.paretovariate(1.1)) - 1, nusers - 1)
        r = rng.random()
        if r < 0.02:
            step = GAP
        elif r < 0.04:
            step = GAP + 1
        elif r < 0.12:
            step = rng.randrange(GAP + 2, 8 * 3600)
        else:
            step = rng.randrange(0, 400)
        clock[u] += step
        rows.append((u, clock[u]))
    rng.shuffle(rows)
    return rows


def split(times, gap=GAP):
    """The reference rule, on a plain Python list."""
    out = []
    for t in sorted(times):
        if out and t - out[-1][1] <= gap:
            out[-1][1] = t
            out[-1][2] += 1
        else:
            out.append([t, t, 1])
    return [tuple(s) for s in out]


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
    for user, ts in _slice(value):
        emit(user, ts)


def partitionfn(key):
    return key % _CFG["parts"]


def reducefn(key, values, emit):
    for session in split(values):
        emit(session)


def finalfn(pairs):
    RESULTS.clear()
    for user, sessions in pairs:
        RESULTS[user] = [tuple(s) for s in sessions]
    return True


# ---- GPU-tier hooks: mapfn_gpu_pairs stages one map job's rows as (key,
# time) columns; reducefn_gpu names the gap.  Users are their own i64 bit
# patterns, so no gpu_key_decode.

def mapfn_gpu_pairs(key, value):
    rows = _slice(value)
    return [u for u, _ in rows], [ts for _, ts in rows]
