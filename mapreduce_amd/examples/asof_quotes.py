"""As-of join of trades with the prevailing quote as a task script (both
tiers).

Every map job reads one slice of ONE relation — trades (symbol, time,
quantity) or quotes (symbol, time, price) — and emits its rows tagged with
the side they came from; the reducer of a symbol sorts its trades and its
quotes by time and walks the two lists together, pairing every trade with
ONE quote:

    backward   the latest quote at or before the trade (the prevailing one)
    forward    the earliest quote at or after it
    nearest    the closer of the two, the earlier one on a tie

"strict" leaves out quotes at exactly the trade's time, "tolerance" those
further from it than that many time units, and "inner" drops the trades
without a quote instead of reporting them with (None, None).  Among quotes
of one symbol at one time, backward takes the highest price and forward the
lowest (the order of the rows is (time, price)).

The GPU hooks at the bottom route the same task onto the as-of engine
(Server GPU dispatch, kind="asof": gpu/asof.py); both tiers leave the same
RESULTS: symbol -> [(time, quantity, quote time, price), ...] by (time,
quantity).

init_args: {"direction", "tolerance", "strict", "inner"}, and either
{"left": [(key, time, val), ...], "right": [...]} with explicit rows or
{"seed", "nl", "nr", "nkeys"} for two synthetic relations; "splits" map jobs
per side, "parts" host-tier partitions.  Times and quantities are ints,
synthetic prices floats.
"""

from __future__ import annotations

import random

_DIRECTIONS = ("backward", "forward", "nearest")

_CFG = {"direction": "backward", "tolerance": None, "strict": False,
        "inner": False, "seed": 0, "nl": 400, "nr": 300, "nkeys": 40,
        "splits": 3, "parts": 4, "left": None, "right": None}
_REL = {0: [], 1: []}  # side -> [(key, time, val)]
RESULTS = {}           # finalfn: key -> rows (time, qty, quote time, price)

reducefn_gpu = "join_asof"


def make_relations(seed: int, nl: int, nr: int, nkeys: int):
    """Trades and quotes over a shared symbol space: symbols that miss on
    either side, several rows of a symbol at one time, trades before a
    symbol's first quote and after its last."""
    rng = random.Random(seed)
    span = 4 * (nl + nr) // max(nkeys, 1) + 8
    left = [(rng.randrange(nkeys), rng.randrange(span), 1 + i % 97)
            for i in range(nl)]
    right = [(rng.randrange(nkeys // 4, nkeys + nkeys // 4),
              rng.randrange(span // 8, span - span // 8),
              100 + rng.randrange(4000) / 4)
             for _ in range(nr)]
    return left, right


def init(arg):
    global reducefn_gpu
    if arg:
        _CFG.update({k: v for k, v in arg.items() if k in _CFG})
    if _CFG["direction"] not in _DIRECTIONS:
        raise ValueError(f"direction must be one of {_DIRECTIONS}")
    opts = [_CFG["direction"]]
    if _CFG["strict"]:
        opts.append("strict")
    if _CFG["inner"]:
        opts.append("inner")
    if _CFG["tolerance"] is not None:
        opts.append(f"tol={int(_CFG['tolerance'])}")
    reducefn_gpu = "join_asof:" + ",".join(opts)
    if _CFG["left"] is not None or _CFG["right"] is not None:
        left, right = _CFG["left"] or [], _CFG["right"] or []
    else:
        left, right = make_relations(_CFG["seed"], _CFG["nl"], _CFG["nr"],
                                     _CFG["nkeys"])
    _REL[0] = [tuple(r) for r in left]
    _REL[1] = [tuple(r) for r in right]


def _slice(value):
    rows = _REL[value["side"]]
    n = _CFG["splits"]
    return rows[value["part"]::n]


def taskfn(emit):
    for side, tag in ((0, "L"), (1, "R")):
        for p in range(_CFG["splits"]):
            emit(f"{tag}{p}", {"side": side, "part": p})


def mapfn(key, value, emit):
    tag = "LR"[value["side"]]
    for k, t, v in _slice(value):
        emit(k, (tag, t, v))


def partitionfn(key):
    return key % _CFG["parts"]


def reducefn(key, values, emit):
    trades = sorted((t, v) for tag, t, v in values if tag == "L")
    quotes = sorted((t, v) for tag, t, v in values if tag == "R")
    exact, tol = not _CFG["strict"], _CFG["tolerance"]
    direction = _CFG["direction"]

    def near(c, t):
        return (0 <= c < len(quotes)
                and (tol is None or abs(quotes[c][0] - t) <= tol))

    p = q = 0  # quotes before the trade's time / not after it
    for t, v in trades:
        while p < len(quotes) and quotes[p][0] < t:
            p += 1
        while q < len(quotes) and quotes[q][0] <= t:
            q += 1
        back = (q if exact else p) - 1
        fwd = p if exact else q
        hit = None
        if direction != "forward" and near(back, t):
            hit = back
        if direction != "backward" and near(fwd, t) and (
                hit is None or quotes[fwd][0] - t < t - quotes[hit][0]):
            hit = fwd
        if hit is not None:
            emit((t, v) + quotes[hit])
        elif not _CFG["inner"]:
            emit((t, v, None, None))


def _order(row):
    t, v, rt, rv = row
    return (t, v, rt is not None, rt or 0, rv or 0)


def finalfn(pairs):
    RESULTS.clear()
    for key, values in pairs:
        rows = [tuple(v) for v in values]
        if rows:
            RESULTS[key] = sorted(rows, key=_order)
    return True


# ---- GPU-tier hooks: mapfn_gpu_pairs stages one map job's rows as (keys,
# times, vals, side) columns; reducefn_gpu (set by init from the options)
# names the as-of join.  Keys are their own i64 bit patterns, so no
# gpu_key_decode.

def mapfn_gpu_pairs(key, value):
    rows = _slice(value)
    return ([k for k, _, _ in rows], [t for _, t, _ in rows],
            [v for _, _, v in rows], value["side"])
