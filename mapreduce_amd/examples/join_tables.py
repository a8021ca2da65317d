"""Reduce-side join of two relations as a task script (both tiers).

The classic MapReduce join: every map job reads one slice of ONE relation
and emits its rows tagged with the side they came from; the reducer of a
key crosses that key's "L" values with its "R" values.  Four joins, chosen
by init_args["how"]:

    inner   (l, r) for every left and right row of the key
    left    as inner, plus (l, None) for a left row of a key with no right
    semi    l for every left row of a key that has a right row
    anti    l for every left row of a key that has none

The GPU hooks at the bottom route the same task onto the join engine
(Server GPU dispatch, kind="join": gpu/join.py); both tiers leave the same
RESULTS, values sorted within a key since the host tier promises no value
order there.

init_args: {"how": ..., "left": [(key, val), ...], "right": [...]} with
explicit rows, or {"seed", "nl", "nr", "nkeys"} for two synthetic
relations; "splits" map jobs per side, "parts" host-tier partitions.
Left values are ints, synthetic right values floats.
"""

from __future__ import annotations

import random

_HOWS = {"inner": "join", "left": "join_left", "semi": "join_semi",
         "anti": "join_anti"}

_CFG = {"how": "inner", "seed": 0, "nl": 400, "nr": 300, "nkeys": 120,
        "splits": 3, "parts": 4, "left": None, "right": None}
_REL = {0: [], 1: []}  # side -> [(key, val)]
RESULTS = {}           # finalfn: key -> sorted pairs (or sorted left values)

reducefn_gpu = "join"


def make_relations(seed: int, nl: int, nr: int, nkeys: int):
    """Two relations over a shared key space with duplicates on both
    sides and keys that miss on either."""
    rng = random.Random(seed)
    left = [(rng.randrange(nkeys), i) for i in range(nl)]
    right = [(rng.randrange(nkeys // 3, nkeys + nkeys // 3), i + 0.25)
             for i in range(nr)]
    return left, right


def init(arg):
    global reducefn_gpu
    if arg:
        _CFG.update({k: v for k, v in arg.items() if k in _CFG})
    if _CFG["how"] not in _HOWS:
        raise ValueError(f"how must be one of {tuple(_HOWS)}")
    reducefn_gpu = _HOWS[_CFG["how"]]
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
    for k, v in _slice(value):
        emit(k, (tag, v))


def partitionfn(key):
    return key % _CFG["parts"]


def reducefn(key, values, emit):
    ls = [v for t, v in values if t == "L"]
    rs = [v for t, v in values if t == "R"]
    how = _CFG["how"]
    if how in ("inner", "left"):
        for l in ls:
            for r in rs:
                emit((l, r))
            if how == "left" and not rs:
                emit((l, None))
    elif (how == "semi") == bool(rs):
        for l in ls:
            emit(l)


def _order(p):
    if isinstance(p, tuple):
        return (p[0], p[1] is not None, p[1] or 0)
    return (p,)


def finalfn(pairs):
    RESULTS.clear()
    pairwise = _CFG["how"] in ("inner", "left")
    for key, values in pairs:
        vals = [tuple(v) if pairwise else v for v in values]
        if vals:
            RESULTS[key] = sorted(vals, key=_order)
    return True


# ---- GPU-tier hooks: mapfn_gpu_pairs stages one map job's rows as
# (keys, vals, side) columns; reducefn_gpu (set by init from "how") names
# the join.  Keys are their own i64 bit patterns, so no gpu_key_decode.

def mapfn_gpu_pairs(key, value):
    rows = _slice(value)
    return [k for k, _ in rows], [v for _, v in rows], value["side"]
