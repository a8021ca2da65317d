"""Distributed equi-join of two (key, value) relations held as tensor columns.

The reduce-side join as a public primitive: orders x customers, edges x
ranks, postings x document metadata.  Keys are i64 (u64 bit order), each
side carries one i64 or f64 value column:

    job = JoinJob(device, how="inner")
    res = job.run(lkeys, lvals, rkeys, rvals)
    # JoinResult(keys, lvals, rvals, matched)

Single rank: a stable sort of each side (K1), ops.join_sorted on the two
sorted key columns (ops/hip/join.hip), then one gather per output column.
Rows come out by key ascending (u64), then left input order, then right
input order — the stable sorts give the last two.

Multi-rank, the shape of KeyedReduceJob: sort locally, mulhi-partition
each side (rank r owns the keys with mulhi(key, world) == r), ONE packed
count exchange, one all-to-all per column in the same order on every rank
(left keys, left values, right keys, right values), a stable re-sort of
the received runs — within a key the rows keep (source rank, source
order) — and the local join.  The exchange is single-round: a rank's whole
partition of both relations must fit in its memory.

Values are opaque 64-bit payloads: f64 columns ride every sort, exchange
and gather as their int64 view and are viewed back at the end, so NaN
payloads, -0.0 and inf come through bit for bit.

Output size: a join can be far larger than its inputs (a key with a left
and b right rows gives a * b).  max_rows bounds the rows ONE RANK may
produce; past it run() raises ops.JoinTooLarge before anything is
allocated.  Multi-rank, the ranks all-gather their (rows, limit) after the
bounds pass and every rank raises if any is over — no rank raises alone
between collectives.
"""

from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from .. import ops
from . import dist as dx

_HOWS = ("inner", "left", "semi", "anti")
ROW_BYTES = 40  # one output row: key, two indices, two values


class JoinResult(NamedTuple):
    keys: torch.Tensor                # i64[total], ascending in u64 order
    lvals: torch.Tensor               # left values, the input's dtype
    rvals: Optional[torch.Tensor]     # inner/left; 0 where unmatched
    matched: Optional[torch.Tensor]   # left only: bool[total]


def _as_i64(v: torch.Tensor, name: str) -> torch.Tensor:
    if v.dtype == torch.float64:
        return v.view(torch.int64)
    if v.dtype == torch.int64:
        return v
    raise TypeError(f"{name} must be int64 or float64, got {v.dtype}")


class JoinJob:
    def __init__(self, device, group=None, how: str = "inner",
                 max_rows: Optional[int] = None):
        if how not in _HOWS:
            raise ValueError(f"how must be one of {_HOWS}, got {how!r}")
        self.device = torch.device(device)
        self.group = group
        self.rank, self.world = dx.world_info(group)
        self.how = how
        self.max_rows = max_rows

    def _limit(self) -> Optional[int]:
        """Rows this rank may produce: max_rows, else half of the free
        device memory at ROW_BYTES per row; no limit on the CPU tier."""
        if self.max_rows is not None:
            return int(self.max_rows)
        if self.device.type == "cuda":
            free, _ = torch.cuda.mem_get_info(self.device)
            return free // 2 // ROW_BYTES
        return None

    def _shuffle(self, lk, lv, rk, rv):
        """Sorted sides -> this rank's partition of both, re-sorted."""
        w = self.world
        cl = ops.partition_counts(lk, w)
        cr = ops.partition_counts(rk, w)
        # a side's keys and values share one count vector: two segments
        # cover the four columns, in one collective
        send = torch.cat([cl, cr])
        recv = dx.exchange_counts(send, self.group)
        sc = send.cpu().tolist()
        rc = recv.cpu().tolist()
        lk = dx.exchange(lk, sc[:w], rc[:w], self.group)
        lv = dx.exchange(lv, sc[:w], rc[:w], self.group)
        rk = dx.exchange(rk, sc[w:], rc[w:], self.group)
        if rv is not None:
            rv = dx.exchange(rv, sc[w:], rc[w:], self.group)
        lk, lv = ops.sort_by_key(lk, lv)
        if rv is not None:
            rk, rv = ops.sort_by_key(rk, rv)
        else:
            (rk,) = ops.sort_by_key(rk)
        return lk, lv, rk, rv

    def _agree_on_size(self, cnt: torch.Tensor, limit: Optional[int]):
        """All-gather (rows, limit) of every rank; raise on all of them
        if any rank is over its limit."""
        import torch.distributed as td

        per = cnt if self.how == "inner" else cnt.clamp(min=1)
        mine = torch.stack([per.sum(), torch.tensor(
            -1 if limit is None else limit, dtype=torch.int64,
            device=per.device)])
        every = [torch.zeros_like(mine) for _ in range(self.world)]
        td.all_gather(every, mine.contiguous(), group=self.group)
        for total, lim in torch.stack(every).cpu().tolist():
            if lim >= 0 and total > lim:
                raise ops.JoinTooLarge(total, lim)

    def run(self, lkeys: torch.Tensor, lvals: torch.Tensor,
            rkeys: torch.Tensor,
            rvals: Optional[torch.Tensor] = None) -> JoinResult:
        """One relation per side, one value per key; rvals may be None
        under semi and anti, which never read it.  Returns this rank's
        partition of the join."""
        how = self.how
        pairs = how in ("inner", "left")
        if lkeys.numel() != lvals.numel():
            raise ValueError("one left value per left key required")
        if pairs and rvals is None:
            raise ValueError(f"how={how!r} needs right values")
        if rvals is not None and rkeys.numel() != rvals.numel():
            raise ValueError("one right value per right key required")
        ldt = lvals.dtype
        rdt = rvals.dtype if rvals is not None else None
        lv = _as_i64(lvals, "lvals")
        rv = _as_i64(rvals, "rvals") if pairs else None

        lk, lv = ops.sort_by_key(lkeys, lv)
        if pairs:
            rk, rv = ops.sort_by_key(rkeys, rv)
        else:
            (rk,) = ops.sort_by_key(rkeys)
        collective = self.world > 1 or dx.force_collectives()
        if collective:
            lk, lv, rk, rv = self._shuffle(lk, lv, rk, rv)

        if not pairs:
            li = ops.join_sorted(lk, rk, how)
            return JoinResult(lk.index_select(0, li),
                              lv.index_select(0, li).view(ldt), None, None)

        limit = self._limit()
        bounds = None
        if collective:
            bounds = ops.join_bounds(lk, rk)
            self._agree_on_size(bounds[1], limit)
            limit = None  # checked, on every rank at once
        li, ri = ops.join_sorted(lk, rk, how, max_rows=limit, bounds=bounds)
        keys = lk.index_select(0, li)
        lout = lv.index_select(0, li).view(ldt)
        if how == "inner":
            return JoinResult(keys, lout, rv.index_select(0, ri).view(rdt),
                              None)
        matched = ri >= 0
        if rv.numel():
            rout = rv.index_select(0, ri.clamp(min=0))
            rout.masked_fill_(~matched, 0)
        else:
            rout = torch.zeros_like(ri)
        return JoinResult(keys, lout, rout.view(rdt), matched)
