"""Distributed group-by with the rows of every key in order, for reducers
whose answer is as long as their input: running totals, running minima and
maxima, and gap-based sessions of an event log.

    job = WindowJob(device)
    res = job.run(users, times, amounts)  # OrderedRows(keys, offsets,
                                          #             order, values)
    res.scan("sum")                       # running amount, by time
    res.sessions(1800)                    # Sessions(keys, start, end, ...)
    res.scan("sum", within_sessions=1800)
    res.rolling("sum", 3600)              # amount over the trailing hour
    res.rolling("max", 99, unit="rows")   # over the trailing 100 rows

Keys are i64 (u64 bit order).  The order column and the optional value
column are i64 or f64 and ride every sort and exchange as their int64
views; their order is that of ops.group_order_keys (-0.0 equals +0.0, every
NaN is one value above +inf) and the stored bits come through unaltered.

The rows of a key are arranged by (order key of the order column, order key
of the value), lexicographically.  Two rows that compare equal under that
rule are interchangeable, so the result depends neither on the order of the
input rows nor on the world size, up to the sign of a zero and the payload
of a NaN.

Single rank: one ops.sort_by_key(keys, order, vals), then
ops.sort_values_in_groups(..., return_perm=True) on the values and again on
the order column as the first pass left it (the op is stable, so the two
passes give the lexicographic order); the two permutations are composed and
applied once.  Without a value column one pass is enough.

Multi-rank, the shape of GroupedValuesJob: sort locally, mulhi-partition
(rank r owns the keys with mulhi(key, world) == r), ONE count exchange, one
all-to-all per column, a re-sort by key and the ordering above.  The
exchange is single-round: a rank's whole partition must fit in its memory.
There is no combine: every row matters.
"""

from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

import torch

from .. import ops
from . import dist as dx


ROLLING_OPS = ("sum", "min", "max", "count", "mean")


class Sessions(NamedTuple):
    keys: torch.Tensor      # i64[nsess]: the key of every session
    start: torch.Tensor     # i64[nsess]: its first time
    end: torch.Tensor       # i64[nsess]: its last time
    count: torch.Tensor     # i64[nsess]: its rows
    per_key: torch.Tensor   # i64[nkeys]: the sessions of every key

    def to_host(self) -> List[Tuple[int, list]]:
        """[(key as i64, [(start, end, count), ...])] in key order."""
        rows = list(zip(self.start.cpu().tolist(), self.end.cpu().tolist(),
                        self.count.cpu().tolist()))
        out, a = [], 0
        keys = self.keys.cpu().tolist()
        for m in self.per_key.cpu().tolist():
            out.append((keys[a], rows[a:a + m]))
            a += m
        return out


class OrderedRows(NamedTuple):
    keys: torch.Tensor     # i64[nseg], ascending in u64 order, unique
    offsets: torch.Tensor  # i64[nseg + 1]: key s owns rows o[s]:o[s + 1]
    order: torch.Tensor    # the order column, ascending within each key
    values: Optional[torch.Tensor]  # the value column beside it, or None

    def counts(self) -> torch.Tensor:
        return self.offsets[1:] - self.offsets[:-1]

    def _row_keys(self) -> torch.Tensor:
        """The segment number of every row: it stands in for the key."""
        return torch.repeat_interleave(
            torch.arange(self.keys.numel(), device=self.keys.device),
            self.counts(), output_size=self.order.numel())

    def _session_flags(self, gap) -> torch.Tensor:
        return ops.session_flags(self._row_keys(), self.order, gap)

    def scan(self, op: str = "sum", within_sessions=None) -> torch.Tensor:
        """The running sum / min / max of the value column within each key,
        rows in order; within_sessions=gap restarts it at every session."""
        if self.values is None:
            raise ValueError("scan needs a value column")
        if within_sessions is None:
            rows = self._row_keys()
        else:  # the session number of every row as the key
            rows = torch.cumsum(self._session_flags(within_sessions), 0)
        return ops.scan_by_key_sorted(rows, self.values, op)

    def sessions(self, gap) -> Sessions:
        """The sessions of every key: a row opens one when it starts its
        key or its time exceeds the previous row's by more than gap.  The
        order column must be i64."""
        rows = self._row_keys()
        srow, soff = ops.group_sessions(rows, self.order, gap)
        st, en = soff[:-1], soff[1:]
        if self.order.numel():
            start = self.order.index_select(0, st)
            end = self.order.index_select(0, en - 1)
        else:
            start = end = self.order[:0]
        per_key = torch.bincount(srow, minlength=self.keys.numel())
        return Sessions(self.keys.index_select(0, srow), start, end, en - st,
                        per_key)

    def frames(self, preceding, following=0, unit: str = "range"):
        """-> (lo, hi): the frame [lo[i], hi[i]) of every row, of rows of
        its own key.  unit="range": the rows whose order entry lies in
        [order - preceding, order + following], peers included
        (ops.frame_bounds; the order column must be i64).  unit="rows": the
        preceding rows before and the following rows behind it
        (ops.frame_bounds_rows), which depends on how (order, value)
        arranged the rows."""
        if unit == "range":
            return ops.frame_bounds(self._row_keys(), self.order, preceding,
                                    following)
        if unit == "rows":
            return ops.frame_bounds_rows(self.offsets, preceding, following,
                                         nrows=self.order.numel())
        raise ValueError(f"unit must be 'range' or 'rows', got {unit!r}")

    def rolling(self, op: str, preceding=0, following=0, unit: str = "range",
                frames=None) -> torch.Tensor:
        """The sum / min / max / count / mean of the value column over every
        row's frame (ops.frame_reduce).  frames= takes a pair from frames(),
        so several aggregates share one bounds pass; preceding, following
        and unit are not read then.  count is i64 and needs no value column;
        mean is f64, sum / count with an i64 sum converted after
        wrapping."""
        if op not in ROLLING_OPS:
            raise ValueError(
                f"op must be one of {ROLLING_OPS}, got {op!r}")
        if op != "count" and self.values is None:
            raise ValueError("rolling needs a value column")
        lo, hi = (frames if frames is not None
                  else self.frames(preceding, following, unit))
        if op == "count":
            return hi - lo
        if op != "mean":
            return ops.frame_reduce(self.values, lo, hi, op)
        total = ops.frame_reduce(self.values, lo, hi, "sum")
        return total.to(torch.float64) / (hi - lo).to(torch.float64)

    def to_host(self) -> List[Tuple[int, list]]:
        """[(key as i64, [(order, value), ...])] in key order, the rows
        ascending; [(key, [order, ...])] without a value column."""
        off = self.offsets.cpu().tolist()
        rows = self.order.cpu().tolist()
        if self.values is not None:
            rows = list(zip(rows, self.values.cpu().tolist()))
        return [(k, rows[off[s]:off[s + 1]])
                for s, k in enumerate(self.keys.cpu().tolist())]


def _check_col(t: torch.Tensor, name: str) -> None:
    if t.dtype not in (torch.int64, torch.float64):
        raise TypeError(f"{name} must be int64 or float64, got {t.dtype}")


class WindowJob:
    def __init__(self, device, group=None):
        self.device = torch.device(device)
        self.group = group
        self.rank, self.world = dx.world_info(group)

    def _shuffle(self, cols):
        """Key-sorted columns (keys first) -> this rank's partition,
        re-sorted by key."""
        counts = ops.partition_counts(cols[0], self.world)
        recv = dx.exchange_counts(counts, self.group)
        sc = counts.cpu().tolist()
        rc = recv.cpu().tolist()
        cols = [dx.exchange(c, sc, rc, self.group) for c in cols]
        return ops.sort_by_key(*cols)

    def run(self, keys: torch.Tensor, order: torch.Tensor,
            vals: Optional[torch.Tensor] = None) -> OrderedRows:
        """One order entry (and one value) per key; returns this rank's
        partition.  The inputs are never written."""
        n = keys.numel()
        if order.numel() != n or (vals is not None and vals.numel() != n):
            raise ValueError("one order entry and one value per key required")
        _check_col(order, "order")
        if vals is not None:
            _check_col(vals, "vals")
        cols = [keys, order.view(torch.int64)]
        if vals is not None:
            cols.append(vals.view(torch.int64))
        cols = ops.sort_by_key(*cols)
        if self.world > 1 or dx.force_collectives():
            cols = self._shuffle(cols)
        k, o = cols[0], cols[1].view(order.dtype)
        uk, off = ops.group_by_key_sorted(k)
        if vals is None:
            return OrderedRows(uk, off, ops.sort_values_in_groups(k, o, off),
                               None)
        # by value, then stably by the order column: lexicographic
        v = cols[2].view(vals.dtype)
        _, p1 = ops.sort_values_in_groups(k, v, off, return_perm=True)
        _, p2 = ops.sort_values_in_groups(k, o.index_select(0, p1), off,
                                          return_perm=True)
        perm = p1.index_select(0, p2)
        return OrderedRows(uk, off, o.index_select(0, perm),
                           v.index_select(0, perm))
