"""Distributed as-of join of two time-ordered relations held as tensor
columns: every left row (a trade, a click, a sensor reading) is paired with
ONE right row of its key (a quote, a session state, a calibration), the
latest at or before its time, the earliest at or after it, or the nearer of
the two.

    job = AsofJoinJob(device, direction="backward", tolerance=None)
    res = job.run(lkeys, ltimes, lvals, rkeys, rtimes, rvals)
    # AsofResult(keys, ltimes, lvals, rtimes, rvals, matched)

Keys are i64 (u64 bit order).  Times are i64 or f64, one dtype on both
sides, ordered by ops.group_order_keys (-0.0 equals +0.0, every NaN is one
value above +inf); each side carries one i64 or f64 value column, an opaque
64-bit payload whose bits (NaN payloads, -0.0) come through unaltered.

Each side is arranged by WindowJob.run(keys, times, vals): rows by (key,
time, value) and, multi-rank, mulhi-shuffled so that rank r owns the keys
with mulhi(key, world) == r on BOTH sides.  The per-row keys are rebuilt
from the offsets, ops.asof_sorted (ops/hip/asof.hip) matches the rows and
one gather per column builds the output: one row per left row in the
arranged order, by key ascending (u64), then time, then left value.

Right rows with equal (key, time) are arranged by the order key of their
value, so the result depends neither on the order of the input rows nor on
the world size: backward takes the largest such value, forward the
smallest.  The exchange is single-round: a rank's whole partition of both
relations must fit in its memory.

how="left" keeps every left row: rtimes and rvals are 0 and matched is
False where there is no match.  how="inner" keeps the matched rows only
(matched is None) at the cost of one host sync.
"""

from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from .. import ops
from .window import WindowJob

_HOWS = ("left", "inner")


class AsofResult(NamedTuple):
    keys: torch.Tensor     # i64[n], ascending in u64 order
    ltimes: torch.Tensor   # left times, ascending within each key
    lvals: torch.Tensor    # left values, the input's dtype
    rtimes: torch.Tensor   # the matched right row's time; 0 where unmatched
    rvals: torch.Tensor    # the matched right row's value; 0 where unmatched
    matched: Optional[torch.Tensor]  # left only: bool[n]


def _row_keys(rows) -> torch.Tensor:
    """The key of every row of an OrderedRows."""
    return torch.repeat_interleave(rows.keys, rows.counts(),
                                   output_size=rows.order.numel())


class AsofJoinJob:
    def __init__(self, device, group=None, direction: str = "backward",
                 tolerance: Optional[int] = None, allow_exact: bool = True,
                 how: str = "left"):
        if how not in _HOWS:
            raise ValueError(f"how must be one of {_HOWS}, got {how!r}")
        if direction not in ops._ASOF_DIRECTIONS:
            raise ValueError(
                f"direction must be one of {tuple(ops._ASOF_DIRECTIONS)}, "
                f"got {direction!r}")
        self.device = torch.device(device)
        self.group = group
        self.direction = direction
        self.tolerance = ops._asof_tolerance(tolerance)
        self.allow_exact = bool(allow_exact)
        self.how = how
        self._arrange = WindowJob(device, group)
        self.rank, self.world = self._arrange.rank, self._arrange.world

    def run(self, lkeys: torch.Tensor, ltimes: torch.Tensor,
            lvals: torch.Tensor, rkeys: torch.Tensor, rtimes: torch.Tensor,
            rvals: torch.Tensor) -> AsofResult:
        """One time and one value per key on each side.  Returns this
        rank's partition.  The inputs are never written."""
        if not (lkeys.numel() == ltimes.numel() == lvals.numel()):
            raise ValueError("one left time and one left value per left key "
                             "required")
        if not (rkeys.numel() == rtimes.numel() == rvals.numel()):
            raise ValueError("one right time and one right value per right "
                             "key required")
        if ltimes.dtype != rtimes.dtype:
            raise TypeError(
                "both sides need one time dtype, got "
                f"{ltimes.dtype} and {rtimes.dtype}")
        if ltimes.dtype == torch.float64 and self.tolerance is not None:
            raise TypeError("a tolerance needs int64 times, got float64")

        left = self._arrange.run(lkeys, ltimes, lvals)
        right = self._arrange.run(rkeys, rtimes, rvals)
        lk = _row_keys(left)
        ri = ops.asof_sorted(lk, left.order, _row_keys(right), right.order,
                             self.direction, self.tolerance,
                             self.allow_exact)
        if self.how == "inner":
            li = torch.nonzero(ri >= 0).squeeze(1)  # the host sync
            ri = ri.index_select(0, li)
            return AsofResult(lk.index_select(0, li),
                              left.order.index_select(0, li),
                              left.values.index_select(0, li),
                              right.order.index_select(0, ri),
                              right.values.index_select(0, ri), None)
        matched = ri >= 0
        if right.order.numel():
            at = ri.clamp(min=0)
            # filled as int64 views: the unmatched rows are all-zero bits
            rt = right.order.index_select(0, at)
            rv = right.values.index_select(0, at)
            rt.view(torch.int64).masked_fill_(~matched, 0)
            rv.view(torch.int64).masked_fill_(~matched, 0)
        else:
            rt = torch.zeros(ri.numel(), dtype=rtimes.dtype, device=ri.device)
            rv = torch.zeros(ri.numel(), dtype=rvals.dtype, device=ri.device)
        return AsofResult(lk, left.order, left.values, rt, rv, matched)
