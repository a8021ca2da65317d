"""Distributed group-by with the values of every key in order: the general
reduce, reducefn(key, values), for reducers that need the whole value list
(median and percentiles, the k largest, the number of distinct values).

    job = GroupedValuesJob(device)
    res = job.run(keys, vals)      # GroupedResult(keys, offsets, values)
    res.quantiles([(1, 2), (99, 100)])

Keys are i64 (u64 bit order); the value column is i64 or f64 and rides
every sort and exchange as its int64 view.  The order of values is that of
ops.group_order_keys: -0.0 equals +0.0 and every NaN is one value above
+inf; the stored bits come through unaltered.

Single rank: one ops.sort_by_key(keys, vals), then
ops.sort_values_in_groups (ops/hip/group.hip).

Multi-rank, the shape of JoinJob for one side: sort locally,
mulhi-partition (rank r owns the keys with mulhi(key, world) == r), ONE
count exchange, one all-to-all of the keys and one of the values, a re-sort
by key and the sort within groups.  The exchange is single-round: a rank's
whole partition must fit in its memory.

combine trims the value lists, before the exchange and again after it, so
the result does not depend on the world size (up to which of several values
with one order key is kept):
    ("topk", k) / ("bottomk", k)   the k largest / smallest values per key
    "distinct"                     one value per order key
Under combine one key's rows no longer all cross the wire; without it they
do.
"""

from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

import torch

from .. import ops
from . import dist as dx


def parse_combine(combine):
    """-> None, ("distinct", 0), ("topk", k) or ("bottomk", k)."""
    if combine is None:
        return None
    if combine == "distinct":
        return ("distinct", 0)
    if (isinstance(combine, (tuple, list)) and len(combine) == 2
            and combine[0] in ("topk", "bottomk")
            and isinstance(combine[1], int)
            and not isinstance(combine[1], bool) and combine[1] >= 1):
        return (combine[0], int(combine[1]))
    raise ValueError(
        "combine must be None, 'distinct', ('topk', k) or ('bottomk', k) "
        f"with k >= 1, got {combine!r}")


class GroupedResult(NamedTuple):
    keys: torch.Tensor     # i64[nseg], ascending in u64 order, unique
    offsets: torch.Tensor  # i64[nseg + 1]: key s owns values[o[s]:o[s + 1]]
    values: torch.Tensor   # the input's dtype, ordered within each key

    def counts(self) -> torch.Tensor:
        return self.offsets[1:] - self.offsets[:-1]

    def quantiles(self, fracs, interpolation: str = "lower") -> torch.Tensor:
        return ops.group_quantiles(self.offsets, self.values, fracs,
                                   interpolation)

    def median(self) -> torch.Tensor:
        """The lower median of each key."""
        return self.quantiles([(1, 2)])[:, 0]

    def topk(self, k: int, largest: bool = True):
        return ops.group_topk(self.offsets, self.values, k, largest)

    def distinct(self) -> torch.Tensor:
        """The number of distinct values of each key."""
        n = self.keys.numel()
        if not n:
            return self.counts()
        # the segment number of every row stands in for its key
        rows = torch.repeat_interleave(
            torch.arange(n, device=self.keys.device), self.counts(),
            output_size=self.values.numel())
        return ops.group_distinct(rows, self.values)

    def to_host(self) -> List[Tuple[int, list]]:
        """[(key as i64, [values ascending])] in key order."""
        off = self.offsets.cpu().tolist()
        vals = self.values.cpu().tolist()
        return [(k, vals[off[s]:off[s + 1]])
                for s, k in enumerate(self.keys.cpu().tolist())]


class GroupedValuesJob:
    def __init__(self, device, group=None, combine=None):
        self.device = torch.device(device)
        self.group = group
        self.rank, self.world = dx.world_info(group)
        self.combine = parse_combine(combine)

    def _shuffle(self, k, v):
        """Sorted rows -> this rank's partition, re-sorted by key."""
        counts = ops.partition_counts(k, self.world)
        recv = dx.exchange_counts(counts, self.group)
        sc = counts.cpu().tolist()
        rc = recv.cpu().tolist()
        k = dx.exchange(k, sc, rc, self.group)
        v = dx.exchange(v, sc, rc, self.group)
        return ops.sort_by_key(k, v)

    def _order(self, k, v):
        """Key-sorted rows -> (keys, values, ukeys, offsets), the values in
        order within each key and trimmed by combine."""
        uk, off = ops.group_by_key_sorted(k)
        v = ops.sort_values_in_groups(k, v, off)
        if self.combine is None or not k.numel():
            return k, v, uk, off
        what, kk = self.combine
        if what == "distinct":
            keep = ops.group_distinct_flags(k, v) != 0
        else:
            lens = off[1:] - off[:-1]
            row = torch.arange(k.numel(), device=k.device)
            if what == "topk":
                rank = torch.repeat_interleave(off[1:], lens,
                                               output_size=k.numel()) - row
                keep = rank <= kk
            else:
                rank = row - torch.repeat_interleave(off[:-1], lens,
                                                     output_size=k.numel())
                keep = rank < kk
        sel = torch.nonzero(keep).squeeze(1)
        k = k.index_select(0, sel)
        v = v.index_select(0, sel)
        uk, off = ops.group_by_key_sorted(k)
        return k, v, uk, off

    def run(self, keys: torch.Tensor, vals: torch.Tensor) -> GroupedResult:
        """One value per key; returns this rank's partition.  The inputs
        are never written."""
        if keys.numel() != vals.numel():
            raise ValueError("one value per key required")
        if vals.dtype not in (torch.int64, torch.float64):
            raise TypeError(
                f"vals must be int64 or float64, got {vals.dtype}")
        dt = vals.dtype
        k, v = ops.sort_by_key(keys, vals.view(torch.int64))
        collective = self.world > 1 or dx.force_collectives()
        if collective:
            if self.combine is not None:
                k, v, _, _ = self._order(k, v.view(dt))
                v = v.view(torch.int64)
            k, v = self._shuffle(k, v)
        k, v, uk, off = self._order(k, v.view(dt))
        return GroupedResult(uk, off, v)
