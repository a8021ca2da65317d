"""Shared pieces of the bucket_count tests (not a test module): host-built
(hashes, pos, bucket_off) cases, the Counter oracle and the GPU harness.

Element i of a case carries pos = i << 16 | 1, so an extracted exemplar p
can be checked against the input: hashes[p >> 16] must be its key."""

import collections

import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
SLOT_SIZES = (512, 1024, 2048)
ILPS = (1, 2, 4)
PROBE_LIMIT = 64  # LDS probes of bucket_count_kernel before the fallback


def next_pow2(n):  # ops._next_pow2: HashTable(c).cap == next_pow2(2 * c)
    return 1 << max(4, int(np.ceil(np.log2(max(n, 2)))))


def lds_slot(k, slots):  # start slot in bucket_count_kernel's LDS table
    return (k ^ (k >> 17)) & (slots - 1)


def global_slot(k, cap):  # first_slot() of the global table
    return (k ^ (k >> 32)) & (cap - 1)


def positions(n):
    return (np.arange(n, dtype=np.int64) << 16) | 1


def distinct_keys(rng, m):
    """m distinct real keys (never all-ones, nor all-ones minus 1, under
    which insert_count files an all-ones key)."""
    k = np.unique(rng.integers(0, 2 ** 64 - 3, size=2 * m + 16,
                               dtype=np.uint64, endpoint=True))
    assert k.size >= m
    return rng.permutation(k)[:m]


class Case:
    """One bucket_count call.  stride == 0: bucket b is
    hashes[off[b]:off[b + 1]]; stride > 0: `off` holds lengths and bucket b
    is hashes[b * stride : b * stride + min(off[b], stride)]."""

    def __init__(self, name, hashes, off, nbuckets, slices, stride=0,
                 capacity=None):
        self.name = name
        self.hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
        self.pos = positions(self.hashes.size)
        self.off = np.asarray(off, dtype=np.int64)
        self.nbuckets = nbuckets
        self.slices = slices
        self.stride = stride
        self.expect = oracle(self.hashes, self.off, nbuckets, stride)
        # HashTable doubles its capacity argument: >= 2 x distinct slots
        self.capacity = capacity or max(len(self.expect), 8)

    @property
    def table_slots(self):
        return next_pow2(2 * self.capacity)

    def ranges(self):
        return bucket_ranges(self.off, self.nbuckets, self.stride)


def bucket_ranges(off, nbuckets, stride):
    if stride > 0:
        return [(b * stride, b * stride + min(int(off[b]), stride))
                for b in range(nbuckets)]
    return [(int(off[b]), int(off[b + 1])) for b in range(nbuckets)]


def oracle(hashes, off, nbuckets, stride):
    """Counter of the real keys inside the described ranges."""
    c = collections.Counter()
    for a, b in bucket_ranges(off, nbuckets, stride):
        seg = hashes[a:b]
        c.update(seg[seg != EMPTY].tolist())
    return c


# ------------------------------------------------------------------ cases
def raw_layout_keys():
    """Case 1 input, before radix_bucketize: 20 000 keys over 3000 distinct
    values.  2600 of them are frequent and sit in top bytes 0..127; 400
    occur once, in top bytes 128..255, so those buckets hold fewer
    elements than 16 slices (per = 1, trailing empty slices) and some are
    empty.  A few pads ride along for the bucketize to drop."""
    rng = np.random.default_rng(20_000)
    pool = distinct_keys(rng, 3000)
    low = np.uint64((1 << 56) - 1)
    top = np.concatenate([rng.integers(0, 128, size=2600),
                          rng.integers(128, 256, size=400)]).astype(np.uint64)
    pool = (pool & low) | (top << np.uint64(56))
    pool = np.unique(pool)
    counts = np.where(pool >> np.uint64(56) < 128, 7, 1)
    np.add.at(counts, rng.integers(0, 2600, size=19_960 - counts.sum()), 1)
    keys = np.repeat(pool, counts)
    keys = np.concatenate([keys, np.full(40, EMPTY)])
    return rng.permutation(keys)


def case_overflow(slots):
    """Case 2: 3 * slots distinct keys, 1..3 copies each, one bucket, one
    slice: at most `slots` fit the LDS table, the rest take ht_add."""
    rng = np.random.default_rng(slots + 2)
    pool = distinct_keys(rng, 3 * slots)
    keys = rng.permutation(np.repeat(pool, rng.integers(1, 4, pool.size)))
    return Case(f"overflow{slots}", keys, [0, keys.size], 1, 1)


def case_probe_chain():
    """Case 3: 200 keys j << 40, five copies each, one slice.  All start
    at LDS slot 0 for every table size, so the chain passes the probe limit
    with the LDS table nearly empty; the 2^16-slot global table spreads
    them (first slot j << 8)."""
    rng = np.random.default_rng(3)
    pool = np.arange(1, 201, dtype=np.uint64) << np.uint64(40)
    keys = rng.permutation(np.repeat(pool, 5))
    return Case("probe_chain", keys, [0, keys.size], 1, 1, capacity=1 << 15)


def case_hot_key():
    """Case 4: 100 000 copies of one key and 10 others, one slice."""
    rng = np.random.default_rng(4)
    pool = distinct_keys(rng, 11)
    keys = np.full(100_010, pool[0])
    keys[rng.choice(keys.size, size=10, replace=False)] = pool[1:]
    return Case("hot_key", keys, [0, keys.size], 1, 1)


def case_pads():
    """Case 5: pads at random inside the range and as a tail run."""
    rng = np.random.default_rng(5)
    pool = distinct_keys(rng, 300)
    keys = pool[rng.integers(0, 300, size=5000)]
    keys[rng.random(5000) < 0.3] = EMPTY
    keys = np.concatenate([keys, np.full(700, EMPTY)])
    return Case("pads", keys, [0, keys.size], 1, 3)


def _some_keys(seed, n, distinct):
    rng = np.random.default_rng(seed)
    return distinct_keys(rng, distinct)[rng.integers(0, distinct, size=n)]


def cases_degenerate():
    """Case 6: empty and one-element buckets, 1 and 3 buckets with
    hand-written offsets, ranges that start past 0 and end before the
    array does (the keys outside are real-looking and must not count)."""
    k = _some_keys(6, 900, 150)
    return [
        Case("one_bucket", k, [0, 900], 1, 1),
        Case("one_bucket_sliced", k, [0, 900], 1, 7),
        Case("len0_len1_rest", k, [0, 0, 1, 900], 3, 4),
        Case("offset_range", k, [137, 600], 1, 2),
        Case("offset_len0_len1", k, [100, 100, 101, 650], 3, 5),
        Case("single_element", k, [899, 900], 1, 16),
        Case("all_empty_buckets", k, [5, 5, 5, 5], 3, 2),
    ]


STRIDE = 512


def case_stride():
    """Case 7: lengths, not offsets.  Bucket 2 states 90 more than the
    stride: unclamped it would run into bucket 3's region, whose one
    element and the garbage after it would then be counted."""
    k = _some_keys(7, 4 * STRIDE, 200)
    return Case("stride", k, [300, 0, STRIDE + 90, 1], 4, 3, stride=STRIDE)


def host_cases():
    """Every host-built case that does not depend on the LDS size."""
    return ([case_probe_chain(), case_hot_key(), case_pads(), case_stride()]
            + cases_degenerate())


# ---------------------------------------------------------------- harness
def u64_dev(a, dev):
    import torch
    return torch.from_numpy(a.view(np.int64).copy()).to(dev)


def extracted(ht, hashes, exemplar):
    """extract() -> {key: count}; keys unique, and with `exemplar` every
    exemplar points at an input element holding its key."""
    k, v, p = ht.extract()
    keys = k.cpu().numpy().view(np.uint64)
    assert np.unique(keys).size == keys.size, "a key was extracted twice"
    assert not (keys == EMPTY).any()
    if exemplar:
        pp = p.cpu().numpy()
        assert pp.size == keys.size
        assert ((pp & 0xFFFF) == 1).all()
        idx = pp >> 16
        assert ((idx >= 0) & (idx < hashes.size)).all()
        np.testing.assert_array_equal(hashes[idx], keys)
    else:
        assert p.numel() == 0
    return dict(zip(keys.tolist(), v.cpu().tolist()))


def run_case(case, dev, slots, exemplar):
    import torch
    from mapreduce_amd import ops
    ht = ops.HashTable(case.capacity, dev, exemplar=exemplar)
    assert ht.cap == case.table_slots >= 2 * len(case.expect)
    h = u64_dev(case.hashes, dev)
    p = torch.from_numpy(case.pos.copy()).to(dev)
    off = torch.from_numpy(case.off.copy()).to(dev)
    ops.ext().bucket_count(h, p, off, case.nbuckets, case.slices, ht.tkeys,
                           ht.tvals, ht.texm, case.stride, slots)
    assert extracted(ht, case.hashes, exemplar) == dict(case.expect)
