"""CPU self-check of the case generators in radix_common and bucket_common:
the properties the GPU tests rely on really hold, and the sort cases pass
through the CPU tier against the same oracle.  Needs no GPU."""

import numpy as np
import pytest
import torch

import bucket_common as bc
import radix_common as rc


# ------------------------------------------------------------ sort cases
def test_case_lists_cover_what_they_claim():
    sizes = {n for _, n, _ in rc.FULL_CASES}
    assert sizes >= set(rc.SIZES)
    assert {b for _, _, b in rc.FULL_CASES} == set(rc.BITS)
    assert {f for f, _, _ in rc.FULL_CASES} == set(rc.FAMILIES)
    assert len(set(rc.FULL_CASES)) == len(rc.FULL_CASES)
    assert {rc.T - 1, rc.T, rc.T + 1} <= sizes
    assert {n for _, n, _ in rc.VARIANT_CASES} == {
        rc.T - 1, rc.T, rc.T + 1, 3 * rc.T + 17}
    assert {b for _, _, b in rc.VARIANT_CASES} == {20, 64}
    assert {f for f, _, _ in rc.VARIANT_CASES} == {"random", "equal",
                                                   "dupes"}


@pytest.mark.parametrize(
    "case", list(dict.fromkeys(rc.FULL_CASES + rc.VARIANT_CASES)),
    ids=rc.case_id)
def test_sort_case_properties_and_cpu_tier(case):
    from mapreduce_amd.ops import _cpu
    f, n, bits = case
    keys = rc.make_keys(case)
    np.testing.assert_array_equal(keys, rc.make_keys(case))  # seeded
    assert keys.size == n
    if bits < 64:
        assert int(keys.max()) < 2 ** bits
    if f == "random" and n >= 64:
        top = keys >> np.uint64(bits - 1)
        assert top.max() == 1 and top.min() == 0
    if f == "equal":
        assert np.unique(keys).size == 1
    if f == "alternating" and n >= 2:
        a, b = int(keys[0]), int(keys[1])
        assert a > b
        for p in range((bits + 7) // 8):
            assert (a >> 8 * p) & 0xFF != (b >> 8 * p) & 0xFF
    if f == "sorted" and n >= 64:
        assert (np.diff(keys.astype(object)) >= 0).all()
    if f == "reverse" and n >= 64:
        assert (np.diff(keys.astype(object)) <= 0).all()
        assert keys[0] != keys[-1]
    if f == "ones" and n >= 64:
        share = (keys == rc.EMPTY).mean()
        assert 0.02 < share < 0.25
    if f == "dupes":
        assert np.unique(keys).size <= 64
        if n >= 3 * rc.T and bits >= 8:
            assert np.unique(keys).size >= 32
            assert np.bincount(np.unique(keys, return_inverse=True)[1]
                               ).max() > 64  # runs longer than a wave
    if f.startswith("byte"):
        p = int(f[4:])
        diff = np.bitwise_or.reduce(keys ^ keys[0])
        assert diff != 0 and diff & ~np.uint64(0xFF << 8 * p) == 0
        assert np.unique(keys).size > 100
        bg = [(rc.BACKGROUND >> 8 * q) & 0xFF for q in range(8)]
        assert len(set(bg)) == 8

    ek, order = rc.oracle(keys)
    assert (np.diff(ek.astype(object)) >= 0).all()
    assert sorted(order.tolist()) == list(range(n))
    ties = ek[1:] == ek[:-1]
    assert (np.diff(order)[ties] > 0).all()  # stable
    k = torch.from_numpy(keys.view(np.int64).copy())
    v = torch.arange(n, dtype=torch.int64)
    sk, sv = _cpu.sort_pairs(k, v, bits)
    np.testing.assert_array_equal(sk.numpy().view(np.uint64), ek)
    np.testing.assert_array_equal(sv.numpy(), order)
    col = rc.make_column(case)
    assert col.shape == (n,) and col.dtype == np.int64


# ---------------------------------------------------------- bucket cases
def all_bucket_cases():
    return [bc.case_overflow(s) for s in bc.SLOT_SIZES] + bc.host_cases()


@pytest.mark.parametrize("case", all_bucket_cases(), ids=lambda c: c.name)
def test_bucket_case_is_well_formed(case):
    n = case.hashes.size
    assert case.pos.shape == (n,)
    np.testing.assert_array_equal(case.pos >> 16, np.arange(n))
    assert case.off.size >= (case.nbuckets if case.stride
                             else case.nbuckets + 1)
    for a, b in case.ranges():
        assert 0 <= a <= b <= n  # the kernel reads nothing outside
    if case.stride:
        assert n >= case.nbuckets * case.stride
    # at least twice the distinct keys, so ht_add always finds a free slot
    assert case.table_slots >= 2 * len(case.expect)
    assert case.table_slots >= 2 * case.capacity
    assert int(bc.EMPTY) not in case.expect
    assert all(c > 0 for c in case.expect.values())


def test_raw_layout_has_the_bucket_sizes_it_claims():
    raw = bc.raw_layout_keys()
    assert raw.size == 20_000
    real = raw[raw != bc.EMPTY]
    assert 0 < raw.size - real.size < 100
    assert 2900 <= np.unique(real).size <= 3000
    sizes = np.bincount((real >> np.uint64(56)).astype(np.int64),
                        minlength=256)
    assert (sizes == 0).any()  # an empty bucket
    assert (sizes == 1).any()
    assert ((sizes > 0) & (sizes < 16)).sum() > 50  # per = 1 at 16 slices
    assert (sizes % 3 != 0).sum() > 100
    assert sizes.max() > 16 * 4


@pytest.mark.parametrize("slots", bc.SLOT_SIZES)
def test_overflow_case_overflows_one_slice(slots):
    case = bc.case_overflow(slots)
    assert case.nbuckets == 1 and case.slices == 1
    assert len(case.expect) == 3 * slots > slots
    assert set(case.expect.values()) == {1, 2, 3}


def test_probe_chain_case_collides_in_lds_only():
    case = bc.case_probe_chain()
    keys = sorted(case.expect)
    assert len(keys) == 200 > bc.PROBE_LIMIT
    assert set(case.expect.values()) == {5}
    assert case.nbuckets == 1 and case.slices == 1
    for slots in bc.SLOT_SIZES:
        assert {bc.lds_slot(k, slots) for k in keys} == {0}
        assert len(keys) < slots  # the LDS table itself is far from full
    first = {bc.global_slot(k, case.table_slots) for k in keys}
    assert len(first) == len(keys)


def test_hot_key_and_pad_cases():
    hot = bc.case_hot_key()
    assert sorted(hot.expect.values()) == [1] * 10 + [100_000]
    pads = bc.case_pads()
    inner = pads.hashes[:5000] == bc.EMPTY
    assert 1000 < inner.sum() < 2000 and not inner.all()
    assert (pads.hashes[5000:] == bc.EMPTY).all()
    assert pads.hashes.size == 5700
    assert sum(pads.expect.values()) == 5000 - inner.sum()


def test_degenerate_cases_are_degenerate():
    by = {c.name: c for c in bc.cases_degenerate()}
    lens = {name: [b - a for a, b in c.ranges()] for name, c in by.items()}
    assert lens["len0_len1_rest"][:2] == [0, 1]
    assert lens["offset_len0_len1"][:2] == [0, 1]
    assert lens["all_empty_buckets"] == [0, 0, 0]
    assert lens["single_element"] == [1]
    assert {c.nbuckets for c in by.values()} == {1, 3}
    for name in ("offset_range", "offset_len0_len1"):
        c = by[name]
        a, b = c.ranges()[0][0], c.ranges()[-1][1]
        assert a > 0 and b < c.hashes.size
        outside = np.concatenate([c.hashes[:a], c.hashes[b:]])
        assert (outside != bc.EMPTY).all()
        whole = bc.oracle(c.hashes, [0, c.hashes.size], 1, 0)
        assert whole != c.expect  # reading outside the range would show


def test_stride_case_overstates_one_length():
    case = bc.case_stride()
    s = case.stride
    assert case.off[2] > s  # stated length exceeds the stride
    assert case.ranges()[2] == (2 * s, 3 * s)  # the oracle counts `stride`
    assert (case.off[[0, 1, 3]] < s).all() and case.off[1] == 0
    assert (case.hashes != bc.EMPTY).all()  # the gaps hold real-looking keys
    assert sum(case.expect.values()) == 300 + s + 1
    unclamped = bc.Case("u", case.hashes, [0, 300], 1, 1).expect
    a = 2 * s
    unclamped.update(case.hashes[a:a + int(case.off[2])].tolist())
    unclamped.update(case.hashes[3 * s:3 * s + 1].tolist())
    assert unclamped != case.expect  # a missing clamp would show
