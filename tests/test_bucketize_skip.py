"""Pad-dropping bucketize (radix_bucketize with skip_empty) and the
spill drain built on it: NumPy oracle at tile-edge sizes and every pad
layout the spill allocator can produce, the default (keep-everything) mode
on all-ones keys, and an end-to-end word count whose spill provably holds
both real records and pads."""

import collections
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
T = 256 * (4 if os.environ.get("MR_RS_ITEMS") == "4" else 8)
SIZES = [0, 1, 63, 64, T - 1, T, T + 1, 3 * T + 17]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mapreduce_amd import ops
    ops.require_gpu_ext()
    return torch.device("cuda:0")


# ---------------------------------------------------------------- inputs
def real_keys(rng, n, heavy=False):
    # high is exclusive: the all-ones pattern is never a real key
    k = rng.integers(0, 2 ** 64 - 1, size=n, dtype=np.uint64)
    if heavy:  # 90 % share one top byte: digit runs longer than a wave
        same = rng.random(n) < 0.9
        k[same] = (k[same] & np.uint64((1 << 56) - 1)) | np.uint64(0xA7 << 56)
    return k


def mask_none(rng, n):
    return np.zeros(n, dtype=bool)


def mask_all(rng, n):
    return np.ones(n, dtype=bool)


def mask_chunk_tails(rng, n):
    """Runs of 1..T-1 pads ending on multiples of T (allocator layout);
    the first two runs pin the extreme lengths."""
    m = np.zeros(n, dtype=bool)
    for j, end in enumerate(range(T, n + 1, T)):
        run = (1, T - 1)[j] if j < 2 else int(rng.integers(1, T))
        m[end - run:end] = True
    return m


def mask_whole_tile(rng, n):
    m = np.zeros(n, dtype=bool)
    m[T:2 * T] = True  # tile 1 of >= 3: entirely pads
    return m


def mask_final_partial(rng, n):
    m = np.zeros(n, dtype=bool)
    if n:
        start = (n - 1) // T * T
        m[start:n] = rng.random(n - start) < 0.5
        m[n - 1] = True
    return m


def mask_isolated(rng, n):
    m = np.zeros(n, dtype=bool)
    if n:
        m[rng.integers(0, n, size=max(1, n // 32))] = True
    return m


LAYOUTS = {
    "none": mask_none, "all": mask_all, "chunk_tails": mask_chunk_tails,
    "final_partial": mask_final_partial, "isolated": mask_isolated,
}
CASES = ([(n, name) for n in SIZES for name in LAYOUTS]
         + [(3 * T, "whole_tile"), (3 * T + 17, "whole_tile")])
ALL_LAYOUTS = dict(LAYOUTS, whole_tile=mask_whole_tile)


def make_input(n, layout, heavy=False):
    rng = np.random.default_rng(1000003 * n + sum(map(ord, layout)) + heavy)
    keys = real_keys(rng, n, heavy)
    keys[ALL_LAYOUTS[layout](rng, n)] = EMPTY
    return keys


# ---------------------------------------------------------------- oracle
def oracle(keys, skip):
    idx = np.arange(keys.size, dtype=np.int64)
    if skip:
        idx = idx[keys != EMPTY]
    k = keys[idx]
    digit = (k >> np.uint64(56)).astype(np.int64)
    order = np.argsort(digit, kind="stable")
    totals = np.bincount(digit, minlength=256).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(totals)]).astype(np.int64)
    return k[order], idx[order], totals, off


def to_dev(keys, dev, vdtype=torch.int64):
    k = torch.from_numpy(keys.view(np.int64).copy()).to(dev)
    v = torch.arange(keys.size, dtype=vdtype, device=dev)
    return k, v


def check(kout, vout, off, keys, skip):
    ek, ev, _, eoff = oracle(keys, skip)
    assert kout.numel() == keys.size and vout.numel() == keys.size
    off = off.cpu().numpy()
    np.testing.assert_array_equal(off, eoff)
    m = int(eoff[-1])
    np.testing.assert_array_equal(
        kout[:m].cpu().numpy().view(np.uint64), ek)
    np.testing.assert_array_equal(
        vout[:m].cpu().numpy().astype(np.int64), ev)


# ----------------------------------------------------------------- tests
@pytest.mark.parametrize("n,layout", CASES)
def test_bucketize_skip_matches_oracle(dev, n, layout):
    from mapreduce_amd import ops
    keys = make_input(n, layout)
    k, v = to_dev(keys, dev)
    kout, vout, off = ops.ext().radix_bucketize(k, v, 56, True)
    assert off.numel() == 257
    check(kout, vout, off, keys, skip=True)


@pytest.mark.parametrize("ntiles", [300, 1024 + 2])
def test_bucketize_skip_many_tiles(dev, ntiles):
    """The native row scan walks 4 x 256 tiles per round: 300 tiles uses
    its second sub-chunk, 1026 tiles carries into a second round."""
    from mapreduce_amd import ops
    keys = make_input((ntiles - 1) * T + 5, "chunk_tails")
    k, v = to_dev(keys, dev)
    kout, vout, off = ops.ext().radix_bucketize(k, v, 56, True)
    check(kout, vout, off, keys, skip=True)


@pytest.mark.parametrize("layout", sorted(ALL_LAYOUTS))
def test_bucketize_skip_u32_payload(dev, layout):
    from mapreduce_amd import ops
    keys = make_input(3 * T + 17, layout)
    k, v = to_dev(keys, dev, torch.int32)
    kout, vout, off = ops.ext().radix_bucketize(k, v, 56, True)
    assert vout.dtype == torch.int32
    check(kout, vout, off, keys, skip=True)


@pytest.mark.parametrize("n", [T + 1, 3 * T + 17])
@pytest.mark.parametrize("layout", ["chunk_tails", "isolated"])
def test_default_mode_keeps_all_ones_keys(dev, n, layout):
    """Skip off: all-ones keys are data (TeraSort), kept in stable order;
    today's positional radix_pass call and radix_bucketize agree."""
    from mapreduce_amd import ops
    keys = make_input(n, layout)
    assert (keys == EMPTY).any()
    k, v = to_dev(keys, dev)
    pk, pv, totals = ops.ext().radix_pass(k, v, 56)
    ek, ev, etot, eoff = oracle(keys, skip=False)
    assert int(eoff[-1]) == n
    np.testing.assert_array_equal(totals.cpu().numpy(), etot)
    np.testing.assert_array_equal(pk.cpu().numpy().view(np.uint64), ek)
    np.testing.assert_array_equal(pv.cpu().numpy(), ev)
    bk, bv, off = ops.ext().radix_bucketize(k, v, 56)
    check(bk, bv, off, keys, skip=False)
    assert torch.equal(bk, pk) and torch.equal(bv, pv)


@pytest.mark.parametrize("layout", ["none", "chunk_tails", "isolated"])
def test_heavy_digit(dev, layout):
    from mapreduce_amd import ops
    keys = make_input(3 * T + 17, layout, heavy=True)
    k, v = to_dev(keys, dev)
    kout, vout, off = ops.ext().radix_bucketize(k, v, 56, True)
    check(kout, vout, off, keys, skip=True)
    _, _, etot, _ = oracle(keys, True)
    assert etot[0xA7] > 64 * 3  # the run really is longer than a wave


# ------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def corpus():
    """~300 KB, ~20k distinct words, uniform draws (seeded)."""
    rng = np.random.default_rng(4242)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    vocab = set()
    while len(vocab) < 20000:
        ln = int(rng.integers(3, 10))
        vocab.add(bytes(letters[rng.integers(0, 26, size=ln)]))
    vocab = sorted(vocab)
    draws = rng.integers(0, len(vocab), size=46000)
    seps = [b" ", b"\n", b"\t", b"  "]
    parts = []
    for i, d in enumerate(draws):
        parts.append(vocab[d])
        parts.append(seps[i % 4] if i % 7 else seps[(i // 7) % 4])
    data = b"".join(parts)
    assert 250_000 < len(data) < 400_000
    # the LDS cache (2048 entries) must miss: one block's share of the
    # text already holds more distinct words than it has slots
    assert len(set(data[:137 * 1024].split())) > 2048
    return data, collections.Counter(data.split())


def slice_settings():
    from mapreduce_amd.gpu.wordcount import DEFAULT_BUCKET_SLICES
    return sorted({1, DEFAULT_BUCKET_SLICES})


@pytest.mark.parametrize("slices", slice_settings())
def test_wordcount_streaming_drops_pads(dev, corpus, monkeypatch, slices):
    from mapreduce_amd.gpu.wordcount import WordCountJob
    data, expect = corpus
    monkeypatch.setenv("MR_BUCKET_SLICES", str(slices))
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    job = WordCountJob(dev, vocab_estimate=40000, mode="streaming")
    job.begin_map(text)
    job.map_split(0, text.numel())
    reserved = int(job._spill_c.item())
    pads = int((job._spill_h[:reserved] == -1).sum().item())
    assert 0 < pads < reserved, (pads, reserved)  # real records AND pads
    nwords = job.finish_map()
    res = job.shuffle_reduce(nwords)
    assert res.nwords == sum(expect.values())
    got = res.to_host()
    assert len(got) == len(expect)
    assert collections.Counter(dict(got)) == expect
