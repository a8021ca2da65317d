"""Spilled (key, offset<<16 | len) records of tokenize_v6.

The tokenizer no longer buffers a record's position: it rebuilds it where
the record is stored, from the window's start mask, the whitespace mask
and one saved long-word length.  What can break is therefore the (offset,
len) of a spilled record, so the records themselves are checked: each one
must point at a complete word of the text whose wordhash64 is its key, and
table counts plus records must add up to the Python split oracle.

Two launchers write records through the same loop.  The LDS-cached one
(tokenize_cache_spill, the word-count default) spills only what misses its
2048-slot, 2-probe per-block cache; which words those are depends on which
lane wins a slot, so that path is checked on whatever it spills (a dense
3-letter filler of ~6000 distinct words keeps every 4 KB tile near 1000
distinct words, i.e. misses in every tile).  The spill-all one
(tokenize_spill_v2, the inverted-index instantiation) spills every word,
so there every edge case below is required to show up with its exact
(offset, len)."""

import collections
import itertools

import numpy as np
import pytest
import torch

from mapreduce_amd.utils.tuple import wordhash64

pytestmark = pytest.mark.gpu

HT_EMPTY = (1 << 64) - 1
WS = frozenset(b" \t\n\v\f\r")
TILE = 4096
HALO = 64
# slack the chunked spill allocator may strand: <= 2048 blocks x 4 waves x
# one 2048-entry chunk (WordCountJob.begin_map sizes its spill the same way)
SLACK = 2048 * 4 * 2048


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mapreduce_amd import ops
    ops.require_gpu_ext()
    return torch.device("cuda:0")


def device_key(word: bytes) -> int:
    h = wordhash64(word)
    return HT_EMPTY - 1 if h == HT_EMPTY else h  # remap_key


# ------------------------------------------------------------------ inputs
def _vocab():
    rng = np.random.default_rng(20240)
    words = [bytes(t) for t in itertools.product(range(97, 123), repeat=3)]
    idx = rng.permutation(len(words))[:6000]
    return [words[i] for i in idx]


def _filler(nbytes: int, seed: int) -> bytearray:
    """nbytes of 'abc ' units (nbytes % 4 == 0), ~6000 distinct words."""
    assert nbytes % 4 == 0
    vocab = _vocab()
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, len(vocab), nbytes // 4)
    return bytearray(b"".join(vocab[i] + b" " for i in ids))


def _place(buf: bytearray, off: int, word: bytes, expect: list) -> None:
    """Overwrite buf so that `word` stands at `off`, bounded by spaces."""
    assert off >= 1 and off + len(word) + 1 <= len(buf)
    buf[off - 1] = 0x20
    buf[off:off + len(word)] = word
    buf[off + len(word)] = 0x20
    expect.append((off, word))


def _named(tag: str, length: int) -> bytes:
    w = tag.encode() + b"x" * length
    return w[:length]


def build_edge_text():
    """-> (text bytes, [(offset, word)] that must be found exactly)."""
    buf = _filler(24 * TILE, seed=1)
    expect = []
    # 1. eight one-byte words in one 16-byte window (maximum slot index),
    #    three windows with distinct letters
    for w, letters in enumerate((b"abcdefgh", b"ijklmnop", b"QRSTUVWX")):
        base = 2 * TILE + 160 + 16 * w
        buf[base - 1] = 0x20
        for i, c in enumerate(letters):
            buf[base + 2 * i] = c
            buf[base + 2 * i + 1] = 0x20
            expect.append((base + 2 * i, bytes([c])))
    # 2. a word that starts at byte 15 of a window
    _place(buf, 3 * TILE + 320 + 15, b"Start15", expect)
    # 3. lengths on either side of the 32-byte register window, at window
    #    offsets 0, 7 and 15: offset + len <= 31 takes the length from the
    #    whitespace mask, anything longer from the saved long-word length
    at = 4 * TILE + 64
    for length in (16, 17, 31, 32, 33):
        for s in (0, 7, 15):
            _place(buf, at + s, _named(f"L{length}s{s}", length), expect)
            at += 64
    # 4. a 40-byte word that is the last of three starts in its window,
    #    with two words before it in the same window
    base = 6 * TILE + 480
    _place(buf, base, b"p1", expect)
    _place(buf, base + 3, b"q2", expect)
    _place(buf, base + 6, _named("Forty", 40), expect)
    # 5. words across the tile edge and the halo edge, short and long
    _place(buf, 8 * TILE - 5, b"TileEdge12ch", expect)
    _place(buf, 8 * TILE + HALO - 4, b"HaloEdge10", expect)
    _place(buf, 9 * TILE - 20, _named("PastHalo", 100), expect)
    _place(buf, 10 * TILE + HALO - 10, _named("LongHalo", 45), expect)
    _place(buf, 11 * TILE - 1, b"Zlastbyte", expect)
    # 6. length not a multiple of 16, last word runs to the end of text
    del buf[len(buf) - 9:]
    tail = b"EndWord"
    buf[len(buf) - len(tail) - 1] = 0x20
    buf[len(buf) - len(tail):] = tail
    expect.append((len(buf) - len(tail), tail))
    assert len(buf) % 16 != 0 and buf[-1] not in WS
    text = bytes(buf)
    for off, w in expect:  # the placements did not overwrite each other
        assert text[off:off + len(w)] == w
        assert text[off - 1] in WS
        assert off + len(w) == len(text) or text[off + len(w)] in WS
    return text, expect


@pytest.fixture(scope="module")
def edge():
    text, expect = build_edge_text()
    return text, expect, collections.Counter(text.split())


def to_dev(data: bytes, dev):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)


def u64_list(t: torch.Tensor):
    return t.cpu().numpy().view(np.uint64).tolist()


# ----------------------------------------------------------------- checker
def check_records(text: bytes, keys, pos, weights=None):
    """Every non-pad record is a complete word of `text` with the right
    key.  -> (Counter of the words, set of (offset, len))."""
    n = len(text)
    got = collections.Counter()
    where = set()
    for i, (k, p) in enumerate(zip(keys, pos)):
        if k == HT_EMPTY:
            continue
        off, ln = p >> 16, p & 0xFFFF
        assert ln >= 1 and off + ln <= n, (off, ln)
        w = text[off:off + ln]
        assert not WS.intersection(w), (off, ln, w)
        assert off == 0 or text[off - 1] in WS, (off, ln, w)
        assert off + ln == n or text[off + ln] in WS, (off, ln, w)
        assert device_key(w) == k, (off, ln, w)
        got[w] += 1 if weights is None else weights[i]
        where.add((off, ln))
    return got, where


def run_cache_spill(dev, text: bytes, cuts=None):
    """tokenize_cache_spill over `text` (one launch per [s, e) of cuts).
    -> (record keys, record pos, table keys, table counts, table pos,
    nwords)."""
    from mapreduce_amd import ops
    t = to_dev(text, dev)
    table = ops.make_table(1 << 14, dev)
    cuts = cuts or [(0, len(text))]
    cap = len(text) // 2 + 16 + len(cuts) * SLACK
    opts = dict(dtype=torch.int64, device=dev)
    sh = torch.empty(cap, **opts)
    sp = torch.empty(cap, **opts)
    sc = torch.zeros(1, **opts)
    nw = torch.zeros(1, **opts)
    for s, e in cuts:
        ops.ext().tokenize_cache_spill(t[s:e], s, table.tkeys, table.tvals,
                                       table.texm, cap, nw, sh, sp, sc)
    n = int(sc.item())
    assert n <= cap
    tk, tv, tp = table.extract()
    return (u64_list(sh[:n]), u64_list(sp[:n]), u64_list(tk),
            tv.cpu().tolist(), u64_list(tp), int(nw.item()))


def run_spill_all(dev, text: bytes, start: int = 0):
    from mapreduce_amd import ops
    t = to_dev(text, dev)
    cap = len(text) // 2 + 16 + 2048 * 4 * 512
    k, p, c, nw = ops.ext().tokenize_spill_v2(t[start:], start, cap)
    n = int(c.item())
    assert n <= cap
    return u64_list(k[:n]), u64_list(p[:n]), int(nw.item())


# ------------------------------------------------------------ record tests
def test_cache_spill_records(dev, edge):
    text, _, oracle = edge
    rk, rp, tk, tv, tp, nw = run_cache_spill(dev, text)
    spilled, _ = check_records(text, rk, rp)
    tabled, _ = check_records(text, tk, tp, weights=tv)
    print("cache path: records", len(rk), "real", sum(spilled.values()),
          "table entries", len(tk))
    assert sum(spilled.values()) > 0, "the text was built to spill"
    assert spilled + tabled == oracle
    assert nw == sum(oracle.values())


def test_spill_all_records(dev, edge):
    text, expect, oracle = edge
    rk, rp, nw = run_spill_all(dev, text)
    spilled, where = check_records(text, rk, rp)
    assert spilled == oracle
    assert nw == sum(oracle.values())
    missing = [(o, w) for o, w in expect if (o, len(w)) not in where]
    assert not missing, missing


def test_length_clamp(dev):
    word = b"x" * 70_000
    text = b"ab " + word + b" cd"
    want = (3, 0xFFFF, device_key(word))
    # spill-all: the long word is a record
    rk, rp, nw = run_spill_all(dev, text)
    recs = {(p >> 16, p & 0xFFFF, k) for k, p in zip(rk, rp) if k != HT_EMPTY}
    assert recs == {(0, 2, device_key(b"ab")), want,
                    (len(text) - 2, 2, device_key(b"cd"))}
    assert nw == 3
    # cached: it is a record or a table exemplar, with the same position
    rk, rp, tk, tv, tp, nw = run_cache_spill(dev, text)
    recs = {(p >> 16, p & 0xFFFF, k) for k, p in zip(rk, rp) if k != HT_EMPTY}
    recs |= {(p >> 16, p & 0xFFFF, k) for k, p in zip(tk, tp)}
    assert want in recs
    assert nw == 3 and len(recs) == 3


def test_pos_base_offsets_are_absolute(dev, edge):
    from mapreduce_amd.gpu.wordcount import WordCountJob
    text, expect, oracle = edge
    cut = next(c for c in range(7 * TILE + 100, len(text))
               if text[c - 1] in WS and text[c] not in WS and c % 16 not in (0, 8))
    # the job's own phase API: two launches appending to one spill
    job = WordCountJob(dev, vocab_estimate=8000)
    job.begin_map(to_dev(text, dev), expected_launches=2)
    job.map_split(0, cut)
    job.map_split(cut, len(text))
    n = int(job._spill_c.item())
    assert n <= job._spill_cap
    spilled, _ = check_records(text, u64_list(job._spill_h[:n]),
                               u64_list(job._spill_p[:n]))
    tk, tv, tp = job.table.extract()
    tabled, _ = check_records(text, u64_list(tk), u64_list(tp),
                              weights=tv.cpu().tolist())
    assert sum(spilled.values()) > 0
    assert spilled + tabled == oracle
    # spill-all over the second part only: every word, absolute offsets
    rk, rp, nw = run_spill_all(dev, text, start=cut)
    got, where = check_records(text, rk, rp)
    assert got == collections.Counter(text[cut:].split())
    assert min(o for o, _ in where) == cut
    missing = [(o, w) for o, w in expect
               if o >= cut and (o, len(w)) not in where]
    assert not missing, missing


# -------------------------------------------------------------- end to end
def test_wordcount_end_to_end(dev, edge):
    from mapreduce_amd.gpu.wordcount import WordCountJob
    text, _, oracle = edge
    res = WordCountJob(dev, vocab_estimate=8000).run(to_dev(text, dev))
    got = res.to_host()
    assert all(w in oracle for w, _ in got)
    assert dict(got) == dict(oracle)
    assert res.nwords == sum(oracle.values())


def test_inverted_index_end_to_end(dev, edge):
    from mapreduce_amd.gpu.inverted_index import InvertedIndexJob
    text, _, _ = edge
    cuts = [0]
    for target in (len(text) // 3, 2 * len(text) // 3):
        cuts.append(next(c for c in range(target, len(text))
                         if text[c - 1] in WS))
    cuts.append(len(text))
    splits = list(zip(cuts[:-1], cuts[1:]))
    exp = {}
    for d, (s, e) in enumerate(splits):
        for w, n in collections.Counter(text[s:e].split()).items():
            exp.setdefault(w, []).append((d, n))
    got = InvertedIndexJob(dev).run(to_dev(text, dev), splits).to_host()
    assert got == exp


# --------------------------------------------------------- occupancy, grid
def test_occupancy_guard(dev):
    from mapreduce_amd import ops
    occ = ops.ext().tokenizer_occupancy()
    print("tokenizer occupancy:", dict(occ))
    assert occ["lds_bytes"] == 28736
    assert occ["blocks_per_cu"] >= 5
    assert 0 < occ["num_regs"] <= 96


def test_grid_below_and_above_resident(dev, edge):
    from mapreduce_amd import ops
    from mapreduce_amd.gpu.wordcount import WordCountJob
    text, _, oracle = edge
    occ = ops.ext().tokenizer_occupancy()
    resident = occ["blocks_per_cu"] * occ["cus"]
    # fewer tiles than resident blocks: the grid is the tile count
    small = text[:3 * TILE + 100]
    assert -(-len(small) // TILE) < resident
    res = WordCountJob(dev, vocab_estimate=8000).run(to_dev(small, dev))
    assert dict(res.to_host()) == dict(collections.Counter(small.split()))
    # many more tiles than the grid can hold: the grid-stride tail
    reps = -(-40_000_000 // (len(text) + 1))
    big = to_dev(text + b" ", dev).repeat(reps)
    assert big.numel() // TILE > 4 * 2048
    res = WordCountJob(dev, vocab_estimate=8000).run(big)
    assert res.nwords == reps * sum(oracle.values())
    assert dict(res.to_host()) == {w: c * reps for w, c in oracle.items()}
