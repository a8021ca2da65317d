"""GPU-free case generators and checkers for test_tokenizer_multitile.py.

Everything here is plain Python / numpy: texts that make one tokenizer block
walk several 4 KB tiles (with words on every tile and halo edge), texts of
one or two keys repeated, a text that overfills one block's word cache, and
the checker that compares table counts plus spilled records with the Python
split oracle.  test_tokenizer_multitile_cpu.py checks the generators without
a GPU."""

import collections
import functools
import hashlib
import itertools
import re

import numpy as np

from mapreduce_amd.utils.tuple import splitmix64, wordhash64

HT_EMPTY = (1 << 64) - 1
MASK64 = (1 << 64) - 1
WS = frozenset(b" \t\n\v\f\r")
TILE = 4096
HALO = 64
CACHE_SLOTS = 2048

WALK_SIZES = (0, 1, 15, 16, 17, 4095, 4096, 4097, 4096 + 63, 4096 + 64,
              4096 + 65, 8191, 8192, 8193, 3 * 4096 + 5, 24 * 4096)
WALK_BLOCKS = (1, 2, 3)
UNALIGNED_STARTS = (1, 7, 15)
UNALIGNED_PREFIX = b" xxxx  yyyyyy  zz "  # a word starts at 1, 7 and 15


def device_key(word: bytes) -> int:
    h = wordhash64(word)
    return HT_EMPTY - 1 if h == HT_EMPTY else h  # remap_key


def composite_key(word: bytes, doc: int) -> int:
    h = wordhash64(word) ^ splitmix64(doc & MASK64)
    return HT_EMPTY - 1 if h == HT_EMPTY else h


def cache_slot(key: int) -> int:
    return (key ^ (key >> 32)) & (CACHE_SLOTS - 1)


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def vocab():
    rng = np.random.default_rng(20240)
    words = [bytes(t) for t in itertools.product(range(97, 123), repeat=3)]
    idx = rng.permutation(len(words))[:6000]
    return tuple(words[i] for i in idx)


def filler(nbytes: int, seed: int) -> bytearray:
    """nbytes of 'abc ' units over ~6000 distinct words (the last unit is
    cut where nbytes is no multiple of 4)."""
    v = vocab()
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, len(v), (nbytes + 3) // 4)
    return bytearray(b"".join(v[i] + b" " for i in ids))[:nbytes]


def place(buf: bytearray, off: int, word: bytes, expect: list) -> bool:
    """Overwrite buf so that `word` stands at `off` between spaces; a word
    that does not fit is cut so that it runs to the end of the text."""
    n = len(buf)
    if off < 1 or off >= n:
        return False
    word = word[:n - off]
    buf[off - 1] = 0x20
    buf[off:off + len(word)] = word
    if off + len(word) < n:
        buf[off + len(word)] = 0x20
    expect.append((off, bytes(word)))
    return True


def named(tag: str, length: int) -> bytes:
    return (tag.encode() + b"x" * length)[:length]


@functools.lru_cache(maxsize=None)
def walk_text(n: int):
    """-> (text of n bytes, ((offset, word), ...) that must be found).

    Filler, plus at every tile edge k * TILE inside the text a 12-byte word
    across the edge and a 10-byte word across the halo edge k * TILE + HALO;
    at the first edge the word across it is 100 bytes long instead, so it
    also runs past the halo."""
    buf = filler(n, seed=n + 1)
    expect = []
    for k in range(1, n // TILE + 1):
        edge = k * TILE
        if k == 1:
            place(buf, edge - 20, named("PastHalo", 100), expect)
        else:
            place(buf, edge - 5, named(f"Edge{k}", 12), expect)
            place(buf, edge + HALO - 4, named(f"Halo{k}", 10), expect)
    text = bytes(buf)
    assert len(text) == n
    for off, w in expect:  # the placements did not overwrite each other
        assert text[off:off + len(w)] == w and text[off - 1] in WS
        assert off + len(w) == n or text[off + len(w)] in WS
    return text, tuple(expect)


@functools.lru_cache(maxsize=None)
def unaligned_text():
    buf = filler(3 * TILE + 40, seed=77)
    buf[:len(UNALIGNED_PREFIX)] = UNALIGNED_PREFIX
    expect = []
    place(buf, TILE - 3, b"AcrossTile", expect)
    place(buf, 2 * TILE + HALO - 2, b"AcrossHalo", expect)
    return bytes(buf), tuple(expect)


@functools.lru_cache(maxsize=None)
def slot_sharing_pair():
    """Two words of the vocabulary whose keys fall into one cache slot."""
    seen = {}
    for w in sorted(vocab()):
        s = cache_slot(device_key(w))
        if s in seen:
            return seen[s], w
        seen[s] = w
    raise AssertionError("no two of 6000 words share one of 2048 slots")


@functools.lru_cache(maxsize=None)
def same_key_texts():
    a, b = slot_sharing_pair()
    return {
        "a_x8192": b"a " * 8192,
        "the_x4096": b"the " * 4096,
        "slot_pair": (a + b" " + b + b" ") * 2048,
    }


@functools.lru_cache(maxsize=None)
def saturation_text():
    return bytes(filler(24 * TILE, seed=5))


def key_oracle(text: bytes, keyfn=device_key):
    """Counter of device keys of text.split()."""
    out = collections.Counter()
    for w, c in collections.Counter(text.split()).items():
        out[keyfn(w)] += c
    return out


def composite_oracle(text: bytes, split_off, doc_base: int):
    """Counter of composite keys, one per word occurrence of text."""
    out = collections.Counter()
    for m in re.finditer(rb"[^ \t\n\v\f\r]+", text):
        doc = doc_of(m.start(), split_off) + doc_base
        out[composite_key(m.group(), doc)] += 1
    return out


def doc_of(off: int, split_off) -> int:
    """Index of the last split offset <= off (the kernel's ub_minus1)."""
    return int(np.searchsorted(np.asarray(split_off), off, side="right")) - 1


# ----------------------------------------------------------------- checker
def check_records(text: bytes, keys, pos, weights=None, keyfn=None):
    """Every non-pad record is a complete word of `text` whose key is the
    record's.  -> (Counter by key, set of (offset, len)).  keyfn(word, off)
    defaults to the plain word key."""
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
        want = device_key(w) if keyfn is None else keyfn(w, off)
        assert want == k, (off, ln, w)
        got[k] += 1 if weights is None else weights[i]
        where.add((off, ln))
    return got, where


def digest(keys, pos) -> str:
    """Order-free fingerprint of the non-pad (key, pos) records."""
    recs = sorted((k, p) for k, p in zip(keys, pos) if k != HT_EMPTY)
    h = hashlib.sha256()
    h.update(np.asarray(recs, dtype=np.uint64).tobytes())
    return f"{len(recs)}:{h.hexdigest()[:24]}"
