"""Lexicographic result order and prefix queries on the CPU tier: the ops
fallbacks against sorted()/bisect_left, and every layer above the kernels
(result classes, pair iterators, the /prefix endpoint) against Python
oracles."""

import bisect
import collections

import numpy as np
import pytest
import torch

from mapreduce_amd import ops


# ---------------------------------------------------------------- inputs
def pack(strings, lead=b"", trail=b""):
    """(text u8, pos i64) holding `strings` back to back."""
    pos = []
    off = len(lead)
    for s in strings:
        pos.append((off << 16) | len(s))
        off += len(s)
    data = lead + b"".join(strings) + trail
    text = (torch.frombuffer(bytearray(data), dtype=torch.uint8)
            if data else torch.empty(0, dtype=torch.uint8))
    return text, torch.tensor(pos, dtype=torch.int64)


def tiny_alphabet(n, seed=0):
    """{0x00, 'a', 0xFF}, lengths 0..24: deep ties, NUL-suffix pairs,
    empty strings, duplicates."""
    rng = np.random.default_rng(seed + n)
    alpha = np.frombuffer(b"\x00a\xff", dtype=np.uint8)
    out = [b"a", b"a\x00", b"a\x00\x00", b"", b"a", b""][:n]
    while len(out) < n:
        ln = int(rng.integers(0, 25))
        out.append(bytes(alpha[rng.integers(0, 3, size=ln)]))
    order = rng.permutation(n)
    return [out[i] for i in order]


def chunk_boundaries():
    base = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ"
    out = []
    for ln in (7, 8, 9, 15, 16, 17):
        out.append(base[:ln])
        out.append(base[:ln - 1] + b"\x00")
        out.append(base[:ln - 1] + b"\xff")
    out += [base[:8] + b"zz", base[:16] + b"\x00", base[:16]]
    return out[::-1]


def shared_prefix(n=300, plen=70):
    rng = np.random.default_rng(5)
    pre = bytes(rng.integers(1, 255, size=plen, dtype=np.uint8))
    return [pre + bytes(rng.integers(0, 256, size=int(rng.integers(0, 6)),
                                     dtype=np.uint8)) for _ in range(n)]


SETS = {
    "empty": [], "one": [b"x"], "tiny5000": tiny_alphabet(5000),
    "tiny65": tiny_alphabet(65), "chunks": chunk_boundaries(),
    "prefix70": shared_prefix(),
}


def oracle_perm(strings):
    return sorted(range(len(strings)), key=strings.__getitem__)


def queries_for(strings, nq=64):
    rng = np.random.default_rng(len(strings))
    qs = [b"", b"\xff" * 3, b"a", b"a\x00", b"zzzz-absent"]
    while len(qs) < nq and strings:
        w = strings[int(rng.integers(0, len(strings)))]
        kind = len(qs) % 3
        qs.append(w if kind == 0 else w[:len(w) // 2] if kind == 1
                  else w + b"\x01")
    return qs


# ------------------------------------------------------------------- ops
@pytest.mark.parametrize("name", sorted(SETS))
def test_ops_lex_order_cpu(name):
    strings = SETS[name]
    text, pos = pack(strings)
    perm = ops.lex_order(text, pos)
    assert perm.dtype == torch.int64
    assert perm.tolist() == oracle_perm(strings)


@pytest.mark.parametrize("name", sorted(SETS))
def test_ops_lex_lower_bound_cpu(name):
    strings = SETS[name]
    text, pos = pack(strings)
    perm = ops.lex_order(text, pos)
    ordered = sorted(strings)
    qs = queries_for(strings)
    got = ops.lex_lower_bound(text, pos, perm, qs).tolist()
    assert got == [bisect.bisect_left(ordered, q) for q in qs]


def test_prefix_succ():
    assert ops.prefix_succ(b"a") == b"b"
    assert ops.prefix_succ(b"a\xff") == b"b"
    assert ops.prefix_succ(b"a\xff\xff") == b"b"
    assert ops.prefix_succ(b"\xff\xff") is None
    assert ops.prefix_succ(b"") is None
    assert ops.prefix_succ(b"ab\x00") == b"ab\x01"


def test_prefix_range_succ_edges():
    strings = [b"a", b"a\xff", b"a\xff\xff", b"a\xffz", b"b", b"\xff",
               b"\xff\xff", b"\xff\xff\x00", b"", b"a\xfe"]
    text, pos = pack(strings)
    perm = ops.lex_order(text, pos)
    ordered = sorted(strings)
    for p in (b"a\xff", b"\xff\xff", b"\xff", b"", b"a",
              b"a\xff\xff\xff\xff\xff"):  # last: longer than any word
        lo, hi = ops.lex_prefix_range(text, pos, perm, p)
        assert ordered[lo:hi] == [w for w in ordered if w.startswith(p)]


# ------------------------------------------------------------ word count
@pytest.fixture(scope="module")
def wc():
    from mapreduce_amd.gpu.corpus import make_corpus
    from mapreduce_amd.gpu.wordcount import WordCountJob
    c = make_corpus("cpu", nwords=30_000, nsplits=4, vocab_size=900, seed=2)
    res = WordCountJob("cpu").run(c.text, c.splits())
    exp = sorted(collections.Counter(
        bytes(c.text.numpy().tobytes()).split()).items())
    return res, exp


def decode(mat):
    keys, counts, lens, blob = mat
    raw = bytes(blob.numpy().tobytes())
    out = []
    off = 0
    for L, c in zip(lens.tolist(), counts.tolist()):
        out.append((raw[off:off + L], c))
        off += L
    return out


def test_wordcount_lex_views(wc):
    res, exp = wc
    assert len(exp) > 500
    assert res.to_host(order="lex") == exp
    assert decode(res.materialize(order="lex")) == exp
    # default order unchanged: hash order, same content
    assert decode(res.materialize()) == res.to_host()
    assert sorted(res.to_host()) == exp
    assert list(res.pair_iterator(order="lex")) == [(w, [c])
                                                    for w, c in exp]
    # keys travel with their rows
    k = res.materialize(order="lex")[0].tolist()
    assert k == [res.key_of(w) for w, _ in exp]


def test_wordcount_prefix(wc):
    res, exp = wc
    full = exp[len(exp) // 2][0]
    for p in (b"", b"a", b"aa", full, full + b"x", b"\xff"):
        want = [(w, c) for w, c in exp if w.startswith(p)]
        assert res.prefix(p) == want
        assert res.count_prefix(p) == len(want)
    assert res.prefix(full + b"x") == []
    assert res.count_prefix(b"") == len(exp)
    assert res.prefix(b"", limit=7) == exp[:7]
    want_a = [(w, c) for w, c in exp if w.startswith(b"a")]
    assert len(want_a) > 3
    assert res.prefix(b"a", limit=3) == want_a[:3]
    assert res.prefix("a", limit=10 ** 6) == want_a  # str accepted


# -------------------------------------------------------- inverted index
def test_inverted_index_lex_and_prefix():
    from mapreduce_amd.gpu.inverted_index import InvertedIndexJob
    rng = np.random.default_rng(3)
    vocab = [b"ab", b"abc", b"abd", b"b", b"ba", b"zeta", b"a", b"abcde",
             b"q", b"ab\xff"]
    docs = [b" ".join(vocab[i] for i in rng.integers(0, len(vocab), 40))
            + b"\n" for _ in range(20)]
    data = b"".join(docs)
    splits, off = [], 0
    for d in docs:
        splits.append((off, off + len(d)))
        off += len(d)
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    res = InvertedIndexJob("cpu").run(text, splits)
    exp = res.to_host()
    assert set(exp) == set(vocab)
    assert list(res.pair_iterator(order="lex")) == sorted(exp.items())
    assert dict(res.pair_iterator()) == exp
    for p in (b"", b"ab", b"abc", b"abcdef", b"z", b"ab\xff", b"\xff"):
        want = [(w, exp[w]) for w in sorted(exp) if w.startswith(p)]
        assert res.prefix(p) == want
    assert res.prefix(b"ab", limit=2) == [
        (w, exp[w]) for w in sorted(exp) if w.startswith(b"ab")][:2]


# ----------------------------------------------------------------- serve
def test_prefix_endpoint(wc):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from mapreduce_amd.serve import make_app
    res, exp = wc
    client = TestClient(make_app(wordcount=res))
    want = [(w, c) for w, c in exp if w.startswith(b"a")]
    r = client.get("/prefix", params={"p": "a", "limit": 5})
    assert r.status_code == 200
    body = r.json()
    assert body["prefix"] == "a"
    assert body["total"] == len(want)
    assert body["words"] == [{"word": w.decode(), "count": c}
                             for w, c in want[:5]]
    r = client.get("/prefix", params={"p": "no-such-prefix"})
    assert r.json() == {"prefix": "no-such-prefix", "total": 0, "words": []}
    assert TestClient(make_app()).get(
        "/prefix", params={"p": "a"}).status_code == 404
