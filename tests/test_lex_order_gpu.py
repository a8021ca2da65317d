"""Device lexicographic order (ops.lex_order), the string lower bound and
the result-class views built on them, against Python sorted()/bisect_left.
The whole permutation is compared, so duplicates must keep index order.
Inputs are built by concatenation (no tokenizer): any byte may appear."""

import bisect
import collections

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 63, 64, 65, 257, 5000]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mapreduce_amd import ops
    ops.require_gpu_ext()
    return torch.device("cuda:0")


# ---------------------------------------------------------------- inputs
def tiny_alphabet(n, seed=0):
    """{0x00, 'a', 0xFF}, lengths 0..24: deep ties, NUL-suffix pairs,
    empty strings, duplicates."""
    rng = np.random.default_rng(seed + n)
    alpha = np.frombuffer(b"\x00a\xff", dtype=np.uint8)
    out = [b"a", b"a\x00", b"a\x00\x00", b"", b"a", b""][:n]
    while len(out) < n:
        ln = int(rng.integers(0, 25))
        out.append(bytes(alpha[rng.integers(0, 3, size=ln)]))
    return [out[i] for i in rng.permutation(n)]


def deep_ties(n=5000):
    """Four shared 8-byte heads + tiny-alphabet tails of 0..16 bytes: nearly
    everything is still tied after chunk 0, so later rounds stay large."""
    rng = np.random.default_rng(77)
    alpha = np.frombuffer(b"\x00a\xff", dtype=np.uint8)
    heads = [b"headhead", b"headhea\x00", b"\xff" * 8, b"\x00" * 8]
    return [heads[int(rng.integers(0, 4))]
            + bytes(alpha[rng.integers(0, 3, size=int(rng.integers(0, 17)))])
            for _ in range(n)]


def chunk_boundaries():
    """Lengths exactly 7, 8, 9, 15, 16, 17 sharing the first 8 and then
    the first 16 bytes, differing only in the last byte."""
    base = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ"
    out = []
    for ln in (7, 8, 9, 15, 16, 17):
        out.append(base[:ln])
        out.append(base[:ln - 1] + b"\x00")
        out.append(base[:ln - 1] + b"\xff")
        out.append(base[:ln])  # duplicate: index order must hold
    out += [base[:8] + b"zz", base[:16] + b"\x00", base[:16]]
    return out[::-1]


def shared_prefix(n=300, plen=70):
    rng = np.random.default_rng(5)
    pre = bytes(rng.integers(1, 255, size=plen, dtype=np.uint8))
    return [pre + bytes(rng.integers(0, 256, size=int(rng.integers(0, 6)),
                                     dtype=np.uint8)) for _ in range(n)]


def over_read_bait():
    """The buffer's LAST and FIRST strings each have a neighbour that an
    over-read of adjacent 0xFF bytes would reorder."""
    return [b"ab", b"mm", b"ab\x01", b"zz\x01", b"", b"q" * 9, b"q" * 9 + b"\x01",
            b"zz\x00", b"zz"]


def pack(strings, dev, lead=b"", trail=b"", tail_exact=False):
    """-> (text, pos).  text is the slice of a larger device tensor that
    holds exactly the concatenated strings; lead/trail are the foreign
    bytes around it.  tail_exact: no trail, the slice ends on the
    allocation's last byte."""
    pos = []
    off = 0
    for s in strings:
        pos.append((off << 16) | len(s))
        off += len(s)
    data = b"".join(strings)
    if tail_exact:
        trail = b""
    big = torch.frombuffer(bytearray(lead + data + trail + b"\x00"),
                           dtype=torch.uint8)[:-1].to(dev)
    text = big[len(lead):len(lead) + len(data)]
    assert text.numel() == len(data)
    return text, torch.tensor(pos, dtype=torch.int64, device=dev).reshape(-1)


def oracle_perm(strings):
    return sorted(range(len(strings)), key=strings.__getitem__)  # stable


def check_order(dev, strings, **kw):
    from mapreduce_amd import ops
    text, pos = pack(strings, dev, **kw)
    perm = ops.lex_order(text, pos)
    assert perm.dtype == torch.int64 and perm.numel() == len(strings)
    got = perm.cpu().tolist()
    if got != oracle_perm(strings):
        exp = oracle_perm(strings)
        bad = next(i for i, (a, b) in enumerate(zip(got, exp)) if a != b)
        raise AssertionError(
            f"first mismatch at rank {bad}: got #{got[bad]} "
            f"{strings[got[bad]][:40]!r}, want #{exp[bad]} "
            f"{strings[exp[bad]][:40]!r}")
    return text, pos, perm


# ----------------------------------------------------------------- order
@pytest.mark.parametrize("n", SIZES)
def test_tiny_alphabet(dev, n):
    strings = tiny_alphabet(n)
    if n >= 6:
        assert {b"a", b"a\x00", b"a\x00\x00", b""} <= set(strings)
        assert len(set(strings)) < n  # duplicates present
    check_order(dev, strings)


def test_chunk_boundary_lengths(dev):
    check_order(dev, chunk_boundaries())


@pytest.mark.parametrize("rounds", [None, "1", "2", "64"])
def test_shared_70_byte_prefix(dev, monkeypatch, rounds):
    """Default cap (8 rounds = 64 bytes) and "1"/"2" finish on the host;
    "64" finishes on the device."""
    if rounds is None:
        monkeypatch.delenv("MR_LEX_ROUNDS", raising=False)
    else:
        monkeypatch.setenv("MR_LEX_ROUNDS", rounds)
    check_order(dev, shared_prefix())


def test_two_64k_strings_bounded_work(dev, monkeypatch):
    """8,192 chunks long: must not become 8,192 sorts."""
    monkeypatch.delenv("MR_LEX_ROUNDS", raising=False)
    rng = np.random.default_rng(9)
    body = bytes(rng.integers(0, 256, size=65534, dtype=np.uint8))
    strings = tiny_alphabet(100) + [body + b"\x02", body + b"\x01"]
    from mapreduce_amd import ops
    calls = []
    real = ops.sort_by_key

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "sort_by_key", counting)
    check_order(dev, strings)
    assert len(calls) <= 2 + 2 * 8  # length + chunk 0 + two per round


# ------------------------------------------------------ alignment, bounds
@pytest.mark.parametrize("k", range(8))
def test_storage_offsets(dev, k):
    """Same strings at storage offsets 0..7; the view ends on the
    allocation's last byte."""
    strings = tiny_alphabet(257) + chunk_boundaries() + over_read_bait()
    text, _, _ = check_order(dev, strings, lead=b"\xff" * k,
                             tail_exact=True)
    assert text.storage_offset() == k


@pytest.mark.parametrize("k", [0, 3])
def test_odd_size_last_string_ends_on_final_byte(dev, k):
    strings = chunk_boundaries() + [b"x" * 11, b"x" * 10, b"x" * 12]
    if sum(map(len, strings)) % 2 == 0:
        strings.append(b"x")
    assert sum(map(len, strings)) % 2 == 1 and len(strings[-1]) > 0
    check_order(dev, strings, lead=b"\xff" * k, tail_exact=True)


@pytest.mark.parametrize("k", [0, 1, 5, 8])
def test_foreign_ff_bytes_around_text(dev, k):
    """The text is an exact-size slice inside a larger tensor full of
    0xFF: reading past either end changes the order."""
    strings = over_read_bait()
    assert strings[-1] == b"zz" and strings[0] == b"ab"
    check_order(dev, strings, lead=b"\xff" * k, trail=b"\xff" * 64)
    check_order(dev, strings[::-1], lead=b"\xff" * (k + 16),
                trail=b"\xff" * 64)


# ---------------------------------------------------- in-tree radix path
@pytest.mark.parametrize("name", ["tiny", "deep"])
def test_radix_path(dev, monkeypatch, name):
    """n=5000 above a lowered small-sort threshold: every sort rides
    radix_sort_idx32 / gather_by_u32 instead of torch.sort."""
    from mapreduce_amd import ops
    monkeypatch.setenv("MR_SMALL_SORT_N", "1024")
    hits = []
    real = ops.sort_idx32

    def spy(*a, **k):
        hits.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "sort_idx32", spy)
    strings = tiny_alphabet(5000) if name == "tiny" else deep_ties(5000)
    check_order(dev, strings)
    assert len(hits) >= (2 if name == "tiny" else 4)


def test_deep_ties_default_threshold(dev):
    check_order(dev, deep_ties(5000))


# ----------------------------------------------------------- lower bound
def queries_for(strings, nq=64):
    rng = np.random.default_rng(len(strings))
    qs = [b"", b"\xff" * 3, b"a", b"a\x00", b"zzzz-absent", b"\x00"]
    while len(qs) < nq:
        w = strings[int(rng.integers(0, len(strings)))] if strings else b"w"
        kind = len(qs) % 3
        qs.append(w if kind == 0 else w[:len(w) // 2] if kind == 1
                  else w + b"\x01")
    return qs


@pytest.mark.parametrize("name", ["empty", "one", "tiny257", "chunks",
                                  "prefix70", "deep"])
def test_lower_bound(dev, name):
    from mapreduce_amd import ops
    strings = {"empty": [], "one": [b"m"], "tiny257": tiny_alphabet(257),
               "chunks": chunk_boundaries(), "prefix70": shared_prefix(),
               "deep": deep_ties(5000)}[name]
    text, pos, perm = check_order(dev, strings, lead=b"\xff" * 3,
                                  trail=b"\xff" * 16)
    ordered = sorted(strings)
    qs = queries_for(strings)
    assert len(qs) == 64
    got = ops.lex_lower_bound(text, pos, perm, qs)
    assert got.is_cuda and got.dtype == torch.int64
    assert got.cpu().tolist() == [bisect.bisect_left(ordered, q) for q in qs]


# ------------------------------------------------------------ end to end
def decode(mat):
    keys, counts, lens, blob = mat
    raw = bytes(blob.numpy().tobytes())
    out = []
    off = 0
    for L, c in zip(lens.tolist(), counts.tolist()):
        out.append((raw[off:off + L], c))
        off += L
    return out


@pytest.fixture(scope="module")
def wc_corpus(dev):
    from mapreduce_amd.gpu.corpus import make_corpus
    c = make_corpus(dev, nwords=200_000, nsplits=8, vocab_size=5_000)
    exp = sorted(collections.Counter(
        bytes(c.text.cpu().numpy().tobytes()).split()).items())
    return c, exp


def check_wc_result(res, exp):
    assert res.to_host("lex") == exp
    assert decode(res.materialize(order="lex")) == exp
    assert sorted(decode(res.materialize())) == exp
    full = exp[len(exp) // 3][0]
    for p in (b"", b"a", b"th", full, full + b"x", b"\xff"):
        want = [(w, c) for w, c in exp if w.startswith(p)]
        assert res.prefix(p) == want
        assert res.count_prefix(p) == len(want)
    assert res.prefix(b"", limit=9) == exp[:9]
    assert list(res.pair_iterator("lex")) == [(w, [c]) for w, c in exp]


def test_wordcount_lex_gpu(dev, wc_corpus):
    from mapreduce_amd.gpu.wordcount import WordCountJob
    c, exp = wc_corpus
    res = WordCountJob(dev, vocab_estimate=8_000).run(c.text, c.splits())
    assert res.lex_perm() is res.lex_perm()  # cached
    check_wc_result(res, exp)


def test_wordcount_lex_through_pipeline(dev, wc_corpus):
    """lex_perm()/prefix() on a result that carries a ready-event from
    the pipeline's side stream."""
    from mapreduce_amd.gpu.pipeline import PipelinedWordCount
    c, exp = wc_corpus
    pipe = PipelinedWordCount(dev, vocab_estimate=8_000)
    res = pipe.step(c.text, c.splits())
    assert getattr(res, "_ready", None) is not None
    want = [(w, n) for w, n in exp if w.startswith(b"s")]
    assert res.prefix(b"s") == want
    assert getattr(res, "_ready", None) is None  # waited on
    tail = pipe.flush()
    assert getattr(tail, "_ready", None) is not None
    assert tail.lex_perm().numel() == len(exp)
    check_wc_result(tail, exp)


def test_inverted_index_lex_gpu(dev):
    from mapreduce_amd.gpu.inverted_index import InvertedIndexJob
    rng = np.random.default_rng(31)
    letters = np.frombuffer(b"abcdefgh", dtype=np.uint8)
    vocab = sorted({bytes(letters[rng.integers(0, 8, size=int(
        rng.integers(1, 12)))]) for _ in range(400)})
    docs = [b" ".join(vocab[i] for i in rng.integers(0, len(vocab), 300))
            + b"\n" for _ in range(20)]
    splits, off = [], 0
    for d in docs:
        splits.append((off, off + len(d)))
        off += len(d)
    text = torch.frombuffer(bytearray(b"".join(docs)),
                            dtype=torch.uint8).to(dev)
    exp = {}
    for di, d in enumerate(docs):
        for w, tf in collections.Counter(d.split()).items():
            exp.setdefault(w, []).append((di, tf))
    res = InvertedIndexJob(dev).run(text, splits)
    assert list(res.pair_iterator("lex")) == sorted(exp.items())
    for p in (b"", b"a", b"ab", b"abc", vocab[7], vocab[7] + b"z", b"\xff"):
        want = [(w, exp[w]) for w in sorted(exp) if w.startswith(p)]
        assert res.prefix(p) == want
    assert res.prefix(b"", limit=5) == sorted(exp.items())[:5]
