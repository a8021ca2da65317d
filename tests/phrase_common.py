"""Shared pieces of the positional-index / phrase-search tests (not a test
module): whitespace cases and the bytes.split() oracle of token ordinals,
synthetic CSR + positions built with NumPy, the brute-force phrase oracle
over position lists, the one over documents' split() word lists, and the
2,000-document corpus of the end-to-end checks."""

import bisect
import re

import numpy as np
import torch

from index_search_common import SynthIndex, as_i64, expect

WORD_RE = re.compile(rb"[^ \t\n\v\f\r]+")


# ---------------------------------------------------------------- ordinals
def pack_pos(off: int, length: int) -> int:
    return (off << 16) | min(length, 0xFFFF)


def ordinal_oracle(raw: bytes, starts):
    """-> (pos, doc, ord) lists, one entry per word of raw in text order.
    Words are those of bytes.split(); a word belongs to the document of its
    first byte (last starts[] entry <= offset) and its ordinal counts the
    words before it that begin in the same document."""
    words = [(m.start(), m.end() - m.start()) for m in WORD_RE.finditer(raw)]
    assert [raw[o:o + n] for o, n in words] == raw.split()
    pos, doc, ordn = [], [], []
    seen = {}
    for off, n in words:
        d = bisect.bisect_right(starts, off) - 1
        pos.append(pack_pos(off, n))
        doc.append(d)
        ordn.append(seen.get(d, 0))
        seen[d] = seen.get(d, 0) + 1
    return pos, doc, ordn


def ordinal_cases():
    """[(name, raw bytes, starts)]: starts = document offsets + the end."""
    out = [
        ("six_ws", b"a b\tc\nd\ve\ff\rg", []),
        ("runs", b"a  b \t\n c\r\r\r\rd", []),
        ("lead_trail", b"  \t a b  c \n\n", []),
        ("only_ws", b" \t\n ", []),
        ("one_word", b"word", []),
        ("empty_text", b"", []),
        # documents 1 and 3 are empty (equal offsets); 4 is whitespace only
        ("empty_docs", b"a b\nc d e\n  \nf\n", [4, 4, 10, 10, 13]),
        # boundary inside the whitespace run between b and c
        ("split_in_ws", b"a b   c d", [5]),
        # boundary inside "cccc": the fragment is no word of document 1
        ("split_mid_word", b"a b cccc d e", [6]),
        ("high_bytes", b"\xc3\xa9t\xc3\xa9 \x80\xff\x85 \xa0x\xa0 z", [6]),
        # words straddling 8-byte and 64-byte boundaries
        ("straddle", b"abcdefg hijklmnopq r " + b"x" * 40 + b" " +
         b"y" * 30 + b" zz " + b"w" * 70 + b" q", [30, 64, 100]),
    ]
    return [(n, r, [0] + cuts + [len(r)]) for n, r, cuts in out]


def check_ordinals(ops_mod, text_t, raw: bytes, starts, dev):
    """ops.token_ordinals over every word of raw == the split() oracle."""
    pos, doc, ordn = ordinal_oracle(raw, starts)
    # a shuffled order: the op must not depend on sorted occurrences
    perm = np.random.default_rng(len(raw)).permutation(len(pos))
    p = torch.tensor([pos[i] for i in perm], dtype=torch.int64).to(dev)
    s = torch.tensor(starts, dtype=torch.int64).to(dev)
    gd, go = ops_mod.token_ordinals(text_t, p, s)
    assert gd.dtype == torch.int64 and go.dtype == torch.int32
    assert gd.cpu().tolist() == [doc[i] for i in perm]
    assert go.cpu().tolist() == [ordn[i] for i in perm]
    return p, s, gd, go


# ------------------------------------------------- synthetic CSR + positions
class PosIndex:
    """{u64 hash: [(doc, [ord, ...]), ...]} (docs ascending and unique,
    ordinals ascending and unique) as the CSR arrays of a positional
    InvertedIndexResult."""

    def __init__(self, lists: dict):
        self.lists = {h: [(d, list(p)) for d, p in pl]
                      for h, pl in lists.items()}
        self.csr = SynthIndex({h: [(d, len(p)) for d, p in pl]
                               for h, pl in self.lists.items()})
        flat = [p for h in self.csr.hashes for _, p in self.lists[h]]
        self.pos_offsets = np.concatenate(
            [[0], np.cumsum([len(p) for p in flat])]).astype(np.int64)
        self.positions = np.array([x for p in flat for x in p],
                                  dtype=np.int32)
        self.by_doc = {h: dict(pl) for h, pl in self.lists.items()}

    def tensors(self, dev, bait_keys=(), bait=True):
        """(keys, doc_offsets, docs, tf, pos_offsets, positions) on dev,
        each the exact-size middle slice of a larger tensor (see
        SynthIndex.tensors); positions are flanked by the ordinals that
        would continue the first and the last slice."""
        keys, offs, docs, tf, _ = self.csr.tensors(dev, bait_keys, bait)
        nocc = len(self.positions)

        def wrap(a, lead, trail):
            if not bait:
                return torch.from_numpy(a.copy()).to(dev)
            big = np.concatenate([np.asarray(lead, dtype=a.dtype), a,
                                  np.asarray(trail, dtype=a.dtype)])
            return torch.from_numpy(big).to(dev)[len(lead):
                                                 len(lead) + len(a)]

        first = int(self.positions[0]) if nocc else 0
        last = int(self.positions[-1]) if nocc else 0
        return (keys, offs, docs, tf,
                wrap(self.pos_offsets, [0, 0], [nocc, nocc]),
                wrap(self.positions, [first - 2, first - 1],
                     [last + 1, last + 2]))

    def ranked(self, terms):
        """Brute force: every matching (doc, phrase frequency), best
        first."""
        if not terms or any(h not in self.by_doc for h in terms):
            return []
        docs = set.intersection(*[set(self.by_doc[h]) for h in terms])
        out = []
        for d in docs:
            sets = [set(self.by_doc[h][d]) for h in terms]
            cnt = sum(1 for s in sets[0]
                      if all(s + i in ps for i, ps in enumerate(sets)))
            if cnt:
                out.append((d, cnt))
        return sorted(out, key=lambda kv: (-kv[1], kv[0]))


def run_phrase(ops, tens, queries, k):
    """One ops.postings_phrase launch over `queries` (lists of u64 hashes)
    -> per query (docs[k], scores[k], n, hits) as Python lists."""
    flat = [as_i64(h) for q in queries for h in q]
    qoff = np.concatenate([[0], np.cumsum([len(q) for q in queries])])
    out = ops.postings_phrase(
        *tens, torch.tensor(flat, dtype=torch.int64),
        torch.from_numpy(qoff.astype(np.int64)), k)
    d, s, n, h = [t.cpu() for t in out]
    assert d.shape == (len(queries), k) and s.shape == (len(queries), k)
    assert n.shape == (len(queries),) and h.shape == (len(queries),)
    assert all(t.dtype == torch.int64 for t in (d, s, n, h))
    return [(d[i].tolist(), s[i].tolist(), int(n[i]), int(h[i]))
            for i in range(len(queries))]


def check_phrase(ops, index, tens, queries, ks):
    """Full equality of (docs, scores, n, hits) with the oracle for every
    query and k; one launch per k."""
    ranked = [index.ranked(q) for q in queries]
    for k in ks:
        got = run_phrase(ops, tens, queries, k)
        for q, r, g in zip(queries, ranked, got):
            assert g == expect(r, k), (
                f"k={k} terms={[hex(h) for h in q]} hits={len(r)}")
    return ranked


ABSENT = 0x8000000000000001
DENSE = 0x7000000000000001   # every doc of the universe, ordinals 0..11
EQ_A, EQ_B = 0x11, 0x8000000000000022
REP, REP2 = 0x31, 0x32
GUARD_X, GUARD_Y = 0x41, 0x42
BIG, BIG_NEXT = 0x51, 0x52
BAIT_W, BAIT_V = 0x61, 0x62
FIRST_KEY, LAST_KEY = 0x2, 0xFFFFFFFFFFFFFF00
CHAIN0 = 0x7100000000000000


def driver_lengths(buf: int):
    return [1, 255, 256, 257, buf + 1, 2 * buf + 300]


def sweep_lists(buf: int, tmax: int, big: int = 5000):
    """The synthetic index of the kernel sweep -> (lists, by_len, chain).
    buf and tmax come from the caps on the GPU; the CPU tier passes smaller
    ones to keep its NumPy form quick."""
    rng = np.random.default_rng(77)
    n_max = 2 * buf + 300
    universe = n_max + buf
    lists, by_len = {}, {}

    def rand_pos():
        return sorted(rng.choice(12, size=int(rng.integers(1, 5)),
                                 replace=False).tolist())

    for i, n in enumerate(driver_lengths(buf)):
        h = (n * 0x9E3779B97F4A7C15 + (i << 60)) & ((1 << 64) - 1)
        by_len[n] = h
        docs = np.sort(rng.choice(universe, size=n, replace=False))
        lists[h] = [(int(d), rand_pos()) for d in docs]
    lists[DENSE] = [(d, list(range(12))) for d in range(universe)]
    # all scores equal: the order across prunes rests on the doc id
    eq_docs = list(range(10, 10 + 3 * n_max, 3))
    lists[EQ_A] = [(d, [2]) for d in eq_docs]
    lists[EQ_B] = [(d, [3]) for d in range(0, 10 + 3 * n_max + 10)]
    # repeated terms: "a a a" over a run of ten is 8
    lists[REP] = [(0, list(range(10))), (1, [0, 1, 3, 4, 5]), (2, [4, 6]),
                  (3, [1, 2])]
    lists[REP2] = [(0, [10]), (1, [6]), (3, [0]), (4, [1])]
    # the driver (shorter list) is the SECOND term and holds ordinal 0
    lists[GUARD_X] = [(0, [0]), (1, [4]), (2, [0, 3]), (3, [9]), (5, [0])]
    lists[GUARD_Y] = [(0, [0]), (1, [0, 5]), (2, [0, 1]), (5, [1])]
    # one posting with thousands of positions among postings with one
    lists[BIG] = ([(d, [d % 7]) for d in range(7)] +
                  [(7, list(range(0, 2 * big, 2)))] +
                  [(d, [3]) for d in range(8, 40)])
    lists[BIG_NEXT] = ([(d, [d % 7 + 1]) for d in range(0, 7, 2)] +
                       [(7, list(range(1, 2 * big, 4)) + [2 * big + 1])] +
                       [(d, [4]) for d in range(8, 40, 3)])
    # slice-bound bait: W's doc-10 slice ends with 7 and its doc-11 slice
    # starts with 8; V holds 8 and 21 only in doc 10.  Reading W past its
    # slice end matches "W W" in doc 10; reading V's doc-10 slice for doc
    # 11 matches "W V" there (20 -> 21).
    lists[BAIT_W] = [(10, [3, 7]), (11, [8, 20]), (12, [5])]
    lists[BAIT_V] = [(10, [8, 21]), (11, [30]), (12, [9])]
    # first / last key rows; LAST's final slice ends the positions array
    # on 7, which the trailing bait continues with 8
    lists[FIRST_KEY] = [(4, [1, 2]), (9, [0])]
    lists[LAST_KEY] = [(4, [3]), (9, [1, 5, 7])]
    # a TMAX-term phrase: term i at ordinal i + d % 5 (+ 40 every third
    # doc); doc 17 lacks one link
    chain = [CHAIN0 + i for i in range(tmax)]
    for i, h in enumerate(chain):
        pl = []
        for d in range(300):
            p = [i + d % 5] + ([i + 40] if d % 3 == 0 else [])
            if d == 17 and i == tmax // 2:
                p = [i + 50]
            pl.append((d, p))
        lists[h] = pl
    return lists, by_len, chain


def sweep_queries(by_len, chain, buf):
    """The kernel sweep's queries with the properties some must have."""
    tmax = len(chain)
    qs = []
    for h in by_len.values():
        qs += [[h], [h, DENSE], [DENSE, h], [DENSE, h, DENSE], [h, h],
               [h, ABSENT]]
    big_h = by_len[2 * buf + 300]
    qs += [[EQ_A, EQ_B], [EQ_B, EQ_A], [EQ_A],
           [REP, REP, REP], [REP, REP], [REP, REP2], [REP, REP, REP2],
           [GUARD_X, GUARD_Y], [GUARD_Y, GUARD_X],
           [BIG, BIG_NEXT], [BIG], [BIG_NEXT, BIG], [BIG, DENSE],
           [DENSE, DENSE, DENSE],
           [BAIT_W, BAIT_W], [BAIT_W, BAIT_V], [BAIT_V, BAIT_W],
           [FIRST_KEY, LAST_KEY], [LAST_KEY, LAST_KEY], [LAST_KEY],
           chain, chain[:tmax - 1] + [ABSENT], [DENSE] * tmax,
           chain[1:] + [chain[0]], [big_h] + [DENSE] * (tmax - 1),
           [ABSENT], [ABSENT, DENSE], []]
    return qs


def check_sweep_properties(index, by_len, chain, buf, big=5000):
    """The oracle itself says the sweep exercises what it claims to."""
    r = index.ranked
    n_max = 2 * buf + 300
    assert r([REP, REP, REP]) == [(0, 8), (1, 1)]
    assert dict(r([REP]))[0] == 10                       # T = 1 is tf
    # GUARD_Y drives as second term; its ordinal 0 must start nothing
    assert len(index.by_doc[GUARD_Y]) < len(index.by_doc[GUARD_X])
    assert r([GUARD_X, GUARD_Y]) == [(1, 1), (2, 1), (5, 1)]
    assert dict(r([BIG, BIG_NEXT]))[7] == big // 2
    assert dict(r([BIG]))[7] == big
    assert index.csr.hashes[0] == FIRST_KEY
    assert index.csr.hashes[-1] == LAST_KEY
    assert len(r([EQ_A, EQ_B])) == n_max
    assert {s for _, s in r([EQ_A, EQ_B])} == {1}
    assert r([BAIT_W, BAIT_W]) == [] and r([BAIT_W, BAIT_V]) == [(10, 1)]
    assert r([LAST_KEY, LAST_KEY]) == []
    full = r(chain)
    assert len(full) == 299 and full[0] == (0, 2) and 17 not in dict(full)
    assert len(r([by_len[n_max], DENSE])) > buf          # forces a prune


# ------------------------------------------------------------ end to end
E2E_NDOCS = 2000
E2E_VOCAB = [b"alpha", b"beta", b"gamma", b"delta", b"a", b"of", b"the",
             b"caf\xc3\xa9", b"\xff\x80", b"parliament", b"european", b"x"]
E2E_SEPS = [b" ", b"  ", b"\t", b"\n", b" \t ", b"\r\n", b"\v", b"\f "]
E2E_PLANTS = [[b"european", b"parliament"],
              [b"the", b"the", b"alpha"],
              [b"a", b"of", b"a", b"of"]]


def e2e_corpus():
    """-> (text u8 tensor on the host, splits, docs as lists of words).
    2,000 documents of 0-40 tokens over a 12-word vocabulary joined by
    mixed whitespace, a few phrases planted; every 50th is a zero-length
    split and every 77th holds whitespace only."""
    rng = np.random.default_rng(4242)
    docs, raw = [], []
    for i in range(E2E_NDOCS):
        if i % 50 == 7:
            docs.append([])
            raw.append(b"")
            continue
        if i % 77 == 5:
            docs.append([])
            raw.append(b" \t \n")
            continue
        n = int(rng.integers(0, 41))
        words = [E2E_VOCAB[j] for j in rng.integers(0, 12, n)]
        if i % 9 == 0:
            ph = E2E_PLANTS[(i // 9) % 3]
            at = int(rng.integers(0, len(words) + 1))
            words[at:at] = ph
        words = words[:40]
        r = b"  " if i % 5 == 0 else b""
        for w in words:
            r += w + E2E_SEPS[int(rng.integers(0, len(E2E_SEPS)))]
        docs.append(words)
        raw.append(r + b"\n")
    offs = np.concatenate([[0], np.cumsum([len(r) for r in raw])]).tolist()
    blob = b"".join(raw)
    assert [blob[a:b].split() for a, b in zip(offs[:-1], offs[1:])] == docs
    text = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy())
    return text, list(zip(offs[:-1], offs[1:])), docs


def doc_phrase_ranked(docs, terms):
    """Brute force over the documents' split() word lists, best first."""
    terms = list(terms)
    t = len(terms)
    out = []
    if t == 0:
        return out
    for i, d in enumerate(docs):
        cnt = sum(1 for s in range(len(d) - t + 1) if d[s:s + t] == terms)
        if cnt:
            out.append((i, cnt))
    return sorted(out, key=lambda kv: (-kv[1], kv[0]))


def doc_positions(docs, word):
    """Oracle of lookup_positions."""
    out = []
    for i, d in enumerate(docs):
        p = [j for j, w in enumerate(d) if w == word]
        if p:
            out.append((i, p))
    return out


V = E2E_VOCAB
E2E_QUERIES = [
    [V[10], V[9]], [V[9], V[10]], [V[6], V[6]], [V[4], V[5]],
    [V[7], V[8]], [V[6], V[6], V[0]], [V[0], V[1], V[2]],
    [V[4], V[5], V[4]], [V[11], V[11], V[11]],
    [V[4], V[5], V[4], V[5]], [V[0], V[1], V[2], V[3]],
    [V[6], V[6], V[0], V[6]], [V[10], V[9], V[10], V[9]],
    [V[8], V[8], V[8], V[8]], [V[3], V[2], V[1], V[0]],
    [b"absent", V[0]], [V[0], b"absent"], [V[2]], [],
    [V[5], V[11], V[7], V[1]], [V[1], V[7], V[11], V[5]],
]
E2E_K = 10


def check_e2e(idx, docs, k=E2E_K):
    """phrase() / phrase_batch() == the document oracle, after the oracle
    has shown that the queries cover > k hits, 1..k hits and none."""
    assert idx.ndocs == E2E_NDOCS
    want = [doc_phrase_ranked(docs, q) for q in E2E_QUERIES]
    multi = [w for q, w in zip(E2E_QUERIES, want) if len(q) >= 2]
    assert any(len(w) > k for w in multi)
    assert any(1 <= len(w) <= k for w in multi)
    assert any(len(w) == 0 for q, w in zip(E2E_QUERIES, want)
               if len(q) >= 2 and b"absent" not in q)
    for t in (2, 3, 4):
        assert any(len(q) == t and w for q, w in zip(E2E_QUERIES, want))
        assert any(len(q) == t and w and len(set(q)) < t
                   for q, w in zip(E2E_QUERIES, want))
    got = idx.phrase_batch(E2E_QUERIES, k=k)
    for q, g, w in zip(E2E_QUERIES, got, want):
        assert g.hits == len(w), q
        assert g.docs == w[:k], q
    for q, w in list(zip(E2E_QUERIES, want))[:6]:
        one = idx.phrase(q, k=256)
        assert one.hits == len(w) and one.docs == w[:256], q
    assert idx.phrase(b"european \t parliament") == got[0]
    assert idx.phrase("the the alpha") == got[5]
    assert idx.phrase_batch([]) == []


def check_layer(idx, base, docs):
    """The positional build agrees with the default build on the four base
    arrays and its layer is consistent with them and with the oracle."""
    for name in ("keys", "doc_offsets", "docs", "tf"):
        assert torch.equal(getattr(idx, name), getattr(base, name)), name
    assert base.positions is None and base.pos_offsets is None
    assert idx.positions.dtype == torch.int32
    assert idx.pos_offsets.dtype == torch.int64
    assert idx.pos_offsets.numel() == idx.docs.numel() + 1
    assert int(idx.pos_offsets[-1]) == idx.positions.numel() \
        == int(idx.tf.sum()) == sum(len(d) for d in docs)
    assert torch.equal(idx.pos_offsets[1:] - idx.pos_offsets[:-1], idx.tf)
    for w in (V[0], V[6], V[7], V[8], V[11]):
        assert idx.lookup_positions(w) == doc_positions(docs, w), w
    assert idx.lookup_positions(b"absent") == []
