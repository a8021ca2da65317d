"""Shared pieces of the ranked-search tests (not a test module): synthetic
CSR indexes built with NumPy, the brute-force Python oracle, and the
5,000-document corpus of the end-to-end checks."""

import numpy as np
import torch

MASK64 = (1 << 64) - 1


def as_i64(h: int) -> int:
    return h - (1 << 64) if h >= (1 << 63) else h


class SynthIndex:
    """{u64 hash: [(doc, tf), ...]} (docs ascending, unique) as the CSR
    arrays of InvertedIndexResult, plus optional per-word weights."""

    def __init__(self, lists: dict, weights: dict = None):
        self.lists = {h: list(p) for h, p in lists.items()}
        self.hashes = sorted(self.lists)  # unsigned order
        self.weights = weights
        self.keys = np.array([as_i64(h) for h in self.hashes],
                             dtype=np.int64)
        lens = [len(self.lists[h]) for h in self.hashes]
        self.doc_offsets = np.concatenate(
            [[0], np.cumsum(lens)]).astype(np.int64)
        flat = [p for h in self.hashes for p in self.lists[h]]
        self.docs = np.array([d for d, _ in flat], dtype=np.int64)
        self.tf = np.array([t for _, t in flat], dtype=np.int64)
        self.w = (None if weights is None else
                  np.array([weights[h] for h in self.hashes],
                           dtype=np.int64))

    def tensors(self, dev, bait_keys=(), bait=True):
        """(keys, doc_offsets, docs, tf, weights or None) on dev.  With
        bait, each is the exact-size middle slice of a larger tensor whose
        neighbouring elements would add matches if a kernel read them:
        keys are flanked by bait_keys (hashes the tests query as absent),
        doc_offsets by a plausible span, docs/tf by the doc ids next to
        the first and last posting with a large tf."""
        def wrap(a, lead, trail):
            if not bait:
                return torch.from_numpy(a.copy()).to(dev)
            big = np.concatenate([np.asarray(lead, dtype=np.int64), a,
                                  np.asarray(trail, dtype=np.int64)])
            t = torch.from_numpy(big).to(dev)
            return t[len(lead):len(lead) + len(a)]

        np_ = len(self.docs)
        bk = [as_i64(h) for h in bait_keys] or [0]
        lo_doc = int(self.docs[0]) - 1 if np_ else 0
        hi_doc = int(self.docs[-1]) + 1 if np_ else 0
        out = [wrap(self.keys, bk * 4, bk[::-1] * 4),
               wrap(self.doc_offsets, [0, 0, 0], [np_, np_, np_]),
               wrap(self.docs, [lo_doc - 1, lo_doc], [hi_doc, hi_doc + 1]),
               wrap(self.tf, [1 << 40] * 2, [1 << 40] * 2)]
        out.append(None if self.w is None
                   else wrap(self.w, [1 << 20] * 2, [1 << 20] * 2))
        return out

    def ranked(self, terms, mode, weighted=True):
        """Brute force: every matching (doc, score), best first."""
        per = [dict(self.lists.get(h, ())) for h in terms]
        if not per:
            docs = set()
        elif mode == "and":
            docs = set.intersection(*[set(p) for p in per])
        else:
            docs = set.union(*[set(p) for p in per])
        use_w = weighted and self.weights is not None
        score = {}
        for d in docs:
            score[d] = sum(p[d] * (self.weights[h] if use_w else 1)
                           for h, p in zip(terms, per) if d in p)
        return sorted(score.items(), key=lambda kv: (-kv[1], kv[0]))


def expect(ranked, k):
    """Oracle outputs for one query: (docs[k], scores[k], n, hits)."""
    n = min(k, len(ranked))
    docs = [d for d, _ in ranked[:n]] + [-1] * (k - n)
    scores = [s for _, s in ranked[:n]] + [0] * (k - n)
    return docs, scores, n, len(ranked)


def run_queries(ops, tens, queries, k, mode, weighted=True):
    """One ops.postings_search launch over `queries` (lists of u64
    hashes) -> per query (docs[k], scores[k], n, hits) as Python lists."""
    keys, offs, docs, tf, w = tens
    flat = [as_i64(h) for q in queries for h in q]
    qoff = np.concatenate([[0], np.cumsum([len(q) for q in queries])])
    out = ops.postings_search(
        keys, offs, docs, tf, w if weighted else None,
        torch.tensor(flat, dtype=torch.int64),
        torch.from_numpy(qoff.astype(np.int64)), k, mode)
    d, s, n, h = [t.cpu() for t in out]
    assert d.shape == (len(queries), k) and s.shape == (len(queries), k)
    assert n.shape == (len(queries),) and h.shape == (len(queries),)
    return [(d[i].tolist(), s[i].tolist(), int(n[i]), int(h[i]))
            for i in range(len(queries))]


def check_queries(ops, index, tens, queries, ks, modes=("and", "or"),
                  weightings=(True, False)):
    """Full equality of (docs, scores, n, hits) with the oracle for every
    query, k, mode and weighting; one launch per (k, mode, weighting)."""
    for mode in modes:
        for weighted in weightings:
            ranked = [index.ranked(q, mode, weighted) for q in queries]
            for k in ks:
                got = run_queries(ops, tens, queries, k, mode, weighted)
                for q, r, g in zip(queries, ranked, got):
                    assert g == expect(r, k), (
                        f"mode={mode} weighted={weighted} k={k} "
                        f"terms={[hex(h) for h in q]}")


def random_list(rng, universe: int, length: int, tf_hi: int = 6):
    docs = np.sort(rng.choice(universe, size=length, replace=False))
    tfs = rng.integers(1, tf_hi, size=length)
    return list(zip(docs.tolist(), tfs.tolist()))


# ------------------------------------------------------------ end to end
E2E_NDOCS = 5000


def e2e_corpus():
    """-> (text u8 tensor on the host, splits, docs as lists of words).
    Every doc has "all" one to three times, even docs "even", every third
    "three" twice, doc 1234 "rare", plus 0-5 filler words out of 40."""
    rng = np.random.default_rng(2024)
    filler = [b"f%02d" % i for i in range(40)]
    docs = []
    for i in range(E2E_NDOCS):
        words = [b"all"] * int(rng.integers(1, 4))
        if i % 2 == 0:
            words.append(b"even")
        if i % 3 == 0:
            words += [b"three", b"three"]
        if i == 1234:
            words.append(b"rare")
        words += [filler[j] for j in rng.integers(0, 40,
                                                  int(rng.integers(0, 6)))]
        docs.append([words[j] for j in rng.permutation(len(words))])
    raw = [b" ".join(d) + b"\n" for d in docs]
    offs = np.concatenate([[0], np.cumsum([len(r) for r in raw])]).tolist()
    text = torch.from_numpy(np.frombuffer(b"".join(raw),
                                          dtype=np.uint8).copy())
    return text, list(zip(offs[:-1], offs[1:])), docs


def e2e_ranked(docs, terms, mode, scoring):
    """Brute force over the documents' words, best first."""
    terms = list(dict.fromkeys(terms))
    n = len(docs)
    w = {}
    for t in terms:
        df = sum(1 for d in docs if t in d)
        w[t] = (1 if scoring == "tf" or df == 0 else
                int(np.rint(65536.0 * np.log(1.0 + n / np.float64(df)))))
    out = []
    for i, d in enumerate(docs):
        present = [t for t in terms if t in d]
        ok = (len(present) == len(terms) and terms) if mode == "and" \
            else present
        if ok:
            out.append((i, sum(d.count(t) * w[t] for t in present)))
    return sorted(out, key=lambda kv: (-kv[1], kv[0]))


E2E_QUERIES = [
    [b"all"], [b"even"], [b"rare"], [b"all", b"even"], [b"even", b"three"],
    [b"all", b"even", b"three"], [b"rare", b"all"], [b"rare", b"three"],
    [b"f03", b"f17"], [b"f03", b"even", b"f39"], [b"absent"],
    [b"absent", b"all"], [b"three", b"three", b"all"],
]


def check_e2e(idx, docs):
    assert idx.ndocs == E2E_NDOCS
    for mode in ("and", "or"):
        for scoring in ("tf", "tfidf"):
            got = idx.search_batch(E2E_QUERIES, mode=mode, k=10,
                                   scoring=scoring)
            for q, g in zip(E2E_QUERIES, got):
                r = e2e_ranked(docs, q, mode, scoring)
                assert g.hits == len(r), (q, mode, scoring)
                assert g.docs == r[:10], (q, mode, scoring)
    one = idx.search([b"even", b"three"], mode="and", k=256, scoring="tfidf")
    r = e2e_ranked(docs, [b"even", b"three"], "and", "tfidf")
    assert one.hits == len(r) and one.docs == r[:256]
