"""Ranked index search measurements (profiles/index_search.md).

    python benchmarks/index_search_bench.py [--words N] [--splits D]
                                            [--vocab V] [--reps R]

Builds the inverted index of a many-document corpus on cuda:0 (one split
= one document; the default shape is 10^5 documents of 2,500 words over a
3,000-word Zipf vocabulary, so every list holds thousands of documents
and the index job's posting table still fits), then answers the same two-term AND top-10 queries two
ways, at 1, 64 and 1024 queries per call:

  * batched: InvertedIndexResult.search_batch — one postings_search
    launch, two uploads and one readback per call;
  * host (what the tree offered before search existed): lookup() per
    term, then intersect, score and sort in Python (host_search below).

Both must give the same answers before anything is timed.  Times are a
host clock around work that ends in a device synchronise (a readback),
warmed, the two paths alternated inside one process.  Prints one JSON
line per measurement.  A machine without a GPU fails."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from mapreduce_amd import ops
from mapreduce_amd.gpu.corpus import _build_vocab, make_corpus
from mapreduce_amd.gpu.inverted_index import InvertedIndexJob

K = 10
SEED = 1234


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def report(name, nq, ms, **extra):
    ms = sorted(ms)
    med = statistics.median(ms)
    print(json.dumps(dict(
        name=name, nq=nq, reps=len(ms), median_ms=round(med, 3),
        min_ms=round(ms[0], 3), max_ms=round(ms[-1], 3),
        queries_per_s=round(nq / (med * 1e-3), 1), **extra)), flush=True)


def host_search(idx, terms, k=K):
    """Two-or-more-term AND top-k with what the index offered before
    search(): each term's postings pulled to the host by lookup(), then
    intersected, scored (sum of tf) and sorted in Python."""
    lists = [idx.lookup(t) for t in terms]
    score = dict(lists[0])
    for other in lists[1:]:
        o = dict(other)
        score = {d: s + o[d] for d, s in score.items() if d in o}
    ranked = sorted(score.items(), key=lambda kv: (-kv[1], kv[0]))
    return len(ranked), ranked[:k]


def expected_postings(words: int, docs: int, vocab: int,
                      zipf_s: float = 1.07) -> float:
    """Expected unique (word, doc) pairs of make_corpus's Zipf draw."""
    p = np.arange(1, vocab + 1, dtype=np.float64) ** (-zipf_s)
    p /= p.sum()
    return docs * float((1.0 - (1.0 - p) ** (words / docs)).sum())


def check_fits_job_table(text_bytes: int, postings: float) -> None:
    """InvertedIndexJob counts unique postings in an open-addressing table
    sized from the text (next_pow2(2 * bytes / 36) slots): built for long
    documents, where a word repeats within its document.  A corpus with
    more unique postings than slots never finishes probing, so a shape
    that would load the table past 0.6 is refused here."""
    slots = ops._next_pow2(2 * max(1 << 16, text_bytes // 36))
    if postings > 0.6 * slots:
        raise SystemExit(
            f"corpus shape does not fit the index job: ~{postings:.3g} "
            f"unique postings for a {slots}-slot table; use longer "
            "documents (more --words per split) or a smaller --vocab")


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--words", type=int, default=250_000_000)
    p.add_argument("--splits", type=int, default=100_000)
    p.add_argument("--vocab", type=int, default=3_000)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--host-reps", type=int, default=3,
                   help="repetitions of the host path at nq = 64 "
                        "(nq = 1 takes --reps, nq = 1024 is timed once)")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("index_search_bench needs a GPU")
    ops.require_gpu_ext()
    dev = torch.device("cuda:0")

    corpus = make_corpus(dev, nwords=args.words, nsplits=args.splits,
                         vocab_size=args.vocab, seed=SEED)
    check_fits_job_table(int(corpus.text.numel()),
                         expected_postings(args.words, args.splits,
                                           args.vocab))
    build_ms, idx = timed(
        lambda: InvertedIndexJob(dev).run(corpus.text, corpus.splits()))
    df = (idx.doc_offsets[1:] - idx.doc_offsets[:-1]).cpu().numpy()
    shape = dict(words=args.words, docs=args.splits, vocab=args.vocab,
                 unique_words=int(idx.keys.numel()),
                 postings=int(idx.docs.numel()))
    print(json.dumps(dict(
        name="index", build_ms=round(build_ms, 1),
        list_len_max=int(df.max()), list_len_median=int(np.median(df)),
        list_len_p99=int(np.percentile(df, 99)), **shape)), flush=True)

    # query terms by Zipf rank, log-uniform over the head and the middle
    # of the vocabulary: list lengths from every document down to a few
    words = _build_vocab(args.vocab, SEED + 1)
    rng = np.random.default_rng(SEED)
    hi = np.log(min(args.vocab, 10_000))
    ranks = np.exp(rng.uniform(0.0, hi, size=(1024, 2))).astype(np.int64) - 1
    queries = [[words[a], words[b if b != a else a + 1]]  # two distinct
               for a, b in ranks.tolist()]

    # same answers first: faster and different is not faster
    got = idx.search_batch(queries, mode="and", k=K)
    want = [host_search(idx, q) for q in queries]
    assert [(g.hits, g.docs) for g in got] == want, \
        "batched search differs from the host path"
    lens = sorted(min(len(idx.lookup(t)) for t in q) for q in queries[:64])
    print(json.dumps(dict(
        name="queries", n=len(queries), terms=2, mode="and", k=K,
        hits_median=int(np.median([g.hits for g in got])),
        hits_max=max(g.hits for g in got),
        driver_len_median_first64=lens[len(lens) // 2])), flush=True)

    for nq in (1, 64, 1024):
        idx.search_batch(queries[:nq], mode="and", k=K)  # warm this grid
        host_reps = (args.reps if nq == 1 else
                     args.host_reps if nq <= 64 else 1)
        batched, host = [], []
        for r in range(max(args.reps, host_reps)):
            # nq = 1 walks the query list so no single pair decides it
            qs = queries[r:r + 1] if nq == 1 else queries[:nq]
            if r < args.reps:
                batched.append(timed(
                    lambda: idx.search_batch(qs, mode="and", k=K))[0])
            if r < host_reps:
                host.append(timed(
                    lambda: [host_search(idx, q) for q in qs])[0])
        report("search_batch(and,k=10)", nq, batched, **shape)
        report("host lookup+intersect(previous)", nq, host, **shape)
    return 0


if __name__ == "__main__":
    sys.exit(main())
