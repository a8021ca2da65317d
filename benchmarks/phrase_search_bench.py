"""Positional index and phrase search measurements
(profiles/phrase_search.md).

    python benchmarks/phrase_search_bench.py [--part build|ordinals|query|all]
                                             [--reps R]

  build     InvertedIndexJob at the BASELINE shape (49.2M words, 197
            documents, 130k-word Zipf vocabulary) with and without
            positions=True, alternated inside one process;
  ordinals  ops.token_ordinals alone over every occurrence of that corpus,
            against the bytes it streams (the text once, 8 bytes of
            position in and 12 bytes of (doc, ord) out per occurrence);
  query     a many-document corpus (one split = one document; default
            8,000 documents of 5,000 words over a 3,000-word vocabulary,
            checked against the index job's posting table like
            index_search_bench.py): phrase_batch for 2-, 3- and 5-term
            phrases drawn from the text itself, beside
            search_batch(mode="and") on the same term sets, at 64 and 1024
            queries per call.  The answers are first compared with a host
            evaluation over lookup_positions().

Times are a host clock around work that ends in a device synchronise,
warmed.  Prints one JSON line per measurement.  A machine without a GPU
fails."""

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
from mapreduce_amd.gpu.corpus import make_corpus
from mapreduce_amd.gpu.inverted_index import InvertedIndexJob

from index_search_bench import (check_fits_job_table,  # noqa: E402
                                expected_postings)

K = 10
SEED = 1234


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def report(name, ms, **extra):
    ms = sorted(ms)
    print(json.dumps(dict(
        name=name, reps=len(ms), median_ms=round(statistics.median(ms), 3),
        min_ms=round(ms[0], 3), max_ms=round(ms[-1], 3), **extra)),
        flush=True)
    return statistics.median(ms)


def host_phrase(idx, terms, k=K):
    """The phrase evaluated on the host from lookup_positions()."""
    lists = [dict(idx.lookup_positions(t)) for t in terms]
    docs = set.intersection(*[set(l) for l in lists])
    out = []
    for d in docs:
        sets = [set(l[d]) for l in lists]
        c = sum(1 for s in sets[0]
                if all(s + i in ps for i, ps in enumerate(sets)))
        if c:
            out.append((d, c))
    out.sort(key=lambda kv: (-kv[1], kv[0]))
    return len(out), out[:k]


def part_build(dev, args):
    corpus = make_corpus(dev, nwords=args.base_words,
                         nsplits=args.base_splits,
                         vocab_size=args.base_vocab, seed=77)
    splits = corpus.splits()
    shape = dict(words=args.base_words, docs=args.base_splits,
                 vocab=args.base_vocab, text_bytes=int(corpus.text.numel()))
    plain = InvertedIndexJob(dev)
    posit = InvertedIndexJob(dev, positions=True)
    for _ in range(2):
        base = plain.run(corpus.text, splits)
        idx = posit.run(corpus.text, splits)
    for name in ("keys", "doc_offsets", "docs", "tf"):
        assert torch.equal(getattr(idx, name), getattr(base, name)), name
    assert idx.positions.numel() == args.base_words
    a, b = [], []
    for _ in range(args.reps):
        a.append(timed(lambda: plain.run(corpus.text, splits))[0])
        b.append(timed(lambda: posit.run(corpus.text, splits))[0])
    report("build positions=False", a, **shape)
    report("build positions=True", b, **shape,
           postings=int(idx.docs.numel()),
           occurrences=int(idx.positions.numel()))


def part_ordinals(dev, args):
    corpus = make_corpus(dev, nwords=args.base_words,
                         nsplits=args.base_splits,
                         vocab_size=args.base_vocab, seed=77)
    splits = corpus.splits()
    starts = torch.tensor([s for s, _ in splits] + [splits[-1][1]],
                          device=dev, dtype=torch.int64)
    _, p, n = ops.tokenize_words(corpus.text)
    assert n == args.base_words
    # the tokenizer appends in no particular order; the check below wants
    # text order (the op itself does not)
    ps = torch.sort(p).values
    doc, ordn = ops.token_ordinals(corpus.text, ps, starts)
    # ordinals of a text-ordered stream restart at 0 and step by 1
    want = torch.searchsorted(starts, ps >> 16, right=True) - 1
    assert torch.equal(doc, want)
    step = ordn[1:] - ordn[:-1]
    same = doc[1:] == doc[:-1]
    assert bool(((step == 1) | ~same).all())
    assert bool((ordn[1:][~same] == 0).all()) and int(ordn[0]) == 0
    ms = [timed(lambda: ops.token_ordinals(corpus.text, p, starts))[0]
          for _ in range(args.reps)]
    nbytes = int(corpus.text.numel()) + 20 * n
    med = report("token_ordinals", ms, occurrences=n,
                 text_bytes=int(corpus.text.numel()), bytes_streamed=nbytes)
    print(json.dumps(dict(name="token_ordinals rate",
                          gb_per_s=round(nbytes / (med * 1e-3) / 1e9, 1),
                          text_gb_per_s=round(int(corpus.text.numel())
                                              / (med * 1e-3) / 1e9, 1))),
          flush=True)


def part_query(dev, args):
    corpus = make_corpus(dev, nwords=args.words, nsplits=args.splits,
                         vocab_size=args.vocab, seed=SEED)
    check_fits_job_table(int(corpus.text.numel()),
                         expected_postings(args.words, args.splits,
                                           args.vocab))
    build_ms, idx = timed(lambda: InvertedIndexJob(
        dev, positions=True).run(corpus.text, corpus.splits()))
    shape = dict(words=args.words, docs=args.splits, vocab=args.vocab,
                 postings=int(idx.docs.numel()),
                 occurrences=int(idx.positions.numel()))
    print(json.dumps(dict(name="index positions=True",
                          build_ms=round(build_ms, 1), **shape)), flush=True)

    # phrases that occur: T consecutive words read from the text itself
    ndoc = min(256, args.splits)
    offs = corpus.split_offsets[:ndoc + 1]
    head = bytes(corpus.text[:offs[-1]].cpu().numpy().tobytes())
    lines = [head[a:b].split() for a, b in zip(offs[:-1], offs[1:])]
    rng = np.random.default_rng(SEED)
    for t in (2, 3, 5):
        qs = []
        while len(qs) < 1024:
            ln = lines[int(rng.integers(0, len(lines)))]
            if len(ln) >= t:
                at = int(rng.integers(0, len(ln) - t + 1))
                qs.append(ln[at:at + t])
        got = idx.phrase_batch(qs, k=K)
        for q, g in list(zip(qs, got))[:6]:
            assert (g.hits, g.docs) == host_phrase(idx, q), q
        both = idx.search_batch(qs, mode="and", k=K)
        assert all(p.hits <= a.hits for p, a in zip(got, both))
        print(json.dumps(dict(
            name="queries", terms=t, n=len(qs), k=K,
            phrase_hits_median=int(np.median([g.hits for g in got])),
            and_hits_median=int(np.median([g.hits for g in both])))),
            flush=True)
        for nq in (64, 1024):
            sub = qs[:nq]
            idx.phrase_batch(sub, k=K)
            idx.search_batch(sub, mode="and", k=K)
            a, b = [], []
            for _ in range(args.reps):
                a.append(timed(lambda: idx.phrase_batch(sub, k=K))[0])
                b.append(timed(
                    lambda: idx.search_batch(sub, mode="and", k=K))[0])
            ma = statistics.median(a)
            mb = statistics.median(b)
            report("phrase_batch(k=10)", a, terms=t, nq=nq,
                   queries_per_s=round(nq / (ma * 1e-3), 1))
            report("search_batch(and,k=10)", b, terms=t, nq=nq,
                   queries_per_s=round(nq / (mb * 1e-3), 1))


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--part", default="all",
                   choices=["build", "ordinals", "query", "all"])
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--base-words", type=int, default=49_158_635)
    p.add_argument("--base-splits", type=int, default=197)
    p.add_argument("--base-vocab", type=int, default=130_000)
    p.add_argument("--words", type=int, default=40_000_000)
    p.add_argument("--splits", type=int, default=8_000)
    p.add_argument("--vocab", type=int, default=3_000)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("phrase_search_bench needs a GPU")
    ops.require_gpu_ext()
    dev = torch.device("cuda:0")
    for name, fn in (("build", part_build), ("ordinals", part_ordinals),
                     ("query", part_query)):
        if args.part in (name, "all"):
            fn(dev, args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
