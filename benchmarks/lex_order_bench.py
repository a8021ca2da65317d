"""Lexicographic-order measurements (profiles/lex_order.md).

    python benchmarks/lex_order_bench.py [--words N] [--vocab V]
                                         [--large N] [--reps R]

Times, on cuda:0, warmed, host clock around work that ends in a device
synchronise, variants alternated inside one process:

  * lex_perm() (cache cleared per repetition) on the word-count result of
    the bench corpus at its default arguments, per MR_LEX_ROUNDS setting;
  * lex_perm() on a synthetic dictionary of --large unique words (above
    the small-sort threshold: the in-tree radix path);
  * to_host(order="lex"): this tree (cold = permutation recomputed, warm =
    cached) against the previous implementation (hash-order extraction +
    Python list.sort), reproduced here verbatim as host_sort_to_host();
  * materialize(order="lex") next to materialize() in hash order.

Prints one JSON line per measurement.  A machine without a GPU fails."""

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
from mapreduce_amd.gpu.wordcount import WordCountJob, WordCountResult


def sync():
    torch.cuda.synchronize()


def timed(fn):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return (time.perf_counter() - t0) * 1e3, out


def report(name, ms, **extra):
    ms = sorted(ms)
    print(json.dumps(dict(
        name=name, reps=len(ms), median_ms=round(statistics.median(ms), 3),
        min_ms=round(ms[0], 3), max_ms=round(ms[-1], 3), **extra)),
        flush=True)


def host_sort_to_host(res):
    """to_host(order="lex") as it was before the device permutation."""
    out = res.to_host(order="hash")
    out.sort(key=lambda kv: kv[0])
    return out


def cold_perm(res):
    res._lex_perm = None
    return res.lex_perm()


def large_dictionary(n, dev):
    """n distinct words of 12..15 bytes: one of 8 five-letter prefixes, a
    7-letter base-26 id unique per word (low digit first, shuffled), 0..3
    random letters.  Chunk 0 sees the prefix and 3 id digits (8 * 26^3
    values), so for n >> 140k every word is still tied after round 0 and
    round 1 re-sorts the whole dictionary: harder than natural text."""
    rng = np.random.default_rng(11)
    ids = rng.permutation(n).astype(np.int64)
    mat = np.empty((n, 15), dtype=np.uint8)
    prefixes = rng.integers(ord("a"), ord("z") + 1, size=(8, 5),
                            dtype=np.uint8)
    mat[:, :5] = prefixes[rng.integers(0, 8, size=n)]
    for j in range(7):
        mat[:, 5 + j] = ord("a") + ids % 26
        ids //= 26
    mat[:, 12:] = rng.integers(ord("a"), ord("z") + 1, size=(n, 3),
                               dtype=np.uint8)
    lens = 12 + rng.integers(0, 4, size=n)
    mask = np.arange(15)[None, :] < lens[:, None]
    text = torch.from_numpy(mat[mask]).to(dev)
    off = np.cumsum(lens) - lens
    pos = torch.from_numpy((off << 16) | lens).to(dev)
    return text, pos


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--words", type=int, default=49_158_635)
    p.add_argument("--splits", type=int, default=197)
    p.add_argument("--vocab", type=int, default=130_000)
    p.add_argument("--large", type=int, default=3_000_000)
    p.add_argument("--reps", type=int, default=15)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lex_order_bench needs a GPU")
    ops.require_gpu_ext()
    dev = torch.device("cuda:0")

    corpus = make_corpus(dev, nwords=args.words, nsplits=args.splits,
                         vocab_size=args.vocab, seed=1234)
    res = WordCountJob(dev, vocab_estimate=max(args.vocab, 1 << 12)).run(
        corpus.text, corpus.splits())
    n = int(res.keys.numel())
    shape = dict(words=args.words, vocab=args.vocab, unique=n)

    # correctness at the timed size first: faster and different is not faster
    new = res.to_host(order="lex")
    assert new == host_sort_to_host(res), "lex order differs from host sort"

    for rounds in ("8", "1", "2", "4"):
        os.environ["MR_LEX_ROUNDS"] = rounds
        cold_perm(res)
    per = {r: [] for r in ("8", "1", "2", "4")}
    for _ in range(args.reps):
        for rounds in per:
            os.environ["MR_LEX_ROUNDS"] = rounds
            per[rounds].append(timed(lambda: cold_perm(res))[0])
    del os.environ["MR_LEX_ROUNDS"]
    for rounds, ms in per.items():
        report("lex_perm", ms, MR_LEX_ROUNDS=int(rounds), **shape)

    old_ms, cold_ms, warm_ms = [], [], []
    for _ in range(args.reps):
        old_ms.append(timed(lambda: host_sort_to_host(res))[0])
        res._lex_perm = None
        cold_ms.append(timed(lambda: res.to_host(order="lex"))[0])
        warm_ms.append(timed(lambda: res.to_host(order="lex"))[0])
    report("to_host_lex/host_sort(previous)", old_ms, **shape)
    report("to_host_lex/device_perm_cold", cold_ms, **shape)
    report("to_host_lex/device_perm_cached", warm_ms, **shape)

    hash_ms, lex_ms, lexc_ms = [], [], []
    res.materialize()
    for _ in range(args.reps):
        hash_ms.append(timed(lambda: res.materialize())[0])
        res._lex_perm = None
        lexc_ms.append(timed(lambda: res.materialize(order="lex"))[0])
        lex_ms.append(timed(lambda: res.materialize(order="lex"))[0])
    report("materialize/hash", hash_ms, **shape)
    report("materialize/lex_cold", lexc_ms, **shape)
    report("materialize/lex_cached", lex_ms, **shape)

    # large vocabulary: every full-size sort is the in-tree radix sort
    text, pos = large_dictionary(args.large, dev)
    big = WordCountResult(
        keys=torch.arange(args.large, dtype=torch.int64, device=dev),
        counts=torch.ones(args.large, dtype=torch.int64, device=dev),
        pos=pos, blob_src=text, nwords=args.large)
    perm = cold_perm(big)
    lens, blob = ops.extract_words(text, pos.index_select(0, perm))
    raw = bytes(blob.cpu().numpy().tobytes())
    ends = np.cumsum(lens.cpu().numpy())
    words = [raw[a:b] for a, b in zip(ends - lens.cpu().numpy(), ends)]
    assert all(a < b for a, b in zip(words, words[1:])), "large: not sorted"
    del words, raw
    ms = [timed(lambda: cold_perm(big))[0]
          for _ in range(max(5, args.reps // 2))]
    report("lex_perm", ms, MR_LEX_ROUNDS=8, unique=args.large,
           word_bytes="12..15",
           shape="synthetic distinct words, all tied after chunk 0")
    return 0


if __name__ == "__main__":
    sys.exit(main())
