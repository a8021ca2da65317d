"""Ranked multi-term search on the device (ops.postings_search and the
InvertedIndexResult.search API over it) against a brute-force Python
oracle over the same lists.  Inputs are synthetic CSR arrays (no
tokenizer), uploaded as exact-size slices of larger tensors; every size
comes from ops.postings_search_caps().  All comparisons are full equality
of (docs, scores, n, hits)."""

import numpy as np
import pytest
import torch

from index_search_common import (SynthIndex, check_e2e, check_queries,
                                 e2e_corpus, expect, random_list,
                                 run_queries)

pytestmark = pytest.mark.gpu

ABSENT_LO = 0x0000000000000001   # below every key
ABSENT_HI = 0xFFFFFFFFFFFFFFFE   # above every key
ABSENT_MID = 0x8000000000000001
FIRST = 0x0000000000000010       # first key row
LAST = 0xFFFFFFFFFFFFFF00        # last key row, negative as i64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mapreduce_amd import ops
    ops.require_gpu_ext()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops_mod():
    from mapreduce_amd import ops
    return ops


@pytest.fixture(scope="module")
def caps(dev, ops_mod):
    return ops_mod.postings_search_caps()


def lengths(caps):
    _, _, buf = caps
    return [1, 2, 63, 64, 65, 255, 256, 257, buf - 1, buf, buf + 1,
            2 * buf + 300]


@pytest.fixture(scope="module")
def sweep(dev, caps):
    """One word per list length (hash = length, spread over both halves
    of the u64 range), two dense lists, the first and last key rows."""
    tmax, _, buf = caps
    rng = np.random.default_rng(42)
    universe = 3 * buf
    lists, weights, by_len = {}, {}, {}
    for i, n in enumerate(lengths(caps)):
        h = (n * 0x9E3779B97F4A7C15 + (i << 60)) & ((1 << 64) - 1)
        by_len[n] = h
        lists[h] = random_list(rng, universe, n)
    dense = [0x7000000000000000 + i for i in range(2)]
    for h in dense:
        lists[h] = random_list(rng, universe, (universe * 2) // 3)
    # first row starts at doc 5 and the last row ends on doc universe+5,
    # the final posting of the arrays; a neighbour list holds the docs
    # just outside both, which the bait elements repeat
    lists[FIRST] = [(5, 2), (9, 1), (universe + 5, 3)]
    lists[LAST] = [(5, 1), (7, 4), (universe + 5, 2)]
    edge = 0x7000000000000010
    lists[edge] = [(3, 1), (4, 9), (5, 1), (universe + 5, 1),
                   (universe + 6, 9), (universe + 7, 9)]
    extra = [0x7100000000000000 + i for i in range(tmax)]
    for h in extra:
        lists[h] = random_list(rng, universe, int(rng.integers(200, 900)))
    for h in lists:
        weights[h] = int(rng.integers(1, 1 << 17))
    index = SynthIndex(lists, weights)
    assert index.hashes[0] == FIRST and index.hashes[-1] == LAST
    assert index.docs[-1] == universe + 5  # LAST ends the posting arrays
    tens = index.tensors(dev, bait_keys=(ABSENT_LO, ABSENT_HI))
    return index, tens, by_len, dense, edge, extra


def ks(caps):
    return [1, 2, 10, caps[1]]


def test_caps_match_python_constants(ops_mod, caps):
    assert caps == (ops_mod.POSTINGS_TMAX, ops_mod.POSTINGS_KMAX,
                    ops_mod.POSTINGS_BUF)
    assert caps[1] + 256 <= caps[2]


def test_list_lengths_and_term_counts(ops_mod, caps, sweep):
    """Every list length x T in {1, 2, 3} (+ an absent term) x k x mode x
    weights; 2*BUF+300 forces at least two prunes."""
    index, tens, by_len, dense, _, _ = sweep
    queries = []
    for n, h in by_len.items():
        queries += [[h], [h, dense[0]], [dense[0], h], [dense[1], h, dense[0]],
                    [h, ABSENT_MID], [ABSENT_HI, h, dense[0]]]
    queries += [[dense[0], dense[1]], [ABSENT_LO], [ABSENT_HI], []]
    check_queries(ops_mod, index, tens, queries, ks(caps))


def test_tmax_terms(ops_mod, caps, sweep):
    index, tens, by_len, dense, _, extra = sweep
    tmax, _, buf = caps
    queries = [extra,                                  # TMAX mid-size lists
               extra[:tmax - 1] + [by_len[2 * buf + 300]],
               [dense[0]] + extra[:tmax - 2] + [dense[1]],
               extra[:tmax - 1] + [ABSENT_MID]]
    assert all(len(q) == tmax for q in queries)
    check_queries(ops_mod, index, tens, queries, [1, 10, caps[1]])


def test_key_rows_and_posting_bounds(ops_mod, caps, sweep):
    """First and last key rows resolve (the last is negative as i64 and
    its list ends on the final posting); docs just outside the first and
    last posting, which only the bait holds, must not match."""
    index, tens, _, dense, edge, _ = sweep
    queries = [[FIRST], [LAST], [FIRST, LAST], [LAST, edge], [edge, FIRST],
               [edge, LAST, FIRST], [LAST, dense[0]]]
    check_queries(ops_mod, index, tens, queries, [1, 10])
    got = run_queries(ops_mod, tens, [[LAST]], 10, "and", weighted=False)
    assert got[0][2] == 3 and got[0][0][:3] == [7, index.docs[-1], 5]


def stress_index(caps, kind, dev):
    _, _, buf = caps
    n = 2 * buf + 300
    docs = list(range(10, 10 + 3 * n, 3))
    if kind == "equal":
        tfs = [7] * n
    elif kind == "increasing":
        tfs = list(range(1, n + 1))
    else:
        tfs = list(range(n, 0, -1))
    a, b, c = 0x11, 0x8000000000000022, 0x33
    lists = {a: list(zip(docs, tfs)),
             b: [(d, 1) for d in range(0, 10 + 3 * n + 10)],   # every doc
             c: [(d, 1) for d in docs[1::2]]}
    index = SynthIndex(lists)
    return index, index.tensors(dev, bait_keys=(ABSENT_HI,)), (a, b, c)


@pytest.mark.parametrize("kind", ["equal", "increasing", "decreasing"])
def test_tie_and_prune_stress(ops_mod, caps, dev, kind):
    """All-equal tf: the order rests on ascending doc id across prune
    boundaries; increasing: the winners arrive after every prune;
    decreasing: they must survive every prune."""
    index, tens, (a, b, c) = stress_index(caps, kind, dev)
    queries = [[a], [a, b], [b, a], [a, c], [c, a, b]]
    check_queries(ops_mod, index, tens, queries, ks(caps),
                  weightings=(False,))


def test_result_size_and_padding(ops_mod, caps, sweep):
    index, tens, by_len, dense, _, _ = sweep
    kmax = caps[1]
    # k larger than the matches: padding slots are -1 / 0
    got = run_queries(ops_mod, tens, [[by_len[2]], [by_len[63]]], kmax, "or")
    for g, n in zip(got, (2, 63)):
        assert g[2] == n and g[3] == n
        assert g[0][n:] == [-1] * (kmax - n) and g[1][n:] == [0] * (kmax - n)
        assert g == expect(index.ranked([by_len[n]], "or"), kmax)
    # a disjoint pair under AND
    lists = {0x5: [(d, 1) for d in range(0, 600, 2)],
             0x6: [(d, 1) for d in range(1, 600, 2)]}
    dj = SynthIndex(lists)
    t = dj.tensors(tens[0].device)
    got = run_queries(ops_mod, t, [[0x5, 0x6]], 10, "and")
    assert got[0] == ([-1] * 10, [0] * 10, 0, 0)
    got = run_queries(ops_mod, t, [[0x5, 0x6]], 10, "or")
    assert got[0][3] == 600 and got[0][0] == list(range(10))


def test_batch_of_mixed_queries(ops_mod, caps, sweep):
    """>= 64 mixed queries in one launch equal their one-query launches;
    includes an empty, an unknown-only and a duplicated-term query."""
    index, tens, by_len, dense, edge, extra = sweep
    rng = np.random.default_rng(9)
    pool = list(by_len.values()) + dense + extra + [FIRST, LAST, edge,
                                                    ABSENT_MID]
    queries = [[], [ABSENT_LO, ABSENT_HI], [dense[0], dense[0]],
               [extra[0], dense[1], extra[0]]]
    while len(queries) < 72:
        t = int(rng.integers(1, 5))
        queries.append([pool[i] for i in rng.integers(0, len(pool), t)])
    for mode in ("and", "or"):
        batch = run_queries(ops_mod, tens, queries, 10, mode)
        for q, g in zip(queries, batch):
            assert g == run_queries(ops_mod, tens, [q], 10, mode)[0], q
            assert g == expect(index.ranked(q, mode), 10), q
    assert batch[0] == ([-1] * 10, [0] * 10, 0, 0)
    assert batch[1] == ([-1] * 10, [0] * 10, 0, 0)


def test_no_queries(ops_mod, sweep):
    _, tens, *_ = sweep
    keys, offs, docs, tf, w = tens
    out = ops_mod.postings_search(
        keys, offs, docs, tf, w, torch.empty(0, dtype=torch.int64),
        torch.zeros(1, dtype=torch.int64), 10, "and")
    assert [tuple(t.shape) for t in out] == [(0, 10), (0, 10), (0,), (0,)]
    assert all(t.is_cuda and t.dtype == torch.int64 for t in out)


@pytest.fixture(scope="module")
def e2e(dev):
    from mapreduce_amd.gpu.inverted_index import InvertedIndexJob
    text, splits, docs = e2e_corpus()
    idx = InvertedIndexJob(dev).run(text.to(dev), splits)
    return idx, docs


def test_end_to_end_search(e2e):
    idx, docs = e2e
    assert idx.keys.is_cuda and idx.hash_kind == "wordhash64"
    check_e2e(idx, docs)
    assert idx.search("even three") == idx.search([b"even", "three"])
    assert idx.search_batch([]) == []


def test_search_batch_is_one_call(e2e, ops_mod, monkeypatch):
    idx, _ = e2e
    calls = []
    real = ops_mod.postings_search

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(ops_mod, "postings_search", spy)
    qs = [["all", "even"], "even three", [], ["absent"]] * 16
    out = idx.search_batch(qs, mode="and", k=5)
    assert len(out) == 64 and len(calls) == 1
    assert out[2].hits == 0 and out[2].docs == [] and out[3].hits == 0
    idx.search("all even")
    assert len(calls) == 2
