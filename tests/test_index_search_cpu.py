"""Ranked multi-term search on the CPU tier: the NumPy implementation
behind ops.postings_search against the brute-force oracle, the
InvertedIndexResult.search API end to end, and the host-side checks."""

import numpy as np
import pytest
import torch

from index_search_common import (E2E_NDOCS, SynthIndex, check_e2e,
                                 check_queries, e2e_corpus, random_list,
                                 run_queries)

from mapreduce_amd import ops
from mapreduce_amd.gpu.inverted_index import (InvertedIndexJob,
                                              InvertedIndexResult,
                                              SearchResult)

TMAX, KMAX, BUF = ops.POSTINGS_TMAX, ops.POSTINGS_KMAX, ops.POSTINGS_BUF
ABSENT = 0xFFFFFFFFFFFFFFFE
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(3)
    universe = 700
    lens = [1, 2, 63, 64, 65, 255, 256, 257]
    lists = {(n * 0x9E3779B97F4A7C15 + (i << 61)) & ((1 << 64) - 1):
             random_list(rng, universe, n) for i, n in enumerate(lens)}
    lists[0x7000000000000000] = random_list(rng, universe, 500)
    weights = {h: int(rng.integers(1, 1 << 17)) for h in lists}
    index = SynthIndex(lists, weights)
    return index, index.tensors(CPU, bait_keys=(1, ABSENT))


def test_cpu_matches_oracle_small(small):
    index, tens = small
    dense = 0x7000000000000000
    queries = [[], [ABSENT], [dense, dense]]
    for h in index.hashes:
        queries += [[h], [h, dense], [dense, h, index.hashes[0]],
                    [h, ABSENT]]
    check_queries(ops, index, tens, queries, [1, 2, 10, KMAX])


def test_cpu_beyond_two_buffers():
    rng = np.random.default_rng(4)
    n = 2 * BUF + 300
    a, b = 0x8000000000000005, 0x6
    index = SynthIndex({a: [(d, 3) for d in range(n)],      # all tf equal
                        b: random_list(rng, n + 50, BUF + 1)},
                       {a: 5, b: 11})
    tens = index.tensors(CPU, bait_keys=(ABSENT,))
    check_queries(ops, index, tens, [[a], [a, b], [b, a]], [1, 10, KMAX])
    got = run_queries(ops, tens, [[a]], KMAX, "and", weighted=False)
    assert got[0] == (list(range(KMAX)), [3] * KMAX, KMAX, n)


def test_cpu_no_queries(small):
    _, (keys, offs, docs, tf, w) = small
    out = ops.postings_search(keys, offs, docs, tf, w,
                              torch.empty(0, dtype=torch.int64),
                              torch.zeros(1, dtype=torch.int64), 7, "or")
    assert [tuple(t.shape) for t in out] == [(0, 7), (0, 7), (0,), (0,)]


@pytest.fixture(scope="module")
def e2e():
    text, splits, docs = e2e_corpus()
    return InvertedIndexJob("cpu").run(text, splits), docs


def test_end_to_end_cpu_tier(e2e):
    idx, docs = e2e
    assert idx.hash_kind == "fnv1a64" and idx.ndocs == E2E_NDOCS
    lens = {w: len(idx.lookup(w)) for w in ("all", "even", "three", "rare")}
    assert lens == {"all": 5000, "even": 2500, "three": 1667, "rare": 1}
    check_e2e(idx, docs)


def test_string_and_sequence_queries_agree(e2e):
    idx, _ = e2e
    r = idx.search("all even")
    assert isinstance(r, SearchResult) and r.hits == 2500 and len(r.docs) == 10
    assert r == idx.search(["all", "even"]) == idx.search(b"all\teven\n")
    assert r == idx.search([b"all", "even", "all"])  # duplicates dropped
    assert idx.search_batch(["all even", ["rare"]], k=3) == [
        idx.search("all even", k=3), idx.search("rare", k=3)]
    assert idx.search_batch([]) == []
    assert idx.search("") == SearchResult(0, [])


def test_value_errors(e2e):
    idx, _ = e2e
    with pytest.raises(ValueError, match="k must be"):
        idx.search("all", k=0)
    with pytest.raises(ValueError, match="k must be"):
        idx.search("all", k=KMAX + 1)
    assert idx.search("all", k=KMAX).hits == 5000
    many = [f"t{i}" for i in range(TMAX + 1)]
    with pytest.raises(ValueError, match="terms per query"):
        idx.search(many, mode="or")
    assert idx.search(many[:TMAX], mode="or").hits == 0
    with pytest.raises(ValueError, match="mode"):
        idx.search("all", mode="xor")
    with pytest.raises(ValueError, match="scoring"):
        idx.search("all", scoring="bm25")
    unknown_n = InvertedIndexResult(
        keys=idx.keys, doc_offsets=idx.doc_offsets, docs=idx.docs,
        tf=idx.tf, pos=idx.pos, blob_src=idx.blob_src,
        hash_kind=idx.hash_kind)
    assert unknown_n.ndocs is None
    with pytest.raises(ValueError, match="ndocs"):
        unknown_n.search("all", scoring="tfidf")
    assert unknown_n.search("all even", scoring="tfidf", ndocs=E2E_NDOCS) \
        == idx.search("all even", scoring="tfidf")


def test_idf_weights_cached_and_match_formula(e2e):
    idx, _ = e2e
    w = idx.idf_weights()
    assert w is idx.idf_weights() and w is idx.idf_weights(E2E_NDOCS)
    assert w.dtype == torch.int64 and w.shape == idx.keys.shape
    df = np.diff(idx.doc_offsets.numpy()).astype(np.float64)
    exp = np.rint(65536.0 * np.log(1.0 + E2E_NDOCS / df)).astype(np.int64)
    assert np.array_equal(w.numpy(), exp)
    w2 = idx.idf_weights(10 * E2E_NDOCS)
    assert w2 is not w and w2 is idx.idf_weights(10 * E2E_NDOCS)
    assert int(w2.min()) > int(w.min())
    # "all" is in every document: w = rint(65536 ln 2)
    assert int(w.min()) == 45426
