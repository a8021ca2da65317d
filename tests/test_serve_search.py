"""GET /search of mapreduce_amd.serve: ranked multi-term queries over a
mounted inverted index, against a brute-force pass over the documents."""

import pytest

fastapi = pytest.importorskip("fastapi")
from fastapi.testclient import TestClient  # noqa: E402

from index_search_common import e2e_corpus, e2e_ranked  # noqa: E402

from mapreduce_amd import ops  # noqa: E402
from mapreduce_amd.gpu.inverted_index import InvertedIndexJob  # noqa: E402
from mapreduce_amd.serve import make_app  # noqa: E402


@pytest.fixture(scope="module")
def served():
    text, splits, docs = e2e_corpus()
    idx = InvertedIndexJob("cpu").run(text, splits)
    return TestClient(make_app(index=idx)), docs


@pytest.mark.parametrize("mode", ["and", "or"])
@pytest.mark.parametrize("scoring", ["tf", "tfidf"])
def test_search_matches_oracle(served, mode, scoring):
    client, docs = served
    for q in ("even three", "all", "rare all", "f03 f17 even", "absent all"):
        r = client.get("/search", params={"q": q, "mode": mode, "k": 7,
                                          "scoring": scoring})
        assert r.status_code == 200, r.text
        body = r.json()
        exp = e2e_ranked(docs, q.encode().split(), mode, scoring)
        assert body["query"] == q and body["terms"] == q.split()
        assert body["hits"] == len(exp)
        assert [(e["doc"], e["score"]) for e in body["results"]] == exp[:7]


def test_search_defaults(served):
    client, docs = served
    body = client.get("/search", params={"q": "even  even\tthree"}).json()
    exp = e2e_ranked(docs, [b"even", b"three"], "and", "tf")
    assert body["terms"] == ["even", "three"]  # split, duplicates dropped
    assert body["hits"] == len(exp) and len(body["results"]) == 10
    assert [(e["doc"], e["score"]) for e in body["results"]] == exp[:10]


def test_search_unmounted_404():
    client = TestClient(make_app())
    assert client.get("/search", params={"q": "x"}).status_code == 404


def test_search_rejects_out_of_range(served):
    client, _ = served
    kmax = ops.POSTINGS_KMAX
    for params in ({"q": "all", "k": 0}, {"q": "all", "k": kmax + 1},
                   {"q": "all", "k": "ten"}, {"q": "all", "mode": "xor"},
                   {"q": "all", "scoring": "bm25"}, {},
                   {"q": " ".join(f"t{i}" for i in range(
                       ops.POSTINGS_TMAX + 1)), "mode": "or"}):
        assert client.get("/search", params=params).status_code in (400, 422)
    assert client.get("/search",
                      params={"q": "all", "k": kmax}).status_code == 200
