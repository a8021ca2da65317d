"""GET /phrase of mapreduce_amd.serve over a CPU-tier positional index."""

import pytest

fastapi = pytest.importorskip("fastapi")
from fastapi.testclient import TestClient  # noqa: E402

from mapreduce_amd.gpu.inverted_index import InvertedIndexJob
from mapreduce_amd.serve import make_app
from phrase_common import doc_phrase_ranked, e2e_corpus


@pytest.fixture(scope="module")
def served():
    text, splits, docs = e2e_corpus()
    idx = InvertedIndexJob("cpu", positions=True).run(text, splits)
    base = InvertedIndexJob("cpu").run(text, splits)
    return (TestClient(make_app(index=idx)), TestClient(make_app(index=base)),
            docs)


def test_phrase_endpoint_equals_oracle(served):
    client, _, docs = served
    for q, k in (("european parliament", 10), ("the  the\talpha", 10),
                 ("a of a of", 3), ("alpha beta gamma delta", 10),
                 ("absent alpha", 10), ("x x x", 256)):
        r = client.get("/phrase", params={"q": q, "k": k})
        assert r.status_code == 200, r.text
        body = r.json()
        want = doc_phrase_ranked(docs, [t.encode() for t in q.split()])
        assert body["query"] == q and body["terms"] == q.split()
        assert body["hits"] == len(want)
        assert [(e["doc"], e["score"]) for e in body["results"]] == want[:k]
    # same body shape as /search
    s = client.get("/search", params={"q": "a of"}).json()
    p = client.get("/phrase", params={"q": "a of"}).json()
    assert set(s) == set(p) and p["hits"] <= s["hits"]


def test_phrase_422(served):
    client, plain, _ = served
    for k in (0, 257):
        assert client.get("/phrase", params={"q": "a of", "k": k}
                          ).status_code == 422
    many = " ".join(["a"] * 17)
    assert client.get("/phrase", params={"q": many}).status_code == 422
    # an index built without positions
    r = plain.get("/phrase", params={"q": "a of"})
    assert r.status_code == 422 and "positions" in r.json()["detail"]
    assert plain.get("/search", params={"q": "a of"}).status_code == 200


def test_phrase_unmounted_404():
    client = TestClient(make_app())
    assert client.get("/phrase", params={"q": "a of"}).status_code == 404


def test_build_from_files_with_positions(tmp_path):
    from mapreduce_amd.serve import build_results_from_files

    p1 = tmp_path / "a.txt"
    p2 = tmp_path / "b.txt"
    p1.write_text("alpha beta alpha gamma\n")
    p2.write_text("beta  alpha beta\talpha gamma\n")
    wc, ix = build_results_from_files([str(p1), str(p2)], device="cpu",
                                      positions=True)
    client = TestClient(make_app(wordcount=wc, index=ix))
    r = client.get("/phrase", params={"q": "beta alpha"}).json()
    assert [(e["doc"], e["score"]) for e in r["results"]] == [(1, 2), (0, 1)]
    _, plain = build_results_from_files([str(p1), str(p2)], device="cpu")
    assert plain.positions is None
