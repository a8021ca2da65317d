"""Positional index and exact-phrase search on the device: the
token_ordinals kernels against the bytes.split() oracle and the CPU form,
ops.postings_phrase against a brute-force oracle over position lists, and
the positional InvertedIndexJob end to end against the documents' word
lists.  Inputs are exact-size slices of larger tensors whose neighbouring
elements would change the answer if a kernel read them; every size comes
from the caps functions.  All comparisons are full equality."""

import numpy as np
import pytest
import torch

from phrase_common import (ABSENT, BAIT_V, BAIT_W, LAST_KEY, PosIndex,
                           check_e2e, check_layer, check_ordinals,
                           check_phrase, check_sweep_properties,
                           driver_lengths, e2e_corpus, ordinal_cases,
                           run_phrase, sweep_lists, sweep_queries)

pytestmark = pytest.mark.gpu


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


def flanked(raw: bytes, dev, lead: int = 13):
    """raw on the device as an exact-size slice of a larger tensor whose
    flanking bytes are non-whitespace: a read of text[-1] merges the first
    word into a longer one (it loses its start), a read of text[n] cannot
    add a word but changes a carry.  lead = 13 leaves the slice unaligned;
    a multiple of 8 keeps the 8-byte loads."""
    big = np.frombuffer(b"#" * lead + raw + b"#" * 19, dtype=np.uint8).copy()
    return torch.from_numpy(big).to(dev)[lead:lead + len(raw)]


# ---------------------------------------------------------------- ordinals
def test_ordinals_caps(ops_mod, dev):
    (g,) = ops_mod.token_ordinals_caps()
    assert g == ops_mod.TOKEN_ORDINALS_GRANULE and g % 8 == 0


@pytest.mark.parametrize("lead", [13, 16])
def test_ordinals_whitespace_cases(ops_mod, dev, lead):
    from mapreduce_amd.ops import _cpu
    for name, raw, starts in ordinal_cases():
        t = flanked(raw, dev, lead)
        p, s, gd, go = check_ordinals(ops_mod, t, raw, starts, dev)
        cd, co = _cpu.token_ordinals(t.cpu(), p.cpu(), s.cpu())
        assert torch.equal(gd.cpu(), cd) and torch.equal(go.cpu(), co), name


@pytest.mark.parametrize("lead", [13, 16])
def test_ordinals_random_binary_lengths(ops_mod, dev, lead):
    """Random bytes (a quarter of them whitespace, all 256 values present)
    at the lengths around the 8-byte unit, the granule and the block."""
    from mapreduce_amd.ops import _cpu
    (g,) = ops_mod.token_ordinals_caps()
    rng = np.random.default_rng(11)
    ws = np.frombuffer(b" \t\n\v\f\r", dtype=np.uint8)
    for n in (0, 1, 7, 8, 9, g - 1, g, g + 1, 4095, 4096, 4097,
              3 * 4096 + 5):
        a = rng.integers(0, 256, n, dtype=np.uint8)
        mask = rng.random(n) < 0.25
        a[mask] = ws[rng.integers(0, 6, int(mask.sum()))]
        raw = a.tobytes()
        cuts = sorted(rng.integers(0, n + 1, 5).tolist())
        starts = [0] + cuts + [n]
        t = flanked(raw, dev, lead)
        p, s, gd, go = check_ordinals(ops_mod, t, raw, starts, dev)
        cd, co = _cpu.token_ordinals(t.cpu(), p.cpu(), s.cpu())
        assert torch.equal(gd.cpu(), cd) and torch.equal(go.cpu(), co), n


# ------------------------------------------------------------ phrase kernel
@pytest.fixture(scope="module")
def sweep(dev, caps):
    tmax, _, buf = caps
    lists, by_len, chain = sweep_lists(buf, tmax)
    index = PosIndex(lists)
    return index, index.tensors(dev, bait_keys=(ABSENT,)), by_len, chain


def test_sweep_exercises_what_it_claims(sweep, caps):
    index, _, by_len, chain = sweep
    assert sorted(by_len) == sorted(driver_lengths(caps[2]))
    check_sweep_properties(index, by_len, chain, caps[2])


def test_phrase_sweep(ops_mod, caps, sweep):
    """Driver lengths 1 .. 2*BUF+300 (prunes), T in {1, 2, 3, TMAX},
    repeated terms, the p < r guard, the 5000-position posting, equal
    scores across prunes, unknown term, empty query; k in {1, 10, KMAX}."""
    index, tens, by_len, chain = sweep
    check_phrase(ops_mod, index, tens,
                 sweep_queries(by_len, chain, caps[2]), [1, 10, caps[1]])


def test_phrase_slice_bounds_bait(ops_mod, sweep):
    """Neighbouring slices and the elements next to the arrays hold the
    ordinals that would complete a phrase; none may be read."""
    index, tens, _, _ = sweep
    got = run_phrase(ops_mod, tens, [[BAIT_W, BAIT_W], [BAIT_W, BAIT_V],
                                     [LAST_KEY, LAST_KEY]], 10)
    none = ([-1] * 10, [0] * 10, 0, 0)
    assert got[0] == none and got[2] == none
    assert got[1] == ([10] + [-1] * 9, [1] + [0] * 9, 1, 1)


def test_phrase_batch_of_mixed_queries(ops_mod, caps, sweep):
    """64 mixed queries in one launch equal their one-query launches."""
    index, tens, by_len, chain = sweep
    qs = sweep_queries(by_len, chain, caps[2])
    rng = np.random.default_rng(3)
    pool = sorted(index.lists)
    while len(qs) < 64:
        qs.append([pool[i] for i in rng.integers(0, len(pool),
                                                 int(rng.integers(1, 5)))])
    qs = qs[:64]
    batch = run_phrase(ops_mod, tens, qs, 10)
    for q, g in zip(qs, batch):
        assert g == run_phrase(ops_mod, tens, [q], 10)[0], q


def test_phrase_no_queries(ops_mod, sweep):
    _, tens, _, _ = sweep
    out = ops_mod.postings_phrase(
        *tens, torch.empty(0, dtype=torch.int64),
        torch.zeros(1, dtype=torch.int64), 10)
    assert [tuple(t.shape) for t in out] == [(0, 10), (0, 10), (0,), (0,)]
    assert all(t.is_cuda and t.dtype == torch.int64 for t in out)


# ------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def e2e(dev):
    from mapreduce_amd.gpu.inverted_index import InvertedIndexJob
    text, splits, docs = e2e_corpus()
    t = text.to(dev)
    idx = InvertedIndexJob(dev, positions=True).run(t, splits)
    base = InvertedIndexJob(dev).run(t, splits)
    return idx, base, docs


def test_end_to_end_phrase(e2e):
    idx, _, docs = e2e
    assert idx.keys.is_cuda and idx.positions.is_cuda
    assert idx.hash_kind == "wordhash64"
    check_e2e(idx, docs)


def test_positional_and_default_builds_agree(e2e):
    idx, base, docs = e2e
    check_layer(idx, base, docs)
    with pytest.raises(ValueError):
        base.phrase("a of")


def test_phrase_batch_is_one_call(e2e, ops_mod, monkeypatch):
    idx, _, _ = e2e
    calls = []
    real = ops_mod.postings_phrase

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(ops_mod, "postings_phrase", spy)
    qs = [["a", "of"], "european parliament", [], ["absent", "a"]] * 16
    out = idx.phrase_batch(qs, k=5)
    assert len(out) == 64 and len(calls) == 1
    assert out[0].hits > 5 and len(out[0].docs) == 5
    assert out[2].hits == 0 and out[2].docs == [] and out[3].hits == 0
    idx.phrase("a of")
    assert len(calls) == 2


def test_positions_refuses_lds_cache(dev, monkeypatch):
    from mapreduce_amd.gpu.inverted_index import InvertedIndexJob
    monkeypatch.setenv("MR_II_CACHE", "1")
    t = torch.from_numpy(np.frombuffer(b"a b a\n", dtype=np.uint8).copy())
    with pytest.raises(ValueError):
        InvertedIndexJob(dev, positions=True).run(t.to(dev), [(0, 6)])
