"""Positional index and exact-phrase search on the CPU tier: the NumPy
forms of ops.token_ordinals and ops.postings_phrase against brute-force
oracles (bytes.split() word lists, position sets), and the positional
InvertedIndexJob end to end.  The kernel sweep runs at reduced sizes (the
CPU form has no tile or buffer of its own)."""

import numpy as np
import pytest
import torch

from mapreduce_amd import ops
from mapreduce_amd.gpu.inverted_index import InvertedIndexJob
from mapreduce_amd.ops import _cpu
from phrase_common import (ABSENT, DENSE, PosIndex, REP, check_e2e,
                           check_layer, check_ordinals, check_phrase,
                           check_sweep_properties, e2e_corpus,
                           ordinal_cases, ordinal_oracle, run_phrase,
                           sweep_lists, sweep_queries)

CPU = torch.device("cpu")
BUF, BIG = 64, 300   # stand-ins for the kernel's buffer and the long slice


def u8(raw: bytes) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy())


@pytest.mark.parametrize("name,raw,starts", ordinal_cases(),
                         ids=[c[0] for c in ordinal_cases()])
def test_token_ordinals_cases(name, raw, starts):
    check_ordinals(ops, u8(raw), raw, starts, CPU)
    pos, doc, ordn = ordinal_oracle(raw, starts)
    gd, go = _cpu.token_ordinals(u8(raw),
                                 torch.tensor(pos, dtype=torch.int64),
                                 torch.tensor(starts, dtype=torch.int64))
    assert gd.tolist() == doc and go.tolist() == ordn


def test_token_ordinals_random_binary():
    rng = np.random.default_rng(5)
    for n in (1, 7, 64, 65, 1000):
        raw = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        cuts = sorted(rng.integers(0, n + 1, 3).tolist())
        check_ordinals(ops, u8(raw), raw, [0] + cuts + [n], CPU)


def test_token_ordinals_caps_and_limits():
    assert ops.token_ordinals_caps() == (ops.TOKEN_ORDINALS_GRANULE,)
    with pytest.raises(ValueError):
        ops.token_ordinals(u8(b"a b"), torch.zeros(1, dtype=torch.int64),
                           torch.empty(0, dtype=torch.int64))


@pytest.fixture(scope="module")
def sweep():
    tmax = ops.POSTINGS_TMAX
    lists, by_len, chain = sweep_lists(BUF, tmax, big=BIG)
    index = PosIndex(lists)
    return index, index.tensors(CPU, bait_keys=(ABSENT,)), by_len, chain


def test_sweep_exercises_what_it_claims(sweep):
    index, _, by_len, chain = sweep
    check_sweep_properties(index, by_len, chain, BUF, big=BIG)


def test_postings_phrase_sweep(sweep):
    index, tens, by_len, chain = sweep
    check_phrase(ops, index, tens, sweep_queries(by_len, chain, BUF),
                 [1, 10, ops.POSTINGS_KMAX])


def test_postings_phrase_batch_equals_single(sweep):
    index, tens, by_len, chain = sweep
    qs = sweep_queries(by_len, chain, BUF)[:24]
    batch = run_phrase(ops, tens, qs, 10)
    for q, g in zip(qs, batch):
        assert g == run_phrase(ops, tens, [q], 10)[0], q


def test_postings_phrase_checks(sweep):
    _, tens, _, _ = sweep
    one = torch.tensor([0, 1], dtype=torch.int64)
    h = torch.tensor([REP], dtype=torch.int64)
    for k in (0, ops.POSTINGS_KMAX + 1):
        with pytest.raises(ValueError):
            ops.postings_phrase(*tens, h, one, k)
    too_many = torch.tensor([DENSE] * (ops.POSTINGS_TMAX + 1),
                            dtype=torch.int64)
    with pytest.raises(ValueError):
        ops.postings_phrase(
            *tens, too_many,
            torch.tensor([0, ops.POSTINGS_TMAX + 1], dtype=torch.int64), 10)
    with pytest.raises(ValueError):
        ops.postings_phrase(*tens[:4], tens[4][:-1], tens[5], h, one, 10)
    out = ops.postings_phrase(*tens, torch.empty(0, dtype=torch.int64),
                              torch.zeros(1, dtype=torch.int64), 10)
    assert [tuple(t.shape) for t in out] == [(0, 10), (0, 10), (0,), (0,)]


@pytest.fixture(scope="module")
def e2e():
    text, splits, docs = e2e_corpus()
    idx = InvertedIndexJob("cpu", positions=True).run(text, splits)
    base = InvertedIndexJob("cpu").run(text, splits)
    return idx, base, docs


def test_end_to_end_phrase(e2e):
    idx, _, docs = e2e
    check_e2e(idx, docs)


def test_positional_layer_and_base_arrays(e2e):
    idx, base, docs = e2e
    check_layer(idx, base, docs)


def test_default_build_has_no_positions(e2e):
    _, base, _ = e2e
    assert base.positions is None and base.pos_offsets is None
    for call in (lambda: base.phrase("a of"),
                 lambda: base.phrase_batch([["a", "of"]]),
                 lambda: base.lookup_positions("a")):
        with pytest.raises(ValueError):
            call()
    assert base.search("a of").hits > 0  # the default surface still works


def test_positions_refuses_collectives(monkeypatch):
    from mapreduce_amd.gpu import dist as dx
    monkeypatch.setattr(dx, "force_collectives", lambda: True)
    with pytest.raises(NotImplementedError):
        InvertedIndexJob("cpu", positions=True).run(u8(b"a b"), [(0, 3)])
