"""The generators and oracles of graph_common, and ops.graph_propagate /
ops.pagerank_update through the CPU tier on every kernel case: the same
cases the device runs in test_graph_gpu, sized by the Python constants."""

import math

import numpy as np
import pytest
import torch

import graph_common as gc
from mapreduce_amd import ops

E = ops.GRAPH_TILE
CASES = gc.kernel_cases(E)


def test_caps_on_the_cpu_tier_are_the_python_constants():
    if not torch.cuda.is_available():
        assert ops.graph_caps() == (ops.GRAPH_TILE, ops.GRAPH_PR_BLOCKS)
    assert E == 256 * 8


def test_kernel_cases_have_the_shapes_they_claim():
    for name, (off, src) in CASES.items():
        gc.check_case(off, src)
    for m in (0, 1, 63, 64, 65, E - 1, E, E + 1, 3 * E + 17):
        assert len(CASES[f"m{m}"][1]) == m
    assert len(CASES["n0"][0]) == 1
    off, src = CASES["n1_selfloops"]
    assert len(off) == 2 and set(src.tolist()) == {0}
    hub = 5 * E + 3
    for name, start in (("hub_mid", 100), ("hub_head_on_tile", E),
                        ("hub_tail_on_tile", E - 3)):
        off, _ = CASES[name]
        v = int(np.argmax(np.diff(off)))
        assert off[v + 1] - off[v] == hub and off[v] == start
        assert v > 0 and v < len(off) - 2
    assert CASES["hub_mid"][0][34] % E != 0
    assert CASES["hub_head_on_tile"][0][683] % E == 0
    off, _ = CASES["hub_tail_on_tile"]
    v = int(np.argmax(np.diff(off)))
    assert off[v + 1] % E == 0 and off[v] % E != 0
    off, src = CASES["empties"]
    deg = np.diff(off)
    assert len(deg) == 40 * E and len(src) == E + 1
    full = np.nonzero(deg)[0]
    assert full[0] >= 1000 and full[-1] < 40 * E - 1000
    assert np.diff(full).max() > 30 * E
    off, src = CASES["singles"]
    assert (np.diff(off) == 1).all() and len(src) == 2 * E + 5
    deg = np.diff(CASES["mixed"][0])
    assert deg.max() == 3 * E and 7 * E < deg.sum() < 9 * E
    assert (deg == 0).any() and np.sort(deg)[-2] <= 400


def _run(off, src, x, op):
    return ops.graph_propagate(torch.from_numpy(off), torch.from_numpy(src),
                               torch.from_numpy(x), op)


@pytest.mark.parametrize("name", sorted(CASES))
def test_cpu_tier_matches_the_oracle(name):
    off, src = CASES[name]
    n = len(off) - 1
    xi = gc.values_i64(n)
    for op in ("sum", "min", "max"):
        got = _run(off, src, xi, op)
        assert got.dtype == torch.int64
        assert got.tolist() == gc.propagate_oracle(off, src, xi, op)
    for x in (gc.values_dyadic(n, 5), gc.values_general(n, 6)):
        got = _run(off, src, x, "sum")
        assert got.dtype == torch.float64
        exp = gc.propagate_oracle(off, src, x, "sum")
        assert got.numpy().tobytes() == np.array(
            exp, dtype=np.float64).tobytes()


def test_sums_wrap_and_dyadic_sums_stay_below_two_to_the_32():
    off, src = CASES["mixed"]
    n = len(off) - 1
    xi = gc.values_i64(n)
    assert len(set(xi.tolist())) == n
    exact = [sum(xi[src[off[v]:off[v + 1]]].tolist()) for v in range(n)]
    assert any(not gc.I64_MIN <= s <= gc.I64_MAX for s in exact)
    xd = gc.values_dyadic(n, 5)
    assert ((xd * (1 << 20)) % 1 == 0).all()
    assert max(s for _, s in gc.row_abs_sums(off, src, xd)) < 2.0 ** 32


def test_identity_of_empty_rows_and_bad_src_on_the_cpu_tier():
    off = np.array([0, 0, 2, 4, 4], dtype=np.int64)
    src = np.array([1, -1, 4, 3], dtype=np.int32)
    xi = np.array([10, 20, 30, 40], dtype=np.int64)
    assert _run(off, src, xi, "sum").tolist() == [0, 20, 40, 0]
    assert _run(off, src, xi, "min").tolist() == [
        gc.I64_MAX, 20, 40, gc.I64_MAX]
    assert _run(off, src, xi, "max").tolist() == [
        gc.I64_MIN, 20, 40, gc.I64_MIN]
    assert gc.propagate_oracle(off, src, xi, "min") == [
        gc.I64_MAX, 20, 40, gc.I64_MAX]
    xf = xi.astype(np.float64)
    assert _run(off, src, xf, "sum").tolist() == [0.0, 20.0, 40.0, 0.0]


def test_refusals_on_the_cpu_tier():
    off = torch.tensor([0, 1], dtype=torch.int64)
    src = torch.tensor([0], dtype=torch.int32)
    x = torch.tensor([1.5], dtype=torch.float64)
    with pytest.raises(TypeError, match="src must be int32"):
        ops.graph_propagate(off, src.to(torch.int64), x)
    with pytest.raises(TypeError, match="graph min needs int64 values"):
        ops.graph_propagate(off, src, x, "min")
    with pytest.raises(TypeError, match="x must be int64 or float64"):
        ops.graph_propagate(off, src, x.to(torch.float32))
    with pytest.raises(ValueError, match="offsets must hold 2 entries"):
        ops.graph_propagate(off[:1], src, x)
    with pytest.raises(ValueError, match="op must be"):
        ops.graph_propagate(off, src, x, "mean")


def test_pagerank_update_on_the_cpu_tier():
    sums = torch.tensor([0.1, 0.2, 0.0, 0.3], dtype=torch.float64)
    old = torch.tensor([0.25] * 4, dtype=torch.float64)
    inv = torch.tensor([0.5, 0.0, 1.0, 0.0], dtype=torch.float64)
    dang = torch.tensor(0.4, dtype=torch.float64)
    new, contrib, partials = ops.pagerank_update(sums, old, inv, 0.85, dang)
    exp = [0.15 / 4 + 0.85 * (s + 0.4 / 4) for s in sums.tolist()]
    assert new.tolist() == pytest.approx(exp, rel=1e-15)
    assert contrib.tolist() == pytest.approx(
        [e * i for e, i in zip(exp, inv.tolist())], rel=1e-15)
    p = partials.sum(0).tolist()
    assert partials.shape[1] == 2
    assert p[0] == pytest.approx(sum(abs(e - 0.25) for e in exp), rel=1e-14)
    assert p[1] == pytest.approx(exp[1] + exp[3], rel=1e-14)
    with pytest.raises(TypeError, match="sums must be float64"):
        ops.pagerank_update(sums.float(), old, inv, 0.85, dang)


def test_job_cases_hold_what_the_pagerank_tests_need():
    s, d = gc.multigraph(11, 300, 3000)
    f = gc.graph_features(s, d)
    assert f["dangling"] >= 5 and f["source_only"] >= 5
    assert f["parallel"] >= 20 and f["self_loops"] >= 20
    assert f["max_indeg"] > len(s) // 4
    assert min(s + d) < 0 < max(s + d)
    ranks, iters, deltas = gc.pagerank_oracle(s, d, 0.85, 20)
    assert iters == 20 and abs(math.fsum(ranks.values()) - 1) < 1e-12
    assert all(a > b for a, b in zip(deltas, deltas[1:]))
    assert gc.pagerank_bound(s, d, 20) < 1e-9


def test_early_stop_tol_is_ten_times_away_from_every_delta():
    s, d = gc.multigraph(11, 300, 3000)
    _, _, deltas = gc.pagerank_oracle(s, d, gc.EARLY_DAMPING, 8)
    tol = gc.early_stop_tol(deltas)
    assert all(x >= 10 * tol or x * 10 <= tol for x in deltas), (tol, deltas)
    assert deltas[1] > tol > deltas[2]
    _, iters, ds = gc.pagerank_oracle(s, d, gc.EARLY_DAMPING, 8, tol)
    assert iters == 3 and ds[-1] <= tol


def test_component_cases_and_the_union_find_oracle():
    cases = gc.component_cases()
    for name in ("path_sorted", "path_zigzag", "path_random"):
        s, d = cases[name]
        lab = gc.component_oracle(s, d)
        assert len(lab) == 1 << 12 and set(lab.values()) == {0}
    s, d = cases["sparse_random"]
    lab = gc.component_oracle(s, d)
    assert len(set(lab.values())) > 500
    assert all(gc.u64_order(l) <= gc.u64_order(v) for v, l in lab.items())
    lab = gc.component_oracle(*cases["star"])
    assert len(lab) == 1000 and set(lab.values()) == {0}
    lab = gc.component_oracle(*cases["two_cliques"])
    assert len(lab) == 80 and set(lab.values()) == {0}
    lab = gc.component_oracle(*cases["negative_keys"])
    # negative keys are the largest u64 patterns: a component of both signs
    # is labelled by its smallest non-negative key
    assert lab[-5] == 3 and lab[-9] == 3
    mixed = [l for v, l in lab.items() if v < 0 and l >= 0]
    assert len(mixed) > 10
    assert gc.rounds_bound(1 << 12) == 28 and gc.rounds_bound(80) == 18
