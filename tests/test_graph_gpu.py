"""ops.graph_propagate and ops.pagerank_update on the device, GraphJob,
Graph.pagerank and Graph.components above them, and the Server routing of
examples/pagerank.  The i64 and dyadic-f64 comparisons are exact on bit
patterns against the oracle of graph_common; the general f64 sum is held to
the bound test_window_gpu derives (deg * 2^-52 * sum |v| per row against
math.fsum).  Sizes come from the extension (ops.graph_caps): E edges per
tile."""

import math

import numpy as np
import pytest
import torch

import graph_common as gc
from mapreduce_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PE = ops.GRAPH_TILE
CASES = gc.kernel_cases(PE)
BIG = 2 ** 63 - 1


@pytest.fixture(scope="module")
def caps():
    return ops.graph_caps()


def test_caps_come_from_the_extension(caps):
    assert caps == tuple(ops.ext().graph_caps()) == (PE, ops.GRAPH_PR_BLOCKS)
    assert caps[0] == 256 * 8


def bait(a, below, above):
    """-> (buffer, view): the numpy array as the exact-size inner slice of a
    device tensor two entries longer, so the view sits one entry (8 bytes,
    or 4 for src) off the buffer's 16-byte alignment."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.empty(t.numel() + 2, dtype=t.dtype)
    buf[1:-1] = t
    raw = buf.view(torch.int64 if t.element_size() == 8 else torch.int32)
    raw[0], raw[-1] = below, above
    buf = buf.to(DEV)
    assert buf.data_ptr() % 16 == 0
    assert not t.numel() or buf[1:-1].data_ptr() % 16 != 0
    return buf, buf[1:-1]


class Staged:
    """A case on the device behind baits: an out-of-range read of src gives
    a valid node, of x a huge value, of offsets a wrong row end, and each
    changes an answer."""

    def __init__(self, off, src, x):
        n = len(off) - 1
        self.bufs = []
        self.off = self._put(off, 12345, 0)
        self.src = self._put(src, max(n - 1, 0), max(n // 2, 0))
        self.x = self._put(x, BIG - 7, BIG - 11)

    def _put(self, a, below, above):
        buf, view = bait(a, below, above)
        self.bufs.append((buf, buf.clone()))
        return view

    def run(self, op):
        out = ops.graph_propagate(self.off, self.src, self.x, op)
        assert out.numel() == self.x.numel() and out.dtype == self.x.dtype
        return out

    def unchanged(self):
        return all(torch.equal(b.view(torch.int32), c.view(torch.int32))
                   for b, c in self.bufs)


def bits(t):
    return t.view(torch.int64).cpu().tolist()


def f64_bits(vals):
    return np.array(vals, dtype=np.float64).view(np.int64).tolist()


# ------------------------------------------------------------------ kernel

# parametrised by name over the Python constant; the first assertion checks
# it is the extension's, so the ids name the cases the device runs
@pytest.mark.parametrize("name", sorted(CASES))
def test_i64_sum_min_max_are_exact(name, caps, monkeypatch):
    assert caps[0] == PE
    off, src = CASES[name]
    x = gc.values_i64(len(off) - 1)
    st = Staged(off, src, x)
    got = {}
    for op in ("sum", "min", "max"):
        got[op] = st.run(op)
        assert got[op].cpu().tolist() == gc.propagate_oracle(off, src, x, op)
    # the composition from the project's other ops agrees bit for bit
    monkeypatch.setenv("MR_GRAPH_COMPOSED", "1")
    for op in ("sum", "min", "max"):
        assert torch.equal(st.run(op), got[op])
    assert st.unchanged()


@pytest.mark.parametrize("name", sorted(CASES))
def test_dyadic_f64_sums_are_exact_on_bits(name):
    off, src = CASES[name]
    x = gc.values_dyadic(len(off) - 1, 5)
    st = Staged(off, src, x)
    assert bits(st.run("sum")) == f64_bits(
        gc.propagate_oracle(off, src, x, "sum"))
    assert st.unchanged()


@pytest.mark.parametrize("name", sorted(CASES))
def test_general_f64_sum_within_the_derived_bound(name):
    off, src = CASES[name]
    x = gc.values_general(len(off) - 1, 6)
    st = Staged(off, src, x)
    got = st.run("sum").cpu().tolist()
    exp = gc.propagate_oracle(off, src, x, "sum")
    worst = 0.0
    for g, e, (deg, tot) in zip(got, exp, gc.row_abs_sums(off, src, x)):
        bound = deg * 2.0 ** -52 * tot
        assert abs(g - e) <= bound, (g, e, deg, tot)
        if bound:
            worst = max(worst, abs(g - e) / bound)
    print(f"{name}: worst |err| / bound = {worst:.4f}")
    assert st.unchanged()


@pytest.mark.parametrize("name", ["mixed", "hub_mid"])
def test_two_calls_return_identical_bits(name):
    off, src = CASES[name]
    st = Staged(off, src, gc.values_general(len(off) - 1, 6))
    assert torch.equal(st.run("sum").view(torch.int64),
                       st.run("sum").view(torch.int64))


@pytest.mark.parametrize("name", ["mixed", "hub_mid", "empties"])
def test_inf_and_nan_reach_exactly_the_rows_they_feed(name):
    off, src = CASES[name]
    n = len(off) - 1
    x = gc.values_general(n, 6)
    clean = Staged(off, src, x).run("sum")
    a, b = int(src[len(src) // 3]), int(src[len(src) // 2])
    assert a != b
    x[a], x[b] = math.inf, math.nan
    got = Staged(off, src, x).run("sum").cpu()
    has_a = np.zeros(n, dtype=bool)
    has_b = np.zeros(n, dtype=bool)
    rows = np.repeat(np.arange(n), np.diff(off))
    has_a[rows[src == a]] = True
    has_b[rows[src == b]] = True
    assert has_a.any() and has_b.any() and not (has_a | has_b).all()
    g = got.numpy()
    assert np.isnan(g[has_b]).all()
    assert (g[has_a & ~has_b] == math.inf).all()
    # x does not influence the association: the other rows keep their bits
    rest = torch.from_numpy(~(has_a | has_b))
    assert torch.equal(got.view(torch.int64)[rest],
                       clean.cpu().view(torch.int64)[rest])


def test_src_outside_the_nodes_contributes_the_identity():
    off, src = CASES["mixed"]
    n = len(off) - 1
    src = src.copy()
    src[::7] = -1
    src[3::11] = n
    src[5::13] = 2 ** 31 - 1
    src[-1] = -2 ** 31
    # a row of nothing but bad edges
    v = int(np.argmax(np.diff(off) == 2))
    src[off[v]:off[v + 1]] = n
    xi = gc.values_i64(n)
    st = Staged(off, src, xi)
    for op in ("sum", "min", "max"):
        exp = gc.propagate_oracle(off, src, xi, op)
        assert exp[v] == gc.IDENT[op]
        assert st.run(op).cpu().tolist() == exp
    xd = gc.values_dyadic(n, 5)
    assert bits(Staged(off, src, xd).run("sum")) == f64_bits(
        gc.propagate_oracle(off, src, xd, "sum"))
    assert st.unchanged()


def test_offsets_that_break_the_contract_give_a_defined_answer():
    """Offsets are only ever compared with edge numbers, never used as an
    index, so garbage in them cannot address anything: the call returns n
    values and leaves the inputs alone."""
    off, src = CASES["mixed"]
    n, m = len(off) - 1, len(src)
    rng = np.random.default_rng(9)
    xi = gc.values_i64(n)
    for bad in (off[::-1].copy(), rng.integers(-5, m + 5, size=n + 1),
                np.full(n + 1, m, dtype=np.int64),
                np.full(n + 1, -1, dtype=np.int64), off + 3):
        st = Staged(bad.astype(np.int64), src, xi)
        for op in ("sum", "min"):
            assert st.run(op).numel() == n
        torch.cuda.synchronize()
        assert st.unchanged()


def test_refusals_raise_with_their_messages():
    off, src = CASES["m65"]
    n = len(off) - 1
    o = torch.from_numpy(off).to(DEV)
    s = torch.from_numpy(src).to(DEV)
    xf = torch.from_numpy(gc.values_dyadic(n, 1)).to(DEV)
    xi = torch.from_numpy(gc.values_i64(n)).to(DEV)
    with pytest.raises(TypeError, match="src must be int32"):
        ops.graph_propagate(o, s.to(torch.int64), xi)
    with pytest.raises(TypeError, match="graph min needs int64 values"):
        ops.graph_propagate(o, s, xf, "min")
    with pytest.raises(TypeError, match="graph max needs int64 values"):
        ops.graph_propagate(o, s, xf, "max")
    with pytest.raises(ValueError, match=f"offsets must hold {n + 1} entries"):
        ops.graph_propagate(o[:-1], s, xi)
    with pytest.raises(RuntimeError, match="src must be on GPU"):
        ops.graph_propagate(o, s.cpu(), xi)
    with pytest.raises(RuntimeError, match="x must be on GPU"):
        ops.graph_propagate(o, s, xi.cpu())
    # the binding's own checks
    e = ops.ext()
    with pytest.raises(RuntimeError, match="src must be int32"):
        e.graph_propagate(o, s.to(torch.int64), xi, 0, False)
    with pytest.raises(RuntimeError, match="offsets must hold"):
        e.graph_propagate(o[:-1], s, xi, 0, False)
    with pytest.raises(RuntimeError, match="graph min / max take int64"):
        e.graph_propagate(o, s, xf.view(torch.int64), 1, True)
    with pytest.raises(RuntimeError, match="op must be 0"):
        e.graph_propagate(o, s, xi, 3, False)
    with pytest.raises(RuntimeError, match="old must hold"):
        e.pagerank_update(xf, xf[:-1], xf, 0.85, xf[:1])
    with pytest.raises(RuntimeError, match="inv_out must be float64"):
        e.pagerank_update(xf, xf, xi, 0.85, xf[:1])


@pytest.mark.parametrize("n", [1, 255, 257, 256 * ops.GRAPH_PR_BLOCKS + 77])
def test_pagerank_update_matches_the_formula(n, caps):
    rng = np.random.default_rng(n)
    sums = rng.random(n) / n
    old = rng.random(n) / n
    outdeg = rng.integers(0, 4, size=n)
    inv = np.where(outdeg > 0, 1.0 / np.maximum(outdeg, 1), 0.0)
    dang, d = 0.37, 0.85
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    new, contrib, partials = ops.pagerank_update(
        t(sums), t(old), t(inv), d, torch.tensor(dang, dtype=torch.float64,
                                                 device=DEV))
    assert partials.shape == (min((n + 255) // 256, caps[1]), 2)
    exp = (1.0 - d) / n + d * (sums + dang / n)
    # one rounding per operation, or one fewer where the compiler fuses
    assert np.abs(new.cpu().numpy() - exp).max() <= 4 * 2.0 ** -53 * exp.max()
    assert torch.equal(contrib, new * t(inv))
    p = partials.sum(0).cpu().tolist()
    got = new.cpu().numpy()
    delta = math.fsum(np.abs(got - old).tolist())
    held = math.fsum(got[outdeg == 0].tolist())
    # sums of n non-negative terms in a fixed tree
    assert abs(p[0] - delta) <= n * 2.0 ** -53 * delta
    assert abs(p[1] - held) <= n * 2.0 ** -53 * held + 0.0
    again = ops.pagerank_update(
        t(sums), t(old), t(inv), d, torch.tensor(dang, dtype=torch.float64,
                                                 device=DEV))
    assert all(torch.equal(a, b) for a, b in zip(
        (new, contrib, partials), again))


# --------------------------------------------------------------- job level

SRC, DST = gc.multigraph(11, 300, 3000)
COMPONENTS = gc.component_cases()


def test_pagerank_matches_the_oracle_within_the_derived_bound():
    gc.check_pagerank(DEV, SRC, DST)


def test_pagerank_over_several_tiles_of_edges():
    s, d = gc.multigraph(12, 700, 3 * PE + 17)
    g, _ = gc.check_pagerank(DEV, s, d)
    assert g.m == 3 * PE + 17 and g.src.is_cuda


def test_pagerank_stops_at_the_oracles_iteration():
    gc.check_early_stop(DEV, SRC, DST)


def test_more_continues_bit_for_bit():
    gc.check_more(DEV, SRC, DST)


@pytest.mark.parametrize("name", sorted(COMPONENTS))
def test_components_match_union_find(name):
    gc.check_components(DEV, *COMPONENTS[name])


# ---------------------------------------------------------- Server routing

def test_pagerank_example_routes_onto_the_device(monkeypatch):
    import test_graph_cpu as tc

    args = {"seed": 3, "n": 60, "m": 400, "splits": 3, "parts": 4}
    pg, srv = tc.run_example_gpu_tier(monkeypatch, "auto", args)
    edges = pg.make_edges(3, 60, 400)
    tc.check_example_result(pg, dict(pg.RESULTS), edges)
    assert pg._STATE["rounds"] == 2
    assert list(pg.RESULTS) == sorted(pg.RESULTS)


def test_components_task_routes_onto_the_device(monkeypatch):
    import test_graph_cpu as tc

    monkeypatch.setattr(
        tc, "_server", lambda mp, **over: _auto_server(mp, tc, **over))
    tc.test_components_task_given_as_a_dict_of_functions(monkeypatch)


def _auto_server(monkeypatch, tc, **over):
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.setenv("MR_GPU_TIER", "auto")
    return Server(coord=LocalCoordinator()).configure(
        {"fns": tc._toy_fns(**over), "verbose": False})
