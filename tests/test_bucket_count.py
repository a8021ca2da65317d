"""bucket_count called directly, and the chunked extract on small tables.

bucket_count: every <512|1024|2048 slots, ILP 1|2|4> instantiation against
a collections.Counter over the ranges that bucket_off describes, on the
layout radix_bucketize really produces and on host-built cases that force
the paths a word-count corpus only meets by luck: LDS-table overflow, a
probe chain past the 64-probe limit, one hot key, pads inside a range,
empty / one-element / offset ranges, the region_stride layout with its
length clamp, accumulation into a table that already holds counts.  Tables
always have at least twice as many slots as distinct keys (ht_add never
gives up on a full table).

hash_extract_v2: forced onto tables from 16 slots up, with and without
exemplars, against the plain extract of the same table and a Counter."""

import collections

import numpy as np
import pytest
import torch

import bucket_common as bc

pytestmark = pytest.mark.gpu

MATRIX = [(s, i) for s in bc.SLOT_SIZES for i in bc.ILPS]
PAIR = [(1024, 1), (512, 4)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mapreduce_amd import ops
    ops.require_gpu_ext()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def env(monkeypatch):
    # the `slots` argument is what runs; small tables extract by v1
    monkeypatch.delenv("MR_BKT_SLOTS", raising=False)
    monkeypatch.delenv("MR_BKT_ILP", raising=False)
    monkeypatch.delenv("MR_EXTRACT_V2_MIN", raising=False)


@pytest.fixture(scope="module")
def layout(dev):
    """Case 1: the raw keys, and what radix_bucketize makes of them."""
    from mapreduce_amd import ops
    raw = bc.raw_layout_keys()
    h = bc.u64_dev(raw, dev)
    p = torch.from_numpy(bc.positions(raw.size)).to(dev)
    hk, pv, off = ops.ext().radix_bucketize(h, p, 56, True)
    return raw, hk, pv, off


# the probe chain has the whole matrix to itself below
HOST_CASES = [c for c in bc.host_cases() if c.name != "probe_chain"]


# ------------------------------------------------------------ the matrix
@pytest.mark.parametrize("exemplar", [True, False])
@pytest.mark.parametrize("slices", [1, 3, 16])
@pytest.mark.parametrize("slots,ilp", MATRIX)
def test_real_layout(dev, layout, monkeypatch, slots, ilp, slices,
                     exemplar):
    from mapreduce_amd import ops
    monkeypatch.setenv("MR_BKT_ILP", str(ilp))
    raw, hk, pv, off = layout
    expect = collections.Counter(raw[raw != bc.EMPTY].tolist())
    assert int(off[256].item()) == sum(expect.values())
    ht = ops.HashTable(len(expect), dev, exemplar=exemplar)
    assert ht.cap >= 2 * len(expect)
    ops.ext().bucket_count(hk, pv, off, 256, slices, ht.tkeys, ht.tvals,
                           ht.texm, 0, slots)
    assert bc.extracted(ht, raw, exemplar) == dict(expect)


@pytest.mark.parametrize("exemplar", [True, False])
@pytest.mark.parametrize("slots,ilp", MATRIX)
def test_lds_overflow(dev, monkeypatch, slots, ilp, exemplar):
    monkeypatch.setenv("MR_BKT_ILP", str(ilp))
    bc.run_case(bc.case_overflow(slots), dev, slots, exemplar)


@pytest.mark.parametrize("exemplar", [True, False])
@pytest.mark.parametrize("slots,ilp", MATRIX)
def test_probe_chain_past_the_limit(dev, monkeypatch, slots, ilp, exemplar):
    monkeypatch.setenv("MR_BKT_ILP", str(ilp))
    bc.run_case(bc.case_probe_chain(), dev, slots, exemplar)


# ------------------------------------------------- the other cases, at 2
@pytest.mark.parametrize("exemplar", [True, False])
@pytest.mark.parametrize("slots,ilp", PAIR)
@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: c.name)
def test_host_built_case(dev, monkeypatch, case, slots, ilp, exemplar):
    monkeypatch.setenv("MR_BKT_ILP", str(ilp))
    bc.run_case(case, dev, slots, exemplar)


@pytest.mark.parametrize("slots,ilp", PAIR)
def test_two_calls_accumulate(dev, monkeypatch, slots, ilp):
    """Disjoint halves counted by two calls equal one oracle over all."""
    from mapreduce_amd import ops
    monkeypatch.setenv("MR_BKT_ILP", str(ilp))
    case = bc.case_pads()
    n = case.hashes.size
    cut = n // 2 + 3
    ht = ops.HashTable(case.capacity, dev, exemplar=True)
    h = bc.u64_dev(case.hashes, dev)
    p = torch.from_numpy(case.pos.copy()).to(dev)
    for a, b in ((0, cut), (cut, n)):
        off = torch.tensor([a, b], dtype=torch.int64, device=dev)
        ops.ext().bucket_count(h, p, off, 1, 3, ht.tkeys, ht.tvals,
                               ht.texm, 0, slots)
    assert bc.extracted(ht, case.hashes, True) == dict(case.expect)


@pytest.mark.parametrize("slots,ilp", PAIR)
def test_adds_to_a_prefilled_table(dev, monkeypatch, slots, ilp):
    """Counts that insert_count put there are added to, not overwritten;
    keys only the pre-fill holds survive."""
    from mapreduce_amd import ops
    monkeypatch.setenv("MR_BKT_ILP", str(ilp))
    case = bc.cases_degenerate()[0]
    rng = np.random.default_rng(8)
    seen = np.array(sorted(case.expect), dtype=np.uint64)
    pre = np.concatenate([seen[rng.integers(0, seen.size, size=400)],
                          bc.distinct_keys(rng, 50)])
    # pre-fill positions continue the case's numbering
    both = np.concatenate([case.hashes, pre])
    pos = bc.positions(both.size)
    expect = case.expect + collections.Counter(pre.tolist())
    ht = ops.HashTable(len(expect), dev, exemplar=True)
    assert ht.cap >= 2 * len(expect)
    h = bc.u64_dev(both, dev)
    p = torch.from_numpy(pos).to(dev)
    ht.insert_count(h[case.hashes.size:], p[case.hashes.size:])
    off = torch.tensor([0, case.hashes.size], dtype=torch.int64, device=dev)
    ops.ext().bucket_count(h, p, off, 1, 2, ht.tkeys, ht.tvals, ht.texm, 0,
                           slots)
    assert bc.extracted(ht, both, True) == dict(expect)


@pytest.mark.parametrize("slots", [0, 256, 777, 4096])
def test_unsupported_slots_fall_back(dev, slots):
    """A slots argument outside {512, 1024, 2048} runs the 2048 form."""
    bc.run_case(bc.case_overflow(512), dev, slots, True)


def test_env_override_of_slots(dev, monkeypatch):
    """MR_BKT_SLOTS wins over the argument (read per call)."""
    monkeypatch.setenv("MR_BKT_SLOTS", "512")
    bc.run_case(bc.case_overflow(512), dev, 2048, True)


def test_mismatched_arguments_are_refused(dev):
    """Checked on the host before any launch."""
    from mapreduce_amd import ops
    e = ops.ext()
    # the guards arrived together with radix_sort_caps: without them the
    # calls below would read out of bounds, so do not make them
    assert hasattr(e, "radix_sort_caps")
    case = bc.cases_degenerate()[0]
    n = case.hashes.size
    h = bc.u64_dev(case.hashes, dev)
    p = torch.from_numpy(case.pos.copy()).to(dev)
    off = torch.tensor([0, n], dtype=torch.int64, device=dev)
    ht = ops.HashTable(case.capacity, dev, exemplar=True)

    def call(h=h, p=p, off=off, nb=1, sl=1, tk=ht.tkeys, tv=ht.tvals,
             tx=ht.texm, stride=0):
        e.bucket_count(h, p, off, nb, sl, tk, tv, tx, stride, 1024)

    bad = [
        dict(p=p[:n - 1]), dict(p=p.to(torch.int32)), dict(p=p.cpu()),
        dict(p=torch.zeros(2 * n, dtype=torch.int64, device=dev)[::2]),
        dict(off=off.cpu()), dict(off=off.to(torch.int32)),
        dict(off=off[:1]), dict(off=off, nb=2),
        dict(nb=0), dict(sl=0), dict(nb=-1), dict(sl=-3),
        dict(h=h.cpu()),
        dict(tv=ht.tvals[:8]), dict(tx=ht.texm[:8]),
        dict(tk=ht.tkeys[:24], tv=ht.tvals[:24], tx=ht.texm[:24]),
        dict(off=torch.tensor([n, n], dtype=torch.int64, device=dev), nb=2,
             stride=n),
    ]
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)
    # nothing above reached the table
    assert bc.extracted(ht, case.hashes, True) == {}
    call()
    assert bc.extracted(ht, case.hashes, True) == dict(case.expect)


# ------------------------------------------------------- chunked extract
def fill_keys(rng, m):
    """m insertions over about m / 2 distinct keys; from 4 up, one is the
    all-ones pattern, which insert_count files under all-ones minus 1."""
    pool = bc.distinct_keys(rng, max(1, m // 2))
    keys = pool[rng.integers(0, pool.size, size=m)]
    keys[:pool.size] = pool  # every pool key at least once
    if m >= 4:
        keys[m // 2] = bc.EMPTY
    return keys


def table_dict(k, v, p):
    keys = k.cpu().numpy().view(np.uint64).tolist()
    assert len(set(keys)) == len(keys)
    pos = p.cpu().tolist() if p.numel() else [None] * len(keys)
    return dict(zip(keys, zip(v.cpu().tolist(), pos)))


@pytest.mark.parametrize("exemplar", [True, False])
@pytest.mark.parametrize("fill", ["empty", "one", "quarter", "dense"])
@pytest.mark.parametrize("capacity", [8, 40, 3000])
def test_chunked_extract_small_tables(dev, monkeypatch, capacity, fill,
                                      exemplar):
    from mapreduce_amd import ops
    ht = ops.HashTable(capacity, dev, exemplar=exemplar)
    distinct = {"empty": 0, "one": 1, "quarter": ht.cap // 4,
                "dense": ht.cap * 45 // 100}[fill]
    rng = np.random.default_rng(capacity * 7 + distinct)
    keys = fill_keys(rng, 2 * distinct) if distinct > 1 else \
        bc.distinct_keys(rng, 1)[:distinct]
    pos = bc.positions(keys.size)
    filed = np.where(keys == bc.EMPTY, bc.EMPTY - np.uint64(1), keys)
    expect = collections.Counter(filed.tolist())
    assert len(expect) <= ht.cap // 2  # never a full table
    if fill in ("quarter", "dense"):
        assert abs(len(expect) - distinct) <= 1
    ht.insert_count(bc.u64_dev(keys, dev),
                    torch.from_numpy(pos).to(dev) if exemplar else None)
    before = (ht.tkeys.clone(), ht.tvals.clone(), ht.texm.clone())

    monkeypatch.setenv("MR_EXTRACT_V2_MIN", "1")
    k2, v2, p2 = ht.extract()
    raw = ops.ext().hash_extract_v2(ht.tkeys, ht.tvals, ht.texm)
    monkeypatch.delenv("MR_EXTRACT_V2_MIN")
    k1, v1, p1 = ht.extract()
    for a, b in zip(before, (ht.tkeys, ht.tvals, ht.texm)):
        assert torch.equal(a, b)  # extraction reads only

    assert k2.dtype == v2.dtype == p2.dtype == torch.int64
    assert not bool((k2 == -1).any())
    if distinct == 0:
        assert k2.numel() == v2.numel() == p2.numel() == 0
    assert p2.numel() == (k2.numel() if exemplar else 0)
    got = table_dict(k2, v2, p2)
    assert got == table_dict(k1, v1, p1)
    assert {k: c for k, (c, _) in got.items()} == dict(expect)
    if exemplar:
        where = collections.defaultdict(set)
        for key, q in zip(filed.tolist(), pos.tolist()):
            where[key].add(q)
        for key, (_, q) in got.items():
            assert q in where[key]

    # the raw kernel output: whole 256-entry chunks, pads only in the key
    # column, every real entry aligned across the three columns
    rk, rv, rp, rc_ = raw
    m = int(rc_.item())
    assert m % 256 == 0 and m <= rk.numel()
    assert rp.numel() == (rk.numel() if exemplar else 0)
    real = rk[:m] != -1
    assert int(real.sum().item()) == len(expect)
    assert table_dict(rk[:m][real], rv[:m][real],
                      rp[:m][real] if exemplar else rp) == got
