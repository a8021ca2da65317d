"""The tokenizer's multi-tile loop, on both of its bodies.

With the launchers' own grids a small text gets one block per 4 KB tile, so
the loop in which a block walks from tile to tile (the part tokenize_v7
re-schedules: next tile prefetched into registers while the current one is
hashed and probed) is only reached at sizes no quick test can afford.  The
bindings' trailing `max_blocks` caps the grid instead: with 1, 2 or 3 blocks
a block owns an odd or even number of consecutive tiles, a partial last
tile, or a last tile whose bytes lie only in what was its predecessor's
halo.

Every case is checked against the Python split oracle: table counts plus
spilled records (pads skipped) must add up to Counter(text.split()) keyed
by wordhash64, and every record must point at a complete word whose hash is
its key.  The cases run here on the default body and once more, all of
them, in one child process with MR_TOKENIZE_V6=1; the spill-all and
composite launches, whose records do not depend on any race, must also give
the same multiset of (key, pos) under both.  The cached cases run a third
time in a child with MR_TOK_GPOS=0 (exemplar positions in LDS, another
instantiation).  After every launch the extension is asked which body the
launcher dispatched."""

import collections
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tokenizer_multitile_common as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "MR_TOKENIZE_V6"
DOC_BASE = 3


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mapreduce_amd import ops
    ops.require_gpu_ext()
    return torch.device("cuda:0")


# ----------------------------------------------------------------- runners
def to_dev(data: bytes, dev):
    import torch
    if not data:
        return torch.empty(0, dtype=torch.uint8, device=dev)
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)


def u64_list(t):
    return t.cpu().numpy().view(np.uint64).tolist()


def launched(ops, t):
    """The launcher's own record of the body it just dispatched (an empty
    text dispatches nothing)."""
    if t.numel() == 0:
        return
    want = "v6" if os.environ.get(SWITCH) == "1" else "v7"
    assert ops.ext().tokenizer_last_body() == want


def spill_cap(nbytes: int, blocks: int, chunk: int) -> int:
    """Room for every word (at most nbytes / 2 of them), for the pads of
    retired chunks (a wave pads less than the window total that made it
    grab the next chunk, so fewer pads than records) and for one stranded
    chunk per wave of the grid."""
    grid = blocks if blocks else -(-nbytes // tc.TILE) + 1
    return nbytes + 16 + grid * 4 * chunk


def run_cached(dev, text: bytes, start: int, max_blocks: int):
    """tokenize_cache_spill over text[start:] -> (record keys, record pos,
    table keys, table counts, table pos, nwords)."""
    import torch
    from mapreduce_amd import ops
    t = to_dev(text, dev)[start:]
    assert t.data_ptr() % 16 == start % 16 or t.numel() == 0
    table = ops.make_table(1 << 14, dev)
    cap = spill_cap(len(text), max_blocks, 2048)
    opts = dict(dtype=torch.int64, device=dev)
    sh, sp = torch.empty(cap, **opts), torch.empty(cap, **opts)
    sc, nw = torch.zeros(1, **opts), torch.zeros(1, **opts)
    ops.ext().tokenize_cache_spill(t, start, table.tkeys, table.tvals,
                                   table.texm, cap, nw, sh, sp, sc,
                                   max_blocks)
    launched(ops, t)
    n = int(sc.item())
    assert n <= cap
    tk, tv, tp = table.extract()
    return (u64_list(sh[:n]), u64_list(sp[:n]), u64_list(tk),
            tv.cpu().tolist(), u64_list(tp), int(nw.item()))


def run_spill_all(dev, text: bytes, start: int, max_blocks: int):
    from mapreduce_amd import ops
    t = to_dev(text, dev)[start:]
    cap = spill_cap(len(text), max_blocks, 512)
    k, p, c, nw = ops.ext().tokenize_spill_v2(t, start, cap, max_blocks)
    launched(ops, t)
    n = int(c.item())
    assert n <= cap
    return u64_list(k[:n]), u64_list(p[:n]), int(nw.item())


def split_offsets(n: int):
    """Three documents; the cuts fall inside tiles, not on their edges."""
    return [0, n // 3 + 7, 2 * n // 3 + 11]


def run_composite(dev, text: bytes, max_blocks: int):
    """The inverted index's tokenizer entry point (spill-all, composite)."""
    import torch
    from mapreduce_amd import ops
    t = to_dev(text, dev)
    so = torch.tensor(split_offsets(len(text)), dtype=torch.int64, device=dev)
    cap = spill_cap(len(text), max_blocks, 512)
    k, p, c, nw = ops.ext().tokenize_spill_composite(t, 0, cap, so, DOC_BASE,
                                                     max_blocks)
    launched(ops, t)
    n = int(c.item())
    assert n <= cap
    return u64_list(k[:n]), u64_list(p[:n]), int(nw.item())


def run_cached_composite(dev, text: bytes, max_blocks: int):
    """tokenize_cache_spill_composite (the inverted index's cached path)."""
    import torch
    from mapreduce_amd import ops
    t = to_dev(text, dev)
    so = torch.tensor(split_offsets(len(text)), dtype=torch.int64, device=dev)
    table = ops.make_table(1 << 15, dev)
    cap = spill_cap(len(text), max_blocks, 2048)
    opts = dict(dtype=torch.int64, device=dev)
    sh, sp = torch.empty(cap, **opts), torch.empty(cap, **opts)
    sc, nw = torch.zeros(1, **opts), torch.zeros(1, **opts)
    ops.ext().tokenize_cache_spill_composite(
        t, 0, table.tkeys, table.tvals, table.texm, cap, nw, sh, sp, sc, so,
        DOC_BASE, max_blocks)
    launched(ops, t)
    n = int(sc.item())
    assert n <= cap
    tk, tv, tp = table.extract()
    return (u64_list(sh[:n]), u64_list(sp[:n]), u64_list(tk),
            tv.cpu().tolist(), u64_list(tp), int(nw.item()))


# ------------------------------------------------------------------ checks
def check_cached(dev, text: bytes, start: int, max_blocks: int, oracle):
    rk, rp, tk, tv, tp, nw = run_cached(dev, text, start, max_blocks)
    spilled, where = tc.check_records(text, rk, rp)
    tabled, twhere = tc.check_records(text, tk, tp, weights=tv)
    assert spilled + tabled == oracle, (len(text), start, max_blocks)
    assert nw == sum(oracle.values())
    return sum(spilled.values()), where | twhere


def check_spill_all(dev, text: bytes, start: int, max_blocks: int, oracle,
                    expect=()):
    rk, rp, nw = run_spill_all(dev, text, start, max_blocks)
    spilled, where = tc.check_records(text, rk, rp)
    assert spilled == oracle, (len(text), start, max_blocks)
    assert nw == sum(oracle.values())
    missing = [(o, w) for o, w in expect
               if o >= start and (o, len(w)) not in where]
    assert not missing, missing
    return tc.digest(rk, rp)


def check_composite(dev, text: bytes, max_blocks: int):
    so = split_offsets(len(text))

    def keyfn(w, off):
        return tc.composite_key(w, tc.doc_of(off, so) + DOC_BASE)

    rk, rp, nw = run_composite(dev, text, max_blocks)
    got, where = tc.check_records(text, rk, rp, keyfn=keyfn)
    words = collections.Counter(text.split())
    assert sum(got.values()) == nw == sum(words.values())
    starts = [o for o, _ in where]
    assert len(starts) == len(set(starts)) == nw  # each word exactly once
    return tc.digest(rk, rp)


def check_cached_composite(dev, text: bytes, max_blocks: int):
    if not text:
        return  # the launcher returns before it touches anything
    so = split_offsets(len(text))

    def keyfn(w, off):
        return tc.composite_key(w, tc.doc_of(off, so) + DOC_BASE)

    rk, rp, tk, tv, tp, nw = run_cached_composite(dev, text, max_blocks)
    spilled, _ = tc.check_records(text, rk, rp, keyfn=keyfn)
    tabled, _ = tc.check_records(text, tk, tp, weights=tv, keyfn=keyfn)
    oracle = tc.composite_oracle(text, so, DOC_BASE)
    assert spilled + tabled == oracle, (len(text), max_blocks)
    assert nw == sum(oracle.values())


def case_tile_walk(dev, n: int):
    text, expect = tc.walk_text(n)
    oracle = tc.key_oracle(text)
    out = {}
    for mb in tc.WALK_BLOCKS:
        check_cached(dev, text, 0, mb, oracle)
        out[f"all/{n}/{mb}"] = check_spill_all(dev, text, 0, mb, oracle,
                                               expect)
        out[f"comp/{n}/{mb}"] = check_composite(dev, text, mb)
        check_cached_composite(dev, text, mb)
    return out


def case_unaligned(dev, s: int):
    text, expect = tc.unaligned_text()
    oracle = tc.key_oracle(text[s:])
    _, where = check_cached(dev, text, s, 1, oracle)
    assert min(o for o, _ in where) == s  # offsets index the whole buffer
    return {f"all/unaligned/{s}": check_spill_all(dev, text, s, 1, oracle,
                                                  expect)}


def case_same_key(dev, name: str):
    text = tc.same_key_texts()[name]
    oracle = tc.key_oracle(text)
    out = {}
    for mb in (1, 2, 0):
        check_cached(dev, text, 0, mb, oracle)
        out[f"all/{name}/{mb}"] = check_spill_all(dev, text, 0, mb, oracle)
        out[f"comp/{name}/{mb}"] = check_composite(dev, text, mb)
        check_cached_composite(dev, text, mb)
    return out


def case_saturation(dev):
    text = tc.saturation_text()
    oracle = tc.key_oracle(text)
    assert len(oracle) > tc.CACHE_SLOTS
    nspilled, _ = check_cached(dev, text, 0, 1, oracle)
    assert nspilled > 0, "one block's cache cannot hold this vocabulary"
    check_cached_composite(dev, text, 1)
    return {}


def tokenizer_body() -> str:
    from mapreduce_amd import ops
    return str(ops.ext().tokenizer_occupancy()["body"])


# ------------------------------------------------------------------- tests
DIGESTS = {}  # what the default body gave, for test_previous_body_agrees


@pytest.mark.parametrize("n", tc.WALK_SIZES)
def test_tile_walk(dev, n):
    DIGESTS.update(case_tile_walk(dev, n))


@pytest.mark.parametrize("s", tc.UNALIGNED_STARTS)
def test_unaligned_base(dev, s):
    DIGESTS.update(case_unaligned(dev, s))


@pytest.mark.parametrize("name", sorted(tc.same_key_texts()))
def test_same_key_many_times(dev, name):
    DIGESTS.update(case_same_key(dev, name))


def test_cache_saturation_in_one_block(dev):
    case_saturation(dev)


def test_default_body_is_v7(dev):
    """What the launchers dispatched, not only what the switch says."""
    from mapreduce_amd import ops
    assert tokenizer_body() == "v7"
    text, _ = tc.walk_text(4097)
    for run in (lambda: run_cached(dev, text, 0, 1),
                lambda: run_spill_all(dev, text, 0, 1),
                lambda: run_composite(dev, text, 1),
                lambda: run_cached_composite(dev, text, 1)):
        run()
        assert ops.ext().tokenizer_last_body() == "v7"


def run_everything(dev):
    out = {}
    for n in tc.WALK_SIZES:
        out.update(case_tile_walk(dev, n))
    for s in tc.UNALIGNED_STARTS:
        out.update(case_unaligned(dev, s))
    for name in sorted(tc.same_key_texts()):
        out.update(case_same_key(dev, name))
    case_saturation(dev)
    return out


def child_main():
    """Body of the variant child: every case above, then one JSON line."""
    import torch
    from mapreduce_amd import ops
    ops.require_gpu_ext()
    out = run_everything(torch.device("cuda:0"))
    assert tokenizer_body() == ops.ext().tokenizer_last_body()
    print(json.dumps({"body": ops.ext().tokenizer_last_body(),
                      "digests": out}))


def child_cached_main():
    """Body of the MR_TOK_GPOS=0 child: every cached word-count case."""
    import torch
    from mapreduce_amd import ops
    ops.require_gpu_ext()
    dev = torch.device("cuda:0")
    calls = 0
    for n in tc.WALK_SIZES:
        text, _ = tc.walk_text(n)
        for mb in tc.WALK_BLOCKS:
            check_cached(dev, text, 0, mb, tc.key_oracle(text))
            calls += 1
    text, _ = tc.unaligned_text()
    for s in tc.UNALIGNED_STARTS:
        check_cached(dev, text, s, 1, tc.key_oracle(text[s:]))
        calls += 1
    for name, text in sorted(tc.same_key_texts().items()):
        for mb in (1, 2, 0):
            check_cached(dev, text, 0, mb, tc.key_oracle(text))
            calls += 1
    text = tc.saturation_text()
    nspilled, _ = check_cached(dev, text, 0, 1, tc.key_oracle(text))
    assert nspilled > 0
    calls += 1
    print(json.dumps({"body": ops.ext().tokenizer_last_body(),
                      "calls": calls}))


CHILD = ("import sys; sys.path[:0] = [{root!r}, {tests!r}]; "
         "import test_tokenizer_multitile as t; t.{main}()")
EXPECTED_CACHED_CALLS = (len(tc.WALK_SIZES) * len(tc.WALK_BLOCKS)
                         + len(tc.UNALIGNED_STARTS)
                         + 3 * len(tc.same_key_texts()) + 1)


def run_child(main: str, **extra):
    env = dict(os.environ)
    for name in (SWITCH, "MR_TOK_GPOS"):
        env.pop(name, None)
    env.update(extra)
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"),
                        main=main)
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_lds_exemplar_instantiation(dev):
    """MR_TOK_GPOS=0: the cached cases on tokenize_v7_kernel<2048, false>,
    which keeps exemplar positions in LDS (45 KB, 3 blocks per CU)."""
    r = run_child("child_cached_main", MR_TOK_GPOS="0")
    assert r["body"] == "v7"
    assert r["calls"] == EXPECTED_CACHED_CALLS > 0


def test_previous_body_agrees(dev):
    """MR_TOKENIZE_V6=1: every case on the v6 body, and the same (key, pos)
    multisets from the spill-all and composite launches as the default."""
    mine = dict(DIGESTS)
    if len(mine) < EXPECTED_DIGESTS:  # run alone: compute them here
        mine = run_everything(dev)
    r = run_child("child_main", **{SWITCH: "1"})
    assert r["body"] == "v6"
    assert len(r["digests"]) == EXPECTED_DIGESTS == len(mine)
    assert r["digests"] == mine


EXPECTED_DIGESTS = (2 * len(tc.WALK_SIZES) * len(tc.WALK_BLOCKS)
                    + len(tc.UNALIGNED_STARTS)
                    + 2 * 3 * len(tc.same_key_texts()))
