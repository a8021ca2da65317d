"""ops.extract_sorted: the native table -> sorted, packed result op against
the composed path on the same table (extract + sort_by_key + extract_words),
itself cross-checked against np.argsort of the u64 keys.  Everything is
compared exactly: keys, counts, pos, lens, offs, the byte total and the
packed buffer.  Sizes sit at the edges of the kernels: the minimum table,
a full table, one bin holding everything up to and past the rank kernel's
LDS capacity, and the offsets-scan tile boundary."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TEXT_LEN = 70000
MAXLEN = 65535


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mapreduce_amd import ops
    ops.require_gpu_ext()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def text(dev):
    rng = np.random.default_rng(99)
    return torch.from_numpy(
        rng.integers(0, 256, size=TEXT_LEN, dtype=np.uint8)).to(dev)


@pytest.fixture(scope="module")
def caps(dev):
    from mapreduce_amd import ops
    return ops.extract_sorted_caps()  # (RANK_M, SCAN_TILE)


# ---------------------------------------------------------------- helpers
def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def uniform_keys(rng, n):
    """n distinct keys; high is exclusive, so never the all-ones pattern."""
    k = np.unique(rng.integers(0, 2 ** 64 - 1, size=n + 64, dtype=np.uint64))
    assert k.size >= n
    return rng.permutation(k)[:n]


def cluster_keys(rng, n, hi32):
    """n distinct keys sharing their top 32 bits."""
    lo = np.unique(rng.integers(0, 1 << 32, size=n + 64, dtype=np.uint64))
    assert lo.size >= n
    return (np.uint64(hi32) << np.uint64(32)) | rng.permutation(lo)[:n]


def rand_pos(rng, n, maxlen=20):
    ln = rng.integers(0, maxlen + 1, size=n).astype(np.uint64)
    off = rng.integers(0, TEXT_LEN - MAXLEN, size=n).astype(np.uint64)
    return (off << np.uint64(16)) | ln


def make_table(dev, capacity, keys, pos, rng, exemplar=True):
    """HashTable holding `keys` once each, exemplar pos[i], count i-varied."""
    from mapreduce_amd import ops
    assert np.unique(keys).size == keys.size
    t = ops.HashTable(capacity, dev, exemplar)
    assert keys.size <= t.cap
    extra = rng.integers(0, 1000, size=keys.size).astype(np.int64)
    if keys.size:
        if exemplar:
            t.insert_count(to_dev(keys, dev), to_dev(pos, dev))
        else:
            t.insert_sum(to_dev(keys, dev), torch.ones(keys.size,
                                                       dtype=torch.int64,
                                                       device=dev))
        t.insert_sum(to_dev(keys, dev), torch.from_numpy(extra).to(dev))
    return t


def oracle(table, text):
    """The existing path on the same table, as host arrays, cross-checked
    against NumPy's argsort of the unsorted extraction."""
    from mapreduce_amd import ops
    k, v, p = table.extract()
    has_pos = p.numel() > 0
    if has_pos:
        sk, sv, sp = ops.sort_by_key(k, v, p)
        lens, blob = ops.extract_words(text, sp)
    elif k.numel():
        sk, sv = ops.sort_by_key(k, v)
        sp = lens = p
        blob = torch.empty(0, dtype=torch.uint8)
    else:
        sk, sv, sp, lens = k, v, p, p
        blob = torch.empty(0, dtype=torch.uint8)
    order = np.argsort(u64(k), kind="stable")
    np.testing.assert_array_equal(u64(sk), u64(k)[order])
    np.testing.assert_array_equal(sv.cpu().numpy(), v.cpu().numpy()[order])
    if has_pos:
        np.testing.assert_array_equal(u64(sp), u64(p)[order])
        np.testing.assert_array_equal(lens.cpu().numpy(),
                                      (u64(sp) & np.uint64(0xFFFF))
                                      .astype(np.int64))
    ln = lens.cpu().numpy()
    offs = np.cumsum(ln) - ln
    total = int(blob.numel())
    if has_pos:
        assert total == int(ln.sum())
    return dict(keys=u64(sk), counts=sv.cpu().numpy(), pos=u64(sp), lens=ln,
                offs=offs, total=total)


def compare(got, exp):
    keys, counts, pos, lens, offs, total, packed = got
    np.testing.assert_array_equal(u64(keys), exp["keys"])
    np.testing.assert_array_equal(counts.cpu().numpy(), exp["counts"])
    np.testing.assert_array_equal(u64(pos), exp["pos"])
    np.testing.assert_array_equal(lens.cpu().numpy(), exp["lens"])
    np.testing.assert_array_equal(offs.cpu().numpy(), exp["offs"])
    assert total == exp["total"]
    assert keys.dtype == counts.dtype == torch.int64
    assert pos.dtype == lens.dtype == offs.dtype == torch.int64
    np.testing.assert_array_equal(
        packed.cpu().numpy(),
        np.concatenate([exp["keys"].view(np.int64), exp["counts"],
                        exp["lens"]]))


def raw_meta(table):
    from mapreduce_amd import ops
    meta = ops.ext().extract_sorted(table.tkeys, table.tvals, table.texm)[3]
    assert not meta.is_cuda
    return [int(x) for x in meta.tolist()]


def check(table, text, overflow=False):
    """Native op == oracle; returns the oracle.  `overflow` states whether
    the raw binding must raise meta[2] for this key set."""
    from mapreduce_amd import ops
    exp = oracle(table, text)
    n, total, over = raw_meta(table)
    assert n == exp["keys"].size
    assert bool(over) == overflow
    if not overflow:
        assert total == exp["total"]
    got = ops.extract_sorted(table)
    compare(got, exp)
    if not overflow:  # the native buffers, not the fallback's
        assert got[0].data_ptr() == got[6].data_ptr()
    return exp


# ------------------------------------------------------------------ sizes
@pytest.mark.parametrize("nkeys", [0, 1, 8, 16])
def test_minimum_table(dev, text, nkeys):
    from mapreduce_amd import ops
    rng = np.random.default_rng(nkeys)
    keys = uniform_keys(rng, nkeys)
    t = make_table(dev, 8, keys, rand_pos(rng, nkeys), rng)
    assert t.cap == 16  # 16 keys: a full table
    exp = check(t, text)
    assert exp["keys"].size == nkeys
    if nkeys == 0:
        out = ops.extract_sorted(t)
        assert all(x.numel() == 0 for x in out[:5]) and out[5] == 0


def test_one_key_large_table(dev, text):
    rng = np.random.default_rng(5)
    keys = uniform_keys(rng, 1)
    check(make_table(dev, 32768, keys, rand_pos(rng, 1), rng), text)


# ------------------------------------------- unsigned, full-width ordering
@pytest.mark.parametrize("capacity", [32, 4096])  # one bin; 128 bins
def test_unsigned_full_width_order(dev, text, capacity):
    rng = np.random.default_rng(11)
    x = np.uint64(0x1234567800000000)
    y = np.uint64(0x00000ABC0000DEF0)
    z = np.uint64(0xF000000000000000)
    keys = np.array(
        [0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 2,
         x | np.uint64(2), x | np.uint64(3),            # differ in bit 0
         z | np.uint64(4), z | np.uint64(5),
         y, y | np.uint64(1 << 32),                     # differ in bit 32
         z | np.uint64(8), z | np.uint64(8) | np.uint64(1 << 32)],
        dtype=np.uint64)
    keys = rng.permutation(keys)
    exp = check(make_table(dev, capacity, keys, rand_pos(rng, keys.size),
                           rng), text)
    assert list(exp["keys"][:2]) == [0, 1]
    assert int(exp["keys"][-1]) == 2 ** 64 - 2
    i = list(exp["keys"]).index(2 ** 63 - 1)
    assert int(exp["keys"][i + 1]) == 2 ** 63


# ------------------------------------------------------------------- bins
@pytest.mark.parametrize("which", ["2", "63", "64", "65", "M", "M+1"])
def test_one_bin_holds_everything(dev, text, caps, which):
    M = caps[0]
    n = {"M": M, "M+1": M + 1}.get(which) or int(which)
    rng = np.random.default_rng(n)
    keys = cluster_keys(rng, n, 0xDEADBEEF)
    t = make_table(dev, M + 88, keys, rand_pos(rng, n), rng)
    assert t.cap >= 2 * (M + 1)
    check(t, text, overflow=(n > M))


def test_two_clusters_in_neighbouring_bins(dev, text, caps):
    M = caps[0]
    rng = np.random.default_rng(21)
    cap_req = 4096  # 2^13 slots -> 128 bins on the top 7 bits
    a = cluster_keys(rng, M - 112, (40 << 25) | 0x123)   # bin 40
    b = cluster_keys(rng, 100, (41 << 25) | 0x456)       # bin 41
    u = uniform_keys(rng, 2000)  # ~16 a bin: both clusters stay under M
    keys = rng.permutation(np.unique(np.concatenate([a, b, u])))
    t = make_table(dev, cap_req, keys, rand_pos(rng, keys.size), rng)
    assert t.cap == 1 << 13
    check(t, text)


def test_overflowing_cluster_among_uniform_keys(dev, text, caps):
    M = caps[0]
    rng = np.random.default_rng(22)
    a = cluster_keys(rng, M + 1, (40 << 25) | 0x123)
    b = cluster_keys(rng, 100, (41 << 25) | 0x456)
    keys = rng.permutation(np.unique(np.concatenate(
        [a, b, uniform_keys(rng, 1000)])))
    t = make_table(dev, 4096, keys, rand_pos(rng, keys.size), rng)
    check(t, text, overflow=True)


# ----------------------------------------------------------- random tables
def _random_cases():
    tile = 2048  # asserted against the extension below
    out = []
    for seed in (1, 2):
        for n in (1000, 5000):
            for capacity in (1 << 12, 1 << 15):   # 2^13 and 2^16 slots
                out.append((n, capacity, seed))
    for n in (tile - 1, tile, tile + 1):
        out.append((n, 1 << 12, 3))
    return out


@pytest.mark.parametrize("n,capacity,seed", _random_cases())
def test_random_tables(dev, text, caps, n, capacity, seed):
    assert caps[1] == 2048
    rng = np.random.default_rng(seed * 7919 + n)
    keys = uniform_keys(rng, n)
    t = make_table(dev, capacity, keys, rand_pos(rng, n), rng)
    assert t.cap == 2 * capacity
    check(t, text)


# ---------------------------------------------------------------- lengths
def test_extreme_lengths(dev, text):
    rng = np.random.default_rng(31)
    n = 300
    keys = uniform_keys(rng, n)
    ln = rng.choice(np.array([0, 1, MAXLEN], dtype=np.uint64), size=n)
    ln[:3] = [0, 1, MAXLEN]
    off = rng.integers(0, TEXT_LEN - MAXLEN, size=n).astype(np.uint64)
    t = make_table(dev, 512, keys, (off << np.uint64(16)) | ln, rng)
    exp = check(t, text)
    assert set(exp["lens"].tolist()) == {0, 1, MAXLEN}


def test_all_max_lengths_across_scan_tiles(dev, text, caps):
    rng = np.random.default_rng(32)
    n = caps[1] + 300  # two tiles of the offsets scan
    keys = uniform_keys(rng, n)
    off = rng.integers(0, TEXT_LEN - MAXLEN, size=n).astype(np.uint64)
    pos = (off << np.uint64(16)) | np.uint64(MAXLEN)
    exp = check(make_table(dev, 4096, keys, pos, rng), text)
    assert exp["total"] == n * MAXLEN
    assert int(exp["offs"][-1]) == (n - 1) * MAXLEN


# ----------------------------------------------------------- no exemplars
@pytest.mark.parametrize("n", [0, 700])
def test_no_exemplars(dev, text, n):
    from mapreduce_amd import ops
    rng = np.random.default_rng(41)
    keys = uniform_keys(rng, n)
    t = make_table(dev, 1024, keys, None, rng, exemplar=False)
    check(t, text)
    keys_o, counts, pos, lens, offs, total, packed = ops.extract_sorted(t)
    assert keys_o.numel() == counts.numel() == n
    assert pos.numel() == lens.numel() == offs.numel() == 0
    assert total == 0 and packed.numel() == 2 * n


# ------------------------------------------------------------ side stream
def test_side_stream(dev, text):
    from mapreduce_amd import ops
    rng = np.random.default_rng(51)
    keys = uniform_keys(rng, 3000)
    t = make_table(dev, 4096, keys, rand_pos(rng, 3000), rng)
    exp = oracle(t, text)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        got = ops.extract_sorted(t)
    s.synchronize()
    compare(got, exp)
    assert got[0].data_ptr() == got[6].data_ptr()


# ------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def corpus(dev):
    from mapreduce_amd.gpu.corpus import make_corpus
    return make_corpus(dev, nwords=6000, nsplits=4, vocab_size=900, seed=17)


def _delivered(res):
    k, c, ln, blob = res.materialize()
    return ([a.numpy().copy() for a in (k, c, ln, blob)], res.to_host(),
            res.nwords)


@pytest.fixture(scope="module")
def composed_result(dev, corpus):
    """The job under MR_EXTRACT_SORTED=0: computed once, never changed."""
    from mapreduce_amd.gpu.wordcount import WordCountJob
    mp = pytest.MonkeyPatch()
    mp.setenv("MR_EXTRACT_SORTED", "0")
    try:
        res = WordCountJob(dev, vocab_estimate=2000).run(corpus.text,
                                                         corpus.splits())
        assert res.keys.data_ptr() != res.packed.data_ptr()
        return _delivered(res)
    finally:
        mp.undo()


def _same(got, exp):
    for a, b in zip(got[0], exp[0]):
        assert a.dtype == b.dtype and a.shape == b.shape
        np.testing.assert_array_equal(a, b)
    assert got[1] == exp[1]
    assert got[2] == exp[2]


def test_wordcount_job_matches_composed(dev, corpus, composed_result,
                                        monkeypatch):
    from mapreduce_amd.gpu.wordcount import WordCountJob
    monkeypatch.delenv("MR_EXTRACT_SORTED", raising=False)
    res = WordCountJob(dev, vocab_estimate=2000).run(corpus.text,
                                                     corpus.splits())
    assert res.keys.data_ptr() == res.packed.data_ptr()  # the native op ran
    assert res.cache_src is res.blob_src
    _same(_delivered(res), composed_result)
    assert len(composed_result[1]) == composed_result[0][0].size > 0


def test_pipelined_wordcount_matches_composed(dev, corpus, composed_result,
                                              monkeypatch):
    from mapreduce_amd.gpu.pipeline import PipelinedWordCount
    monkeypatch.delenv("MR_EXTRACT_SORTED", raising=False)
    pipe = PipelinedWordCount(dev, vocab_estimate=2000, use_runner=False)
    splits = corpus.splits()
    for _ in range(3):
        res = pipe.step(corpus.text, splits)
        _same(_delivered(res), composed_result)
    pipe.flush()
