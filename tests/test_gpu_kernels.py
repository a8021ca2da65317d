"""Numerics tests for the CDNA4 HIP kernels vs plain CPU references.

Every kernel is compared against a NumPy/PyTorch CPU oracle on random data
(guide rule: asymmetric, non-trivial inputs)."""

import collections

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mapreduce_amd import ops
    ops.require_gpu_ext()
    return torch.device("cuda:0")


def u64view(t_i64_cpu):
    return t_i64_cpu.numpy().view(np.uint64)


TEXT = (b"the quick brown fox jumps over the lazy dog\n"
        b"pack my box  with five dozen liquor jugs\t\n"
        b"the the the end x yz  multi   spaces\r\n" * 50)


def py_tokenize(data: bytes):
    from mapreduce_amd.utils.tuple import fnv1a64
    words = data.split()
    return [fnv1a64(w) for w in words], words


def test_tokenize_matches_python_split(dev):
    from mapreduce_amd import ops
    text = torch.frombuffer(bytearray(TEXT), dtype=torch.uint8).to(dev)
    h, p, n = ops.tokenize_words(text)
    exp_hashes, exp_words = py_tokenize(TEXT)
    assert n == len(exp_words)
    got = sorted(u64view(h.cpu()).tolist())
    assert got == sorted(exp_hashes)


def test_tokenize_edge_cases(dev):
    from mapreduce_amd import ops
    for data in (b"", b"   ", b"a", b" a", b"a ", b"ab\ncd", b"\t\n x \r\n",
                 b"x" * 70000):
        text = torch.frombuffer(bytearray(data or b"\x20"),
                                dtype=torch.uint8).to(dev)
        if data == b"":
            text = text[:0]
        h, p, n = ops.tokenize_words(text)
        exp_hashes, exp_words = py_tokenize(data)
        assert n == len(exp_words), data
        assert sorted(u64view(h.cpu()).tolist()) == sorted(exp_hashes), data


def test_hash_table_count_vs_counter(dev):
    from mapreduce_amd import ops
    rng = np.random.default_rng(42)
    # zipf-ish duplicates
    keys_np = rng.integers(0, 5000, size=200_000, dtype=np.uint64) ** 3 + 7
    keys = torch.from_numpy(keys_np.view(np.int64)).to(dev)
    ht = ops.HashTable(20_000, dev, exemplar=False)
    ht.insert_count(keys, None)
    uk, uv, _ = ht.extract()
    got = dict(zip(u64view(uk.cpu()).tolist(), uv.cpu().tolist()))
    exp = collections.Counter(keys_np.tolist())
    assert got == dict(exp)


def test_hash_table_sum_vs_numpy(dev):
    from mapreduce_amd import ops
    rng = np.random.default_rng(1)
    keys_np = rng.integers(0, 1000, size=50_000, dtype=np.uint64) * 2654435761
    vals_np = rng.integers(-100, 100, size=50_000, dtype=np.int64)
    keys = torch.from_numpy(keys_np.view(np.int64)).to(dev)
    vals = torch.from_numpy(vals_np).to(dev)
    ht = ops.HashTable(2000, dev, exemplar=False)
    ht.insert_sum(keys, vals)
    uk, uv, _ = ht.extract()
    got = dict(zip(u64view(uk.cpu()).tolist(), uv.cpu().tolist()))
    exp = {}
    for k, v in zip(keys_np.tolist(), vals_np.tolist()):
        exp[k] = exp.get(k, 0) + v
    assert got == exp


def test_hash_table_big_capacity_chunked_extract(dev):
    """Tables >= 2^22 slots use the chunked-compaction extract (HT_EMPTY
    padding masked in the wrapper) — verify exact contents at scale."""
    from mapreduce_amd import ops
    n = 3_000_000
    base = torch.arange(n, dtype=torch.int64, device=dev) * 2654435761
    keys = torch.cat([base, base])  # every key exactly twice
    ht = ops.HashTable(n, dev, exemplar=False)
    assert ht.cap >= (1 << 22)
    ht.insert_sum(keys, torch.ones_like(keys))
    uk, uv, _ = ht.extract()
    assert uk.numel() == n
    assert bool((uv == 2).all())
    sk, sv = ops.sort_pairs(uk, uv)
    exp = np.sort(base.cpu().numpy().view(np.uint64))
    assert np.array_equal(sk.cpu().numpy().view(np.uint64), exp)


def _small_sort_n():
    import os
    from mapreduce_amd import ops
    return int(os.environ.get("MR_SMALL_SORT_N", ops._SMALL_SORT_N))


def _empty(dev):
    return torch.empty(0, dtype=torch.int64, device=dev)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 2048, 2049, 1_000_000,
                               (1 << 20) + 1])
def test_radix_sort_keys(dev, n):
    """First half: ops.sort_by_key, which below the small-sort threshold
    (2^20 keys; every size here but the last) is one stable torch.sort
    (rocPRIM) and from it up the in-tree radix sort.  Second half: the same
    input through radix_sort_pairs itself, whatever the size."""
    from mapreduce_amd import ops
    rng = np.random.default_rng(n + 1)
    keys_np = rng.integers(0, 2 ** 63 - 1, size=n, dtype=np.uint64)
    keys_np |= rng.integers(0, 2, size=n, dtype=np.uint64) << 63  # top bit too
    keys = torch.from_numpy(keys_np.view(np.int64)).to(dev)
    (sk,) = ops.sort_by_key(keys)
    got = u64view(sk.cpu())
    assert np.array_equal(got, np.sort(keys_np))
    rk, _ = ops.ext().radix_sort_pairs(keys, _empty(dev), 64)
    assert np.array_equal(u64view(rk.cpu()), np.sort(keys_np))
    assert np.array_equal(u64view(keys.cpu()), keys_np)  # input untouched


def test_radix_sort_pairs_stable(dev):
    """Above the small-sort threshold, so ops.sort_pairs runs the in-tree
    radix sort (first half); the second half calls radix_sort_pairs and
    radix_sort_idx32 directly.  The torch path of the wrapper is compared
    with the same oracle in test_radix_full_sort.py."""
    from mapreduce_amd import ops
    rng = np.random.default_rng(3)
    n = (1 << 20) + 4099
    assert n >= _small_sort_n()
    keys_np = rng.integers(0, 64, size=n, dtype=np.uint64)  # heavy dupes
    vals_np = np.arange(n, dtype=np.uint64)
    keys = torch.from_numpy(keys_np.view(np.int64)).to(dev)
    vals = torch.from_numpy(vals_np.view(np.int64)).to(dev)
    sk, sv = ops.sort_pairs(keys, vals)
    got_k = u64view(sk.cpu())
    got_v = u64view(sv.cpu())
    order = np.argsort(keys_np, kind="stable")
    assert np.array_equal(got_k, keys_np[order])
    assert np.array_equal(got_v, vals_np[order])  # stability
    rk, rv = ops.ext().radix_sort_pairs(keys, vals, 64)
    assert np.array_equal(u64view(rk.cpu()), keys_np[order])
    assert np.array_equal(u64view(rv.cpu()), vals_np[order])
    ik, perm = ops.ext().radix_sort_idx32(keys, 64)
    assert np.array_equal(u64view(ik.cpu()), keys_np[order])
    assert np.array_equal(perm.cpu().numpy().astype(np.int64), order)
    assert np.array_equal(u64view(keys.cpu()), keys_np)  # inputs untouched
    assert np.array_equal(u64view(vals.cpu()), vals_np)


def test_radix_sort_fewer_bits(dev):
    """bits=16 runs two of the eight passes.  First half: ops.sort_by_key
    above the small-sort threshold, i.e. the in-tree radix sort; second
    half: radix_sort_pairs directly.  Keys are below 2**16, where both
    must equal the full 64-bit sort."""
    from mapreduce_amd import ops
    rng = np.random.default_rng(5)
    n = (1 << 20) + 77
    assert n >= _small_sort_n()
    keys_np = rng.integers(0, 2 ** 16, size=n, dtype=np.uint64)
    keys = torch.from_numpy(keys_np.view(np.int64)).to(dev)
    (sk,) = ops.sort_by_key(keys, bits=16)
    assert np.array_equal(u64view(sk.cpu()), np.sort(keys_np))
    rk, _ = ops.ext().radix_sort_pairs(keys, _empty(dev), 16)
    assert np.array_equal(u64view(rk.cpu()), np.sort(keys_np))


def test_reduce_by_key_sorted_i64(dev):
    from mapreduce_amd import ops
    rng = np.random.default_rng(7)
    n = 400_000
    keys_np = np.sort(rng.integers(0, 10_000, size=n, dtype=np.uint64) * 7919)
    vals_np = rng.integers(0, 1000, size=n, dtype=np.int64)
    keys = torch.from_numpy(keys_np.view(np.int64)).to(dev)
    vals = torch.from_numpy(vals_np).to(dev)
    uk, uv, _, nseg = ops.reduce_by_key_sorted(keys, vals)
    exp_keys, idx = np.unique(keys_np, return_index=True)
    exp_sums = np.add.reduceat(vals_np, idx)
    assert nseg == len(exp_keys)
    assert np.array_equal(u64view(uk.cpu()), exp_keys)
    assert np.array_equal(uv.cpu().numpy(), exp_sums)


def test_reduce_by_key_counts_and_aux(dev):
    from mapreduce_amd import ops
    keys_np = np.sort(np.repeat(
        np.array([5, 9, 9, 9], dtype=np.uint64) * 10 ** 15, [3, 1, 2, 1]))
    aux_np = np.arange(len(keys_np), dtype=np.uint64) + 100
    keys = torch.from_numpy(keys_np.view(np.int64)).to(dev)
    aux = torch.from_numpy(aux_np.view(np.int64)).to(dev)
    uk, uv, ua, nseg = ops.reduce_by_key_sorted(keys, None, aux)
    assert nseg == 2
    assert uv.cpu().tolist() == [3, 4]
    assert u64view(ua.cpu()).tolist() == [100, 103]  # first aux per segment


def test_reduce_by_key_f64(dev):
    from mapreduce_amd import ops
    rng = np.random.default_rng(11)
    n = 100_000
    keys_np = np.sort(rng.integers(0, 500, size=n, dtype=np.uint64))
    vals_np = rng.standard_normal(n)
    keys = torch.from_numpy(keys_np.view(np.int64)).to(dev)
    vals = torch.from_numpy(vals_np).to(dev)
    uk, uv, _, nseg = ops.reduce_by_key_sorted(keys, vals)
    exp_keys, idx = np.unique(keys_np, return_index=True)
    exp = np.add.reduceat(vals_np, idx)
    assert np.allclose(uv.cpu().numpy(), exp, rtol=1e-12, atol=1e-9)


def test_partition_hist_matches_mulhi(dev):
    from mapreduce_amd import ops
    rng = np.random.default_rng(13)
    n = 500_000
    keys_np = rng.integers(0, 2 ** 64 - 1, size=n, dtype=np.uint64)
    keys = torch.from_numpy(keys_np.view(np.int64)).to(dev)
    # 1000 and 1024 (= MAX_PARTS) take the strided LDS init and flush loops
    # of the 256-thread block through four rounds
    for P in (1, 2, 7, 8, 15, 64, 1000, 1024):
        hist = ops.partition_counts(keys, P).cpu().numpy()
        exp = np.bincount(
            ((keys_np.astype(object) * P) >> 64).astype(np.int64),
            minlength=P)
        assert np.array_equal(hist, exp), P
        assert hist.sum() == n
        assert hist.size == P and (P < 1000 or hist.min() > 0)
    with pytest.raises(RuntimeError, match="nparts too large"):
        ops.partition_counts(keys, 1025)


def test_extract_words_roundtrip(dev):
    from mapreduce_amd import ops
    data = b"alpha beta gamma  delta\nepsilon"
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    h, p, n = ops.tokenize_words(text)
    lens, blob = ops.extract_words(text, p)
    words = []
    raw = bytes(blob.cpu().numpy().tobytes())
    off = 0
    for L in lens.cpu().tolist():
        words.append(raw[off:off + L])
        off += L
    assert sorted(words) == sorted(data.split())


def test_tokenize_spill_matches_python(dev):
    from mapreduce_amd import ops
    text = torch.frombuffer(bytearray(TEXT), dtype=torch.uint8).to(dev)
    from mapreduce_amd.utils.tuple import wordhash64
    ht_empty = (1 << 64) - 1
    # + what the chunked allocator may strand: <= 2048 blocks x 4 waves x
    # one 512-entry chunk
    cap = text.numel() // 2 + 16 + 2048 * 4 * 512
    h, p, c, nw = ops.ext().tokenize_spill_v2(text, 0, cap)
    n = int(c.item())
    assert n <= cap
    exp_words = TEXT.split()
    assert int(nw.item()) == len(exp_words)
    got = [k for k in u64view(h[:n].cpu()).tolist() if k != ht_empty]
    exp = [wordhash64(w) for w in exp_words]
    exp = [ht_empty - 1 if k == ht_empty else k for k in exp]  # remap_key
    assert sorted(got) == sorted(exp)


def test_streaming_wordcount_mode_vs_counter(dev):
    """The full streaming map+combine path (spill -> bucketize -> LDS
    count) vs the naive oracle, including exemplar extraction."""
    from mapreduce_amd.gpu.wordcount import WordCountJob
    rng = np.random.default_rng(23)
    vocab = [f"word{i}x".encode() for i in range(3000)]
    widx = rng.integers(0, len(vocab), size=150_000)
    data = b" ".join(vocab[i] for i in widx.tolist()) + b"\n"
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    job = WordCountJob(dev, vocab_estimate=6000, mode="streaming")
    res = job.run(text)
    assert res.nwords == len(widx)
    got = dict(res.to_host())
    exp = collections.Counter(vocab[i] for i in widx.tolist())
    assert got == dict(exp)
    # hash parity: the engine's dictionary hash must match
    # utils.tuple.wordhash64 bit-for-bit (partitioning consistency).
    from mapreduce_amd.utils.tuple import wordhash64
    got_keys = set(u64view(res.keys.cpu()).tolist())
    assert got_keys == {wordhash64(w) for w in exp}
    # lexicographic materialization option
    lex = res.to_host(order="lex")
    assert [w for w, _ in lex] == sorted(got)
    # topk serving shortcut on device
    top = res.topk(5)
    assert [c for _, c in top] == [c for _, c in exp.most_common(5)]
    for w, c in top:
        assert exp[w] == c
    # point lookups on the device-resident result
    for w in list(exp)[:5]:
        assert res.count_of(w) == exp[w]
    assert res.count_of(b"absent-word-xq") == 0
    # A/B: fused mode must produce identical counts
    job2 = WordCountJob(dev, vocab_estimate=6000, mode="fused")
    res2 = job2.run(text)
    assert dict(res2.to_host()) == got


def test_tokenize_random_binary_all_byte_values(dev):
    """Whitespace classification over ALL 256 byte values (the SWAR
    ws_mask8 path must match bytes.split(): ws = {9..13, 32}; bytes
    >= 128 and control chars are word bytes)."""
    from mapreduce_amd.gpu.wordcount import WordCountJob
    rng = np.random.default_rng(77)
    data = rng.integers(0, 256, size=300_000, dtype=np.uint8)
    # salt in extra whitespace so words stay shortish
    data[rng.random(data.size) < 0.12] = 32
    raw = data.tobytes()
    text = torch.from_numpy(data.copy()).to(dev)
    job = WordCountJob(dev, vocab_estimate=1 << 17, mode="streaming")
    res = job.run(text)
    exp = collections.Counter(raw.split())
    assert res.nwords == sum(exp.values())
    got = dict(res.to_host())
    assert got == dict(exp)


def test_chunked_spill_matches_oracle(dev):
    """A vocabulary larger than the block cache, so that words really
    spill: the wave-chunked spill + radix_pass(56) drain must match the
    oracle exactly."""
    from mapreduce_amd.gpu.wordcount import WordCountJob
    rng = np.random.default_rng(31)
    vocab = [f"tk{i}q".encode() for i in range(8000)]  # > cache: real spill
    widx = rng.integers(0, len(vocab), size=400_000)
    data = b" ".join(vocab[i] for i in widx.tolist()) + b"\n"
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    exp = collections.Counter(vocab[i] for i in widx.tolist())
    job = WordCountJob(dev, vocab_estimate=16000, mode="streaming")
    res = job.run(text)
    assert res.nwords == len(widx)
    assert dict(res.to_host()) == dict(exp)


def test_wordcount_deterministic_across_runs(dev):
    """Counts are exactly reproducible run-to-run despite nondeterministic
    kernel scheduling (aggregation is commutative; exemplars may differ in
    POSITION but always name the same word)."""
    from mapreduce_amd.gpu.corpus import make_corpus
    from mapreduce_amd.gpu.wordcount import WordCountJob
    c = make_corpus(dev, nwords=200_000, nsplits=7, vocab_size=3000, seed=6)
    job = WordCountJob(dev, vocab_estimate=6000)
    r1 = dict(job.run(c.text, c.splits()).to_host())
    r2 = dict(job.run(c.text, c.splits()).to_host())
    assert r1 == r2


def test_cluster_runner_dynamic_gpu(dev):
    """Control-plane dynamic claims driving GPU map jobs (per-job CAS,
    WRITTEN transitions) — single rank on hardware."""
    import collections
    from mapreduce_amd.gpu.corpus import make_corpus
    from mapreduce_amd.gpu.runner import GpuClusterRunner
    from mapreduce_amd.gpu.wordcount import WordCountJob
    c = make_corpus(dev, nwords=100_000, nsplits=6, vocab_size=2000, seed=3)
    job = WordCountJob(dev, vocab_estimate=4000)
    runner = GpuClusterRunner(job, claim_mode="dynamic")
    res = runner.run(c.text, c.splits())
    assert res.nwords == 100_000
    got = dict(res.to_host())
    exp = collections.Counter(bytes(c.text.cpu().numpy().tobytes()).split())
    assert got == dict(exp)
    st = runner.job_stats()
    assert st == {"jobs": 6, "written": 6, "broken": 0,
                  "shuffle_rounds": 1}


def test_streamed_file_wordcount_gpu(dev, tmp_path):
    """K8 path on hardware: pinned staging + side-stream H2D chunks feed
    the engine; counts equal the file oracle; phase tracing populates."""
    from mapreduce_amd.gpu.input import StreamLoader, load_corpus
    from mapreduce_amd.gpu.wordcount import WordCountJob
    rng = np.random.default_rng(41)
    p = tmp_path / "in.txt"
    words = [f"s{int(x)}" for x in rng.integers(0, 500, size=200_000)]
    p.write_text(" ".join(words))
    exp = collections.Counter(open(p, "rb").read().split())

    got = collections.Counter()
    job = WordCountJob(dev, vocab_estimate=1000, timing=True)
    total = 0
    for chunk, base in StreamLoader(str(p), dev, chunk_bytes=256 << 10):
        res = job.run(chunk)
        total += res.nwords
        for w, n in res.to_host():
            got[w] += n
    assert total == len(words)
    assert got == exp
    assert job.last_phase_ms and "map_tokenize" in job.last_phase_ms

    # one-shot load_corpus path
    c = load_corpus([str(p)], dev)
    res = job.run(c.text, c.splits())
    assert dict(res.to_host()) == dict(exp)


def test_gpu_wordcount_pipeline_vs_counter(dev):
    """Fused single-GPU wordcount: tokenize -> hash combine -> sort uniques
    -> counts, vs collections.Counter (the naive oracle)."""
    from mapreduce_amd import ops
    rng = np.random.default_rng(17)
    vocab = [f"w{i}".encode() for i in range(2000)]
    words = rng.choice(len(vocab), size=300_000,
                       p=np.arange(len(vocab), 0, -1) /
                       np.arange(len(vocab), 0, -1).sum())
    data = b" ".join(vocab[i] for i in words.tolist())
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    h, p, n = ops.tokenize_words(text)
    assert n == len(words)
    ht = ops.HashTable(4000, dev)
    ht.insert_count(h, p)
    uk, uv, up = ht.extract()
    sk, sv, sp = ops.sort_by_key(uk, uv, up)
    lens, blob = ops.extract_words(text, sp)
    raw = bytes(blob.cpu().numpy().tobytes())
    got = {}
    off = 0
    for L, c in zip(lens.cpu().tolist(), sv.cpu().tolist()):
        got[raw[off:off + L]] = c
        off += L
    exp = collections.Counter(vocab[i] for i in words.tolist())
    assert got == dict(exp)
    # sortedness of the final key order (u64 bit order)
    ks = u64view(sk.cpu())
    assert np.array_equal(ks, np.sort(ks))


def test_reduce_by_key_min_max(dev):
    """i64 min/max segmented reduce vs NumPy reduceat (negative values
    included — signed comparison, not the u64 bit order keys use)."""
    from mapreduce_amd import ops
    rng = np.random.default_rng(13)
    n = 300_000
    keys_np = np.sort(rng.integers(0, 5_000, size=n, dtype=np.uint64) * 7919)
    vals_np = rng.integers(-10 ** 12, 10 ** 12, size=n, dtype=np.int64)
    keys = torch.from_numpy(keys_np.view(np.int64)).to(dev)
    vals = torch.from_numpy(vals_np).to(dev)
    exp_keys, idx = np.unique(keys_np, return_index=True)
    for op, red in (("min", np.minimum), ("max", np.maximum)):
        uk, uv, _, nseg = ops.reduce_by_key_sorted(keys, vals, op=op)
        assert nseg == len(exp_keys)
        assert np.array_equal(u64view(uk.cpu()), exp_keys)
        assert np.array_equal(uv.cpu().numpy(), red.reduceat(vals_np, idx))
    # f64 twin (native double atomicMin/Max)
    fvals_np = rng.standard_normal(n)
    fvals = torch.from_numpy(fvals_np).to(dev)
    for op, red in (("min", np.minimum), ("max", np.maximum)):
        uk, uv, _, nseg = ops.reduce_by_key_sorted(keys, fvals, op=op)
        assert nseg == len(exp_keys)
        assert np.array_equal(uv.cpu().numpy(), red.reduceat(fvals_np, idx))


def test_reduce_by_key_minmax_nan_gpu(dev):
    """NaN contract on the GPU tier: a NaN never displaces an ordered
    value (atomicMin/Max = IEEE minNum/maxNum); all-NaN segments fall
    through to the init identity (+/-inf) — see ops.reduce_by_key_sorted
    docstring."""
    from mapreduce_amd import ops

    keys = torch.tensor([1, 1, 1, 2, 2, 3], dtype=torch.int64, device=dev)
    vals = torch.tensor([float("nan"), 5.0, 7.0,
                         2.0, float("nan"), float("nan")],
                        dtype=torch.float64, device=dev)
    _, mn, _, _ = ops.reduce_by_key_sorted(keys, vals, op="min")
    _, mx, _, _ = ops.reduce_by_key_sorted(keys, vals, op="max")
    assert mn.cpu().tolist()[:2] == [5.0, 2.0]
    assert mx.cpu().tolist()[:2] == [7.0, 2.0]
    assert mn.cpu().tolist()[2] == float("inf")   # all-NaN -> identity
    assert mx.cpu().tolist()[2] == float("-inf")
    # empty input keeps the value dtype on GPU too
    e = torch.empty(0, dtype=torch.int64, device=dev)
    _, uv, _, _ = ops.reduce_by_key_sorted(
        e, torch.empty(0, dtype=torch.float64, device=dev), e)
    assert uv.dtype == torch.float64


def test_sort_idx32_matches_argsort(dev):
    """idx32 permutation sort vs NumPy stable argsort in u64 order —
    sorted keys AND permutation must match exactly (stability included:
    duplicated keys present)."""
    from mapreduce_amd import ops

    rng = np.random.default_rng(41)
    n = 3_000_000
    keys_np = rng.integers(0, 1 << 20, size=n, dtype=np.uint64) * \
        0x9E3779B97F4A7C15  # duplicates + full-range bits
    keys = torch.from_numpy(keys_np.view(np.int64)).to(dev)
    k, perm32 = ops.sort_idx32(keys)
    order = np.argsort(keys_np, kind="stable")
    assert np.array_equal(u64view(k.cpu()), keys_np[order])
    assert np.array_equal(perm32.cpu().numpy().astype(np.uint32), order)
    # gather_by_u32 applies the permutation to an i64 column
    vals = torch.from_numpy(rng.integers(-2**62, 2**62, size=n)).to(dev)
    g = ops.gather_by_u32(vals, perm32)
    assert np.array_equal(g.cpu().numpy(), vals.cpu().numpy()[order])
    # sort_by_key rides the same path above the small-sort threshold
    k2, v2 = ops.sort_by_key(keys, vals)
    assert torch.equal(k2, k) and torch.equal(v2, g)
