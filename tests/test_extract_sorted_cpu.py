"""CPU tier of ops.extract_sorted: on a CpuHashTable it composes the _cpu
functions into the same tuple the GPU op returns."""

import numpy as np
import torch


def test_cpu_tier_matches_composed_path():
    from mapreduce_amd import ops
    from mapreduce_amd.ops import _cpu

    rng = np.random.default_rng(7)
    n = 500
    keys = np.unique(rng.integers(0, 2 ** 64 - 1, size=n, dtype=np.uint64))
    keys = rng.permutation(np.unique(np.concatenate(
        [keys, np.array([0, 2 ** 63, 2 ** 64 - 2], dtype=np.uint64)])))
    text = torch.from_numpy(rng.integers(0, 256, size=4096, dtype=np.uint8))
    ln = rng.integers(0, 30, size=keys.size).astype(np.uint64)
    off = rng.integers(0, 4000, size=keys.size).astype(np.uint64)
    pos = (off << np.uint64(16)) | ln
    table = ops.make_table(1024, "cpu")
    assert isinstance(table, _cpu.CpuHashTable)
    tk = torch.from_numpy(keys.view(np.int64))
    table.insert_count(tk, torch.from_numpy(pos.view(np.int64)))
    table.insert_sum(tk, torch.arange(keys.size, dtype=torch.int64))

    k, v, p = table.extract()
    sk, sv, sp = ops.sort_by_key(k, v, p)
    lens, blob = ops.extract_words(text, sp)
    order = np.argsort(keys, kind="stable")
    np.testing.assert_array_equal(sk.numpy().view(np.uint64), keys[order])

    gk, gv, gp, gl, go, total, packed = ops.extract_sorted(table)
    assert torch.equal(gk, sk) and torch.equal(gv, sv)
    assert torch.equal(gp, sp) and torch.equal(gl, lens)
    assert torch.equal(go, torch.cumsum(lens, 0) - lens)
    assert total == blob.numel() == int(ln.sum())
    assert torch.equal(packed, torch.cat([sk, sv, lens]))
    assert torch.equal(ops.gather_words(text, gp, go, total), blob)

    empty = ops.extract_sorted(ops.make_table(16, "cpu", exemplar=False))
    assert all(x.numel() == 0 for x in empty[:5]) and empty[5] == 0
