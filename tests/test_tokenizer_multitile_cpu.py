"""CPU self-check of the case generators in tokenizer_multitile_common: the
properties test_tokenizer_multitile.py relies on really hold, and the
record checker accepts a correct tokenization and refuses broken ones.
Needs no GPU."""

import collections

import pytest

import tokenizer_multitile_common as tc


def python_records(text: bytes, start: int = 0):
    """(keys, pos) of every word of text[start:], offsets into text."""
    keys, pos = [], []
    i, n = start, len(text)
    while i < n:
        if text[i] in tc.WS:
            i += 1
            continue
        j = i
        while j < n and text[j] not in tc.WS:
            j += 1
        keys.append(tc.device_key(text[i:j]))
        pos.append((i << 16) | min(j - i, 0xFFFF))
        i = j
    return keys, pos


def test_walk_sizes_cover_what_they_claim():
    sizes = set(tc.WALK_SIZES)
    T, H = tc.TILE, tc.HALO
    assert {0, 1, 15, 16, 17} <= sizes
    for edge in (T, T + H, 2 * T):
        assert {edge - 1, edge, edge + 1} <= sizes
    assert any(n % T and n > 2 * T for n in sizes)
    assert 24 * T in sizes
    assert set(tc.WALK_BLOCKS) == {1, 2, 3}
    # with 1..3 blocks a block owns both odd and even tile counts
    owned = {-(-(-(-n // T)) // b) for n in sizes if n for b in tc.WALK_BLOCKS}
    assert any(x % 2 for x in owned) and any(x % 2 == 0 for x in owned)


@pytest.mark.parametrize("n", tc.WALK_SIZES)
def test_walk_text(n):
    text, expect = tc.walk_text(n)
    assert len(text) == n and tc.walk_text(n)[0] == text  # seeded
    T, H = tc.TILE, tc.HALO
    for k in range(1, n // T + 1):
        if k * T < n:  # a word stands across (or up to) every tile edge
            assert any(o < k * T <= o + len(w) for o, w in expect), k
    if n >= T + H + 40:
        o, w = expect[0]
        assert o < T and o + len(w) > T + H and len(w) == 100
    if n >= 24 * T:
        assert sum(1 for o, w in expect
                   if o < (o // T) * T + H < o + len(w)) >= 22
    keys, pos = python_records(text)
    got, where = tc.check_records(text, keys, pos)
    assert got == tc.key_oracle(text)
    assert all((o, len(w)) in where for o, w in expect)


def test_unaligned_text():
    text, expect = tc.unaligned_text()
    assert 3 * tc.TILE < len(text) < 3 * tc.TILE + tc.HALO
    for s in tc.UNALIGNED_STARTS:
        assert text[s - 1] in tc.WS and text[s] not in tc.WS
        keys, pos = python_records(text, s)
        got, where = tc.check_records(text, keys, pos)
        assert got == tc.key_oracle(text[s:])
        assert min(o for o, _ in where) == s
    assert len(expect) == 2


def test_same_key_texts():
    texts = tc.same_key_texts()
    assert texts["a_x8192"] == b"a " * 8192
    assert texts["the_x4096"] == b"the " * 4096
    a, b = tc.slot_sharing_pair()
    ka, kb = tc.device_key(a), tc.device_key(b)
    assert ka != kb and tc.cache_slot(ka) == tc.cache_slot(kb)
    assert collections.Counter(texts["slot_pair"].split()) == {a: 2048,
                                                               b: 2048}
    for t in texts.values():
        assert len(t) >= 4 * tc.TILE and len(t) % tc.TILE == 0


def test_saturation_text():
    text = tc.saturation_text()
    assert len(text) == 24 * tc.TILE
    assert len(tc.key_oracle(text)) > 2 * tc.CACHE_SLOTS


def test_checker_refuses_broken_records():
    text, _ = tc.walk_text(4097)
    keys, pos = python_records(text)
    tc.check_records(text, keys + [tc.HT_EMPTY], pos + [12345])  # pads pass
    with pytest.raises(AssertionError):  # a length one short
        tc.check_records(text, keys[:1], [pos[0] - 1])
    with pytest.raises(AssertionError):  # an offset one late
        tc.check_records(text, keys[:1], [pos[0] + (1 << 16)])
    with pytest.raises(AssertionError):  # another word's key
        tc.check_records(text, keys[1:2], pos[:1])
    assert tc.digest(keys, pos) == tc.digest(keys[::-1] + [tc.HT_EMPTY],
                                             pos[::-1] + [0])
    assert tc.digest(keys, pos) != tc.digest(keys[1:], pos[1:])


def test_composite_key_and_doc_lookup():
    so = [0, 10, 20]
    assert [tc.doc_of(o, so) for o in (0, 9, 10, 19, 20, 99)] == [
        0, 0, 1, 1, 2, 2]
    assert tc.composite_key(b"abc", 3) != tc.composite_key(b"abc", 4)
    assert tc.composite_key(b"abc", 3) == (
        tc.device_key(b"abc") ^ tc.splitmix64(3))


def test_composite_oracle_counts_every_occurrence():
    text, _ = tc.walk_text(8193)
    so = [0, len(text) // 3 + 7, 2 * len(text) // 3 + 11]
    oracle = tc.composite_oracle(text, so, 3)
    assert sum(oracle.values()) == len(text.split())
    first = text.split()[0]
    assert oracle[tc.composite_key(first, 3)] >= 1  # offset 0 is doc 0 + 3
    plain = tc.key_oracle(text)
    assert len(oracle) > len(plain)  # a word in two documents is two keys
