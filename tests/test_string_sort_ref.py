"""The reference of the String sort (tests/string_sort_ref.py) orders what the C ABI promises, and the word-round scheme the kernels
implement -- key (word, c) per 8-byte word, segments with their own depth -- agrees with it.  No GPU."""
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import string_sort_ref as ssr  # noqa: E402


def test_zero_byte_ladder_and_high_bytes():
    values = [b"ab\1", b"ab\0\0", b"ab", b"ab\0", b"a", b"", b"b"]
    assert [values[i] for i in ssr.get_permutation(values)] == [b"", b"a", b"ab", b"ab\0", b"ab\0\0", b"ab\1", b"b"]
    assert [values[i] for i in ssr.get_permutation(values, descending=True)] == [b"b", b"ab\1", b"ab\0\0", b"ab\0", b"ab", b"a", b""]
    # bytes are unsigned: 0x7f < 0x80 < 0xff, and the shorter of two values that agree is the smaller
    values = [b"\x80", b"\x7f", b"\xff", b"\x7f\xff", b"\x80\x00"]
    assert ssr.get_permutation(values) == [1, 3, 0, 4, 2]


def test_empty_strings_and_ties_keep_incoming_order_in_both_directions():
    values = [b"b", b"", b"a", b"", b"b", b"a", b""]
    assert ssr.get_permutation(values) == [1, 3, 6, 2, 5, 0, 4]
    assert ssr.get_permutation(values, descending=True) == [0, 4, 2, 5, 1, 3, 6]
    # the incoming order is perm_in order when one is given; entries beyond the column count as row 0; limit cuts the full permutation
    assert ssr.get_permutation(values, perm_in=[6, 5, 4, 3, 2, 1, 0]) == [6, 3, 1, 5, 2, 4, 0]
    assert ssr.get_permutation(values, perm_in=[4, 4, 99, 1]) == [1, 4, 4, 0]
    assert ssr.get_permutation(values, limit=4) == [1, 3, 6, 2]
    assert ssr.get_permutation(values, limit=7) == ssr.get_permutation(values, limit=12) == ssr.get_permutation(values)


def test_key_keeps_a_value_apart_from_its_zero_padded_twin():
    assert ssr.key_at(b"ab", 0, False) < ssr.key_at(b"ab\0", 0, False) < ssr.key_at(b"ab\0\0", 0, False) < ssr.key_at(b"ab\1", 0, False)
    assert ssr.key_at(b"ab", 0, True) > ssr.key_at(b"ab\0", 0, True)
    assert ssr.key_at(b"12345678", 0, False)[1] == 8 and ssr.key_at(b"123456789", 0, False)[1] == 9
    assert ssr.key_at(b"12345678", 1, False) == (0, 0) and ssr.key_at(b"123456789", 1, False) == (ord("9") << 56, 1)


def _random_column(rng, n):
    alphabet = rng.choice([b"\0a", b"ab", b"\0\x7f\x80\xff", bytes(range(256))])
    lengths = rng.choice([[0, 1, 7, 8, 9], [15, 16, 17], [23, 24, 25, 40], [0, 1, 7, 8, 9, 15, 16, 17, 24, 25, 40]])
    prefix = bytes(rng.choice(alphabet) for _ in range(rng.choice([0, 0, 3, 8, 19, 64])))
    values = []
    for _ in range(n):
        v = bytes(rng.choice(alphabet) for _ in range(rng.choice(lengths)))
        values.append(prefix + v if rng.random() < 0.8 else v)
    return values


def test_word_round_model_agrees_with_sorted_on_a_seeded_fuzz():
    rng = random.Random(20260419)
    for case in range(400):
        n = rng.choice([0, 1, 2, 5, 30, 120])
        values = _random_column(rng, n)
        descending = rng.random() < 0.5
        perm_in = None
        if n and rng.random() < 0.4:
            perm_in = [rng.randrange(n) for _ in range(rng.randrange(0, n + 1))] if rng.random() < 0.5 else rng.sample(range(n), n)
        m = n if perm_in is None else len(perm_in)
        limit = rng.choice([0, 0, 1, max(1, m // 2), max(1, m - 1), m, m + 5])
        want = ssr.get_permutation(values, descending, perm_in, limit)
        got = ssr.word_round_model(values, descending, perm_in, limit)
        assert got == want, (case, values, descending, perm_in, limit)


def test_rounds_do_not_grow_with_a_prefix_a_whole_segment_shares():
    short, long_ = [], []
    values = [b"p" * 1024 + bytes([i % 7]) for i in range(50)] + [b"q", b"", b"p" * 1024]
    assert ssr.word_round_model(values, stats=long_) == ssr.get_permutation(values)
    values = [b"p" * 8 + bytes([i % 7]) for i in range(50)] + [b"q", b"", b"p" * 8]
    assert ssr.word_round_model(values, stats=short) == ssr.get_permutation(values)
    assert len(long_) == len(short) == 2


def test_multi_column_reference():
    ints = np.array([2, 1, 2, 1, 2], dtype=np.int64)
    strs = [b"b", b"a", b"a", b"a", b"b"]
    assert ssr.sort_block([(ints, False, 1), (strs, False, 1)]) == [1, 3, 2, 0, 4]
    assert ssr.sort_block([(strs, True, 1), (ints, True, 1)]) == [0, 4, 2, 1, 3]
