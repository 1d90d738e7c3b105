"""The uniqExact reference (tests/uniq_exact_ref.py) pinned on hand-written cases.  No GPU."""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from uniq_exact_ref import UniqExactRef, bits, from_bits  # noqa: E402


def _f64(word):
    return np.array([word], dtype=np.uint64).view(np.float64)[0]


def _f32(word):
    return np.array([word], dtype=np.uint32).view(np.float32)[0]


def test_positive_and_negative_zero_are_two_values():
    r = UniqExactRef(np.uint32, np.float64).add(np.array([7, 7, 7], dtype=np.uint32), np.array([0.0, -0.0, 0.0]))
    assert r.finalize() == {7: 2}
    assert r.pairs == {(7, 0), (7, 1 << 63)}


def test_nan_payloads():
    a, b = _f64(0x7FF8000000000001), _f64(0x7FF8000000000002)
    r = UniqExactRef(np.uint8, np.float64).add(np.array([1, 1, 1, 1], dtype=np.uint8), np.array([a, b, a, b]))
    assert len(r) == 2 and r.finalize() == {1: 2}          # one payload: one value; two payloads: two
    r.add(np.array([1], dtype=np.uint8), np.array([_f64(0xFFF8000000000001)]))
    assert r.finalize() == {1: 3}                            # the sign bit is part of the bits


def test_float32_is_compared_as_its_32_bits():
    x32 = np.array([_f32(0x7FC00001), _f32(0x7FC00002), np.float32(1.5), np.float32(1.5)], dtype=np.float32)
    r = UniqExactRef(None, np.float32).add(None, x32)
    assert r.pairs == {(0, 0x7FC00001), (0, 0x7FC00002), (0, struct.unpack("<I", struct.pack("<f", 1.5))[0])}
    # the same numbers as Float64 have other bits: the two sets share nothing but the count
    r64 = UniqExactRef(None, np.float64).add(None, np.array([1.5, 1.5]))
    assert r64.pairs == {(0, struct.unpack("<Q", struct.pack("<d", 1.5))[0])}
    assert bits(np.array([-1], dtype=np.int8)).tolist() == [0xFF]   # zero-extended, not sign-extended
    assert from_bits([0xFF], np.int8).tolist() == [-1]


def test_the_zero_pair_and_all_ones_are_ordinary():
    k = np.array([0, 0, 2**64 - 1, 2**64 - 1, 0], dtype=np.uint64)
    v = np.array([0, 0, 2**64 - 1, 0, 2**64 - 1], dtype=np.uint64)
    r = UniqExactRef(np.uint64, np.uint64).add(k, v)
    assert r.pairs == {(0, 0), (2**64 - 1, 2**64 - 1), (2**64 - 1, 0), (0, 2**64 - 1)}
    assert r.finalize() == {0: 2, 2**64 - 1: 2}
    assert r.counts_for_keys(np.array([0, 5, 2**64 - 1], dtype=np.uint64)).tolist() == [2, 0, 2]


def test_filter_bytes_0_1_2_255():
    k = np.array([1, 2, 3, 4, 4], dtype=np.uint16)
    v = np.array([10, 20, 30, 40, 41], dtype=np.int32)
    r = UniqExactRef(np.uint16, np.int32).add(k, v, filter=np.array([0, 1, 2, 255, 0], dtype=np.uint8))
    assert r.finalize() == {2: 1, 3: 1, 4: 1}                # key 1 never entered: no group
    assert r.counts_for_keys(np.array([1, 4], dtype=np.uint16)).tolist() == [0, 1]
    r.add(k, v, row_begin=4, row_end=5)
    assert r.finalize() == {2: 1, 3: 1, 4: 2}


def test_without_key_on_an_empty_set_is_one_zero():
    r = UniqExactRef(None, np.int64)
    assert r.finalize() == {None: 0}
    r.add(None, np.array([5, 5, 6], dtype=np.int64), filter=np.zeros(3, dtype=np.uint8))
    assert r.finalize() == {None: 0}
    r.add(None, np.array([5, 5, 6], dtype=np.int64))
    assert r.finalize() == {None: 2}


def test_merge_is_union():
    a = UniqExactRef(np.uint8, np.uint8).add(np.array([1, 1], dtype=np.uint8), np.array([1, 2], dtype=np.uint8))
    b = UniqExactRef(np.uint8, np.uint8).add(np.array([1, 2], dtype=np.uint8), np.array([2, 2], dtype=np.uint8))
    a.merge(b)
    assert a.finalize() == {1: 2, 2: 1} and b.finalize() == {1: 1, 2: 1}
