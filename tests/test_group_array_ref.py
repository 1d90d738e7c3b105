"""tests/group_array_ref.py pinned on hand-written cases (no GPU): the reference the device tests compare against must itself be the
contract of include/chgpu.h -- arrival order across blocks, merge order, max_size across a merge, absent keys, without key, empty --
and must agree with the constants and the pass planning of clickhouse_amd/csrc/group_array_host.h and with the Python class."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import group_array_ref as R  # noqa: E402
from group_array_ref import GroupArrayRef  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _the_operator_this_reference_is_for():
    # a reference without its operator pins nothing: every case here needs the class the device tests drive
    sys.path.insert(0, REPO)
    from clickhouse_amd.group_array import GroupArray
    assert GroupArray._prefix == "chgpu_group_array"


def _arrays(ref):
    return {k: v.tolist() for k, v in ref.arrays().items()}


def test_the_python_class_exists_and_names_its_functions():
    sys.path.insert(0, REPO)
    import clickhouse_amd
    from clickhouse_amd.group_array import GroupArray
    assert clickhouse_amd.GroupArray is GroupArray and GroupArray._prefix == "chgpu_group_array"


def test_constants_agree_with_the_host_header():
    text = open(os.path.join(REPO, "clickhouse_amd", "csrc", "group_array_host.h")).read()
    for name, value in (("GA_TILE", R.GA_TILE), ("GA_UNIT", R.GA_UNIT)):
        m = re.search(rf"static constexpr uint64_t {name} = (\d+);", text)
        assert m and int(m.group(1)) == value, name


def test_order_across_blocks_ranges_and_filters():
    ref = GroupArrayRef(np.uint32, np.int64)
    ref.add(np.array([7, 3, 7, 3, 7], dtype=np.uint32), np.array([10, 11, 12, 13, 14], dtype=np.int64))
    ref.add(np.array([3, 7, 9, 3], dtype=np.uint32), np.array([20, 21, 22, 23], dtype=np.int64), row_begin=1, row_end=4)
    ref.add(np.array([9, 9, 7], dtype=np.uint32), np.array([30, 31, 32], dtype=np.int64), filter=np.array([0, 5, 1], dtype=np.uint8))
    assert _arrays(ref) == {3: [11, 13, 23], 7: [10, 12, 14, 21, 32], 9: [22, 31]}
    gk, off, data = ref.finalize()
    assert gk.tolist() == [3, 7, 9] and off.tolist() == [3, 8, 10] and off.dtype == np.uint64
    assert data.tolist() == [11, 13, 23, 10, 12, 14, 21, 32, 22, 31] and len(ref) == 10
    k, v = ref.pairs()
    assert k.tolist() == [7, 3, 7, 3, 7, 7, 9, 3, 9, 7] and v.tolist() == [10, 11, 12, 13, 14, 21, 22, 23, 31, 32]


def test_merge_puts_the_source_behind_the_destination_and_leaves_it():
    a = GroupArrayRef(np.uint8, np.int32).add(np.array([1, 2], dtype=np.uint8), np.array([1, 2], dtype=np.int32))
    b = GroupArrayRef(np.uint8, np.int32).add(np.array([2, 1, 5], dtype=np.uint8), np.array([3, 4, 5], dtype=np.int32))
    a.merge(b)
    assert _arrays(a) == {1: [1, 4], 2: [2, 3], 5: [5]}
    assert _arrays(b) == {1: [4], 2: [3], 5: [5]}
    b.merge(a)
    assert _arrays(b) == {1: [4, 1, 4], 2: [3, 2, 3], 5: [5, 5]}


def test_max_size_is_the_first_n_also_across_a_merge():
    a = GroupArrayRef(np.uint16, np.uint8, max_size=3).add(np.array([4, 4, 6], dtype=np.uint16), np.array([1, 2, 3], dtype=np.uint8))
    b = GroupArrayRef(np.uint16, np.uint8, max_size=3).add(np.array([4, 4, 4, 6, 8], dtype=np.uint16), np.array([4, 5, 6, 7, 8], dtype=np.uint8))
    a.merge(b)
    assert _arrays(a) == {4: [1, 2, 4], 6: [3, 7], 8: [8]}      # dst's values first, then N - size of src's
    assert a.trimmed() == 2 and len(a) == 8                       # the store keeps every entered row
    one = GroupArrayRef(np.uint16, np.uint8, max_size=1).add(np.array([4, 4, 6], dtype=np.uint16), np.array([1, 2, 3], dtype=np.uint8))
    assert _arrays(one) == {4: [1], 6: [3]} and one.finalize()[1].tolist() == [1, 2]


def test_values_come_back_bit_for_bit_and_signed_keys_are_their_bits():
    nan_a = np.array([0x7FC00001], dtype=np.uint32).view(np.float32)[0]
    nan_b = np.array([0xFFC12345], dtype=np.uint32).view(np.float32)[0]
    values = np.array([nan_a, -0.0, nan_b, 0.0, np.inf], dtype=np.float32)
    ref = GroupArrayRef(np.int8, np.float32).add(np.array([-1, -1, 2, -1, 2], dtype=np.int8), values)
    gk, off, data = ref.finalize()
    assert gk.tolist() == [2, 0xFF] and off.tolist() == [2, 5]
    assert R.bits(data).tolist() == [0xFFC12345, 0x7F800000, 0x7FC00001, 0x80000000, 0]


def test_for_keys_absent_twice_and_zero_rows():
    ref = GroupArrayRef(np.uint32, np.int64).add(np.array([7, 3, 7], dtype=np.uint32), np.array([10, 11, 12], dtype=np.int64))
    off, data = ref.for_keys(np.array([7, 5, 3, 7], dtype=np.uint32))
    assert off.tolist() == [2, 2, 3, 5] and data.tolist() == [10, 12, 11, 10, 12]
    off, data = ref.for_keys(np.zeros(0, dtype=np.uint32))
    assert len(off) == 0 and len(data) == 0 and data.dtype == np.int64
    empty = GroupArrayRef(np.uint32, np.int64)
    off, data = empty.for_keys(np.array([1, 2], dtype=np.uint32))
    assert off.tolist() == [0, 0] and len(data) == 0
    limited = GroupArrayRef(np.uint32, np.int64, max_size=1).add(np.array([7, 3, 7], dtype=np.uint32), np.array([10, 11, 12], dtype=np.int64))
    off, data = limited.for_keys(np.array([7, 7, 9], dtype=np.uint32))
    assert off.tolist() == [1, 2, 2] and data.tolist() == [10, 10]


def test_without_key_and_empty():
    ref = GroupArrayRef(None, np.float64)
    gk, off, data = ref.finalize()
    assert gk is None and off.tolist() == [0] and len(data) == 0 and ref.passes() == 0
    ref.add(None, np.array([3.0, 1.0, 2.0]), filter=np.array([1, 0, 1], dtype=np.uint8))
    assert _arrays(ref) == {None: [3.0, 2.0]}
    lim = GroupArrayRef(None, np.float64, max_size=1).add(None, np.array([3.0, 1.0]))
    assert lim.finalize()[1].tolist() == [1] and lim.finalize()[2].tolist() == [3.0]
    keyed_empty = GroupArrayRef(np.uint64, np.float64)
    gk, off, data = keyed_empty.finalize()
    assert len(gk) == 0 and len(off) == 0 and len(data) == 0 and keyed_empty.passes() == 0


def test_passes_are_the_key_bytes_that_vary():
    assert R.varying_bytes(np.array([5, 5, 5], dtype=np.uint64)) == []
    assert R.varying_bytes(np.array([0x0000050000000011, 0x0000070000000011], dtype=np.uint64)) == [5]
    assert R.varying_bytes(np.array([0x0100000000000001, 0x0200000000000002], dtype=np.uint64)) == [0, 7]
    assert R.varying_bytes(np.array([0, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)) == list(range(8))
    assert R.varying_bytes(np.array([0x1FF, 0x100], dtype=np.uint64)) == [0]
    ref = GroupArrayRef(np.int16, np.uint8).add(np.array([-1, 1], dtype=np.int16), np.array([1, 2], dtype=np.uint8))
    assert ref.passes() == 2   # 0xFFFF and 0x0001 as zero-extended bits


def test_check_column_array_accepts_any_row_order_and_catches_a_swap():
    ref = GroupArrayRef(np.uint32, np.int64).add(np.array([7, 3, 7, 9], dtype=np.uint32), np.array([10, 11, 12, 13], dtype=np.int64))
    keys = np.array([9, 7, 3], dtype=np.uint32)
    off = np.array([1, 3, 4], dtype=np.uint64)
    assert R.check_column_array(keys, off, np.array([13, 10, 12, 11], dtype=np.int64), ref) is None
    assert "values differ" in R.check_column_array(keys, off, np.array([13, 12, 10, 11], dtype=np.int64), ref)
    assert "lengths" in R.check_column_array(keys, np.array([2, 3, 4], dtype=np.uint64), np.array([13, 10, 12, 11], dtype=np.int64), ref)
    assert R.check_column_array(keys[:2], off[:2], np.array([13, 10, 12], dtype=np.int64), ref) is not None
