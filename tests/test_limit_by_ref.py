"""tests/limit_by_ref.py against itself (no GPU): the loop and the vectorised form agree, both give the two hand-checked vectors,
DISTINCT is numpy's first positions, and the split of an input into blocks does not change the answer."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import limit_by_ref as R  # noqa: E402
from limit_by_ref import LimitByLoop, LimitByRef  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = [(1, 0), (1, 1), (2, 0), (2, 1), (3, 5), (1000, 0)]


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def test_constants_agree_with_the_host_header():
    text = open(os.path.join(REPO, "clickhouse_amd", "csrc", "limit_by_host.h")).read()
    assert int(re.search(r"LB_TILE = (\d+);", text).group(1)) == R.LB_TILE
    assert int(re.search(r"LB_CAP_MIN = (\d+);", text).group(1)) == R.LB_CAP_MIN
    assert int(re.search(r"LB_NONE = (0x[0-9A-Fa-f]+)u;", text).group(1), 16) == R.LB_NONE


@pytest.mark.parametrize("cls", [LimitByLoop, LimitByRef])
@pytest.mark.parametrize("length,offset,blocks,want", R.VECTORS)
def test_the_two_vectors(cls, length, offset, blocks, want):
    op = cls(length, offset)
    for b, w in zip(blocks, want):
        got, passed = op.filter_block(np.array(b, dtype=np.uint32))
        assert got.tolist() == w and passed == sum(w)


@pytest.mark.parametrize("length,offset", BOUNDS)
@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.uint64, np.int64])
def test_loop_and_vectorised_forms_agree_on_random_blocks(length, offset, dtype):
    rng = _rng(length * 131 + offset * 7 + np.dtype(dtype).itemsize)
    a, b = LimitByLoop(length, offset), LimitByRef(length, offset)
    info = np.iinfo(dtype)
    pool = rng.integers(info.min, info.max, size=23, dtype=dtype, endpoint=True)
    pool[:3] = [0, info.max, info.min]
    for blk in range(6):
        n = int(rng.integers(0, 400))
        keys = pool[rng.integers(0, pool.shape[0], size=n)]
        filt = None if blk % 2 == 0 else (rng.random(n) < 0.7).astype(np.uint8)
        lo = int(rng.integers(0, n + 1))
        hi = int(rng.integers(lo, n + 1))
        ga, pa = a.filter_block(keys, lo, hi, filt)
        gb, pb = b.filter_block(keys, lo, hi, filt)
        assert np.array_equal(ga, gb) and pa == pb and ga.shape[0] == hi - lo
        assert a.count == b.count and a.keys() == b.keys()


def test_negative_keys_are_their_raw_bits():
    assert R.bits(np.array([-1, 0, 1], dtype=np.int8)).tolist() == [255, 0, 1]
    assert R.bits(np.array([-1], dtype=np.int64)).tolist() == [2**64 - 1]


def test_distinct_is_the_first_position_of_every_value():
    rng = _rng(5)
    keys = rng.integers(0, 300, size=5000).astype(np.uint32)
    got, passed = LimitByRef(1, 0).filter_block(keys)
    _, first = np.unique(keys, return_index=True)
    want = np.zeros(keys.shape[0], dtype=np.uint8)
    want[first] = 1
    assert np.array_equal(got, want) and passed == first.shape[0]


@pytest.mark.parametrize("length,offset", BOUNDS)
def test_the_split_into_blocks_does_not_change_the_filter(length, offset):
    rng = _rng(11 + length + offset)
    keys = rng.integers(0, 40, size=3000).astype(np.uint16)
    filt = (rng.random(keys.shape[0]) < 0.8).astype(np.uint8)
    results = []
    for parts in (1, 2, 7):
        op = LimitByRef(length, offset)
        cuts = np.linspace(0, keys.shape[0], parts + 1).astype(int)
        results.append(np.concatenate([op.filter_block(keys, int(a), int(b), filt)[0] for a, b in zip(cuts[:-1], cuts[1:])]))
    assert np.array_equal(results[0], results[1]) and np.array_equal(results[0], results[2])
    assert np.array_equal(results[0], LimitByLoop(length, offset).filter_block(keys, filter=filt)[0])
