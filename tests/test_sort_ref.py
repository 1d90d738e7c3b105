"""tests/sort_ref.py (vectorised, on values) held against oracle/sorting.py (per-row comparator): every dtype, direction and NaN hint at up
to 400 rows, on inputs that are mostly ties and special values.  The GPU edge tests trust sort_ref at sizes the comparator cannot reach."""
import os
import sys

import numpy as np
import pytest

from oracle import sorting as OS

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sort_ref as R  # noqa: E402

TYPES = [np.int64, np.uint64, np.int32, np.uint32, np.int16, np.uint16, np.int8, np.uint8, np.float64, np.float32]


def special_values(dtype):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        fi = np.finfo(dt)
        bits ={4: (np.uint32, 0x7FC00001, 0xFFC00000, 0x7F800001), 8: (np.uint64, 0x7FF8000000000001, 0xFFF8000000000000, 0x7FF0000000000001)}[dt.itemsize]
        nans = np.array(bits[1:], dtype=bits[0]).view(dt)    # quiet, negative quiet and signalling NaN payloads
        return np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, np.nan, fi.max, -fi.max, fi.tiny, -fi.tiny, fi.smallest_subnormal,
                                         -fi.smallest_subnormal, 1.0, -1.0, 1.5, 2.0], dtype=dt), nans])
    ii = np.iinfo(dt)
    v = [ii.min, ii.max, 0, 1, 2, ii.max - 1, ii.min + 1, ii.max // 2, ii.max // 2 + 1]
    if ii.min < 0:
        v += [-1, -2]
    return np.array(v, dtype=dt)


def tie_heavy(rng, dtype, n):
    sp = special_values(dtype)
    x = sp[rng.integers(0, sp.shape[0], size=n)]
    x[rng.random(n) < 0.3] = sp[0]          # one large tie class
    return x


@pytest.mark.parametrize("dtype", TYPES)
def test_sort_ref_equals_the_comparator_oracle(dtype):
    rng = np.random.Generator(np.random.PCG64(np.dtype(dtype).num))
    for n in (0, 1, 2, 3, 17, 400):
        x = tie_heavy(rng, dtype, n)
        for desc in (False, True):
            for hint in (1, -1):
                got = R.get_permutation(x, desc, hint)
                assert got.dtype == np.uint64 and np.array_equal(got, OS.get_permutation(x, desc, hint)), (dtype, n, desc, hint)


def test_sort_ref_pinned_semantics():
    x = np.array([2.0, np.nan, -0.0, 1.0, 0.0, np.nan, 2.0, -np.inf], dtype=np.float64)   # the rows test_sorting.py pins for the oracle
    assert R.get_permutation(x, False, 1).tolist() == [7, 2, 4, 3, 0, 6, 1, 5]
    assert R.get_permutation(x, False, -1).tolist() == [1, 5, 7, 2, 4, 3, 0, 6]
    assert R.get_permutation(x, True, -1).tolist() == [0, 6, 3, 2, 4, 7, 1, 5]
    assert R.get_permutation(x, True, 1).tolist() == [1, 5, 0, 6, 3, 2, 4, 7]


def test_sort_ref_sort_block_equals_the_comparator_oracle():
    rng = np.random.Generator(np.random.PCG64(11))
    n = 300
    cols = [tie_heavy(rng, dt, n) for dt in (np.uint8, np.float32, np.int64, np.float64)]
    for spec in ([(0, False, 1), (1, True, -1)], [(1, False, -1), (0, True, 1), (3, True, 1)], [(3, False, 1), (2, True, 1), (1, False, 1)]):
        d = [(cols[p], desc, hint) for p, desc, hint in spec]
        assert np.array_equal(R.sort_block(d), OS.sort_block(d)), spec
