"""The two CPU restatements of the merge of sorted runs (tests/merge_sorted_ref.py) agree with each other and with the oracle's stable
sort of the concatenation: all ten dtypes, both directions, both NaN hints, -0.0 / +0.0 / NaN ties, empty runs, limits."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import merge_sorted_ref as R  # noqa: E402
from oracle import sorting  # noqa: E402

RUN_LENS = [5, 0, 17, 1, 0, 30, 8]


def _case(seed, dtypes, spec, run_lens=RUN_LENS):
    rng = np.random.Generator(np.random.PCG64(seed))
    offs = R.offsets_of(run_lens)
    cols = [R.random_column(rng, dt, int(offs[-1])) for dt in dtypes]
    return R.sort_runs(cols, spec, offs), offs


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("hint", [1, -1])
def test_forms_agree_with_the_oracle_sort_for_every_dtype(dtype, descending, hint):
    spec = [(0, descending, hint)]
    cols, offs = _case(11, [dtype], spec)
    d = R.describe(cols, spec)
    assert R.is_sorted_ref(d, offs) is None
    want = sorting.sort_block(d)
    assert np.array_equal(R.merge_cursors(d, offs), want)
    assert np.array_equal(R.merge_lexsort(d), want)


def test_float_ties_across_runs_keep_the_run_order():
    # every run holds NaN, -0.0 and +0.0: equal rows come out by run number, then by row
    run = np.array([-0.0, 0.0, -0.0, np.nan, np.nan], dtype=np.float64)
    col = np.concatenate([run, run, run])
    offs = R.offsets_of([5, 5, 5])
    d = [(col, False, 1)]
    assert R.is_sorted_ref(d, offs) is None
    want = np.array([0, 1, 2, 5, 6, 7, 10, 11, 12, 3, 4, 8, 9, 13, 14], dtype=np.uint64)
    assert np.array_equal(R.merge_cursors(d, offs), want)
    assert np.array_equal(R.merge_lexsort(d), want)
    assert np.array_equal(sorting.sort_block(d), want)
    d = [(col, True, 1)]   # descending, NaN greatest: NaNs first; the zeros are still one tie class
    nan_first = np.array([3, 4, 8, 9, 13, 14, 0, 1, 2, 5, 6, 7, 10, 11, 12], dtype=np.uint64)
    assert R.is_sorted_ref(d, offs) == 3   # as an ascending run it is not sorted descending
    assert np.array_equal(R.merge_lexsort(d), nan_first)
    assert np.array_equal(sorting.sort_block(d), nan_first)


@pytest.mark.parametrize("spec,dtypes", [
    ([(0, False, 1), (1, True, 1)], [np.uint8, np.int64]),
    ([(1, True, -1), (0, False, 1), (2, False, -1)], [np.int16, np.float32, np.float64]),
    ([(2, False, 1), (0, True, 1)], [np.uint64, np.int8, np.uint32]),
])
def test_several_columns(spec, dtypes):
    cols, offs = _case(5, dtypes, spec)
    d = R.describe(cols, spec)
    want = sorting.sort_block(d)
    assert np.array_equal(R.merge_cursors(d, offs), want)
    assert np.array_equal(R.merge_lexsort(d), want)


@pytest.mark.parametrize("run_lens", [[], [0], [0, 0, 0], [4], [0, 3], [3, 0], [1] * 9])
@pytest.mark.parametrize("limit", [0, 1, 3, 100])
def test_empty_runs_and_limits(run_lens, limit):
    spec = [(0, True, 1), (1, False, 1)]
    cols, offs = _case(3, [np.float32, np.uint16], spec, run_lens)
    d = R.describe(cols, spec)
    want = sorting.sort_block(d) if len(cols[0]) else np.zeros(0, dtype=np.uint64)
    want = want[:limit] if limit else want
    assert np.array_equal(R.merge_cursors(d, offs, limit), want)
    assert np.array_equal(R.merge_lexsort(d, limit), want)


def test_is_sorted_ref_reports_the_lowest_row_and_skips_run_boundaries():
    col = np.array([1, 2, 3, 0, 5, 9, 2, 1], dtype=np.int32)
    assert R.is_sorted_ref([(col, False, 1)], R.offsets_of([3, 5])) == 6       # the drop at row 3 is a run boundary
    assert R.is_sorted_ref([(col, False, 1)], R.offsets_of([8])) == 3
    assert R.is_sorted_ref([(col, False, 1)], R.offsets_of([3, 3, 1, 1])) is None
    assert R.is_sorted_ref([(col, False, 1)], R.offsets_of([3, 0, 0, 3, 2])) == 7
    f = np.array([np.nan, 1.0, -0.0, 0.0], dtype=np.float64)
    assert R.is_sorted_ref([(f, False, -1)], R.offsets_of([4])) == 2
    assert R.is_sorted_ref([(f, False, 1)], R.offsets_of([4])) == 1
