"""The two CPU restatements of the folding merges (tests/merge_fold_ref.py) agree with each other on random small inputs -- several runs,
ties, floats with NaN / -0.0 / +0.0 as keys, descending keys -- and with hand-written cases from the engines' documentation."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import merge_fold_ref as F  # noqa: E402
import merge_sorted_ref as R  # noqa: E402

RUN_LENS = [5, 0, 17, 1, 0, 30, 8]
SPECS = [([np.int64], [(0, False, 1)]), ([np.float64, np.uint8], [(0, False, 1), (1, True, 1)]), ([np.int16, np.float32], [(1, True, -1), (0, False, 1)]),
         ([np.uint32], [(0, True, 1)])]


def _case(seed, dtypes, spec, run_lens=RUN_LENS, distinct=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    offs = R.offsets_of(run_lens)
    cols = [R.random_column(rng, dt, int(offs[-1]), distinct) for dt in dtypes]
    return R.sort_runs(cols, spec, offs), offs, rng


@pytest.mark.parametrize("k", range(len(SPECS)))
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_replacing_forms_agree(k, seed):
    dtypes, spec = SPECS[k]
    cols, offs, rng = _case(seed * 10 + k, dtypes, spec)
    d, n = R.describe(cols, spec), int(offs[-1])
    for vdt in (np.int64, np.uint64, np.int8):
        version = R.random_column(rng, vdt, n, 2)
        deleted = rng.integers(0, 2, n).astype(np.uint8)
        assert np.array_equal(F.replacing_cursor(d, offs), F.replacing_vector(d))
        assert np.array_equal(F.replacing_cursor(d, offs, version), F.replacing_vector(d, version))
        for cleanup in (False, True):
            assert np.array_equal(F.replacing_cursor(d, offs, version, deleted, cleanup), F.replacing_vector(d, version, deleted, cleanup))


@pytest.mark.parametrize("k", range(len(SPECS)))
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_collapsing_forms_agree(k, seed):
    dtypes, spec = SPECS[k]
    cols, offs, rng = _case(seed * 10 + k, dtypes, spec)
    d, n = R.describe(cols, spec), int(offs[-1])
    sign = np.where(rng.integers(0, 2, n) == 1, 1, -1).astype(np.int8)
    got = F.collapsing_cursor(d, offs, sign)
    assert np.array_equal(got, F.collapsing_vector(d, sign)) and 0 < len(got) < n


@pytest.mark.parametrize("k", range(len(SPECS)))
@pytest.mark.parametrize("drop_zero", [False, True])
def test_folding_forms_agree(k, drop_zero):
    dtypes, spec = SPECS[k]
    cols, offs, rng = _case(40 + k, dtypes, spec)
    d, n = R.describe(cols, spec), int(offs[-1])
    values = [rng.integers(-1, 2, n).astype(np.int8), R.random_column(rng, np.uint64, n, 2), R.random_column(rng, np.int32, n, 4), R.random_column(rng, np.uint16, n)]
    for kinds in (["sum", "sum", "min", "max"], ["sum", "max", "sum", "min"], ["min", "max", "max", "min"]):
        a, b = F.folding_cursor(d, offs, values, kinds, drop_zero), F.folding_vector(d, values, kinds, drop_zero)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        for x, y, v in zip(a[2], b[2], values):
            assert x.dtype == y.dtype == v.dtype and np.array_equal(x, y)
    a, b = F.folding_cursor(d, offs, [], [], drop_zero), F.folding_vector(d, [], [], drop_zero)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(a[0]) == len(F.merged_groups_vector(d)[1])


def test_collapsing_documentation_example():
    # (UserID, PageViews, Sign): (5, 146, +1) (5, 146, -1) (6, 185, +1) -> the pair cancels, one row (6, 185, +1) is left
    user = np.array([5, 5, 6], dtype=np.uint64)
    views = np.array([146, 146, 185], dtype=np.uint8)
    sign = np.array([1, -1, 1], dtype=np.int8)
    d = [(user, False, 1)]
    for rows in (F.collapsing_cursor(d, [0, 3], sign), F.collapsing_vector(d, sign)):
        assert rows.tolist() == [2] and (user[rows].tolist(), views[rows].tolist(), sign[rows].tolist()) == ([6], [185], [1])
    # the same rows from two parts: the cancel row arrives in a later part
    for rows in (F.collapsing_cursor(d, [0, 1, 3], sign), F.collapsing_vector(d, sign)):
        assert rows.tolist() == [2]


def test_collapsing_outcomes():
    key = np.zeros(4, dtype=np.int64)
    d = [(key, False, 1)]
    for signs, want in (([-1, 1, -1, 1], [0, 3]), ([1, -1, 1, -1], []), ([1, 1, -1, 1], [3]), ([-1, -1, 1, -1], [0]), ([1, 1, 1, 1], [3]), ([-1, -1, -1, -1], [0])):
        sign = np.array(signs, dtype=np.int8)
        assert F.collapsing_cursor(d, [0, 4], sign).tolist() == want and F.collapsing_vector(d, sign).tolist() == want


def test_summing_documentation_example():
    # keys 1, 1, 2 with values 1, 2, 1 -> (1, 3) (2, 1)
    key = np.array([1, 1, 2], dtype=np.uint32)
    value = np.array([1, 2, 1], dtype=np.uint32)
    d = [(key, False, 1)]
    for first, last, (total,) in (F.folding_cursor(d, [0, 1, 3], [value], ["sum"], True), F.folding_vector(d, [value], ["sum"], True)):
        assert key[first].tolist() == [1, 2] and total.tolist() == [3, 1] and first.tolist() == [0, 2] and last.tolist() == [1, 2]


def test_summing_wraps_and_drops_groups_whose_sums_are_all_zero():
    key = np.array([1, 1, 2, 2, 3, 3], dtype=np.int64)
    a = np.array([127, 1, 5, -5, 1, -1], dtype=np.int8)
    b = np.array([0, 0, 0, 0, 1, 0], dtype=np.uint64)
    d = [(key, False, 1)]
    for f in (F.folding_cursor(d, [0, 6], [a, b], ["sum", "sum"], True), F.folding_vector(d, [a, b], ["sum", "sum"], True)):
        assert f[0].tolist() == [0, 4] and f[2][0].tolist() == [-128, 0] and f[2][1].tolist() == [0, 1]
    for f in (F.folding_cursor(d, [0, 6], [a, b], ["sum", "sum"], False), F.folding_vector(d, [a, b], ["sum", "sum"], False)):
        assert f[0].tolist() == [0, 2, 4]


def test_replacing_takes_the_last_of_the_greatest_versions():
    key = np.zeros(4, dtype=np.int64)
    version = np.array([1, 3, 3, 2], dtype=np.uint64)
    d = [(key, False, 1)]
    for offs in ([0, 4], [0, 2, 4], [0, 1, 2, 3, 4]):
        assert F.replacing_cursor(d, offs, version).tolist() == [2]
    assert F.replacing_vector(d, version).tolist() == [2]
    assert F.replacing_cursor(d, [0, 4]).tolist() == [3] and F.replacing_vector(d).tolist() == [3]
    deleted = np.array([0, 0, 1, 0], dtype=np.uint8)
    assert F.replacing_vector(d, version, deleted, True).tolist() == [] and F.replacing_cursor(d, [0, 4], version, deleted, True).tolist() == []
    assert F.replacing_vector(d, version, deleted, False).tolist() == [2]


def test_bad_values_name_the_lowest_row():
    key = np.array([1, 2, 3, 4], dtype=np.int64)
    d = [(key, False, 1)]
    for form in (lambda s: F.collapsing_cursor(d, [0, 4], s), lambda s: F.collapsing_vector(d, s)):
        with pytest.raises(F.BadValue) as e:
            form(np.array([1, 0, 2, -1], dtype=np.int8))
        assert e.value.row == 1
    with pytest.raises(F.BadValue) as e:
        F.replacing_vector(d, key, np.array([0, 1, 1, 2], dtype=np.uint8))
    assert e.value.row == 3
