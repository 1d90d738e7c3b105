"""tests/asof_ref.py (vectorised, on values) held against oracle.asof_pairs (a Python list and bisect per probe row): every asof dtype,
inequality and join kind on a few hundred rows drawn from the types' edge values, with heavy ties, an empty block, a fully masked block and
absent probe keys; then hand-written rows whose answers are literals.  The GPU edge tests trust asof_ref at sizes the oracle cannot reach."""
import os
import sys

import numpy as np
import pytest

import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asof_ref as R  # noqa: E402

GE, GT, LE, LT = R.ASOF_GREATER_OR_EQUALS, R.ASOF_GREATER, R.ASOF_LESS_OR_EQUALS, R.ASOF_LESS


def test_constants_are_the_oracles():
    for name, value in R.INEQUALITIES.items():
        assert getattr(O, "ASOF_" + name) == value


def edge_case(dtype, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    pool = R.value_pool(dtype)
    build = []
    for n, masks in ((150, "null"), (0, None), (90, "all"), (120, "join"), (60, "both")):
        keys = rng.integers(0, 6, size=n).astype(np.uint16)
        t = pool[rng.integers(0, pool.shape[0], size=n)]
        nm = jm = None
        if masks == "null":
            nm = (rng.random(n) < 0.2).astype(np.uint8)
        elif masks == "all":
            nm = np.ones(n, dtype=np.uint8)
        elif masks == "join":
            jm = (rng.random(n) < 0.8).astype(np.uint8)
        elif masks == "both":
            nm, jm = (rng.random(n) < 0.3).astype(np.uint8), (rng.random(n) < 0.7).astype(np.uint8)
        build.append((keys, t, nm, jm))
    n = 300
    lk = rng.integers(0, 9, size=n).astype(np.uint16)            # keys 6, 7, 8 are absent from the build side
    lt = pool[rng.integers(0, pool.shape[0], size=n)]
    lnm = (rng.random(n) < 0.1).astype(np.uint8)
    return build, lk, lt, lnm


@pytest.mark.parametrize("dtype", R.ASOF_TYPES)
def test_asof_ref_equals_the_oracle(dtype):
    build, lk, lt, lnm = edge_case(dtype, 1000 + np.dtype(dtype).num)
    # the inputs are what the docstring says: ties, an empty block, a fully masked block, absent probe keys
    assert build[1][0].shape[0] == 0 and build[2][2].all() and (lk >= 6).any()
    pairs = set()
    ties = 0
    for keys, t, nm, jm in build:
        for k, v in zip(keys.tolist(), t.tolist()):
            ties += (k, v) in pairs
            pairs.add((k, v))
    assert ties > 50
    for ineq in R.INEQUALITIES.values():
        for left in (False, True):
            for nm in (None, lnm):
                l, b, r = R.asof_ref(build, lk, lt, ineq, nm, left)
                assert l.dtype == b.dtype == r.dtype == np.int64
                got = list(zip(l.tolist(), b.tolist(), r.tolist()))
                assert got == O.asof_pairs(build, lk, lt, ineq, nm, left), (dtype, ineq, left)
                assert 0 < (b >= 0).sum() and (left and (b < 0).any() or not left and len(got) < lk.shape[0])


def test_asof_ref_empty_sides():
    e = np.zeros(0, dtype=np.uint32)
    for left in (False, True):
        l, b, r = R.asof_ref([], np.array([1, 2], dtype=np.uint32), np.array([5, 6], dtype=np.uint32), GE, None, left)
        assert (l.tolist(), b.tolist(), r.tolist()) == (([0, 1], [-1, -1], [-1, -1]) if left else ([], [], []))
        l, b, r = R.asof_ref([(e, e, None, None)], e, e, LT, None, left)
        assert l.shape == b.shape == r.shape == (0,)


def _rows(build, lk, lt, ineq, left=True, nm=None):
    l, b, r = R.asof_ref(build, np.asarray(lk, dtype=build[0][0].dtype), np.asarray(lt, dtype=build[0][1].dtype), ineq, nm, left)
    return list(zip(l.tolist(), b.tolist(), r.tolist()))


def test_hand_written_rows_one_per_inequality():
    #                 row:   0   1   2   3   4
    k = np.array([7, 7, 7, 9, 7], dtype=np.uint32)
    t = np.array([30, 10, 20, 10, 40], dtype=np.int32)
    build = [(k, t, None, None)]
    probes = ([7, 7, 7, 7, 9, 8], [20, 25, 5, 45, 10, 20])
    assert _rows(build, *probes, GE) == [(0, 0, 2), (1, 0, 2), (2, -1, -1), (3, 0, 4), (4, 0, 3), (5, -1, -1)]
    assert _rows(build, *probes, GT) == [(0, 0, 1), (1, 0, 2), (2, -1, -1), (3, 0, 4), (4, -1, -1), (5, -1, -1)]
    assert _rows(build, *probes, LE) == [(0, 0, 2), (1, 0, 0), (2, 0, 1), (3, -1, -1), (4, 0, 3), (5, -1, -1)]
    assert _rows(build, *probes, LT) == [(0, 0, 0), (1, 0, 0), (2, 0, 1), (3, -1, -1), (4, -1, -1), (5, -1, -1)]
    assert _rows(build, *probes, LT, left=False) == [(0, 0, 0), (1, 0, 0), (2, 0, 1)]
    # a NULL left key has no partner
    assert _rows(build, [7, 7], [20, 20], GE, nm=np.array([1, 0], dtype=np.uint8)) == [(0, -1, -1), (1, 0, 2)]


def test_hand_written_ties_in_each_direction():
    # value 20 of key 1 sits at (block 0, row 1), (block 0, row 3) and (block 2, row 0); block 1 is empty
    b0 = (np.array([1, 1, 1, 1], dtype=np.uint8), np.array([10, 20, 30, 20], dtype=np.uint16), None, None)
    b1 = (np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint16), None, None)
    b2 = (np.array([1, 2], dtype=np.uint8), np.array([20, 20], dtype=np.uint16), None, None)
    build = [b0, b1, b2]
    assert _rows(build, [1, 1], [20, 25], GE) == [(0, 2, 0), (1, 2, 0)]      # the last inserted
    assert _rows(build, [1, 1], [21, 30], GT) == [(0, 2, 0), (1, 2, 0)]
    assert _rows(build, [1, 1], [20, 15], LE) == [(0, 0, 1), (1, 0, 1)]      # the first inserted
    assert _rows(build, [1, 1], [19, 10], LT) == [(0, 0, 1), (1, 0, 1)]
    # the last copy masked out by the ON mask, the first by the null map: the last / first SURVIVING copy wins
    b2m = (b2[0], b2[1], None, np.array([0, 1], dtype=np.uint8))
    b0m = (b0[0], b0[1], np.array([0, 1, 0, 0], dtype=np.uint8), None)
    assert _rows([b0m, b1, b2m], [1], [20], GE) == [(0, 0, 3)]
    assert _rows([b0m, b1, b2m], [1], [20], LE) == [(0, 0, 3)]
    assert _rows([b0m, b1, b2], [1], [20], LE) == [(0, 0, 3)]
    assert _rows([b0, b1, b2m], [1], [20], GE) == [(0, 0, 3)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hand_written_signed_zeros_and_nan(dtype):
    k = np.zeros(3, dtype=np.int64)
    build = [(k, np.array([-1.0, 0.0, np.nan], dtype=dtype), None, None)]
    probe = ([0, 0], [-0.0, np.nan])
    assert _rows(build, *probe, GE) == [(0, 0, 1), (1, -1, -1)]            # -0.0 >= +0.0
    assert _rows(build, *probe, LE) == [(0, 0, 1), (1, -1, -1)]            # -0.0 <= +0.0
    assert _rows(build, *probe, GT) == [(0, 0, 0), (1, -1, -1)]            # not -0.0 > +0.0: the next one down
    assert _rows(build, *probe, LT) == [(0, -1, -1), (1, -1, -1)]          # not -0.0 < +0.0, and NaN was never inserted
    assert _rows(build, *probe, GE, left=False) == [(0, 0, 1)]
    # the other way round, and the two zeros as a tie
    build = [(k, np.array([-0.0, 0.0, -0.0], dtype=dtype), None, None)]
    assert _rows(build, [0], [0.0], GE) == [(0, 0, 2)]
    assert _rows(build, [0], [0.0], LE) == [(0, 0, 0)]
    assert _rows(build, [0], [0.0], GT) == [(0, -1, -1)]
    assert _rows(build, [0], [0.0], LT) == [(0, -1, -1)]
