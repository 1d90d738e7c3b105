"""The host-side fold of ONE state row -- the states of an aggregation without key, an overflow row -- on each of its four paths:
without-key merge, without-key one-row merge_states, the overflow-row fold of a merge under limits (no_more_keys and BREAK) and the
is_overflows block of merge_states.  Every word class passes through each of them: integer adds (count, Int64 sum, `seen` words), the
Float64 sum (a fixed-point pair with a key, a plain double without one or after an infinity), min / max order keys, any {claim, value}
and argMin {val key, claim, arg}, under -If and Nullable conditions.

The reference is tests/agg_conditions_ref.py (row order, plain Python): one Ref per partial state, folded with FnState.merge.  Every
comparison is bit for bit; the floats are multiples of 2^-8 below 2^20, so every order of addition gives the same double.  Two things
keep any / argMin independent of the order the device happens to merge concurrent states in: the vals of argMin are distinct over a
whole case, and among the source's groups that the destination lacks only ONE has a row that reaches any()."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import agg_conditions_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

AGGS = [(R.COUNT, None, "if"), (R.SUM, np.float64, "if"), (R.MIN, np.int32, "if"), (R.MAX, np.int64, "null"), (R.ANY, np.int64, "if"),
        (R.ARG_MIN, (np.int64, np.int32), "null"), (R.SUM, np.int64, "null")]
MODES = [m for _, _, m in AGGS]
ANY_J = 4
# block sizes of one partial state; "masked": every row fails every condition / is NULL
SIDES = {"1": [1], "63": [63], "64+65": [64, 65], "1000": [1000], "empty": [], "masked": [65]}
PAIRS = [("1000", "63"), ("64+65", "1"), ("empty", "1000"), ("1000", "empty"), ("masked", "64+65"), ("63", "masked")]


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


class Vals:
    """argument columns for n rows; argMin's vals are distinct over everything one instance hands out"""

    def __init__(self, seed):
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.vals = iter(self.rng.permutation(8192).astype(np.int32) - 4096)

    def block(self, keys, masked=False):
        n, rng = len(keys), self.rng
        f = (rng.integers(-(1 << 27), 1 << 27, size=n) / 256.0).astype(np.float64)
        i64 = rng.integers(-(1 << 62), 1 << 62, size=n)
        i32 = rng.integers(-(1 << 31), 1 << 31, size=n).astype(np.int32)
        v = np.array([next(self.vals) for _ in range(n)], dtype=np.int32)
        args = [None, f, i32, i64, i64, (i64, v), i64]
        byte = rng.choice(np.array([0, 0, 1, 2, 255], dtype=np.uint8), size=n)
        null = (rng.random(n) < 0.5).astype(np.uint8)
        conds = [(np.zeros(n, np.uint8) if m == "if" else np.ones(n, np.uint8)) if masked else (byte if m == "if" else null).copy() for m in MODES]
        return np.asarray(keys), args, conds


def _fold(dst, src):
    for d, s in zip(dst, src):
        d.merge(s)


def _assert_row(ref, st, got_cols, got_flags):
    for j in range(len(AGGS)):
        v, f = ref.value_of(j, st[j])
        g = np.asarray(got_cols[j])
        assert g.dtype == ref.result_dtype(j) and g.tobytes() == np.array([v], dtype=ref.result_dtype(j)).tobytes(), (j, g, v)
        assert (got_flags[j] is None and f is None) or int(got_flags[j][0]) == f, (j, got_flags[j], f)


def _assert_groups(ag, ref):
    keys, res, maps = ag.convert_to_block(null_maps=True)
    klist = [None] if keys is None else keys.tolist()
    assert sorted(klist, key=lambda k: -1 if k is None else k) == sorted(ref.groups, key=lambda k: -1 if k is None else k)
    want, want_maps = ref.columns(klist)
    for j in range(len(AGGS)):
        assert res[j].dtype == want[j].dtype and res[j].tobytes() == want[j].tobytes(), (j, res[j], want[j])
        assert (maps[j] is None and want_maps[j] is None) or maps[j].tobytes() == want_maps[j].tobytes(), j


def _assert_overflow(ag, ref, st):
    cols, flags = ag.overflow_row(final=True, null_maps=True)
    _assert_row(ref, st, [c.numpy() for c in cols], flags)


# ---- without a key: merge, and one-row merge_states ----------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", PAIRS)
def test_without_key_merge_and_one_row_merge_states(ch, a, b):
    ctx = ch.Context(0)
    vals = Vals(11 + len(a) * 7 + len(b))
    parts, refs = [], []
    for side in (a, b):
        blocks = [vals.block(np.zeros(n, np.uint8), masked=side == "masked") for n in SIDES[side]]
        ag, twin, ref = ch.Aggregator(None, AGGS, ctx=ctx), ch.Aggregator(None, AGGS, ctx=ctx), R.Ref(AGGS)
        ref.groups[None] = ref._new()
        for _, args, conds in blocks:
            ag.execute_on_block(None, args, conds=conds)
            twin.execute_on_block(None, args, conds=conds)
            ref.add_block(None, args, conds=conds)
        parts.append((ag, twin))
        refs.append(ref)
    refs[0].merge(refs[1])
    parts[0][0].merge(parts[1][0])
    _assert_groups(parts[0][0], refs[0])
    into = ch.Aggregator(None, AGGS, ctx=ctx)
    for _, twin in parts:
        _, words, rows = twin.export_state_columns()
        assert rows == 1 and len(words) == twin.n_words
        into.merge_states(None, words, rows)
    _assert_groups(into, refs[0])


# ---- with a key, under limits --------------------------------------------------------------------------------------------------------
M = 8
DST_KEYS, SRC_KEYS = np.arange(0, 12), np.arange(6, 18)     # (the zero key among them); 6 .. 11 are in both tables
DST_MISS, SRC_MISS = np.arange(20, 30), np.arange(30, 40)   # reach only the side's own overflow row
ANY_KEY = 17                                                # the one source-only group that has an any() value


def _limited_side(ch, ctx, vals, table_keys, miss_keys, side, mode="any", inf_at=None):
    """One partial state: a first block of 24 rows opens 12 groups (> M: the limit trips), then find-only blocks of the side's sizes over
    the table's keys and keys it lacks.  -> (Aggregator, Ref)"""
    masked = side == "masked"
    ag = ch.Aggregator(np.uint32, AGGS, ctx=ctx, max_rows_to_group_by=M, group_by_overflow_mode=mode, overflow_row=True)
    ref = R.Ref(AGGS)
    keys, args, conds = vals.block(np.concatenate([table_keys, table_keys]).astype(np.uint32), masked=masked)
    conds[ANY_J][(keys >= 12) & (keys != ANY_KEY)] = 0
    if inf_at is not None:
        args[1][inf_at], conds[1][inf_at] = np.inf, 1
    keep = ag.execute_on_block(keys, args, conds=conds)
    ref.add_block(keys, args, conds=conds, overflow_row=True)
    assert len(ag) == 12 and keep is (mode == "any") and ag.no_more_keys is (mode == "any")
    for n in (SIDES[side] if mode == "any" else []):
        keys = vals.rng.choice(np.concatenate([table_keys, miss_keys]), size=n).astype(np.uint32)
        keys, args, conds = vals.block(keys, masked=masked)
        conds[ANY_J][(keys >= 12) & (keys < 20) & (keys != ANY_KEY)] = 0
        ag.execute_on_block(keys, args, conds=conds)
        ref.add_block(keys, args, conds=conds, find_only=True, overflow_row=True)
    return ag, ref


def _merge_no_more_keys(rd, rs):
    """mergeDataNoMoreKeysImpl on the references: the overflow rows first, then the source's groups"""
    _fold(rd.overflow, rs.overflow)
    for key, st in rs.groups.items():
        _fold(rd.groups[key] if key in rd.groups else rd.overflow, st)


@pytest.mark.parametrize("a,b", PAIRS)
def test_overflow_rows_fold_in_a_merge_under_no_more_keys(ch, a, b):
    ctx = ch.Context(0)
    vals = Vals(23 + len(a) * 5 + len(b))
    dst, rd = _limited_side(ch, ctx, vals, DST_KEYS, DST_MISS, a)
    src, rs = _limited_side(ch, ctx, vals, SRC_KEYS, SRC_MISS, b)
    assert dst.merge(src) is True and dst.merge_no_more_keys
    _merge_no_more_keys(rd, rs)
    assert len(dst) == 12
    _assert_groups(dst, rd)
    _assert_overflow(dst, rd, rd.overflow)


@pytest.mark.parametrize("b", ["1000", "64+65", "masked", "empty"])
def test_only_the_overflow_rows_merge_under_break(ch, b):
    ctx = ch.Context(0)
    vals = Vals(37 + len(b))
    dst, rd = _limited_side(ch, ctx, vals, DST_KEYS, DST_MISS, "empty", mode="break")
    src, rs = _limited_side(ch, ctx, vals, SRC_KEYS, SRC_MISS, b)
    assert dst.merge(src) is False
    _fold(rd.overflow, rs.overflow)
    _assert_groups(dst, rd)   # (the keyed data stayed out)
    _assert_overflow(dst, rd, rd.overflow)


@pytest.mark.parametrize("a,b", PAIRS)
def test_an_is_overflows_block_carries_every_word_class(ch, a, b):
    ctx = ch.Context(0)
    vals = Vals(41 + len(a) * 3 + len(b))
    dst, rd = _limited_side(ch, ctx, vals, DST_KEYS, DST_MISS, a)
    src, rs = _limited_side(ch, ctx, vals, SRC_KEYS, SRC_MISS, b)
    words = src.overflow_row(final=False)
    assert len(words) == src.n_words
    assert dst.merge_states(None, words, 1, is_overflows=True) is True
    _fold(rd.overflow, rs.overflow)
    _assert_groups(dst, rd)
    _assert_overflow(dst, rd, rd.overflow)


@pytest.mark.parametrize("inf_side", ["dst", "src"])
def test_overflow_rows_fold_as_plain_doubles_after_an_infinity(ch, inf_side):
    """one side met +inf in a row that reaches the Float64 sum of a group both tables hold: both sides go back to double states, the
    overflow rows add as doubles (exact for these values) in the merge and in an is_overflows block after it, that group's sum is +inf"""
    ctx = ch.Context(0)
    vals = Vals(53 + len(inf_side))
    dst, rd = _limited_side(ch, ctx, vals, DST_KEYS, DST_MISS, "1000", inf_at=7 if inf_side == "dst" else None)   # row 7: key 7
    src, rs = _limited_side(ch, ctx, vals, SRC_KEYS, SRC_MISS, "64+65", inf_at=1 if inf_side == "src" else None)   # row 1: key 7
    assert dst.merge(src) is True
    _merge_no_more_keys(rd, rs)
    _assert_groups(dst, rd)
    _assert_overflow(dst, rd, rd.overflow)
    keys, res, _ = dst.convert_to_block(null_maps=True)
    assert res[1][keys.tolist().index(7)] == np.inf
    # dst keeps double states from here on: an is_overflows block's Float64 word adds as a double too
    extra, re = _limited_side(ch, ctx, vals, SRC_KEYS, SRC_MISS, "63")
    assert dst.merge_states(None, extra.overflow_row(final=False), 1, is_overflows=True) is True
    _fold(rd.overflow, re.overflow)
    _assert_overflow(dst, rd, rd.overflow)
