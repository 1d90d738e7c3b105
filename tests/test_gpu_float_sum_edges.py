"""The fixed-point Float64 sums of GROUP BY (agg_kernels.hip, Fx128) at their numeric edges: carries and borrows between the
two words of a state in every plan, the one rounding at the fold, windows that move by 1 .. 73 bits (through blocks, merges and imported
states), conditions, and more rows than one window holds.

The expectations come from tests/fx_sum_ref.py, a model in Python integers; tests/test_fx_sum_ref.py asserts, without a GPU, that every
input here is made of whole numbers of its window's unit -- so the model's sum is the exact sum and its fold is math.fsum -- except where
a case is about truncation, and there the model is the expectation.  Every comparison is bit for bit unless stated."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fx_sum_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


@pytest.fixture(scope="module")
def ctx(ch):
    c = ch.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.shape[0] == 0, (what, f"{bad.shape[0]} of {want.shape[0]} differ", [(int(i), float(got[i]), float(want[i])) for i in bad[:5]])


def _result(A):
    gk, res = A.convert_to_block()
    order = np.argsort(gk)
    return gk[order], [r[order] for r in res]


def _sum_of(ch, ctx, kd, blocks, hint=16, kind=None, dtype=np.float64):
    """the sorted (keys, sums) of one aggregation over `blocks` of (keys, values)"""
    A = ch.Aggregator(kd, [(ch.AGG_SUM if kind is None else kind, dtype)], size_hint=hint, ctx=ctx)
    for k, v in blocks:
        A.execute_on_block(ctx.upload(np.ascontiguousarray(k, dtype=kd)), [ctx.upload(np.ascontiguousarray(v, dtype=dtype))])
    gk, (s,) = _result(A)
    return gk, s


def _model_of(blocks):
    m = R.Model()
    for k, v in blocks:
        m.add_block(k, v)
    return m


def _by_key(model, keys):
    res = model.result()
    return np.array([res[int(k)] for k in keys])


# ---- a. carries and borrows, in every plan ---------------------------------------------------------------------------------------------
CARRY_CASES = [(p, 53) for p in R.PLAN_SHAPES] + [(p, 24) for p in R.FLOAT32_PLANS]


@pytest.mark.parametrize("plan,mant_bits", CARRY_CASES, ids=[f"{p}-{'f64' if b == 53 else 'f32'}" for p, b in CARRY_CASES])
def test_carries_and_borrows_in_every_plan(ch, capfd, plan, mant_bits):
    kd, rows, groups, hint, opts, plan_words = R.PLAN_SHAPES[plan]
    k, v, _, _ = R.carry_input(plan, mant_bits)
    uk, want, counts = R.carry_expect(plan, mant_bits)
    dt = np.float64 if mant_bits == 53 else np.float32
    vt = v.astype(dt)
    assert np.array_equal(vt.astype(np.float64), v)
    shapes = {"sum": [(ch.AGG_SUM, dt)], "avg": [(ch.AGG_AVG, dt)]}
    if plan == "contended":
        shapes = {"sum": [(ch.AGG_SUM, dt), (ch.AGG_MAX, np.float64)], "avg": [(ch.AGG_AVG, dt), (ch.AGG_MAX, np.float64)]}
        _, order, starts, _ = R.group_rows(k)
        want_max = np.maximum.reduceat(v[order], starts)
    c = ch.Context(0)
    try:
        for opt, value in opts.items():
            c.set_option(opt, value)
        c.set_option("debug", 1)
        kcol, vcol = c.upload(k), c.upload(vt)
        vmax = c.upload(v) if plan == "contended" else None
        for name, aggs in shapes.items():
            runs = []
            for _ in range(2):
                A = ch.Aggregator(kd, aggs, size_hint=hint, ctx=c)
                capfd.readouterr()
                A.execute_on_block(kcol, [vcol, vmax][:len(aggs)])
                gk, res = _result(A)
                err = capfd.readouterr().err
                del A
                lines = [ln for ln in err.splitlines() if ln.startswith("chgpu: ") and "GROUP BY" in ln and "finish rounds" not in ln]
                assert lines and all(w in ln for ln in lines for w in plan_words), (plan, name, err)
                runs.append(res)
                assert np.array_equal(gk, uk)
                _same(res[0], want if name == "sum" else want / counts, (plan, name))
                if plan == "contended":
                    _same(res[1], want_max, (plan, name, "max"))
            assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0])), (plan, name, "two runs differ")
        del kcol, vcol, vmax
    finally:
        c.close()


# ---- b. the rounding at the fold ---------------------------------------------------------------------------------------------------------
FOLD_CASES = R.fold_cases()


@pytest.mark.parametrize("name", list(FOLD_CASES))
def test_fold_rounds_once_to_nearest_even(ch, ctx, name):
    vals = FOLD_CASES[name]
    base, leaves = R.window(vals)
    assert not leaves
    want = R.fold(sum(R.units(x, base) for x in vals), base)
    A = ch.Aggregator(np.uint32, [(ch.AGG_SUM, np.float64), (ch.AGG_AVG, np.float64)], size_hint=16, ctx=ctx)
    col = ctx.upload(np.array(vals))
    A.execute_on_block(ctx.upload(np.full(len(vals), 5, dtype=np.uint32)), [col, col])
    gk, (s, a) = _result(A)
    assert gk.tolist() == [5]
    _same(s, [want], name)
    _same(a, [want / len(vals)], name + " avg")


@pytest.mark.parametrize("name", list(R.spans_both_words_cases()))
def test_fold_whose_remainder_spans_both_words(ch, ctx, name):
    n, big, small = R.spans_both_words_cases()[name]
    base, _ = R.window([big] + small, n + len(small))
    want = R.fold(n * R.units(big, base) + sum(R.units(x, base) for x in small), base)
    v = np.full(n + len(small), big)
    at = np.linspace(1, n, num=len(small), dtype=np.int64)
    v[at] = small
    gk, s = _sum_of(ch, ctx, np.uint32, [(np.full(v.shape[0], 3, dtype=np.uint32), v)])
    _same(s, [want], name)


def test_one_binade_beyond_the_window_is_truncated_per_row(ch, ctx):
    vals = np.array(R.beyond_the_window())
    base, _ = R.window(vals.tolist())
    want = R.fold(sum(R.units(x, base) for x in vals.tolist()), base)
    assert want != math.fsum(vals.tolist())
    for hint in (16, 1_000_000):
        gk, s = _sum_of(ch, ctx, np.uint32, [(np.full(vals.shape[0], 11, dtype=np.uint32), vals)], hint=hint)
        _same(s, [want], hint)


def test_spread_of_73_binades_is_exact_and_74_goes_back_to_doubles(ch, ctx):
    k, v = R.spread_block(73)
    uk, want, _ = R.fsum_groups(k, v)
    gk, s = _sum_of(ch, ctx, np.uint32, [(k, v)])
    assert np.array_equal(gk, uk)
    _same(s, want, 73)
    k, v = R.spread_block(74)
    uk, want, counts = R.fsum_groups(k, v)
    gk, s = _sum_of(ch, ctx, np.uint32, [(k, v)])
    # double adds in hardware order: n * 2^-52 * sum|v| (derived in test_gpu_group_by_launch_arms.py)
    bound = counts * 2.0 ** -52 * np.bincount(np.unique(k, return_inverse=True)[1], weights=np.abs(v))
    print("spread 74: max error / bound", (np.abs(s - want) / bound).max())
    assert np.array_equal(gk, uk) and np.all(np.abs(s - want) <= bound)


# ---- c. a later block widens the window --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh", R.SHIFTS)
def test_window_widened_by_a_larger_exponent(ch, ctx, sh):
    k1, v1, k2, v2 = R.two_scale_blocks(sh)
    uk, want, counts = R.fsum_groups(np.concatenate([k1, k2]), np.concatenate([v1, v2]))
    for kind in (ch.AGG_SUM, ch.AGG_AVG):
        runs = [_sum_of(ch, ctx, np.uint32, [(k1, v1), (k2, v2)], hint=64, kind=kind) for _ in range(2)]
        assert np.array_equal(runs[0][0], uk)
        _same(runs[0][1], want if kind == ch.AGG_SUM else want / counts, (sh, kind))
        assert np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))


def test_widening_floors_states_that_are_no_multiples(ch, ctx):
    k1, v1, k2, v2 = R.two_scale_blocks(50, exact=False)
    m = _model_of([(k1, v1), (k2, v2)])
    outs = []
    for hint in (64, 1_000_000):
        gk, s = _sum_of(ch, ctx, np.uint32, [(k1, v1), (k2, v2)], hint=hint)
        _same(s, _by_key(m, gk), hint)
        outs.append(s)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))


# ---- d. merges, exported and imported states ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh", R.SHIFTS)
def test_merge_of_two_windows_in_both_directions(ch, ctx, sh):
    k1, v1, k2, v2 = R.two_scale_blocks(sh)
    uk, want, _ = R.fsum_groups(np.concatenate([k1, k2]), np.concatenate([v1, v2]))
    for flip in (False, True):
        fine = ch.Aggregator(np.uint32, [(ch.AGG_SUM, np.float64)], size_hint=64, ctx=ctx)
        coarse = ch.Aggregator(np.uint32, [(ch.AGG_SUM, np.float64)], size_hint=64, ctx=ctx)
        fine.execute_on_block(ctx.upload(k1), [ctx.upload(v1)])
        coarse.execute_on_block(ctx.upload(k2), [ctx.upload(v2)])
        dst, src = (coarse, fine) if flip else (fine, coarse)
        dst.merge(src)
        gk, (s,) = _result(dst)
        assert np.array_equal(gk, uk)
        _same(s, want, (sh, flip))


def test_exported_states_are_rounded_once_and_merge_back(ch, ctx):
    T = 2.0 ** 52
    k = np.array([1, 1, 2, 2, 2, 4], dtype=np.uint32)
    v = np.array([T + 1, T, 0.5, 0.25, 2.0 ** 40, -(T + 1)])
    A = ch.Aggregator(np.uint32, [(ch.AGG_SUM, np.float64)], size_hint=16, ctx=ctx)
    A.execute_on_block(ctx.upload(k), [ctx.upload(v)])
    A.execute_on_block(ctx.upload(np.array([4], dtype=np.uint32)), [ctx.upload(np.array([-T]))])
    keys, states, rows = A.export_state_columns()
    ek, es = keys.numpy(), states[0].numpy()
    order = np.argsort(ek)
    assert rows == 3 and ek[order].tolist() == [1, 2, 4]
    exported = [2.0 ** 53, 2.0 ** 40 + 0.75, -(2.0 ** 53)]                                      # 2^53 + 1 leaves as 2^53, and so does its negative
    _same(es[order], exported)
    C = ch.Aggregator(np.uint32, [(ch.AGG_SUM, np.float64)], size_hint=16, ctx=ctx)
    C.merge_states(keys, states, rows)
    k3, v3 = np.array([1, 2, 4, 6], dtype=np.uint32), np.array([1.0, 0.25, -1.0, 3.0])
    C.execute_on_block(ctx.upload(k3), [ctx.upload(v3)])
    m = R.Model()
    m.merge_doubles([1, 2, 4], exported)
    m.add_block(k3, v3)
    gk, (s,) = _result(C)
    assert gk.tolist() == [1, 2, 4, 6]
    _same(s, _by_key(m, gk))
    _same(s, [2.0 ** 53, 2.0 ** 40 + 1.0, -(2.0 ** 53), 3.0])                                   # 2^53 + 1 again: a tie, to even; 2^53 + 2 had the states kept their bits


def test_states_imported_into_a_coarser_window(ch, ctx):
    r = R.rng("import")
    n = 500
    sk = np.arange(n, dtype=np.uint32)
    # 53-bit states at exponent -10 arrive in a window whose unit is 2^(40 - 96): their last six bits are cut, toward zero
    sv = np.ldexp((r.integers(0, 1 << 52, size=n) + (1 << 52)).astype(np.float64), -62) * r.choice(np.array([-1.0, 1.0]), size=n)
    k0, v0 = np.array([9, 3], dtype=np.uint32), np.array([2.0 ** 40, -(2.0 ** 40)])
    D = ch.Aggregator(np.uint32, [(ch.AGG_SUM, np.float64)], size_hint=1000, ctx=ctx)
    D.execute_on_block(ctx.upload(k0), [ctx.upload(v0)])
    D.merge_states(ctx.upload(sk), [ctx.upload(sv)], n)
    m = _model_of([(k0, v0)])
    m.merge_doubles(sk, sv)
    assert m.fixed and m.base == 40 - 96
    gk, (s,) = _result(D)
    assert np.array_equal(gk, sk)
    want = _by_key(m, gk)
    assert np.count_nonzero(want[np.arange(n) != 9] != sv[np.arange(n) != 9]) > n // 2   # (the cut shows)
    _same(s, want)


# ---- e. -If and Nullable arguments over the mix --------------------------------------------------------------------------------------------
def test_conditions_keep_the_window_on_the_kept_rows(ch, ctx):
    k, v, keep = R.masked_mix()
    base = R.CARRY_E - 33 - 96
    uk, us, _ = R.unit_sums(k, np.where(keep == 1, v, 0.0), base)
    want = R.fold_many(us, base)
    kept = np.bincount(np.unique(k, return_inverse=True)[1], weights=keep).astype(np.float64)
    aggs = [(ch.AGG_SUM, np.float64, "if"), (ch.AGG_AVG, np.float64, "if"), (ch.AGG_SUM, np.float64, "null")]
    outs = []
    for _ in range(2):
        A = ch.Aggregator(np.uint32, aggs, size_hint=1000, ctx=ctx)
        col = ctx.upload(v)
        A.execute_on_block(ctx.upload(k), [col, col, col], conds=[keep * np.uint8(255), keep, (1 - keep).astype(np.uint8)])
        gk, res, maps = A.convert_to_block(null_maps=True)
        order = np.argsort(gk)
        gk, (s_if, a_if, s_null) = gk[order], [r[order] for r in res]
        assert np.array_equal(gk, uk) and maps[0] is None and np.array_equal(maps[2][order] != 0, kept == 0)
        _same(s_if, want, "sumIf")
        _same(s_null, want, "sum of Nullable")
        some = kept > 0
        assert some.sum() > 900 and np.all(np.isnan(a_if[~some]))
        _same(a_if[some], (want / np.where(some, kept, 1.0))[some], "avgIf")
        outs.append(s_if)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))


# ---- f. more rows than one window holds ------------------------------------------------------------------------------------------------------
BIG_ROWS, BIG_TIMES = 1 << 22, 257


@pytest.fixture(scope="module")
def big(ctx):
    k, v = R.big_block(BIG_ROWS)
    return k, v, ctx.upload(k), ctx.upload(v)


@pytest.mark.parametrize("hint", [16, 0])
def test_more_than_2_to_30_rows_widen_the_window(ch, ctx, big, hint):
    k, v, kcol, vcol = big
    A = ch.Aggregator(np.uint32, [(ch.AGG_SUM, np.float64), (ch.AGG_AVG, np.float64)], size_hint=hint, ctx=ctx)
    for _ in range(BIG_TIMES):
        A.execute_on_block(kcol, [vcol, vcol])
    gk, (s, a) = _result(A)
    want = R.big_expectation(k, v, BIG_TIMES)
    assert gk.tolist() == sorted(R.BIG_KEYS)
    _same(s, [want[key] for key in gk.tolist()], hint)
    _same(a, [want[key] / (int((k == key).sum()) * BIG_TIMES) for key in gk.tolist()], (hint, "avg"))


def test_a_merge_that_passes_2_to_30_rows_widens_both_windows(ch, ctx, big):
    k, v, kcol, vcol = big
    want = R.big_expectation(k, v, BIG_TIMES)
    for flip in (False, True):
        full = ch.Aggregator(np.uint32, [(ch.AGG_SUM, np.float64)], size_hint=16, ctx=ctx)
        one = ch.Aggregator(np.uint32, [(ch.AGG_SUM, np.float64)], size_hint=16, ctx=ctx)
        for _ in range(BIG_TIMES - 1):
            full.execute_on_block(kcol, [vcol])                                          # exactly 2^30 rows: the window has not moved yet
        one.execute_on_block(kcol, [vcol])
        dst, src = (one, full) if flip else (full, one)
        dst.merge(src)
        gk, (s,) = _result(dst)
        assert gk.tolist() == sorted(R.BIG_KEYS)
        _same(s, [want[key] for key in gk.tolist()], flip)
