"""The model of the fixed-point Float64 sums (tests/fx_sum_ref.py) pinned on hand-written cases, against math.fsum and Fraction, and every
input generator of tests/test_gpu_float_sum_edges.py checked for the property the GPU test relies on.  No GPU."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import fx_sum_ref as R  # noqa: E402


def _model_sums(keys, values, base):
    out = {}
    for k, v in zip(keys.tolist(), values.tolist()):
        out[k] = out.get(k, 0) + R.units(v, base)
    return out


# ---- the model itself --------------------------------------------------------------------------------------------------------------------
def test_expo_units_fold_and_widen_on_hand_written_values():
    assert [R.expo(x) for x in (1.0, 1.5, -2.0, 0.75, 2.0 ** -1022, 2.0 ** -1023, 2.0 ** -1074, 1.7e308)] == [0, 0, 1, -1, -1022, -1022, -1022, 1023]
    assert R.units(1.0, -96) == 1 << 96 and R.units(-1.0, -96) == -(1 << 96)
    assert R.units(3.75, 0) == 3 and R.units(-3.75, 0) == -3                                  # toward zero
    assert R.units(2.0 ** -97, -96) == 0 and R.units(-(2.0 ** -97), -96) == 0
    assert R.fold((1 << 53) + 1, 0) == 2.0 ** 53 and R.fold((1 << 53) + 3, 0) == 2.0 ** 53 + 4  # ties to even
    assert R.fold(-((1 << 53) + 1), 0) == -(2.0 ** 53) and R.fold(((1 << 53) + 1) << 70 | 1, -70) == 2.0 ** 53 + 2
    assert R.fold(3, -1074) == 3 * 2.0 ** -1074 and R.fold(1 << 1024, 0) == math.inf and R.fold(-(1 << 1024), 0) == -math.inf
    assert R.widen(5, 1) == 2 and R.widen(-5, 1) == -3 and R.widen(-1, 64) == -1 and R.widen(-(1 << 70), 70) == -1 and R.widen((1 << 70) - 1, 70) == 0


def test_window_follows_the_largest_exponent_the_rows_and_the_spread():
    assert R.window([1.0, -3.0, 0.0]) == (1 - 96, False)
    assert R.window([0.0, -0.0]) == (None, False)
    assert R.window([1.0], rows=1 << 30) == (-96, False) and R.window([1.0], rows=(1 << 30) + 1) == (-88, False)
    assert R.window([1.0], rows=1 << 38) == (-88, False) and R.window([1.0], rows=(1 << 38) + 1) == (-80, False)
    assert R.window([1.0, 2.0 ** -73]) == (-96, False) and R.window([1.0, 2.0 ** -74]) == (-96, True)
    assert R.window([1.0, 2.0 ** -66], rows=(1 << 30) + 1) == (-88, True)                        # a row step costs 8 bits of spread
    assert R.window([2.0 ** -1074, 2.0 ** -1030]) == (-1022 - 96, False)


def test_low_word_wraps_counts_carries_and_borrows():
    hi_bit = 2.0 ** 63
    assert R.low_word_wraps([hi_bit, hi_bit, hi_bit, hi_bit], 0) == 2
    assert R.low_word_wraps([1.0, -1.0, -1.0, 1.0], 0) == 2             # 1 + (2^64 - 1) wraps, (2^64 - 1) + 1 wraps
    assert R.low_word_wraps([2.0 ** 64, 2.0 ** 70], 0) == 0             # nothing in the low word


def test_model_against_fsum_and_fraction_on_random_values_inside_the_window():
    r = R.rng("model")
    v = (r.integers(-(1 << 40), 1 << 40, size=5000).astype(np.float64)) * 2.0 ** r.integers(-30, 4, size=5000)      # within 2^44 of 2^43
    base, leaves = R.window(v.tolist())
    assert not leaves and R.all_multiples(v, base)
    u = sum(R.units(x, base) for x in v.tolist())
    assert Fraction(u) * Fraction(2) ** base == sum(Fraction(x) for x in v.tolist())
    assert R.fold(u, base) == math.fsum(v.tolist())


def test_model_blocks_merges_and_doubles():
    a = R.Model()
    tiny = (1 + 2.0 ** -40) * 2.0 ** -60                                               # 2^35 + 2^-5 units of 2^-95
    a.add_block([1, 1, 2], [1.0, tiny, -3.0])
    assert (a.base, a.state[1]) == (-95, (1 << 95) + (1 << 35)) and a.result()[2] == -3.0      # the 2^-5 is cut
    a.add_block([1, 2], [2.0 ** 10, -tiny])                                            # the window moves up by 9: floor of every state
    assert a.base == -86 and a.state[1] == (1 << 86) + (1 << 26) + (1 << 96) and a.state[2] == (-3 << 86) - (1 << 26)
    b = R.Model()
    b.add_block([2, 3], [2.0 ** -50, 2.0 ** -40])
    b2 = R.Model()
    b2.add_block([2, 3], [2.0 ** -50, 2.0 ** -40])
    a2 = R.Model()
    a2.add_block([1, 1, 2], [1.0, tiny, -3.0])
    a2.add_block([1, 2], [2.0 ** 10, -tiny])
    assert b.base == -136
    a.merge(b)
    b2.merge(a2)
    assert a.base == b2.base == -86 and a.state == b2.state and a.result()[3] == 2.0 ** -40
    assert a.state[2] == (-3 << 86) - (1 << 26) + (1 << 36) and a.rows == b2.rows == 7
    c = R.Model()
    c.add_block([1, 1], [1.0, 2.0 ** -80])
    c.add_block([1], [2.0 ** 30])                                                      # spread 110: the sums become doubles
    assert not c.fixed and c.result()[1] == (1.0 + 2.0 ** -80) + 2.0 ** 30


# ---- 2a ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan,mant_bits", [(p, 53) for p in R.PLAN_SHAPES] + [(p, 24) for p in R.FLOAT32_PLANS])
def test_carry_mix_is_exact_in_its_window_and_wraps_the_low_word(plan, mant_bits):
    kd, rows, groups, _, _, _ = R.PLAN_SHAPES[plan]
    k, v, kind, exact = R.carry_input(plan, mant_bits)
    uk, order, starts, counts = R.group_rows(k)
    assert uk[0] == 0 and uk[-1] == np.iinfo(kd).max
    if mant_bits == 24:
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)                      # every value is a Float32
    base, leaves = R.window([v.max(), np.abs(v[v != 0]).min()], rows)
    assert base == R.CARRY_E - 96 and not leaves
    # no truncation: with every value a whole number of units the model's sum is the exact sum, and fold is fsum's rounding
    assert R.all_multiples(v, base)
    # the three tiers
    e = np.frexp(np.abs(v[v != 0]))[1] - 1
    assert set(np.unique(e).tolist()) == {R.CARRY_E, R.CARRY_E - 33, R.CARRY_E - 44} and (e == R.CARRY_E).sum() == 4
    assert (e == R.CARRY_E - 33).mean() > 0.9 and (e == R.CARRY_E - 44).sum() > rows // 64
    # the crafted groups have the sums they are built for, every kind is there, the zero key and the all-ones key are among the groups
    _, us, _ = R.unit_sums(k, v, base)
    sums = R.fold_many(us, base)
    for kd_, want in exact.items():
        assert (kind == kd_).sum() >= 8 and np.all(sums[kind == kd_] == want), (plan, kd_)
    assert (kind == R.KIND_MIXED).sum() >= 10 and np.count_nonzero(sums[kind == R.KIND_MIXED]) > 0.9 * (kind == R.KIND_MIXED).sum()
    # the model, in Python integers, on the smaller shapes (the larger ones are the same construction: their sums are unit_sums' integers above)
    if rows <= 200_000:
        ms = _model_sums(k, v, base)
        assert [ms[int(key)] for key in uk] == us                                               # the scalar model and the limbs agree
        assert [R.fold(u, base) if u else 0.0 for u in us] == sums.tolist() == R.fsum_groups(k, v)[1].tolist()
        lo = ((np.ldexp(np.abs(v), -base) % 2.0 ** 64).astype(np.uint64))                     # |units| mod 2^64, exact: 21 or 53 bits
        lo = np.where(v < 0, (~lo) + np.uint64(1), lo)
        # row-order wraps per group: a wrap is a running low word that got smaller
        wraps = np.zeros(uk.shape[0], dtype=np.int64)
        los = lo[order]
        for g in np.flatnonzero(counts >= 100).tolist():
            seg = los[starts[g]:starts[g] + counts[g]]
            run = np.cumsum(seg, dtype=np.uint64)
            wraps[g] = int((run[1:] < run[:-1])[seg[1:] != 0].sum())
        g0 = int(np.flatnonzero(counts >= 100)[0]) if (counts >= 100).any() else None
        if g0 is not None:
            assert wraps[g0] == R.low_word_wraps(v[order][starts[g0]:starts[g0] + counts[g0]].tolist(), base)
        if plan == "ranged":
            # x and -x wrap once between them, so a group wraps about once in two rows: the six groups in ten that share nine rows in
            # ten have 300 rows each.  (The other plans need more groups than rows / 100: there the same values wrap at the same rate,
            # asserted above as the bulk's share of the rows.)
            assert (wraps >= 100).sum() * 2 >= uk.shape[0], (wraps >= 100).mean()
            assert wraps.sum() >= 0.4 * counts[counts >= 100].sum()


# ---- 2b ----------------------------------------------------------------------------------------------------------------------------------
def test_fold_cases_are_exact_in_their_windows_and_round_as_named():
    cases = R.fold_cases()
    assert len(cases) == 6 * 2 * 3 + 5
    for name, vals in cases.items():
        base, leaves = R.window(vals)
        assert not leaves and all(R.units(x, base) * Fraction(2) ** base == Fraction(x) for x in vals), name
        got = R.fold(sum(R.units(x, base) for x in vals), base)
        if "the_top" not in name:                                                      # (fsum overflows on its way there)
            assert got == math.fsum(vals), name
    T = 2.0 ** 53
    for k in (-1000, 0, 900):
        for tag, s in (("pos", 1.0), ("neg", -1.0)):
            want = {"tie_to_even_down": T, "tie_to_even_up": T + 4, "above_half": T + 2, "below_half": T, "above_half_odd": T + 4, "below_half_odd": T + 2}
            for name, w in want.items():
                assert math.fsum(cases[f"{name}-{tag}-2^{k}"]) == math.ldexp(s * w, k), (name, tag, k)
    sub = 2.0 ** -1074
    assert math.fsum(cases["subnormals_stay_subnormal"]) == (2 ** 51 + 2) * sub < 2.0 ** -1022
    assert math.fsum(cases["subnormals_become_normal"]) == 2.0 ** -1021 and math.fsum(cases["subnormals_cancel_to_one"]) == sub
    base, _ = R.window(cases["near_the_top"])
    assert base == 1023 - 96 and R.fold(sum(R.units(x, base) for x in cases["near_the_top"]), base) == 1.7e308
    base, _ = R.window(cases["over_the_top"])
    assert R.fold(sum(R.units(x, base) for x in cases["over_the_top"]), base) == math.inf
    with np.errstate(over="ignore"):
        assert float(np.sum(np.array(cases["over_the_top"]))) == math.inf                  # as a double sum in row order gives


def test_spans_both_words_cases_drop_65_bits_and_land_on_both_sides_of_the_half():
    want = {"tie_even": 2.0 ** 52, "tie_odd": 2.0 ** 52 + 2, "half_plus_one_unit": 2.0 ** 52 + 1, "half_minus_one_unit": 2.0 ** 52,
            "neg_tie_odd": -(2.0 ** 52 + 2), "neg_half_plus_one_unit": -(2.0 ** 52 + 1)}
    cases = R.spans_both_words_cases()
    assert set(cases) == set(want)
    for name, (n, big, small) in cases.items():
        base, leaves = R.window([big] + small, n + len(small))
        assert base == 10 - 96 and not leaves, name
        u = n * R.units(big, base) + sum(R.units(x, base) for x in small)
        assert all(R.units(x, base) * Fraction(2) ** base == Fraction(x) for x in small), name
        assert abs(u).bit_length() - 1 == 117, name                                        # 65 bits are dropped: bit 64 is the half
        assert ("tie" in name) == (abs(u) % (1 << 65) == 1 << 64), name                    # off a tie by one unit of the low word
        assert R.fold(u, base) == want[name] * 2.0 ** (10 - 96 + 65), name


def test_beyond_the_window_truncates_and_differs_from_fsum():
    vals = R.beyond_the_window()
    base, leaves = R.window(vals)
    assert base == 30 - 96 and not leaves
    u = sum(R.units(x, base) for x in vals)
    assert u == 1001 * ((1 << 52) - 1)                                                 # each copy is 2^52 - 1/2 units: the half is cut
    assert R.fold(u, base) != math.fsum(vals) and abs(R.fold(u, base) - math.fsum(vals)) <= 1001 * 2.0 ** base


def test_spread_73_stays_exact_and_74_leaves_fixed_point():
    k, v = R.spread_block(73)
    base, leaves = R.window(v.tolist())
    assert base == 20 - 96 and not leaves and R.all_multiples(v, base)
    e = np.frexp(np.abs(v))[1] - 1
    assert e.max() - e.min() == 73
    ms = _model_sums(k, v, base)
    uk, sums, _ = R.fsum_groups(k, v)
    assert [R.fold(ms[int(key)], base) for key in uk] == sums.tolist()
    k, v = R.spread_block(74)
    e = np.frexp(np.abs(v))[1] - 1
    assert e.max() - e.min() == 74 and R.window(v.tolist())[1]


# ---- 2e ----------------------------------------------------------------------------------------------------------------------------------
def test_masked_mix_is_exact_only_in_the_window_of_its_kept_rows():
    k, v, keep = R.masked_mix()
    kept = v[keep == 1]
    base, leaves = R.window([np.abs(kept).max(), np.abs(kept[kept != 0]).min()], v.shape[0])
    assert (base, leaves) == (R.CARRY_E - 33 - 96, False) and R.all_multiples(kept, base)
    assert 0.4 < keep.mean() < 0.6 and np.abs(v[keep == 0]).max() == 1.5 * 2.0 ** R.CARRY_E and (np.abs(v[keep == 0]) >= 2.0 ** R.CARRY_E).sum() == 4
    e = np.frexp(np.abs(kept[kept != 0]))[1] - 1
    assert e.max() - e.min() == 73 and (e == R.FINE_E).sum() > 1000
    # in the window of all rows the fine values would be cut to nothing
    assert not R.all_multiples(kept, R.CARRY_E - 96) and all(R.units(x, R.CARRY_E - 96) == 0 for x in kept[e.argmin():][:1].tolist())
    uk, us, _ = R.unit_sums(k, np.where(keep == 1, v, 0.0), base)
    assert R.fold_many(us, base).tolist() == R.fsum_groups(k, np.where(keep == 1, v, 0.0))[1].tolist()


# ---- 2c, 2d ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh", R.SHIFTS)
def test_two_scale_blocks_shift_without_a_remainder(sh):
    k1, v1, k2, v2 = R.two_scale_blocks(sh)
    b1, l1 = R.window(v1.tolist())
    b2, l2 = R.window(np.concatenate([v1, v2]).tolist())
    assert (b1, b2 - b1, l1, l2) == (-7 - 96, sh, False, False)
    s1 = _model_sums(k1, v1, b1)
    assert all(u % (1 << sh) == 0 for u in s1.values())                                # remainder 0: the widening loses nothing
    assert sum(1 for u in s1.values() if u < 0) >= 10 and sum(1 for u in s1.values() if u > 0) >= 5
    assert R.all_multiples(v1, b2) and R.all_multiples(v2, b2)
    m = R.Model()
    m.add_block(k1, v1)
    m.add_block(k2, v2)
    uk, sums, _ = R.fsum_groups(np.concatenate([k1, k2]), np.concatenate([v1, v2]))
    assert [m.result()[int(key)] for key in uk] == sums.tolist()
    # some groups keep their shifted block-1 state alone, negative ones among them
    alone = set(k1.tolist()) - set(k2[v2 != 0].tolist())
    assert any(s1[g] < 0 for g in alone)
    # the same through a merge, in both directions
    for flip in (False, True):
        a, b = R.Model(), R.Model()
        a.add_block(k1, v1)
        b.add_block(k2, v2)
        dst, src = (b, a) if flip else (a, b)
        dst.merge(src)
        assert [dst.result()[int(key)] for key in uk] == sums.tolist()


def test_two_scale_blocks_that_are_no_multiples_floor_and_differ_from_fsum():
    k1, v1, k2, v2 = R.two_scale_blocks(50, exact=False)
    b1 = R.window(v1.tolist())[0]
    s1 = _model_sums(k1, v1, b1)
    assert any(u % (1 << 50) for u in s1.values())
    m = R.Model()
    m.add_block(k1, v1)
    m.add_block(k2, v2)
    uk, sums, _ = R.fsum_groups(np.concatenate([k1, k2]), np.concatenate([v1, v2]))
    got = [m.result()[int(key)] for key in uk]
    assert got != sums.tolist() and np.allclose(got, sums, rtol=1e-12)
    # floor, not truncation: a net negative state with a remainder moves away from zero
    assert any(u < 0 and u % (1 << 50) for u in s1.values())


# ---- 2f ----------------------------------------------------------------------------------------------------------------------------------
def test_big_block_overflows_128_bits_without_the_row_step():
    rows, times = 1 << 22, 257
    k, v = R.big_block(rows)
    assert rows * times == (1 << 30) + (1 << 22) and rows * 256 == 1 << 30
    n_dom = int((k == R.BIG_KEYS[0]).sum())
    assert n_dom == rows - 64 - 1024 and int((k == R.BIG_KEYS[1]).sum()) == 64
    narrow = R.window(np.unique(v).tolist(), rows)[0]
    wide, leaves = R.window(np.unique(v).tolist(), rows * times)
    assert (narrow, wide, leaves) == (-96, -88, False)
    # without the widening the dominant state passes 2^127: the sign bit of the pair
    assert n_dom * times * R.units(R.BIG_X, narrow) >= 1 << 127 > n_dom * 256 * R.units(R.BIG_X, narrow)
    assert n_dom * times * R.units(R.BIG_X, wide) < 1 << 127
    # every value is a whole number of units of the wide window too: the widening and the later rows lose nothing
    assert R.all_multiples(v, wide)
    small = np.abs(v[k == R.BIG_KEYS[2]])
    assert small.shape[0] == 1024 and small.min() >= 2.0 ** -60 and small.max() < 2.0 ** -59
    want = R.big_expectation(k, v, times)
    assert want[R.BIG_KEYS[0]] == float(Fraction(R.BIG_X) * n_dom * times) and want[R.BIG_KEYS[1]] == -R.BIG_X * 64 * times
    assert want[R.BIG_KEYS[2]] == math.fsum(v[k == R.BIG_KEYS[2]].tolist() * times)
    # and the product is no double by accident: the fold rounds
    assert Fraction(want[R.BIG_KEYS[0]]) != Fraction(R.BIG_X) * n_dom * times
