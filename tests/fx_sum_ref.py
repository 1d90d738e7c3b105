"""A plain model of the fixed-point Float64 sums of GROUP BY, in Python integers and fractions.Fraction, and the inputs
that tests/test_gpu_float_sum_edges.py feeds to the device.  Written from the contract, not from the kernels:

  * a state is an integer number of units of 2^base; a row adds trunc(x * 2^-base) (toward zero);
  * base = Emax - 96, Emax the largest unbiased exponent seen (a subnormal counts as -1022); the window holds 2^30 rows and moves up by
    8 for every step by which the row count outgrows it (2^30, 2^38, ...); it never moves down;
  * a move of the window by sh is a floor division of every state by 2^sh;
  * the result is the state times 2^base rounded once, to nearest, ties to even;
  * when the smallest non-zero value would keep fewer than 24 bits (Emin - 23 < base: Emax - Emin > 73 before any row step) the sums
    leave fixed point and are double adds from there on.

tests/test_fx_sum_ref.py pins the model on hand-written cases and asserts, for every generator below, the property the GPU test relies on."""
import functools
import math
from fractions import Fraction

import numpy as np

WINDOW_BITS = 96      # base = Emax - WINDOW_BITS
MIN_BITS = 24         # every value keeps at least this many bits, or the sums leave fixed point
ROW_CAP_LOG2 = 30     # rows the window holds before it moves up by ROW_STEP
ROW_STEP = 8
WORD = 1 << 64


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def expo(x):
    """the unbiased exponent of a non-zero finite double; a subnormal counts as -1022"""
    m, e = math.frexp(abs(float(x)))
    assert m != 0.0 and math.isfinite(m)
    return max(e - 1, -1022)


def units(x, base):
    """trunc(x * 2^-base), toward zero"""
    return int(Fraction(float(x)) / Fraction(2) ** base)     # int() of a Fraction truncates toward zero


def fold(u, base):
    """the state as a double: one rounding, to nearest, ties to even (float(Fraction)); beyond the largest double: +-inf"""
    try:
        return float(Fraction(u) * Fraction(2) ** base)
    except OverflowError:
        return math.inf if u > 0 else -math.inf


def row_steps(rows):
    steps = 0
    while ROW_CAP_LOG2 + ROW_STEP * steps < 62 and rows > 1 << (ROW_CAP_LOG2 + ROW_STEP * steps):
        steps += 1
    return steps


def window(values, rows=None):
    """(base, leaves) of a fresh aggregation that has seen `values` in `rows` rows (default: one row per value); base None = zeros only"""
    nz = [expo(v) for v in values if v != 0]
    rows = len(values) if rows is None else rows
    if not nz:
        return None, False
    base = max(nz) - WINDOW_BITS + ROW_STEP * row_steps(rows)
    return base, min(nz) - (MIN_BITS - 1) < base


def widen(state_units, sh):
    """the state in units 2^sh times as large: floor"""
    return state_units >> sh         # Python's >> on int is an arithmetic shift: floor division by 2^sh


def low_word_wraps(values, base):
    """how often the low 64-bit word of the pair wraps when `values` are added in row order (two's complement: a negative value adds
    2^64 - (m mod 2^64) to the low word)"""
    lo = wraps = 0
    for v in values:
        lo += units(v, base) % WORD
        if lo >= WORD:
            lo -= WORD
            wraps += 1
    return wraps


class Model:
    """One aggregation's Float64 sum states, keyed: blocks, merges, and states leaving and arriving as doubles."""

    def __init__(self):
        self.base, self.steps, self.rows, self.emin, self.fixed = None, 0, 0, None, True
        self.state = {}          # key -> units (fixed) or double (after leaving fixed point)

    def _admit(self, nz_expos, rows):
        """the window before `rows` more rows whose non-zero values have these exponents are added; False: fixed point is left"""
        self.rows += rows
        if not nz_expos:
            return True
        steps = max(self.steps, row_steps(self.rows))
        base = max(nz_expos) - WINDOW_BITS + ROW_STEP * steps
        if self.base is not None:
            base = max(base, self.base + ROW_STEP * (steps - self.steps))
        emin = min(nz_expos) if self.emin is None else min(self.emin, min(nz_expos))
        if emin - (MIN_BITS - 1) < base:
            self.leave()
            return False
        if self.base is not None and base > self.base:
            self.state = {k: widen(u, base - self.base) for k, u in self.state.items()}
        self.base, self.steps, self.emin = base, steps, emin
        return True

    def leave(self):
        if self.fixed:
            self.state = {k: fold(u, self.base) for k, u in self.state.items()}
            self.fixed = False

    def add_block(self, keys, values):
        values = [float(v) for v in values]
        if self.fixed:
            self._admit([expo(v) for v in values if v != 0], len(values))
        for k, v in zip(keys, values):
            k = int(k)
            if self.fixed:
                self.state[k] = self.state.get(k, 0) + (units(v, self.base) if v != 0 else 0)
            else:
                self.state[k] = self.state.get(k, 0.0) + v         # (row order: the hardware's order is not modelled)

    def merge(self, other):
        """other's states are added to this aggregation's, in the coarser of the two windows"""
        assert self.fixed and other.fixed, "the model merges fixed-point states only"
        if other.base is None:
            self.rows += other.rows
            for k in other.state:
                self.state.setdefault(k, 0)
            return
        if self.base is None:
            self.base, self.steps, self.emin = other.base, other.steps, other.emin
            self.rows += other.rows
            for k, u in other.state.items():
                self.state[k] = self.state.get(k, 0) + u
            return
        rows = self.rows + other.rows
        steps = max(self.steps, other.steps, row_steps(rows))
        base = max(self.base + ROW_STEP * (steps - self.steps), other.base + ROW_STEP * (steps - other.steps))
        assert min(self.emin, other.emin) - (MIN_BITS - 1) >= base, "the model merges inside one window only"
        self.state = {k: widen(u, base - self.base) for k, u in self.state.items()}
        for k, u in other.state.items():
            self.state[k] = self.state.get(k, 0) + widen(u, base - other.base)
        self.base, self.steps, self.rows, self.emin = base, steps, rows, min(self.emin, other.emin)

    def merge_doubles(self, keys, doubles):
        """states that arrive as a Float64 column: each is one value in one row"""
        self.add_block(keys, doubles)

    def result(self):
        """key -> double"""
        return {k: (fold(u, self.base) if u else 0.0) if self.fixed else u for k, u in self.state.items()}


# ---- helpers of the tests --------------------------------------------------------------------------------------------------------------
def rng(*seed):
    return np.random.Generator(np.random.PCG64([ord(c) for c in "-".join(map(str, seed))]))


def group_rows(keys):
    """(unique keys ascending, row order that sorts by key (stable), start of each group in that order, rows per group)"""
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    starts = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))
    counts = np.diff(np.concatenate([starts, [keys.shape[0]]]))
    return sk[starts], order, starts, counts


def fsum_groups(keys, values):
    """(unique keys ascending, math.fsum per group as float64, rows per group)"""
    uk, order, starts, counts = group_rows(keys)
    v = np.asarray(values, dtype=np.float64)[order]
    ends = starts + counts
    return uk, np.array([math.fsum(v[a:b]) for a, b in zip(starts.tolist(), ends.tolist())]), counts


def unit_sums(keys, values, base):
    """(unique keys ascending, [sum of units(x, base) per group as Python integers], rows per group) for values that are whole numbers of
    units (all_multiples): the model's state, computed in two integer limbs of 48 bits so that a block of millions of rows takes no
    Python loop over its rows.  Holds for |x| < 2^98 units and fewer than 2^13 rows a group."""
    uk, order, starts, counts = group_rows(keys)
    assert counts.max() < 1 << 13
    q = np.ldexp(np.asarray(values, dtype=np.float64)[order], -base)
    assert np.all(q == np.trunc(q)) and np.all(np.abs(q) < 2.0 ** 98)
    hi = np.floor(q * 2.0 ** -48)
    lo = q - hi * 2.0 ** 48                                     # in [0, 2^48), exact: both are whole numbers with 53 bits
    hs = np.add.reduceat(hi.astype(np.int64), starts).tolist()
    ls = np.add.reduceat(lo.astype(np.int64), starts).tolist()
    return uk, [(h << 48) + l for h, l in zip(hs, ls)], counts


def fold_many(us, base):
    """fold() of a list of states, as a float64 array (float(int) rounds to nearest, ties to even; the scaling is exact away from the
    subnormals, where fold itself is used)"""
    return np.array([0.0 if u == 0 else math.ldexp(float(u), base) if base + abs(u).bit_length() > -960 and base + abs(u).bit_length() < 1000
                     else fold(u, base) for u in us])


def all_multiples(values, base):
    """every value is a whole number of units of 2^base (scaling by a power of two is exact: values stay far from the ends of the range)"""
    s = np.ldexp(np.asarray(values, dtype=np.float64), -base)
    return bool(np.all(np.isfinite(s)) and np.all(s == np.trunc(s)))


def keys_with_edges(kd, rows, groups, seed, skewed=False):
    """`rows` keys over about `groups` distinct values, the zero key and the all-ones key among them, every key present"""
    r = rng("keys", seed, np.dtype(kd).name, rows, groups)
    top = np.iinfo(kd).max
    if groups >= top:
        uk = np.arange(int(top) + 1, dtype=np.uint64)
    else:
        uk = np.unique(np.concatenate([r.integers(1, top, size=groups, dtype=np.uint64), np.array([0, top], dtype=np.uint64)]))
    heavy = uk.shape[0] * 6 // 10
    if skewed:                                                  # six groups in ten share nine rows in ten
        idx = np.where(r.random(rows) < 0.9, r.integers(0, heavy, size=rows), r.integers(heavy, uk.shape[0], size=rows))
    else:
        idx = r.integers(0, uk.shape[0], size=rows)
    k = r.permutation(uk)[idx]
    k[:uk.shape[0]] = r.permutation(uk)
    return k.astype(kd)


# ---- 2a: the carry and borrow mix ------------------------------------------------------------------------------------------------------
CARRY_E = 40          # the anchors' exponent: Emax of the block; base = CARRY_E - 96
KIND_ZERO, KIND_PLUS_WORD, KIND_MINUS_WORD, KIND_ALL_ONES, KIND_MIXED = 0, 1, 2, 3, 4


def carry_mix(keys, mant_bits=53, seed=0, E=CARRY_E):
    """-> (values as float64, kind per group in ascending key order, the exact sum each crafted kind must have).

    Three tiers in one block whose window is base = E - 96:
      anchors  +-1.5 * 2^E in four rows (they set Emax);
      bulk     +-(2^20 + r) * 2^(E - 53), r of 20 random bits: exponent E - 33, so a positive value is m * 2^43 units with unit bit 63
               set and a negative one has the low word 2^64 - m * 2^43: nearly every add wraps the low word;
      sprinkle +-(2^mant_bits - 1) * 2^(E - 43 - mant_bits): exponent E - 44 with every mantissa bit set, the last exact binade
               (mant_bits 24: the value is a Float32).
    Group g (ascending key order) is of kind g % 8 when it has the rows for it (at least 4), else mixed:
      0  bulk x, -x pairs: sum 0                                  1  pairs + {a, b, -c} with a + b - c = +2^(E - 32), the word boundary
      2  pairs + {-a, -b, c}: sum -2^(E - 32)                     3  pairs + {s - 2^(E - 60), -s}: sum -2^(E - 60), high word all ones
      4..7  mixed: bulk of random sign, one row in 16 from the sprinkle; the anchors go to four such rows of three such groups."""
    r = rng("carry", seed, mant_bits, keys.shape[0])
    n = keys.shape[0]
    uk, order, starts, counts = group_rows(keys)
    G = uk.shape[0]
    kind = np.where(counts >= 4, np.arange(G) % 8, KIND_MIXED)
    kind[kind > KIND_MIXED] = KIND_MIXED
    gid = np.repeat(np.arange(G), counts)                      # per sorted row
    pos = np.arange(n) - np.repeat(starts, counts)
    cnt = np.repeat(counts, counts)
    rkind = kind[gid]
    bulk_unit = 2.0 ** (E - 53)
    mant = (r.integers(0, 1 << 20, size=n) + (1 << 20)).astype(np.float64)
    sign = r.choice(np.array([-1.0, 1.0]), size=n)
    sprinkle = (2.0 ** mant_bits - 1.0) * 2.0 ** (E - 43 - mant_bits)
    v = np.where(r.random(n) < 1.0 / 16, sprinkle, mant * bulk_unit) * sign                 # mixed rows
    # crafted groups: the last `tail` rows are the remainder, the rows before them pairs (an odd row out is 0.0)
    tail = np.array([0, 3, 3, 2, 0])[rkind]
    crafted = rkind != KIND_MIXED
    body = cnt - tail
    in_pair = crafted & (pos < body - (body & 1))
    first = np.arange(n) - (pos & 1)                            # the pair's first row, in sorted order
    v[in_pair] = (mant[first] * bulk_unit * np.where(pos & 1, -1.0, 1.0))[in_pair]
    v[crafted & (pos == body - 1) & ((body & 1) == 1)] = 0.0
    t = pos - body                                              # 0.. within the tail
    # a + b - c = 2^21 bulk units with all three in [2^20, 2^21): a, b in [3 * 2^19, 2^21) gives c = a + b - 2^21 in [2^20, 2^21)
    a = r.integers(3 << 19, 1 << 21, size=n).astype(np.float64)
    b = r.integers(3 << 19, 1 << 21, size=n).astype(np.float64)
    ga, gb = a[np.arange(n) - np.maximum(t, 0)], b[np.arange(n) - np.maximum(t, 0)]         # the tail's first row holds its a and b
    for k, s in ((KIND_PLUS_WORD, 1.0), (KIND_MINUS_WORD, -1.0)):
        sel = crafted & (rkind == k) & (t >= 0)
        tri = np.where(t == 0, ga, np.where(t == 1, gb, -(ga + gb - float(1 << 21)))) * bulk_unit * s
        v[sel] = tri[sel]
    sel = (rkind == KIND_ALL_ONES) & (t >= 0)
    v[sel] = np.where(t == 0, sprinkle - 2.0 ** (E - 60), -sprinkle)[sel]
    # anchors: +A and -A alone in two mixed groups, and a +A, -A pair in a third
    mixed_groups = np.flatnonzero((kind == KIND_MIXED) & (counts >= 2))[:3]
    assert mixed_groups.shape[0] == 3
    A = 1.5 * 2.0 ** E
    v[starts[mixed_groups[0]]] = A
    v[starts[mixed_groups[1]]] = -A
    v[starts[mixed_groups[2]]], v[starts[mixed_groups[2]] + 1] = A, -A
    out = np.empty(n, dtype=np.float64)
    out[order] = v
    exact = {KIND_ZERO: 0.0, KIND_PLUS_WORD: 2.0 ** (E - 32), KIND_MINUS_WORD: -2.0 ** (E - 32), KIND_ALL_ONES: -2.0 ** (E - 60)}
    return out, kind, exact


# the plans of 2a at the smallest shape that still selects each: (key dtype, rows, groups, size hint, options, plan words of the debug line)
PLAN_SHAPES = {
    "ranged": (np.uint32, 200_000, 1000, 1000, {}, ("ranged GROUP BY",)),
    "rows_lds": (np.uint16, 200_000, 30_000, 30_000, {"tune_agg_no_ranged": 1}, ("direct GROUP BY", "kernel=rows_lds")),
    "rows_direct": (np.uint64, 100_000, 70_000, 1_000_000, {}, ("direct GROUP BY", "kernel=rows_direct")),
    "tile_sorted": (np.uint64, (4 << 20) + 77, 1 << 19, 1 << 19, {}, ("tile-sorted GROUP BY",)),
    "scatter": (np.uint32, (4 << 20) + 77, 1 << 19, 1 << 19, {"tune_gb_no_tiled": 1}, ("partitioned GROUP BY",)),
    # max(Float64) beside the sum: rows take the kernel that adds to the table in HBM, 3000 rows to a cell
    "contended": (np.uint32, 200_000, 64, 64, {}, ("direct GROUP BY", "kernel=rows_direct", "states=extremum")),
}
FLOAT32_PLANS = ("ranged", "rows_lds", "rows_direct")          # the Float32 mix runs at the three small shapes


@functools.lru_cache(maxsize=None)
def carry_input(plan, mant_bits=53):
    """(keys, values, kind per group, exact sums of the crafted kinds) of one plan's shape, read-only; the ranged shape's keys are skewed
    so that most groups have 300 rows"""
    kd, rows, groups = PLAN_SHAPES[plan][:3]
    k = keys_with_edges(kd, rows, groups, plan, skewed=plan == "ranged")
    v, kind, exact = carry_mix(k, mant_bits)
    k.setflags(write=False)
    v.setflags(write=False)
    return k, v, kind, exact


@functools.lru_cache(maxsize=None)
def carry_expect(plan, mant_bits=53):
    """(unique keys ascending, the model's sum per group as float64, rows per group) of carry_input: computed once, read-only"""
    k, v, _, _ = carry_input(plan, mant_bits)
    uk, us, counts = unit_sums(k, v, CARRY_E - WINDOW_BITS)
    sums = fold_many(us, CARRY_E - WINDOW_BITS)
    sums.setflags(write=False)
    return uk, sums, counts


# ---- 2e: the mix under a condition -------------------------------------------------------------------------------------------------------
FINE_E = CARRY_E - 33 - 73      # the smallest exponent the window of the kept rows admits


@functools.lru_cache(maxsize=None)
def masked_mix():
    """(keys, values, keep): the ranged shape's mix with the anchors and half of the rest masked out (keep 0), and one kept row in 64
    replaced by a 24-bit value at exponent FINE_E.  The kept rows' window is base = (CARRY_E - 33) - 96: every kept value is a whole
    number of its units, while the window of all rows (CARRY_E - 96) would cut the fine values to nothing."""
    k, v, _, _ = carry_input("ranged")
    r = rng("masked")
    n = v.shape[0]
    keep = (r.random(n) < 0.5).astype(np.uint8)
    keep[np.abs(v) >= 2.0 ** CARRY_E] = 0
    v = v.copy()
    fine = np.flatnonzero((keep == 1) & (r.random(n) < 1.0 / 64))
    v[fine] = (r.integers(0, 1 << 23, size=fine.shape[0]) + (1 << 23)).astype(np.float64) * 2.0 ** (FINE_E - 23) * r.choice(np.array([-1.0, 1.0]), size=fine.shape[0])
    v.setflags(write=False)
    keep.setflags(write=False)
    return k, v, keep


# ---- 2b: rounding at the fold ------------------------------------------------------------------------------------------------------------
def fold_cases():
    """name -> list of values of one group; every value is a whole number of units of its window, so the exact sum is the model's"""
    T = 2.0 ** 52
    base_sets = {
        "tie_to_even_down": [T + 1, T],                                  # 2^53 + 1 -> 2^53
        "tie_to_even_up": [T + 1, T + 2],                                # 2^53 + 3 -> 2^53 + 4
        "above_half": [T + 1, T, 2.0 ** -20, 2.0 ** -21],                # 2^53 + 1 + eps -> 2^53 + 2
        "below_half": [T + 1, T, -2.0 ** -20, -2.0 ** -21],              # 2^53 + 1 - eps -> 2^53
        "above_half_odd": [T + 1, T + 2, 2.0 ** -21, 2.0 ** -21],        # 2^53 + 3 + eps -> 2^53 + 4
        "below_half_odd": [T + 1, T + 2, -2.0 ** -21, -2.0 ** -21],      # 2^53 + 3 - eps -> 2^53 + 2
    }
    cases = {}
    for k in (-1000, 0, 900):
        for name, vals in base_sets.items():
            for sgn, tag in ((1.0, "pos"), (-1.0, "neg")):
                cases[f"{name}-{tag}-2^{k}"] = [math.ldexp(sgn * v, k) for v in vals]
    sub = 2.0 ** -1074
    cases["subnormals_stay_subnormal"] = [3 * sub, 5 * sub, -7 * sub, (2 ** 51) * sub, 1 * sub]
    cases["subnormals_become_normal"] = [(2 ** 52 - 1) * sub, (2 ** 52 - 1) * sub, 3 * sub, -1 * sub]
    cases["subnormals_cancel_to_one"] = [(2 ** 52 - 1) * sub, -(2 ** 52 - 2) * sub]
    cases["near_the_top"] = [1.7e308, 1.7e308, 1.7e308, -1.7e308, -1.7e308]
    cases["over_the_top"] = [1.7e308] * 4
    return cases


def spans_both_words_cases(E=10, N=1 << 21):
    """name -> (N, big, [small values]): N rows of big = 2^E make a sum of 2^117 units, so the fold drops 65 bits: the half bit is bit 0 of
    the high word and the rest of the remainder is the whole low word.  The small values are whole units at exponents >= E - 73."""
    u = 2.0 ** (E - 96)
    half, one = 2.0 ** 64 * u, [(2.0 ** 23 + 1) * u, -(2.0 ** 23) * u]           # one unit, from two values the window admits
    odd = 2.0 ** 65 * u
    return {
        "tie_even": (N, 2.0 ** E, [half]),
        "tie_odd": (N, 2.0 ** E, [odd, half]),
        "half_plus_one_unit": (N, 2.0 ** E, [half] + one),
        "half_minus_one_unit": (N, 2.0 ** E, [half] + [-x for x in one]),
        "neg_tie_odd": (N, -(2.0 ** E), [-odd, -half]),
        "neg_half_plus_one_unit": (N, -(2.0 ** E), [-half] + [-x for x in one]),
    }


def beyond_the_window(E=30):
    """{A, -A} and 1001 copies of a full-mantissa value one binade below the last exact one: each copy loses its last bit"""
    return [1.5 * 2.0 ** E, -1.5 * 2.0 ** E] + [(2.0 ** 53 - 1) * 2.0 ** (E - 45 - 52)] * 1001


def spread_block(spread, n=4000, groups=7, seed=0, E=20):
    """keys and values: half of the rows at exponent E, half at E - spread, 24-bit mantissas, both signs"""
    r = rng("spread", spread, seed)
    k = r.integers(0, groups, size=n).astype(np.uint32)
    m = (r.integers(0, 1 << 23, size=n) + (1 << 23)).astype(np.float64)
    e = np.where(np.arange(n) % 2 == 0, E, E - spread) - 23
    v = np.ldexp(m, e) * r.choice(np.array([-1.0, 1.0]), size=n)
    return k, v


# ---- 2c, 2d: two blocks whose exponents differ by sh ---------------------------------------------------------------------------------------
SHIFTS = (1, 63, 64, 65, 70, 73)


def two_scale_blocks(sh, n=3000, groups=40, seed=0, e1=-7, exact=True):
    """(keys1, values1, keys2, values2): block 1 at exponent e1 with min(27, 97 - sh) mantissa bits (exact: every value is a whole number of
    the units of the window that block 2, at exponent e1 + sh, brings) or 53 bits (not exact), both signs; the groups with key % 3 == 0 hold
    negative block-1 values only.  Block 2 has 27-bit mantissas."""
    r = rng("two-scale", sh, seed, exact)
    bits = min(27, 97 - sh) if exact else 53
    k1 = r.integers(0, groups, size=n).astype(np.uint32)
    k2 = r.integers(0, groups, size=n).astype(np.uint32)
    m1 = (r.integers(0, 1 << (bits - 1), size=n) + (1 << (bits - 1))).astype(np.float64)
    v1 = np.ldexp(m1, e1 - (bits - 1)) * r.choice(np.array([-1.0, 1.0]), size=n)
    v1[k1 % 3 == 0] = -np.abs(v1[k1 % 3 == 0])
    m2 = (r.integers(0, 1 << 26, size=n) + (1 << 26)).astype(np.float64)
    v2 = np.ldexp(m2, e1 + sh - 26) * r.choice(np.array([-1.0, 1.0]), size=n)
    v2[k2 % 5 == 1] = 0.0                                      # some groups keep their (shifted) block-1 state alone
    v2[0] = 2.0 ** (e1 + sh)                                   # (Emax of block 2, whatever the draw)
    return k1, v1, k2, v2


# ---- 2f: more rows than the window holds -----------------------------------------------------------------------------------------------------
BIG_X = 2.0 - 2.0 ** -36
BIG_KEYS = (7, 9, 0)            # the dominant key, the key of the -x rows, the zero key


def big_block(rows):
    """one block: key 7 holds BIG_X in all of its rows, key 9 holds -BIG_X in 64 rows, key 0 holds small values: whole multiples of
    2^(Emax - 88) of magnitude >= 2^(Emax - 60) (Emax = 0), in 1024 rows"""
    r = rng("big", rows)
    k = np.full(rows, BIG_KEYS[0], dtype=np.uint32)
    v = np.full(rows, BIG_X)
    at = r.permutation(rows)[:64 + 1024]
    k[at[:64]], v[at[:64]] = BIG_KEYS[1], -BIG_X
    small = (r.integers(0, 1 << 20, size=1024) + (1 << 28)).astype(np.float64) * 2.0 ** -88 * r.choice(np.array([-1.0, 1.0]), size=1024)
    k[at[64:]], v[at[64:]] = BIG_KEYS[2], small
    return k, v


def big_expectation(k, v, times):
    """key -> the correctly rounded sum of the block added `times` times"""
    return {key: float(sum(Fraction(float(x)) for x in v[k == key].tolist()) * times) if key != BIG_KEYS[0]
            else float(Fraction(BIG_X) * int((k == key).sum()) * times) for key in BIG_KEYS}
