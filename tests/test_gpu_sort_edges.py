"""The radix sort (k_sort_keys + one stable 256-way partition per key byte) and ORDER BY ... LIMIT at the edges of their code, bit for bit
against tests/sort_ref.py (a stable order computed on values; test_sort_ref.py holds it against oracle/sorting.py).

The partition works in steps of 64 rows, wave strips of STRIP = 1024 rows and tiles of TILE = 4096 rows; its (shard, tile) counts go
through a device-wide scan whose own tile is 2048 elements = 8 partition tiles at 256 shards.  The sizes sit on, one below and one above
each of those; the patterns put whole tie classes across strips and tiles (a stability bug shows as a permutation that is still sorted by
value but not by row), drive every key byte through every digit, and leave all but one digit empty.

The LIMIT tests run at exactly 2^20 rows, where the strided sample takes rows 0, 16, 32, ... (65 536 of them), the threshold is the
sample's value at rank ceil(limit / 16) * 4 + 32, and more than 2^20 / 8 = 131 072 candidates give up.  Each case states the arithmetic
that puts it on its path, and the launch counter confirms the path."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sort_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

STRIP, TILE = 1024, 4096
SIZES = [63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 7 * TILE, 8 * TILE, 8 * TILE + 1]
INT_TYPES = [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64]
ALL_TYPES = INT_TYPES + [np.float32, np.float64]
DIRECTION_HINT = [(False, 1), (False, -1), (True, 1), (True, -1)]


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


@pytest.fixture(scope="module")
def ctx(ch):
    return ch.Context(0)


def check_sort(ch, x, col=None, desc=False, hint=1, ctx=None):
    col = ctx.upload(x) if col is None else col
    got = ch.sort_permutation(col, None, desc, hint).numpy()
    want = R.get_permutation(x, desc, hint)
    assert got.dtype == np.uint64 and got.shape == want.shape
    assert np.array_equal(got, want), (x.dtype, x.shape, desc, hint, np.flatnonzero(got != want)[:5], got[:8], want[:8])
    return got


# ------------------------------------------------------------------------------------------------------------------------------
# sizes and patterns
# ------------------------------------------------------------------------------------------------------------------------------
def patterns(dt, n):
    dt = np.dtype(dt)
    ones = int.from_bytes(b"\x01" * dt.itemsize, "little")
    i = np.arange(n, dtype=np.uint64)
    rep = lambda byte: (byte.astype(np.uint64) * np.uint64(ones)).astype(dt)   # the same byte in every position of the key
    yield "constant", np.full(n, 0x5A * ones, dtype=dt)
    if n <= 1 << (8 * dt.itemsize):
        yield "strictly decreasing", (np.uint64(n - 1) - i).astype(dt)
    else:   # more rows than one byte has values: as steep as the width allows, every value a run of equal rows
        yield "decreasing", ((np.uint64(n - 1) - i) * np.uint64(256) // np.uint64(n)).astype(dt)
    yield "bytes of period 256", rep(i % np.uint64(256))
    yield "bytes of period 257", rep((i % np.uint64(257)) & np.uint64(0xFF))
    yield "all 0xFF", np.full(n, 0xFF * ones, dtype=dt)
    yield "all 0x00", np.zeros(n, dtype=dt)
    yield "two values in blocks of 1000", rep(np.where((i // np.uint64(1000)) % np.uint64(2) == 0, 0xC3, 0x3C))
    last_tile = (n - 1) // TILE * TILE
    last_strip = last_tile + (n - 1 - last_tile) // STRIP * STRIP
    for pos in sorted({0, STRIP - 1, STRIP, last_tile, last_strip, last_strip - 1, n - 1}):
        if 0 <= pos < n:
            x = np.full(n, 0x80 * ones, dtype=dt)
            x[pos] = 0x7F * ones       # differs in every byte: every pass moves this one row across a constant column
            yield f"one different row at {pos}", x


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.uint64])   # digit from a 1-, 2-, 4-, 8-byte key: one sel_at mode each
def test_sizes_and_patterns(ch, ctx, dtype):
    for n in SIZES:
        for name, x in patterns(dtype, n):
            col = ctx.upload(x)
            for desc in (False, True):
                got = check_sort(ch, x, col, desc)
                if name in ("constant", "all 0xFF", "all 0x00"):
                    assert np.array_equal(got, np.arange(n, dtype=np.uint64)), (name, n, desc)


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_aligned_and_unaligned_views_of_the_same_data(ch, ctx, dtype):
    """the same rows at byte offsets 0 and 16 (16-byte aligned) and at one and three elements (not): full tiles and a part tile.  The view
    is what k_sort_keys reads; the passes split the derived key column, which is its own 16-byte aligned allocation, so the histogram's
    16-byte loads are held against its per-row loads by the selector views of test_gpu_partition_edges.py"""
    rng = np.random.Generator(np.random.PCG64(np.dtype(dtype).itemsize))
    N = 3 * TILE + 8
    x = rng.integers(0, np.iinfo(dtype).max, size=N, dtype=dtype, endpoint=True)
    x[rng.random(N) < 0.4] = x[0]                     # one heavy tie class
    x[rng.random(N) < 0.3] &= dtype(0x0300FF)         # and many small ones
    base = ctx.upload(x)
    for start in (0, 1, 3, 16 // np.dtype(dtype).itemsize):
        for n in (3 * TILE, 3 * TILE + 1, 2 * TILE - 1):
            for desc in (False, True):
                check_sort(ch, x[start:start + n], base.cut(start, n), desc)


def test_grid_stride_loop_of_the_scatter(ch, ctx):
    """the scatter runs three workgroups per compute unit: one tile more than that grid, and a part tile, so a workgroup takes a second tile"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (3 * cus + 1) * TILE + 5
    x = np.random.Generator(np.random.PCG64(cus)).integers(0, 256, size=n, dtype=np.uint8)
    got = ch.sort_permutation(ctx.upload(x)).numpy()
    assert np.array_equal(got, np.argsort(x, kind="stable").astype(np.uint64))


# ------------------------------------------------------------------------------------------------------------------------------
# the key fold
# ------------------------------------------------------------------------------------------------------------------------------
def twice_shuffled(values, seed):
    x = np.concatenate([values, values])
    np.random.Generator(np.random.PCG64(seed)).shuffle(x)
    return x


@pytest.mark.parametrize("dtype", [np.uint16, np.int16])
def test_key_fold_every_16_bit_value(ch, ctx, dtype):
    x = twice_shuffled(np.arange(65536, dtype=np.uint16).view(dtype), 16)
    col = ctx.upload(x)
    for desc in (False, True):
        got = check_sort(ch, x, col, desc)
        assert np.array_equal(x[got.astype(np.int64)], np.repeat(np.unique(x)[::-1 if desc else 1], 2))


def float_grid(dtype):
    """every exponent x both signs x mantissa {0, 1, the top bit, all ones}: zeros, denormals, normals, infinities, quiet and signalling NaN"""
    if np.dtype(dtype) == np.float32:
        u, exps, mbits = np.uint32, 256, 23
    else:
        u, exps, mbits = np.uint64, 2048, 52
    e = np.arange(exps, dtype=u) << u(mbits)
    m = np.array([0, 1, 1 << (mbits - 1), (1 << mbits) - 1], dtype=u)
    sign = np.array([0, 1], dtype=u) << u(mbits + (8 if mbits == 23 else 11))
    return (sign[:, None, None] | e[None, :, None] | m[None, None, :]).reshape(-1).view(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_key_fold_float_exponents_signs_and_mantissa_edges(ch, ctx, dtype):
    x = twice_shuffled(float_grid(dtype), 32)
    assert np.isnan(x).sum() == 2 * 2 * 3 and (x == 0).sum() == 4 and np.signbit(x[x == 0]).sum() == 2
    col = ctx.upload(x)
    for desc, hint in DIRECTION_HINT:
        got = check_sort(ch, x, col, desc, hint).astype(np.int64)
        # stated once more without the reference: all NaN patterns are one tie class in row order, and so are the four zeros
        nan_first = (hint < 0) != desc
        nan_rows = got[:12] if nan_first else got[-12:]
        assert np.isnan(x[nan_rows]).all() and (np.diff(nan_rows) > 0).all()
        zero_rows = got[x[got] == 0]
        assert zero_rows.shape[0] == 4 and (np.diff(zero_rows) > 0).all() and (np.diff(np.flatnonzero(x[got] == 0)) == 1).all()


@pytest.mark.parametrize("dtype", [np.int8, np.int32, np.int64])
def test_key_fold_signed_extremes(ch, ctx, dtype):
    ii = np.iinfo(dtype)
    x = twice_shuffled(np.array([ii.min, ii.max, -1, 0, 1], dtype=dtype), 5)
    for desc in (False, True):
        got = check_sort(ch, x, None, desc, ctx=ctx)
        want_values = np.repeat(np.array([ii.min, -1, 0, 1, ii.max], dtype=dtype), 2)
        assert np.array_equal(x[got.astype(np.int64)], want_values[::-1] if desc else want_values)


# ------------------------------------------------------------------------------------------------------------------------------
# perm_in
# ------------------------------------------------------------------------------------------------------------------------------
def test_perm_in_shorter_than_the_column_sorts_only_the_named_rows(ch, ctx):
    rng = np.random.Generator(np.random.PCG64(41))
    n, m = 3 * TILE + 17, TILE + 3
    x = rng.integers(-4, 4, size=n).astype(np.int32)
    rows = rng.permutation(n)[:m].astype(np.uint64)
    rows[5] = rows[9]                                  # a row named twice stays twice, in the order of its two mentions
    col, pin = ctx.upload(x), ctx.upload(rows)
    for desc in (False, True):
        got = ch.sort_permutation(col, pin, desc, 1).numpy()
        want = rows[R.get_permutation(x[rows.astype(np.int64)], desc, 1).astype(np.int64)]
        assert np.array_equal(got, want), desc


def test_perm_in_composes_order_by_a_b(ch, ctx):
    rng = np.random.Generator(np.random.PCG64(42))
    n = 2 * TILE + 1
    a = rng.integers(0, 5, size=n).astype(np.uint8)
    b = np.round(rng.standard_normal(n) * 2).astype(np.float32)
    b[rng.random(n) < 0.1] = np.nan
    b[rng.random(n) < 0.1] = -0.0
    ca, cb = ctx.upload(a), ctx.upload(b)
    for (da, db, hb) in [(False, False, 1), (True, False, -1), (False, True, 1), (True, True, -1)]:
        got = ch.sort_permutation(ca, ch.sort_permutation(cb, None, db, hb), da, 1).numpy()
        assert np.array_equal(got, R.sort_block([(a, da, 1), (b, db, hb)])), (da, db, hb)


def test_perm_in_entry_out_of_range_reads_row_0_and_is_reported_as_0(ch, ctx):
    """k_sort_keys states it: an entry >= rows is a caller bug, read as row 0 and written back as 0"""
    x = np.array([50, 10, 40, 20, 30, 60, 0, 70], dtype=np.int64)
    pin = np.array([7, 8, 1, 2**63, 3, 2**64 - 1], dtype=np.uint64)          # x: 70, 50 (row 0), 10, 50 (row 0), 20, 50 (row 0)
    got = ch.sort_permutation(ctx.upload(x), ctx.upload(pin), False, 1).numpy()
    assert got.tolist() == [1, 3, 0, 0, 0, 7]
    got = ch.sort_permutation(ctx.upload(x), ctx.upload(pin), True, 1).numpy()
    assert got.tolist() == [7, 0, 0, 0, 3, 1]


# ------------------------------------------------------------------------------------------------------------------------------
# ORDER BY ... LIMIT
# ------------------------------------------------------------------------------------------------------------------------------
N = 1 << 20
STRIDE = 16                     # N / 65 536
SAMPLE_ROWS = np.arange(0, N, STRIDE)
CAP = N // 8


def rank_of(limit):
    return (limit * 65536 + N - 1) // N * 4 + 32


def launches(ctx):
    return ctx.counters()["KernelLaunches"]


def check_limit(ch, ctx, x, limit, desc, hint, path, want=None):
    """path: 'full'   refused by the early gate: exactly the launches of a plain sort_permutation;
             'nan'    past the gate, NaN threshold: the sample, its sort, the full sort;
             'late'   past the gate, too few or too many candidates: the sample, its sort, the compare, filterToIndices, the full sort;
             'taken'  the candidates gathered, sorted and mapped back to rows: two gathers more, the second sort over the candidates.
    A sort of any non-empty column of one type costs the same launches P, and filterToIndices of a mask of N rows with a row set the
    same, so the counter tells the four apart exactly (the first line of each branch is the inequality the path check asks for)."""
    col = ctx.upload(x)
    c = launches(ctx)
    full = ch.sort_permutation(col, None, desc, hint)
    P = launches(ctx) - c
    c = launches(ctx)
    got = ch.sort_permutation_limit(col, limit, desc, hint).numpy()
    D = launches(ctx) - c
    if want is None:
        want = R.get_permutation(x, desc, hint)[:limit]
    assert got.dtype == np.uint64 and np.array_equal(got, want), (x.dtype, limit, desc, hint, got[:12], want[:12])
    assert np.array_equal(full.numpy(min(limit, x.shape[0])), want)
    finite = x[~np.isnan(x)] if x.dtype.kind == "f" else x
    c = launches(ctx)
    ch.filter_to_indices(ch.cmp_const(col, ch.LE, finite.max()))
    M = launches(ctx) - c
    print(f"{x.dtype} limit={limit} desc={desc} hint={hint} path={path}: plain sort {P} launches, with limit {D}, compare + indices {M}")
    if path == "full":
        assert D == P
    else:
        assert D > P
        assert D == {"nan": 2 * P + 1, "late": 2 * P + 1 + M, "taken": 2 * P + 3 + M}[path], (path, D, P, M)


def test_limit_early_gate(ch, ctx):
    rng = np.random.Generator(np.random.PCG64(64))
    x = rng.integers(-2**62, 2**62, size=N, dtype=np.int64)
    # 2^20 - 1 rows: below the row gate, whatever the limit
    check_limit(ch, ctx, x[:N - 1], 10, False, 1, "full")
    # limit 16 384: 16 384 * 64 == 2^20, not greater: admitted.  rank = 1024 * 4 + 32 = 4128 of 65 536, so about 4129 * 16 = 66 064
    # rows of a uniform column are candidates (the sample's quantile wobbles by ~ +-1 000 rows): between the limit and the cap
    check_limit(ch, ctx, x, 16384, False, 1, "taken")
    # limit 16 385: 16 385 * 64 > 2^20: refused
    check_limit(ch, ctx, x, 16385, False, 1, "full")


def test_limit_candidate_cap(ch, ctx):
    rows = np.arange(N, dtype=np.int64)
    x = np.where(rows % 8 == 0, 0, 1 + rows)
    # limit 10: rank 36; every sample row (a multiple of 16) holds 0, so the threshold is 0 and the candidates are the 131 072 zero
    # rows == the cap, not above it: taken
    check_limit(ch, ctx, x, 10, False, 1, "taken", want=np.arange(0, 80, 8, dtype=np.uint64))
    # one more zero: 131 073 candidates > cap: the late fallback
    x[3] = 0
    check_limit(ch, ctx, x, 10, False, 1, "late", want=np.array([0, 3, 8, 16, 24, 32, 40, 48, 56, 64], dtype=np.uint64))


def blind_sample_column():
    x = 10**9 + np.arange(N, dtype=np.int64)
    x[SAMPLE_ROWS] = np.arange(65536)
    return x


@pytest.mark.parametrize("limit,path", [(10, "taken"), (1000, "late"), (16384, "late")])
def test_limit_blind_sample_too_few_candidates(ch, ctx, limit, path):
    # the sample sees 0 .. 65535 in order and nothing else, so the threshold IS the rank and rank + 1 rows are candidates:
    # limit 10: rank 36, 37 candidates >= 10: taken.  limit 1000: rank 63 * 4 + 32 = 284, 285 candidates < 1000: fallback.
    # limit 16 384: rank 4128, 4129 candidates < 16 384: fallback
    assert rank_of(limit) + 1 == {10: 37, 1000: 285, 16384: 4129}[limit]
    check_limit(ch, ctx, blind_sample_column(), limit, False, 1, path, want=(np.arange(limit, dtype=np.uint64) * np.uint64(STRIDE)))


def test_limit_blind_sample_too_many_candidates(ch, ctx):
    # the mirror image: the sample rows hold the large values, every other row a small one.  limit 10: rank 36, the threshold is the
    # sample's 37th smallest = 10^9 + 16 * 36, and all 983 040 other rows lie below it: 983 077 candidates > cap: fallback
    x = np.arange(N, dtype=np.int64)
    x[SAMPLE_ROWS] += 10**9
    check_limit(ch, ctx, x, 10, False, 1, "late", want=np.arange(1, 11, dtype=np.uint64))


def near_and_far(dtype, desc):
    """most rows at the far extreme of the order; 400 sample rows and 4000 others hold ten near values.  i8 and i32 (every signed type)
    keep the near values negative in both directions."""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        big = np.finfo(dt).max
        return (-big, [1000.5 - r for r in range(10)]) if desc else (big, [-1000.5 + r for r in range(10)])
    ii = np.iinfo(dt)
    if desc:
        return ii.min, [(-11 - r if ii.min < 0 else ii.max - r) for r in range(10)]
    return ii.max, [ii.min + r for r in range(10)]


def near_far_column(dtype, desc, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    far, near = near_and_far(dtype, desc)
    x = np.full(N, far, dtype=dtype)
    others = rng.choice(np.flatnonzero(np.arange(N) % STRIDE != 0), size=4000, replace=False)
    on_sample = rng.choice(SAMPLE_ROWS, size=400, replace=False)
    x[others] = np.asarray(near, dtype=dtype)[rng.integers(0, 10, size=others.shape[0])]
    x[on_sample] = np.asarray(near, dtype=dtype)[rng.integers(0, 10, size=400)]
    return x


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("dtype", ALL_TYPES)
def test_limit_every_width_through_the_compare(ch, ctx, dtype, desc):
    # limit 10: rank 36.  The sample holds 400 near values (ten distinct, ~40 rows each) and 65 136 far ones, so its value at rank 36 is
    # the nearest or second nearest of the ten; the candidates are the rows of the whole column at or inside it: at least 37, at most
    # the 4400 near rows -- between the limit and the cap: taken.  The threshold is negative for every signed type.
    x = near_far_column(dtype, desc, np.dtype(dtype).num)
    if np.dtype(dtype).kind == "f":
        x[1::STRIDE][:100] = np.nan           # NaN sorts last and off the sample
    thr = (np.sort(x[SAMPLE_ROWS])[::-1] if desc else np.sort(x[SAMPLE_ROWS]))[rank_of(10)]
    n_cand = int((x >= thr).sum() if desc else (x <= thr).sum())
    assert 37 <= n_cand <= 4400 and (np.dtype(dtype).kind != "i" or thr < 0)
    check_limit(ch, ctx, x, 10, desc, -1 if desc else 1, "taken")


def test_limit_fallback_too_few_candidates_uint16(ch, ctx):
    # sample row 16 i holds i // 2 (0 .. 32767, each twice), every other row 40 000 or more.  limit 1000: rank 284, threshold 142,
    # candidates = the 286 sample rows holding 0 .. 142 < 1000: fallback
    x = (40000 + np.arange(N) % 20000).astype(np.uint16)
    x[SAMPLE_ROWS] = np.arange(65536) // 2
    check_limit(ch, ctx, x, 1000, False, 1, "late", want=(np.arange(1000, dtype=np.uint64) * np.uint64(STRIDE)))


def test_limit_fallback_too_many_candidates_int8(ch, ctx):
    # -5 on every fourth row (all of the sample), 100 elsewhere: threshold -5, 262 144 candidates > cap: fallback
    x = np.full(N, 100, dtype=np.int8)
    x[::4] = -5
    check_limit(ch, ctx, x, 10, False, 1, "late", want=np.arange(0, 40, 4, dtype=np.uint64))


@pytest.mark.parametrize("dtype,desc,threshold_sign", [(np.float64, False, -0.0), (np.float64, False, 0.0), (np.float32, True, -0.0), (np.float32, True, 0.0)])
def test_limit_threshold_is_a_zero_of_either_sign(ch, ctx, dtype, desc, threshold_sign):
    # the extreme values of the order are 4400 zeros of mixed sign (400 on the sample), everything else is far away.  limit 10: rank 36;
    # the sample's zeros are one tie class in row order, so the threshold is the 37th sample zero, whose sign is chosen here.  The
    # compare must take both signs: 4400 candidates, taken; the prefix is the first ten zero rows of either sign
    x = near_far_column(dtype, desc, 7)
    zero_rows = np.flatnonzero(np.abs(x) < 2000)
    assert zero_rows.shape[0] == 4400
    x[zero_rows] = np.where(np.arange(4400) % 3 == 0, -0.0, 0.0).astype(dtype)
    sample_zeros = zero_rows[zero_rows % STRIDE == 0]
    x[sample_zeros[rank_of(10)]] = threshold_sign
    assert np.signbit(x[zero_rows[:10]]).any() and not np.signbit(x[zero_rows[:10]]).all()
    check_limit(ch, ctx, x, 10, desc, -1 if desc else 1, "taken", want=zero_rows[:10].astype(np.uint64))


def test_limit_float32_denormals_at_the_threshold(ch, ctx):
    # the ten near values are the denormals -5 .. 4 times 2^-149 (zero among them), the rest 1.0: the threshold is a denormal or zero and
    # every comparison at the threshold is between denormals.  limit 10: rank 36, 37 .. 4400 candidates: taken
    x = near_far_column(np.float32, False, 9)
    near = np.abs(x) < 2000
    tiny = np.float32(2.0 ** -149)
    x[near] = (np.round(x[near] + np.float32(1000.5)) - 5) * tiny
    x[~near] = 1.0
    assert near.sum() == 4400 and np.unique(x).shape[0] == 11 and np.abs(x[near]).max() == 5 * tiny
    check_limit(ch, ctx, x, 10, False, 1, "taken")


def test_limit_nan_threshold_and_nan_first(ch, ctx):
    # 99.99 % NaN: 105 numbers, none of them on a sample row, so the whole sample is NaN and so is its value at rank 36.  NaN last
    # (ascending, hint +1): past the gate, NaN threshold: fallback.  NaN first (hint -1): refused at the gate
    x = np.full(N, np.nan, dtype=np.float64)
    rows = 1 + STRIDE * np.arange(105) * 613
    x[rows] = np.cos(np.arange(105))
    assert rows.max() < N and (rows % STRIDE != 0).all() and np.isnan(x).mean() > 0.9998
    check_limit(ch, ctx, x, 10, False, 1, "nan")
    check_limit(ch, ctx, x, 10, False, -1, "full")
    check_limit(ch, ctx, x.astype(np.float32), 10, True, -1, "nan")
