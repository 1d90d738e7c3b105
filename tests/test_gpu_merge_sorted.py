"""The merge of sorted runs on the device against tests/merge_sorted_ref.py, bit for bit, with the device's own sort_block permutation of
the concatenation as a second witness.

T is the merge tile.  The shapes are the smallest at which each mechanism can break: run lengths around the wave and the tile in mixed
pairs, a diagonal crossing exactly on a tile edge, one run wholly below the other, all-equal runs (the identity), run counts with a
pass-through run in several rounds, 257 tiny runs in one launch, every dtype in both directions, floats with NaN / -0.0 / +0.0 over
different runs, first-word ties that fall through to the gathered columns across a tile edge and a run boundary, and limits at 1, a run
length, one past a tile and above the row count.  Inputs of up to 200 rows are also checked against the per-row (cursor) reference, all
against the vectorised one (test_merge_sorted_ref.py holds the two together).  tests/merge_sorted_driver.cpp pins which plan the two
shapes of test_both_plans take; single-column cases over 1-byte keys in more than two runs go to the sort chain by the byte model, so every dtype is also the
first of two key columns, which the merge tree serves."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_sorted_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


@pytest.fixture(scope="module")
def ctx(ch):
    return ch.Context(0)


@pytest.fixture(scope="module")
def T():
    from clickhouse_amd import merge_sorted
    return merge_sorted.TILE


def check_merge(ch, ctx, cols, spec, offs, limit=0):
    """cols: host columns over the concatenation, every run sorted by spec.  -> the permutation, after comparing it with both
    references and with the device's stable sort of the concatenation"""
    d = R.describe(cols, spec)
    want = R.merge_lexsort(d, limit)
    if len(cols[0]) <= 200:
        assert np.array_equal(R.merge_cursors(d, offs, limit), want)
    dev = [ctx.upload(c) for c in cols]
    got = ch.merge_sorted_permutation(dev, spec, offs, limit=limit).numpy()
    assert got.dtype == np.uint64 and got.shape == want.shape
    assert np.array_equal(got, want), (np.flatnonzero(got != want)[:5], got[:8], want[:8])
    if len(cols[0]):
        _, perm = ch.sort_block(dev, spec)
        assert np.array_equal(got, perm.numpy()[:len(want)])
    return got


def sorted_case(seed, dtypes, spec, run_lens, distinct=7):
    rng = np.random.Generator(np.random.PCG64(seed))
    offs = R.offsets_of(run_lens)
    cols = [R.random_column(rng, dt, int(offs[-1]), distinct) for dt in dtypes]
    return R.sort_runs(cols, spec, offs), offs


ASC = [(0, False, 1)]


def test_run_lengths_around_the_wave_and_the_tile(ch, ctx, T):
    lens = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1]
    pairs = [(a, b) for a in lens for b in lens if (a + b) % 3 != 1 or a == b] + [(1, 3 * T), (3 * T, 1)]
    for k, (a, b) in enumerate(pairs):
        cols, offs = sorted_case(100 + k, [np.int64], ASC, [a, b], distinct=40)
        check_merge(ch, ctx, cols, ASC, offs)


def test_crossing_on_a_tile_edge_and_disjoint_runs(ch, ctx, T):
    evens, odds = np.arange(0, 2 * T, 2, dtype=np.int64), np.arange(1, 2 * T, 2, dtype=np.int64)
    offs = R.offsets_of([T, T])
    got = check_merge(ch, ctx, [np.concatenate([evens, odds])], ASC, offs)     # diagonal T crosses at (T / 2, T / 2)
    assert got[T] == T // 2 and got[T - 1] == T + T // 2 - 1
    low, high = np.arange(T + 7, dtype=np.int64), np.arange(T + 7, 3 * T, dtype=np.int64)
    got = check_merge(ch, ctx, [np.concatenate([low, high])], ASC, R.offsets_of([len(low), len(high)]))   # left below right
    assert np.array_equal(got, np.arange(3 * T, dtype=np.uint64))
    got = check_merge(ch, ctx, [np.concatenate([high, low])], ASC, R.offsets_of([len(high), len(low)]))   # and the reverse
    assert got[0] == len(high) and got[-1] == len(high) - 1
    # runs that end exactly where the tile does: diagonal T crosses at (T, 0)
    check_merge(ch, ctx, [np.concatenate([np.arange(T, dtype=np.int64), np.arange(T, 2 * T + 3, dtype=np.int64)])], ASC, R.offsets_of([T, T + 3]))


@pytest.mark.parametrize("dtype", [np.int64, np.float64, np.uint16])
def test_one_repeated_value_is_the_identity(ch, ctx, T, dtype):
    col = np.full(2 * T + 100, 7, dtype=dtype)
    for lens in ([T + 50, T + 50], [1, 2 * T + 99], [700] * 2 + [2 * T - 1300]):
        for spec in (ASC, [(0, True, -1)]):
            got = check_merge(ch, ctx, [col], spec, R.offsets_of(lens))
            assert np.array_equal(got, np.arange(len(col), dtype=np.uint64))


@pytest.mark.parametrize("K", [1, 2, 3, 5, 8, 9])
def test_run_counts_with_a_pass_through_run(ch, ctx, T, K):
    lens = [(T // 2) + 37 * r + (r % 2) for r in range(K)]
    cols, offs = sorted_case(K, [np.int64], ASC, lens, distinct=100)
    got = check_merge(ch, ctx, cols, ASC, offs)
    if K == 1:
        assert np.array_equal(got, np.arange(lens[0], dtype=np.uint64))
    cols, offs = sorted_case(K + 50, [np.int32, np.float32], [(1, True, 1), (0, False, 1)], lens)
    check_merge(ch, ctx, cols, [(1, True, 1), (0, False, 1)], offs)


def test_257_tiny_runs_share_one_launch(ch, ctx, T):
    rng = np.random.Generator(np.random.PCG64(257))
    lens = [0 if r % 5 == 2 else int(rng.integers(1, 40)) for r in range(257)]
    lens[100] = T + 3
    cols, offs = sorted_case(257, [np.int64], ASC, lens, distinct=60)
    check_merge(ch, ctx, cols, ASC, offs)
    dev = [ctx.upload(c) for c in cols]
    launches = ctx.counters()["KernelLaunches"]
    ch.merge_sorted_permutation(dev, ASC, offs)
    # the two kernels of the check, the key build, nine rounds of ONE split and ONE tile launch, the permutation: never a launch per pair
    assert ctx.counters()["KernelLaunches"] - launches <= 2 + 1 + 2 * 9 + 1
    cols, offs = sorted_case(258, [np.uint32, np.int16], [(0, True, 1), (1, False, 1)], lens)
    check_merge(ch, ctx, cols, [(0, True, 1), (1, False, 1)], offs)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("descending", [False, True])
def test_every_dtype_in_both_directions(ch, ctx, T, dtype, descending):
    hints = (1, -1) if np.dtype(dtype).kind == "f" else (1,)
    for hint in hints:
        spec = [(0, descending, hint)]
        cols, offs = sorted_case(7, [dtype], spec, [T + 9, 300])
        check_merge(ch, ctx, cols, spec, offs)
        # the same column as the first of two keys (the merge tree for every width), three runs
        spec = [(0, descending, hint), (1, not descending, 1)]
        cols, offs = sorted_case(8, [dtype, np.int64], spec, [T + 9, 300, 1000])
        check_merge(ch, ctx, cols, spec, offs)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("hint", [1, -1])
def test_float_specials_spread_over_runs(ch, ctx, dtype, descending, hint):
    spec = [(0, descending, hint)]
    runs = [[np.nan, -0.0, 1.0], [0.0, np.nan, -1.0, -0.0], [np.nan], [], [0.0, 0.0, -0.0, np.inf, -np.inf, np.nan]]
    col = np.array([v for r in runs for v in r], dtype=dtype)
    offs = R.offsets_of([len(r) for r in runs])
    cols = R.sort_runs([col], spec, offs)
    got = check_merge(ch, ctx, cols, spec, offs)
    zeros = [i for i in got.tolist() if cols[0][i] == 0]
    nans = [i for i in got.tolist() if np.isnan(cols[0][i])]
    assert zeros == sorted(zeros) and nans == sorted(nans) and len(zeros) == 6 and len(nans) == 4   # each one tie class, in row order


def test_first_word_ties_fall_through_to_the_gathered_columns(ch, ctx, T):
    n = [T + 300, T - 100, 900]
    for dtypes, spec in (([np.uint32, np.int64], [(0, False, 1), (1, False, 1)]),
                         ([np.int8, np.float64, np.uint16], [(0, True, 1), (1, False, -1), (2, True, 1)])):
        cols, offs = sorted_case(21, dtypes, spec, n, distinct=30)
        cols[0][:] = 5                       # the first column constant: every comparison reads the next columns through the rows
        cols = R.sort_runs(cols, spec, offs)
        check_merge(ch, ctx, cols, spec, offs)
    # a stretch of first-word ties that crosses a tile edge and the run boundary: 1 .. 1 | 2 x (T + 200) in each run | 3 .. 3
    spec = [(0, False, 1), (1, True, 1)]
    first = np.concatenate([np.full(T - 100, 1), np.full(T + 200, 2), np.full(50, 3), np.full(60, 1), np.full(T + 200, 2), np.full(70, 3)]).astype(np.uint32)
    offs = R.offsets_of([2 * T + 150, T + 330])
    rng = np.random.Generator(np.random.PCG64(4))
    second = rng.integers(-50, 50, size=len(first)).astype(np.int64)
    cols = R.sort_runs([first, second], spec, offs)
    check_merge(ch, ctx, cols, spec, offs)


def test_eight_columns_of_mixed_types(ch, ctx, T):
    dtypes = [np.uint8, np.float32, np.int16, np.uint64, np.float64, np.int32, np.int8, np.uint16]
    spec = [(k, k % 3 == 1, 1 if k % 2 else -1) for k in range(8)]
    cols, offs = sorted_case(88, dtypes, spec, [T + 1, 0, 777, 2 * T - 5, 64], distinct=0)   # three or four values a column: deep ties
    check_merge(ch, ctx, cols, spec, offs)
    check_merge(ch, ctx, cols, spec, offs, limit=T + 1)


@pytest.mark.parametrize("limit", ["one", "run", "tile+1", "above"])
def test_limits(ch, ctx, T, limit):
    lens = [T + 5, 700, 2 * T]
    limit = {"one": 1, "run": 700, "tile+1": T + 1, "above": sum(lens) + 10}[limit]
    cols, offs = sorted_case(31, [np.int64], ASC, lens, distinct=50)
    got = check_merge(ch, ctx, cols, ASC, offs, limit=limit)
    assert len(got) == min(limit, sum(lens))
    spec = [(0, True, 1), (1, False, 1)]
    cols, offs = sorted_case(32, [np.uint8, np.float32], spec, lens)
    check_merge(ch, ctx, cols, spec, offs, limit=limit)
    # one run: the identity, cut
    one = np.sort(cols[0])[::-1].copy()
    assert np.array_equal(check_merge(ch, ctx, [one], [(0, True, 1)], R.offsets_of([len(one)]), limit=limit), np.arange(min(limit, len(one)), dtype=np.uint64))


def test_nothing_to_merge(ch, ctx):
    empty = np.zeros(0, dtype=np.int64)
    assert len(check_merge(ch, ctx, [empty], ASC, R.offsets_of([]))) == 0
    assert len(check_merge(ch, ctx, [empty], ASC, R.offsets_of([0, 0, 0]), limit=3)) == 0
    assert ch.is_sorted([ctx.upload(empty)], ASC, [0, 0]) is None and ch.is_sorted([ctx.upload(empty)], ASC) is None
    assert ch.is_sorted([ctx.upload(np.array([3], dtype=np.int64))], ASC) is None


def test_both_plans(ch, ctx):
    # merge_plan sends the first to the sort chain and the second to the merge tree (tests/merge_sorted_driver.cpp asserts which)
    cols, offs = sorted_case(64, [np.uint8], ASC, [300] * 64, distinct=200)
    check_merge(ch, ctx, cols, ASC, offs)
    check_merge(ch, ctx, cols, ASC, offs, limit=1000)
    cols, offs = sorted_case(3, [np.int64], ASC, [5000] * 3, distinct=2000)
    check_merge(ch, ctx, cols, ASC, offs)


def test_is_sorted(ch, ctx, T):
    n = 3 * T + 5
    base = np.arange(n, dtype=np.int64) // 3          # ties are not violations
    col = ctx.upload(base)
    assert ch.is_sorted([col], ASC) is None
    assert ch.is_sorted([col], [(0, True, 1)]) == 3   # descending: the first rise
    for rows, want in (([1], 1), ([n - 1], n - 1), ([T], T), ([2 * T], 2 * T), ([2 * T + 9, T + 1], T + 1), ([n - 1, 1], 1)):
        bad = base.copy()
        for r in rows:
            bad[r] = -1
        bad_rows = sorted(rows)
        d = [(bad, False, 1)]
        assert R.is_sorted_ref(d, [0, n]) == want == bad_rows[0]
        assert ch.is_sorted([ctx.upload(bad)], ASC) == want
    # a drop across a run boundary is no violation; the same drop inside a run is
    two = np.concatenate([np.arange(T + 1, dtype=np.int64), np.arange(100, dtype=np.int64)])
    assert ch.is_sorted([ctx.upload(two)], ASC, [0, T + 1, T + 101]) is None
    assert ch.is_sorted([ctx.upload(two)], ASC, [0, T, T + 101]) == T + 1
    assert ch.is_sorted([ctx.upload(two)], ASC, [0, 0, T + 1, T + 1, T + 101, T + 101]) is None
    # several columns: the violation is in the last one; floats by the hint
    a, b = np.zeros(n, dtype=np.uint8), np.arange(n, dtype=np.float32)
    b[T + 7] = np.nan
    assert ch.is_sorted([a, ctx.upload(b)], [(0, False, 1), (1, False, 1)]) == T + 8      # NaN is greatest: the next number drops
    assert ch.is_sorted([a, ctx.upload(b)], [(0, False, 1), (1, False, -1)]) == T + 7     # NaN is smallest: it drops itself
    assert ch.is_sorted([a, ctx.upload(b)], [(0, False, 1)]) is None


def test_check_refuses_unsorted_runs_and_the_context_goes_on(ch, ctx, T):
    two = np.concatenate([np.arange(T + 1, dtype=np.int64), np.arange(100, dtype=np.int64)])
    col = ctx.upload(two)
    with pytest.raises(ch.ChgpuError) as e:
        ch.merge_sorted_permutation([col], ASC, [0, T, T + 101], check=True)
    assert e.value.code == ch._capi.ERR_BAD_ARGUMENTS and f"row {T + 1} " in str(e.value)
    got = ch.merge_sorted_permutation([col], ASC, [0, T + 1, T + 101], check=True).numpy()
    assert np.array_equal(got, R.merge_lexsort([(two, False, 1)]))
    assert np.array_equal(ch.merge_sorted_permutation([col], ASC, [0, T + 1, T + 101], check=False).numpy(), got)


def test_merge_sorted_blocks_with_carried_columns(ch, ctx, T):
    rng = np.random.Generator(np.random.PCG64(9))
    spec = [(1, True, 1)]
    sizes = [T + 11, 0, 500, 3000]
    host = [[rng.integers(0, 2**40, size=n).astype(np.int64), rng.integers(-20, 20, size=n).astype(np.int32), rng.integers(0, 255, size=n).astype(np.uint8)]
            for n in sizes]
    blocks = []
    for b in host:   # sort every block by the key (stable), carrying the two other widths
        p = R.merge_lexsort([(b[1], True, 1)]).astype(np.int64)
        blocks.append([c[p] for c in b])
    glued = [np.concatenate([b[k] for b in blocks]) for k in range(3)]
    for limit in (0, 777):
        want = R.merge_lexsort([(glued[1], True, 1)], limit).astype(np.int64)
        columns, perm = ch.merge_sorted_blocks([[ctx.upload(c) for c in b] for b in blocks], spec, limit=limit)
        assert np.array_equal(perm.numpy(), want.astype(np.uint64))
        sorted_cols, _ = ch.sort_block([ctx.upload(c) for c in glued], spec, limit)    # concatenate, then sort_block
        for k in range(3):
            assert columns[k].dtype == glued[k].dtype
            assert np.array_equal(columns[k].numpy(), glued[k][want])
            assert np.array_equal(columns[k].numpy(), sorted_cols[k].numpy())


@pytest.mark.parametrize("limit", [0, 100])
def test_merge_sorting_over_five_unequal_blocks(ch, ctx, T, limit):
    rng = np.random.Generator(np.random.PCG64(10))
    spec = [(0, False, 1), (2, True, -1)]
    sizes = [T + 1, 130, 2 * T + 77, 1, 999]      # every block longer than the limit is cut by add_block
    host = [[rng.integers(0, 9, size=n).astype(np.uint16), np.arange(n, dtype=np.int64) + 10**6 * k, R.random_column(rng, np.float64, n)]
            for k, n in enumerate(sizes)]
    op = ch.MergeSorting(spec, limit=limit, ctx=ctx)
    for b in host:
        op.add_block([ctx.upload(c) for c in b])
    if limit:
        assert [len(b[0]) for b in op.blocks] == [min(n, limit) for n in sizes]
    out = op.finish()
    glued = [np.concatenate([b[k] for b in host]) for k in range(3)]
    want = R.merge_lexsort(R.describe(glued, spec), limit).astype(np.int64)
    sorted_cols, _ = ch.sort_block([ctx.upload(c) for c in glued], spec, limit)
    for k in range(3):
        assert np.array_equal(out[k].numpy(), glued[k][want], equal_nan=(k == 2))
        assert np.array_equal(out[k].numpy(), sorted_cols[k].numpy(), equal_nan=(k == 2))
    assert op.finish() is None


def test_error_answers(ch, ctx):
    K = ch._capi
    L = K.lib()
    long_col, short_col = ctx.upload(np.arange(10, dtype=np.int64)), ctx.upload(np.arange(9, dtype=np.int64))
    offs = (C.c_uint64 * 3)(0, 4, 10)
    out, row = C.c_void_p(), C.c_uint64(0)

    def call(cols, n_keys=None, flags=0):
        n = len(cols) if n_keys is None else n_keys
        hs = (C.c_void_p * len(cols))(*[c._h for c in cols])
        return L.chgpu_merge_sorted_permutation(ctx._h, hs, (C.c_int32 * len(cols))(), (C.c_int32 * len(cols))(*([1] * len(cols))), n, offs, 2, 0, flags, C.byref(out))

    assert call([long_col, short_col]) == K.ERR_SIZES_MISMATCH and b"9 rows" in L.chgpu_last_error()
    hs = (C.c_void_p * 1)(short_col._h)
    assert L.chgpu_is_sorted(ctx._h, hs, (C.c_int32 * 1)(), (C.c_int32 * 1)(1), 1, offs, 2, C.byref(row)) == K.ERR_SIZES_MISMATCH
    assert call([long_col] * 9) == K.ERR_BAD_ARGUMENTS and b"key columns" in L.chgpu_last_error()
    assert call([long_col], n_keys=0) == K.ERR_BAD_ARGUMENTS
    assert call([long_col], flags=2) == K.ERR_BAD_ARGUMENTS and b"flag" in L.chgpu_last_error()
    assert call([long_col], flags=K.MERGE_CHECK_SORTED | 4) == K.ERR_BAD_ARGUMENTS
    assert not out.value
    assert call([long_col], flags=K.MERGE_CHECK_SORTED) == K.OK and out.value
    perm = ch.Column(ctx, out)
    assert np.array_equal(perm.numpy(), np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9], dtype=np.uint64))
