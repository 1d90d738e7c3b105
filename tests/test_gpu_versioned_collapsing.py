"""The VersionedCollapsing merge on the device against tests/versioned_collapsing_ref.py, bit for bit: the surviving rows and max_balance.

T is the fold tile.  The shapes are the smallest at which each mechanism can break: group lengths around the wave and the tile under every
kind of sign sequence, heads exactly on tile edges, a row whose cancelling row lies in the next tile or three tiles on, a survivor that is
a tile's last row, one group over more tiles than the one-workgroup carry step takes in a pass (and the same rows cut into short groups),
everything cancelling, 0 and 1 rows, 1 / 2 / 3 / 257 runs, the version as the last key column (floats that are equal only as order words),
every key dtype in both directions.  Every case is checked against the vectorised reference, inputs of up to 200 rows also against the
queue (test_versioned_collapsing_ref.py holds the two together)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_sorted_ref as R  # noqa: E402
import versioned_collapsing_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu

ASC = [(0, False, 1)]
KV = [(0, False, 1), (1, False, 1)]
PATTERNS = ("plus", "minus", "plus_minus", "minus_plus", "open_close", "close_open_3", "half", "mostly_plus")


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


@pytest.fixture(scope="module")
def ctx(ch):
    return ch.Context(0)


@pytest.fixture(scope="module")
def T():
    from clickhouse_amd import merge_fold
    return merge_fold.TILE


def layout(lens, n_runs, rng=None):
    """Groups of the given lengths in merged order, dealt to n_runs sorted runs.  rng None: a group's rows go to the runs in blocks (run
    numbers never decrease along the group, so the merged order is the order written here, and a group of n_runs rows or more has a row
    from every run); else at random, which keeps the merged order too (rows equal on the key merge lowest run first, and inside a run
    they keep the order written here).  -> (group number over the concatenation, offsets, order) where a column written in merged
    order is column[order] over the concatenation."""
    lens = np.asarray(lens, dtype=np.int64)
    n = int(lens.sum())
    group = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    if rng is None:
        within = np.arange(n) - np.repeat(np.cumsum(lens) - lens, lens)
        run = within * n_runs // np.repeat(lens, lens)
    else:
        # inside a group the merged order is (run, position in the run): every group's run numbers are sorted, so that the order
        # written here is M
        run = rng.integers(0, n_runs, n)
        run = run[np.lexsort((run, group))]
    order = np.argsort(run, kind="stable")
    return group[order], R.offsets_of(np.bincount(run, minlength=n_runs)), order


def signs_of(kind, length, rng):
    i = np.arange(length)
    if kind == "plus":
        s = np.ones(length)
    elif kind == "minus":
        s = -np.ones(length)
    elif kind == "plus_minus":
        s = np.where(i % 2 == 0, 1, -1)
    elif kind == "minus_plus":
        s = np.where(i % 2 == 0, -1, 1)
    elif kind == "open_close":                      # + ^ k  - ^ k
        s = np.where(i < length // 2, 1, -1)
    elif kind == "close_open_3":                    # - ^ k  + ^ (k + 3)
        s = np.where(i < max(length - 3, 0) // 2, -1, 1)
    elif kind == "half":
        s = np.where(rng.random(length) < 0.5, 1, -1)
    else:
        s = np.where(rng.random(length) < 0.9, 1, -1)
    return s.astype(np.int8)


def check(ch, ctx, keys, spec, offs, sign):
    """-> (rows, max_balance) of the device, equal to the reference's"""
    d = R.describe(keys, spec)
    want_rows, want_balance = V.versioned_vector(d, sign)
    if len(keys[0]) <= 200:
        cur_rows, cur_balance = V.versioned_cursor(d, offs, sign)
        assert np.array_equal(cur_rows, want_rows) and cur_balance == want_balance
    rows, balance = ch.versioned_collapsing_merge_rows([ctx.upload(k) for k in keys], spec, offs, sign)
    got = rows.numpy()
    assert got.dtype == np.uint64 and got.shape == want_rows.shape and np.array_equal(got, want_rows), (got[:8], want_rows[:8])
    assert isinstance(balance, int) and balance == want_balance, (balance, want_balance)
    return got, balance


def check_merged(ch, ctx, lens, merged_sign, n_runs, rng=None):
    """signs written in merged order over groups of the given lengths"""
    group, offs, order = layout(lens, n_runs, rng)
    merged_sign = np.asarray(merged_sign, dtype=np.int8)
    assert len(merged_sign) == len(group)
    got, balance = check(ch, ctx, [group], ASC, offs, merged_sign[order])
    return order[got.astype(np.int64)], balance           # order[row]: the merged position of a concatenated row


@pytest.mark.parametrize("n_runs", [1, 2, 3])
def test_group_lengths_around_the_wave_and_the_tile_under_every_sign_pattern(ch, ctx, T, n_runs):
    rng = np.random.Generator(np.random.PCG64(n_runs))
    lens = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3]
    for kind in PATTERNS:
        merged = np.concatenate([signs_of(kind, length, rng) for length in lens])
        for dealt in (None, rng):
            check_merged(ch, ctx, lens, merged, n_runs, dealt)
    mixed = np.concatenate([signs_of(PATTERNS[(k + n_runs) % len(PATTERNS)], length, rng) for k, length in enumerate(lens)])
    check_merged(ch, ctx, lens, mixed, n_runs, rng)
    check_merged(ch, ctx, lens[::-1], mixed[::-1].copy(), n_runs)


def test_group_heads_exactly_on_tile_edges(ch, ctx, T):
    rng = np.random.Generator(np.random.PCG64(11))
    for lens in ([T, T, T - 1, 1, T, 2 * T], [T, T], [2 * T, T, 1], [8] * (T // 8 + 3)):
        for kind in ("half", "mostly_plus", "open_close", "minus"):
            merged = np.concatenate([signs_of(kind, length, rng) for length in lens])
            check_merged(ch, ctx, lens, merged, 2, rng)


def test_a_cancelling_row_in_the_next_tile_and_three_tiles_on(ch, ctx, T):
    # the + is the last row of tile 0, its - the first row of tile 1
    lens = [T - 1, 2]
    merged = np.concatenate([-np.ones(T - 1), [1, -1]])
    for n_runs in (1, 2):
        kept, balance = check_merged(ch, ctx, lens, merged, n_runs)
        assert kept.tolist() == list(range(T - 1)) and balance == T - 1
    # one group: +, then 3 T / 2 balanced pairs, then the - of the first row three tiles later, then a + that stays
    merged = np.concatenate([[1], np.tile([1, -1], 3 * T // 2), [-1, 1]])
    for n_runs in (1, 3):
        kept, balance = check_merged(ch, ctx, [3 * T + 3], merged, n_runs)
        assert kept.tolist() == [3 * T + 2] and balance == 2
    # the same without the closing -: the first row stays, from three tiles back
    kept, balance = check_merged(ch, ctx, [3 * T + 2], np.concatenate([[1], np.tile([1, -1], 3 * T // 2), [1]]), 2)
    assert kept.tolist() == [0, 3 * T + 1] and balance == 2


def test_a_survivor_that_is_the_last_row_of_a_tile(ch, ctx, T):
    # group 1 is + - .. + over T - 1 rows: its last + (position T - 2) stays.  Group 2 begins on the tile's last position with + + -:
    # the first + stays, and what decides it lies in the next tile
    lens = [T - 1, 3]
    merged = np.concatenate([signs_of("plus_minus", T - 1, None), [1, 1, -1]])
    for n_runs in (1, 2):
        kept, balance = check_merged(ch, ctx, lens, merged, n_runs)
        assert kept.tolist() == [T - 2, T - 1] and balance == 2
    kept, _ = check_merged(ch, ctx, [2 * T], np.ones(2 * T), 2)          # every row of two full tiles
    assert len(kept) == 2 * T


def test_one_group_over_more_tiles_than_a_carry_pass_and_the_same_rows_in_short_groups(ch, ctx, T):
    """256 T + T + 5 rows: 258 tiles, so k_vc_carry and k_vc_offsets take two passes with a carry between them.  Signs at random with
    p = 0.5: the balance crosses zero many times.  Then the same rows cut into groups of geometric length with mean 40."""
    rng = np.random.Generator(np.random.PCG64(258))
    n = 256 * T + T + 5
    merged = signs_of("half", n, rng)
    kept, balance = check_merged(ch, ctx, [n], merged, 2)
    assert len(kept) == abs(int(merged.astype(np.int64).sum())) and balance > 8
    lens = rng.geometric(1 / 40, n // 20)
    ends = np.cumsum(lens)
    k = int(np.searchsorted(ends, n))
    lens = lens[:k + 1].copy()
    lens[k] -= ends[k] - n
    assert lens.sum() == n and lens.min() >= 1
    kept, balance = check_merged(ch, ctx, lens, merged, 2, rng)
    assert len(kept) > n // 40 and balance >= 4


def test_every_group_cancels(ch, ctx, T):
    kept, balance = check_merged(ch, ctx, [2] * (T + 10), np.tile([1, -1], T + 10), 2)
    assert len(kept) == 0 and balance == 1
    kept, balance = check_merged(ch, ctx, [2 * T, 2 * T + 2], np.concatenate([signs_of("open_close", 2 * T, None), -signs_of("open_close", 2 * T + 2, None)]), 3)
    assert len(kept) == 0 and balance == T + 1


def test_empty_and_single_row_inputs(ch, ctx):
    for n in (0, 1):
        key = np.arange(n, dtype=np.int64)
        for offs in ([0, n], [0, 0, n, n]):
            for value in (1, -1):
                got, balance = check(ch, ctx, [key], ASC, offs, np.full(n, value, dtype=np.int8))
                assert len(got) == n and balance == n


def test_the_version_is_the_last_key(ch, ctx, T):
    rng = np.random.Generator(np.random.PCG64(12))
    key = np.array([7, 7, 7, 7], dtype=np.int64)
    version = np.array([1, 2, 1, 2], dtype=np.uint32)
    sign = np.array([1, 1, -1, 1], dtype=np.int8)
    assert check(ch, ctx, [key, version], KV, [0, 2, 4], sign)[0].tolist() == [1, 3]       # (7, 1) cancels, (7, 2) keeps both
    assert check(ch, ctx, [key], ASC, [0, 2, 4], sign)[0].tolist() == [0, 3]               # without the version: + + - +
    # pairs that share the key, the version splitting a group on a tile edge: every first word ties
    for lens in ([T - 3, 3, 5, T + 1], [T, T], [2 * T - 1, 1, 1]):
        group, offs, order = layout(lens, 2)
        merged = np.concatenate([signs_of("half", length, rng) for length in lens])
        got, _ = check(ch, ctx, [np.zeros(len(group), dtype=np.uint32), group.astype(np.int16)], KV, offs, merged[order])
        counts = np.bincount(group[got.astype(np.int64)], minlength=len(lens))
        assert counts.tolist() == [abs(int(merged[a:a + length].astype(np.int64).sum())) for a, length in zip(np.cumsum(lens) - lens, lens)]


def test_float_versions_equal_as_order_words_share_a_group(ch, ctx):
    for dtype in (np.float64, np.float32):
        key = np.full(7, 7, dtype=np.int64)
        version = np.array([-0.0, np.nan, 0.0, np.nan, -0.0, 0.0, np.nan], dtype=dtype)
        sign = np.array([1, 1, -1, -1, 1, 1, 1], dtype=np.int8)
        got, balance = check(ch, ctx, [key, version], KV, R.offsets_of([2, 2, 3]), sign)
        assert got.tolist() == [4, 5, 6] and balance == 2      # the zeros: + - + +; the NaNs: + - +
        version = np.array([np.nan, -0.0, np.nan, 0.0, np.nan, -0.0, 0.0], dtype=dtype)      # NaN first
        got, _ = check(ch, ctx, [key, version], [(0, False, 1), (1, False, -1)], R.offsets_of([2, 2, 3]), sign)
        assert got.tolist() == [4, 5, 6]                        # the NaNs: + - +; the zeros: + - + +


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_key_dtype_in_both_directions(ch, ctx, T, dtype):
    rng = np.random.Generator(np.random.PCG64(90 + R.DTYPES.index(dtype)))
    offs = R.offsets_of([300, 0, 500, 3 * T - 791])
    n = int(offs[-1])
    for desc in (False, True):
        spec = [(0, desc, 1), (1, not desc, 1)]
        cols = R.sort_runs([R.random_column(rng, dtype, n, 5), R.random_column(rng, np.uint16, n, 3)], spec, offs)
        check(ch, ctx, cols, spec, offs, signs_of("half", n, rng))
    one = [(0, True, 1)]                                        # a single key column: one-byte keys take the sort chain
    cols = R.sort_runs([R.random_column(rng, dtype, n, 5)], one, offs)
    check(ch, ctx, cols, one, offs, signs_of("mostly_plus", n, rng))


def test_257_runs_and_a_group_with_a_row_of_every_run(ch, ctx, T):
    lens = [300, 1, 257, T + 40, 2, 600]
    group, offs, order = layout(lens, 257)
    assert np.all(np.diff(offs.astype(np.int64)) > 0)
    run = np.repeat(np.arange(257), np.diff(offs.astype(np.int64)))
    sign = np.where(run % 2 == 0, 1, -1).astype(np.int8)        # the signs follow the run order: the group of 257 rows alternates
    got, balance = check(ch, ctx, [group], ASC, offs, sign)
    assert np.bincount(group[got.astype(np.int64)], minlength=6)[2] == 1
    dev = [ctx.upload(group)]
    launches = ctx.counters()["KernelLaunches"]
    ch.versioned_collapsing_merge_rows(dev, ASC, offs, sign)
    # the sorted check 2, the sign check 2, the key build and nine rounds of two launches, then heads, tile, carry, decide, offsets, emit
    assert ctx.counters()["KernelLaunches"] - launches <= 2 + 2 + (1 + 2 * 9) + 6
    rng = np.random.Generator(np.random.PCG64(257))
    group, offs, order = layout([7] * 500, 257, rng)
    check(ch, ctx, [group], ASC, offs, signs_of("half", len(group), rng))


def test_a_bad_sign_names_the_lowest_row_and_leaves_nothing_behind(ch, ctx, T):
    group, offs, _ = layout([3, T, T + 7], 2)
    good = np.ones(len(group), dtype=np.int8)
    want = ch.versioned_collapsing_merge_rows([group], ASC, offs, good)      # handle-free: plain arrays in
    assert np.sort(want[0].numpy()).tolist() == list(range(len(group))) and want[1] == T + 7      # every row stays, in merged order
    for value in (0, 2, -2):
        sign = good.copy()
        sign[[2 * T + 1, 31, T + 5]] = value
        with pytest.raises(ch.ChgpuError) as e:
            ch.versioned_collapsing_merge_rows([group], ASC, offs, sign)
        assert e.value.code == ch._capi.ERR_BAD_ARGUMENTS and "row 31 " in str(e.value)
        again = ch.versioned_collapsing_merge_rows([group], ASC, offs, good)  # the same context goes on as if the call had not been made
        assert np.array_equal(again[0].numpy(), want[0].numpy()) and again[1] == want[1]


def test_unsorted_runs_are_refused_with_check(ch, ctx):
    key = np.array([1, 3, 2, 4], dtype=np.int64)
    sign = np.ones(4, dtype=np.int8)
    dev = [ctx.upload(key)]
    with pytest.raises(ch.ChgpuError) as e:
        ch.versioned_collapsing_merge_rows(dev, ASC, [0, 4], sign)
    assert e.value.code == ch._capi.ERR_BAD_ARGUMENTS and "row 2 " in str(e.value)
    rows, balance = ch.versioned_collapsing_merge_rows(dev, ASC, [0, 2, 4], sign)
    assert rows.numpy().tolist() == [0, 2, 1, 3] and balance == 1
    version = np.array([1, 0, 0, 1], dtype=np.uint8)                          # sorted on the key, not on (key, version)
    with pytest.raises(ch.ChgpuError) as e:
        ch.versioned_collapsing_merge_rows([ctx.upload(np.zeros(4, dtype=np.int64)), ctx.upload(version)], KV, [0, 4], sign)
    assert e.value.code == ch._capi.ERR_BAD_ARGUMENTS and "row 1 " in str(e.value)


def test_block_function_returns_the_indexed_columns(ch, ctx, T):
    rng = np.random.Generator(np.random.PCG64(21))
    spec = [(0, True, 1), (2, False, 1)]
    blocks = []
    for n in (T + 5, 0, 700):
        cols = [R.random_column(rng, np.int32, n, 30), rng.integers(0, 2**63, n).astype(np.uint64), R.random_column(rng, np.uint16, n, 2),
                np.where(rng.integers(0, 2, n) == 1, 1, -1).astype(np.int8)]
        blocks.append(R.sort_runs(cols, spec, R.offsets_of([n])))
    glued = [np.concatenate([b[k] for b in blocks]) for k in range(4)]
    offs = R.offsets_of([len(b[0]) for b in blocks])
    want_rows, want_balance = V.versioned_vector(R.describe(glued, spec), glued[3])
    cols, rows, balance = ch.versioned_collapsing_merge([[ctx.upload(c) for c in b] for b in blocks], spec, sign=3)
    assert np.array_equal(rows.numpy(), want_rows) and balance == want_balance and len(cols) == 4
    assert all(np.array_equal(c.numpy(), g[want_rows.astype(np.int64)]) for c, g in zip(cols, glued))
    assert len(want_rows) > 0
    cols, rows, balance = ch.versioned_collapsing_merge(blocks, spec, sign=3)    # plain arrays
    assert np.array_equal(rows.numpy(), want_rows) and balance == want_balance


def test_two_calls_give_identical_bits(ch, ctx, T):
    rng = np.random.Generator(np.random.PCG64(31))
    lens = rng.integers(1, 90, 400)
    group, offs, order = layout(lens, 3, rng)
    sign = signs_of("half", len(group), rng)[order]
    dev = [ctx.upload(group)]
    first = ch.versioned_collapsing_merge_rows(dev, ASC, offs, sign)
    second = ch.versioned_collapsing_merge_rows(dev, ASC, offs, sign)
    assert first[1] == second[1] and first[0].numpy().tobytes() == second[0].numpy().tobytes() and len(first[0].numpy()) > 0
