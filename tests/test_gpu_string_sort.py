"""chgpu_string_sort_permutation / chgpu_string_index on the device against tests/string_sort_ref.py: every permutation is compared
element by element with `sorted` over bytes, ascending and descending.  Columns have at most 2e5 rows."""
import os
import random
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import string_sort_ref as ssr  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(REPO, "clickhouse_amd", "csrc", "partition_kernels.hip")) as _f:
    _SRC = _f.read()
# rows per workgroup tile of a partition pass: PL_TILE = PT * PL_RPT
TILE = int(re.search(r"constexpr u32 PT = (\d+);", _SRC).group(1)) * int(re.search(r"#define PL_RPT_V (\d+)", _SRC).group(1))
assert re.search(r"constexpr u32 PL_TILE = PT \* PL_RPT;", _SRC)
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 24, 25, 40]
ALPHABETS = [b"\0a", b"ab", b"\0\x7f\x80\xff"]


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


@pytest.fixture(scope="module")
def ctx(ch):
    c = ch.Context(0)
    yield c
    c.close()


def _column(ch, ctx, values, misalign=0, slack=b""):
    """a ColumnString of `values`; misalign > 0: chars is a view `misalign` bytes into a padded buffer, offsets built for the view;
    slack: bytes that belong to chars but to no value (chars.size() > offsets.back())"""
    if not misalign and not slack:
        return ch.ColumnString.from_values(ctx, values)
    lens = np.fromiter((len(v) + 1 for v in values), dtype=np.uint64, count=len(values))
    chars = np.frombuffer(b"\xee" * misalign + b"".join(v + b"\0" for v in values) + slack + b"\xee" * 32, dtype=np.uint8)
    whole = ctx.upload(chars)
    view = whole.cut(misalign, int(lens.sum()) + len(slack))
    assert view.device_ptr % 16 == misalign and view.size() == int(lens.sum()) + len(slack)
    col = ch.ColumnString(ctx.upload(np.cumsum(lens, dtype=np.uint64)), view, list(values))
    col._whole = whole
    return col


def _same(got, want, what):
    got = [int(x) for x in got]
    assert len(got) == len(want), (what, len(got), len(want))
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (what, bad[:5], [got[i] for i in bad[:5]], [want[i] for i in bad[:5]])


def _check(ctx, col, values, perm_in=None, limit=0, directions=(False, True)):
    """get_permutation in both directions against the reference"""
    pin = ctx.upload(np.asarray(perm_in, dtype=np.uint64)) if perm_in is not None else None
    for descending in directions:
        got = col.get_permutation(pin, descending, limit).numpy()
        assert got.dtype == np.uint64
        _same(got, ssr.get_permutation(values, descending, perm_in, limit), (descending, limit))


def _random_values(rng, n, alphabet, lengths=LENGTHS):
    return [bytes(rng.choice(alphabet) for _ in range(rng.choice(lengths))) for _ in range(n)]


# ---------------------------------------------------------------- lengths and alphabets
@pytest.mark.parametrize("alphabet", ALPHABETS, ids=["zero_a", "a_b", "zero_7f_80_ff"])
def test_lengths_and_alphabets(ch, ctx, alphabet):
    rng = random.Random(len(alphabet) * 7919)
    values = _random_values(rng, 3 * TILE + 77, alphabet)
    _check(ctx, _column(ch, ctx, values), values)


def test_zero_byte_ladder(ch, ctx):
    values = [b"ab\1", b"ab\0\0", b"ab", b"ab\0", b"", b"ab\0\0\0\0\0\0", b"ab\0\0\0\0\0\0\0", b"ab\0\0\0\0\0", b"\x80", b"\x7f", b"\xff"] * 3
    col = _column(ch, ctx, values)
    _check(ctx, col, values)
    got = [values[int(i)] for i in col.get_permutation().numpy()]
    assert got[:3] == [b""] * 3 and got[3:6] == [b"ab"] * 3 and got[6:9] == [b"ab\0"] * 3 and got[-3:] == [b"\xff"] * 3


# ---------------------------------------------------------------- row counts around the partition pass's tile
@pytest.mark.parametrize("n", [0, 1, 2, TILE - 1, TILE, TILE + 1, 5 * TILE + 1234])
def test_row_counts_around_the_tile(ch, ctx, n):
    rng = random.Random(n)
    values = _random_values(rng, n, b"ab", [0, 1, 7, 8, 9, 17])
    col = _column(ch, ctx, values)
    _check(ctx, col, values)
    if n == 0:
        assert col.get_permutation().size() == 0


# ---------------------------------------------------------------- number of rounds
def test_all_values_equal_is_pure_stability(ch, ctx):
    for v in (b"", b"same", b"exactly8", b"a value of more than eight bytes"):
        values = [v] * (TILE + 5)
        col = _column(ch, ctx, values)
        for descending in (False, True):
            assert np.array_equal(col.get_permutation(None, descending).numpy(), np.arange(len(values), dtype=np.uint64))


def test_distinct_in_the_first_byte_is_one_round(ch, ctx):
    rng = random.Random(1)
    values = [bytes([b]) + bytes(rng.choice(b"xyz") for _ in range(rng.choice([0, 3, 7, 12, 30]))) for b in rng.sample(range(256), 256)]
    stats = []
    assert ssr.word_round_model(values, stats=stats) == ssr.get_permutation(values) and stats == [256]
    _check(ctx, _column(ch, ctx, values), values)


@pytest.mark.parametrize("at", [8, 16, 64])
def test_distinct_only_in_a_later_word(ch, ctx, at):
    rng = random.Random(at)
    prefixes = [bytes(rng.choice(b"pq") for _ in range(at)) for _ in range(6)]
    values = [rng.choice(prefixes) + bytes(rng.choice(b"\0ab\xff") for _ in range(rng.choice([0, 1, 5, 8]))) for _ in range(TILE + 300)]
    _check(ctx, _column(ch, ctx, values), values)


def test_prefixes_of_one_another(ch, ctx):
    rng = random.Random(5)
    values = [b"x" * k for k in range(41)] * 3 + [b"x" * k + b"\0" for k in range(41)]
    rng.shuffle(values)
    _check(ctx, _column(ch, ctx, values), values)


def test_one_segment_ends_at_round_1_another_at_round_5(ch, ctx):
    rng = random.Random(6)
    short = [b"A" * 8 + bytes([rng.randrange(256)]) for _ in range(500)]  # one segment after round 0, decided in round 1
    # a segment that splits in two in every round (so nothing is shared by all its rows) down to word 5
    deep = [b"B" * 8 + b"".join(rng.choice([b"x" * 8, b"y" * 8]) for _ in range(4)) + bytes(rng.choice(b"\0mn") for _ in range(rng.choice([0, 1, 3])))
            for _ in range(700)]
    values = short + deep + [b"C", b"", b"B" * 8]
    rng.shuffle(values)
    stats = []
    assert ssr.word_round_model(values, stats=stats) == ssr.get_permutation(values)
    assert len(stats) == 6 and stats[2] < stats[1] < stats[0]
    _check(ctx, _column(ch, ctx, values), values)


# ---------------------------------------------------------------- shared long prefix
def test_shared_long_prefix_costs_no_rounds(ch, ctx):
    rng = random.Random(7)
    short = [bytes([65 + i % 26, 65 + (i // 26) % 26, 65 + i // 676]) for i in range(4096)]
    assert len(set(short)) == 4096

    def launches(prefix):
        values = short + [prefix + bytes([rng.randrange(256)]) for _ in range(64)]
        random.Random(8).shuffle(values)
        col = _column(ch, ctx, values)
        before = ctx.counters()["KernelLaunches"]
        got = col.get_permutation().numpy()
        n = ctx.counters()["KernelLaunches"] - before
        _same(got, ssr.get_permutation(values), len(prefix))
        _same(col.get_permutation(None, True).numpy(), ssr.get_permutation(values, True), len(prefix))
        return n

    base = launches(b"PREFIX__")
    long_ = launches(b"PREFIX__" * 8192)  # 64 KiB: a word per round would take about 8000 rounds
    print(f"kernel launches: 8-byte prefix {base}, 64 KiB prefix {long_}")
    assert long_ <= 8 * base


# ---------------------------------------------------------------- misaligned and slack buffers
@pytest.mark.parametrize("misalign", [1, 3, 7])
def test_misaligned_chars(ch, ctx, misalign):
    rng = random.Random(misalign)
    values = _random_values(rng, TILE + 19, b"\0a\xff")
    _check(ctx, _column(ch, ctx, values, misalign), values)


def test_chars_with_slack_behind_the_last_value(ch, ctx):
    rng = random.Random(11)
    values = _random_values(rng, 1000, b"ab") + [b"ab" * 6]
    col = _column(ch, ctx, values, 0, slack=b"ab" * 40 + b"\0zz")
    assert col.chars.size() > int(col.offsets.numpy()[-1])
    _check(ctx, col, values)
    col = _column(ch, ctx, values, 3, slack=b"\xff" * 9)
    _check(ctx, col, values)


# ---------------------------------------------------------------- perm_in
def test_perm_in(ch, ctx):
    rng = random.Random(12)
    values = _random_values(rng, TILE + 500, b"ab", [0, 1, 8, 9, 17])
    col = _column(ch, ctx, values)
    n = len(values)
    _check(ctx, col, values, perm_in=rng.sample(range(n), n))               # a shuffled permutation of all rows
    _check(ctx, col, values, perm_in=rng.sample(range(n), n // 3))          # shorter than the column
    _check(ctx, col, values, perm_in=[rng.randrange(50) for _ in range(n)])  # repeated rows
    _check(ctx, col, values, perm_in=[])
    _check(ctx, col, values, perm_in=[3, n + 7, 2**40, 1])                  # entries beyond the column count as row 0


def test_sort_block_with_string_columns(ch, ctx):
    rng = random.Random(13)
    n = TILE + 321
    ints = np.array([rng.randrange(5) for _ in range(n)], dtype=np.int64)
    strs = _random_values(rng, n, b"ab", [0, 1, 8, 9, 10])
    icol, scol = ctx.upload(ints), _column(ch, ctx, strs)
    for description, ref in (([(0, False, 1), (1, False, 1)], [(ints, False, 1), (strs, False, 1)]),   # ORDER BY int, str
                             ([(1, False, 1), (0, True, 1)], [(strs, False, 1), (ints, True, 1)]),    # ORDER BY str, int DESC
                             ([(1, True, -1)], [(strs, True, 1)])):
        for limit in (0, 100):
            want = ssr.sort_block(ref)
            want = want[:limit] if limit else want
            (oi, os_), perm = ch.sort_block([icol, scol], description, limit)
            _same(perm.numpy(), want, (description, limit))
            assert oi.numpy().tolist() == [int(ints[r]) for r in want]
            assert os_.to_list() == [strs[r] for r in want]  # the carried String column arrives permuted
    # a String column that is only carried
    (oi, os_), perm = ch.sort_block([icol, scol], [(0, True, 1)])
    want = ssr.sort_block([(ints, True, 1)])
    _same(perm.numpy(), want, "carried")
    assert os_.to_list() == [strs[r] for r in want]


# ---------------------------------------------------------------- limit
def test_limit(ch, ctx):
    rng = random.Random(14)
    values = _random_values(rng, TILE + 100, b"ab", [0, 1, 2, 8, 9, 12, 17])
    col = _column(ch, ctx, values)
    n = len(values)
    for limit in (1, n - 1, n, n + 5):
        _check(ctx, col, values, limit=limit)
    full = ssr.get_permutation(values)
    # a limit inside a run of equal values
    inside_run = next(i for i in range(10, n - 1) if values[full[i - 1]] == values[full[i]] == values[full[i + 1]])
    _check(ctx, col, values, limit=inside_run)
    _check(ctx, col, values, limit=inside_run + 1)
    # a limit inside a segment still undecided after round 0: rows that share their first 8 bytes but are not all equal
    inside_seg = next(i for i in range(10, n - 1) if len(values[full[i]]) > 8 and values[full[i - 1]][:8] == values[full[i]][:8] == values[full[i + 1]][:8]
                      and values[full[i - 1]] != values[full[i + 1]])
    _check(ctx, col, values, limit=inside_seg)
    _check(ctx, col, values, limit=inside_seg + 1)
    # combined with perm_in
    perm_in = rng.sample(range(n), n // 2)
    for limit in (1, 77, n // 2 - 1, n // 2, n):
        _check(ctx, col, values, perm_in=perm_in, limit=limit)


# ---------------------------------------------------------------- chgpu_string_index
def _check_index(ctx, col, values, indexes, limit=0):
    out = col.index(ctx.upload(np.asarray(indexes, dtype=np.uint64)), limit)
    want = [values[i] for i in (indexes[:limit] if limit else indexes)]
    assert out.to_list() == want
    offs = out.offsets.numpy()
    assert out.size() == len(want)
    assert out.chars.size() == (int(offs[-1]) if len(want) else 0) == sum(len(v) + 1 for v in want)
    return out


@pytest.mark.parametrize("misalign", [0, 5])
def test_string_index(ch, ctx, misalign):
    rng = random.Random(15 + misalign)
    values = [b"", b"1234567", b"12345678", b"123456789", b"", b"\0", b"x" * 40, b"\xff\0\xff"] + _random_values(rng, TILE + 50, b"\0ab")
    col = _column(ch, ctx, values, misalign)
    n = len(values)
    _check_index(ctx, col, values, list(range(n)))
    _check_index(ctx, col, values, list(range(n - 1, -1, -1)))
    _check_index(ctx, col, values, [rng.randrange(8) for _ in range(3 * n)])  # repeated
    _check_index(ctx, col, values, [1, 2, 3, 3, 2, 1, 0, 4, 0])               # lengths 7, 8, 9 and 0 next to one another
    _check_index(ctx, col, values, [])
    idx = rng.sample(range(n), n)
    for limit in (1, 5, n - 1, n, n + 3):
        _check_index(ctx, col, values, idx, limit)
    # permuting by the sort's own result gives the sorted column
    perm = col.get_permutation()
    assert col.index(perm).to_list() == sorted(values)
    # and the result is an ordinary ColumnString: it sorts again
    out = _check_index(ctx, col, values, idx)
    _same(out.get_permutation().numpy(), ssr.get_permutation([values[i] for i in idx]), "resort")


# ---------------------------------------------------------------- error answers (each rejected by a check, or by a flag in a bounds-safe kernel)
def test_error_answers(ch, ctx):
    K = ch._capi
    values = [b"b", b"a", b"c"]
    col = _column(ch, ctx, values)
    u64 = lambda a: ctx.upload(np.asarray(a, dtype=np.uint64))
    # wrong types
    for bad in (ch.ColumnString(ctx.upload(np.array([2, 4, 6], dtype=np.uint32)), col.chars),
                ch.ColumnString(col.offsets, ctx.upload(np.zeros(6, dtype=np.int8)))):
        with pytest.raises(ch.ChgpuError) as e:
            bad.get_permutation()
        assert e.value.code == K.ERR_BAD_ARGUMENTS
        with pytest.raises(ch.ChgpuError) as e:
            bad.index(u64([0]))
        assert e.value.code == K.ERR_BAD_ARGUMENTS
    for bad_perm in (ctx.upload(np.array([0, 1], dtype=np.uint32)), ctx.upload(np.array([0, 1], dtype=np.int64))):
        with pytest.raises(ch.ChgpuError) as e:
            col.get_permutation(bad_perm)
        assert e.value.code == K.ERR_BAD_ARGUMENTS
        with pytest.raises(ch.ChgpuError) as e:
            col.index(bad_perm)
        assert e.value.code == K.ERR_BAD_ARGUMENTS
    # perm_in longer than the column
    with pytest.raises(ch.ChgpuError) as e:
        col.get_permutation(u64([0, 1, 2, 0]))
    assert e.value.code == K.ERR_SIZES_MISMATCH and "Size of permutation (4) is greater than the column (3)" in str(e.value)
    # decreasing offsets, offsets beyond chars
    for offs in ([2, 1, 6], [2, 2, 6], [2, 4, 7]):
        bad = ch.ColumnString(u64(offs), col.chars)
        with pytest.raises(ch.ChgpuError) as e:
            bad.get_permutation()
        assert e.value.code == K.ERR_BAD_ARGUMENTS
        with pytest.raises(ch.ChgpuError) as e:
            bad.index(u64([0]))
        assert e.value.code == K.ERR_BAD_ARGUMENTS
    # an index >= rows
    for idx in ([0, 3], [2**63], [1, 2, 0, 2**64 - 1]):
        with pytest.raises(ch.ChgpuError) as e:
            col.index(u64(idx))
        assert e.value.code == K.ERR_BAD_ARGUMENTS
    empty = _column(ch, ctx, [])
    with pytest.raises(ch.ChgpuError) as e:
        empty.index(u64([0]))
    assert e.value.code == K.ERR_BAD_ARGUMENTS
    assert empty.index(u64([])).size() == 0 and empty.get_permutation().size() == 0
    # the column still works after the refusals
    _check(ctx, col, values)
