"""String predicates on the device against the plain-Python references of tests/string_ref.py: comparison with a constant, contains at
the edges of the flat kernel's tiles (the tile size is read from the kernel source), startsWith / endsWith, LIKE on a fixed table and on a
seeded fuzz, the error answers, and the mask driving ColumnString.filter and a filtered GROUP BY."""
import os
import random
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import string_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(REPO, "clickhouse_amd", "csrc", "string_kernels.hip")) as _f:
    _SRC = _f.read()
SM_TILE = int(re.search(r"constexpr u32 SM_TILE = (\d+);", _SRC).group(1))
SM_ROWS_LDS = int(re.search(r"constexpr u32 SM_ROWS_LDS = (\d+);", _SRC).group(1))
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 40]


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
        col = ch.ColumnString.from_values(ctx, values)
        assert col.chars.size() == 0 or col.chars.device_ptr % 16 == 0
        return col
    lens = np.fromiter((len(v) + 1 for v in values), dtype=np.uint64, count=len(values))
    chars = np.frombuffer(b"\xee" * misalign + b"".join(v + b"\0" for v in values) + slack + b"\xee" * 32, dtype=np.uint8)
    whole = ctx.upload(chars)
    view = whole.cut(misalign, int(lens.sum()) + len(slack))
    assert view.device_ptr % 16 == misalign and view.size() == int(lens.sum()) + len(slack)
    return ch.ColumnString(ctx.upload(np.cumsum(lens, dtype=np.uint64)), view, list(values))


def _check(col, values, method, arg, ref):
    """method(arg) and its negation against ref(value) over every row"""
    want = np.fromiter((ref(v) for v in values), dtype=np.uint8, count=len(values))
    got = getattr(col, method)(arg).numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (method, arg[:40], bad[:5], [values[i][:40] for i in bad[:5]], got[bad[:5]], want[bad[:5]])
    neg = getattr(col, method)(arg, negate=True).numpy()
    assert np.array_equal(neg, 1 - want), (method, arg[:40], "negate")
    return want


def _check_compare(ch, col, values, const):
    for op in (ch.EQ, ch.NE, ch.LT, ch.GT, ch.LE, ch.GE):
        want = np.fromiter((sr.cmp_ref(op, v, const) for v in values), dtype=np.uint8, count=len(values))
        got = col.compare(op, const).numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (op, const, [values[i] for i in bad[:5]], got[bad[:5]], want[bad[:5]])


def _edge_values(rng, consts):
    """values of every length of LENGTHS, and around every constant: itself, its prefixes, extensions, one byte changed up and down"""
    vals = [b"", b"a", b"a\0", b"a\0b", b"\xff", b"\x80", b"\x7f", b"b"]
    for n in LENGTHS:
        vals.append(bytes(rng.randrange(256) for _ in range(n)))
        vals.append(b"a" * n)
    for c in consts:
        vals += [c, c + b"\0", c + b"z", c + c, b"z" + c, c[:-1], c[: len(c) // 2], c[1:]]
        for pos in {0, len(c) // 2, len(c) - 1} if c else ():
            for d in (-1, 1):
                vals.append(c[:pos] + bytes([(c[pos] + d) % 256]) + c[pos + 1:])
    return vals


# ---- comparison -----------------------------------------------------------------------------------------------------------------------------
def test_compare_lengths_and_byte_order(ch, ctx):
    rng = random.Random(1)
    consts = [bytes(rng.randrange(256) for _ in range(n)) for n in LENGTHS] + [b"a" * n for n in LENGTHS] + [b"a", b"a\0", b"\xff", b"a\0b"]
    values = _edge_values(rng, consts)
    col = _column(ch, ctx, values)
    for const in consts:
        _check_compare(ch, col, values, const)
    # unsigned order, embedded zeros, prefixes -- spelled out
    small = [b"a", b"\xff", b"a\0b", b"a\0", b"ab", b""]
    c = _column(ch, ctx, small)
    assert c.compare(ch.GT, b"a").numpy().tolist() == [0, 1, 1, 1, 1, 0]
    assert c.compare(ch.GT, b"a\0").numpy().tolist() == [0, 1, 1, 0, 1, 0]
    assert c.compare(ch.EQ, b"a\0b").numpy().tolist() == [0, 0, 1, 0, 0, 0]
    assert c.compare(ch.LT, "a").numpy().tolist() == [0, 0, 0, 0, 0, 1]


@pytest.mark.parametrize("rows", [0, 1, 257, 5003])
def test_compare_row_counts(ch, ctx, rows):
    rng = random.Random(rows)
    values = [bytes(rng.choice(b"ab\xc3") for _ in range(rng.randrange(0, 20))) for _ in range(rows)]
    col = _column(ch, ctx, values)
    for const in (b"ab", b"abab\xc3\xc3ab\xc3a"):
        _check_compare(ch, col, values, const)
    assert col.compare(ch.EQ, b"ab").dtype == np.uint8 and col.compare(ch.EQ, b"ab").size() == rows


def test_brand_between_as_two_comparisons(ch, ctx):
    rng = random.Random(7)
    values = [b"MFGR#%d" % rng.randrange(2200, 2240) for _ in range(3000)] + [b"MFGR#222", b"MFGR#22211", b"MFGR#2228", b"MFGR#2221", b"MFGR#22280"]
    col = _column(ch, ctx, values)
    got = ch.and_(col.compare(ch.GE, "MFGR#2221"), col.compare(ch.LE, "MFGR#2228")).numpy()
    want = np.array([b"MFGR#2221" <= v <= b"MFGR#2228" for v in values], dtype=np.uint8)
    assert np.array_equal(got, want) and 0 < want.sum() < len(values)


@pytest.mark.parametrize("misalign", [1, 7, 15])
def test_compare_on_a_misaligned_chars_view(ch, ctx, misalign):
    # k_str_row_const reads the value 8 bytes per step at whatever address the view gives it
    rng = random.Random(1)
    consts = [bytes(rng.randrange(256) for _ in range(n)) for n in LENGTHS] + [b"a" * n for n in LENGTHS] + [b"a", b"a\0", b"\xff", b"a\0b"]
    values = _edge_values(rng, consts)
    col = _column(ch, ctx, values, misalign)
    for const in consts:
        _check_compare(ch, col, values, const)


# ---- contains: the flat kernel's edges -------------------------------------------------------------------------------------------------------
def _needle(m):
    return bytes(0x80 + (k * 7) % 0x70 for k in range(m))


def _tile_edge_values(needle, a0=0):
    """one occurrence starting at each of the last len(needle) - 1 bytes of a tile (on the 16-byte grid of an address with low bits a0)"""
    m = len(needle)
    unit = needle[:1] + b"x" * 7     # the filler keeps the kernel's first-byte test busy without ever holding the needle
    values, cur, starts = [], 0, []
    for k in range(1, m):
        boundary = 2 * k * SM_TILE - a0
        fill = boundary - k - 2 - cur - 1
        values.append((unit * (fill // 8 + 1))[:fill])
        cur += fill + 1
        values.append(b"yy" + needle + b"zz")
        starts.append(cur + 2)
        cur += m + 5
    assert [(s + a0) % SM_TILE for s in starts] == [SM_TILE - k for k in range(1, m)]
    values.append(needle[:-1])       # a last partial tile that ends in all but one byte of the needle
    return values


@pytest.mark.parametrize("m", [2, 16, 17, 256])
def test_contains_across_tile_boundaries(ch, ctx, m):
    needle = _needle(m)
    values = _tile_edge_values(needle)
    want = _check(_column(ch, ctx, values), values, "contains", needle, lambda v: needle in v)
    assert want.sum() == m - 1


@pytest.mark.parametrize("misalign", [1, 7, 15])
def test_contains_on_a_misaligned_chars_view(ch, ctx, misalign):
    for m in (2, 17):
        needle = _needle(m)
        values = [needle + b"q"] + _tile_edge_values(needle, misalign)     # the first occurrence starts on the view's first byte
        want = _check(_column(ch, ctx, values, misalign), values, "contains", needle, lambda v: needle in v)
        assert want.sum() == m
    values = [b"\xee\xee", b"a\xee", b"", b"\xee"]                          # the bytes around the view are \xee: none of them may count
    col = _column(ch, ctx, values, misalign)
    _check(col, values, "contains", b"\xee\xee", lambda v: b"\xee\xee" in v)
    _check(col, values, "ends_with", b"\xee", lambda v: v.endswith(b"\xee"))


def test_contains_and_the_terminating_zero(ch, ctx):
    for values, needle, want in [([b"ab"], b"b\0", [0]), ([b"ab\0"], b"b\0", [1]), ([b"ab", b"cd"], b"b\0c", [0, 0]), ([b"ab\0cd"], b"b\0c", [1]),
                                 ([b"xab", b"ab"], b"ab", [1, 1]),            # ends exactly at the value's last byte
                                 ([b"ab", b"abc", b""], b"abc", [0, 1, 0]),   # a needle longer than the value
                                 ([b"a", b"", b"a"], b"", [1, 1, 1]),         # the empty needle
                                 ([b"\0", b"", b"\0\0"], b"\0", [1, 0, 1])]:
        assert [int(needle in v) for v in values] == want
        got = _check(_column(ch, ctx, values), values, "contains", needle, lambda v: needle in v)
        assert got.tolist() == want


def test_contains_one_byte_needle_in_every_row(ch, ctx):
    rng = random.Random(3)
    values = [bytes(rng.choice(b"bcd") for _ in range(rng.randrange(0, 30))) + b"a" + bytes(rng.choice(b"bcd") for _ in range(rng.randrange(0, 30)))
              for _ in range(5000)]
    assert _check(_column(ch, ctx, values), values, "contains", b"a", lambda v: b"a" in v).all()
    _check(_column(ch, ctx, values), values, "contains", b"bc", lambda v: b"bc" in v)


def test_contains_tiles_of_empty_rows(ch, ctx):
    # whole tiles of terminators, and tiles with more rows than the kernel keeps offsets for in LDS that still hold hits
    values = [b"ab"] + [b""] * (2 * SM_TILE + 5) + [b"xab", b"b"] + [b""] * (SM_ROWS_LDS + 300) + [b"ab"] + [b""] * 700 + [b"a", b"b", b"ab"]
    col = _column(ch, ctx, values)
    for needle in (b"ab", b"b", b"a"):
        want = _check(col, values, "contains", needle, lambda v: needle in v)
        assert 0 < want.sum() < 10


@pytest.mark.parametrize("misalign", [1, 7, 15])
def test_contains_tiles_of_empty_rows_on_a_misaligned_view(ch, ctx, misalign):
    # the same column cut off the 16-byte grid: the search of a tile's rows in global memory (more than SM_ROWS_LDS of them) with a0 != 0
    values = [b"ab"] + [b""] * (2 * SM_TILE + 5) + [b"xab", b"b"] + [b""] * (SM_ROWS_LDS + 300) + [b"ab"] + [b""] * 700 + [b"a", b"b", b"ab"]
    col = _column(ch, ctx, values, misalign)
    for needle in (b"ab", b"b", b"a"):
        want = _check(col, values, "contains", needle, lambda v: needle in v)
        assert 0 < want.sum() < 10
    # a needle that starts with the zero byte: every terminator is a candidate and none may count
    for needle in (b"\0", b"\0\0", b"\0a", b"b\0"):
        assert _check(col, values, "contains", needle, lambda v: needle in v).sum() == 0


def test_contains_zero_needles_on_the_aligned_column_of_empty_rows(ch, ctx):
    values = [b"ab"] + [b""] * (2 * SM_TILE + 5) + [b"x\0b", b"\0"] + [b""] * (SM_ROWS_LDS + 300) + [b"a\0\0"] + [b""] * 700 + [b"a", b"\0\0", b"ab"]
    col = _column(ch, ctx, values)
    assert _check(col, values, "contains", b"\0", lambda v: b"\0" in v).sum() == 4
    assert _check(col, values, "contains", b"\0\0", lambda v: b"\0\0" in v).sum() == 2


def _slack_cases(a0):
    """(values, slack, needle, ends_on_a_tile_boundary): chars carries 2 x SM_TILE bytes behind the last value, and they hold the needle:
    completed across the last value's terminating zero, right behind it, again and again at a period that no tile size divides, and
    as the very last bytes of chars.  The last value ends on a tile boundary of a chars address with low bits a0, or one byte beside it."""
    out = []
    for needle in (b"needle", b"e\0n", _needle(17)):
        m = len(needle)
        cut = needle.index(0) if 0 in needle else m - 1           # value ..needle[:cut], its zero, slack needle[cut + 1:].. spells a \0 needle
        head, rest = needle[:cut], (needle[cut + 1:] if 0 in needle else needle[-1:])
        for total in (2 * SM_TILE - a0, 2 * SM_TILE - a0 - 1, 2 * SM_TILE - a0 + 1, 1000):
            values = [b"x" + needle[:-1], needle[1:], b"", b"has " + needle + b" inside", b"ends in " + needle, needle[:-1]]
            fill = total - sum(len(v) + 1 for v in values) - 1 - len(head)
            values.append(((needle[:1] + b"y" * 7) * (fill // 8 + 1))[:fill] + head)
            assert sum(len(v) + 1 for v in values) == total
            unit = needle + b"q" * (1 + m % 2)                    # an odd period: occurrences across every kind of tile boundary
            assert len(unit) % 2 == 1
            slack = (rest + unit * (2 * SM_TILE // len(unit) + 1))[:2 * SM_TILE - m] + needle
            assert len(slack) == 2 * SM_TILE and slack.count(needle) > SM_TILE // len(unit)
            out.append((values, slack, needle, (total + a0) % SM_TILE == 0))
    return out


@pytest.mark.parametrize("misalign", [0, 1, 7, 15])
def test_predicates_do_not_see_bytes_behind_the_last_value(ch, ctx, misalign):
    cases = _slack_cases(misalign)
    assert sum(c[3] for c in cases) == 3
    for values, slack, needle, _ in cases:
        col = _column(ch, ctx, values, misalign, slack)
        assert col.chars.size() == int(col.offsets.numpy()[-1]) + 2 * SM_TILE
        want = _check(col, values, "contains", needle, lambda v: needle in v)
        assert want.tolist() == [0, 0, 0, 1, 1, 0, 0]
        _check(col, values, "like", b"%" + needle + b"%", lambda v: needle in v)
        assert _check(col, values, "ends_with", needle, lambda v: v.endswith(needle)).tolist() == [0, 0, 0, 0, 1, 0, 0]
        _check(col, values, "ends_with", needle[:-1], lambda v: v.endswith(needle[:-1]))
        if max(needle) < 0x80:                                    # the general matcher, one lane per row
            p = b"%" + needle + b"_%"
            assert _check(col, values, "like", p, lambda v: sr.like_regex(p, v)).tolist() == [0, 0, 0, 1, 0, 0, 0]


def test_contains_in_one_value_spanning_many_tiles(ch, ctx):
    rng = random.Random(5)
    big = bytearray(rng.choice(b"abcdefgh") for _ in range(65536))
    needle = b"NEEDLE-17-bytes!!"
    big[30000:30000 + len(needle)] = needle
    values = [b"NEEDLE", b"x" * 100, bytes(big), b"EEDLE-17-bytes!!", b"tail"]
    want = _check(_column(ch, ctx, values), values, "contains", needle, lambda v: needle in v)
    assert want.tolist() == [0, 0, 1, 0, 0]


def test_contains_more_tiles_than_workgroups(ch, ctx):
    # chgpu_grid_for caps the launch at num_cus x 8 workgroups (2048): more than 8 MiB of chars at 4 KiB tiles takes the grid-stride loop
    rng = np.random.Generator(np.random.PCG64(11))
    n = 125_000
    lens = rng.integers(40, 120, size=n)
    raw = rng.integers(ord("a"), ord("p"), size=int(lens.sum()), dtype=np.uint8).tobytes()
    cuts = np.concatenate(([0], np.cumsum(lens)))
    values = [raw[cuts[i]:cuts[i + 1]] for i in range(n)]
    for i in range(0, n, 97):
        values[i] = values[i][:20] + b"google" + values[i][20:]
    col = _column(ch, ctx, values)
    assert col.chars.size() > 2048 * SM_TILE + SM_TILE
    want = _check(col, values, "contains", b"google", lambda v: b"google" in v)
    assert want.sum() >= n // 97
    _check(col, values, "like", b"%google%", lambda v: b"google" in v)
    _check(col, values, "contains", b"ab", lambda v: b"ab" in v)


# ---- startsWith / endsWith -------------------------------------------------------------------------------------------------------------------
def test_starts_with_and_ends_with(ch, ctx):
    rng = random.Random(9)
    needles = [bytes(rng.randrange(256) for _ in range(n)) for n in LENGTHS] + [b"a" * n for n in LENGTHS] + [b"a\0", b"\xff"]
    values = _edge_values(rng, needles)
    col = _column(ch, ctx, values)
    for needle in needles:
        _check(col, values, "starts_with", needle, lambda v: v.startswith(needle))
        _check(col, values, "ends_with", needle, lambda v: v.endswith(needle))
    assert col.starts_with(b"").numpy().all() and col.ends_with("").numpy().all()
    assert not col.starts_with(b"", negate=True).numpy().any()


@pytest.mark.parametrize("misalign", [1, 7, 15])
def test_starts_with_and_ends_with_on_a_misaligned_chars_view(ch, ctx, misalign):
    rng = random.Random(9)
    needles = [bytes(rng.randrange(256) for _ in range(n)) for n in LENGTHS] + [b"a" * n for n in LENGTHS] + [b"a\0", b"\xff"]
    values = _edge_values(rng, needles)
    col = _column(ch, ctx, values, misalign)
    for needle in needles:
        _check(col, values, "starts_with", needle, lambda v: v.startswith(needle))
        _check(col, values, "ends_with", needle, lambda v: v.endswith(needle))


# ---- LIKE -------------------------------------------------------------------------------------------------------------------------------------
LIKE_PATTERNS = ["", "%", "%%", "_", "a", "a%", "%a", "%a%", "a%b", "a%b%c", "%a_c%", "_%_", "a\\%b", "a\\_b", "\\\\", "ж_", "_€_", "%€",
                 "a%ab", "%aab", "%a_a", "a\\xb", "%\n%", "_\n"]
LIKE_VALUES = ["", "a", "b", "ab", "ba", "aa", "abc", "a\nc", "axc", "xa_cx", "aXbYc", "abbc", "a%b", "a_b", "axb", "\\", "\\\\", "a\\xb", "ж", "ж€", "жa",
               "ж😀", "€", "a€b", "😀€😀", "€€€", "x€", "aaab", "aaaab", "aaba", "aab", "abab", "\n", "a\n", "\n\n", "%", "_", "a%", "%a", "😀", "ab" * 20]


def test_like_fixed_table(ch, ctx):
    values = [v.encode("utf-8") for v in LIKE_VALUES]
    col = _column(ch, ctx, values)
    seen = 0
    for pattern in LIKE_PATTERNS:
        p = pattern.encode("utf-8")
        want = _check(col, values, "like", p, lambda v: sr.like_regex(p, v))
        assert [sr.like_bytes(p, v) for v in values] == want.astype(bool).tolist(), pattern
        seen += int(want.sum())
    assert seen > 100
    assert col.like("a%ab").numpy()[values.index(b"aaab")] == 1
    assert col.like("%aab").numpy()[values.index(b"aaaab")] == 1
    assert col.like("%a_a").numpy()[values.index(b"aaba")] == 1


@pytest.mark.parametrize("misalign", [1, 7, 15])
def test_like_fixed_table_on_a_misaligned_chars_view(ch, ctx, misalign):
    values = [v.encode("utf-8") for v in LIKE_VALUES]
    col = _column(ch, ctx, values, misalign)
    seen = 0
    for pattern in LIKE_PATTERNS:
        p = pattern.encode("utf-8")
        seen += int(_check(col, values, "like", p, lambda v: sr.like_regex(p, v)).sum())
    assert seen > 100


def test_like_seeded_fuzz(ch, ctx):
    rng = random.Random(424242)
    values = [sr.random_text(rng) for _ in range(2000)]
    col = _column(ch, ctx, values)
    pairs = matches = 0
    for _ in range(200):
        pattern = sr.random_pattern(rng)
        rx = sr.like_regex_compiled(pattern)
        want = np.fromiter((rx(v) for v in values), dtype=np.uint8, count=len(values))
        got = col.like(pattern).numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (pattern, [values[i] for i in bad[:5]], got[bad[:5]], want[bad[:5]])
        pairs += len(values)
        matches += int(want.sum())
    print(f"like fuzz: {matches} matches in {pairs} pairs")
    assert pairs == 400_000 and 0.01 < matches / pairs < 0.5, (matches, pairs)


def test_like_routes_agree_with_the_general_matcher(ch):
    # the same literal patterns down the general matcher (developer option) and down their own routes
    rng = random.Random(13)
    values = [sr.random_text(rng) for _ in range(3000)] + [b"ab" * 200, b"x" * 300 + b"ab"]
    c = ch.Context(0)
    try:
        col = _column(ch, c, values)
        direct = {n: col.contains(n).numpy() for n in (b"a", b"ab", "ж€".encode(), b"\n")}
        c.set_option("tune_str_contains_general", 1)
        for n, want in direct.items():
            assert np.array_equal(col.contains(n).numpy(), want), n
            assert np.array_equal(want, np.array([n in v for v in values], dtype=np.uint8))
    finally:
        c.close()


# ---- errors, end to end -----------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(ch, ctx):
    K = ch._capi
    chars = ctx.upload(np.frombuffer(b"ab\0cd\0", dtype=np.uint8))
    for offs in ([3, 3], [3, 2], [3, 7], [0, 6]):
        broken = ch.ColumnString(ctx.upload(np.array(offs, dtype=np.uint64)), chars)
        for call in (lambda: broken.compare(ch.EQ, b"ab"), lambda: broken.like("a%"), lambda: broken.contains(b"a"), lambda: broken.like("a_")):
            with pytest.raises(ch.ChgpuError) as e:
                call()
            assert e.value.code == K.ERR_BAD_ARGUMENTS
    good = _column(ch, ctx, [b"ab", b"cd"])
    for call in (lambda: good.like(b"x" * (K.STR_CONST_MAX + 1)), lambda: good.contains(b"x" * (K.STR_CONST_MAX + 1)),
                 lambda: good.compare(ch.EQ, b"x" * (K.STR_CONST_MAX + 1)), lambda: good.starts_with(b"x" * (K.STR_CONST_MAX + 1))):
        with pytest.raises(ch.ChgpuError) as e:
            call()
        assert e.value.code == K.ERR_NOT_IMPLEMENTED
    with pytest.raises(ch.ChgpuError) as e:
        good.like("ab\\")
    assert e.value.code == K.ERR_BAD_ARGUMENTS
    with pytest.raises(ch.ChgpuError) as e:
        ch.ColumnString(good.chars, good.chars).contains(b"a")      # offsets must be UInt64
    assert e.value.code == K.ERR_BAD_ARGUMENTS
    assert good.like("%d").numpy().tolist() == [0, 1]
    assert good.contains(b"x" * K.STR_CONST_MAX).numpy().tolist() == [0, 0]
    empty = _column(ch, ctx, [])
    for mask in (empty.like("a%"), empty.contains("a"), empty.compare(ch.LT, "a"), empty.like("a_")):
        assert mask.size() == 0 and mask.dtype == np.uint8


def test_like_mask_drives_filter_and_group_by(ch, ctx):
    rng = random.Random(21)
    hosts = [b"google.com", b"example.org", b"maps.google.de", b"amd.com", b"", b"goo"]
    values = [b"http://" + rng.choice(hosts) + b"/" + bytes(rng.choice(b"abc") for _ in range(rng.randrange(0, 9))) for _ in range(20_000)]
    keys = np.array([rng.randrange(50) for _ in values], dtype=np.uint32)
    vals = np.array([rng.randrange(-1000, 1000) for _ in values], dtype=np.int64)
    col = _column(ch, ctx, values)
    mask = col.like("%google%")
    want = np.array([b"google" in v for v in values], dtype=np.uint8)
    assert np.array_equal(mask.numpy(), want) and 0 < want.sum() < len(values)
    assert col.filter(mask).to_list() == [v for v, w in zip(values, want) if w]
    agg = ch.Aggregator(np.uint32, [(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None)], ctx=ctx)
    agg.execute_on_block(keys, [vals, None], filter=mask)
    got_keys, (sums, counts) = agg.convert_to_block()
    ref = {}
    for k, v, w in zip(keys.tolist(), vals.tolist(), want.tolist()):
        if w:
            s, c = ref.get(k, (0, 0))
            ref[k] = (s + v, c + 1)
    assert {int(k): (int(s), int(c)) for k, s, c in zip(got_keys, sums, counts)} == ref
