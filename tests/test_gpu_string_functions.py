"""The String functions on the device (clickhouse_amd/csrc/string_func_kernels.hip) against tests/string_func_ref.py, bit for bit.

Every column is a `chars` VIEW into a larger buffer: `misalign` bytes off the 16-byte grid (0, 1, 7, 15) and with 2 x 4096 bytes behind
offsets.back() that belong to chars and to no value.  Those bytes are uppercase letters and copies of the needles -- NEEDLE_Z is
both completed across the last value's zero and whole directly behind it, NEEDLE follows -- and nothing of them may reach a result.
Value lengths sit around the 8- and 16-byte steps of the kernels, the bytes are the edges of the case ranges, of the continuation
test and of the unsigned compare, and one value of 70 000 bytes gives the flat sweep several tiles and the per-row walks a long row.
Every result ColumnString is fed back once (length() walks its offsets through the library's own validation)."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import string_func_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [0, 1, 63, 64, 65, 257, 2049]
MISALIGN = [0, 1, 7, 15]
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 255]
BYTES = bytes([0x00]) + b"@AZ[`az{" + bytes([0x7F, 0x80, 0xBF, 0xC0, 0xFF])
BIG = 70_000
NEEDLE = b"NEEDLE"
NEEDLE_Z = b"qZ\0qZ"          # the last value of every column ends in qZ, its zero follows, the slack begins with qZ\0qZ
SLACK = 2 * 4096
L = 9                         # a length present in every column of 63 rows or more


def _random_value(rng, n):
    return bytes(rng.choice(BYTES) for _ in range(n))


def _values(n, seed):
    rng = random.Random(seed * 1000 + n)
    values = [_random_value(rng, LENGTHS[(i + seed) % len(LENGTHS)] if i < 2 * len(LENGTHS) else rng.choice(LENGTHS)) for i in range(n)]
    if n >= 257:
        values[n // 2] = _random_value(rng, BIG)
    if n:
        values[-1] = values[-1][:15] + NEEDLE_Z[:2]
    return values


def _slack():
    letters = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ"
    head = NEEDLE_Z + NEEDLE
    return (head + letters * (SLACK // len(letters) + 1))[:SLACK]


def _column(ch, ctx, values, misalign=0):
    lens = np.fromiter((len(v) + 1 for v in values), dtype=np.uint64, count=len(values))
    used = int(lens.sum())
    whole = ctx.upload(np.frombuffer(b"Q" * misalign + b"".join(v + b"\0" for v in values) + _slack() + b"Q" * 32, dtype=np.uint8))
    view = whole.cut(misalign, used + SLACK)
    assert view.device_ptr % 16 == misalign and view.size() == used + SLACK
    return ch.ColumnString(ctx.upload(np.cumsum(lens, dtype=np.uint64)), view, list(values))


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


@pytest.fixture(scope="module")
def ctx(ch):
    c = ch.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cols(ch, ctx):
    """(n, misalign, which) -> (values, column), made once; `which` 0 and 1 are two different columns of the same n"""
    made = {}

    def get(n, misalign=0, which=0):
        key = (n, misalign, which)
        if key not in made:
            values = _values(n, 1 + which)
            made[key] = (values, _column(ch, ctx, values, misalign))
        return made[key]

    return get


def _strings(col):
    """the values of a result ColumnString, with the invariants every result keeps"""
    offs = col.offsets.numpy()
    chars = col.chars.numpy().tobytes()
    assert col.offsets.dtype == np.uint64 and col.chars.dtype == np.uint8
    assert len(chars) == (int(offs[-1]) if offs.shape[0] else 0)          # out_chars.rows == offsets.back()
    out, begin = [], 0
    for end in offs.tolist():
        assert end > begin and chars[end - 1] == 0
        out.append(chars[begin:end - 1])
        begin = end
    return out


def _check_strings(col, want):
    got = _strings(col)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g[:64], w[:64])
    # the result is a valid input: its lengths, through the library's own walk over its offsets
    assert col.length().numpy().tolist() == [len(w) for w in want]


def _numbers(column, dtype):
    assert column.dtype == dtype
    return column.numpy().tolist()


# ---- length, lengthUTF8, empty, notEmpty ----
@pytest.mark.parametrize("misalign", MISALIGN)
def test_lengths(cols, misalign):
    for n in ROWS:
        values, col = cols(n, misalign)
        assert _numbers(col.length(), np.uint64) == [R.length(v) for v in values]
        assert _numbers(col.length_utf8(), np.uint64) == [R.length_utf8(v) for v in values]
        assert _numbers(col.empty(), np.uint8) == [int(not v) for v in values]
        assert _numbers(col.not_empty(), np.uint8) == [int(bool(v)) for v in values]


def test_length_utf8_on_text_and_at_the_word_edges(ch, ctx):
    text = ["", "a", "ж", "€", "😀", "aж€😀", "ж" * 4, "€" * 3, "😀" * 2, "abcdefgж", "abcdefgh€", "x" * 7 + "😀" + "y" * 9]
    values = [t.encode() for t in text] + [b"\x80" * k for k in range(1, 18)] + [b"a" * k + b"\xbf" * (17 - k) for k in range(18)]
    col = _column(ch, ctx, values + [NEEDLE_Z[:2]], 7)
    assert _numbers(col.length_utf8(), np.uint64) == [R.length_utf8(v) for v in values] + [2]
    assert [R.length_utf8(t.encode()) for t in text] == [len(t) for t in text]      # on valid UTF-8 it is the number of code points


# ---- lower, upper ----
@pytest.mark.parametrize("misalign", MISALIGN)
def test_lower_and_upper(cols, misalign):
    for n in ROWS:
        values, col = cols(n, misalign)
        low, up = col.lower(), col.upper()
        _check_strings(low, [R.lower(v) for v in values])
        _check_strings(up, [R.upper(v) for v in values])
        assert low.offsets.numpy().tolist() == col.offsets.numpy().tolist()
        _check_strings(low.upper(), [R.upper(v) for v in values])          # lower().upper() == upper()


@pytest.mark.parametrize("misalign", MISALIGN)
def test_case_maps_over_every_byte_value_at_every_chunk_position(ch, ctx, misalign):
    # all 256 bytes at all 16 positions of a chunk, in values short enough that both edge chunks and whole chunks hold each of them
    values = [bytes((b + k) % 256 for b in range(256)) for k in range(16)] + [b"", b"A", b"z" * 15, b"Z" * 16, b"a" * 17, NEEDLE_Z[:2]]
    col = _column(ch, ctx, values, misalign)
    _check_strings(col.lower(), [R.lower(v) for v in values])
    _check_strings(col.upper(), [R.upper(v) for v in values])


# ---- substring ----
SUB_OFFSETS = [1, 2, L, L + 1, -1, -L, -L - 1, 2**40, -2**40, R.INT64_MIN, R.INT64_MAX]
SUB_LENGTHS = [None, 0, 1, L, 2**63, 2**64 - 1]


def _check_substrings(values, col):
    for offset in SUB_OFFSETS:
        for length in SUB_LENGTHS:
            want = [R.substring(v, offset, length) for v in values]
            _check_strings(col.substring(offset, length), want)


@pytest.mark.parametrize("n", ROWS)
def test_substring(cols, n):
    values, col = cols(n)
    assert n < 63 or any(len(v) == L for v in values)
    _check_substrings(values, col)


@pytest.mark.parametrize("misalign", MISALIGN[1:])
def test_substring_on_a_misaligned_chars_view(cols, misalign):
    _check_substrings(*cols(257, misalign))


def test_substring_windows_that_reach_in_front_of_the_value(ch, ctx, cols):
    values, col = cols(65)
    for offset, length in [(-5, 3), (-5, None), (4, None), (-300, 299), (-300, 46), (-256, 2), (-17, 17), (-16, 1), (256, 1), (255, 2**64 - 1),
                           (-2**40, 2**40 - 6), (R.INT64_MIN, 2**63 - 8), (R.INT64_MIN, 2**63 - 7), (R.INT64_MAX, 2**64 - 1)]:
        _check_strings(col.substring(offset, length), [R.substring(v, offset, length) for v in values])
    abc = _column(ch, ctx, [b"abc", b"abcdefgh" + NEEDLE_Z[:2]])
    assert _strings(abc.substring(-5, 3))[0] == b"a" and _strings(abc.substring(-5))[0] == b"abc" and _strings(abc.substring(4))[0] == b""
    with pytest.raises(ch.ChgpuError) as e:
        col.substring(0, 1)
    assert e.value.code == ch._capi.ERR_NOT_IMPLEMENTED


# ---- concat ----
@pytest.mark.parametrize("misalign", MISALIGN)
def test_concat(ch, cols, misalign):
    CS = ch.ColumnString
    for n in ROWS:
        a_values, a = cols(n, misalign, 0)
        b_values, b = cols(n, (16 - misalign) % 16 if misalign else 0, 1)
        _check_strings(CS.concat(a, b), [R.concat(x, y) for x, y in zip(a_values, b_values)])
        _check_strings(CS.concat(a, "/", b), [R.concat(x, b"/", y) for x, y in zip(a_values, b_values)])
        _check_strings(CS.concat(a, a), [R.concat(x, x) for x in a_values])
        _check_strings(CS.concat(b"", a, b""), list(a_values))
        _check_strings(CS.concat(b"\0", a, b"a\0\0b", b, b"\0"), [R.concat(b"\0", x, b"a\0\0b", y, b"\0") for x, y in zip(a_values, b_values)])
        eight = [a, b"<", b, a, b"\xff\0", b"", b, b">" * 9]
        _check_strings(CS.concat(*eight), [R.concat(x, b"<", y, x, b"\xff\0", b"", y, b">" * 9) for x, y in zip(a_values, b_values)])


def test_concat_of_empty_values_and_full_constants(ch, ctx, cols):
    CS = ch.ColumnString
    for n in (1, 65, 257):
        values = [b""] * n
        empty = _column(ch, ctx, values, 7)
        _check_strings(CS.concat(empty, empty), values)
        _check_strings(CS.concat(empty, b""), values)
        _check_strings(CS.concat(empty, b"x", empty), [b"x"] * n)
        other_values, other = cols(n, 1, 1)
        _check_strings(CS.concat(empty, other, empty), list(other_values))
    values, col = cols(65)
    full = bytes(range(256))                                               # CHGPU_STR_CONST_MAX bytes in one constant, and in three
    _check_strings(CS.concat(full, col), [full + v for v in values])
    _check_strings(CS.concat(full[:100], col, full[100:249], col, full[249:]), [full[:100] + v + full[100:249] + v + full[249:] for v in values])
    with pytest.raises(ch.ChgpuError) as e:
        CS.concat(full, col, b"x")
    assert e.value.code == ch._capi.ERR_NOT_IMPLEMENTED
    with pytest.raises(ch.ChgpuError) as e:
        CS.concat(col, cols(64)[1])
    assert e.value.code == ch._capi.ERR_SIZES_MISMATCH


# ---- compare_column ----
def _cmp_pairs(n):
    rng = random.Random(77 + n)
    base = _random_value(rng, 24)
    crafted = []
    for at in (0, 6, 7, 8, 9, 15, 16, 17, 23):                             # first difference at byte `at`
        lo, hi = base[:at] + b"\x7f" + base[at + 1:], base[:at] + b"\x80" + base[at + 1:]      # differ only in a byte >= 0x80 on one side
        crafted += [(lo, hi), (hi, lo), (lo[:at + 1], hi), (hi, lo[:at + 1])]
        crafted += [(base[:at] + b"\xbf", base[:at] + b"\xff"), (base[:at] + b"\xff" + b"a", base[:at] + b"\xbf" + b"z")]
    prefix = [b"ab", b"ab\0", b"ab\0\0", b"ab\1", b"", b"\0", b"a"]
    crafted += [(x, y) for x in prefix for y in prefix]                     # equal up to the shorter length
    for k in LENGTHS:
        v = _random_value(rng, k)
        crafted += [(v, v), (v, v + b"\0"), (v + b"\0", v)]
    pairs = [crafted[i % len(crafted)] if i < 3 * len(crafted) // 2 else (_random_value(rng, rng.choice(LENGTHS)), _random_value(rng, rng.choice(LENGTHS)))
             for i in range(n)]
    if n >= 257:
        big = _random_value(rng, BIG)
        pairs[100] = (big, big)
        pairs[101] = (big, big[:-1] + bytes([big[-1] ^ 0x80]))
        pairs[102] = (big[:-3], big)
    if n:
        pairs[-1] = (pairs[-1][0][:15] + NEEDLE_Z[:2], pairs[-1][1][:15] + NEEDLE_Z[:2])
    return [p[0] for p in pairs], [p[1] for p in pairs]


@pytest.mark.parametrize("misalign", MISALIGN)
def test_compare_column(ch, ctx, misalign):
    K = ch._capi
    for n in ROWS:
        a_values, b_values = _cmp_pairs(n)
        a, b = _column(ch, ctx, a_values, misalign), _column(ch, ctx, b_values, (misalign * 3) % 16)
        for op in (K.EQ, K.NE, K.LT, K.GT, K.LE, K.GE):
            want = [int(R.cmp_op(op, x, y)) for x, y in zip(a_values, b_values)]
            assert _numbers(a.compare_column(op, b), np.uint8) == want, (n, op)
            assert n < 63 or 0 < sum(want) < n
            assert _numbers(a.compare_column(op, a), np.uint8) == [int(R.cmp_op(op, x, x)) for x in a_values]       # a column against itself


def test_compare_column_agrees_with_compare_const(ch, ctx, cols):
    K = ch._capi
    values, col = cols(257)
    for const in (values[3], values[5], b"", b"a"):
        same = _column(ch, ctx, [const] * 256 + [const[:15] + NEEDLE_Z[:2]], 1)
        for op in (K.EQ, K.LT, K.GE):
            assert col.compare_column(op, same).numpy().tolist()[:256] == col.compare(op, const).numpy().tolist()[:256]


CMP_LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17]
CMP_BYTES = (0x00, 0x01, 0x7F, 0x80, 0xFF)


def _cmp_table():
    """(a, b) for every pair of lengths: equal over the common prefix of k bytes, and different in exactly one byte, at 0 or at k - 1; the
    two bytes there run through all ordered pairs of CMP_BYTES.  What the longer one has behind the prefix is random."""
    rng = random.Random(15)
    byte_pairs = [(x, y) for x in CMP_BYTES for y in CMP_BYTES if x != y]
    pairs, turn = [], 0
    for la in CMP_LENGTHS:
        for lb in CMP_LENGTHS:
            k = min(la, lb)
            prefix = _random_value(rng, k)
            a, b = prefix + _random_value(rng, la - k), prefix + _random_value(rng, lb - k)
            pairs.append((a, b))
            for p in sorted({0, k - 1} if k else ()):
                x, y = byte_pairs[turn % len(byte_pairs)]
                turn += 1
                pairs.append((a[:p] + bytes([x]) + a[p + 1:], b[:p] + bytes([y]) + b[p + 1:]))
    assert turn >= 2 * len(byte_pairs) and len(pairs) < 300
    pairs.append((NEEDLE_Z[:2], NEEDLE_Z[:2]))
    return [p[0] for p in pairs], [p[1] for p in pairs]


@pytest.mark.parametrize("misalign", MISALIGN)
def test_one_compare_table_through_both_entries(ch, ctx, misalign):
    """compare_column and compare share one ordered compare of two byte ranges (str_compare): the same pairs go through both, against
    the order of Python's bytes"""
    import operator
    K = ch._capi
    ops = {K.EQ: operator.eq, K.NE: operator.ne, K.LT: operator.lt, K.GT: operator.gt, K.LE: operator.le, K.GE: operator.ge}
    a_values, b_values = _cmp_table()
    a, b = _column(ch, ctx, a_values, misalign), _column(ch, ctx, b_values, (misalign * 3) % 16)
    for op, holds in ops.items():
        want = [int(holds(x, y)) for x, y in zip(a_values, b_values)]
        assert 0 < sum(want) < len(want)
        assert _numbers(a.compare_column(op, b), np.uint8) == want, op
    for const in sorted(set(b_values)):
        for op, holds in ops.items():
            assert _numbers(a.compare(op, const), np.uint8) == [int(holds(x, const)) for x in a_values], (op, const)


# ---- position ----
def _position_values(needle):
    m = len(needle)
    other = b"#" if b"#" not in needle else b"$"
    values = [needle, needle + other, other + needle, needle + needle, needle[:-1], needle[1:], b"", needle[:1]]
    for pad in range(0, 18):                                                # the needle at the start, at the end, across the 8-byte word edges
        values += [other * pad + needle, other * pad + needle + other * 3, other * pad + needle[:-1] + other + needle + needle]
        values += [needle[:1] * pad + needle, needle[:-1] * 2 + other * pad + needle[:m - 1]]
    values += [other * 254 + needle[:1], other * 255, (needle[:-1] + other) * 40 + needle + other * 5]
    return values + [other + NEEDLE_Z[:2]]


POSITION_NEEDLES = [b"a", b"ab", b"aab", b"abcdefg", b"abcdefgh", b"abcdefghi", b"aaaaaaaaaaaaaaaaa", b"\0", b"a\0b", b"\xff\x80", bytes(range(1, 256)) + b"\0",
                    NEEDLE, NEEDLE_Z]


@pytest.mark.parametrize("misalign", MISALIGN)
def test_position_of_crafted_needles(ch, ctx, misalign):
    for needle in POSITION_NEEDLES:
        values = _position_values(needle)
        col = _column(ch, ctx, values, misalign)
        want = [R.position(v, needle) for v in values]
        assert _numbers(col.position(needle), np.uint64) == want, needle[:16]
        assert want[-1] == 0 and sum(1 for w in want if w) > 40
        assert col.contains(needle).numpy().tolist() == [int(w != 0) for w in want]       # CHGPU_STR_CONTAINS is position != 0


@pytest.mark.parametrize("misalign", MISALIGN)
def test_position_on_the_random_columns(cols, misalign):
    for n in ROWS:
        values, col = cols(n, misalign)
        for needle in (b"a", b"\0", b"aZ", b"\xff\x80", b"{\x7f\x80", NEEDLE, NEEDLE_Z, b"qZ", b"q", b"", values[n // 2][-9:] if n else b"x"):
            assert _numbers(col.position(needle), np.uint64) == [R.position(v, needle) for v in values], (n, needle)


def test_position_never_takes_in_a_terminator_or_the_next_row(ch, ctx):
    values = [b"aaab", b"ab", b"c", b"ab", b"\0c", b"ab\0c", b"a", b"b\0c", NEEDLE_Z[:2]]
    col = _column(ch, ctx, values, 15)
    assert col.position(b"aab").numpy().tolist() == [2, 0, 0, 0, 0, 0, 0, 0, 0]              # overlapping candidates
    assert col.position(b"ab\0c").numpy().tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0]            # ab | c is completed across a terminator only
    assert col.position(b"b\0c").numpy().tolist() == [0, 0, 0, 0, 0, 2, 0, 1, 0]
    assert col.position(b"ab" * 3).numpy().tolist() == [0] * 9                                # longer than every value
    assert col.position(b"").numpy().tolist() == [1] * 9
    assert col.position(NEEDLE_Z).numpy().tolist() == [0] * 9 and col.position(NEEDLE).numpy().tolist() == [0] * 9      # the slack
    for n in (1, 64, 65, 2049):
        empty = _column(ch, ctx, [b""] * n, 1)
        for needle in (b"\0", b"\0\0"):                                       # every terminator is a candidate and none may count
            assert empty.position(needle).numpy().tolist() == [0] * n
        assert empty.position(b"").numpy().tolist() == [1] * n
    with pytest.raises(ch.ChgpuError) as e:
        col.position(b"x" * 257)
    assert e.value.code == ch._capi.ERR_NOT_IMPLEMENTED


NEEDLE_LENGTHS = [1, 7, 8, 9, 16, 17, 255, 256]


def _needle_table(m, misalign):
    """(values, needles) for a needle N of m bytes: N at the front, at the end and across an edge of the 16-byte grid of the chars
    address; near misses in N's last byte alone, which is the value's last byte or its terminator; N without its last byte in front
    of a row that begins with that byte.  NZ and NX are N with a zero as its last byte / in front of its last byte: only a terminator
    (and the next row's first byte) would complete them."""
    N = bytes(0x41 + i % 26 for i in range(m))
    last, miss, o = N[-1:], bytes([N[-1] ^ 0x20]), b"#"
    values = [N, N + o, o + N, o * 3 + N, N + N, N[:-1] + miss, o + N[:-1] + miss, miss + N[:-1], N[:-1], last + o, N[:-2], last, o + N[:-1], N[1:], b""]

    def straddling(tail):
        # the pad that puts N's first byte on the last byte of a 16-byte chunk (N itself, when it is one byte)
        at = misalign + sum(len(v) + 1 for v in values)
        return o * ((15 - at) % 16) + N + tail

    values += [straddling(b"")]
    values += [straddling(o * 3)]
    values += [straddling(N[:-1] + miss)]
    needles = [N, N[:-1] + b"\0"] + ([N[:-2] + b"\0" + last] if m >= 2 else [])
    return values + [o + NEEDLE_Z[:2]], needles


@pytest.mark.parametrize("misalign", MISALIGN)
def test_one_needle_table_through_four_entries(ch, ctx, misalign):
    """starts_with, ends_with, contains and position share one test of m bytes against the constant (str_equals_words): the same
    haystacks and needles go through all four"""
    for m in NEEDLE_LENGTHS:
        values, needles = _needle_table(m, misalign)
        col = _column(ch, ctx, values, misalign)
        assert (col.chars.device_ptr + sum(len(v) + 1 for v in values[:15]) + values[15].index(needles[0])) % 16 == 15
        for needle in needles:
            assert _numbers(col.starts_with(needle), np.uint8) == [int(v.startswith(needle)) for v in values], (m, needle[-3:])
            assert _numbers(col.ends_with(needle), np.uint8) == [int(v.endswith(needle)) for v in values], (m, needle[-3:])
            assert _numbers(col.contains(needle), np.uint8) == [int(needle in v) for v in values], (m, needle[-3:])
            assert _numbers(col.position(needle), np.uint64) == [v.find(needle) + 1 for v in values], (m, needle[-3:])
        found = [v.find(needles[0]) + 1 for v in values]
        assert sum(1 for f in found if f) >= 8 and sum(1 for f in found if not f) >= 8


# ---- broken offsets ----
def test_offsets_that_break_the_invariant_are_bad_arguments(ch, ctx):
    chars = ctx.upload(np.zeros(64, dtype=np.uint8))
    good = ch.ColumnString.from_values(ctx, [b"ab", b"c"])
    for offsets in ([3, 3], [3, 2], [0, 5], [3, 65]):
        bad = ch.ColumnString(ctx.upload(np.array(offsets, dtype=np.uint64)), chars)
        calls = [bad.length, bad.length_utf8, bad.lower, lambda: bad.substring(1), lambda: bad.position(b"a"), lambda: bad.compare_column(0, bad),
                 lambda: good.compare_column(0, bad), lambda: ch.ColumnString.concat(bad, b"x"), lambda: ch.ColumnString.concat(good, bad)]
        for call in calls:
            with pytest.raises(ch.ChgpuError) as e:
                call()
            assert e.value.code == ch._capi.ERR_BAD_ARGUMENTS, offsets


# ---- allocation failure ----
ALLOC_CALLS = ["length", "map_case", "cmp_columns", "substring", "concat", "position"]
ALLOCATIONS = {"length": 1, "map_case": 2, "cmp_columns": 1, "substring": 3, "concat": 3, "position": 1}     # results, and the one pool allocation
# KernelLaunches one call adds, as a run of the library of the commit before str_one_column / str_build_values printed them.  The walk
# over a column's offsets counts one, a scan its three kernels: length 1 + 1, map_case 1 + 2, cmp_columns 2 + 1, substring 1 + 2 + 3,
# concat 2 + 2 + 3, position 1 + 1.
LAUNCHES = {"length": 2, "map_case": 3, "cmp_columns": 3, "substring": 6, "concat": 7, "position": 2}


def _alloc_call(ch, cols, name):
    """(call, reference) of one entry point over the columns of 257 rows; the call returns plain host values"""
    values, col = cols(257, 7)
    other_values, other = cols(257, 1, 1)
    return {
        "length": (lambda: col.length_utf8().numpy().tolist(), [R.length_utf8(v) for v in values]),
        "map_case": (lambda: _strings(col.lower()), [R.lower(v) for v in values]),
        "cmp_columns": (lambda: col.compare_column(ch._capi.LT, other).numpy().tolist(), [int(x < y) for x, y in zip(values, other_values)]),
        "substring": (lambda: _strings(col.substring(-L, 4)), [R.substring(v, -L, 4) for v in values]),
        "concat": (lambda: _strings(ch.ColumnString.concat(col, b"/", other)), [x + b"/" + y for x, y in zip(values, other_values)]),
        "position": (lambda: col.position(b"aZ").numpy().tolist(), [R.position(v, b"aZ") for v in values]),
    }[name]


@pytest.mark.parametrize("name", ALLOC_CALLS)
def test_the_kernel_launches_of_a_call_are_as_they_were(ch, ctx, cols, name):
    call, want = _alloc_call(ch, cols, name)
    before = ctx.counters()["KernelLaunches"]
    assert call() == want
    delta = ctx.counters()["KernelLaunches"] - before
    print(f"KernelLaunches[{name}] = {delta}")
    assert delta == LAUNCHES[name], (name, delta)


@pytest.mark.parametrize("name", ALLOC_CALLS)
def test_a_refused_allocation_is_an_error_and_the_same_call_then_succeeds(ch, ctx, cols, name):
    call, want = _alloc_call(ch, cols, name)

    def rows_and_bytes():
        c = ctx.counters()
        return {k: v for k, v in c.items() if k != "KernelLaunches"}

    failed_at = []
    for nth in range(1, 16):
        before = rows_and_bytes()
        ctx.set_option("test_string_fail_alloc", nth)
        refused = None
        try:
            got = call()
        except ch.ChgpuError as e:
            refused = e
        finally:
            ctx.set_option("test_string_fail_alloc", 0)
        if refused is None:
            assert got == want          # the call makes fewer than nth allocations: it went through
            break
        assert refused.code == ch._capi.ERR_OOM and "test_string_fail_alloc" in str(refused), (nth, str(refused))
        assert rows_and_bytes() == before
        failed_at.append(nth)
        assert call() == want           # nothing of the failed call is left behind
    assert failed_at == list(range(1, ALLOCATIONS[name] + 1)), failed_at


# ---- the C++ shim ----
def test_shim_members_against_host_loops(tmp_path):
    exe = tmp_path / "string_functions_shim_driver"
    lib_dir = os.path.join(REPO, "clickhouse_amd")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-Wall", os.path.join(REPO, "tests", "string_functions_shim_driver.cpp"), "-L" + lib_dir, "-lchgpu",
                        "-lpthread", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "string_functions_shim_driver OK" in r.stdout, r.stdout + r.stderr
