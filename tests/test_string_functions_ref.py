"""The references the GPU tests of the String functions rest on (tests/string_func_ref.py), without a GPU: the two statements of the
substring window rule agree, the header's three examples hold, and the other references are pinned on values whose answer is plain."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import string_func_ref as R  # noqa: E402


def test_the_two_substring_rules_agree():
    checked = 0
    for size in range(0, 9):
        v = bytes(range(0x61, 0x61 + size))
        for offset in list(range(-12, 0)) + list(range(1, 13)):
            for length in [None] + list(range(0, 13)):
                a, b = R.substring(v, offset, length), R.substring_by_positions(v, offset, length)
                assert a == b, (v, offset, length, a, b)
                checked += 1
    assert checked == 9 * 24 * 14


def test_the_header_examples():
    for rule in (R.substring, R.substring_by_positions):
        assert rule(b"abc", -5, 3) == b"a"
        assert rule(b"abc", -5) == b"abc"
        assert rule(b"abc", 4) == b""
        assert rule(b"abc", 1) == b"abc" and rule(b"abc", 2, 1) == b"b" and rule(b"abc", -1) == b"c" and rule(b"abc", -3, 2) == b"ab"
        assert rule(b"abc", 3, 0) == b"" and rule(b"", 1) == b"" and rule(b"", -1, 5) == b""


def test_substring_at_the_ends_of_the_argument_types():
    v = b"abcdefgh"
    assert R.substring(v, R.INT64_MIN) == v and R.substring(v, R.INT64_MIN, 2**64 - 1) == v and R.substring(v, R.INT64_MIN, 2**63 - 8) == b"" and R.substring(v, R.INT64_MAX) == b""
    assert R.substring(v, -2**40, 2**40 - 6) == b"ab" and R.substring(v, 2, 2**64 - 1) == v[1:] and R.substring(v, -3, 2**63) == b"fgh"
    assert R.substring(v, R.INT64_MAX, 2**64 - 1) == b""


def test_length_utf8_counts_every_byte_that_is_no_continuation_byte():
    assert R.length_utf8("ж€😀a".encode()) == 4 and R.length("ж€😀a".encode()) == 10
    assert R.length_utf8(b"\x80\xbf") == 0 and R.length_utf8(b"\x7f\xc0\xff\x00") == 4
    assert R.length_utf8(b"") == 0


def test_case_maps_touch_the_letters_alone():
    edges = b"\x00@AZ[`az{\x7f\x80\xbf\xc0\xc1\xda\xe1\xfa\xff"
    assert R.lower(edges) == b"\x00@az[`az{\x7f\x80\xbf\xc0\xc1\xda\xe1\xfa\xff"
    assert R.upper(edges) == b"\x00@AZ[`AZ{\x7f\x80\xbf\xc0\xc1\xda\xe1\xfa\xff"
    assert R.lower(R.upper(edges)) == R.lower(edges)


def test_compare_and_position():
    assert R.cmp(b"ab", b"ab\0") < 0 and R.cmp(b"ab\0", b"ab\0\0") < 0 and R.cmp(b"ab\0\0", b"ab\1") < 0 and R.cmp(b"a\x7f", b"a\x80") < 0
    assert [R.cmp_op(op, b"a", b"b") for op in range(6)] == [False, True, True, False, True, False]
    assert [R.cmp_op(op, b"a", b"a") for op in range(6)] == [True, False, False, False, True, True]
    assert R.position(b"aaab", b"aab") == 2 and R.position(b"abc", b"") == 1 and R.position(b"", b"") == 1 and R.position(b"ab", b"abc") == 0
    assert R.position(b"xabab", b"ab") == 2 and R.position(b"", b"\0") == 0
    assert R.concat(b"a", b"", b"\0b") == b"a\0b"
