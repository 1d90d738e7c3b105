"""References of the String functions (clickhouse_amd/csrc/string_func_kernels.hip) as plain Python `bytes` operations.

The substring window rule of include/chgpu.h is restated twice, once by index arithmetic and once by slicing a padded list of positions;
tests/test_string_functions_ref.py requires the two to agree."""

INT64_MIN, INT64_MAX = -2**63, 2**63 - 1


def length(v: bytes) -> int:
    return len(v)


def length_utf8(v: bytes) -> int:
    """every byte that is not a continuation byte (10xxxxxx), on valid and invalid UTF-8 alike"""
    return sum(1 for b in v if (b & 0xC0) != 0x80)


def lower(v: bytes) -> bytes:
    return bytes(b ^ 0x20 if 0x41 <= b <= 0x5A else b for b in v)


def upper(v: bytes) -> bytes:
    return bytes(b ^ 0x20 if 0x61 <= b <= 0x7A else b for b in v)


def cmp(a: bytes, b: bytes) -> int:
    """unsigned bytes over the common prefix, then the shorter value is the smaller: Python's own order of bytes"""
    return (a > b) - (a < b)


def cmp_op(op: int, a: bytes, b: bytes) -> bool:
    c = cmp(a, b)
    return [c == 0, c != 0, c < 0, c > 0, c <= 0, c >= 0][op]   # EQ, NE, LT, GT, LE, GE


def substring(v: bytes, offset: int, length=None) -> bytes:
    """by index arithmetic (Python integers do not overflow: nothing needs to saturate here)"""
    assert offset != 0 and (length is None or length >= 0)
    size = len(v)
    start = offset - 1 if offset > 0 else size + offset   # may be negative
    end = size if length is None else start + length
    lo, hi = max(start, 0), min(end, size)
    return v[lo:hi] if hi > lo else b""


PAD = 64


def substring_by_positions(v: bytes, offset: int, length=None) -> bytes:
    """by slicing the list of positions PAD places in front of the value, the value's own indexes, PAD places behind it: a window is
    `length` consecutive places of that list, and what it holds of the value's indexes is the result.  For |offset| and length up to PAD."""
    assert offset != 0 and abs(offset) <= PAD and (length is None or 0 <= length <= PAD)
    size = len(v)
    places = [None] * PAD + list(range(size)) + [None] * PAD
    first = PAD + (offset - 1 if offset > 0 else size + offset)
    assert first >= 0
    window = places[first:] if length is None else places[first:first + length]
    return bytes(v[p] for p in window if p is not None)


def concat(*parts: bytes) -> bytes:
    return b"".join(parts)


def position(haystack: bytes, needle: bytes) -> int:
    """1-based byte index of the first occurrence, 0 without one; the empty needle is found at 1"""
    return haystack.find(needle) + 1
