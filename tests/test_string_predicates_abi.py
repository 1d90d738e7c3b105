"""String predicates without a GPU: the error channel of the new entry points, the host-only LIKE pattern compiler pinned on a table
(route, unescaped literal, token counts), the agreement of the two Python references the GPU tests rest on, and a syntax-only compile of
the five new members of the C++ shim's ColumnString (tests/string_predicates_driver.cpp)."""
import ctypes as C
import os
import random
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import string_ref as sr  # noqa: E402


@pytest.fixture(scope="module")
def K():
    from clickhouse_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    _capi.lib()
    return _capi


def _expect_bad(K, rc):
    assert rc == K.ERR_BAD_ARGUMENTS
    with pytest.raises(K.ChgpuError) as e:
        K.check(rc)
    assert e.value.code == K.ERR_BAD_ARGUMENTS and "NULL" in str(e.value)


def test_constants_match_the_header(K):
    with open(os.path.join(REPO, "include", "chgpu.h")) as f:
        text = f.read()
    for name in ("LIKE", "CONTAINS", "STARTS_WITH", "ENDS_WITH", "ROUTE_EQUALS", "ROUTE_STARTS_WITH", "ROUTE_ENDS_WITH", "ROUTE_CONTAINS", "ROUTE_GENERAL"):
        assert f"CHGPU_STR_{name} = {getattr(K, 'STR_' + name)}" in text, name
    assert f"#define CHGPU_STR_CONST_MAX {K.STR_CONST_MAX}" in text
    assert K.STR_CONST_MAX >= 255
    assert C.sizeof(K.LikePlan) == 5 * 4 + K.STR_CONST_MAX // 8 + 2 * K.STR_CONST_MAX


def test_cmp_const_rejects_null(K):
    out = C.c_void_p()
    _expect_bad(K, K.lib().chgpu_string_cmp_const(None, None, None, K.EQ, b"a", 1, C.byref(out)))


def test_match_const_rejects_null(K):
    out = C.c_void_p()
    for kind in (K.STR_LIKE, K.STR_CONTAINS, K.STR_STARTS_WITH, K.STR_ENDS_WITH):
        _expect_bad(K, K.lib().chgpu_string_match_const(None, None, None, kind, b"a", 1, 0, C.byref(out)))


def test_like_compile_rejects_null(K):
    _expect_bad(K, K.lib().chgpu_like_compile(b"a", 1, None))
    plan = K.LikePlan()
    _expect_bad(K, K.lib().chgpu_like_compile(None, 1, C.byref(plan)))


E, S, N, CT, G = "ROUTE_EQUALS", "ROUTE_STARTS_WITH", "ROUTE_ENDS_WITH", "ROUTE_CONTAINS", "ROUTE_GENERAL"
PATTERN_TABLE = [
    # pattern, route, literal, n_percent, n_underscore
    (b"", E, b"", 0, 0),
    (b"abc", E, b"abc", 0, 0),
    (b"abc%", S, b"abc", 1, 0),
    (b"%abc", N, b"abc", 1, 0),
    (b"%abc%", CT, b"abc", 2, 0),
    (b"%", CT, b"", 1, 0),
    (b"%%", CT, b"", 2, 0),
    (b"a\\%b", E, b"a%b", 0, 0),
    (b"a\\\\%", S, b"a\\", 1, 0),
    (b"a\\xb", E, b"a\\xb", 0, 0),
    (b"a\\_b", E, b"a_b", 0, 0),
    (b"a_c", G, b"", 0, 1),
    (b"a%b", G, b"", 1, 0),
    (b"%a%b%", G, b"", 3, 0),
    ("ж_%€\\%_".encode(), G, b"", 1, 2),
    ("%ж€%".encode(), CT, "ж€".encode(), 2, 0),
    (b"a\0b%", S, b"a\0b", 1, 0),
    (b"\xff%", S, b"\xff", 1, 0),
    (b"%" + b"x" * 254 + b"%", CT, b"x" * 254, 2, 0),
    (b"x" * 256, E, b"x" * 256, 0, 0),
]


@pytest.mark.parametrize("pattern,route,literal,n_percent,n_underscore", PATTERN_TABLE, ids=[repr(p[0][:12]) for p in PATTERN_TABLE])
def test_like_pattern_route(K, pattern, route, literal, n_percent, n_underscore):
    from clickhouse_amd import like_compile
    plan = like_compile(pattern)
    assert plan["route"] == getattr(K, "STR_" + route)
    assert plan["literal"] == literal
    assert (plan["n_percent"], plan["n_underscore"]) == (n_percent, n_underscore)
    # the token string the general matcher walks is the reference's own tokenisation, runs of % collapsed
    want = []
    for t in sr.like_tokens(pattern):
        if t is sr.ANY and want and want[-1] is sr.ANY:
            continue
        want.append(t)
    got = [(sr.ANY if b == 0x25 else sr.ONE) if m else b for b, m in zip(plan["tokens"], plan["token_is_meta"])]
    assert got == want


def test_like_pattern_errors(K):
    from clickhouse_amd import ChgpuError, like_compile
    for bad in (b"abc\\", b"\\", b"a\\\\\\"):
        with pytest.raises(ChgpuError) as e:
            like_compile(bad)
        assert e.value.code == K.ERR_BAD_ARGUMENTS and "backslash" in str(e.value)
    with pytest.raises(ChgpuError) as e:
        like_compile(b"x" * (K.STR_CONST_MAX + 1))
    assert e.value.code == K.ERR_NOT_IMPLEMENTED
    assert like_compile("a\\\\")["literal"] == b"a\\"      # an escaped backslash at the end is fine
    assert like_compile("needle")["literal"] == b"needle"   # str arguments are UTF-8


def test_the_two_like_references_agree():
    rng = random.Random(20240517)
    pairs = matches = 0
    for _ in range(300):
        pattern = sr.random_pattern(rng)
        rx = sr.like_regex_compiled(pattern)
        for _ in range(400):
            value = sr.random_text(rng)
            a, b = rx(value), sr.like_bytes(pattern, value)
            assert a == b, (pattern, value, a, b)
            pairs += 1
            matches += a
    assert pairs == 120_000 and 0.01 < matches / pairs < 0.5, (pairs, matches)


def test_like_reference_spot_checks():
    for pattern, value, want in [(b"a%ab", b"aaab", True), (b"%aab", b"aaaab", True), (b"%a_a", b"aaba", True), (b"a_c", b"a\nc", True),
                                 ("ж_".encode(), "ж€".encode(), True), ("_".encode(), "€".encode(), True), (b"_", b"", False),
                                 (b"a\\%b", b"a%b", True), (b"a\\%b", b"axb", False), (b"\\\\", b"\\", True), (b"a\\xb", b"a\\xb", True),
                                 (b"%", b"", True), (b"_%_", b"a", False), (b"_%_", "ж😀".encode(), True), (b"abc", b"abc\n", False)]:
        assert sr.like_regex(pattern, value) == want, (pattern, value)
        assert sr.like_bytes(pattern, value) == want, (pattern, value)


def test_shim_string_predicates_compile():
    # syntax-only: the five members of chgpu::ColumnString as a driver uses them (no GPU, no library)
    src = os.path.join(REPO, "tests", "string_predicates_driver.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
