"""Plain-Python references for the String predicates (tests/test_string_predicates_abi.py, tests/test_gpu_string_predicates.py).

LIKE is restated twice, independently, and the CPU test requires the two to agree:
  like_regex   likePatternToRegexp as a Python regex, run with re.fullmatch(..., re.S) on the decoded str (fullmatch, not `$`: Python's
               `$` also matches before a trailing newline);
  like_bytes   the byte-level two-pointer matcher with the UTF-8 step the library documents for `_`.
Comparison, contains, startsWith and endsWith are Python's own bytes operations (bytes order is unsigned, the shorter one is smaller)."""
import random
import re

ALPHABET = ["a", "b", "ж", "€", "\n", "%", "_", "\\", "😀"]


def like_to_regex(pattern: str) -> str:
    out, i = [], 0
    while i < len(pattern):
        c = pattern[i]
        if c == "\\":
            if i + 1 == len(pattern):
                raise ValueError("LIKE pattern ends in a lone backslash")
            if pattern[i + 1] in "%_\\":
                out.append(re.escape(pattern[i + 1]))
                i += 1
            else:
                out.append(re.escape("\\"))     # a literal backslash; the next character is read as usual
        elif c == "%":
            out.append(".*")
        elif c == "_":
            out.append(".")
        else:
            out.append(re.escape(c))
        i += 1
    return "".join(out)


def like_regex(pattern: bytes, value: bytes) -> bool:
    return re.fullmatch(like_to_regex(pattern.decode("utf-8")), value.decode("utf-8"), re.S) is not None


def like_regex_compiled(pattern: bytes):
    rx = re.compile(like_to_regex(pattern.decode("utf-8")), re.S)
    return lambda value: rx.fullmatch(value.decode("utf-8")) is not None


ANY, ONE = "any", "one"


def like_tokens(pattern: bytes) -> list:
    """[int byte | ANY | ONE]"""
    toks, i = [], 0
    while i < len(pattern):
        c = pattern[i]
        if c == 0x5C:
            if i + 1 == len(pattern):
                raise ValueError("LIKE pattern ends in a lone backslash")
            if pattern[i + 1] in b"%_\\":
                toks.append(pattern[i + 1])
                i += 2
                continue
            toks.append(0x5C)
        elif c == 0x25:
            toks.append(ANY)
        elif c == 0x5F:
            toks.append(ONE)
        else:
            toks.append(c)
        i += 1
    return toks


def utf8_step(value: bytes, pos: int) -> int:
    """bytes of the UTF-8 sequence at pos by its lead byte, 0 when the continuation bytes are not 10xxxxxx inside the value"""
    b = value[pos]
    n = 1 if b < 0x80 else 2 if b & 0xE0 == 0xC0 else 3 if b & 0xF0 == 0xE0 else 4 if b & 0xF8 == 0xF0 else 0
    if n == 0 or pos + n > len(value):
        return 0
    return n if all(value[pos + k] & 0xC0 == 0x80 for k in range(1, n)) else 0


def like_bytes(pattern: bytes, value: bytes) -> bool:
    toks = like_tokens(pattern)
    h = p = mark = 0
    star = -1
    while True:
        if p < len(toks) and toks[p] is ANY:
            star, mark = p, h
            p += 1
            continue
        if p == len(toks) and h == len(value):
            return True
        if p < len(toks) and h < len(value):
            step = utf8_step(value, h) if toks[p] is ONE else (1 if toks[p] == value[h] else 0)
            if step:
                h += step
                p += 1
                continue
        if star < 0 or mark >= len(value):
            return False
        mark += 1                                   # the last % takes one byte more
        h, p = mark, star + 1


def random_text(rng: random.Random, max_chars: int = 12) -> bytes:
    return "".join(rng.choice(ALPHABET) for _ in range(rng.randint(0, max_chars))).encode("utf-8")


def random_pattern(rng: random.Random, max_chars: int = 12) -> bytes:
    p = random_text(rng, max_chars)
    try:
        like_tokens(p)
    except ValueError:
        p += b"a"           # a lone trailing backslash is an error, not a pattern: give it something to stand in front of
    return p


def cmp_ref(op: int, value: bytes, const: bytes) -> bool:
    return [value == const, value != const, value < const, value > const, value <= const, value >= const][op]
