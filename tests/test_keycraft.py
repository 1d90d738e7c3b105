"""The placement functions of tests/keycraft.py against the oracle and the hash vectors, their inverses, and the key sets they craft."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keycraft as kc  # noqa: E402

EDGES = np.array([0, 1, 2, 2**32 - 1, 2**63, 2**64 - 1], dtype=np.uint64)


def _values(seed=1, n=20_000):
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.concatenate([EDGES, rng.integers(0, 2**64 - 1, size=n, dtype=np.uint64, endpoint=True)])


def test_int_hash64_matches_the_oracle_and_the_known_answers(oracle_mod, golden):
    L = oracle_mod.lib()
    x = _values(n=2000)
    assert [int(v) for v in kc.int_hash64(x)] == [L.cho_intHash64(int(v)) for v in x]
    kat = [r for r in golden["kat"] if "intHash64" in r]
    assert kat
    keys = np.array([int(r["key"]) for r in kat], dtype=np.uint64)
    assert [int(v) for v in kc.int_hash64(keys)] == [int(r["intHash64"]) for r in kat]


@pytest.mark.parametrize("fwd,inv", [
    (kc.int_hash64, kc.int_hash64_inv),
    (lambda x: kc._mul(x, kc.RADIX_MULT), lambda y: kc._mul(y, kc.inv_odd(kc.RADIX_MULT))),
    (lambda x: kc._mul(x, kc.GBP_MULT), kc.gbp_inv64),
    (lambda x: kc._mul(x, kc.GBP_MULT1), lambda y: kc.gbp_inv64(y, kc.GBP_MULT1)),
], ids=["intHash64", "radix", "gbp_mult", "gbp_mult1"])
def test_inverses_64(fwd, inv):
    x = _values()
    assert np.array_equal(inv(fwd(x)), x)
    assert np.array_equal(fwd(inv(x)), x)


@pytest.mark.parametrize("mult", [kc.GBP_MULT, kc.GBP_MULT1])
def test_inverses_32(mult):
    x = _values() & np.uint64(kc.M32)
    assert np.array_equal(kc.gbp_inv32(kc._h32(x, mult), mult), x)
    assert np.array_equal(kc._h32(kc.gbp_inv32(x, mult), mult), x)


def test_inv_odd_against_python_ints():
    for c in (kc.INTHASH_MUL1, kc.INTHASH_MUL2, kc.RADIX_MULT, kc.GBP_MULT1):
        assert (c * kc.inv_odd(c)) % 2**64 == 1
        assert (kc._m32(c) * kc.inv_odd(kc._m32(c), 32)) % 2**32 == 1


def test_forward_functions_against_python_ints():
    x = _values(n=500)
    for v, s, p64, c64, p32, c32 in zip(x.tolist(), kc.radix_slot(x, 22), kc.gbp_part64(x, 256), kc.gbp_cell64(x, 8192),
                                         kc.gbp_part32(x & np.uint64(kc.M32), 256), kc.gbp_cell32(x & np.uint64(kc.M32), 256, 8192)):
        assert s == ((v * kc.RADIX_MULT) % 2**64) >> 42
        assert p64 == (((v * kc.GBP_MULT) % 2**64) >> 52) & 255
        assert c64 == (((v * kc.GBP_MULT) % 2**64) >> 20) & 8191
        h = ((v & kc.M32) * ((kc.GBP_MULT >> 32) | 1)) % 2**32
        assert p32 == (h * 256) >> 32
        assert c32 == (((h * 256) % 2**32) * 8192) >> 32


@pytest.mark.parametrize("rows,lg", [(45_876, 18), (91_750, 18), (91_751, 19), (5_872_026, 25), (11_744_051, 25), (11_744_052, 26)])
def test_join_capacity_table(rows, lg):
    assert kc.join_lg_cap(rows) == lg
    assert (kc.LG_CAP_MIN <= lg <= kc.LG_CAP_MAX) == (lg <= 25)
    assert kc.join_lg_cap(45_875) == 17


def test_region_count():
    assert kc.region_count(22) == 64
    assert kc.region_count(26) == kc.MAX_REGIONS
    assert kc.region_count(22, region_kib=64) == kc.MAX_REGIONS


def _rng():
    return np.random.Generator(np.random.PCG64(7))


def _distinct_nonzero(k):
    assert k.dtype == np.uint64 or k.dtype == np.uint32
    assert np.unique(k).shape[0] == k.shape[0] and not np.any(k == 0)


@pytest.mark.parametrize("placement", ["hash", "radix"])
def test_keys_in_one_partition_and_one_slice(placement):
    lg = 22
    slot = kc.join_home if placement == "hash" else kc.radix_slot
    k = kc.keys_in_partition(_rng(), 50_000, lg, 37, placement)
    _distinct_nonzero(k)
    assert np.all(kc.partition_of_slot(slot(k, lg), lg) == 37)
    k = kc.keys_in_slice(_rng(), 6000, lg, 777, placement)
    _distinct_nonzero(k)
    assert np.all(slot(k, lg) // np.uint64(kc.SLICE_CELLS) == 777)
    k = kc.keys_at_slice_end(_rng(), 300, lg, 5, last_cells=3, placement=placement)
    _distinct_nonzero(k)
    s = slot(k, lg)
    assert np.all((s >= np.uint64(6 * kc.SLICE_CELLS - 3)) & (s < np.uint64(6 * kc.SLICE_CELLS)))
    k = kc.keys_in_partitions(_rng(), {10: 100, 12: 5000}, lg, placement)
    _distinct_nonzero(k)
    part = kc.partition_of_slot(slot(k, lg), lg)
    assert set(np.unique(part).tolist()) == {10, 12} and int((part == 10).sum()) == 100
    k = kc.keys_at_slots(_rng(), np.full(40, 123, dtype=np.uint64), lg, placement)
    _distinct_nonzero(k)
    assert np.all(slot(k, lg) == 123)


def test_keys_in_one_region():
    k = kc.keys_in_region(_rng(), 10_000, 22, 17, 64)
    _distinct_nonzero(k)
    assert np.all(kc.join_home(k, 22) >> np.uint64(22 - 6) == 17)


def test_linear_probe_cells_chain_length():
    occ = kc.linear_probe_cells(np.array([4095] * 200 + [10], dtype=np.uint64), 1 << 14)
    assert occ.sum() == 201 and occ[4095:4295].all() and not occ[4295] and occ[10]


def test_gb_keys64_on_one_partition_and_one_cell():
    k = kc.gb_keys64_top(_rng(), 100_000, 12, 0x5A3)
    _distinct_nonzero(k)
    for p in (64, 256, 1024, 4096):
        assert np.unique(kc.gbp_part64(k, p)).shape[0] == 1
    k1 = kc.gb_keys64_top(_rng(), 100_000, 12, 3, kc.GBP_MULT1)
    assert np.unique(kc.gbp_part64(k1, 256, kc.GBP_MULT1)).shape[0] == 1
    c = kc.gb_keys64_on_cell(_rng(), 5000, 14, 1234)
    _distinct_nonzero(c)
    for s in (1024, 8192, 16384):
        assert np.all(kc.gbp_cell64(c, s) == np.uint64(1234 & (s - 1)))
    assert np.unique(kc.gbp_part64(c, 256)).shape[0] > 100


def test_packed_two_uint32_keys_share_one_cell_per_low_half():
    """GROUP BY a, b over two UInt32 columns packs a into the low half: bits 20..32 of key * GBP_MULT see only a and b's lowest bit"""
    rng = _rng()
    a = rng.integers(1, 5, size=50_000, dtype=np.uint64)
    b = rng.integers(0, 2**32, size=50_000, dtype=np.uint64)
    key = a | (b << np.uint64(32))
    cells = kc.gbp_cell64(key, 4096)
    assert np.unique(cells).shape[0] <= 8
    assert np.unique(kc.gbp_part64(key, 256)).shape[0] == 256


def test_gb_keys32_on_one_partition_and_one_cell():
    k = kc.gb_keys32_top(_rng(), 256, 24, 0xABCDE)
    _distinct_nonzero(k)
    for p, s in ((256, 8192), (1024, 16384), (1, 4096)):
        assert np.unique(kc.gbp_part32(k, p)).shape[0] == 1
        assert np.unique(kc.gbp_cell32(k, p, s)).shape[0] == 1
    k = kc.gb_keys32_top(_rng(), 300_000, 10, 77)
    _distinct_nonzero(k)
    assert np.unique(kc.gbp_part32(k, 1024)).shape[0] == 1


# ---- the wide-key dictionary's tag and home cell -----------------------------------------------------------------------------------
KEYDICT_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "clickhouse_amd", "csrc", "keydict_kernels.hip")


def _kd_tag_py(words, weak=False):
    """kd_tag in plain Python ints"""
    h = ((words[0] ^ 0x9E3779B97F4A7C15) * 0xBF58476D1CE4E5B9) % 2**64
    h ^= h >> 31
    for w in words[1:]:
        h = ((h ^ w) * 0x94D049BB133111EB) % 2**64
        h ^= h >> 29
    if weak:
        h &= 0xFFFFF
    return h | 1


def _kd_home_py(tag, capacity):
    return ((((tag >> 1) * 0x9E3779B97F4A7C15) % 2**64) >> 20) & (capacity - 1)


def test_keydict_constants_match_the_kernel_source():
    """a change of the mix or of the home cell in keydict_kernels.hip must fail here, not silently un-craft the GPU cases"""
    import re
    src = open(KEYDICT_SRC).read()
    body = re.search(r"u64 kd_tag\(const u64 \* w, u32 W, int weak\)\s*\{(.*?)\n\}", src, re.S).group(1)
    code = [ln.split("//")[0].strip() for ln in body.splitlines()]
    code = [ln for ln in code if ln and ln not in ("{", "}")]
    assert code == [
        f"u64 h = (w[0] ^ 0x{kc.KD_TAG_XOR0:016X}ull) * 0x{kc.KD_TAG_MUL0:016X}ull;",
        f"h ^= h >> {kc.KD_TAG_SHIFT0};",
        "for (u32 q = 1; q < W; ++q)",
        f"h = (h ^ w[q]) * 0x{kc.KD_TAG_MUL:016X}ull;",
        f"h ^= h >> {kc.KD_TAG_SHIFT};",
        "if (weak)",
        f"h &= 0x{kc.KD_WEAK_MASK:X};",
        "return h | 1ull;",
    ], code
    home = f">> 1) * 0x{kc.KD_HOME_MULT:016X}ull >> {kc.KD_HOME_SHIFT}) & mask"
    assert src.count(home) == 3                       # k_kd_lookup, k_kd_claim, k_kd_rehash: one placement everywhere
    assert src.count("0x9E3779B97F4A7C15ull >>") == 3
    assert f"KD_NO_ID = 0x{kc.KD_NO_ID:X}u;" in src
    lines = src.splitlines()                          # the lines keycraft.py names
    assert "0xBF58476D1CE4E5B9ull" in lines[126] and "0x94D049BB133111EBull" in lines[130] and "0xFFFFF" in lines[134] and "| 1ull" in lines[135]
    assert all(home in lines[k] for k in (164, 226, 418))


@pytest.mark.parametrize("w", [2, 4])
def test_keydict_tag_and_home_against_python_ints(w):
    rng = _rng()
    words = np.concatenate([np.zeros((1, w), dtype=np.uint64), np.full((1, w), 2**64 - 1, dtype=np.uint64),
                            rng.integers(0, 2**64 - 1, size=(2000, w), dtype=np.uint64, endpoint=True)])
    for weak in (False, True):
        tags = kc.keydict_tag(words, weak)
        assert [int(t) for t in tags] == [_kd_tag_py(r, weak) for r in words.tolist()]
        for cap in (2048, 1 << 17, 1 << 24):
            assert [int(h) for h in kc.keydict_home(tags, cap)] == [_kd_home_py(int(t), cap) for t in tags]


@pytest.mark.parametrize("w,cols", [(2, 2), (4, 4), (4, 3)])
def test_keydict_last_word_gives_the_chosen_tag(w, cols):
    """the inverse against the forward function in Python ints, 2000 tags: the crafted key has exactly the tag asked for"""
    rng = _rng()
    tags = rng.integers(0, 2**64 - 1, size=2000, dtype=np.uint64, endpoint=True) | np.uint64(1)
    prefix = rng.integers(0, 2**64 - 1, size=(2000, cols - 1), dtype=np.uint64, endpoint=True)
    last = kc.keydict_last_word(prefix, tags, w - cols)
    for p, l, t in zip(prefix.tolist(), last.tolist(), tags.tolist()):
        assert _kd_tag_py(p + [l] + [0] * (w - cols)) == t
    fam = kc.keydict_same_tag_keys(rng, 40, w, int(tags[0]), cols)
    assert fam.shape == (40, w) and np.unique(fam, axis=0).shape[0] == 40 and np.all(fam[:, cols:] == 0)
    assert {_kd_tag_py(r) for r in fam.tolist()} == {int(tags[0])}


def test_keydict_tag_with_home_is_the_same_cell_of_every_capacity():
    rng = _rng()
    lg = 24
    for bits in ((1 << lg) - 1, (1 << lg) - 2, (1 << lg) - 3, 0, 0x5A5A5):
        tags = kc.keydict_tag_with_home(rng, bits, lg, 2000)
        assert np.unique(tags).shape[0] == 2000 and np.all(tags & np.uint64(1) == 1)
        for t in tags[:400].tolist():
            assert (t >> 1) < 2**63
            for c in range(11, lg + 1):
                assert _kd_home_py(t, 1 << c) == bits & ((1 << c) - 1)
        for c in (11, 17, lg):
            assert np.all(kc.keydict_home(tags, 1 << c) == np.uint64(bits & ((1 << c) - 1)))
    # both together: many keys, one tag, on the last cell of every table
    tag = int(kc.keydict_tag_with_home(rng, (1 << lg) - 1, lg)[0])
    for w in (2, 4):
        fam = kc.keydict_same_tag_keys(rng, 17, w, tag)
        assert np.all(kc.keydict_home(kc.keydict_tag(fam), 2048) == 2047)


# ---- the string dictionary's hash ---------------------------------------------------------------------------------------------------
STRING_SRC = os.path.join(os.path.dirname(KEYDICT_SRC), "string_kernels.hip")
STR_CAPS = [1024, 2048, 1 << 18]


def _str_hash_py(data):
    """str_hash_bytes written out once more, on its own: Python ints, no helper of keycraft"""
    m = 2**64
    h = 0x9E3779B97F4A7C15 ^ (len(data) * 0xFF51AFD7ED558CCD % m)
    i = 0
    while i + 8 <= len(data):
        h = (h ^ int.from_bytes(data[i:i + 8], "little")) * 0xC4CEB9FE1A85EC53 % m
        h ^= h >> 29
        i += 8
    if i < len(data):
        h = (h ^ int.from_bytes(data[i:], "little")) * 0xC4CEB9FE1A85EC53 % m
        h ^= h >> 29
    return int(kc.int_hash64(np.array([h], dtype=np.uint64))[0]) | 1


def test_string_hash_constants_match_the_kernel_source():
    """a change of the string hash, of the home cell or of the table size in string_kernels.hip must fail here, not silently un-craft
    the cases of test_gpu_string_table.py"""
    import re
    src = open(STRING_SRC).read()
    body = re.search(r"u64 str_hash_bytes\(const u8 \* p, u64 len\)\s*\{(.*?)\n\}", src, re.S)
    assert body, "str_hash_bytes is gone or has another signature: restate it in keycraft.py"
    body = body.group(1)
    seed = re.search(r"u64 h = 0x([0-9A-Fa-f]{16})ull \^ \(len \* 0x([0-9A-Fa-f]{16})ull\);", body)
    assert seed, "the seed line of str_hash_bytes changed"
    assert (int(seed.group(1), 16), int(seed.group(2), 16)) == (kc.STR_SEED, kc.STR_LEN_MUL)
    steps = re.findall(r"h = \(h \^ (?:str_load8\(p \+ i\)|tail)\) \* 0x([0-9A-Fa-f]{16})ull;\s*h \^= h >> (\d+);", body)
    assert [(int(m, 16), int(s)) for m, s in steps] == [(kc.STR_WORD_MUL, kc.STR_SHIFT)] * 2, steps   # the full words, the masked tail
    assert re.search(r"tail = str_load8\(p \+ i\) & \(~0ull >> \(8 \* \(8 - \(len - i\)\)\)\);", body), "the tail mask changed"
    assert re.search(r"h = dev_intHash64\(h\);\s*return h \| 1ull;", body), "the last two lines of str_hash_bytes changed"
    assert len(re.findall(r"u64 s = \(h >> 1\) & mask;", src)) == 2                 # k_str_insert and k_str_resolve: one home cell
    assert len(re.findall(r"s = \(s \+ 1\) & mask;", src)) == 2                     # linear probing that wraps
    cap = re.search(r"u64 cap = (\d+);\s*while \(cap < (\d+) \* n\)\s*cap <<= 1;", src)
    assert cap, "the table size rule of chgpu_string_dictionary_encode changed"
    assert (int(cap.group(1)), int(cap.group(2))) == (kc.STR_CAP_MIN, kc.STR_CELLS_PER_ROW)
    assert (kc.STR_SEED, kc.STR_LEN_MUL, kc.STR_WORD_MUL) == (0x9E3779B97F4A7C15, 0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53)


def test_string_table_capacity_steps():
    assert [kc.str_table_cap(n) for n in (0, 1, 511, 512, 513, 1024, 1025, 100_000, 131_072, 131_073)] == \
        [1024, 1024, 1024, 1024, 2048, 2048, 4096, 1 << 18, 1 << 18, 1 << 19]


def test_string_hash_against_python_ints():
    rng = _rng()
    values = [b"", b"a", b"a\0", b"\0", b"\0" * 8, b"\xff" * 9] + [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in range(0, 70)]
    for v in values:
        assert kc.str_hash(v) == _str_hash_py(v) and kc.str_hash(v) & 1 and kc.str_hash(v) == kc.str_raw_hash(v) | 1
        assert kc.str_hash(v) != kc.str_hash(v + b"\0")       # the length is hashed: a zero-extended tail is another value
    assert len({kc.str_hash(v) for v in values}) == len(set(values))


@pytest.mark.parametrize("prefix_len", [0, 8, 16, 64])
def test_str_with_raw_hash_round_trips(prefix_len):
    rng = _rng()
    raws = [0, 1, 2, 2**63, 2**64 - 1] + [int(x) for x in rng.integers(0, 2**64 - 1, size=500, dtype=np.uint64, endpoint=True)]
    for raw in raws:
        prefix = rng.integers(0, 256, size=prefix_len, dtype=np.uint8).tobytes()
        s = kc.str_with_raw_hash(raw, prefix)
        assert len(s) == prefix_len + 8 and s.startswith(prefix)
        assert kc.str_raw_hash(s) == raw and _str_hash_py(s) == raw | 1
    with pytest.raises(AssertionError):
        kc.str_with_raw_hash(5, b"abc")


@pytest.mark.parametrize("cap", STR_CAPS)
def test_str_with_home_lands_where_asked(cap):
    for cell in (0, 1, 31, cap - 500, cap - 2, cap - 1):
        fam = [kc.str_with_home(cell, cap, salt) for salt in range(300)]
        assert len(set(fam)) == 300 and all(len(s) == 8 for s in fam)
        assert {kc.str_home(_str_hash_py(s), cap) for s in fam} == {cell}
        assert len({_str_hash_py(s) for s in fam}) == 300
    # eight strings homed at cell 1022 of 1024 -- the chain of the wrap case -- and a prefixed one
    assert kc.str_home(kc.str_hash(kc.str_with_home(cap - 2, cap, 7, b"prefix--")), cap) == cap - 2
    # salts 1 << k: one home, tags that differ in one high bit only
    lg = cap.bit_length() - 1
    base = kc.str_hash(kc.str_with_home(5, cap, 0))
    for k in (0, 1, 30, 62 - lg):
        t = kc.str_hash(kc.str_with_home(5, cap, 1 << k))
        assert t ^ base == 1 << (k + lg + 1) and kc.str_home(t, cap) == 5


def test_str_tag_twins_differ_and_share_a_tag():
    rng = _rng()
    for tag in [1, 2**64 - 1] + [int(x) | 1 for x in rng.integers(0, 2**64 - 1, size=200, dtype=np.uint64, endpoint=True)]:
        for pa, pb in ((b"", b""), (b"", b"8 bytes!"), (b"sixteen bytes...", b"")):
            a, b = kc.str_tag_twins(tag, pa, pb)
            assert a != b and (len(a), len(b)) == (len(pa) + 8, len(pb) + 8)
            assert _str_hash_py(a) == _str_hash_py(b) == tag
            assert {kc.str_raw_hash(a), kc.str_raw_hash(b)} == {tag, tag ^ 1}
    with pytest.raises(AssertionError):
        kc.str_tag_twins(2)


def test_string_hash_matches_the_kernel_source_compiled_for_the_host(tmp_path):
    """str_load8, str_hash_bytes and dev_intHash64 cut out of the HIP sources and compiled with the host compiler: the crafted strings have
    the tags and home cells they were made for under the kernel's own code, and twins share a tag there"""
    import ctypes
    import re
    import subprocess
    src = open(STRING_SRC).read()
    internal = open(os.path.join(os.path.dirname(STRING_SRC), "chgpu_internal.h")).read()
    column = open(os.path.join(os.path.dirname(STRING_SRC), "string_column.h")).read()   # the one str_load8 of the string kernels

    def cut(text, head):
        m = re.search(r"__device__ __forceinline__ " + re.escape(head) + r"\s*\{.*?\n\}", text, re.S)
        assert m, head
        return m.group(0)
    code = "\n".join(["#include <cstdint>", "typedef uint64_t u64; typedef uint8_t u8;", "#define __device__", "#define __forceinline__ inline",
                      cut(internal, "u64 dev_intHash64(u64 x)"), cut(column, "u64 str_load8(const u8 * p)"), cut(src, "u64 str_hash_bytes(const u8 * p, u64 len)"),
                      'extern "C" u64 host_str_hash(const u8 * p, u64 len) { return str_hash_bytes(p, len); }', ""])
    (tmp_path / "h.cpp").write_text(code)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", str(tmp_path / "h.cpp"), "-o", str(tmp_path / "h.so")])
    fn = ctypes.CDLL(str(tmp_path / "h.so")).host_str_hash
    fn.restype, fn.argtypes = ctypes.c_uint64, [ctypes.c_char_p, ctypes.c_uint64]

    def host(v):
        return fn(v + b"\xee" * 8, len(v))       # the bytes behind the value are not zero: the tail mask is what drops them
    rng = _rng()
    for n in list(range(40)) + [63, 64, 65, 1000]:
        v = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        assert host(v) == kc.str_hash(v), n
    for cap in STR_CAPS:
        for cell in (0, cap - 2, cap - 1):
            for salt in (0, 1, 12345):
                assert kc.str_home(host(kc.str_with_home(cell, cap, salt)), cap) == cell
    for pa, pb in ((b"", b""), (b"", b"a prefix")):
        a, b = kc.str_tag_twins(0x0123456789ABCDEF, pa, pb)
        assert host(a) == host(b) == 0x0123456789ABCDEF
    # a helper with another multiplier does not craft twins: the check above is not vacuous
    good = kc.STR_WORD_MUL
    try:
        kc.STR_WORD_MUL = kc.KD_TAG_MUL
        a, b = kc.str_tag_twins(0x0123456789ABCDEF)
        assert kc.str_hash(a) == kc.str_hash(b) and host(a) != host(b)
    finally:
        kc.STR_WORD_MUL = good
