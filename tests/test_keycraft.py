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
