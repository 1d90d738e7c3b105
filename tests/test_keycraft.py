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
