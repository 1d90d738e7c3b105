"""tests/uniq_craft.py against the formula of clickhouse_amd/csrc/uniq_kernels.hip.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import uniq_craft as U  # noqa: E402

# (key, value, uq_hash(key, value)): computed once with the HIP source's formula, intHash64(value ^ key * 0x9E3779B97F4A7C15), in C++
GOLDEN = [
    (0x0000000000000000, 0x0000000000000000, 0x0000000000000000),
    (0x0000000000000000, 0x0000000000000001, 0xB456BCFC34C2CB2C),
    (0x0000000000000001, 0x0000000000000000, 0x9CA066F1A4AB2EEA),
    (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0x25B775FAECA8F520),
    (0x8000000000000000, 0x7FF8000000000001, 0xFA6216DCD0F44095),
    (0x0000000000003039, 0x0000000000010932, 0xB9160B927D56F624),
    (0xDEADBEEFCAFEF00D, 0x0123456789ABCDEF, 0x03B9CB961A122C35),
    (0x000000000000002A, 0x00000000FFFFFFFF, 0xCC2A82656A5B0242),
]


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def test_python_hash_equals_the_source_formula():
    k = np.array([g[0] for g in GOLDEN], dtype=np.uint64)
    v = np.array([g[1] for g in GOLDEN], dtype=np.uint64)
    assert U.uq_hash(k, v).tolist() == [g[2] for g in GOLDEN]


def test_constants_match_the_sources():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(repo, "clickhouse_amd", "csrc", "uniq_kernels.hip")) as f:
        hip = f.read()
    with open(os.path.join(repo, "clickhouse_amd", "csrc", "uniq_host.h")) as f:
        host = f.read()
    assert f"UQ_T = {U.UQ_T};" in hip and f"UQ_R = {U.UQ_R};" in hip and f"UQ_LDS_LG_CELLS = {U.UQ_LDS_LG_CELLS};" in hip
    assert f"UQ_LDS_PROBES = {U.UQ_LDS_PROBES};" in hip and "UQ_KEY_MULT = 0x9E3779B97F4A7C15ull;" in hip
    assert "return dev_intHash64(val ^ key * UQ_KEY_MULT);" in hip
    assert f"UQ_CAP_MIN = {U.UQ_CAP_MIN};" in host and "UQ_MAX_SLOTS = 1ull << 31;" in host
    assert "return cap < (1ull << 23) ? cap * 4 : cap * 2;" in host


def test_inverses_round_trip():
    rng = _rng(1)
    k = rng.integers(0, 2**64, size=1000, dtype=np.uint64)
    v = rng.integers(0, 2**64, size=1000, dtype=np.uint64)
    h = U.uq_hash(k, v)
    assert np.array_equal(U.int_hash64_inv(U.int_hash64(v)), v)
    assert np.array_equal(U.value_for(k, h), v)
    assert np.array_equal(U.key_for(v, h), k)
    edge = np.array([0, 1, 2**63, 2**64 - 1], dtype=np.uint64)
    assert np.array_equal(U.value_for(edge, U.uq_hash(edge, edge[::-1])), edge[::-1])


def test_crafted_pairs_land_where_they_were_sent():
    rng = _rng(2)
    keys = rng.integers(0, 50, size=300, dtype=np.uint64)
    h = U.hashes(rng, 300, lg_cap=11, cell=2047)
    k, v = U.pairs_for(keys, h)
    assert len(set(zip(k.tolist(), v.tolist()))) == 300
    assert set(U.home(U.uq_hash(k, v), 2048).tolist()) == {2047}
    assert set(U.home(U.uq_hash(k, v), 1024).tolist()) == {1023}     # and on the matching cell of every smaller table
    h = U.hashes(rng, 40, lds_cell=5)
    k, v = U.pairs_for(keys[:40], h)
    assert set(U.lds_home(U.uq_hash(k, v)).tolist()) == {5} and len(set(h.tolist())) == 40
    h = U.hashes(rng, 8, lg_cap=13, cell=77, fp=0xABCD1234)
    k, v = U.pairs_for(keys[:8], h)
    got = U.uq_hash(k, v)
    assert set(U.fingerprint(got).tolist()) == {0xABCD1234} and set(U.home(got, 8192).tolist()) == {77}
    assert len(set(zip(k.tolist(), v.tolist()))) == 8


def test_geometry():
    assert U.grow(2048) == 8192 and U.grow(1 << 21) == 1 << 23 and U.grow(1 << 23) == 1 << 24
    assert U.limit(2048) == 1024 and U.limit(1 << 33) == 1 << 31
