"""(key, value) pairs with a chosen placement in the uniqExact set's tables (clickhouse_amd/csrc/uniq_kernels.hip).

The placement hash is a bijection of the value for a fixed key and of the key for a fixed value, so a pair with a chosen global home
cell, fingerprint or LDS home cell is made by inverting it rather than by searching, and the library needs no weakened-hash option.
A plain helper module for the tests, numpy only."""
import numpy as np

M64 = (1 << 64) - 1

# uniq_kernels.hip:31-36: the tile and the workgroup's LDS set
UQ_T = 256
UQ_R = 8
UQ_TILE = UQ_T * UQ_R
UQ_LDS_LG_CELLS = 10
UQ_LDS_CELLS = 1 << UQ_LDS_LG_CELLS
UQ_LDS_PROBES = 16
# uniq_kernels.hip:37 (UQ_KEY_MULT) and chgpu_internal.h:289-297 (dev_intHash64)
UQ_KEY_MULT = 0x9E3779B97F4A7C15
INTHASH_MUL1 = 0xFF51AFD7ED558CCD
INTHASH_MUL2 = 0xC4CEB9FE1A85EC53
# uniq_host.h:12-17: the smallest table, the largest set, growth x4 up to 2^23 cells and then x2; the table holds capacity / 2 pairs
UQ_CAP_MIN = 2048
UQ_MAX_SLOTS = 1 << 31


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def _mul(x, c):
    with np.errstate(over="ignore"):
        return _u64(x) * np.uint64(c)  # wraps mod 2^64


def _xs33(x):
    x = _u64(x)
    return x ^ (x >> np.uint64(33))  # its own inverse on 64 bits


def int_hash64(x):
    x = _xs33(x)
    x = _xs33(_mul(x, INTHASH_MUL1))
    return _xs33(_mul(x, INTHASH_MUL2))


def int_hash64_inv(h):
    x = _mul(_xs33(h), pow(INTHASH_MUL2, -1, 1 << 64))
    x = _mul(_xs33(x), pow(INTHASH_MUL1, -1, 1 << 64))
    return _xs33(x)


def uq_hash(key, val):
    """uniq_kernels.hip:76-79 (uq_hash): intHash64(value ^ key * UQ_KEY_MULT)"""
    return int_hash64(_u64(val) ^ _mul(key, UQ_KEY_MULT))


def value_for(key, h):
    """the value whose pair with `key` hashes to `h`"""
    return int_hash64_inv(h) ^ _mul(key, UQ_KEY_MULT)


def key_for(val, h):
    """the key whose pair with `val` hashes to `h`"""
    return _mul(int_hash64_inv(h) ^ _u64(val), pow(UQ_KEY_MULT, -1, 1 << 64))


def home(h, capacity):
    """uniq_kernels.hip:75: global home cell = hash & (capacity - 1)"""
    return _u64(h) & np.uint64(capacity - 1)


def fingerprint(h):
    """uniq_kernels.hip:75: fingerprint = hash >> 32"""
    return _u64(h) >> np.uint64(32)


def lds_home(h):
    """uniq_kernels.hip:75: LDS home cell = hash >> (64 - UQ_LDS_LG_CELLS)"""
    return _u64(h) >> np.uint64(64 - UQ_LDS_LG_CELLS)


def grow(cap):
    """uniq_host.h:17 (uq_grow)"""
    return cap * 4 if cap < (1 << 23) else cap * 2


def limit(cap):
    """uniq_host.h:20 (uq_limit)"""
    return min(cap // 2, UQ_MAX_SLOTS)


def hashes(rng, n, lg_cap=None, cell=None, fp=None, lds_cell=None):
    """n distinct 64-bit hashes with the low lg_cap bits = cell, the top 32 bits = fp and / or the top UQ_LDS_LG_CELLS bits = lds_cell
    (whichever are given; fp and lds_cell must agree when both are).  The free bits are drawn without repetition."""
    fixed_lo = lg_cap if cell is not None else 0
    fixed_hi = 32 if fp is not None else (UQ_LDS_LG_CELLS if lds_cell is not None else 0)
    free = 64 - fixed_lo - fixed_hi
    assert free >= 1 and n <= (1 << min(free, 40))
    mid = set()
    while len(mid) < n:
        mid.update(int(x) for x in rng.integers(0, 1 << free, size=n - len(mid), dtype=np.uint64))
    out = []
    for m in sorted(mid):
        h = m << fixed_lo
        if cell is not None:
            h |= int(cell)
        if fp is not None:
            assert lds_cell is None or (int(fp) >> (32 - UQ_LDS_LG_CELLS)) == int(lds_cell)
            h |= int(fp) << 32
        elif lds_cell is not None:
            h |= int(lds_cell) << (64 - UQ_LDS_LG_CELLS)
        out.append(h)
    arr = np.array(out, dtype=np.uint64)
    rng.shuffle(arr)
    return arr


def pairs_for(keys, h):
    """(keys, values): pair i has key keys[i] and hashes to h[i]"""
    keys = _u64(keys)
    return keys, value_for(keys, h)
