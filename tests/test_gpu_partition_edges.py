"""The stable partition (k_part_hist_lds -> device scan -> k_part_scatter_lds) through its two public doors, Column.scatter and
partition_by_hash, bit for bit against boolean indexing / a stable argsort of the oracle's selector.

Row counts sit on, below and above the 64-row step, the 1024-row wave strip and the 4096-row tile; shard counts cover the register
counting path (<= 8 shards) and the LDS one, shard_bits == 0, and column counts that are no power of two; payloads cover the four
element widths the LDS stage is reinterpreted for.  Every scatter case runs with the selector at a 16-byte aligned address (full tiles
take the 16-byte loads of the histogram) and as a view one or three elements in (the per-row loads), so the two are compared on the same
data -- through the kernel that reads them again per row, since a histogram that disagreed with the scatter would misplace rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STRIP, TILE = 1024, 4096
SIZES = [63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 7 * TILE, 8 * TILE, 8 * TILE + 1]
WIDTHS = [np.uint8, np.uint16, np.uint32, np.uint64]
PAD = 4   # selector columns are uploaded with PAD leading elements: cut(PAD, n) is 16-byte aligned, cut(1, n) and cut(3, n) are not


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


@pytest.fixture(scope="module")
def ctx(ch):
    return ch.Context(0)


def selector_patterns(rng, n, k):
    i = np.arange(n, dtype=np.uint64)
    yield "all rows to the last shard", np.full(n, k - 1, dtype=np.uint32)
    yield "round-robin", (i % np.uint64(k)).astype(np.uint32)
    yield "blocks of 1000 rows", ((i // np.uint64(1000)) % np.uint64(k)).astype(np.uint32)
    yield "most shards empty", np.array([0, k // 2, k - 1], dtype=np.uint32)[rng.integers(0, 3, size=n)]


def payload(dtype, n, salt=0):
    """the row number (plus salt) cut to the width: neighbours differ, so a misplaced row shows even in one byte"""
    return (np.arange(n, dtype=np.uint64) * np.uint64(2 * salt + 1) + np.uint64(salt)).astype(dtype)


def check_scatter(ctx, data, sel, k, offsets, want_sel=None):
    """want_sel: the shard every row must land in (defaults to the selector itself)"""
    n = data.shape[0]
    want_sel = sel if want_sel is None else want_sel
    col = ctx.upload(data)
    padded = ctx.upload(np.concatenate([np.full(PAD, 0xFFFFFFFF, dtype=np.uint32), sel]))
    for off in offsets:
        view = padded.cut(PAD, n) if off == 0 else ctx.upload(np.concatenate([np.zeros(off, dtype=np.uint32), sel])).cut(off, n)
        parts = col.scatter(k, view)
        sizes = [p.size() for p in parts]
        assert len(parts) == k and sum(sizes) == n, (n, k, off, sum(sizes))
        assert sizes == np.bincount(want_sel.astype(np.int64), minlength=k).tolist(), (n, k, off)
        filled = [s for s in range(k) if sizes[s]]
        got = type(col).numpy_many([parts[s] for s in filled])
        for s, g in zip(filled, got):
            assert np.array_equal(g, data[want_sel == s]), (n, k, off, s, data.dtype)


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 9, 16, 100, 255, 256])
def test_scatter_column_counts_sizes_widths_and_selector_patterns(ctx, k):
    rng = np.random.Generator(np.random.PCG64(k))
    for si, n in enumerate(SIZES):
        for pi, (name, sel) in enumerate(selector_patterns(rng, n, k)):
            dtype = WIDTHS[(si + pi) % 4]          # every width meets every pattern and, over the sizes, every size class
            check_scatter(ctx, payload(dtype, n, si), sel, k, offsets=(0, 1 if (si + pi) % 2 else 3))


@pytest.mark.parametrize("dtype", WIDTHS)
def test_scatter_every_width_at_every_size(ctx, dtype):
    rng = np.random.Generator(np.random.PCG64(np.dtype(dtype).itemsize))
    for n in SIZES:
        k = int(rng.choice([2, 7, 8, 9, 256]))
        check_scatter(ctx, payload(dtype, n, n % 5), rng.integers(0, k, size=n).astype(np.uint32), k, offsets=(0,))


def test_scatter_into_257_columns_is_not_implemented(ch, ctx):
    from clickhouse_amd import _capi as K
    with pytest.raises(K.ChgpuError) as e:
        ctx.upload(np.arange(10, dtype=np.int64)).scatter(257, ctx.upload(np.zeros(10, dtype=np.uint32)))
    assert e.value.code == K.ERR_NOT_IMPLEMENTED


@pytest.mark.parametrize("k", [3, 5, 100])
def test_scatter_selectors_beyond_the_column_count_fold_into_shard_0(ctx, k):
    """a selector >= num_columns is a caller bug that the kernels fold into shard 0, at the row's stable position -- also the selectors
    below the power of two that the shard count is rounded up to (3 of 4; 5, 6, 7 of 8; 100 .. 127 of 128), which used to land in a shard
    nobody is handed"""
    rng = np.random.Generator(np.random.PCG64(1000 + k))
    p2 = 1 << (k - 1).bit_length()
    beyond = np.array(list(range(k, p2)) + [p2, p2 + 1, 255, 256, 257, 2**31, 2**32 - 1], dtype=np.uint32)
    for n in (65, TILE, TILE + 1, 2 * TILE + 1):
        sel = rng.integers(0, k, size=n).astype(np.uint32)
        bad = rng.random(n) < 0.3
        sel[bad] = beyond[rng.integers(0, beyond.shape[0], size=int(bad.sum()))]
        sel[:p2 - k] = np.arange(k, p2)                   # every value of [num_columns, p2) is present
        want = np.where(sel >= k, 0, sel).astype(np.uint32)
        assert (want == 0).sum() > (sel == 0).sum()
        for dtype in (np.uint8, np.uint64):
            check_scatter(ctx, payload(dtype, n, 3), sel, k, offsets=(0, 1, 3), want_sel=want)


# ------------------------------------------------------------------------------------------------------------------------------
# partition_by_hash
# ------------------------------------------------------------------------------------------------------------------------------
PAYLOAD_TYPES = [np.uint8, np.int16, np.float32, np.int64, np.int8, np.uint16, np.int32, np.float64]   # widths 1, 2, 4, 8, 1, 2, 4, 8


@pytest.fixture(scope="module")
def selector_table(oracle_mod):
    """shard count -> the oracle's hash_to_selector over the keys 0 .. 65535"""
    keys = np.arange(65536, dtype=np.uint64)
    return {s: oracle_mod.hash_to_selector(keys, s).astype(np.int64) for s in (1, 2, 4, 8, 16, 64, 256)}


def crafted_keys(rng, table, shards, n):
    """rows 0 .. 4095 -- one whole tile -- hash to shard `full`; no row at all hashes to shard `empty`"""
    full = shards // 2
    empty = (full + 1) % shards if shards > 1 else None
    by_shard = [np.flatnonzero(table == s) for s in range(shards)]
    assert all(b.shape[0] >= 100 for b in by_shard)
    keys = np.empty(n, dtype=np.uint64)
    keys[:TILE] = by_shard[full][rng.integers(0, by_shard[full].shape[0], size=TILE)]
    allowed = np.flatnonzero(table != empty) if empty is not None else np.arange(65536)
    keys[TILE:] = allowed[rng.integers(0, allowed.shape[0], size=n - TILE)]
    return keys, full, empty


@pytest.mark.parametrize("n", [TILE + 1, 2 * TILE + 1])
@pytest.mark.parametrize("shards", [1, 2, 4, 8, 16, 64, 256])
def test_partition_by_hash_eight_columns_of_every_width(ch, ctx, oracle_mod, selector_table, shards, n):
    rng = np.random.Generator(np.random.PCG64(shards * 3 + n))
    keys, full, empty = crafted_keys(rng, selector_table[shards], shards, n)
    sel = oracle_mod.hash_to_selector(keys, shards).astype(np.int64)
    assert np.array_equal(sel, selector_table[shards][keys.astype(np.int64)])
    cols = [payload(np.dtype(f"u{np.dtype(dt).itemsize}"), n, c).view(dt) for c, dt in enumerate(PAYLOAD_TYPES)]
    outs, counts = ch.partition_by_hash(ctx.upload(keys), shards, [ctx.upload(c) for c in cols])
    want_counts = np.bincount(sel, minlength=shards)
    assert want_counts[full] >= TILE and (empty is None or want_counts[empty] == 0)
    assert counts.dtype == np.uint64 and counts.tolist() == want_counts.tolist()
    order = np.argsort(sel, kind="stable")
    for c, (o, g) in enumerate(zip(cols, type(outs[0]).numpy_many(outs))):
        assert g.dtype == o.dtype and np.array_equal(g.view(np.uint8), o[order].view(np.uint8)), (shards, n, c)


def test_partition_by_hash_argument_errors(ch, ctx):
    from clickhouse_amd import _capi as K
    keys = ctx.upload(np.arange(100, dtype=np.uint64))
    col = ctx.upload(np.arange(100, dtype=np.int32))
    with pytest.raises(K.ChgpuError) as e:
        ch.partition_by_hash(keys, 4, [col] * 9)
    assert e.value.code == K.ERR_NOT_IMPLEMENTED
    with pytest.raises(K.ChgpuError) as e:
        ch.partition_by_hash(keys, 4, [col, ctx.upload(np.arange(99, dtype=np.int32))])
    assert e.value.code == K.ERR_SIZES_MISMATCH
