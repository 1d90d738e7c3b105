"""The device-wide scan (scan.hip) with more tiles than one pass of its one-workgroup kernel covers.

k_scan_tile_offsets scans the tile sums 1024 a pass with a carry between the passes, and a tile is 2048 elements, so the second pass
starts at element 1024 * 2048.  Most callers scan one element per chunk or per group (filter_to_indices: one per 1024 rows) and never get
there at a test's size.  ColumnString.filter scans one element PER ROW, twice: the kept flags give a value's row in the result, the kept
byte counts its place in the chars.  Every value here spells its own row number in three non-zero bytes, so the result names the rows it
holds and the reference is np.flatnonzero of the mask, exact.

ColumnString.index scans one element per row of its result as well, and at this size its sizes and move kernels walk their
grid-stride loops more than once: indexed by a permutation of the rows, the result spells the index array itself."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PASS = 1024 * 2048                      # elements one pass of the one-workgroup kernel covers
ROWS = PASS + 2048 + 5                  # a second pass of one whole tile and a ragged one


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


@pytest.fixture(scope="module")
def column(ch):
    ctx = ch.Context(0)
    i = np.arange(ROWS, dtype=np.uint32)
    chars = np.zeros((ROWS, 4), dtype=np.uint8)      # three base-255 digits + 1, then the value's zero byte
    chars[:, 0], chars[:, 1], chars[:, 2] = i % 255 + 1, i // 255 % 255 + 1, i // (255 * 255) + 1
    offsets = (np.arange(ROWS, dtype=np.uint64) + 1) * 4
    return ctx, ch.ColumnString(ctx.upload(offsets), ctx.upload(chars.reshape(-1)))


def masks():
    rng = np.random.Generator(np.random.PCG64(2048))
    edge = np.zeros(ROWS, dtype=np.uint8)
    edge[[PASS - 1, PASS]] = [1, 200]               # the last row of the first pass's last tile, the first row of the second pass
    return {"random": (rng.random(ROWS) < 0.3).astype(np.uint8), "ones": np.ones(ROWS, dtype=np.uint8), "pass_edge": edge}


@pytest.mark.parametrize("name", ["random", "ones", "pass_edge"])
def test_a_scan_of_one_element_per_row_loops_twice_in_its_one_workgroup_pass(column, name):
    ctx, cs = column
    mask = masks()[name]
    want = np.flatnonzero(mask)
    got = cs.filter(ctx.upload(mask))
    offsets = got.offsets.numpy()
    assert np.array_equal(offsets, (np.arange(len(want), dtype=np.uint64) + 1) * 4)
    b = got.chars.numpy().reshape(-1, 4).astype(np.int64)
    assert np.all(b[:, 3] == 0)
    assert np.array_equal(b[:, 0] - 1 + 255 * (b[:, 1] - 1) + 255 * 255 * (b[:, 2] - 1), want)


def indexes():
    i = np.arange(ROWS, dtype=np.uint64)
    return {"reversed": i[::-1].copy(), "stride_7919": i * np.uint64(7919) % np.uint64(ROWS)}   # 7919 is prime, ROWS = 5 * 419841: a permutation


@pytest.mark.parametrize("name", ["reversed", "stride_7919"])
def test_an_index_of_more_rows_than_one_trip_of_its_grid_stride_loop(column, name):
    ctx, cs = column
    want = indexes()[name]
    assert np.array_equal(np.sort(want), np.arange(ROWS, dtype=np.uint64))
    got = cs.index(ctx.upload(want))
    assert np.array_equal(got.offsets.numpy(), (np.arange(ROWS, dtype=np.uint64) + 1) * 4)
    b = got.chars.numpy().reshape(-1, 4).astype(np.int64)
    assert np.all(b[:, 3] == 0)
    assert np.array_equal((b[:, 0] - 1 + 255 * (b[:, 1] - 1) + 255 * 255 * (b[:, 2] - 1)).astype(np.uint64), want)
