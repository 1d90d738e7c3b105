"""The String dictionary encoder and ColumnString::filter on the device with CHOSEN placements (tests/keycraft.py restates the string
hash, so a value with a wanted tag or home cell is made by inverting it): probe chains that wrap from the last cell to cell 0, the step
of the table size at 512 / 513 rows, long chains, one home cell for a whole column, two different strings under one 64-bit tag (the
call's NOT_IMPLEMENTED answer -- which also proves that the Python hash is the device's), and both calls on misaligned `chars` views and
on a `chars` with bytes behind the last value.  Every comparison is bit for bit against oracle.lowcardinality."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keycraft as kc  # noqa: E402
from oracle import lowcardinality as OL  # noqa: E402

pytestmark = pytest.mark.gpu

MISALIGN = [1, 7, 15]


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


@pytest.fixture(scope="module")
def ctx(ch):
    c = ch.Context(0)
    yield c
    c.close()


def _layout(values):
    lens = np.fromiter((len(v) + 1 for v in values), dtype=np.uint64, count=len(values))
    return np.cumsum(lens, dtype=np.uint64), b"".join(v + b"\0" for v in values)


def _column(ch, ctx, values, misalign=0, slack=b""):
    """a ColumnString of `values`.  misalign > 0: chars is a view `misalign` bytes into a padded buffer (Column.cut), offsets built for
    the view; slack: bytes that belong to chars but to no value (chars.size() > offsets.back())"""
    if not misalign and not slack:
        col = ch.ColumnString.from_values(ctx, values)
        assert col.chars.device_ptr % 16 == 0
        return col
    offsets, body = _layout(values)
    whole = ctx.upload(np.frombuffer(b"\xee" * misalign + body + slack + b"\xee" * 32, dtype=np.uint8))
    view = whole.cut(misalign, len(body) + len(slack))
    assert view.device_ptr % 16 == misalign and view.size() == len(body) + len(slack)
    return ch.ColumnString(ctx.upload(offsets), view, list(values))


def _encode(ch, col):
    """chgpu_string_dictionary_encode itself: (ids, first rows, number of distinct values)"""
    K = ch._capi
    ids, rows, n = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
    ctx = col.offsets.ctx
    K.check(K.lib().chgpu_string_dictionary_encode(ctx._h, col.offsets._h, col.chars._h, C.byref(ids), C.byref(rows), C.byref(n)))
    return ch.Column(ctx, ids).numpy(), ch.Column(ctx, rows).numpy(), int(n.value)


def _check_encode(ch, ctx, values, misalign=0):
    """ids, first rows and the dictionary (read back from the device column, in first-appearance order) equal the oracle's"""
    want_ids, want_dict, want_first = OL.dictionary_encode(values)
    col = _column(ch, ctx, values, misalign)
    ids, first, n = _encode(ch, col)
    assert ids.dtype == np.uint32 and first.dtype == np.uint64
    assert n == len(want_dict) == first.shape[0]
    assert np.array_equal(first, want_first), np.flatnonzero(first != want_first)[:5]
    bad = np.flatnonzero(ids != want_ids)
    assert bad.size == 0, (bad[:5], ids[bad[:5]], want_ids[bad[:5]])
    col._host_values = None                     # the dictionary's strings come from the device bytes
    lc = col.dictionary_encode()
    assert lc.dictionary == want_dict and np.array_equal(lc.indexes.numpy(), want_ids)
    return n


def _refused(ch, ctx, values, code, misalign=0, col=None):
    with pytest.raises(ch.ChgpuError) as e:
        _encode(ch, col if col is not None else _column(ch, ctx, values, misalign))
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def _spread(distinct, rows, seed):
    """exactly `rows` rows: every value of `distinct` at least rows // len(distinct) times, shuffled with a fixed seed"""
    reps = rows // len(distinct)
    assert reps >= 2
    values = list(distinct) * reps + list(distinct[:rows - reps * len(distinct)])
    assert len(values) == rows
    rng = np.random.Generator(np.random.PCG64(seed))
    return [values[int(i)] for i in rng.permutation(rows)]


def _ordinary(n, seed):
    """n distinct everyday values of 0 .. 40 bytes (none is 8 or 16 bytes of a crafted kind: they are text)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [b""] + [b"value-%06d" % i + b"x" * int(rng.integers(0, 28)) for i in range(n - 1)]


# ---- chosen home cells ------------------------------------------------------------------------------------------------------------------------
def _wrap_set(cap):
    """64 strings homed at the last but one cell -- their chain runs cap - 2, cap - 1, 0, 1, ... 61 -- and 32 more homed at cells 0 .. 31,
    which that chain displaces"""
    chain = [kc.str_with_home(cap - 2, cap, salt) for salt in range(64)]
    low = [kc.str_with_home(cell, cap, 1000 + cell) for cell in range(32)]
    assert [kc.str_home(kc.str_hash(s), cap) for s in chain + low] == [cap - 2] * 64 + list(range(32))
    assert len(set(chain + low)) == 96
    occupied = kc.linear_probe_cells([cap - 2] * 64 + list(range(32)), cap)
    assert occupied[cap - 2] and occupied[cap - 1] and occupied[:94].all() and not occupied[94:cap - 2].any()
    return chain + low


@pytest.mark.parametrize("rows,cap", [(512, 1024), (513, 2048)], ids=["wrap-512-rows", "capacity-step-513-rows"])
def test_encode_chain_wraps_to_cell_zero(ch, ctx, rows, cap):
    assert kc.str_table_cap(rows) == cap and kc.str_table_cap(rows - 1) == 1024
    values = _spread(_wrap_set(cap), rows, seed=rows)
    assert _check_encode(ch, ctx, values) == 96
    # the set made for the OTHER table size is an everyday column here: same strings, no chosen placement
    assert _check_encode(ch, ctx, _spread(_wrap_set(3072 - cap), rows, seed=rows + 1)) == 96


def test_encode_long_chain_across_the_end_of_a_large_table(ch, ctx):
    rows = 100_003
    cap = kc.str_table_cap(rows)
    assert cap == 1 << 18
    chain = [kc.str_with_home(cap - 500, cap, salt) for salt in range(1000)]        # 500 cells before the end, 500 behind cell 0
    assert {kc.str_home(kc.str_hash(s), cap) for s in chain} == {cap - 500} and len(set(chain)) == 1000
    plain = _ordinary(3000, seed=2)
    rng = np.random.Generator(np.random.PCG64(3))
    values = chain * 3 + [plain[int(i)] for i in rng.integers(0, len(plain), size=rows - 3000)]
    values = [values[int(i)] for i in rng.permutation(rows)]
    assert _check_encode(ch, ctx, values) == len(set(values)) and set(chain) <= set(values)


def test_encode_every_value_on_one_home_cell(ch, ctx):
    rows = 2048                                                                      # no repeats: a chain of 2048, about 4 M probe steps
    cap = kc.str_table_cap(rows)
    assert cap == 4096
    for cell in (77, cap - 1):
        values = [kc.str_with_home(cell, cap, salt) for salt in range(rows)]
        assert {kc.str_home(kc.str_hash(s), cap) for s in values} == {cell}
        assert _check_encode(ch, ctx, values) == rows


def test_encode_tags_that_differ_in_one_high_bit(ch, ctx):
    cap = 1024
    near = [kc.str_with_home(300, cap, 0)] + [kc.str_with_home(300, cap, 1 << k) for k in range(53)]
    tags = [kc.str_hash(s) for s in near]
    assert len(set(tags)) == 54 and {kc.str_home(t, cap) for t in tags} == {300}
    assert all(bin(t ^ tags[0]).count("1") == 1 and (t ^ tags[0]) >= 1 << 11 for t in tags[1:])
    values = _spread(near, 500, seed=5)
    assert kc.str_table_cap(len(values)) == cap
    assert _check_encode(ch, ctx, values) == 54


# ---- two different strings under one tag -----------------------------------------------------------------------------------------------------
TWIN_TAG = 0x0123456789ABCDEF


def _twin_columns():
    """name -> (values, the twin to take out).  Both twins of a pair have the tag TWIN_TAG; `a` is always 8 bytes."""
    a, b8 = kc.str_tag_twins(TWIN_TAG)
    a2, b16 = kc.str_tag_twins(TWIN_TAG, b"", b"a prefix")
    assert a2 == a and (len(a), len(b8), len(b16)) == (8, 8, 16) and len({a, b8, b16}) == 3
    assert kc.str_hash(a) == kc.str_hash(b8) == kc.str_hash(b16) == TWIN_TAG
    plain = _ordinary(200, seed=7)
    assert not {a, b8, b16} & set(plain)
    mid = _spread(plain, 600, seed=8)
    big = _spread(_ordinary(5000, seed=9), 100_001, seed=10)
    return {
        "pair-of-8-bytes": ([a, b8], b8),
        "pair-of-8-bytes-among-others": (mid[:300] + [a] + mid[300:400] + [b8] + mid[400:], b8),
        "8-and-16-bytes": (mid[:300] + [a, a] + mid[300:400] + [b16] + mid[400:], b16),      # the length branch
        "twin-in-the-first-row": ([b8] + mid[:300] + [a, a, a] + mid[300:], b8),
        "twin-in-the-last-row": (mid[:300] + [a] + mid[300:] + [b16], b16),
        "100000-rows-apart": ([a] + big[1:100_000] + [b8], b8),
    }


@pytest.mark.parametrize("name", ["pair-of-8-bytes", "pair-of-8-bytes-among-others", "8-and-16-bytes", "twin-in-the-first-row",
                                  "twin-in-the-last-row", "100000-rows-apart"])
def test_encode_refuses_two_strings_under_one_tag(ch, ctx, name):
    values, twin = _twin_columns()[name]
    assert sum(v == twin for v in values) == 1
    if name == "100000-rows-apart":
        assert values.index(twin) - values.index(kc.str_tag_twins(TWIN_TAG)[0]) == 100_000
    text = _refused(ch, ctx, values, ch._capi.ERR_NOT_IMPLEMENTED)
    assert "hash tag" in text
    # the same context goes on: the column without that twin is an everyday one
    rest = [v for v in values if v != twin]
    _check_encode(ch, ctx, rest)
    # and the other way round: the twin stays, its partner leaves
    partner = kc.str_tag_twins(TWIN_TAG)[0]
    _check_encode(ch, ctx, [v for v in values if v != partner])


def test_encode_one_twin_many_times_is_no_collision(ch, ctx):
    a, b16 = kc.str_tag_twins(TWIN_TAG, b"", b"a prefix")
    plain = _spread(_ordinary(50, seed=11), 400, seed=12)
    for twin in (a, b16):
        values = [twin] + plain[:200] + [twin] * 50 + plain[200:] + [twin]
        _check_encode(ch, ctx, values)
    assert _check_encode(ch, ctx, [a] * 700) == 1


# ---- invariants and views --------------------------------------------------------------------------------------------------------------------
def test_encode_refuses_chars_longer_than_the_last_offset(ch, ctx):
    values = _spread(_ordinary(20, seed=13), 100, seed=14)
    for slack in (b"\0", b"\xee" * 40):
        col = _column(ch, ctx, values, 0, slack)
        text = _refused(ch, ctx, values, ch._capi.ERR_SIZES_MISMATCH, col=col)
        assert "offsets.back()" in text
    _check_encode(ch, ctx, values)


def _view_values():
    """every length 0 .. 17 and 63, 64, 65: a random value, the same with its last byte changed, and the same plus a zero byte"""
    rng = np.random.Generator(np.random.PCG64(15))
    distinct = []
    for n in list(range(18)) + [63, 64, 65]:
        v = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        distinct += [v, v + b"\0"]
        if n:
            distinct += [v[:-1] + bytes([v[-1] ^ 1]), v[:-1] + bytes([v[-1] ^ 0x80])]
    distinct = list(dict.fromkeys(distinct))
    return _spread(distinct, 3 * len(distinct) + 1, seed=16)


@pytest.mark.parametrize("misalign", [0] + MISALIGN)
def test_encode_on_a_misaligned_chars_view(ch, ctx, misalign):
    values = _view_values()
    assert _check_encode(ch, ctx, values, misalign) == len(set(values))
    # crafted strings are read with the same unaligned loads: a wrapping chain on a view
    assert _check_encode(ch, ctx, _spread(_wrap_set(1024), 512, seed=17), misalign) == 96


def test_encode_views_see_a_collision_too(ch, ctx):
    values, _ = _twin_columns()["8-and-16-bytes"]
    for misalign in MISALIGN:
        _refused(ch, ctx, values, ch._capi.ERR_NOT_IMPLEMENTED, misalign)


# ---- ColumnString::filter --------------------------------------------------------------------------------------------------------------------
FILTER_LENGTHS = list(range(18)) + [23, 24, 25, 63, 64, 65]
LONG = 100_000


def _filter_values(rows):
    """`rows` values cycling through FILTER_LENGTHS (random bytes, zeros among them), one value of 100 000 bytes in the middle"""
    rng = np.random.Generator(np.random.PCG64(rows))
    values = [rng.integers(0, 256, size=FILTER_LENGTHS[i % len(FILTER_LENGTHS)], dtype=np.uint8).tobytes() for i in range(rows)]
    values[rows // 2] = rng.integers(0, 256, size=LONG, dtype=np.uint8).tobytes()
    return values, rows // 2


def _masks(rows, long_row):
    z = np.zeros(rows, dtype=np.uint8)
    first, last, only_long = z.copy(), z.copy(), z.copy()
    first[0], last[-1], only_long[long_row] = 255, 1, 2
    return {"all": (np.arange(rows) % 255 + 1).astype(np.uint8), "none": z, "first": first, "last": last,
            "alternating": ((np.arange(rows) % 2) * 0x80).astype(np.uint8), "only-long": only_long}


def _check_filter(ch, ctx, values, mask, misalign=0, slack=b""):
    offsets, body = _layout(values)
    want_offsets, want_chars = OL.string_filter(offsets, np.frombuffer(body + slack, dtype=np.uint8), mask)
    got = _column(ch, ctx, values, misalign, slack).filter(ctx.upload(mask))
    got_offsets, got_chars = got.offsets.numpy(), got.chars.numpy()
    assert got_offsets.dtype == np.uint64 and got_chars.dtype == np.uint8
    assert np.array_equal(got_offsets, want_offsets), (got_offsets[:5], want_offsets[:5])
    assert got_chars.shape[0] == (int(want_offsets[-1]) if want_offsets.shape[0] else 0)      # ends at the last kept value
    assert np.array_equal(got_chars, want_chars), np.flatnonzero(got_chars != want_chars)[:5]
    assert got.to_list() == [v for v, m in zip(values, mask) if m]


@pytest.mark.parametrize("misalign", [0] + MISALIGN)
@pytest.mark.parametrize("rows", [1, 255, 256, 257])
def test_filter_lengths_masks_and_views(ch, ctx, rows, misalign):
    values, long_row = _filter_values(rows)
    assert rows == 1 or {len(v) for v in values} == set(FILTER_LENGTHS) | {LONG}
    for name, mask in _masks(rows, long_row).items():
        _check_filter(ch, ctx, values, mask, misalign)


@pytest.mark.parametrize("misalign", [0] + MISALIGN)
def test_filter_one_row_of_every_length(ch, ctx, misalign):
    rng = np.random.Generator(np.random.PCG64(18))
    for n in FILTER_LENGTHS:
        v = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()]
        _check_filter(ch, ctx, v, np.array([7], dtype=np.uint8), misalign)
        _check_filter(ch, ctx, v, np.array([0], dtype=np.uint8), misalign)


@pytest.mark.parametrize("misalign", [0] + MISALIGN)
def test_filter_ignores_bytes_behind_the_last_value(ch, ctx, misalign):
    values, long_row = _filter_values(257)
    for slack in (b"\xee", b"\xee" * 100):
        for name, mask in _masks(257, long_row).items():
            _check_filter(ch, ctx, values, mask, misalign, slack)
