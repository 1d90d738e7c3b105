"""The wide-key dictionary (chgpu_keydict, keys128 / keys256) at its packing, collision, wrap, growth, look-up, chunk and entry edges.

The reference is the oracle's packFixed + HashMap (ids by first appearance) or numpy over the packed words.  The dictionary is free
to number its keys in any order, so ids are compared up to that bijection (`_Ref.check`, `_check_numpy`): the same partition of the
rows, len(dict) = the number of distinct packed keys, ids dense in [0, len), ids of an earlier call unchanged by every later one, and
key_columns(ids) equal to the input columns bit for bit; a find call gives 0xFFFFFFFF exactly on the absent rows and leaves len alone.
Crafted key sets come from tests/keycraft.py (many keys under one full 64-bit tag, tags homed on the last cells of every capacity);
the `debug` option's `keydict plan=` line says what a call did, so that "the crafted keys went where they were meant to" is asserted."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keycraft as kc  # noqa: E402

pytestmark = pytest.mark.gpu

NO_ID = 0xFFFFFFFF
ABSENT = np.uint64(2**64 - 1)
U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64
I8, I16, I32, I64 = np.int8, np.int16, np.int32, np.int64
LG = 24                                   # crafted homes hold for every capacity up to 2^24 cells
KD_T = 256                                # keydict_kernels.hip: KD_T, and the rows per lane of k_kd_lookup<2, 4> / <4, 2>
LOOKUP_U = {2: 4, 4: 2}


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


@contextlib.contextmanager
def _context(ch, **opts):
    ctx = ch.Context(0)
    try:
        for name, value in opts.items():
            ctx.set_option(name, value)
        ctx.set_option("debug", 1)
        yield ctx
    finally:
        ctx.close()


def _plan(err):
    got = [ln[len("chgpu: "):] for ln in err.splitlines() if ln.startswith("chgpu: keydict plan=")]
    assert len(got) == 1, err
    return dict(kv.split("=", 1) for kv in got[0].split() if "=" in kv)


def _encode(d, capfd, cols, **kw):
    """-> (ids Column, the call's plan line as a dict)"""
    capfd.readouterr()
    ids = d.encode(cols, **kw)
    return ids, _plan(capfd.readouterr().err)


def _ints(field):
    return [int(x) for x in field.split(",")]


def _cast(d, cols):
    return [np.ascontiguousarray(c).astype(t, copy=False) for c, t in zip(cols, d.key_dtypes)]


def _words(cols, key_bytes):
    """packFixed in numpy: the columns' bytes side by side, zero padded -> uint64[n, key_bytes / 8]"""
    n = cols[0].shape[0]
    b = np.zeros((n, key_bytes), dtype=np.uint8)
    off = 0
    for c in cols:
        sz = c.dtype.itemsize
        b[:, off:off + sz] = np.ascontiguousarray(c).view(np.uint8).reshape(n, sz)
        off += sz
    return b.view(np.uint64)


def _cols_from_bytes(b, dtypes):
    """uint8[n, total] -> one column per dtype, the bytes laid consecutively (packFixed undone)"""
    cols, off = [], 0
    for t in dtypes:
        sz = np.dtype(t).itemsize
        cols.append(np.ascontiguousarray(b[:, off:off + sz]).view(t).reshape(-1))
        off += sz
    assert off == b.shape[1]
    return cols


def _ref_inverse(words):
    """np.unique(return_inverse) over the packed keys, a word at a time (exact; the structured-view sort is far slower at size)
    -> (number of distinct keys, group number per row)"""
    inv = np.zeros(words.shape[0], dtype=np.uint64)
    k = 1
    for q in range(words.shape[1]):
        u, iq = np.unique(words[:, q], return_inverse=True)
        assert k * u.shape[0] < 2**63
        uu, inv = np.unique(inv * np.uint64(u.shape[0]) + iq.reshape(-1).astype(np.uint64), return_inverse=True)
        inv = inv.reshape(-1).astype(np.uint64)
        k = uu.shape[0]
    return k, inv.astype(np.int64)


class _Ref:
    """the oracle's HashMap next to one dictionary, over all its calls: the map GPU id -> oracle id must be one function for the
    dictionary's whole life (ids are stable, equal keys get equal ids) and one-to-one (different keys get different ids)"""

    def __init__(self, O, d):
        self.O, self.d = O, d
        self.map = O.WideKeyMap(d.key_bytes)
        self.g2o = np.full(0, -1, dtype=np.int64)

    def check(self, cols, ids_col, insert=True):
        d, O = self.d, self.O
        cols = _cast(d, cols)
        ids = ids_col.numpy()
        assert ids.dtype == np.uint32 and ids.shape[0] == cols[0].shape[0]
        packed = O.pack_fixed(cols, d.key_bytes)
        assert np.array_equal(packed.view(np.uint64), _words(cols, d.key_bytes))
        oid = self.map.batch(packed, insert)
        absent = oid == ABSENT
        assert insert is False or not absent.any()
        assert np.array_equal(ids == NO_ID, absent), "NO_ID exactly on the absent rows"
        assert len(d) == len(self.map), (len(d), len(self.map))
        if ids.shape[0] <= 200_000:                                                  # (the oracle map against numpy, at small sizes)
            nref, inv = _ref_inverse(packed.view(np.uint64))
            _, first = np.unique(inv, return_index=True)
            assert np.array_equal(oid[first][inv], oid) and np.unique(oid[~absent]).shape[0] == nref - np.unique(inv[absent]).shape[0]
        g, o = ids[~absent].astype(np.int64), oid[~absent].astype(np.int64)
        assert g.shape[0] == 0 or int(g.max()) < len(d), "an id beyond len(dict)"
        if self.g2o.shape[0] < len(d):
            self.g2o = np.concatenate([self.g2o, np.full(len(d) - self.g2o.shape[0], -1, dtype=np.int64)])
        old = self.g2o[g]
        assert np.all((old == -1) | (old == o)), "an id of an earlier call now names another key"
        self.g2o[g] = o
        assert np.array_equal(self.g2o[g], o), "one id for two different keys"
        known = self.g2o[self.g2o >= 0]
        assert np.unique(known).shape[0] == known.shape[0], "two ids for one key"
        assert bool((self.g2o >= 0).all()), "ids are not dense in [0, len)"       # every key of the map entered through a checked call
        back = d.key_columns(ids_col)
        assert len(back) == len(cols)
        for b, c in zip(back, cols):
            want = np.where(absent, c.dtype.type(0), c)
            got = b.numpy()
            assert got.dtype == c.dtype and np.array_equal(got, want), "key_columns differs from the input column"
        return ids


def _check_numpy(d, cols, ids_col, n_before=0):
    """the same contract with numpy only, for one emplace call into a dictionary that held n_before keys none of which is in `cols`
    (n_before = 0: a fresh one); every row takes part"""
    cols = _cast(d, cols)
    ids = ids_col.numpy()
    nref, inv = _ref_inverse(_words(cols, d.key_bytes))
    assert len(d) == n_before + nref, (len(d), n_before, nref)
    _, first = np.unique(inv, return_index=True)
    gid = ids[first]                                                                # the id of each reference group ...
    assert np.array_equal(gid[inv], ids), "rows of one key got different ids"       # ... is the id of all its rows,
    assert np.array_equal(np.sort(gid), np.arange(n_before, n_before + nref, dtype=np.uint32)), "ids not one-to-one and dense"
    for b, c in zip(d.key_columns(ids_col), cols):
        got = b.numpy()
        assert got.dtype == c.dtype and np.array_equal(got, c)
    return ids


def _check_find_numpy(d, cols_in, ids_in, cols_find, ids_find_col):
    """numpy only: a find call's ids are exactly the ids the emplace call gave to equal keys, and NO_ID for every other row"""
    cols_in, cols_find = _cast(d, cols_in), _cast(d, cols_find)
    n1 = cols_in[0].shape[0]
    nref, inv = _ref_inverse(np.concatenate([_words(cols_in, d.key_bytes), _words(cols_find, d.key_bytes)]))
    gid = np.full(nref, NO_ID, dtype=np.uint32)
    gid[inv[:n1]] = ids_in
    want = gid[inv[n1:]]
    got = ids_find_col.numpy()
    assert np.array_equal(got, want)
    for b, c in zip(d.key_columns(ids_find_col), cols_find):
        assert np.array_equal(b.numpy(), np.where(want == NO_ID, c.dtype.type(0), c))
    return want


def _word_cols(keys, dtypes):
    """packed keys uint64[n, W] -> columns of `dtypes`, which tile the leading words exactly"""
    total = sum(np.dtype(t).itemsize for t in dtypes)
    b = np.ascontiguousarray(keys).view(np.uint8).reshape(keys.shape[0], -1)
    assert not b[:, total:].any()
    return _cols_from_bytes(b[:, :total], dtypes)


# ---- a. the packing matrix ---------------------------------------------------------------------------------------------------------
MIXES = [
    (U8, U64), (U16, U64), (U32, U64), (U8, U16, U32, U64), (U32, U64, U16), (U8, U64, U64), (U8, U64, U64, U64),
    (U16, U64, U32, U64, U16), (I8, I64), (I32, I64, I16), (U8,) * 16, (U16,) * 16, (U64, U32, U16, U8, U8), (U64, U64, U64, U32, U16, U8, U8),
    (U64, U8), (U64, U64, U8), (I16, I8, I64, I32), (U32, U32, U64, U64, U64),
]


def _mix_id(m):
    return "-".join(np.dtype(t).name for t in m) if len(m) < 8 else f"{len(m)}x{np.dtype(m[0]).name}"


def _byte_variants(rng, total):
    """keys that differ from one random base key in exactly one byte, for every byte of the key and three different changes of it:
    so some pairs differ only in a straddling column's low bytes, some only in its high bytes (the next word), some only in the key's
    last byte, some only in a high word; then the all-zero and the all-ones key and their one-byte neighbours"""
    base = rng.integers(0, 256, size=total, dtype=np.uint8)
    rows = [base]
    for fixed in (base, np.zeros(total, dtype=np.uint8), np.full(total, 255, dtype=np.uint8)):
        rows.append(fixed)
        for p in range(total):
            for x in (0x01, 0x80, 0xFF):
                r = fixed.copy()
                r[p] ^= x
                rows.append(r)
    return np.unique(np.stack(rows), axis=0)


def _matrix_blocks(rng, dtypes):
    """three emplace blocks and a find block of byte matrices uint8[n, total]"""
    total = sum(np.dtype(t).itemsize for t in dtypes)
    var = rng.permutation(_byte_variants(rng, total))
    few = rng.integers(0, 256, size=(300, total), dtype=np.uint8)
    few[:, rng.integers(0, total, size=total // 2)] = 0                 # low-cardinality random keys around them
    more = rng.integers(0, 256, size=(500, total), dtype=np.uint8)

    def rows(parts, n):
        pool = np.concatenate(parts)
        return np.concatenate([pool, pool[rng.integers(0, pool.shape[0], size=n)]])[rng.permutation(pool.shape[0] + n)]

    b1 = rows([var[: var.shape[0] // 2], few[:150]], 2000)
    b2 = rows([var, few], 3000)                                          # old keys, their one-byte neighbours, new keys
    b3 = rows([var, few, more], 3000)
    absent = var.copy()
    absent[:, 0] ^= 0x55
    absent[:, total - 1] ^= 0x2A                                         # two bytes changed: none of these is a key of `var`
    find = rows([var, absent, few, rng.integers(0, 256, size=(200, total), dtype=np.uint8)], 1000)
    return [b1, b2, b3], find


@pytest.mark.parametrize("dtypes", MIXES, ids=_mix_id)
def test_packing_matrix_ids_and_key_columns(ch, oracle_mod, capfd, dtypes):
    """every column order that makes a column straddle an 8-byte word (the `hi` half of kd_pack_row, the word + 1 read of
    k_kd_key_column), signed columns, 16 columns, keys of exactly 9, 16, 17 and 32 bytes"""
    rng = _rng(100 + len(dtypes))
    blocks, find = _matrix_blocks(rng, dtypes)
    with _context(ch) as ctx:
        d = ch.KeyDict(dtypes, ctx)
        assert d.key_bytes == (16 if sum(np.dtype(t).itemsize for t in dtypes) <= 16 else 32)
        ref = _Ref(oracle_mod, d)
        for k, b in enumerate(blocks):
            cols = _cols_from_bytes(b, dtypes)
            ids, plan = _encode(d, capfd, cols)
            ref.check(cols, ids)
            assert plan["plan"] == "emplace" and int(plan["W"]) == d.key_bytes // 8 and plan["chunks"] == "1" and plan["rc"] == "0"
            assert plan["lookup"] == ("0" if k == 0 else "1")           # the look-up kernel and the in-place compare both see the mix
        n = len(d)
        cols = _cols_from_bytes(find, dtypes)
        ids, plan = _encode(d, capfd, cols, insert=False)
        got = ref.check(cols, ids, insert=False)
        assert plan["plan"] == "find" and len(d) == n and plan["ids"] == f"{n}->{n}"
        assert (got == NO_ID).sum() >= 200 and (got != NO_ID).sum() >= 500
        del d, ref, ids


@pytest.mark.parametrize("dtypes", MIXES, ids=_mix_id)
def test_packing_matrix_group_by_matches_oracle(ch, oracle_mod, dtypes):
    O = oracle_mod
    rng = _rng(200 + len(dtypes))
    blocks, _ = _matrix_blocks(rng, dtypes)
    aggs = [(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None)]
    with _context(ch) as ctx:
        G = ch.KeysFixedAggregator(dtypes, aggs, ctx=ctx)
        R = O.KeysFixedAggregator(dtypes, aggs)
        for b in blocks:
            cols = _cols_from_bytes(b, dtypes)
            v = rng.integers(-2**62, 2**62, size=b.shape[0], dtype=np.int64)
            G.execute_on_block(cols, [v, None])
            R.execute_on_block(cols, [v, None])
        gk, (gs, gc) = G.convert_to_block()
        rk, (rs, rc) = R.convert_to_block()
        assert len(G) == rk[0].shape[0] == np.unique(np.concatenate(blocks), axis=0).shape[0]
        kb = G.dict.key_bytes
        go, ro = np.lexsort(_words(gk, kb).T), np.lexsort(_words(rk, kb).T)
        for a, b in zip(gk, rk):
            assert a.dtype == b.dtype and np.array_equal(a[go], b[ro])
        assert np.array_equal(gs[go], rs[ro]) and np.array_equal(gc[go], rc[ro])
        del G


# ---- b. one tag, many keys; c. the end of the table ----------------------------------------------------------------------------------
# (W, the UInt64 columns of the key): keys128, keys256, and keys256 of three columns with a zero fourth word
SHAPES = [(2, 2), (4, 4), (4, 3)]


def _repeat(rng, keys, reps):
    return keys[rng.permutation(np.repeat(np.arange(keys.shape[0]), reps))]


def _launches(ctx):
    return ctx.counters()["KernelLaunches"]


def _one_tag_protocol(ch, O, capfd, rng, w, ncols, K, tag, j, back=None):
    """K keys under `tag`: the first j in one call, all K in the next, all again, then find.  Rounds, from the protocol in the header of
    keydict_kernels.hip: all rows of the family walk the same cells, k_kd_claim lets exactly one row claim the first empty one, every
    other row becomes a candidate of that cell, k_kd_verify settles the rows of the claimer's key and sends the rest on -- one new key
    per round.  Keys of an earlier call are compared in place and cost no round.  So a call that brings m new keys of the tag takes
    max(m, 1) rounds."""
    dt = (U64,) * ncols
    fam = kc.keydict_same_tag_keys(rng, K + 6, w, tag, ncols)
    keys, absent_same_tag = fam[:K], fam[K:]
    with _context(ch) as ctx:
        d = ch.KeyDict(dt, ctx)
        ref = _Ref(O, d)

        def call(rows, insert=True):
            cols = _word_cols(rows, dt)
            dev = [ctx.upload(c) for c in cols]
            before = _launches(ctx)
            ids, plan = _encode(d, capfd, dev, insert=insert)
            spent = _launches(ctx) - before
            ref.check(cols, ids, insert)
            assert plan["chunks"] == "1" and plan["grown"] == "0" and plan["rc"] == "0"
            rounds, lookup = int(plan["rounds"]), int(plan["lookup"])
            assert spent == 2 * rounds + lookup                          # the second witness: two kernels per round, one for the look-up
            if back is not None:
                cap = int(plan["cap"])
                assert cap <= 1 << LG and int(kc.keydict_home(np.uint64(tag), cap)) == cap - 1 - back
            return plan, rounds, lookup
        if j:
            plan, rounds, lookup = call(_repeat(rng, keys[:j], 5))
            assert (rounds, lookup, plan["ids"]) == (j, 0, f"0->{j}")
        plan, rounds, lookup = call(_repeat(rng, keys, 5))
        assert (rounds, lookup, plan["ids"]) == (K - j, 1 if j else 0, f"{j}->{K}")
        plan, rounds, lookup = call(_repeat(rng, keys, 3))
        assert (rounds, lookup, plan["ids"]) == (1, 1, f"{K}->{K}")
        # find: present keys, absent keys of the same tag (past all K cells to the empty one), absent keys of other tags
        other = rng.integers(0, 2**64 - 1, size=(50, w), dtype=np.uint64, endpoint=True)
        other[:, ncols:] = 0
        probe = rng.permutation(np.concatenate([_repeat(rng, keys, 2), _repeat(rng, absent_same_tag, 3), other]))
        plan, rounds, lookup = call(probe, insert=False)
        assert (plan["plan"], rounds, lookup, plan["ids"]) == ("find", 1, 1, f"{K}->{K}")
        del d, ref


@pytest.mark.parametrize("w,ncols", SHAPES)
@pytest.mark.parametrize("K", [2, 3, 17, 40])
def test_one_tag_many_keys_in_one_call(ch, oracle_mod, capfd, w, ncols, K):
    rng = _rng(300 + K + w)
    tag = int(rng.integers(0, 2**64 - 1, dtype=np.uint64, endpoint=True)) | 1
    _one_tag_protocol(ch, oracle_mod, capfd, rng, w, ncols, K, tag, 0)


@pytest.mark.parametrize("w,ncols", SHAPES)
@pytest.mark.parametrize("K,j", [(2, 1), (3, 1), (3, 2), (17, 1), (17, 8), (17, 16), (40, 13), (40, 39)])
def test_one_tag_many_keys_across_calls(ch, oracle_mod, capfd, w, ncols, K, j):
    """the later call walks past j cells of earlier keys in one kernel (compare in place, slot + 1), and so does the find side"""
    rng = _rng(400 + K + j + w)
    tag = int(rng.integers(0, 2**64 - 1, dtype=np.uint64, endpoint=True)) | 1
    _one_tag_protocol(ch, oracle_mod, capfd, rng, w, ncols, K, tag, j)


@pytest.mark.parametrize("w,ncols", SHAPES)
@pytest.mark.parametrize("back", [0, 1])
@pytest.mark.parametrize("K,j", [(3, 0), (3, 1), (17, 0), (17, 6), (40, 21)])
def test_one_tag_chain_wraps_at_the_end_of_the_table(ch, oracle_mod, capfd, w, ncols, back, K, j):
    """the tag's home is the last cell (back = 0) or the last but one (back = 1) of every capacity: a keys128 walk starts on the odd and
    on the even cell of the last line and goes on in line 0; the plan line's `cap` is checked against the crafted home"""
    rng = _rng(500 + K + j + w + back)
    tag = int(kc.keydict_tag_with_home(rng, (1 << LG) - 1 - back, LG)[0])
    _one_tag_protocol(ch, oracle_mod, capfd, rng, w, ncols, K, tag, j, back=back)


@pytest.mark.parametrize("w,ncols", SHAPES)
def test_cluster_of_different_tags_on_the_last_three_cells(ch, oracle_mod, capfd, w, ncols):
    rng = _rng(600 + w + ncols)
    dt = (U64,) * ncols
    tags = np.stack([kc.keydict_tag_with_home(rng, (1 << LG) - 1 - b, LG, 7) for b in range(3)], axis=1).reshape(-1)   # 21 tags, 7 per cell
    assert np.unique(tags).shape[0] == 21
    prefix = rng.integers(0, 2**64 - 1, size=(21, ncols - 1), dtype=np.uint64, endpoint=True)
    keys = np.concatenate([prefix, kc.keydict_last_word(prefix, tags, w - ncols)[:, None], np.zeros((21, w - ncols), dtype=np.uint64)], axis=1)
    assert np.array_equal(kc.keydict_tag(keys), tags)
    present, absent = rng.permutation(keys[:15]), keys[15:]             # five keys per cell go in: 15 keys on three cells, 12 of them past the wrap
    with _context(ch) as ctx:
        d = ch.KeyDict(dt, ctx)
        ref = _Ref(oracle_mod, d)
        for c in range(3):                                               # later calls find the end of the table occupied
            rows = _repeat(rng, present[: 5 * (c + 1)], 3)
            ids, plan = _encode(d, capfd, _word_cols(rows, dt))
            ref.check(_word_cols(rows, dt), ids)
            cap = int(plan["cap"])
            assert np.all(kc.keydict_home(tags, cap) >= np.uint64(cap - 3))
            assert plan["ids"] == f"{5 * c}->{5 * (c + 1)}" and plan["rounds"] == "1"        # different tags: nothing to verify twice
        occ = kc.linear_probe_cells(kc.keydict_home(kc.keydict_tag(present), cap), cap)
        assert occ[cap - 3:].all() and occ[:12].all() and occ.sum() == 15                      # (the model: cells 0..11 are taken)
        rows = rng.permutation(np.concatenate([_repeat(rng, present, 2), _repeat(rng, absent, 2)]))
        ids, plan = _encode(d, capfd, _word_cols(rows, dt), insert=False)
        got = ref.check(_word_cols(rows, dt), ids, insert=False)
        assert (got == NO_ID).sum() == 12 and plan["rounds"] == "1"
        ids, plan = _encode(d, capfd, _word_cols(keys, dt))              # and the six absent ones go in behind them
        ref.check(_word_cols(keys, dt), ids)
        assert plan["ids"] == "15->21"
        del d, ref, ids


# ---- g. row ranges and entry checks --------------------------------------------------------------------------------------------------
def test_encode_row_ranges(ch, oracle_mod, capfd):
    rng = _rng(700)
    n = 5000
    dt = (U32, U64, U16)
    cols = [rng.integers(0, 30, size=n).astype(t) for t in dt]
    with _context(ch) as ctx:
        d = ch.KeyDict(dt, ctx)
        ref = _Ref(oracle_mod, d)
        dev = [ctx.upload(c) for c in cols]
        for rb, re in [(0, 0), (n, n), (17, 17), (3, 4), (1001, 3777), (n - 1, n), (0, n)]:
            ids, plan = _encode(d, capfd, dev, row_begin=rb, row_end=re)
            assert ids.size() == re - rb and int(plan["n"]) == re - rb and int(plan["chunks"]) == (1 if re > rb else 0)
            ref.check([c[rb:re] for c in cols], ids)
        for rb, re in [(0, 0), (4990, n), (n - 1, n), (2, 4000)]:
            ids, _ = _encode(d, capfd, dev, insert=False, row_begin=rb, row_end=re)
            ref.check([c[rb:re] for c in cols], ids, insert=False)
        del d, ref, ids, dev


def test_group_by_row_ranges_match_oracle(ch, oracle_mod):
    O = oracle_mod
    rng = _rng(701)
    n = 6000
    dt = (U8, U64, U64)
    cols = [rng.integers(0, 12, size=n).astype(t) for t in dt]
    v = rng.integers(-2**62, 2**62, size=n, dtype=np.int64)
    aggs = [(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None)]
    with _context(ch) as ctx:
        G = ch.KeysFixedAggregator(dt, aggs, ctx=ctx)
        R = O.KeysFixedAggregator(dt, aggs)
        for rb, re in [(0, 0), (0, 1), (100, 2500), (2400, 2401), (n - 1, n), (3000, n)]:
            G.execute_on_block(cols, [v, None], rb, re)
            R.execute_on_block([c[rb:re] for c in cols], [v[rb:re], None])
        gk, (gs, gc) = G.convert_to_block()
        rk, (rs, rc) = R.convert_to_block()
        go, ro = np.lexsort(_words(gk, 32).T), np.lexsort(_words(rk, 32).T)
        assert len(G) == rk[0].shape[0]
        for a, b in zip(gk, rk):
            assert a.dtype == b.dtype and np.array_equal(a[go], b[ro])
        assert np.array_equal(gs[go], rs[ro]) and np.array_equal(gc[go], rc[ro])
        del G


@pytest.mark.parametrize("dtypes", [(U64, U32, U16), (U8, U64, U64, U32)], ids=_mix_id)
def test_selector_and_key_columns_over_ids_with_no_id(ch, oracle_mod, capfd, dtypes):
    """UInt128HashCRC32 / UInt256HashCRC32 -> two-level bucket & (shards - 1) on every row; NO_ID reads as the all-zero key"""
    O = oracle_mod
    rng = _rng(702 + len(dtypes))
    n = 3000
    cols = [rng.integers(0, 2**64 - 1, size=n, dtype=np.uint64, endpoint=True).astype(t) for t in dtypes]
    cols = [np.concatenate([c, c[:500]]) for c in cols]
    with _context(ch) as ctx:
        d = ch.KeyDict(dtypes, ctx)
        ids = _Ref(O, d).check(cols, d.encode(cols))
        packed = O.pack_fixed(_cast(d, cols), d.key_bytes)
        holes = ids.copy()
        holes[rng.integers(0, holes.shape[0], size=700)] = NO_ID
        holes[[0, -1]] = NO_ID
        packed[holes == NO_ID] = 0
        hcol = ctx.upload(holes)
        h = np.array([O.hash_keys_fixed(r) for r in packed], dtype=np.uint64)
        for shards in (1, 2, 8, 256):
            sel = d.selector(hcol, shards).numpy()
            assert sel.dtype == np.uint32 and np.array_equal(sel, (((h >> np.uint64(24)) & np.uint64(0xFF)) & np.uint64(shards - 1)).astype(np.uint32))
        for b, c in zip(d.key_columns(hcol), _cast(d, cols)):
            assert np.array_equal(b.numpy(), np.where(holes == NO_ID, c.dtype.type(0), c))
        assert d.selector(ctx.upload(np.empty(0, dtype=np.uint32)), 8).size() == 0
        del d, hcol


def test_entry_checks_return_their_error_codes_and_leave_the_dictionary_usable(ch, oracle_mod, capfd):
    K = ch._capi
    L = K.lib()
    rng = _rng(703)

    def encode_rc(d, cols, rb, re, insert=1):
        ptrs = (C.c_void_p * len(cols))(*[c._h for c in cols])
        h = C.c_void_p()
        rc = L.chgpu_keydict_encode(d._h, len(cols), ptrs, rb, re, insert, C.byref(h))
        if rc == K.OK:
            ch.Column(d.ctx, h)
        return rc

    def key_column_rc(d, ids, off, tag):
        h = C.c_void_p()
        rc = L.chgpu_keydict_key_column(d._h, ids._h, off, tag, C.byref(h))
        if rc == K.OK:
            ch.Column(d.ctx, h)
        return rc

    def selector_rc(d, ids, shards):
        h = C.c_void_p()
        rc = L.chgpu_keydict_selector(d._h, ids._h, shards, C.byref(h))
        if rc == K.OK:
            ch.Column(d.ctx, h)
        return rc

    with _context(ch) as ctx:
        h = C.c_void_p()
        for kb in (0, 8, 24, 33):
            assert L.chgpu_keydict_create(ctx._h, kb, 0, C.byref(h)) == K.ERR_BAD_ARGUMENTS
        with pytest.raises(ch.ChgpuError) as e:
            ch.KeyDict((U64,) * 4 + (U8,), ctx)
        assert e.value.code == K.ERR_NOT_IMPLEMENTED
        d = ch.KeyDict((U64, U64), ctx)
        d32 = ch.KeyDict((U64, U64, U64), ctx)
        ref = _Ref(oracle_mod, d)
        a, b = rng.integers(0, 50, size=1000, dtype=np.uint64), rng.integers(0, 50, size=1000, dtype=np.uint64)
        ids = d.encode([a, b])
        ref.check([a, b], ids)
        n0 = len(d)
        u64c, u64d = ctx.upload(a), ctx.upload(b)
        u8c = [ctx.upload(a.astype(np.uint8)) for _ in range(17)]
        f64c, short, u64ids = ctx.upload(a.astype(np.float64)), ctx.upload(a[:999]), ctx.upload(a)
        assert encode_rc(d32, u8c, 0, 1000) == K.ERR_NOT_IMPLEMENTED                # 17 columns
        assert encode_rc(d32, u8c[:16], 0, 1000) == K.OK
        assert encode_rc(d, [u64c, u64d, u8c[0]], 0, 1000) == K.ERR_BAD_ARGUMENTS   # 17 key bytes into keys128
        assert encode_rc(d32, [u64c] * 4 + [u8c[0]], 0, 1000) == K.ERR_BAD_ARGUMENTS  # 33 into keys256
        assert encode_rc(d, [u64c, f64c], 0, 1000) == K.ERR_NOT_IMPLEMENTED         # Float64 key column
        assert encode_rc(d, [u64c, short], 0, 999) == K.ERR_SIZES_MISMATCH          # unequal lengths
        assert encode_rc(d, [u64c, u64d], 0, 1001) == K.ERR_BAD_ARGUMENTS           # row_end past the column
        assert encode_rc(d, [u64c, u64d], 7, 6) == K.ERR_BAD_ARGUMENTS
        assert encode_rc(d, [u64c, u64d], 0, 1001, insert=0) == K.ERR_BAD_ARGUMENTS
        for shards in (0, 3, 512, 257):
            assert selector_rc(d, ids, shards) == K.ERR_BAD_ARGUMENTS
        assert selector_rc(d, u64ids, 8) == K.ERR_BAD_ARGUMENTS                     # ids that are not UInt32
        assert key_column_rc(d, u64ids, 0, K.U64) == K.ERR_BAD_ARGUMENTS
        assert key_column_rc(d, ids, 9, K.U64) == K.ERR_BAD_ARGUMENTS               # a key part outside the key
        assert key_column_rc(d, ids, 16, K.U8) == K.ERR_BAD_ARGUMENTS
        assert key_column_rc(d, ids, 0, K.F64) == K.ERR_BAD_ARGUMENTS
        assert key_column_rc(d, ids, 8, K.U64) == K.OK and key_column_rc(d, ids, 15, K.U8) == K.OK
        assert len(d) == n0
        # still usable: old ids unchanged, new keys go in
        ids2, plan = _encode(d, capfd, [np.concatenate([a, a + np.uint64(100)]), np.concatenate([b, b])])
        got = ref.check([np.concatenate([a, a + np.uint64(100)]), np.concatenate([b, b])], ids2)
        assert np.array_equal(got[:1000], ids.numpy()) and plan["rc"] == "0"
        del d, d32, ref, ids, ids2, u64c, u64d, u8c, f64c, short, u64ids


# ---- e. the look-up kernel on purpose -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtypes", [(U64, U64), (U64, U32, U32), (U64, U64, U64, U64), (U64, U32, U32, U64, U64)], ids=_mix_id)
def test_lookup_kernel_over_settled_displaced_new_and_absent_keys(ch, oracle_mod, capfd, dtypes):
    """k_kd_lookup<2, 4> and <4, 2>, with and without words8, against a dictionary of 300 000 keys in 4 Mi cells: keys at home, crafted
    keys displaced from an occupied home, new keys, absent keys over an empty and over an occupied home; block lengths around the
    workgroup, and one row either side of a whole number of rows per lane for the grid the plan line reports"""
    rng = _rng(800 + len(dtypes))
    w = 2 if sum(np.dtype(t).itemsize for t in dtypes) <= 16 else 4
    assert sum(np.dtype(t).itemsize for t in dtypes) == 8 * w
    n_keys = 300_000

    def random_keys(n):
        return rng.integers(0, 2**64 - 1, size=(n, w), dtype=np.uint64, endpoint=True)

    def homed_on(victims, n):
        """n keys with tags of their own whose home, in every table up to 2^LG cells, is the home of victims[i]"""
        home = kc.keydict_home(kc.keydict_tag(victims[:n]), 1 << LG)
        tags = np.array([int(kc.keydict_tag_with_home(rng, int(h), LG)[0]) for h in home], dtype=np.uint64)
        prefix = random_keys(n)[:, : w - 1]
        keys = np.concatenate([prefix, kc.keydict_last_word(prefix, tags)[:, None]], axis=1)
        assert np.array_equal(kc.keydict_home(kc.keydict_tag(keys), 1 << LG), home)
        return keys

    settled = random_keys(n_keys)
    with _context(ch) as ctx:
        d = ch.KeyDict(dtypes, ctx, size_hint=2_000_000)
        ref = _Ref(oracle_mod, d)

        def call(rows, insert=True, lookup=1):
            cols = _word_cols(rows, dtypes)
            ids, plan = _encode(d, capfd, cols, insert=insert)
            got = ref.check(cols, ids, insert)
            assert int(plan["lookup"]) == lookup and int(plan["cap"]) == 1 << 22 and plan["grown"] == "0" and plan["chunks"] == "1"
            assert len(d) * 8 <= int(plan["cap"])
            return got, plan
        _, plan = call(np.concatenate([settled, settled]), lookup=0)
        G = int(plan["grid"])
        assert G * KD_T < 2 * n_keys                                      # the grid is the device's cap, not the block's length
        displaced, absent_occupied = homed_on(settled, 600), homed_on(settled[600:], 600)
        call(rng.permutation(np.concatenate([displaced, settled[:3000], random_keys(500)])))
        big = G * KD_T * LOOKUP_U[w]
        for n in (1, 255, 256, 257, 1023, big - 1, big + 1):
            pool = np.concatenate([settled[rng.integers(0, n_keys, size=max(n // 2, 1))], displaced, random_keys(max(n // 64, 1))])
            rows = displaced[:1] if n == 1 else np.concatenate([displaced, pool[rng.integers(0, pool.shape[0], size=n)]])[-n:]
            got, plan = call(rows if n == 1 else rng.permutation(rows))
            assert int(plan["n"]) == n and int(plan["grid"]) == min((n + KD_T - 1) // KD_T, G)
            pool = np.concatenate([settled[rng.integers(0, n_keys, size=max(n // 2, 1))], displaced, absent_occupied, random_keys(max(n // 4, 1))])
            rows = absent_occupied[:1] if n == 1 else np.concatenate([absent_occupied, displaced, pool[rng.integers(0, pool.shape[0], size=n)]])[-n:]
            got, plan = call(rows if n == 1 else rng.permutation(rows), insert=False)
            assert int(plan["n"]) == n and (got == NO_ID).any() and (n == 1 or (got != NO_ID).any())
        del d, ref


# ---- the cases this file takes over from test_gpu_round2.py --------------------------------------------------------------------------
@pytest.mark.parametrize("key_dtypes", [(np.uint64, np.uint64), (np.uint64, np.uint32, np.uint16), (np.uint64, np.uint64, np.uint64, np.uint32, np.uint8)])
def test_keys_fixed_group_by_matches_oracle(ch, oracle_mod, key_dtypes):
    O = oracle_mod
    rng = np.random.Generator(np.random.PCG64(11))
    aggs = [(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None)]
    with _context(ch) as ctx:
        G = ch.KeysFixedAggregator(key_dtypes, aggs, ctx=ctx)
        R = O.KeysFixedAggregator(key_dtypes, aggs)
        for n in (70_001, 1, 300_000):                                    # several blocks: ids persist, the table grows
            cols = [rng.integers(0, 40, size=n).astype(d) for d in key_dtypes]
            cols[0][: n // 50] = 0
            for c in cols[1:]:
                c[: n // 50] = 0                                          # the all-zero key
            v = rng.integers(-2**62, 2**62, size=n, dtype=np.int64)
            G.execute_on_block(cols, [v, None])
            R.execute_on_block(cols, [v, None])
        gk, (gs, gc) = G.convert_to_block()
        rk, (rs, rc) = R.convert_to_block()
        assert len(G) == len(rk[0])
        go = np.lexsort([k.astype(np.uint64) for k in gk])
        ro = np.lexsort([k.astype(np.uint64) for k in rk])
        for a, b in zip(gk, rk):
            assert a.dtype == b.dtype and np.array_equal(a[go], b[ro])
        assert np.array_equal(gs[go], rs[ro]) and np.array_equal(gc[go], rc[ro])
        del G


def test_keys_fixed_join_and_selector(ch, oracle_mod):
    O = oracle_mod
    rng = np.random.Generator(np.random.PCG64(12))
    bk = [rng.integers(0, 300, size=20_000, dtype=np.uint64), rng.integers(0, 5, size=20_000).astype(np.uint32), rng.integers(0, 3, size=20_000).astype(np.uint16)]
    pk = [rng.integers(0, 400, size=50_000, dtype=np.uint64), rng.integers(0, 6, size=50_000).astype(np.uint32), rng.integers(0, 3, size=50_000).astype(np.uint16)]
    bv = rng.integers(-2**40, 2**40, size=20_000, dtype=np.int64)
    with _context(ch) as ctx:
        j = ch.KeysFixedHashJoin([np.uint64, np.uint32, np.uint16], ch.JOIN_INNER, ch.STRICT_ALL, ctx=ctx)
        j.add_block(bk)
        c, s = j.probe_count_sum(pk, ctx.upload(bv))
        m = O.WideKeyMap(16)
        bid = m.batch(O.pack_fixed(bk, 16), True).astype(np.int64)
        pid = m.batch(O.pack_fixed(pk, 16), False)
        mult = np.bincount(bid, minlength=len(m))
        sums = np.zeros(len(m), dtype=np.uint64)
        np.add.at(sums, bid, bv.astype(np.uint64))
        hit = pid != np.uint64(2**64 - 1)
        assert c == int(mult[pid[hit].astype(np.int64)].sum()) and s % 2**64 == int(sums[pid[hit].astype(np.int64)].sum(dtype=np.uint64))
        # the shard of a wide key by the reference's own hash: UInt128HashCRC32 -> two-level bucket & (shards - 1)
        ids = j.dict.encode(bk, insert=False)
        sel = j.dict.selector(ids, 8).numpy()
        packed = O.pack_fixed(bk, 16)
        want = np.array([((O.hash_keys_fixed(r) >> 24) & 0xFF) & 7 for r in packed[:2000]], dtype=np.uint32)
        assert np.array_equal(sel[:2000], want)
        del j, ids


def test_keys_fixed_tag_collisions_are_resolved_exactly(ch, oracle_mod, capfd):
    """with 20-bit tags (test hook) dozens of different keys share a tag: the verification rounds must still give exact ids"""
    rng = np.random.Generator(np.random.PCG64(5))
    a = rng.integers(0, 30000, size=400_000, dtype=np.uint64)
    b = rng.integers(0, 3, size=400_000, dtype=np.uint64)
    with _context(ch, test_keydict_weak_tags=1) as ctx:
        d = ch.KeyDict([np.uint64, np.uint64], ctx)
        idc, plan = _encode(d, capfd, [a, b])
        ids = idc.numpy()
        pairs = np.stack([a, b], axis=1)
        uniq = np.unique(pairs, axis=0)
        assert len(d) == uniq.shape[0], (len(d), uniq.shape[0])
        first = {}
        for i, (x, y) in enumerate(pairs.tolist()):
            assert first.setdefault(int(ids[i]), (x, y)) == (x, y)
        assert len(first) == uniq.shape[0]
        k0, k1 = [c.numpy() for c in d.key_columns(ctx.upload(ids))]
        assert np.array_equal(k0, a) and np.array_equal(k1, b)
        # the hook was on: keys do share tags (the model), and the call took further rounds for them
        tags = kc.keydict_tag(uniq, weak=True)
        assert np.unique(tags).shape[0] < uniq.shape[0] - 1000 and int(plan["rounds"]) >= 2
        _check_numpy(d, [a, b], idc)
        del d, idc


def test_keys_fixed_dictionary_grows_when_rows_defer_at_its_limit(ch, capfd):
    """the table is sized for the keys it holds, not for the rows of a chunk: 3 M distinct keys into a dictionary made for 1024 run past
    limit = capacity / 2 (rows defer, the table grows fourfold, the deferred rows run again); ids stay dense, stable and exact"""
    rng = np.random.Generator(np.random.PCG64(21))
    n = 3_000_000
    a = rng.permutation(n).astype(np.uint64) * np.uint64(2654435761)
    b = (np.arange(n, dtype=np.uint64) * np.uint64(40503)) ^ np.uint64(0xDEADBEEF)
    with _context(ch) as ctx:
        d = ch.KeyDict([np.uint64, np.uint64], ctx)
        idc, plan = _encode(d, capfd, [a, b])
        ids = idc.numpy()
        assert int(plan["grown"]) >= 1 and plan["chunks"] == "1"
        assert len(d) == n and np.array_equal(np.sort(ids), np.arange(n, dtype=np.uint32))          # dense: every id exactly once
        k0, k1 = [c.numpy() for c in d.key_columns(ctx.upload(ids))]
        assert np.array_equal(k0, a) and np.array_equal(k1, b)
        # a second block: old keys (compared in place, no second kernel), new keys and repeats of the new keys inside the block
        a2 = np.concatenate([a[::7], a[:1000] + np.uint64(1), a[:1000] + np.uint64(1)])
        b2 = np.concatenate([b[::7], b[:1000], b[:1000]])
        ids2 = d.encode([a2, b2]).numpy()
        m = a[::7].shape[0]
        assert np.array_equal(ids2[:m], ids[::7]) and len(d) == n + 1000
        assert np.array_equal(ids2[m:m + 1000], ids2[m + 1000:]) and np.array_equal(np.sort(ids2[m:m + 1000]), np.arange(n, n + 1000, dtype=np.uint32))
        # findKey: present keys keep their ids, absent ones get NO_ID
        probe = d.encode([np.concatenate([a[:500], a[:500] + np.uint64(3)]), np.concatenate([b[:500], b[:500]])], insert=False).numpy()
        assert np.array_equal(probe[:500], ids[:500]) and (probe[500:] == 0xFFFFFFFF).all() and len(d) == n + 1000
        del d, idc


# ---- f. more than one chunk -----------------------------------------------------------------------------------------------------------
MI = 1 << 20


def _chunked_block(rng, n, dtypes, distinct, regions=5):
    """`distinct` base keys tiled at random over n rows; a third of them twisted by the region of the row, so that every stretch of
    the block brings new keys and repeats old ones"""
    base = [rng.integers(0, 2**64 - 1, size=distinct, dtype=np.uint64, endpoint=True).astype(t) for t in dtypes]
    idx = rng.integers(0, distinct, size=n)
    region = (np.arange(n, dtype=np.uint64) * np.uint64(regions)) // np.uint64(n)
    cols = [b[idx] for b in base]
    cols[0] = np.where(idx % 3 == 0, cols[0] ^ (region + np.uint64(1)).astype(cols[0].dtype), cols[0])
    return cols


def _expected_chunks(n, first, longest):
    """the chunk lengths of chgpu_keydict_encode: first, 4 x, ... up to `longest`; a tail shorter than half a chunk joins the last"""
    out, c0, chunk = [], 0, first
    while c0 < n:
        m = n - c0 if n - c0 < chunk + chunk // 2 else chunk
        out.append(m)
        c0 += m
        chunk = min(chunk * 4, longest)
    return out


@pytest.mark.parametrize("n,chunks", [(28 * 1024 + 3, 3), (1024 + 511, 1), (1024 + 512, 2), (6 * 1024, 2), (120 * 1024, 9)])
def test_emplace_in_several_chunks_with_the_chunk_rows_hook(ch, capfd, n, chunks):
    """test_keydict_chunk_rows = 1024 stands for the 4 Mi first chunk: 28 Ki + 3 rows are chunks of 1 Ki, 4 Ki and the rest joined, as
    28 Mi + 3 rows are 4 Mi, 16 Mi and the rest; 1.5 Ki - 1 and 1.5 Ki rows are the boundary of "a short tail joins", as 6 Mi - 1 and
    6 Mi are.  The offsets of a chunk into the ids and the rows, and keys of an earlier chunk met again in a later one"""
    rng = _rng(900 + n)
    assert len(_expected_chunks(n, 1024, 16 * 1024)) == chunks
    with _context(ch, test_keydict_chunk_rows=1024) as ctx:
        d = ch.KeyDict((U64, U64), ctx)
        cols = _chunked_block(rng, n, (U64, U64), max(n // 8, 100))
        ids, plan = _encode(d, capfd, cols)
        assert int(plan["chunks"]) == chunks and len(_ints(plan["rounds"])) == chunks
        assert _ints(plan["grid"]) == [(m + KD_T - 1) // KD_T for m in _expected_chunks(n, 1024, 16 * 1024)]
        assert _ints(plan["lookup"])[0] == 0
        first = _check_numpy(d, cols, ids)
        # again, as a second call over the same rows shifted by one and some new keys: nothing new but those, the old ids as they were
        cols2 = [np.concatenate([c[1:], (c[:50] ^ c.dtype.type(0x5555))]) for c in cols]
        ids2, plan2 = _encode(d, capfd, cols2)
        got = ids2.numpy()
        assert np.array_equal(got[: n - 1], first[1:]) and int(plan2["chunks"]) == len(_expected_chunks(n + 49, 1024, 16 * 1024))
        for b, c in zip(d.key_columns(ids2), cols2):
            assert np.array_equal(b.numpy(), c)
        both = [np.concatenate([a, b]) for a, b in zip(cols, cols2)]
        assert len(d) == _ref_inverse(_words(both, 16))[0] and int(got.max()) == len(d) - 1
        del d, ids, ids2


@pytest.mark.parametrize("n,chunks", [(24 * 1024 - 1, 1), (24 * 1024, 2), (24 * 1024 + 1, 2), (70 * 1024 + 5, 4)])
def test_find_in_several_chunks_with_the_chunk_rows_hook(ch, capfd, n, chunks):
    """the find side takes the longest chunk from the start (64 Mi rows; 16 Ki under the hook), so 96 Mi + 1 rows over (UInt64, UInt8)
    are two chunks.  That call is run here through the hook (24 Ki + 1 rows): at its real size the host would make and sort a gigabyte
    of rows, with several more of sort buffers, for the same lines of host code"""
    rng = _rng(950 + n)
    dt = (U64, U8)
    assert len(_expected_chunks(n, 16 * 1024, 16 * 1024)) == chunks
    with _context(ch, test_keydict_chunk_rows=1024) as ctx:
        d = ch.KeyDict(dt, ctx)
        base = _chunked_block(rng, 5000, dt, 2000)
        ids_in = _check_numpy(d, base, d.encode(base))
        probe = _chunked_block(rng, n, dt, 2000)
        pick = rng.integers(0, 5000, size=n)
        present = rng.random(n) < 0.6
        probe = [np.where(present, b[pick], p) for b, p in zip(base, probe)]
        before = len(d)
        ids, plan = _encode(d, capfd, probe, insert=False)
        assert plan["plan"] == "find" and int(plan["chunks"]) == chunks and len(d) == before
        want = _check_find_numpy(d, base, ids_in, probe, ids)
        assert (want == NO_ID).sum() > n // 4 and (want != NO_ID).sum() > n // 2
        del d, ids


# ---- d. growth with work in flight ----------------------------------------------------------------------------------------------------
def _growth_case(ch, O, capfd, rng, dtypes, n_distinct, min_grown, weak, family=None):
    """one block that passes `limit` while a same-tag family (or, under 20-bit tags, hundreds of them) holds verify candidates: rows are
    deferred, the table grows fourfold, every unsettled row starts again in the new cells (`restart`)"""
    total = sum(np.dtype(t).itemsize for t in dtypes)
    with _context(ch, test_keydict_weak_tags=int(weak)) as ctx:
        d = ch.KeyDict(dtypes, ctx)
        ref = _Ref(O, d)
        early = _cols_from_bytes(rng.integers(0, 256, size=(1000, total), dtype=np.uint8), dtypes)
        ref.check(early, d.encode(early))                               # keys settled before the growth: their ids must stay
        rows = rng.integers(0, 256, size=(n_distinct, total), dtype=np.uint8)
        if family is not None:
            fam = np.ascontiguousarray(family).view(np.uint8).reshape(family.shape[0], -1)[:, :total]
            at = rng.integers(0, n_distinct, size=(5, fam.shape[0]))     # each key of the family five times, spread over the block
            for r in at:
                rows[r] = fam
        cols = _cols_from_bytes(rows, dtypes)
        cols = [np.concatenate([c, e]) for c, e in zip(cols, early)]
        rehashes = ctx.counters()["TableRehashes"]
        ids, plan = _encode(d, capfd, cols)
        ref.check(cols, ids)
        assert plan["chunks"] == "1" and int(plan["grown"]) >= min_grown, plan
        assert ctx.counters()["TableRehashes"] - rehashes >= int(plan["grown"])
        if family is not None:
            assert int(plan["rounds"]) >= family.shape[0]
        if weak:
            words = _words(cols, d.key_bytes)
            assert np.unique(kc.keydict_tag(words, weak=True)).shape[0] < len(d) - 300        # hundreds of keys share their tags
        n1 = len(d)
        # a second and a third block over old, new and repeated keys, then find
        new = rng.integers(0, 256, size=(3000, total), dtype=np.uint8)
        for k in range(2):
            b = np.concatenate([rows[rng.integers(0, n_distinct, size=200_000)], new[: 1500 * (k + 1)], new[: 1500 * (k + 1)]])
            c = _cols_from_bytes(b[rng.permutation(b.shape[0])], dtypes)
            i2, plan = _encode(d, capfd, c)
            ref.check(c, i2)
            assert plan["grown"] == "0"
        assert n1 < len(d) <= n1 + 3000
        b = np.concatenate([rows[:50_000], new, rng.integers(0, 256, size=(5000, total), dtype=np.uint8)])
        c = _cols_from_bytes(b[rng.permutation(b.shape[0])], dtypes)
        i3, plan = _encode(d, capfd, c, insert=False)
        got = ref.check(c, i3, insert=False)
        assert (got == NO_ID).sum() >= 4000
        del d, ref, ids, i2, i3


def test_growth_with_a_same_tag_family_in_flight(ch, oracle_mod, capfd):
    """4.3 M distinct keys and a family of 17 under one tag in one chunk of a default dictionary: the limit is passed twice"""
    rng = _rng(1000)
    tag = int(rng.integers(0, 2**64 - 1, dtype=np.uint64, endpoint=True)) | 1
    _growth_case(ch, oracle_mod, capfd, rng, (U64, U64), 4_300_000, 2, False, kc.keydict_same_tag_keys(rng, 17, 2, tag))


def test_growth_under_20_bit_tags_for_a_mixed_width_keys256_mix(ch, oracle_mod, capfd):
    rng = _rng(1001)
    _growth_case(ch, oracle_mod, capfd, rng, (U8, U64, U64, U32), 1_300_000, 1, True)


# ---- f. at the real chunk sizes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,chunks", [(6 * MI - 1, 1), (6 * MI, 2), (28 * MI + 3, 3)])
def test_emplace_at_the_real_chunk_sizes(ch, capfd, n, chunks):
    """6 Mi - 1 rows are one chunk, 6 Mi rows are 4 Mi + 2 Mi, 28 Mi + 3 rows are 4 Mi, 16 Mi and the rest joined; every row is checked"""
    rng = _rng(1100 + chunks)
    assert len(_expected_chunks(n, 4 * MI, 64 * MI)) == chunks
    with _context(ch) as ctx:
        d = ch.KeyDict((U64, U64), ctx)
        cols = _chunked_block(rng, n, (U64, U64), 300_000)
        ids, plan = _encode(d, capfd, cols)
        assert int(plan["chunks"]) == chunks and plan["rc"] == "0"
        _check_numpy(d, cols, ids)
        del d, ids
