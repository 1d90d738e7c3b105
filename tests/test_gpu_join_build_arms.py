"""Every arm of the join's table build -- slice or generic inserts, hashed / dense / no prefilter, unique or duplicate keys, one block or
several -- under the join kinds that lay the table out differently (CSR arrays, consumed-by words, used flags).  Each case builds at the
smallest size at which its gate flips, reads the `join build plan=` debug line, probes ~100 000 left keys through chgpu_join_probe and
compares with numpy (sorted build keys + searchsorted): rows and filter bit for bit and in order, the pairs of a replicating join as a
multiset per left row, n_keys and total_rows exactly."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO_ROW = np.uint64(2**64 - 1)
TOP64 = np.uint64(2**64 - 1)
N_LEFT = 100_003
FIRST = (1 << 20) + 77      # the slice build wants >= 2^20 rows; 77 more leave a ragged last tile


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _unique_u64(rng, n):
    """n distinct keys, the zero key and 2^64 - 1 among them"""
    k = np.empty(0, dtype=np.uint64)
    while k.shape[0] < n - 2:
        k = np.unique(np.concatenate([k, rng.integers(1, 2**64 - 1, size=n - k.shape[0] + 1000, dtype=np.uint64)]))
    return rng.permutation(np.concatenate([rng.permutation(k)[: n - 2], np.array([0, TOP64], dtype=np.uint64)]))


def _unique_u32(rng, n):
    """n distinct keys in [1, 2^25), the largest of them 2^25 - 1"""
    k = (rng.permutation((1 << 25) - 2)[: n - 1] + 1).astype(np.uint32)
    return rng.permutation(np.concatenate([k, np.array([(1 << 25) - 1], dtype=np.uint32)]))


# name -> (blocks of build keys, expected fields of the build line, the flag the slice build declines with or None)
@functools.lru_cache(maxsize=None)
def _shape(name):
    if name == "u64_slices":
        return [_unique_u64(_rng(1), FIRST)], dict(plan="slices", pf="hash", unique="1"), None
    if name == "u64_below_slices":
        return [_unique_u64(_rng(2), (1 << 20) - 1)], dict(plan="generic", pf="hash", unique="1"), None
    if name == "u64_last_hashed_pf":       # 16 bits per row: 2^21 rows fill the 2^25-bit limit exactly
        return [_unique_u64(_rng(3), 1 << 21)], dict(pf="hash", unique="1"), None
    if name == "u64_past_hashed_pf":
        return [_unique_u64(_rng(4), (1 << 21) + 1)], dict(pf="none", unique="1"), None
    if name == "u32_dense_pf":
        return [_unique_u32(_rng(5), (1 << 21) + 1)], dict(plan="slices", pf="dense", unique="1"), None
    if name == "u32_past_dense_pf":
        k = _unique_u32(_rng(6), (1 << 21) + 1)
        k[np.argmax(k)] = 1 << 25
        return [k], dict(pf="none", unique="1"), None
    if name == "u64_duplicate":            # one duplicated key, both rows in the last tile
        k = _unique_u64(_rng(1), FIRST).copy()
        k[FIRST - 5] = k[FIRST - 100]
        return [k], dict(plan="generic", pf="hash", unique="0"), "dup"
    if name == "u64_three_blocks":
        k = _unique_u64(_rng(1), FIRST)
        return [k[: 1 << 20], k[:0], k[1 << 20:]], dict(plan="generic", pf="hash", unique="1"), None
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the build side sorted once, the left side (half present, half absent, the zero key, the largest key, NULL on every 37th row) and
    what searchsorted says about it; shared by the kinds of a shape and left unchanged"""
    blocks = _shape(name)[0]
    bk = np.concatenate(blocks)
    rid_of_row = np.concatenate([(np.uint64(b) << np.uint64(32)) | np.arange(blk.shape[0], dtype=np.uint64) for b, blk in enumerate(blocks)])
    rng = _rng(100 + len(name))
    top = np.iinfo(bk.dtype).max
    near = min(int(top), 2 * int(bk.max()))          # absent keys both inside the build keys' range and beyond it
    absent = np.concatenate([rng.integers(1, near, size=N_LEFT // 4, dtype=bk.dtype), rng.integers(1, int(top), size=N_LEFT // 4, dtype=bk.dtype)])
    absent = absent[~np.isin(absent, bk)]
    edges = np.array([0, 0, bk.max(), bk.max(), top, top], dtype=bk.dtype)
    present = bk[rng.integers(0, bk.shape[0], size=N_LEFT - absent.shape[0] - edges.shape[0])]
    left = rng.permutation(np.concatenate([present, absent, edges]))
    null = (np.arange(N_LEFT) % 37 == 36).astype(np.uint8)
    order = np.argsort(bk, kind="stable")             # rows by key, the rows of one key in insertion order
    sk = bk[order]
    lo, hi = np.searchsorted(sk, left, side="left"), np.searchsorted(sk, left, side="right")
    found = (hi > lo) & (null == 0)
    # the first left row that finds a key is the one that consumes it (setUsedOnce)
    first = np.zeros(N_LEFT, dtype=bool)
    first[np.flatnonzero(found)[np.unique(left[found], return_index=True)[1]]] = True
    for a in (bk, rid_of_row, left, null, order, lo, hi, found, first):
        a.setflags(write=False)
    return dict(bk=bk, rid=rid_of_row, left=left, null=null, order=order, lo=lo, hi=hi, found=found, first=first, n_keys=int(np.unique(bk).shape[0]))


def _runs(ref, counts):
    """the build rows of every left row's key, `counts` of them per left row -> (left row, row id) pairs sorted"""
    left_rows = np.repeat(np.arange(N_LEFT), counts)
    within = np.arange(left_rows.shape[0]) - np.repeat(np.cumsum(counts) - counts, counts)
    rids = ref["rid"][ref["order"][np.repeat(ref["lo"], counts) + within]]
    o = np.lexsort((rids, left_rows))
    return left_rows[o], rids[o]


def _check_pairs(ref, r, counts):
    assert np.array_equal(r["offsets"].numpy(), np.cumsum(counts).astype(np.uint64))
    got = r["right_rowid"].numpy()
    left_rows = np.repeat(np.arange(N_LEFT), counts)
    o = np.lexsort((got, left_rows))
    want_left, want_rid = _runs(ref, counts)
    assert np.array_equal(left_rows[o], want_left) and np.array_equal(got[o], want_rid)


KINDS = ["inner_all", "inner_any", "left_any_last", "left_semi_filter", "right_any"]


def _run(ch, capfd, name, kind):
    blocks, fields, declined = _shape(name)
    ref = _reference(name)
    found, first, lo, hi = ref["found"], ref["first"], ref["lo"], ref["hi"]
    make = {"inner_all": (ch.JOIN_INNER, ch.STRICT_ALL, False), "inner_any": (ch.JOIN_INNER, ch.STRICT_ANY, False),
            "left_any_last": (ch.JOIN_LEFT, ch.STRICT_ANY, True), "left_semi_filter": (ch.JOIN_LEFT, ch.STRICT_SEMI, False),
            "right_any": (ch.JOIN_RIGHT, ch.STRICT_ANY, False)}[kind]
    ctx = ch.Context(0)
    try:
        ctx.set_option("debug", 1)
        j = ch.HashJoin(make[0], make[1], any_take_last_row=make[2], key_dtype=ref["bk"].dtype, ctx=ctx)
        for b in blocks:
            j.add_block(b)
        capfd.readouterr()
        r = j.probe_columns(ref["left"], null_map=ref["null"], need_right_rows=kind != "left_semi_filter")
        err = capfd.readouterr().err
        lines = [ln for ln in err.splitlines() if ln.startswith("chgpu: join build plan=")]
        assert len(lines) == 1, err
        got_fields = dict(kv.split("=", 1) for kv in lines[0][len("chgpu: "):].split() if "=" in kv)
        print(lines[0])
        assert lines[0].split()[-2].startswith("pf=") and lines[0].split()[-1].startswith("unique="), err     # the new fields come last
        for k, v in fields.items():
            assert got_fields[k] == v, (k, err)
        assert int(got_fields["rows"]) == ref["bk"].shape[0], err
        dec = [ln for ln in err.splitlines() if ln.startswith("chgpu: join build slices declined:")]
        if declined:
            assert dec and declined in dec[0].split(":", 2)[2].split(), err
        elif "plan" in fields:
            assert not dec, err
        assert r["consumed"] == N_LEFT
        if kind == "inner_all":
            counts = np.where(found, hi - lo, 0)
            assert r["filter"] is None and r["n_out"] == int(counts.sum())
            _check_pairs(ref, r, counts)
        elif kind == "inner_any":
            assert r["offsets"] is None and r["n_out"] == int(first.sum())
            assert np.array_equal(r["filter"].numpy(), first.astype(np.uint8))
            assert np.array_equal(r["right_rowid"].numpy(), ref["rid"][ref["order"][lo[first]]])                # the first row of the key
        elif kind == "left_any_last":
            assert r["filter"] is None and r["offsets"] is None and r["n_out"] == N_LEFT
            want = np.where(found, ref["rid"][ref["order"][np.where(found, hi - 1, 0)]], NO_ROW)             # any_take_last_row
            assert np.array_equal(r["right_rowid"].numpy(), want)
        elif kind == "left_semi_filter":
            assert r["offsets"] is None and r["n_out"] == int(found.sum())
            assert np.array_equal(r["filter"].numpy(), found.astype(np.uint8))
        else:
            counts = np.where(first, hi - lo, 0)                                                             # the first finder takes every row of the key
            assert r["filter"] is None and r["n_out"] == int(counts.sum())
            _check_pairs(ref, r, counts)
            blk, row = j.non_joined_rows()
            unused = ~np.isin(ref["bk"], ref["left"][found])
            assert np.array_equal((blk.astype(np.uint64) << np.uint64(32)) | row.astype(np.uint64), ref["rid"][unused])
        assert j.total_rows == ref["bk"].shape[0] and j.n_keys == ref["n_keys"]
        del j, r
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["u64_slices", "u64_duplicate", "u64_three_blocks"])
def test_build_arm_under_every_table_layout(ch, capfd, name, kind):
    _run(ch, capfd, name, kind)


@pytest.mark.parametrize("kind", ["inner_all", "left_any_last"])
@pytest.mark.parametrize("name", ["u64_below_slices", "u64_last_hashed_pf", "u64_past_hashed_pf", "u32_dense_pf", "u32_past_dense_pf"])
def test_build_arm_at_its_gate(ch, capfd, name, kind):
    _run(ch, capfd, name, kind)
