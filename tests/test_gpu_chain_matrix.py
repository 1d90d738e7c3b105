"""chgpu_join_probe_chain where its kernels turn: many grid-stride turns of k_chain_lds / k_chain_tail / k_chain_indexes (at the natural
grid, rows derived from the device's CU count, and under the test_chain_grid option), every edge of the LDS slice geometry, the tail's
switches (coalesced step at 96 alive rows of a unit, one queue pass up to 1024, quarter passes above), row counts around the LDS threshold
and a part's end, and every representation of a join a step can read (key set, row map, finished table with a dense, a hashed or no
prefilter).  Every case compares filter bytes, the count, indexes, row ids / payload columns, carried columns and the count-only call with
the numpy reference of tests/chain_cases.py bit for bit, and asserts the chain's `debug` line, so that a case written for the 4-slice
sweep cannot quietly run in the tail."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu

SB = cc.JC_SLICE_BITS
M = 1 << 20


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _ctx(ch, **opts):
    ctx = ch.Context(0)
    for name, value in opts.items():
        ctx.set_option(name, value)
    ctx.set_option("debug", 1)
    return ctx


def _join(ch, ctx, st):
    j = ch.HashJoin(st.kind, st.strictness, key_dtype=st.dtype, ctx=ctx)
    for keys, nm, jm in st.build:
        j.add_block(np.asarray(keys, dtype=st.dtype), nm, jm)
    j.finish_build()
    return j


def _up(ctx, arr, cut=False):
    """the column, or (cut) the same rows as a view one element into a longer column: not 16-byte (4-byte for a null map) aligned"""
    if arr is None:
        return None
    if not cut:
        return ctx.upload(arr)
    return ctx.upload(np.concatenate([arr[:1], arr])).cut(1, arr.shape[0])


def _plan(err):
    lines = [ln for ln in err.splitlines() if ln.startswith("chgpu: join chain ")]
    assert len(lines) == 1, err
    m = re.fullmatch(r"chgpu: join chain rows=(\d+) parts=(\d+) lds_grid=(\d+) tail_grid=(\d+) idx_grid=(\d+) steps=\[(.*)\]", lines[0])
    assert m, lines[0]
    return dict(rows=int(m.group(1)), parts=int(m.group(2)), lds_grid=int(m.group(3)), tail_grid=int(m.group(4)), idx_grid=int(m.group(5)),
                steps=m.group(6).split(" | "), line=lines[0])


def _call(ch, capfd, joins, cols, nms, **kw):
    capfd.readouterr()
    r = ch.join_probe_chain(joins, cols, nms if nms is not None and any(m is not None for m in nms) else None, **kw)
    return r, _plan(capfd.readouterr().err)


def _explain(got, want, plan):
    """a readable account of a wrong filter: the first differing row with its part / unit / lane, and the parts whose count differs"""
    bad = np.flatnonzero(got != want)
    kp_got, kp_want = cc.kept_per_part(got), cc.kept_per_part(want)
    parts = np.flatnonzero(kp_got != kp_want)
    return (f"{bad.shape[0]} rows differ; first {cc.locate(int(bad[0]))} got={bool(got[bad[0]])}; last {cc.locate(int(bad[-1]))}; "
            f"parts with a wrong count: {parts[:12].tolist()}{'...' if parts.shape[0] > 12 else ''} "
            f"(got {kp_got[parts[:6]].tolist()} want {kp_want[parts[:6]].tolist()}); {plan['line']}")


def check(ch, capfd, ctx, steps, right_rows=None, carries=(), payloads=None, cut=(), joins=None, count_only=True, cols=None, expect=None):
    """one chain call against the reference.  right_rows: per step; payloads: per step a right column or None (a second call);
    cut: the steps whose key column (and null map) are misaligned views; expect: the `debug` line's step tokens"""
    n = steps[0].probe.shape[0]
    joins = joins if joins is not None else [_join(ch, ctx, st) for st in steps]
    cols = cols if cols is not None else [(_up(ctx, st.probe, s in cut), _up(ctx, st.null_map, s in cut)) for s, st in enumerate(steps)]
    keys, nms = [c[0] for c in cols], [c[1] for c in cols]
    ref = cc.chain_reference(steps, carries, payloads)
    r, plan = _call(ch, capfd, joins, keys, nms, right_rows=right_rows, carry=[ctx.upload(c) for c in carries], want_filter=True)
    assert plan["rows"] == n
    if expect is not None:
        assert plan["steps"] == expect, plan["line"]
    got = r["filter"].numpy()
    assert got.dtype == np.uint8 and got.shape[0] == n and (got <= 1).all()
    got = got.astype(bool)
    assert np.array_equal(got, ref["filter"]), _explain(got, ref["filter"], plan)
    assert r["kept"] == ref["kept"], plan["line"]
    assert np.array_equal(r["indexes"].numpy(), ref["indexes"]), plan["line"]
    for c, want in zip(r["carry"], ref["carry"]):
        got_c = c.numpy()
        assert got_c.dtype == want.dtype and np.array_equal(got_c, want), plan["line"]
    for s in range(len(steps)):
        if right_rows is not None and right_rows[s]:
            assert np.array_equal(r["right_rowid"][s].numpy(), ref["rowids"][s]), (s, plan["line"])
        else:
            assert r["right_rowid"][s] is None
    if payloads is not None:
        rr = [p is not None or bool(right_rows and right_rows[s]) for s, p in enumerate(payloads)]
        r3, _ = _call(ch, capfd, joins, keys, nms, right_rows=rr, right_cols=[ctx.upload(p) if p is not None else None for p in payloads], want_indexes=False)
        assert r3["kept"] == ref["kept"] and r3["indexes"] is None
        for s, p in enumerate(payloads):
            if p is not None:
                got_p = r3["right_rowid"][s].numpy()
                assert got_p.dtype == p.dtype and np.array_equal(got_p, ref["payload"][s]), (s, plan["line"])
    if count_only:
        r2, _ = _call(ch, capfd, joins, keys, nms, want_indexes=False)
        assert r2["kept"] == ref["kept"] and r2["indexes"] is None and r2["filter"] is None
    return plan, ref, joins, cols


def _payload(rows, dtype, salt=7):
    return ((np.arange(rows, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(salt)) % np.uint64(251)).astype(dtype)


def _carries(rng, n, count=2):
    kinds = [lambda: rng.integers(0, 256, size=n).astype(np.uint8), lambda: rng.integers(0, 2**32, size=n, dtype=np.uint32),
             lambda: rng.integers(0, 2**16, size=n).astype(np.uint16), lambda: rng.integers(0, 2**63, size=n, dtype=np.uint64),
             lambda: rng.integers(-2**31, 2**31, size=n).astype(np.int32), lambda: rng.integers(-128, 128, size=n).astype(np.int8),
             lambda: rng.integers(-2**62, 2**62, size=n, dtype=np.int64), lambda: rng.integers(-2**15, 2**15, size=n).astype(np.int16)]
    return [kinds[c % 8]() for c in range(count)]


# ---- many turns -----------------------------------------------------------------------------------------------------------------
def test_many_turns_at_the_natural_grid(ch, capfd):
    """(2 * CUs + 1) parts and a ragged end: workgroup 0 of k_chain_lds takes a forward, a reverse and a second forward turn, the others
    two, k_chain_tail and k_chain_indexes start their second turn.  Every part has its own hit rate in every step."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (2 * cus + 1) * cc.PART_ROWS + 5 * cc.UNIT_ROWS + 1235
    rng = _rng(cus)
    ctx = _ctx(ch)
    spec = [  # (kind, strictness, max_key, build keys, zero key, null map, (lo, hi) of the parts' hit rates)
        (cc.JOIN_LEFT, cc.STRICT_SEMI, cc.LDS_MAX_KEY, 2_000_000, True, False, (0.35, 0.95)),        # 4 slices, the zero key
        (cc.JOIN_INNER, cc.STRICT_ALL, SB - 1000, 300_000, False, False, (0.4, 0.95)),               # 1 slice, rows wanted: the row map
        (cc.JOIN_LEFT, cc.STRICT_ANTI, 2 * SB - 77, 600_000, False, True, (0.05, 0.6)),              # 2 slices (slice 0 after the one-slice step's), ANTI, null map
        (cc.JOIN_INNER, cc.STRICT_ALL, 6_000_000, 1_500_000, True, True, (0.4, 0.95)),               # beyond LDS: the tail
    ]
    steps = []
    for s, (kind, strictness, max_key, count, zero, with_nm, (lo, hi)) in enumerate(spec):
        bk = cc.build_keys(rng, max_key, count, zero).astype(np.uint32)
        probe = cc.probe_mix(rng, n, bk, cc.per_part_rates(n, lo, hi, salt=s), max_key + max_key // 8)
        nm = (rng.random(n) < 0.03).astype(np.uint8) if with_nm else None
        steps.append(cc.Step(kind, strictness, [bk], probe, nm))
    carries = _carries(rng, n, 2)
    plan, ref, joins, cols = check(ch, capfd, ctx, steps, right_rows=[False, True, False, True], carries=carries,
                                   expect=["lds:4 ks", "lds:1 dm", "lds:2 ks", "tail dense dm"])
    assert plan["lds_grid"] == cus and plan["parts"] == 2 * cus + 1 > 2 * plan["lds_grid"], plan["line"]
    assert plan["tail_grid"] == 4 * cus and plan["idx_grid"] == 8 * cus, plan["line"]
    assert (n + cc.UNIT_ROWS - 1) // cc.UNIT_ROWS > plan["idx_grid"] * cc.JCT_WAVES                      # second turns of the unit walks
    kp = cc.kept_per_part(ref["filter"])
    assert ref["kept"] > 100_000 and (kp > 0).all() and np.unique(kp[:-1]).shape[0] > cus
    del joins, cols, steps, carries, ref
    ctx.trim()
    ctx.close()


@pytest.fixture(scope="module")
def grid_pairs(ch):
    """per slice count 1..4 and step position 0..3 a build side (position 1: ANTI, 2: a null map on the probe side, 3: the zero key),
    plus an 8-byte hash step for the tail; joins live on one context with at most 16 workgroups per chain kernel"""
    rng = _rng(99)
    ctx = _ctx(ch, test_chain_grid=16)
    tops = {1: SB - 4000, 2: 2 * SB - 64, 3: 2 * SB + 5000, 4: cc.LDS_MAX_KEY}
    builds = {}
    for sl, top in tops.items():
        for pos in range(4):
            mk = top - 32 * pos
            bk = cc.build_keys(rng, mk, 700_000 if sl > 1 else 400_000, pos == 3).astype(np.uint32)
            st = cc.Step(cc.JOIN_LEFT, cc.STRICT_ANTI if pos == 1 else cc.STRICT_SEMI, [bk], np.zeros(0, dtype=np.uint32))
            builds[sl, pos] = (mk, bk, _join(ch, ctx, st), st)
    wide = rng.integers(1, 2**63, size=50_000, dtype=np.uint64)
    wide_step = cc.Step(cc.JOIN_INNER, cc.STRICT_ALL, [np.unique(wide)], np.zeros(0, dtype=np.uint64))
    yield ctx, builds, (np.unique(wide), _join(ch, ctx, wide_step), wide_step)
    ctx.close()


@pytest.mark.parametrize("turns", [2, 3, 4, 5])
def test_lds_walk_under_a_capped_grid(ch, capfd, grid_pairs, turns):
    """L in 1..4 steps x 1..4 slices each, 16 workgroups: the first three workgroups take `turns` turns, the others one fewer (a last
    turn that is a forward and one that is a reverse walk, `more` false on different turns)"""
    ctx, builds, (wide_keys, wide_join, wide_step) = grid_pairs
    rng = _rng(turns)
    n = (16 * (turns - 1) + 3) * cc.PART_ROWS + 2 * cc.UNIT_ROWS + 77
    for sl in range(1, 5):
        col = []
        for pos in range(4):
            mk, bk, j, base = builds[sl, pos]
            probe = rng.integers(0, mk + mk // 6, size=n, dtype=np.uint32, endpoint=True)
            hit = rng.random(n) < 0.6
            probe[hit] = bk[rng.integers(0, bk.shape[0], size=int(hit.sum()))]
            nm = (rng.random(n) < 0.04).astype(np.uint8) if pos == 2 else None
            st = base.on(probe, nm)
            col.append((st, j, (ctx.upload(probe), ctx.upload(nm) if nm is not None else None)))
        wprobe = np.where(rng.random(n) < 0.7, wide_keys[rng.integers(0, wide_keys.shape[0], size=n)], rng.integers(0, 2**63, size=n, dtype=np.uint64))
        wst = (wide_step.on(wprobe), wide_join, (ctx.upload(wprobe), None))
        for L in range(1, 5):
            use = col[:L] + ([wst] if L % 2 == 0 else [])
            expect = [f"lds:{sl} ks"] * L + (["tail hash table"] if L % 2 == 0 else [])
            plan, _, _, _ = check(ch, capfd, ctx, [u[0] for u in use], joins=[u[1] for u in use], cols=[u[2] for u in use],
                                  carries=_carries(rng, n, 1), count_only=L == 1, expect=expect)
            assert plan["lds_grid"] == 16 and plan["parts"] == 16 * (turns - 1) + 3 and plan["tail_grid"] == 16 and plan["idx_grid"] == 16, plan["line"]


# ---- slice edges ----------------------------------------------------------------------------------------------------------------
SLICE_EDGE_MAX_KEYS = [31, SB - 33, SB - 32, SB - 1, SB, 256 * 32 * 8 - 1, 2 * SB - 1, 2 * SB, 3 * SB + 12345, cc.LDS_MAX_KEY - 32, cc.LDS_MAX_KEY, cc.LDS_MAX_KEY + 1]


@pytest.mark.parametrize("dtype", [np.uint32, np.int32])
@pytest.mark.parametrize("max_key", SLICE_EDGE_MAX_KEYS)
def test_slice_edges(ch, capfd, max_key, dtype):
    """keys at lo - 1, lo, lo + nb - 1, lo + nb of every slice, at max_key, max_key + 1, dense_bits - 1, 2^31, 0xFFFFFFFF (negative
    Int32 probe keys), planted among filler; every second edge key is in the build side, the others are not.  SEMI and ANTI, with and
    without the zero key; a last slice of one word, slices of 256 x k words, exactly four slices, and one key more: the tail."""
    rng = _rng(max_key)
    n = 16 * cc.PART_ROWS + cc.UNIT_ROWS + 1
    ctx = _ctx(ch)
    edges = cc.slice_edge_keys(max_key)
    token = f"lds:{cc.n_slices(max_key)} ks" if cc.fits_lds(max_key) else "tail dense ks"
    assert (cc.n_slices(max_key) <= 4) == cc.fits_lds(max_key)
    for with_zero in (False, True):
        bk = cc.alternating_edge_build(rng, max_key, min(200_000, max_key // 2 + 1), with_zero).astype(np.uint32)
        probe = cc.probe_mix(rng, n, bk, 0.5, min(max_key + max_key // 4 + 64, 0xFFFFFFFF))
        cc.plant(rng, probe, edges, copies=40)
        cc.plant(rng, probe, edges, rows=np.arange(n - edges.shape[0], n))                          # the ragged end behind the last whole part too
        cc.plant(rng, probe, edges[::-1], rows=np.arange(edges.shape[0]))
        for strictness in (cc.STRICT_SEMI, cc.STRICT_ANTI):
            st = cc.Step(cc.JOIN_LEFT, strictness, [bk.astype(dtype)], probe.view(dtype))
            plan, ref, _, _ = check(ch, capfd, ctx, [st], carries=[probe], expect=[token])
            assert 0 < ref["kept"] < n
    ctx.close()


# ---- the tail's switches --------------------------------------------------------------------------------------------------------
UNIT_PLAN = {0: 0, 1: 1, 2: 95, 3: 96, 4: 1024, 5: 1025, 6: 4096, 7: (1024, 0, 0, 0), 8: (0, 0, 0, 1024), 9: (1024, 1, 0, 0), 10: (0, 1024, 1024, 0),
             11: 97, 12: 200, 13: 4096, 14: 4096, 15: (1, 1024, 0, 0), 16: (24, 24, 24, 24), 17: (24, 24, 24, 23), 18: 1023, 19: (256, 256, 256, 257),
             255: 96, 254: 1025}
TAIL_ROWS = [M - 1, M, M + 1, M + 4095, M + 4096, M + 4097]


@pytest.fixture(scope="module")
def tail_builds():
    rng = _rng(3)
    shaper = np.array([11, 3, 500], dtype=np.uint32)                                               # the LDS step that sets the alive counts
    dense = cc.build_keys(rng, cc.LDS_MAX_KEY + 4097, 900_000, True).astype(np.uint32)             # an exact bitmap beyond LDS
    wide = np.unique(rng.integers(1, 2**64 - 1, size=60_000, dtype=np.uint64))
    mk = lambda kind, strictness, keys: cc.Step(kind, strictness, [keys], np.zeros(0, dtype=keys.dtype))
    return shaper, dense, wide, (mk(cc.JOIN_LEFT, cc.STRICT_SEMI, shaper), mk(cc.JOIN_LEFT, cc.STRICT_SEMI, dense), mk(cc.JOIN_INNER, cc.STRICT_ALL, wide))


@pytest.mark.parametrize("cut", [False, True], ids=["aligned", "cut1"])
@pytest.mark.parametrize("variant", ["dense", "dense_anti", "hash", "dense+hash", "dense_anti+hash"])
@pytest.mark.parametrize("n", TAIL_ROWS)
def test_tail_switches(ch, capfd, tail_builds, n, variant, cut):
    """units at 0, 1, 95, 96, 97, 1023, 1024, 1025 and 4096 alive rows (and with one full quarter, the others empty) in front of a dense
    4-byte step beyond LDS (read whole from 96 alive rows on, row by row below or through a misaligned view), an 8-byte hash step (one
    queue pass up to 1024 alive rows, four quarter passes above) and both in sequence; a unit the coalesced step empties (12), units
    it leaves at 1025 (13) and 1024 (14) rows; row counts around the LDS threshold, a part's end and 16- / 64-byte filter ends"""
    shaper, dense, wide, (shaper_step, dense_step, wide_step) = tail_builds
    rng = _rng(n * 7 + len(variant))
    ctx = _ctx(ch)
    plan = {u: a for u, a in UNIT_PLAN.items() if (u + 1) * cc.UNIT_ROWS <= n}
    s0 = shaper_step.on(cc.unit_alive_column(rng, n, 11, 12, plan, fill_rate=0.3))
    steps, expect, cuts = [s0], ["lds:1 ks" if n >= M else "tail dense ks"], set()
    anti = "anti" in variant
    if "dense" in variant:
        absent = np.setdiff1d(np.arange(1, 5000, dtype=np.uint32), dense)[:64]
        probe = cc.probe_mix(rng, n, dense, 0.6, int(dense.max()) + 100_000)
        u = cc.UNIT_ROWS
        probe[12 * u:13 * u] = dense[7] if anti else absent[0]                                      # the coalesced step empties unit 12
        for unit, keep in ((13, 1025), (14, 1024)):
            rows = rng.permutation(u)
            probe[unit * u + rows[:keep]] = absent[1] if anti else dense[9]
            probe[unit * u + rows[keep:]] = dense[9] if anti else absent[1]
        nm = (rng.random(n) < 0.05).astype(np.uint8)
        nm[12 * u:15 * u] = 0
        steps.append(dense_step.on(probe, nm, strictness=cc.STRICT_ANTI if anti else cc.STRICT_SEMI))
        expect.append("tail dense ks")
        if cut:
            cuts.add(len(steps) - 1)
    if "hash" in variant:
        probe = np.where(rng.random(n) < 0.7, wide[rng.integers(0, wide.shape[0], size=n)], rng.integers(0, 2**64 - 1, size=n, dtype=np.uint64))
        steps.append(wide_step.on(probe, (rng.random(n) < 0.05).astype(np.uint8)))
        expect.append("tail hash table")
        if cut:
            cuts.add(len(steps) - 1)
    got_plan, ref, _, _ = check(ch, capfd, ctx, steps, right_rows=[False] * (len(steps) - 1) + [variant.endswith("hash")], carries=_carries(rng, n, 1),
                                cut=cuts, expect=expect)
    if variant in ("dense", "dense_anti"):
        a = cc.alive_per_unit_quarter(ref["filter"]).sum(axis=1)
        assert a[12] == 0 and a[13] == 1025 and a[14] == 1024 and a[0] == 0 and a[1] <= 1
    ctx.close()


def test_tail_switches_with_a_misaligned_lds_column(ch, capfd, tail_builds):
    """the shaping step read through a cut(1, n) view leaves the LDS sweep: every step runs in the tail, every unit starts whole"""
    shaper, dense, wide, _ = tail_builds
    rng = _rng(17)
    n = M + 4097
    ctx = _ctx(ch)
    s0 = cc.Step(cc.JOIN_LEFT, cc.STRICT_SEMI, [shaper], cc.unit_alive_column(rng, n, 11, 12, UNIT_PLAN, fill_rate=0.3), (rng.random(n) < 0.02).astype(np.uint8))
    s1 = cc.Step(cc.JOIN_LEFT, cc.STRICT_ANTI, [dense], cc.probe_mix(rng, n, dense, 0.4, int(dense.max()) + 5))
    check(ch, capfd, ctx, [s0, s1], cut={0}, expect=["tail dense ks", "tail dense ks"])
    check(ch, capfd, ctx, [s1, s0], cut={1}, expect=["tail dense ks", "tail dense ks"])
    ctx.close()


# ---- one join, every representation -----------------------------------------------------------------------------------------------
REPRESENTATIONS = {
    # name: (max_key, build rows, LDS / tail token of a key set, token of the finished table)
    "dense_lds": (3 * SB - 5, 300_000, "lds:3", "lds:3"),
    "dense_at_limit": (cc.KEYSET_LIMIT - 1, 200_000, "tail dense", "tail hash"),
    "dense_large": (cc.KEYSET_LIMIT - 1, (1 << 21) + 1000, "tail dense", "tail dense"),
    "sparse_hashed_prefilter": (cc.KEYSET_LIMIT, 200_000, None, "tail hash"),
    "too_large_for_a_prefilter": (3 * cc.KEYSET_LIMIT, (1 << 21) + 1000, None, "tail nopf"),
}


@pytest.mark.parametrize("name", list(REPRESENTATIONS))
def test_one_join_in_every_state_gives_one_answer(ch, capfd, name):
    """the chain run with the join (a) fresh, rows not wanted: the key set (k_join_keyset_fill); (b) fresh, rows wanted: the row map
    (k_join_dense_fill, k_join_bitmap_from_dense); (c) after tune_join_no_dense_map: the table; (d) after probe_columns built the table;
    then (a) and (b) again on the join of (b) and (a).  Every state gives the reference's filter, indexes and row ids."""
    max_key, rows, ks_token, table_token = REPRESENTATIONS[name]
    rng = _rng(rows)
    n = 16 * cc.PART_ROWS + 4097
    bk = cc.build_keys(rng, max_key, rows, True).astype(np.uint32)
    probe = cc.probe_mix(rng, n, bk, 0.5, min(2 * max_key, 0xFFFFFFFF))
    cc.plant(rng, probe, [0, max_key, max_key + 1, max_key - 1, 0xFFFFFFFF], copies=50)
    st = cc.Step(cc.JOIN_LEFT, cc.STRICT_SEMI, [bk], probe, (rng.random(n) < 0.05).astype(np.uint8))
    other = cc.Step(cc.JOIN_LEFT, cc.STRICT_ANTI, [np.arange(1, 1000, 3, dtype=np.uint32)], rng.integers(0, 1200, size=n).astype(np.uint32))
    pay = _payload(bk.shape[0], np.uint32)
    ks = ks_token is not None

    ctx = _ctx(ch)
    ja = _join(ch, ctx, st)
    check(ch, capfd, ctx, [other, st], joins=[_join(ch, ctx, other), ja], expect=["lds:1 ks", f"{ks_token} ks" if ks else f"{table_token} table"])
    jb = _join(ch, ctx, st)
    check(ch, capfd, ctx, [other, st], joins=[_join(ch, ctx, other), jb], right_rows=[False, True], payloads=[None, pay],
          expect=["lds:1 ks", f"{ks_token} dm" if ks else f"{table_token} table"])
    # the key set of (a) with rows wanted now: the row map is added; the row map of (b) with rows not wanted: its key set answers
    check(ch, capfd, ctx, [st], joins=[ja], right_rows=[True], expect=[f"{ks_token} dm" if ks else f"{table_token} table"])
    check(ch, capfd, ctx, [st], joins=[jb], expect=[f"{ks_token} ks" if ks else f"{table_token} table"])
    jd = _join(ch, ctx, st)
    r = jd.probe_columns(ctx.upload(probe[:1000]), ctx.upload(st.null_map[:1000]))
    assert np.array_equal(r["filter"].numpy().astype(bool), cc.step_filter(cc.Step(st.kind, st.strictness, st.build, probe[:1000], st.null_map[:1000])))
    check(ch, capfd, ctx, [st, other], joins=[jd, _join(ch, ctx, other)], right_rows=[True, False], payloads=[pay, None], expect=[f"{table_token} table", "lds:1 ks"])
    check(ch, capfd, ctx, [st], joins=[jd], expect=[f"{table_token} table"])
    ctx.close()

    ctx = _ctx(ch, tune_join_no_dense_map=1)
    jc = _join(ch, ctx, st)
    check(ch, capfd, ctx, [st], joins=[jc], right_rows=[True], payloads=[pay], carries=[probe], expect=[f"{table_token} table"])
    ctx.close()


def test_duplicate_build_keys(ch, capfd, oracle_mod):
    """SEMI with rows wanted over duplicates: the row map's deferred duplicate flag sends the step to the table, which names the first
    row of a key.  INNER ALL over duplicates is refused, and the join still answers probe_columns like the oracle."""
    rng = _rng(8)
    n = 16 * cc.PART_ROWS + 100
    bk = cc.build_keys(rng, 2 * SB - 9, 150_000, True).astype(np.uint32)
    bk = np.concatenate([bk, bk[:5000], bk[100:200], np.zeros(2, dtype=np.uint32)])
    probe = cc.probe_mix(rng, n, bk, 0.5, 2 * SB + 999)
    ctx = _ctx(ch)
    st = cc.Step(cc.JOIN_LEFT, cc.STRICT_SEMI, [bk], probe)
    _, ref, _, _ = check(ch, capfd, ctx, [st], right_rows=[True], payloads=[_payload(bk.shape[0], np.uint16)], expect=["lds:2 table"])
    assert np.isin(ref["rowids"][0], np.arange(bk.shape[0] - 5102, dtype=np.uint64)).all()        # never one of the later copies
    check(ch, capfd, ctx, [st], expect=["lds:2 ks"])                                              # a set does not mind duplicates
    # the same duplicates in a second block: the row map declines (two blocks), the table's row ids carry the block number
    st2 = cc.Step(cc.JOIN_LEFT, cc.STRICT_SEMI, [bk[:60_000], bk[50_000:]], probe)
    check(ch, capfd, ctx, [st2], right_rows=[True], expect=["lds:2 table"])

    allj = ch.HashJoin(ch.JOIN_INNER, ch.STRICT_ALL, key_dtype=np.uint32, ctx=ctx)
    allj.add_block(bk)
    allj.finish_build()
    small = probe[:5000]
    for rr in (None, [True]):
        with pytest.raises(ch.ChgpuError) as e:
            ch.join_probe_chain([allj], [ctx.upload(probe)], right_rows=rr)
        assert e.value.code == ch._capi.ERR_NOT_IMPLEMENTED
        o = oracle_mod.HashJoin(ch.JOIN_INNER, ch.STRICT_ALL)
        o.add_block(bk)
        want, got = o.joined_pairs(small), allj.joined_pairs(small)
        assert want[3] == got[3] == small.shape[0]
        a = sorted(zip(want[0].tolist(), want[1].tolist(), want[2].tolist()))
        b = sorted(zip(got[0].tolist(), got[1].tolist(), got[2].tolist()))
        assert a == b and len(a) > small.shape[0] // 2
    ctx.close()


def test_one_join_at_two_steps_and_multi_block_build_sides(ch, capfd):
    rng = _rng(21)
    n = 16 * cc.PART_ROWS + 4095
    ctx = _ctx(ch)
    bk = cc.build_keys(rng, SB + 31, 150_000, True).astype(np.uint32)
    p0, p1 = cc.probe_mix(rng, n, bk, 0.7, SB + 9999), cc.probe_mix(rng, n, bk, 0.7, SB + 9999)
    for rr, token in ((None, "lds:2 ks"), ([True, True], "lds:2 dm"), ([False, True], "lds:2 dm")):
        j = _join(ch, ctx, cc.Step(cc.JOIN_LEFT, cc.STRICT_SEMI, [bk], p0))
        steps = [cc.Step(cc.JOIN_LEFT, cc.STRICT_SEMI, [bk], p0), cc.Step(cc.JOIN_LEFT, cc.STRICT_SEMI, [bk], p1)]
        plan, _, _, _ = check(ch, capfd, ctx, steps, joins=[j, j], right_rows=rr, count_only=False)
        assert plan["steps"][1] == token and plan["steps"][0].startswith("lds:2 "), plan["line"]
    # two and three blocks (one of them empty): row ids carry the block number; a right column inside the chain is refused
    for blocks in ([bk[:70_000], bk[70_000:]], [bk[:10], np.zeros(0, dtype=np.uint32), bk[10:]]):
        steps = [cc.Step(cc.JOIN_INNER, cc.STRICT_ALL, blocks, p0), cc.Step(cc.JOIN_LEFT, cc.STRICT_SEMI, [bk[::2]], p1)]
        plan, ref, joins, cols = check(ch, capfd, ctx, steps, right_rows=[True, True], carries=[p1],
                                       expect=["lds:2 table", f"lds:{cc.n_slices(cc.build_stats(steps[1])[0])} dm"])
        assert (ref["rowids"][0] >> np.uint64(32)).max() == len(blocks) - 1
        with pytest.raises(ch.ChgpuError) as e:
            ch.join_probe_chain(joins, [c[0] for c in cols], right_rows=[True, True], right_cols=[ctx.upload(_payload(bk.shape[0], np.uint8)), None])
        assert e.value.code == ch._capi.ERR_NOT_IMPLEMENTED
    ctx.close()


@pytest.mark.parametrize("right_rows", [False, True])
def test_build_side_null_maps_and_join_masks(ch, capfd, right_rows):
    """max_key and has_zero count valid rows only: the largest key (far beyond every bitmap) and the zero key sit on masked-out rows"""
    rng = _rng(33)
    n = 16 * cc.PART_ROWS + 17
    ctx = _ctx(ch)
    bk = cc.build_keys(rng, SB - 64, 50_000, False).astype(np.uint32)
    keys = np.concatenate([bk, np.array([0xFFFFFFF0, 0, 3 * SB, SB - 10], dtype=np.uint32)])
    nm = np.zeros(keys.shape[0], dtype=np.uint8)
    jm = np.ones(keys.shape[0], dtype=np.uint8)
    nm[-4], jm[-3], nm[-2] = 1, 0, 1
    nm[:200] = 1
    jm[300:700] = 0
    probe = cc.probe_mix(rng, n, keys, 0.6, SB + 64)
    cc.plant(rng, probe, [0, 0xFFFFFFF0, 3 * SB, SB - 10, SB - 64], copies=100)
    for v, build in enumerate(([(keys, nm, jm)], [(keys, nm, None)], [(keys, None, np.where(nm, 0, jm).astype(np.uint8))])):
        for strictness in (cc.STRICT_SEMI, cc.STRICT_ANTI):
            st = cc.Step(cc.JOIN_LEFT, strictness, build, probe)
            assert cc.build_stats(st) == (SB - 10, v == 1)
            rr = right_rows and strictness == cc.STRICT_SEMI
            check(ch, capfd, ctx, [st], right_rows=[rr], payloads=[_payload(keys.shape[0], np.uint64)] if rr else None,
                  expect=["lds:1 dm" if rr else "lds:1 ks"])
    ctx.close()


@pytest.mark.parametrize("n", [1000, 16 * 65536 + 5])
def test_empty_build_sides(ch, capfd, n):
    rng = _rng(n)
    ctx = _ctx(ch)
    probe = rng.integers(0, 50, size=n).astype(np.uint32)
    other = cc.Step(cc.JOIN_LEFT, cc.STRICT_SEMI, [np.arange(0, 40, dtype=np.uint32)], rng.integers(0, 50, size=n).astype(np.uint32))
    for build in ([], [np.zeros(0, dtype=np.uint32)]):
        for kind, strictness in ((cc.JOIN_LEFT, cc.STRICT_SEMI), (cc.JOIN_LEFT, cc.STRICT_ANTI), (cc.JOIN_INNER, cc.STRICT_ALL)):
            for rr in (False, True):
                st = cc.Step(kind, strictness, build, probe)
                _, ref, _, _ = check(ch, capfd, ctx, [other, st], right_rows=[rr, rr], carries=[probe])
                assert ref["kept"] == (int(cc.step_filter(other).sum()) if strictness == cc.STRICT_ANTI else 0)
    ctx.close()


@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint64])
def test_signed_narrow_and_wide_keys(ch, capfd, dtype):
    """keys are compared as the column's bytes, zero-extended: a negative key matches itself and nothing else (a negative Int32 build key
    is a key above 2^31: no key set, the table)"""
    rng = _rng(np.dtype(dtype).itemsize * 3 + (np.dtype(dtype).kind == "i"))
    n = 16 * cc.PART_ROWS + 333
    ctx = _ctx(ch)
    info = np.iinfo(dtype)
    lo, hi = max(int(info.min), -40_000), min(int(info.max), 40_000)
    domain = np.arange(lo, hi + 1, dtype=np.int64)
    bk = rng.permutation(domain)[:max(3, domain.shape[0] // 3)].astype(dtype)
    ends = np.array([info.min, info.max, 0], dtype=dtype)
    bk = np.unique(np.concatenate([bk, ends]))
    probe = rng.choice(np.concatenate([domain.astype(dtype), ends]), size=n)
    size = np.dtype(dtype).itemsize
    for kind, strictness, rr in ((cc.JOIN_LEFT, cc.STRICT_SEMI, False), (cc.JOIN_LEFT, cc.STRICT_ANTI, False), (cc.JOIN_INNER, cc.STRICT_ALL, True)):
        st = cc.Step(kind, strictness, [rng.permutation(bk)], probe, (rng.random(n) < 0.1).astype(np.uint8))
        if size == 8:
            token = "tail hash table"
        elif size == 4:
            token = "tail hash table"                                # max_key >= 2^31
        else:
            token = "tail dense dm" if rr else "tail dense ks" if strictness != cc.STRICT_ALL else "tail dense table"
        check(ch, capfd, ctx, [st], right_rows=[rr], payloads=[_payload(bk.shape[0], np.int16 if size < 8 else np.uint64)] if rr else None, expect=[token])
    ctx.close()


def test_eight_steps_eight_carries_and_nine_refused(ch, capfd):
    rng = _rng(88)
    n = 16 * cc.PART_ROWS + 2049
    ctx = _ctx(ch)
    steps = []
    for s in range(9):
        mk = [SB - 1, 2 * SB - 1, 5000, 3 * SB - 1, cc.LDS_MAX_KEY, 70_000, SB + 31, 900, 40][s]
        bk = cc.build_keys(rng, mk, min(mk // 2, 200_000), s % 3 == 0).astype(np.uint32)
        kind, strictness = [(cc.JOIN_LEFT, cc.STRICT_SEMI), (cc.JOIN_LEFT, cc.STRICT_ANTI), (cc.JOIN_INNER, cc.STRICT_ALL), (cc.JOIN_LEFT, cc.STRICT_ANY)][s % 4]
        steps.append(cc.Step(kind, strictness, [bk], cc.probe_mix(rng, n, bk, 0.2 if strictness == cc.STRICT_ANTI else 0.85, mk + 50),
                             (rng.random(n) < 0.02).astype(np.uint8) if s % 2 else None))
    carries = _carries(rng, n, 9)
    plan, _, joins, cols = check(ch, capfd, ctx, steps[:8], right_rows=[s % 4 >= 2 for s in range(8)], carries=carries[:8],
                                 payloads=[_payload(st.build[0][0].shape[0], np.uint8) if s % 4 == 2 else None for s, st in enumerate(steps[:8])])
    assert plan["steps"] == ["lds:1 ks", "lds:2 ks", "lds:1 dm", "skip dm", "lds:4 ks", "lds:1 ks", "lds:2 dm", "skip dm"], plan["line"]
    j9 = _join(ch, ctx, steps[8])
    keys = [c[0] for c in cols]
    with pytest.raises(ch.ChgpuError) as e:
        ch.join_probe_chain(joins + [j9], keys + [ctx.upload(steps[8].probe)])
    assert e.value.code == ch._capi.ERR_NOT_IMPLEMENTED
    with pytest.raises(ch.ChgpuError) as e:
        ch.join_probe_chain(joins, keys, carry=[ctx.upload(c) for c in carries])
    assert e.value.code == ch._capi.ERR_NOT_IMPLEMENTED
    ctx.close()
