"""GPU parity, GROUP BY / hash join / sharding: HIP kernels through the C ABI vs the CPU
oracle and vs the reference's golden SQL outputs (tests/golden/sql_reference_rows.json)."""
import numpy as np
import pytest

import scenarios as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


@pytest.fixture(scope="module")
def ctx(ch):
    c = ch.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def engine(ch, ctx):
    class Engine:
        @staticmethod
        def HashJoin(kind, strictness, any_take_last_row=False):
            return ch.HashJoin(kind, strictness, any_take_last_row, ctx=ctx)

        @staticmethod
        def Aggregator(key_dtype, aggs, two_level_threshold=100000, size_hint=0):
            return ch.Aggregator(key_dtype, aggs, two_level_threshold, size_hint, ctx=ctx)
    return Engine


# ---- the reference's own expected rows, through the GPU path --------------------------------------
@pytest.mark.parametrize("name,fn", [
    ("00049_any_left_join", S.q00049), ("00050_any_left_join", S.q00050), ("00051_any_inner_join", S.q00051),
    ("00052_all_left_join", S.q00052), ("00053_all_inner_join", S.q00053), ("00055_join_two_numbers", S.q00055),
    ("00041_aggregation_remap", S.q00041), ("00266_read_overflow_mode", S.q00266), ("01091_sum_numbers_1e6", S.q01091),
])
def test_sql_reference_rows_on_gpu(engine, golden, name, fn):
    assert fn(engine) == golden["rows"][name]["rows"]


def test_00120_join_group_by_on_gpu(engine, golden, oracle_mod):
    L = oracle_mod.lib()  # only the SQL hash *input columns* come from the oracle's (KAT-pinned) hash functions
    got = S.q00120(engine, L.cho_sql_intHash64, L.cho_sql_intHash32)
    assert got == golden["rows"]["00120_join_and_group_by"]["rows"]


def test_02144_avg_wraps_like_reference_on_gpu(engine, golden):
    want = float(golden["rows"]["02144_avg_ubsan"]["rows"][0][0])
    for got in S.q02144(engine):
        assert f"{got:.2f}" == f"{want:.2f}"


def test_01300_avg_float64_group_by_on_gpu(engine, golden):
    want = sorted(float(r[0]) for r in golden["rows"]["01300_avg_group_by_mod5"]["rows"])
    got = S.q01300(engine)
    # Float64 avg: the device folds partial sums in a different order than the reference's 16-lane loop, so the 6th
    # printed decimal may differ by one ulp of rounding; BASELINE.json's north_star tolerance is 1e-6 relative.
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-6 * abs(w)
    assert sum(round(g, 6) == w for g, w in zip(got, want)) >= 3   # and most of them print identically


# ---- randomized parity against the oracle ------------------------------------------------------------
def _group_ref(k, cols):
    uk, inv = np.unique(k, return_inverse=True)
    return uk, inv


@pytest.mark.parametrize("key_dtype,groups,size_hint", [
    (np.uint32, 1000, 0), (np.uint32, 200_000, 0), (np.uint64, 50_000, 1_000_000), (np.int64, 3000, 0), (np.int32, 70_000, 100_000),
])
def test_group_by_sum_count_avg_matches_oracle(ch, engine, oracle_mod, key_dtype, groups, size_hint):
    O = oracle_mod
    rng = np.random.Generator(np.random.PCG64(groups))
    n = 600_000
    if np.dtype(key_dtype).kind == "i":
        k = rng.integers(-groups // 2, groups // 2, size=n).astype(key_dtype)
    else:
        k = rng.integers(0, groups, size=n).astype(key_dtype)
    k[:7] = 0
    v = rng.integers(-2**62, 2**62, size=n, dtype=np.int64)          # sums wrap modulo 2^64
    u = rng.integers(0, 2**32, size=n, dtype=np.uint32)
    f = rng.random(n)
    aggs = [(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None), (ch.AGG_AVG, np.float64), (ch.AGG_SUM, np.uint32), (ch.AGG_AVG, np.int64)]
    g = engine.Aggregator(key_dtype, aggs, size_hint=size_hint)
    o = O.Aggregator(key_dtype, aggs)
    for b in range(0, n, 65409 * 3):
        e = min(n, b + 65409 * 3)
        g.execute_on_block(k[b:e], [v[b:e], None, f[b:e], u[b:e], v[b:e]])
        o.execute_on_block(k[b:e], [v[b:e], None, f[b:e], u[b:e], v[b:e]])
    assert len(g) == len(o)
    gk, gr = g.convert_to_block()
    ok, orr = o.convert_to_block()
    gi, oi = np.argsort(gk, kind="stable"), np.argsort(ok, kind="stable")
    assert gk.dtype == ok.dtype and np.array_equal(gk[gi], ok[oi])
    for j, (kind, dt) in enumerate(aggs):
        a, b = gr[j][gi], orr[j][oi]
        assert a.dtype == b.dtype
        if a.dtype == np.float64:
            assert np.allclose(a, b, rtol=1e-6, atol=0), j   # north_star tolerance for sum/avg(Float64)
        else:
            assert np.array_equal(a, b), j                   # integer sums / counts bit-exact


def test_group_by_growth_from_small_hint_and_row_ranges(ch, engine, oracle_mod):
    # more groups than half the initial table (2^22 cells): exercises pending rows + rehash (resize on overflow)
    O = oracle_mod
    rng = np.random.Generator(np.random.PCG64(77))
    n = 5_000_000
    k = rng.integers(0, 2**40, size=n, dtype=np.uint64)
    v = rng.integers(-1000, 1000, size=n, dtype=np.int64)
    g = engine.Aggregator(np.uint64, [(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None)], size_hint=100_000)
    g.execute_on_block(k, [v, None], 0, 1_700_001)
    g.execute_on_block(k, [v, None], 1_700_001, n)
    assert g.ctx.counters()["TableRehashes"] >= 1
    gk, (gs, gc) = g.convert_to_block()
    uk, inv = np.unique(k, return_inverse=True)
    ws = np.zeros(uk.shape[0], dtype=np.int64)
    np.add.at(ws, inv, v)
    gi = np.argsort(gk)
    assert np.array_equal(gk[gi], uk) and np.array_equal(gs[gi], ws) and np.array_equal(gc[gi], np.bincount(inv).astype(np.uint64))


def test_group_by_skew_single_hot_key_and_merge(ch, engine, oracle_mod):
    O = oracle_mod
    rng = np.random.Generator(np.random.PCG64(5))
    n = 2_000_000
    k = (rng.zipf(1.1, size=n) % 1_000_000).astype(np.uint32)
    v = rng.integers(-2**31, 2**31, size=n, dtype=np.int64)
    aggs = [(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None)]
    parts = []
    for lo, hi in ((0, 900_000), (900_000, n)):
        g = engine.Aggregator(np.uint32, aggs)
        g.execute_on_block(k[lo:hi], [v[lo:hi], None])
        parts.append(g)
    parts[0].merge(parts[1])                       # mergeDataImpl on the device
    keys_c, states, rows = parts[1].export_state_columns()
    third = engine.Aggregator(np.uint32, aggs)     # mergeOnBlock-style: states arriving as columns
    third.merge_states(keys_c, states, rows)
    third.execute_on_block(k[:900_000], [v[:900_000], None])
    o = O.Aggregator(np.uint32, aggs)
    o.execute_on_block(k, [v, None])
    ok, (os_, oc) = o.convert_to_block()
    oi = np.argsort(ok)
    for g in (parts[0], third):
        gk, (gs, gc) = g.convert_to_block()
        gi = np.argsort(gk)
        assert np.array_equal(gk[gi], ok[oi]) and np.array_equal(gs[gi], os_[oi]) and np.array_equal(gc[gi], oc[oi])


def test_without_key_and_empty_input(ch, engine, oracle_mod):
    a = engine.Aggregator(None, [(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None), (ch.AGG_AVG, np.float64)])
    keys, (s, c, avg) = a.convert_to_block()
    # no-key aggregation over an empty input still yields ONE row (AggregatingTransform.cpp:700-708); avg = 0/0 = NaN
    assert keys is None and s.tolist() == [0] and c.tolist() == [0] and np.isnan(avg[0])
    v = np.arange(100_000, dtype=np.int64)
    f = np.linspace(0, 1, 100_000)
    a.execute_on_block(None, [v, None, f])
    b = engine.Aggregator(None, [(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None), (ch.AGG_AVG, np.float64)])
    b.execute_on_block(None, [v, None, f], 10, 20)
    a.merge(b)
    _, (s, c, avg) = a.convert_to_block()
    assert int(s[0]) == int(v.sum()) + int(v[10:20].sum()) and int(c[0]) == 100_010
    assert abs(avg[0] - (f.sum() + f[10:20].sum()) / 100_010) < 1e-9
    g = engine.Aggregator(np.uint32, [(ch.AGG_COUNT, None)])
    assert len(g) == 0
    gk, (gc,) = g.convert_to_block()
    assert gk.shape[0] == 0 and gc.shape[0] == 0


def _pairs(left, block, row):
    return sorted(zip(left.tolist(), block.tolist(), row.tolist()))


@pytest.mark.parametrize("kind,strict,kw", [
    ("INNER", "ALL", {}), ("LEFT", "ALL", {}), ("LEFT", "ANY", {}), ("LEFT", "ANY", {"any_take_last_row": True}),
    ("INNER", "ANY", {}), ("LEFT", "SEMI", {}), ("LEFT", "ANTI", {}),
])
def test_join_matrix_matches_oracle(ch, engine, oracle_mod, kind, strict, kw):
    O = oracle_mod
    K_ = {"INNER": ch.JOIN_INNER, "LEFT": ch.JOIN_LEFT}[kind]
    S_ = {"ALL": ch.STRICT_ALL, "ANY": ch.STRICT_ANY, "SEMI": ch.STRICT_SEMI, "ANTI": ch.STRICT_ANTI}[strict]
    rng = np.random.Generator(np.random.PCG64(31))
    rb = [rng.integers(0, 5000, size=n, dtype=np.uint64) for n in (20_000, 1, 30_001)]   # duplicates + key 0
    lb = [rng.integers(0, 10_000, size=n, dtype=np.uint64) for n in (50_000, 777)]
    rnull = (rng.integers(0, 50, size=20_000) == 0).astype(np.uint8)
    rmask = (rng.integers(0, 20, size=30_001) != 0).astype(np.uint8)
    lnull = (rng.integers(0, 40, size=50_000) == 0).astype(np.uint8)
    g, o = engine.HashJoin(K_, S_, **kw), O.HashJoin(K_, S_, **kw)
    for j in (g, o):
        j.add_block(rb[0], null_map=rnull)
        j.add_block(rb[1])
        j.add_block(rb[2], join_mask=rmask)
    assert g.total_rows == o.total_rows and g.n_keys == o.n_keys
    for keys, nm in ((lb[0], lnull), (lb[1], None)):
        gl, gb, gr, gc = g.joined_pairs(keys, nm)
        ol, ob, orow, oc = o.joined_pairs(keys, nm)
        assert gc == oc
        if strict == "ALL":
            # per left row the matches are a multiset (RowRefList order is an implementation detail) but the first
            # match of a left row is the first-inserted right row in both
            assert _pairs(gl, gb, gr) == _pairs(ol, ob, orow)
            first_g = np.concatenate([[True], gl[1:] != gl[:-1]])
            first_o = np.concatenate([[True], ol[1:] != ol[:-1]])
            assert np.array_equal(gb[first_g], ob[first_o]) and np.array_equal(gr[first_g], orow[first_o])
            rg, ro = g.probe(keys, nm), o.probe(keys, nm)
            assert np.array_equal(rg["offsets"], ro["offsets"])          # offsets_to_replicate bit-exact
        else:
            assert np.array_equal(gl, ol) and np.array_equal(gb, ob) and np.array_equal(gr, orow)   # bit-exact, in order


def test_join_max_joined_block_rows_resubmission(ch, engine, oracle_mod):
    O = oracle_mod
    rng = np.random.Generator(np.random.PCG64(8))
    right = rng.integers(0, 300, size=5000, dtype=np.uint64)
    left = rng.integers(0, 400, size=3000, dtype=np.uint64)
    g, o = engine.HashJoin(ch.JOIN_INNER, ch.STRICT_ALL), O.HashJoin(O.JOIN_INNER, O.STRICT_ALL)
    g.add_block(right)
    o.add_block(right)
    pos, total_g, total_o = 0, [], []
    while pos < left.shape[0]:                      # JoiningTransform::readExecute resubmits the not_processed tail
        gl, gb, gr, gc = g.joined_pairs(left[pos:], max_joined_block_rows=65)
        ol, ob, orow, oc = o.joined_pairs(left[pos:], max_joined_block_rows=65)
        assert gc == oc and gc > 0
        total_g += _pairs(gl + pos, gb, gr)
        total_o += _pairs(ol + pos, ob, orow)
        pos += gc
    assert total_g == total_o and len(total_g) > 10_000


def test_join_empty_sides_and_errors(ch, engine):
    j = engine.HashJoin(ch.JOIN_LEFT, ch.STRICT_ALL)
    l, b, r, c = j.joined_pairs(np.array([1, 2, 3], dtype=np.uint64))     # empty right table: LEFT keeps rows with defaults
    assert l.tolist() == [0, 1, 2] and b.tolist() == [-1, -1, -1] and c == 3
    j = engine.HashJoin(ch.JOIN_INNER, ch.STRICT_ALL)
    j.add_block(np.array([5], dtype=np.uint64))
    l, b, r, c = j.joined_pairs(np.array([], dtype=np.uint64))
    assert l.shape[0] == 0 and c == 0
    with pytest.raises(ch.ChgpuError) as e:
        j.add_block(np.array([6], dtype=np.uint64))                         # addBlockToJoin after the build phase finished
    assert e.value.code == ch._capi.ERR_LOGICAL
    with pytest.raises(ch.ChgpuError) as e:
        ch.HashJoin(ch.JOIN_FULL, ch.STRICT_SEMI)                           # FULL SEMI is not a join (joinDispatch.h:52-56): explicit CPU fallback signal
    assert e.value.code == ch._capi.ERR_NOT_IMPLEMENTED


def test_join_payload_gather_and_replicate_end_to_end(ch, ctx, engine, oracle_mod):
    # SELECT pk, bv FROM probe INNER JOIN build ON pk = bk  (C4 shape, small) — materialised on the device
    rng = np.random.Generator(np.random.PCG64(5))
    nb, npb = 200_000, 1_000_000
    bk = (rng.permutation(nb).astype(np.uint64) + 1) * np.uint64(2654435761)
    bv = rng.integers(-2**40, 2**40, size=nb, dtype=np.int64)
    pk = np.where(rng.integers(0, 2, size=npb) == 0, bk[rng.integers(0, nb, size=npb)], rng.integers(0, 2**63, size=npb, dtype=np.uint64))
    j = engine.HashJoin(ch.JOIN_INNER, ch.STRICT_ALL)
    j.add_block(bk)
    pk_col = ctx.upload(pk)
    r = j.probe_columns(pk_col)
    out_bv = ctx.upload(bv).index(r["right_rowid"], default_for_missing=True)   # fillFromBlocksAndRowNumbers (single block: rowid == row)
    out_pk = pk_col.replicate(r["offsets"])                                      # columns[i]->replicate(offsets)
    assert r["consumed"] == npb
    lut = dict(zip(bk.tolist(), bv.tolist()))
    hit = np.array([x in lut for x in pk.tolist()])
    assert r["n_out"] == int(hit.sum())
    assert np.array_equal(out_pk.numpy(), pk[hit])
    assert np.array_equal(out_bv.numpy(), np.array([lut[x] for x in pk[hit].tolist()], dtype=np.int64))
    s, c = ch.filter_sum(out_bv, ch.GE, -2**62)                                 # count(), sum(bv) checksum form
    assert c == int(hit.sum()) and int(s) == int(np.array([lut[x] for x in pk[hit].tolist()], dtype=np.int64).sum())


def test_selector_weak_hash_scatter_partition(ch, ctx, oracle_mod):
    O = oracle_mod
    rng = np.random.Generator(np.random.PCG64(5))
    n = 300_007
    for dtype in (np.uint64, np.uint32, np.int64):
        keys = rng.integers(0, 2**31, size=n).astype(dtype)
        keys[:3] = 0
        kc = ctx.upload(keys)
        assert np.array_equal(kc.get_weak_hash32().numpy(), O.weak_hash32(keys))               # bit-exact CRC32-C
        seed = rng.integers(0, 2**32, size=n, dtype=np.uint32)
        assert np.array_equal(kc.get_weak_hash32(ctx.upload(seed)).numpy(), O.weak_hash32(keys, seed))
        for shards in (1, 2, 8, 64, 256):
            sel = ch.hash_to_selector(kc, shards)
            want = O.hash_to_selector(keys, shards)
            assert np.array_equal(sel.numpy().astype(np.uint64), want)
            if shards in (8, 256):
                parts = kc.scatter(shards, sel)
                wparts = O.scatter(keys, want, shards)
                for s in range(shards):
                    assert np.array_equal(parts[s].numpy(), wparts[s])                          # stable, bit-exact
    keys = rng.integers(0, 2**63, size=n, dtype=np.uint64)
    pay = rng.integers(-5, 5, size=n).astype(np.int64)
    pay32 = rng.integers(0, 100, size=n).astype(np.uint32)
    kc = ctx.upload(keys)
    outs, counts = ch.partition_by_hash(kc, 8, [kc, ctx.upload(pay), ctx.upload(pay32)])
    want_sel = O.hash_to_selector(keys, 8)
    assert counts.tolist() == np.bincount(want_sel.astype(np.int64), minlength=8).tolist()
    order = np.argsort(want_sel, kind="stable")
    assert np.array_equal(outs[0].numpy(), keys[order]) and np.array_equal(outs[1].numpy(), pay[order]) and np.array_equal(outs[2].numpy(), pay32[order])
    # non-power-of-two scatter with an arbitrary selector
    sel3 = rng.integers(0, 3, size=n).astype(np.uint32)
    parts = ctx.upload(pay).scatter(3, ctx.upload(sel3))
    for s in range(3):
        assert np.array_equal(parts[s].numpy(), pay[sel3 == s])


@pytest.mark.parametrize("aggs_name", ["sum_count", "avg_f64", "two_args", "five_args"])
def test_group_by_partitioned_path_large_cardinality(ch, engine, oracle_mod, aggs_name):
    # >= 4 Mi rows with a large size hint take the partition -> LDS-aggregate path
    rng = np.random.Generator(np.random.PCG64(99))
    n, groups = 6_000_000, 300_000
    k = rng.integers(0, groups, size=n).astype(np.uint32)
    k[:3] = 0
    v = rng.integers(-2**62, 2**62, size=n, dtype=np.int64)
    f = rng.random(n)
    if aggs_name == "sum_count":
        aggs, args = [(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None)], [v, None]
    elif aggs_name == "avg_f64":
        aggs, args = [(ch.AGG_AVG, np.float64)], [f]
    elif aggs_name == "two_args":
        aggs, args = [(ch.AGG_SUM, np.int64), (ch.AGG_SUM, np.float64), (ch.AGG_COUNT, None)], [v, f, None]
    else:   # more argument columns than a partition buffer row carries: three partitioned calls over the same rows
        u = rng.integers(0, 2**32, size=n, dtype=np.uint32)
        aggs = [(ch.AGG_AVG, np.int64), (ch.AGG_SUM, np.uint32), (ch.AGG_COUNT, None), (ch.AGG_SUM, np.float64), (ch.AGG_AVG, np.uint32), (ch.AGG_SUM, np.int64)]
        args = [v, u, None, f, u, v]
    g = engine.Aggregator(np.uint32, aggs, size_hint=groups)
    before = g.ctx.counters()["KernelLaunches"]
    g.execute_on_block(k, args, 1, n)          # odd row_begin on purpose
    assert g.ctx.counters()["KernelLaunches"] - before >= 6   # hist + scan(3) + scatter + aggregate
    o = oracle_mod.Aggregator(np.uint32, aggs)
    o.execute_on_block(k, args, 1, n)
    gk, gr = g.convert_to_block()
    ok, orr = o.convert_to_block()
    gi, oi = np.argsort(gk), np.argsort(ok)
    assert np.array_equal(gk[gi], ok[oi])
    for j in range(len(aggs)):
        a, b = gr[j][gi], orr[j][oi]
        if a.dtype == np.float64:
            assert np.allclose(a, b, rtol=1e-6, atol=0)
        else:
            assert np.array_equal(a, b)


def _check_against_numpy(g, k, v, f=None):
    gk, res = g.convert_to_block()
    uk, inv = np.unique(k, return_inverse=True)
    ws = np.zeros(uk.shape[0], dtype=np.int64)
    np.add.at(ws, inv, v)
    gi = np.argsort(gk)
    assert np.array_equal(gk[gi], uk)
    assert np.array_equal(res[0][gi], ws)
    cnt = np.bincount(inv)
    if f is not None:
        wf = np.zeros(uk.shape[0])
        np.add.at(wf, inv, f)
        assert np.allclose(res[1][gi], wf / cnt, rtol=1e-6, atol=0)      # avg(Float64): north_star tolerance
        assert np.array_equal(res[2][gi], cnt.astype(np.uint64))
    else:
        assert np.array_equal(res[1][gi], cnt.astype(np.uint64))


@pytest.mark.parametrize("key_dtype,groups,size_hint,row_begin", [
    (np.uint32, 1, 0, 0), (np.uint64, 100, 0, 3), (np.int64, 5000, 5000, 0), (np.uint32, 4096, 0, 64), (np.int32, 3000, 3000, 1),
])
def test_group_by_lds_range_mode(ch, engine, key_dtype, groups, size_hint, row_begin):
    # 4/8-byte keys with <= 2 eight-byte arguments and few groups: the partition-aggregate kernel in RANGE mode
    rng = np.random.Generator(np.random.PCG64(groups + row_begin))
    n = 2_500_000
    k = rng.integers(0, groups, size=n).astype(key_dtype)
    if np.dtype(key_dtype).kind == "i":
        k -= groups // 2                                  # negative keys keep their raw bits
    k[row_begin:row_begin + 5] = 0                        # the zero key lives out of line
    v = rng.integers(-2**62, 2**62, size=n, dtype=np.int64)
    f = rng.random(n)
    g = engine.Aggregator(key_dtype, [(ch.AGG_SUM, np.int64), (ch.AGG_AVG, np.float64), (ch.AGG_COUNT, None)], size_hint=size_hint)
    mid = row_begin + 1_000_001
    g.execute_on_block(k, [v, f, None], row_begin, mid)
    g.execute_on_block(k, [v, f, None], mid, n)
    _check_against_numpy(g, k[row_begin:], v[row_begin:], f[row_begin:])


@pytest.mark.parametrize("groups,size_hint,n", [(7, 0, 1_000_003), (3000, 3000, 2_500_000), (400_000, 400_000, 5_000_000), (None, 0, 700_001)])
def test_group_by_with_fused_where_mask(ch, ctx, engine, groups, size_hint, n):
    # FilterTransform fused in front of the aggregation: low cardinalities read the mask inside the kernel, the partitioned /
    # keyless strategies filter the block first; rows that fail create no groups
    rng = np.random.Generator(np.random.PCG64(n))
    v = rng.integers(-2**62, 2**62, size=n, dtype=np.int64)
    f = rng.random(n)
    mask = ((rng.random(n) < 0.1) * rng.integers(1, 255, size=n)).astype(np.uint8)
    sel = mask != 0
    aggs = [(ch.AGG_SUM, np.int64), (ch.AGG_AVG, np.float64), (ch.AGG_COUNT, None)]
    if groups is None:                                   # without a key: addManyConditional + countBytesInFilter
        g = engine.Aggregator(None, aggs)
        g.execute_on_block(None, [v, f, None], 3, n, filter=mask)
        _, (s, avg, c) = g.convert_to_block()
        m = sel[3:]
        assert int(c[0]) == int(m.sum()) and int(s[0]) == int(v[3:][m].view(np.uint64).sum(dtype=np.uint64).astype(np.int64))
        assert abs(float(avg[0]) - f[3:][m].mean()) <= 1e-6 * abs(f[3:][m].mean())
        return
    k = rng.integers(0, groups, size=n).astype(np.uint32)
    k[~sel] += np.uint32(groups)                          # keys that only occur on filtered-out rows must not become groups
    g = engine.Aggregator(np.uint32, aggs, size_hint=size_hint)
    mid = n // 3
    g.execute_on_block(k, [v, f, None], 0, mid, filter=mask)
    g.execute_on_block(k, [v, f, None], mid, n, filter=mask)
    _check_against_numpy(g, k[sel], v[sel], f[sel])


def test_group_by_many_functions_take_several_range_passes(ch, engine, oracle_mod):
    # TPC-H Q1 shape: seven argument functions of three widths + count -> several passes of the RANGE kernel over the same rows
    rng = np.random.Generator(np.random.PCG64(41))
    n = 900_001
    k = rng.integers(0, 6, size=n).astype(np.uint32)
    i64 = rng.integers(-2**62, 2**62, size=n, dtype=np.int64)
    u32 = rng.integers(0, 2**32, size=n, dtype=np.uint32)
    i32 = rng.integers(-2**31, 2**31, size=n).astype(np.int32)
    f64 = rng.random(n)
    u8 = rng.integers(0, 256, size=n).astype(np.uint8)
    aggs = [(ch.AGG_SUM, np.int64), (ch.AGG_AVG, np.uint32), (ch.AGG_SUM, np.float64), (ch.AGG_COUNT, None), (ch.AGG_AVG, np.int32),
            (ch.AGG_SUM, np.uint8), (ch.AGG_AVG, np.float64), (ch.AGG_SUM, np.int32)]
    args = [i64, u32, f64, None, i32, u8, f64, i32]
    g = engine.Aggregator(np.uint32, aggs)
    o = oracle_mod.Aggregator(np.uint32, aggs)
    before = g.ctx.counters()["KernelLaunches"]
    g.execute_on_block(k, args, 5, n)
    assert g.ctx.counters()["KernelLaunches"] - before >= 4     # 8-byte x2 (two passes of <= 2), 4-byte x2, 1-byte
    o.execute_on_block(k, args, 5, n)
    gk, gr = g.convert_to_block()
    ok, orr = o.convert_to_block()
    gi, oi = np.argsort(gk), np.argsort(ok)
    assert np.array_equal(gk[gi], ok[oi])
    for j in range(len(aggs)):
        x, y = gr[j][gi], orr[j][oi]
        assert x.dtype == y.dtype
        if x.dtype == np.float64:
            assert np.allclose(x, y, rtol=1e-6, atol=0), j
        else:
            assert np.array_equal(x, y), j


@pytest.mark.parametrize("key_dtype", [np.uint32, np.uint64])
def test_group_by_partitioned_wide_path_with_hot_partition(ch, engine, key_dtype):
    # aligned first row (wide loads), a key holding 30 % of the rows: its partition is cut into many work units
    rng = np.random.Generator(np.random.PCG64(31))
    n, groups = 6_000_000, 200_000
    k = rng.integers(1, groups, size=n).astype(key_dtype)
    hot = rng.random(n) < 0.3
    k[hot] = 77_777
    k[:2] = 0
    v = rng.integers(-2**62, 2**62, size=n, dtype=np.int64)
    f = rng.random(n)
    g = engine.Aggregator(key_dtype, [(ch.AGG_SUM, np.int64), (ch.AGG_AVG, np.float64), (ch.AGG_COUNT, None)], size_hint=groups)
    before = g.ctx.counters()["KernelLaunches"]
    g.execute_on_block(k, [v, f, None])
    assert g.ctx.counters()["KernelLaunches"] - before >= 6
    _check_against_numpy(g, k, v, f)


def test_group_by_cardinality_beyond_partitioned_capacity(ch, engine):
    # more groups than partitions x LDS cells: LDS tables overflow into the HBM table, pending rows, growth
    rng = np.random.Generator(np.random.PCG64(8))
    n = 9_000_000
    k = rng.integers(0, 6_000_000, size=n).astype(np.uint32)
    v = rng.integers(-2**40, 2**40, size=n, dtype=np.int64)
    for hint in (300_000, 0):                             # a hint that is 20x too small, and none at all
        g = engine.Aggregator(np.uint32, [(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None)], size_hint=hint)
        g.execute_on_block(k, [v, None])
        _check_against_numpy(g, k, v)


def test_group_by_without_hint_adapts_to_high_cardinality(ch, engine):
    # no size hint, >= 8 Mi rows: the first 1 Mi rows are probed through the LDS-staged kernel, the rest is partitioned
    rng = np.random.Generator(np.random.PCG64(123))
    n = 9_000_000
    k = rng.integers(0, 700_000, size=n).astype(np.uint32)
    v = rng.integers(-2**40, 2**40, size=n, dtype=np.int64)
    g = engine.Aggregator(np.uint32, [(ch.AGG_SUM, np.int64), (ch.AGG_COUNT, None)])
    g.execute_on_block(k, [v, None])
    gk, (gs, gc) = g.convert_to_block()
    uk, inv = np.unique(k, return_inverse=True)
    ws = np.zeros(uk.shape[0], dtype=np.int64)
    np.add.at(ws, inv, v)
    gi = np.argsort(gk)
    assert np.array_equal(gk[gi], uk) and np.array_equal(gs[gi], ws) and np.array_equal(gc[gi], np.bincount(inv).astype(np.uint64))


@pytest.mark.parametrize("strict_name", ["SEMI", "ANTI"])
def test_join_filter_only_probe_matches_full_probe(ch, ctx, strict_name):
    # right_rowid == NULL (the right side contributes no columns): same filter and n_out as the full probe, NULL keys included
    strict = getattr(ch, "STRICT_" + strict_name)
    rng = np.random.Generator(np.random.PCG64(17))
    build = rng.integers(0, 50_000, size=30_000).astype(np.uint32)
    build[:3] = 0
    left = rng.integers(0, 100_000, size=1_000_003).astype(np.uint32)
    nulls = (rng.random(left.shape[0]) < 0.01).astype(np.uint8)
    j = ch.HashJoin(ch.JOIN_LEFT, strict, key_dtype=np.uint32, ctx=ctx)
    j.add_block(build)
    j.finish_build()
    full = j.probe_columns(left, null_map=nulls)
    fast = j.probe_columns(left, null_map=nulls, need_right_rows=False)
    assert fast["right_rowid"] is None and fast["consumed"] == full["consumed"] == left.shape[0]
    assert fast["n_out"] == full["n_out"]
    f_full, f_fast = full["filter"].numpy(), fast["filter"].numpy()
    assert np.array_equal(f_full, f_fast)
    found = np.isin(left, build) & (nulls == 0)
    assert np.array_equal(f_fast.astype(bool), found if strict_name == "SEMI" else ~found)
    with pytest.raises(ch.ChgpuError):
        ch.HashJoin(ch.JOIN_INNER, ch.STRICT_ALL, key_dtype=np.uint32, ctx=ctx).probe_columns(left, need_right_rows=False)


@pytest.mark.parametrize("strict_name", ["SEMI", "ANTI"])
@pytest.mark.parametrize("domain,with_nulls", [(50_000, True), (3_000_000, False), (3_000_000, True), (1_228_800, False)])
def test_join_filter_only_probe_dense_keys_lds_slices(ch, ctx, strict_name, domain, with_nulls):
    """dense UInt32 keys (dimension surrogate keys) and enough left rows: the key set is probed as an LDS-resident bitmap in 150 KiB
    slices of the key domain, in one sweep over the rows (1 and 3 slices here, and a domain that ends exactly at a slice boundary); left keys beyond the
    domain, the zero key, NULL keys and a row count that is not a multiple of four included"""
    strict = getattr(ch, "STRICT_" + strict_name)
    rng = np.random.Generator(np.random.PCG64(domain % 1000 + 3))
    build = rng.integers(0, domain, size=domain // 5).astype(np.uint32)
    build[0] = domain - 1
    build[1] = 0
    left = rng.integers(0, domain + domain // 3, size=3_000_003).astype(np.uint32)
    left[::1001] = 0
    left[-1] = domain - 1
    left[-2] = domain + 7
    nulls = (rng.random(left.shape[0]) < 0.02).astype(np.uint8) if with_nulls else None
    j = ch.HashJoin(ch.JOIN_LEFT, strict, key_dtype=np.uint32, ctx=ctx)
    j.add_block(build)
    j.finish_build()
    r = j.probe_columns(left, null_map=nulls, need_right_rows=False)
    found = np.isin(left, build)
    if with_nulls:
        found &= nulls == 0
    want = found if strict_name == "SEMI" else ~found
    assert np.array_equal(r["filter"].numpy().astype(bool), want)
    assert r["n_out"] == int(want.sum()) and r["consumed"] == left.shape[0]


@pytest.mark.parametrize("dtype", [np.uint16, np.int16, np.int8, np.uint8, np.int32])
def test_narrow_key_types_join_selector_and_pack(ch, ctx, oracle_mod, dtype):
    # UInt16 (Date) / Int16 / Int8 keys: raw bits zero-extended into the 64-bit table key, like every other key type
    O = oracle_mod
    info = np.iinfo(dtype)
    rng = np.random.Generator(np.random.PCG64(info.bits))
    build = rng.integers(info.min, int(info.max) + 1, size=3000).astype(dtype)
    left = rng.integers(info.min, int(info.max) + 1, size=200_003).astype(dtype)
    j = ch.HashJoin(ch.JOIN_LEFT, ch.STRICT_SEMI, key_dtype=dtype, ctx=ctx)
    j.add_block(build)
    r = j.probe_columns(left, need_right_rows=False)
    assert np.array_equal(r["filter"].numpy().astype(bool), np.isin(left, build))
    ja = ch.HashJoin(ch.JOIN_INNER, ch.STRICT_ALL, key_dtype=dtype, ctx=ctx)
    ja.add_block(build)
    assert ja.probe_columns(left)["n_out"] == int(sum(np.count_nonzero(build == v) * c for v, c in zip(*np.unique(left, return_counts=True))))
    lc = ctx.upload(left)
    assert np.array_equal(ch.hash_to_selector(lc, 8).numpy(), O.hash_to_selector(left, 8))
    assert np.array_equal(lc.get_weak_hash32().numpy(), O.weak_hash32(left))
    if info.bits <= 16:
        other = rng.integers(0, 2**32, size=left.shape[0], dtype=np.uint32)
        packed = ch.pack_fixed_keys([lc, ctx.upload(other)])
        assert np.array_equal(ch.unpack_fixed_key(packed, 0, dtype).numpy(), left)
        assert np.array_equal(ch.unpack_fixed_key(packed, info.bits // 8, np.uint32).numpy(), other)


def test_join_payload_across_many_right_blocks(ch, ctx, engine):
    # the build side arrives Block by Block (FillingRightJoinSideTransform); payload = concatenated columns + flattened row ids
    rng = np.random.Generator(np.random.PCG64(17))
    blocks_k = [rng.integers(0, 50_000, size=n, dtype=np.uint64) for n in (65_409, 1, 30_000, 65_409, 12_345)]
    blocks_v = [rng.integers(-2**50, 2**50, size=b.shape[0], dtype=np.int64) for b in blocks_k]
    j = engine.HashJoin(ch.JOIN_LEFT, ch.STRICT_ALL)
    for b in blocks_k:
        j.add_block(b)
    payload = ch.concat([ctx.upload(v) for v in blocks_v])
    left = rng.integers(0, 60_000, size=200_000, dtype=np.uint64)
    r = j.probe_columns(ctx.upload(left))
    flat = j.flatten_rowids(r["right_rowid"])
    got_v = payload.index(flat, default_for_missing=True).numpy()
    got_l = ctx.upload(left).replicate(r["offsets"]).numpy()
    all_k, all_v = np.concatenate(blocks_k), np.concatenate(blocks_v)
    order = np.argsort(all_k, kind="stable")
    sk, sv = all_k[order], all_v[order]
    lo, hi = np.searchsorted(sk, left, "left"), np.searchsorted(sk, left, "right")
    cnt = np.maximum(hi - lo, 1)                       # LEFT: unmatched rows appear once with the default 0
    assert got_l.shape[0] == int(cnt.sum()) and np.array_equal(got_l, np.repeat(left, cnt))
    pos = 0
    for i in range(0, left.shape[0], 997):             # spot-check rows: multiset of payloads per left row
        start = int(cnt[:i].sum())
        want = sorted(sv[lo[i]:hi[i]].tolist()) if hi[i] > lo[i] else [0]
        assert sorted(got_v[start:start + int(cnt[i])].tolist()) == want


@pytest.mark.parametrize("kind_name", ["RIGHT", "FULL"])
def test_right_and_full_join_all_with_non_joined_rows(ch, ctx, oracle_mod, kind_name):
    """RIGHT / FULL × ALL: joinBlock behaves like INNER / LEFT ALL (compared with the oracle's INNER / LEFT ALL, pair by pair) and sets
    the used flags; getNonJoinedBlocks returns exactly the right rows the definition gives (NULL keys, zero ON masks, keys no left
    row had), in insertion order."""
    O = oracle_mod
    rng = np.random.Generator(np.random.PCG64(len(kind_name)))
    kind = ch.JOIN_RIGHT if kind_name == "RIGHT" else ch.JOIN_FULL
    g = ch.HashJoin(kind, ch.STRICT_ALL, ctx=ctx)
    o = O.HashJoin(O.JOIN_INNER if kind_name == "RIGHT" else O.JOIN_LEFT, O.STRICT_ALL)
    build = []
    for b in range(4):
        n = [5000, 1, 0, 7001][b]
        keys = rng.integers(0, 3000, size=n).astype(np.uint64)
        keys[: min(n, 3)] = 0  # the zero key
        nm = (rng.random(n) < 0.05).astype(np.uint8) if b % 2 == 0 else None
        jm = (rng.random(n) < 0.9).astype(np.uint8) if b == 3 else None
        g.add_block(keys, nm, jm)
        o.add_block(keys, nm, jm)
        build.append((keys, nm, jm))
    probes = []
    for batch in range(3):
        n = [4000, 0, 2500][batch]
        left = rng.integers(0, 2000, size=n).astype(np.uint64)  # keys 2000..2999 of the build side are never probed
        lnm = (rng.random(n) < 0.1).astype(np.uint8) if batch == 0 else None
        gl, gb, gr, gc = g.joined_pairs(left, lnm)
        ol, ob, orow, oc = o.joined_pairs(left, lnm)
        assert gc == oc == n
        assert sorted(zip(gl.tolist(), gb.tolist(), gr.tolist())) == sorted(zip(ol.tolist(), ob.tolist(), orow.tolist()))
        probes.append((left, lnm))
    nb, nr = g.non_joined_rows()
    got = list(zip(nb.tolist(), nr.tolist()))
    assert got == sorted(got)  # insertion order
    assert got == O.non_joined_rows(build, probes)
    # matched + non-joined partition the build side
    assert len(got) + len({(b, r) for b, r in zip(gb.tolist(), gr.tolist()) if b >= 0}) <= g.total_rows


@pytest.mark.parametrize("strict_name", ["ANY", "SEMI", "ANTI"])
def test_right_any_semi_anti_joins(ch, ctx, oracle_mod, strict_name):
    """RIGHT ANY / SEMI / ANTI (joinDispatch.h:37,53,61: MapsAll with one flag per key): the first left row to find a key -- over all probed
    blocks -- is joined with every right row of it, later ones add nothing; RIGHT ANTI emits nothing.  getNonJoinedBlocks: the right rows
    whose key no left row found for ANY / ANTI, none for SEMI (JoinCommon::hasNonJoinedBlocks).  Checked against the oracle's restatement
    of joinRightColumns, triple by triple, with duplicate build keys, NULLs, ON masks, the zero key and a max_joined_block_rows cut."""
    O = oracle_mod
    rng = np.random.Generator(np.random.PCG64(len(strict_name) + 40))
    strict = getattr(ch, "STRICT_" + strict_name)
    g = ch.HashJoin(ch.JOIN_RIGHT, strict, ctx=ctx)
    build = []
    for b in range(4):
        n = [5000, 1, 0, 7001][b]
        keys = rng.integers(0, 3000, size=n).astype(np.uint64)       # ~4 right rows per key
        keys[: min(n, 3)] = 0
        nm = (rng.random(n) < 0.05).astype(np.uint8) if b % 2 == 0 else None
        jm = (rng.random(n) < 0.9).astype(np.uint8) if b == 3 else None
        g.add_block(keys, nm, jm)
        build.append((keys, nm, jm))
    probes, got = [], []
    for batch in range(3):
        n = [4000, 0, 2500][batch]
        left = rng.integers(0, 2000, size=n).astype(np.uint64)       # keys 2000..2999 of the build side are never probed
        lnm = (rng.random(n) < 0.1).astype(np.uint8) if batch == 0 else None
        if batch == 2:
            # the early stop of need_replication joins: the tail comes back unprocessed and is resubmitted (HashJoinMethodsImpl.h:434-444)
            pairs, pos = [], 0
            while pos < n:
                gl, gb, gr, gc = g.joined_pairs(left[pos:], lnm[pos:] if lnm is not None else None, max_joined_block_rows=300 if strict_name != "ANTI" else 0)
                assert gc > 0
                pairs += [(int(l) + pos, int(b), int(r)) for l, b, r in zip(gl, gb, gr)]
                pos += gc
        else:
            gl, gb, gr, gc = g.joined_pairs(left, lnm)
            assert gc == n
            pairs = list(zip(gl.tolist(), gb.tolist(), gr.tolist()))
        got.append(sorted(pairs))
        probes.append((left, lnm))
    want, flagged = O.right_once_pairs(build, probes, anti=strict_name == "ANTI")
    assert got == want
    if strict_name == "ANTI":
        assert all(len(p) == 0 for p in got)
    nb, nr = g.non_joined_rows()
    non_joined = list(zip(nb.tolist(), nr.tolist()))
    assert non_joined == sorted(non_joined)
    if strict_name == "SEMI":
        assert non_joined == []
    else:
        assert non_joined == O.non_joined_rows(build, probes)
        total = sum(k.shape[0] for k, _, _ in build)
        assert len(non_joined) + len(flagged) == total and not (set(non_joined) & set(flagged))


def test_right_join_restrictions_and_empty_cases(ch, ctx):
    with pytest.raises(ch.ChgpuError) as ei:
        ch.HashJoin(ch.JOIN_FULL, ch.STRICT_ANY, ctx=ctx)              # a TODO in the reference too (HashJoinMethodsImpl.h:511-514)
    assert ei.value.code == ch._capi.ERR_NOT_IMPLEMENTED
    j = ch.HashJoin(ch.JOIN_INNER, ch.STRICT_ALL, ctx=ctx)
    j.add_block(np.array([1, 2], dtype=np.uint64))
    with pytest.raises(ch.ChgpuError) as ei:
        j.non_joined_rows()
    assert ei.value.code == ch._capi.ERR_LOGICAL
    f = ch.HashJoin(ch.JOIN_FULL, ch.STRICT_ALL, ctx=ctx)
    f.add_block(np.array([7, 8, 7], dtype=np.uint64))
    b, r = f.non_joined_rows()  # nothing probed yet: every right row is non-joined
    assert list(zip(b.tolist(), r.tolist())) == [(0, 0), (0, 1), (0, 2)]
    l, bb, rr, c = f.joined_pairs(np.array([7, 9], dtype=np.uint64))
    assert sorted(zip(l.tolist(), bb.tolist(), rr.tolist())) == [(0, 0, 0), (0, 0, 2), (1, -1, -1)]  # FULL keeps the unmatched left row
    b, r = f.non_joined_rows()
    assert list(zip(b.tolist(), r.tolist())) == [(0, 1)]
    e = ch.HashJoin(ch.JOIN_RIGHT, ch.STRICT_ALL, ctx=ctx)
    b, r = e.non_joined_rows()  # empty right table
    assert b.shape[0] == 0


def test_00974_full_outer_join_reference_rows(ch, ctx):
    """tests/queries/0_stateless/00974_full_outer_join: two GROUP BY results joined ALL FULL OUTER on a Date key; the right rows without
    a partner come back through getNonJoinedBlocks with default left columns (Date 0 = 1970-01-01, cnt 0)"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "string_key_rows.json")) as f:
        want = [tuple(r) for r in json.load(f)["00974_full_outer_join"]["rows"]]
    day0 = int((np.datetime64("2015-12-01") - np.datetime64("1970-01-01")).astype(np.int64))

    def grouped(n):  # SELECT toDate(addDays(toDate('2015-12-01'), number)) AS dt, sum(number) FROM numbers(n) GROUP BY dt
        number = np.arange(n, dtype=np.uint64)
        agg = ch.Aggregator(np.uint16, [(ch.AGG_SUM, np.uint64)], ctx=ctx)
        agg.execute_on_block((day0 + number).astype(np.uint16), [number])
        k, (s,) = agg.convert_to_block()
        o = np.argsort(k)
        return k[o], s[o]
    ldt, lcnt = grouped(2)
    rdt, rcnt = grouped(5)
    j = ch.HashJoin(ch.JOIN_FULL, ch.STRICT_ALL, key_dtype=np.uint16, ctx=ctx)
    j.add_block(rdt)
    l, b, r, c = j.joined_pairs(ldt)
    rows = [(int(ldt[i]), int(lcnt[i]), int(rcnt[rr]) if rr >= 0 else 0) for i, rr in zip(l.tolist(), r.tolist())]
    nb, nr = j.non_joined_rows()
    rows += [(0, 0, int(rcnt[rr])) for rr in nr.tolist()]  # insertManyDefaults for q0.dt, q0.cnt
    rows.sort(key=lambda t: t[2])  # ORDER BY q1.cnt2
    fmt = [(str(np.datetime64("1970-01-01") + np.timedelta64(d, "D")), str(a), str(b2)) for d, a, b2 in rows]
    assert fmt == want


# ---- round 3: min / max states in the hash aggregator (AggregateFunctionsMinMax.cpp, SingleValueDataFixed) ----------------------------------
def test_min_max_reference_rows_on_gpu(engine, golden):
    """the reference's own expected rows: Float64 max per group (01300) and integer min / max per group (01321): bit-exact, no tolerance --
    an extremum is one of the inputs"""
    assert S.q01300_max(engine) == sorted(float(r[0]) for r in golden["rows"]["01300_max_group_by_mod2_mod3"]["rows"])
    assert S.q01321_min_max(engine) == sorted(golden["rows"]["01321_min_max_group_by_mod2_mod3"]["rows"])
    assert S.q01321_max_product(engine) == sorted(int(r[0]) for r in golden["rows"]["01321_max_product_group_by_mod7_mod5"]["rows"])


@pytest.mark.parametrize("dt", [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64, np.float32, np.float64])
def test_min_max_states_match_oracle_every_type_with_growth_and_merge(ch, ctx, oracle_mod, dt):
    O = oracle_mod
    rng = np.random.Generator(np.random.PCG64(int(np.dtype(dt).itemsize) * 7 + (np.dtype(dt).kind == "f")))
    n, groups = 300_000, 150_000                      # more groups than the initial table's max fill would take without growing? no: growth is
    keys = rng.integers(0, groups, size=n, dtype=np.uint64)   # exercised by the second block below (size_hint = 0, 4 Mi cells) -- merges rehash
    keys[:7] = 0                                       # the zero key lives out of line
    if np.dtype(dt).kind == "f":
        vals = ((rng.random(n) - 0.5) * 10.0 ** rng.integers(-30, 30, size=n)).astype(dt)
        vals[::1000] = dt(0.0)
        vals[5::1000] = dt(-0.0)
        vals[7::5000] = np.inf
        vals[9::5000] = -np.inf
    else:
        info = np.iinfo(dt)
        vals = rng.integers(info.min, info.max, size=n, dtype=np.int64 if info.min < 0 else np.uint64, endpoint=True).astype(dt)
        vals[3::1000] = info.min
        vals[4::1000] = info.max
    aggs = [(ch.AGG_MIN, dt), (ch.AGG_MAX, dt), (ch.AGG_COUNT, None), (ch.AGG_SUM, np.uint64)]
    ones = np.ones(n, dtype=np.uint64)
    A, B = ch.Aggregator(np.uint64, aggs, ctx=ctx), ch.Aggregator(np.uint64, aggs, ctx=ctx)
    OA, OB = O.Aggregator(np.uint64, aggs), O.Aggregator(np.uint64, aggs)
    h = n // 2
    for g_, o_, lo, hi in ((A, OA, 0, h), (B, OB, h, n)):
        for b in range(lo, hi, 65409):
            e = min(hi, b + 65409)
            g_.execute_on_block(keys[b:e], [vals[b:e], vals[b:e], None, ones[b:e]])
            o_.execute_on_block(keys[b:e], [vals[b:e], vals[b:e], None, ones[b:e]])
    A.merge(B)                                          # mergeDataImpl: min of mins, max of maxes
    OA.merge(OB)
    gk, (gmn, gmx, gc, gs) = A.convert_to_block()
    ok, (omn, omx, oc, os_) = OA.convert_to_block()
    i, j = np.argsort(gk), np.argsort(ok)
    assert np.array_equal(gk[i], ok[j]) and np.array_equal(gc[i], oc[j]) and np.array_equal(gs[i], os_[j])
    assert gmn.dtype == np.dtype(dt) and gmx.dtype == np.dtype(dt)
    # bit-exact: an extremum is one of the inputs (-0.0 / +0.0 compare equal: either may stand for the group, so compare by value there)
    assert np.array_equal(gmn[i], omn[j]) and np.array_equal(gmx[i], omx[j])
    # partial states travel like the sums': export, then merge into a fresh aggregator (the sharded GROUP BY's route)
    k2, words, rows = A.export_state_columns()
    Cg = ch.Aggregator(np.uint64, aggs, ctx=ctx)
    Cg.merge_states(k2, words, rows)
    Cg.merge_states(k2, words, rows)                    # twice: min / max are idempotent, counts and sums double
    ck, (cmn, cmx, cc, cs) = Cg.convert_to_block()
    q = np.argsort(ck)
    assert np.array_equal(ck[q], gk[i]) and np.array_equal(cmn[q], gmn[i]) and np.array_equal(cmx[q], gmx[i]) and np.array_equal(cc[q], 2 * gc[i])


def test_any_reference_rows_on_gpu(engine, golden):
    """01321's second query -- any(number % 2), anyLast(number % 3) GROUP BY the two -- as the reference prints it"""
    assert S.q01321_any(engine) == sorted(golden["rows"]["01321_any_group_by_mod2_mod3"]["rows"])


@pytest.mark.parametrize("dt", [np.int8, np.uint16, np.int32, np.uint64, np.float32, np.float64])
def test_any_is_the_first_row_of_the_group_like_the_oracle(ch, ctx, oracle_mod, dt):
    """any(x) = the value of the group's first row over all blocks (AggregateFunctionAny.cpp: setIfFirst), whatever order the device serves
    the rows in; merge keeps the destination's value (changeFirstTime); states travel as {claim, value} columns; a WHERE mask and a table
    that grows in between change nothing.  Bit-exact against the oracle (single-stream row order)."""
    O = oracle_mod
    rng = np.random.Generator(np.random.PCG64(int(np.dtype(dt).itemsize) + 100))
    n, groups = 400_000, 150_000
    keys = rng.integers(0, groups, size=n, dtype=np.uint64)
    keys[:5] = 0
    vals = (rng.random(n) * 200 - 100).astype(dt) if np.dtype(dt).kind == "f" else rng.integers(0, 120, size=n).astype(dt)
    mask = (rng.random(n) < 0.7).astype(np.uint8)
    aggs = [(ch.AGG_ANY, dt), (ch.AGG_COUNT, None), (ch.AGG_MAX, dt)]
    A, B = ch.Aggregator(np.uint64, aggs, ctx=ctx), ch.Aggregator(np.uint64, aggs, ctx=ctx)
    OA, OB = O.Aggregator(np.uint64, aggs), O.Aggregator(np.uint64, aggs)
    h = n // 2
    for g_, o_, lo, hi in ((A, OA, 0, h), (B, OB, h, n)):
        for b in range(lo, hi, 65409):
            e = min(hi, b + 65409)
            g_.execute_on_block(keys[b:e], [vals[b:e], None, vals[b:e]], filter=mask[b:e])
            kept = mask[b:e] != 0
            o_.execute_on_block(keys[b:e][kept], [vals[b:e][kept], None, vals[b:e][kept]])
    for agg, ora in ((A, OA), (B, OB)):
        gk, (ga, gc, gm) = agg.convert_to_block()
        ok, (oa, oc, om) = ora.convert_to_block()
        i, j = np.argsort(gk), np.argsort(ok)
        assert ga.dtype == np.dtype(dt) and np.array_equal(gk[i], ok[j]) and np.array_equal(gc[i], oc[j])
        assert np.array_equal(ga[i].view(np.uint8), oa[j].view(np.uint8)) and np.array_equal(gm[i], om[j])
    A.merge(B)                                          # groups only B has take B's value, the others keep A's
    OA.merge(OB)
    gk, (ga, gc, gm) = A.convert_to_block()
    ok, (oa, oc, om) = OA.convert_to_block()
    i, j = np.argsort(gk), np.argsort(ok)
    assert np.array_equal(gk[i], ok[j]) and np.array_equal(ga[i].view(np.uint8), oa[j].view(np.uint8)) and np.array_equal(gc[i], oc[j])
    # states: export, merge into a fresh aggregation that already holds other rows (its own values stay), and into an empty one
    k2, words, rows = A.export_state_columns()
    assert len(words) == 4
    E = ch.Aggregator(np.uint64, aggs, ctx=ctx)
    E.merge_states(k2, words, rows)
    ek, (ea, ec, em) = E.convert_to_block()
    q = np.argsort(ek)
    assert np.array_equal(ek[q], gk[i]) and np.array_equal(ea[q].view(np.uint8), ga[i].view(np.uint8)) and np.array_equal(ec[q], gc[i])
    F = ch.Aggregator(np.uint64, aggs, ctx=ctx)
    first = np.arange(1000, dtype=np.uint64)
    fv = np.full(1000, 7, dtype=dt)
    F.execute_on_block(first, [fv, None, fv])
    F.merge_states(k2, words, rows)
    fk, (fa, fc, fm) = F.convert_to_block()
    got = dict(zip(fk.tolist(), fa.tolist()))
    assert all(got[k] == 7 for k in range(1000)) and all(got[int(k)] == v for k, v in zip(gk.tolist(), ga.tolist()) if k >= 1000)
    # without key (executeWithoutKeyImpl): one state, fed block by block with a WHERE mask, merged, exported
    aggs0 = [(ch.AGG_ANY, dt), (ch.AGG_MIN, dt), (ch.AGG_MAX, dt), (ch.AGG_COUNT, None)]
    W, W2, OW, OW2 = ch.Aggregator(None, aggs0, ctx=ctx), ch.Aggregator(None, aggs0, ctx=ctx), O.Aggregator(None, aggs0), O.Aggregator(None, aggs0)
    m2 = mask.copy()
    m2[:70_000] = 0                                          # the first block passes nothing: any() must wait for the second
    for g_, o_, lo, hi in ((W, OW, 0, h), (W2, OW2, h, n)):
        for b in range(lo, hi, 65409):
            e = min(hi, b + 65409)
            g_.execute_on_block(None, [vals[b:e], vals[b:e], vals[b:e], None], filter=m2[b:e])
            kept = m2[b:e] != 0
            if kept.any():
                o_.execute_on_block(None, [vals[b:e][kept], vals[b:e][kept], vals[b:e][kept], None])
    W.merge(W2)
    OW.merge(OW2)
    _, gw = W.convert_to_block()
    _, ow = OW.convert_to_block()
    assert [x.tobytes() for x in gw] == [x.tobytes() for x in ow] and gw[0].dtype == np.dtype(dt)
    _, words, rows = W.export_state_columns()
    X = ch.Aggregator(None, aggs0, ctx=ctx)
    X.merge_states(None, words, 1)
    _, gx = X.convert_to_block()
    assert [x.tobytes() for x in gx] == [x.tobytes() for x in gw]
    Z = ch.Aggregator(None, aggs0, ctx=ctx)                 # an empty input: the defaults (insertResultInto of a state without value)
    Z.execute_on_block(None, [vals[:0], vals[:0], vals[:0], None])
    _, gz = Z.convert_to_block()
    assert [float(x[0]) for x in gz] == [0.0, 0.0, 0.0, 0.0]


def test_min_max_with_where_mask_and_table_growth(ch, ctx, oracle_mod):
    O = oracle_mod
    rng = np.random.Generator(np.random.PCG64(99))
    n = 6_000_000                                        # 3 M distinct keys: beyond the 2 Mi max fill of the initial table -> grow + rehash of max words
    keys = rng.integers(0, 3_000_000, size=n, dtype=np.uint64).astype(np.uint32)
    vals = rng.integers(-2**40, 2**40, size=n, dtype=np.int64)
    mask = (rng.random(n) < 0.7).astype(np.uint8)
    aggs = [(ch.AGG_MAX, np.int64), (ch.AGG_MIN, np.int64)]
    A = ch.Aggregator(np.uint32, aggs, ctx=ctx)
    A.execute_on_block(keys, [vals, vals], filter=mask)
    OA = O.Aggregator(np.uint32, aggs)
    m = mask.astype(bool)
    OA.execute_on_block(keys[m], [vals[m], vals[m]])
    gk, (gmx, gmn) = A.convert_to_block()
    ok, (omx, omn) = OA.convert_to_block()
    i, j = np.argsort(gk), np.argsort(ok)
    assert np.array_equal(gk[i], ok[j]) and np.array_equal(gmx[i], omx[j]) and np.array_equal(gmn[i], omn[j])
    W = ch.Aggregator(None, [(ch.AGG_MIN, np.int64), (ch.AGG_MAX, np.int64)], ctx=ctx)   # without key: one reduction per block
    W.execute_on_block(None, [vals, vals], filter=mask)
    _, (wmn, wmx) = W.convert_to_block()
    assert (int(wmn[0]), int(wmx[0])) == (int(vals[m].min()), int(vals[m].max()))


# ---- round 3: ASOF joins (JoinStrictness::Asof; RowRefs.cpp SortedLookupVector) ---------------------------------------------------------------
def _gpu_asof_pairs(ch, ctx, inequality=None):
    def jp(build, lk, lt, left):
        j = ch.AsofJoin(ch.JOIN_LEFT if left else ch.JOIN_INNER, inequality if inequality is not None else ch.ASOF_GREATER_OR_EQUALS,
                        key_dtype=lk.dtype, asof_dtype=lt.dtype, ctx=ctx)
        for k, t, nm, jm in build:
            j.add_block(k, t, nm, jm)
        l, b, r = j.joined_pairs(lk, lt)
        return list(zip(l.tolist(), b.tolist(), r.tolist()))
    return jp


def test_asof_reference_rows_on_gpu(ch, ctx, golden):
    """the reference's own expected rows: 00927_asof_join_noninclusive (LEFT, INNER `>=`, ASOF JOIN USING), 00927_asof_joins (a build side
    inserted out of time order) and the checksum of 00927_asof_join_long at its full size (1e7 build rows, 3e6 probe rows)"""
    jp = _gpu_asof_pairs(ch, ctx)
    assert S.asof_noninclusive(jp) == golden["rows"]["00927_asof_noninclusive"]["rows"]
    assert S.asof_joins_left(jp) == golden["rows"]["00927_asof_joins_left"]["rows"]

    def jp_arrays(build, lk, lt, left):
        j = ch.AsofJoin(ch.JOIN_LEFT, ch.ASOF_GREATER_OR_EQUALS, key_dtype=lk.dtype, asof_dtype=lt.dtype, ctx=ctx)
        for k, t, nm, jm in build:
            j.add_block(k, t, nm, jm)
        l, b, r = j.joined_pairs(lk, lt)
        return l, r
    assert S.asof_join_long(jp_arrays) == golden["rows"]["00927_asof_join_long"]["rows"]


@pytest.mark.parametrize("asof_dt", [np.uint32, np.int64, np.float64, np.int16, np.float32])
@pytest.mark.parametrize("ineq_name", ["LESS", "GREATER", "LESS_OR_EQUALS", "GREATER_OR_EQUALS"])
def test_asof_matches_oracle(ch, ctx, oracle_mod, ineq_name, asof_dt):
    O = oracle_mod
    rng = np.random.Generator(np.random.PCG64(len(ineq_name) * 31 + np.dtype(asof_dt).itemsize))
    ineq = getattr(ch, "ASOF_" + ineq_name)
    build = []
    seen = set()
    for b in range(3):
        n = [4000, 0, 2500][b]
        keys = rng.integers(0, 300, size=n).astype(np.uint64)
        keys[: min(n, 2)] = 0
        if np.dtype(asof_dt).kind == "f":
            t = (rng.integers(-5000, 5000, size=n) / 8.0).astype(asof_dt)
        else:
            info = np.iinfo(asof_dt)
            t = rng.integers(max(info.min, -20000), min(info.max, 20000), size=n).astype(asof_dt)
        # no two build rows with the same (key, asof): the reference's pick among equals is unspecified
        keep = np.ones(n, dtype=bool)
        for i in range(n):
            pair = (int(keys[i]), float(t[i]))
            keep[i] = pair not in seen
            seen.add(pair)
        keys, t = keys[keep], t[keep]
        n = keys.shape[0]
        nm = (rng.random(n) < 0.05).astype(np.uint8) if b == 0 else None
        jm = (rng.random(n) < 0.9).astype(np.uint8) if b == 2 else None
        if np.dtype(asof_dt).kind == "f" and n:
            t[::97] = np.nan                                             # never inserted: no comparison with NaN holds
        build.append((keys, t, nm, jm))
    n = 6000
    lk = rng.integers(0, 330, size=n).astype(np.uint64)
    lt = (rng.integers(-5200, 5200, size=n) / 8.0).astype(asof_dt) if np.dtype(asof_dt).kind == "f" else \
        rng.integers(max(np.iinfo(asof_dt).min, -21000), min(np.iinfo(asof_dt).max, 21000), size=n).astype(asof_dt)
    lnm = (rng.random(n) < 0.1).astype(np.uint8)
    if np.dtype(asof_dt).kind == "f":
        lt[::101] = np.nan
    for left in (False, True):
        j = ch.AsofJoin(ch.JOIN_LEFT if left else ch.JOIN_INNER, ineq, key_dtype=np.uint64, asof_dtype=asof_dt, ctx=ctx)
        for k, t, nm, jm in build:
            j.add_block(k, t, nm, jm)
        l, b, r = j.joined_pairs(lk, lt, lnm)
        got = list(zip(l.tolist(), b.tolist(), r.tolist()))
        want = O.asof_pairs(build, lk, lt, getattr(O, "ASOF_" + ineq_name), lnm, left)
        assert got == want
        assert left or 0 < len(got) < n
        with pytest.raises(ch.ChgpuError) as e:
            j.add_block(build[0][0], build[0][1])                        # the sorted vectors are immutable after the first lookup
        assert e.value.code == ch._capi.ERR_LOGICAL


def test_asof_restrictions_and_empty_build(ch, ctx):
    with pytest.raises(ch.ChgpuError) as e:
        ch.AsofJoin(ch.JOIN_RIGHT, ctx=ctx)                              # ASOF exists for INNER and LEFT only (joinDispatch.h:66-67)
    assert e.value.code == ch._capi.ERR_NOT_IMPLEMENTED
    j = ch.AsofJoin(ch.JOIN_LEFT, key_dtype=np.uint32, asof_dtype=np.uint32, ctx=ctx)
    l, b, r = j.joined_pairs(np.array([1, 2], dtype=np.uint32), np.array([5, 6], dtype=np.uint32))
    assert l.tolist() == [0, 1] and b.tolist() == [-1, -1]
    i = ch.AsofJoin(ch.JOIN_INNER, key_dtype=np.uint32, asof_dtype=np.uint32, ctx=ctx)
    l, b, r = i.joined_pairs(np.array([1, 2], dtype=np.uint32), np.array([5, 6], dtype=np.uint32))
    assert l.shape[0] == 0
