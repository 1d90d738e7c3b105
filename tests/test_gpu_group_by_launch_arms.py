"""Every arm of the GROUP BY host dispatch (agg_kernels.hip: agg_tile_run, agg_scatter_run, agg_add_block_ranged) that the rest of the
suite does not reach, each checked against numpy (np.unique + per-group sums) AND recognised by the fields of its `debug` line, so that
a case cannot pass through a different arm.

Arms the existing tests reach (derived from their shapes and the plan functions; they compare results but, except where noted, do not
assert the arm):

  tile-sorted plan, partition pass k_rp_tilesort<TILE, KT, .., AT, EX>
    KT=u32 x (u64,0) (u32,0) (u32,3) (u32,4)      test_gpu_round2: partitioned_shapes, tile_sorted_plan_widens_narrow_arguments
    KT=u64 x (u64,0)                              test_gpu_round2: partitioned_shapes, tile_sorted_plan_edge_cases
  tile-sorted plan, aggregate pass k_agg_tiles_lds<KT, OPS, TILE>
    u32, u64 x 0x51 0x15 0x1 0x957                test_gpu_round2 (sum_count, count_sum, sum / the second word pass, avg_f64),
                                                  test_gpu_group_by_limits (0x15, plan asserted), test_gpu_crafted_keys, test_gpu_float_sums
  scatter plan, histogram
    k_rp_hist_wide<u32>, <u64>                    test_gpu_group_by_limits "partitioned" (plan asserted)
    k_gb_hist                                     test_gpu_round2 partitioned_shapes with UInt16 keys
  scatter plan, k_rp_scatter<TILE, KT>
    (12288,u32) (8192,u64)                        test_gpu_group_by_limits "partitioned"
  scatter plan, k_gb_scatter<TILE, KT, WIDE>
    (12288,u32,false) (4096,u32,false)            test_gpu_round2 partitioned_shapes with UInt16 keys (K = 1 and K = 2)
  scatter plan, aggregate pass k_agg_part_lds<KT, 8, KT, false, OPS>
    u32 x 0x51 0x15 0x1 0x957 0x521               test_gpu_round2 partitioned_shapes with UInt16 keys
    u64 x 0x15                                    test_gpu_group_by_limits, test_gpu_crafted_keys
  ranged plan k_agg_part_lds<KT, AW, KS, EXT>
    KS = u8 u16 u32 u64 x AW = 8                  test_gpu_group_by_limits "ranged" (plan asserted)

Added here: the tile-sorted partition pass with 8-byte keys over UInt32 / Int32 / Float32 arguments; the tile-sorted codes 0x53 0x3 0x61
0x16 0x97 0x967 with both key widths; k_rp_scatter (8192,u32); k_gb_scatter (8192,u32,false) (8192,u64,false) (4096,u64,false)
(12288,u64,false) (4096,u32,true) (4096,u64,true) (12288,u32,true) (12288,u64,true); the scatter plan's codes 0x5 0x53 0x3 0x21 0x97 and the generic OPS = 0 with 4-byte keys and all but
0x15 with 8-byte keys; the ranged plan's 1-, 2- and 4-byte arguments with and without extension over every key width.

Not reachable below 2^32 rows without the tune_gb_tile option, so not here: k_gb_scatter<8192, KT, true> (keys alone fit 12288-row tiles,
one wide 8-byte word goes through k_rp_scatter unless n + slack >= 2^32, two words only fit 4096-row tiles).

Shapes: (4 << 20) + 77 rows -- the partition gate is 4 Mi rows, the tile-sorted plan needs TILE x CUs rows, the ragged end is the last
tile's -- over ~2^19 distinct keys with the zero key and the all-ones key, a size hint of 2^19; 200 000 rows and 1000 groups for the
ranged plan.  A view that starts at row 1 makes the first row miss 16-byte alignment (the non-wide arms).

Tolerances: integer sums and counts bit for bit (mod 2^64); fixed-point Float64 sums bit for bit against math.fsum; avg at rtol 1e-6 (as
test_gpu_crafted_keys); Float64 sums with deterministic_float_sums off are atomic double adds in hardware order: any order of n adds
stays within (n - 1) * 2^-53 * sum|v| of the exact sum (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4, to first order;
the bound below uses n * 2^-52 to cover the higher-order terms)."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_BIG, HINT_BIG = (4 << 20) + 77, 1 << 19
N_RANGED, HINT_RANGED = 200_000, 1000
DTYPES = {"u64": np.uint64, "i64": np.int64, "i64b": np.int64, "u64b": np.uint64, "u32": np.uint32, "i32": np.int32, "u16": np.uint16, "i16": np.int16,
          "u8": np.uint8, "i8": np.int8, "f32": np.float32, "f64": np.float64}


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


def _rng(*seed):
    return np.random.Generator(np.random.PCG64([ord(c) for c in "-".join(map(str, seed))]))


@functools.lru_cache(maxsize=None)
def _keys(kd, rows, groups):
    """rows + 1 keys (a view may start at row 1) over `groups` distinct values, the zero key and the all-ones key among them"""
    rng = _rng("keys", kd, rows)
    top = np.iinfo(kd).max
    if groups > top:
        uk = np.arange(top + 1, dtype=np.uint64)
    else:
        uk = np.unique(np.concatenate([rng.integers(1, top, size=groups, dtype=np.uint64), np.array([0, top], dtype=np.uint64)]))
    k = uk[rng.integers(0, uk.shape[0], size=rows + 1)]
    k[1:1 + uk.shape[0]] = rng.permutation(uk)           # every key in either view
    k = k.astype(kd)
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def _arg(name, rows):
    rng = _rng("arg", name, rows)
    dt = np.dtype(DTYPES[name])
    if dt.kind == "f":
        v = (rng.random(rows + 1) * 2000.0 - 1000.0).astype(dt)
    else:
        info = np.iinfo(dt)
        v = rng.integers(info.min, info.max, size=rows + 1, dtype=dt, endpoint=True)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _grouping(kd, rows, groups, start):
    k = _keys(kd, rows, groups)[start:start + rows]
    order = np.argsort(k, kind="stable")
    sk = k[order]
    starts = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))
    cnt = np.diff(np.concatenate([starts, [rows]])).astype(np.uint64)
    return sk[starts], order, starts, cnt


@functools.lru_cache(maxsize=None)
def _ref_sum(kd, rows, groups, start, name):
    """integers: the sums mod 2^64 as uint64; floats: (math.fsum per group, sum of magnitudes per group)"""
    _, order, starts, _ = _grouping(kd, rows, groups, start)
    v = _arg(name, rows)[start:start + rows][order]
    if v.dtype.kind == "f":
        v = v.astype(np.float64)
        ends = np.concatenate([starts[1:], [rows]])
        exact = np.array([math.fsum(v[a:b]) for a, b in zip(starts.tolist(), ends.tolist())])
        return exact, np.add.reduceat(np.abs(v), starts)
    wide = v.astype(np.int64).view(np.uint64) if v.dtype.kind == "i" else v.astype(np.uint64)
    return np.add.reduceat(wide, starts)


def S(name):
    return ("sum", name)


COUNT = ("count", None)
NO_TILED = {"tune_gb_no_tiled": 1}
PLAIN_F64 = {"deterministic_float_sums": 0}
COUNT64 = {"tune_gb_nocnt32": 1}


def _tile(kd, aggs, ops, arg_w=8, ex=0, **opts):
    tile = 12288 if np.dtype(kd).itemsize == 4 else 8192
    return dict(plan="tile-sorted GROUP BY", kd=kd, aggs=aggs, opts=opts, rows=N_BIG, groups=HINT_BIG, hint=HINT_BIG, start=0,
                lines=[dict(tile=str(tile), ops=hex(ops), arg_w=str(arg_w), ex=str(ex))])


def _scatter(kd, aggs, lines, start=0, hint=HINT_BIG, **opts):
    return dict(plan="partitioned GROUP BY", kd=kd, aggs=aggs, opts={**NO_TILED, **opts}, rows=N_BIG, groups=HINT_BIG, hint=hint, start=start,
                lines=[dict(level="0", tile=str(t), ops=hex(o), wide=str(w), rp_tile=str(r)) for t, o, w, r in lines])


def _ranged(kd, arg, aw, ext):
    return dict(plan="ranged GROUP BY", kd=kd, aggs=[S(arg), COUNT], opts={}, rows=N_RANGED, groups=HINT_RANGED, hint=HINT_RANGED, start=0,
                lines=[dict(passes="1", key_w=str(np.dtype(kd).itemsize), aw=str(aw), ext=str(ext))])


CASES = {}
# ---- tile-sorted plan: (tile, ops, arg_w, ex) ----
for _a, _ops, _ex in (("u32", 0x51, 0), ("i32", 0x51, 3), ("f32", 0x957, 4)):
    CASES[f"tile-u64-arg_{_a}"] = _tile(np.uint64, [S(_a), COUNT], _ops, arg_w=4, ex=_ex)
for _kd in (np.uint32, np.uint64):
    _k = np.dtype(_kd).name
    CASES[f"tile-{_k}-0x53"] = _tile(_kd, [S("f64"), COUNT], 0x53, **PLAIN_F64)
    CASES[f"tile-{_k}-0x3"] = _tile(_kd, [S("f64")], 0x3, **PLAIN_F64)
    CASES[f"tile-{_k}-0x61"] = _tile(_kd, [S("i64"), COUNT], 0x61, **COUNT64)
    CASES[f"tile-{_k}-0x16"] = _tile(_kd, [COUNT, S("u64")], 0x16, **COUNT64)
    CASES[f"tile-{_k}-0x97"] = _tile(_kd, [S("f64")], 0x97)
    CASES[f"tile-{_k}-0x967"] = _tile(_kd, [S("f64"), COUNT], 0x967, **COUNT64)
# ---- scatter plan: lines of (tile, ops, wide, rp_tile); one 8-byte word from an aligned row goes through k_rp_scatter ----
for _kd in (np.uint32, np.uint64):
    _k = np.dtype(_kd).name
    _t1 = 12288 if _kd is np.uint32 else 8192             # K = 1
    CASES[f"scatter-{_k}-0x5"] = _scatter(_kd, [COUNT], [(12288, 0x5, 1, 0)])                      # K = 0: keys alone fit 12288-row tiles
    CASES[f"scatter-{_k}-0x53"] = _scatter(_kd, [S("f64"), COUNT], [(_t1, 0x53, 1, _t1)], **PLAIN_F64)
    CASES[f"scatter-{_k}-0x3"] = _scatter(_kd, [S("f64")], [(_t1, 0x3, 1, _t1)], **PLAIN_F64)
    CASES[f"scatter-{_k}-0x97"] = _scatter(_kd, [S("f64")], [(_t1, 0x97, 1, _t1)])
    CASES[f"scatter-{_k}-0x21-two_wide_words"] = _scatter(_kd, [S("i64"), S("u64")], [(4096, 0x21, 1, 0)])
    # three argument words: a call with two of them, then one with the third; each leaves state words of the other alone (no code)
    CASES[f"scatter-{_k}-generic"] = _scatter(_kd, [S("i64"), S("u64"), S("i64b")], [(4096, 0x0, 1, 0), (_t1, 0x0, 1, _t1)])
CASES["scatter-uint64-0x51"] = _scatter(np.uint64, [S("i64"), COUNT], [(8192, 0x51, 1, 8192)])
CASES["scatter-uint64-0x1-odd_first_row"] = _scatter(np.uint64, [S("i64")], [(8192, 0x1, 0, 0)], start=1)
CASES["scatter-uint64-0x521-odd_first_row"] = _scatter(np.uint64, [S("i64"), S("u64"), COUNT], [(4096, 0x521, 0, 0)], start=1)
CASES["scatter-uint64-0x5-odd_first_row"] = _scatter(np.uint64, [COUNT], [(12288, 0x5, 0, 0)], start=1)
CASES["scatter-uint64-0x957-avg"] = _scatter(np.uint64, [("avg", "f64")], [(8192, 0x957, 1, 8192)])
# P = 1024 (a promise of 3.2 M groups): 12288-row tiles of 4-byte keys no longer fit next to the partition counters
CASES["scatter-uint32-P1024"] = _scatter(np.uint32, [S("i64"), COUNT], [(8192, 0x51, 1, 8192)], hint=3_200_000)
CASES["scatter-uint32-P1024-odd_first_row"] = _scatter(np.uint32, [S("i64"), COUNT], [(8192, 0x51, 0, 0)], hint=3_200_000, start=1)
# ---- ranged plan: key width x argument width x extension ----
for _kd in (np.uint8, np.uint16, np.uint32, np.uint64):
    for _a, _aw, _ext in (("u32", 4, 0), ("i32", 4, 1), ("u16", 2, 0), ("i16", 2, 1), ("u8", 1, 0), ("i8", 1, 1)):
        CASES[f"ranged-{np.dtype(_kd).name}-{_a}"] = _ranged(_kd, _a, _aw, _ext)
CASES["ranged-uint32-f32"] = _ranged(np.uint32, "f32", 4, 1)


def _fields(line):
    return dict(kv.split("=", 1) for kv in line.split() if "=" in kv)


@pytest.mark.parametrize("name", list(CASES))
def test_group_by_launch_arm(ch, capfd, name):
    c = CASES[name]
    kd, rows, groups, start = c["kd"], c["rows"], c["groups"], c["start"]
    ctx = ch.Context(0)
    try:
        for opt, value in c["opts"].items():
            ctx.set_option(opt, value)
        ctx.set_option("debug", 1)
        kinds = {"sum": ch.AGG_SUM, "avg": ch.AGG_AVG, "count": ch.AGG_COUNT}
        A = ch.Aggregator(kd, [(kinds[k], DTYPES[a] if a else None) for k, a in c["aggs"]], size_hint=c["hint"], ctx=ctx)
        cols = {a: ctx.upload(_arg(a, rows)) for _, a in c["aggs"] if a}
        kcol = ctx.upload(_keys(kd, rows, groups))
        capfd.readouterr()
        A.execute_on_block(kcol, [cols[a] if a else None for _, a in c["aggs"]], start, start + rows)
        gk, res = A.convert_to_block()
        err = capfd.readouterr().err
        del A, cols, kcol
    finally:
        ctx.close()
    # the arm: every plan line of the block is of this plan, and carries these fields
    lines = [ln for ln in err.splitlines() if ln.startswith("chgpu: ") and "GROUP BY" in ln and "finish rounds" not in ln]
    print(name, lines)
    assert len(lines) == len(c["lines"]) and all(c["plan"] in ln for ln in lines), err
    for ln, want in zip(lines, c["lines"]):
        got = _fields(ln)
        assert {f: got.get(f) for f in want} == want, ln
    # the groups
    uk, _, _, cnt = _grouping(kd, rows, groups, start)
    order = np.argsort(gk)
    assert np.array_equal(gk[order], uk)
    for (kind, a), r in zip(c["aggs"], res):
        r = r[order]
        if kind == "count":
            assert np.array_equal(r.view(np.uint64), cnt), (name, kind)
            continue
        ref = _ref_sum(kd, rows, groups, start, a)
        if kind == "avg":
            assert np.allclose(r, ref[0] / cnt, rtol=1e-6, atol=0), (name, kind, a)
        elif np.dtype(DTYPES[a]).kind != "f":
            assert np.array_equal(r.view(np.uint64), ref), (name, kind, a)
        elif c["opts"].get("deterministic_float_sums", 1):
            assert np.array_equal(r.view(np.uint64), ref[0].view(np.uint64)), (name, kind, a, np.abs(r - ref[0]).max())
        else:
            bound = cnt.astype(np.float64) * 2.0 ** -52 * ref[1]
            print(name, "max error / bound", (np.abs(r - ref[0]) / bound).max())
            assert np.all(np.abs(r - ref[0]) <= bound), (name, kind, a)
