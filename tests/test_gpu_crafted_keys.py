"""The hash-placed join and GROUP BY plans over key sets crafted to land where those plans give up: crowded slices, chains past the
staged window, tiles spanning three partitions, duplicate build keys, overfilled slice builds, LDS tables with one home cell.  Every
case compares with a numpy reference (integer counts and sums bit-exact mod 2^64, averages within 1e-6) and reads the `debug`
option's plan lines, so a plan that should answer -- or should decline and hand over -- is known to have done so.  Each fallback
runs again with the declined plan switched off: both answers must equal the reference."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keycraft as kc  # noqa: E402

pytestmark = pytest.mark.gpu

TOP = np.uint64(2**64 - 1)
VARIANTS = [("INNER", "ALL"), ("LEFT", "ALL"), ("LEFT", "SEMI"), ("LEFT", "ANTI")]
LOW_ROWS = {"tune_join_lds_min_rows": 1 << 20, "tune_join_region_min_rows": 1 << 20}   # the plans run; realistic sizes are not needed


@pytest.fixture(scope="module")
def ch():
    import clickhouse_amd
    return clickhouse_amd


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _lines(err, prefix):
    return [ln[len("chgpu: "):] for ln in err.splitlines() if ln.startswith("chgpu: " + prefix)]


def _fields(line):
    return dict(kv.split("=", 1) for kv in line.split() if "=" in kv)


def _plan(err, what):
    got = _lines(err, what + " plan=")
    assert len(got) == 1, err
    return _fields(got[0])


def _declined(err, what):
    got = _lines(err, what + " declined:")
    assert len(got) <= 1, err
    return got[0].split(":", 1)[1].split() if got else None


# ---- join ---------------------------------------------------------------------------------------------------------------------
def _unique_keys(rng, n, avoid=None):
    """n distinct keys, nonzero and below 2^64 - 1 (those two are added by the cases), none for which avoid(keys) is true"""
    k = np.empty(0, dtype=np.uint64)
    while k.shape[0] < n:
        more = rng.integers(1, 2**64 - 1, size=n - k.shape[0] + 1000, dtype=np.uint64)
        if avoid is not None:
            more = more[~avoid(more)]
        k = np.unique(np.concatenate([k, more]))
    return rng.permutation(k)[:n]


def _with_edges(k):
    return np.concatenate([k, np.array([0, 2**64 - 1], dtype=np.uint64)])


def _probe_mix(rng, bk, n, extra=None):
    """half hits, half random keys, the zero key and 2^64 - 1 a few times each"""
    parts = [bk[rng.integers(0, bk.shape[0], size=n // 2)], rng.integers(0, 2**64 - 1, size=n - n // 2 - 20, dtype=np.uint64, endpoint=True),
             np.zeros(10, dtype=np.uint64), np.full(10, TOP)]
    if extra is not None:
        parts.append(extra)
    return rng.permutation(np.concatenate(parts))


def _join_ref(bk, bv, pk, kind, strict):
    order = np.argsort(bk, kind="stable")
    sk = bk[order]
    uk, first, cnt = np.unique(sk, return_index=True, return_counts=True)
    sums = np.add.reduceat(bv[order].astype(np.uint64), first)                 # wraps modulo 2^64 like AggregateFunctionSum
    pos = np.searchsorted(uk, pk)
    pos[pos == uk.shape[0]] = 0
    hit = uk[pos] == pk
    s = int(sums[pos[hit]].sum(dtype=np.uint64))
    if strict == "ANTI":
        return int((~hit).sum()), 0
    if strict == "SEMI":
        assert cnt.max() == 1                                                    # (with duplicates, which row SEMI keeps is not checked here)
        return int(hit.sum()), s
    c = int(cnt[pos[hit]].sum()) + (int((~hit).sum()) if kind == "LEFT" else 0)
    return c, s


def _fused(ch, capfd, blocks, bv, pk, kind, strict, **opts):
    """chgpu_join_probe_agg on a context of its own with `opts` set -> (count, sum mod 2^64, stderr of the probe)"""
    ctx = ch.Context(0)
    try:
        for name, value in opts.items():
            ctx.set_option(name, value)
        ctx.set_option("debug", 1)
        j = ch.HashJoin({"INNER": ch.JOIN_INNER, "LEFT": ch.JOIN_LEFT}[kind],
                        {"ALL": ch.STRICT_ALL, "SEMI": ch.STRICT_SEMI, "ANTI": ch.STRICT_ANTI}[strict], ctx=ctx)
        for b in blocks:
            j.add_block(b)
        kcol, pcol = ctx.upload(pk), ctx.upload(bv)
        capfd.readouterr()
        c, s = j.probe_count_sum(kcol, pcol)
        err = capfd.readouterr().err
        del j, kcol, pcol
    finally:
        ctx.close()
    return c, s % 2**64, err


def _check_fused(ch, capfd, bk, bv, pk, variants, expect, blocks=None, **opts):
    """every variant: the answer equals numpy's and expect(err) holds; returns the stderr of the last run"""
    err = ""
    for kind, strict in variants:
        want = _join_ref(bk, bv, pk, kind, strict)
        c, s, err = _fused(ch, capfd, blocks or [bk], bv, pk, kind, strict, **opts)
        assert (c, s) == want, (kind, strict, err)
        expect(err)
    return err


def _expect(answered, declined=None, declined_what="join probe radix", lg_cap=None, regions=None):
    def check(err):
        p = _plan(err, "join probe")
        assert p["plan"] == answered, err
        if lg_cap is not None:
            assert int(p["cap"]) == 1 << lg_cap, err
        if regions is not None:
            assert int(p["regions"]) == regions, err
        if declined is not None:
            got = _declined(err, declined_what)
            assert got is not None and declined in got, err
    return check


NB = 1_200_000      # a one-block build side the radix join takes: 2^22 cells, 16 slices per first-level partition
LG = kc.join_lg_cap(NB + 2)
NP = 1_500_000


def _build(seed, nb=NB, avoid=None):
    rng = _rng(seed)
    bk = _with_edges(_unique_keys(rng, nb, avoid))
    bv = rng.integers(-2**62, 2**62, size=bk.shape[0], dtype=np.int64)
    return rng, bk, bv


def test_radix_join_answers_a_hot_probe_key(ch, capfd):
    """case 1: half the probe rows are one build key (the other half still fills every first-level partition beyond one probe tile:
    partitions smaller than a tile make tiles span three of them, and the radix join declines such a shape)"""
    rng, bk, bv = _build(11)
    n = 4_000_000
    pk = _probe_mix(rng, bk, n)
    pk[: n // 2] = bk[12345]
    assert LG == 22
    _check_fused(ch, capfd, bk, bv, rng.permutation(pk), VARIANTS, _expect("radix", lg_cap=LG), **LOW_ROWS)


def test_radix_join_answers_probe_keys_in_one_partition(ch, capfd):
    """case 1: every probe key in radix partition 0 -- the zero key's -- and 2^64 - 1 alone in its own, starting a tile of its own"""
    rng, bk, bv = _build(12)
    top_part = int(kc.partition_of_slot(kc.radix_slot(TOP, LG), LG))
    assert top_part > 1
    in0 = bk[kc.partition_of_slot(kc.radix_slot(bk, LG), LG) == 0]
    n0 = 6 * kc.PROBE_TILE                                                         # partition 0 fills whole tiles
    hits = in0[rng.integers(0, in0.shape[0], size=n0 // 2)]
    miss = kc.keys_in_partition(rng, n0 - hits.shape[0] - 16, LG, 0, "radix")
    pk = np.concatenate([rng.permutation(np.concatenate([hits, miss, np.zeros(16, dtype=np.uint64)])), np.full(100, TOP)])
    assert np.all(kc.partition_of_slot(kc.radix_slot(pk[:n0], LG), LG) == 0)
    opts = dict(LOW_ROWS, tune_join_lds_min_rows=n0)
    _check_fused(ch, capfd, bk, bv, pk, VARIANTS, _expect("radix"), **opts)


def test_radix_join_declines_a_crowded_slice_window(ch, capfd):
    """case 2: 4500 build keys in one radix slice overflow its 4096 + 256 cell window: stray, and the table plans answer"""
    rng, bk, bv = _build(13)
    crowd = kc.keys_in_slice(rng, 4500, LG, 100, "radix")
    bk = np.concatenate([bk, crowd])
    bv = np.concatenate([bv, rng.integers(-2**62, 2**62, size=crowd.shape[0], dtype=np.int64)])
    assert kc.join_lg_cap(bk.shape[0]) == LG
    pk = _probe_mix(rng, bk, NP, extra=crowd)
    # the table (with a prefilter at this size, which the LDS-staged probe does not take) is probed by regions; with the radix join off, the same
    _check_fused(ch, capfd, bk, bv, pk, VARIANTS, _expect("regions", "stray"), **LOW_ROWS)
    _check_fused(ch, capfd, bk, bv, pk, VARIANTS, _expect("regions", "shape"), tune_join_no_radix=1, **LOW_ROWS)


def test_radix_join_declines_one_duplicate_build_key_in_the_last_tile(ch, capfd):
    """case 3: one build key twice, placed in the last radix slice (the last tile of the sorted build rows): dup, and the table plans answer"""
    rng, bk, bv = _build(14)
    last_slice = (1 << (LG - kc.LG_SLICE_CELLS)) - 1
    dk = kc.keys_at_slice_end(rng, 1, LG, last_slice, last_cells=64, placement="radix")
    assert int(kc.partition_of_slot(kc.radix_slot(dk, LG), LG)[0]) == (1 << kc.LG_P1) - 1
    bk = np.concatenate([bk, dk, dk])
    bv = np.concatenate([bv, np.array([123456789, -987654321], dtype=np.int64)])
    pk = _probe_mix(rng, bk, NP, extra=np.repeat(dk, 1000))
    variants = [v for v in VARIANTS if v[1] != "SEMI"]
    _check_fused(ch, capfd, bk, bv, pk, variants, _expect("regions", "dup"), **LOW_ROWS)
    _check_fused(ch, capfd, bk, bv, pk, variants, _expect("regions", "shape"), tune_join_no_radix=1, **LOW_ROWS)


@pytest.mark.parametrize("nb,lg,plan", [(60_000, 18, "lds"), (6_000_000, 25, "lds"), (11_800_000, 26, "regions")])
def test_lds_probe_capacity_bounds(ch, capfd, nb, lg, plan):
    """case 4: the LDS-staged probe takes tables of 2^18 .. 2^25 cells; at 2^26 it declines and the region probe (R = 512) answers"""
    rng, bk, bv = _build(15 + lg, nb)
    assert kc.join_lg_cap(bk.shape[0]) == lg
    pk = _probe_mix(rng, bk, NP)
    opts = dict(LOW_ROWS, tune_join_no_radix=1, tune_join_no_prefilter=1)
    if plan == "lds":
        _check_fused(ch, capfd, bk, bv, pk, VARIANTS, _expect("lds", lg_cap=lg), **opts)
    else:
        _check_fused(ch, capfd, bk, bv, pk, VARIANTS, _expect("regions", "shape", "join probe lds", lg_cap=lg, regions=kc.MAX_REGIONS), **opts)
        _check_fused(ch, capfd, bk, bv, pk, VARIANTS[:1], _expect("regions", "shape", "join probe lds"), tune_join_no_lds_probe=1, **opts)


@pytest.mark.parametrize("nb,chain,plan", [(NB, 200, "lds"), (NB, 300, "regions"), (300_000, 200, "lds"), (300_000, 300, "one_pass")])
def test_lds_probe_chains_at_the_slice_end(ch, capfd, nb, chain, plan):
    """case 5: `chain` build keys homed on the last cell of a slice whose successor holds no key of its own: the chain ends inside the
    256 staged cells behind the slice (answered from LDS) or runs past them (stray; the region probe answers, or the one-pass probe
    for a table under 2^22 cells)"""
    lg = kc.join_lg_cap(nb + 2 + chain)
    s = 37
    near = lambda k: (kc.join_home(k, lg) >> np.uint64(kc.LG_SLICE_CELLS)) - np.uint64(s) <= np.uint64(1)  # homed in slice s or s + 1
    rng, bk, bv = _build(20 + chain + lg, nb, near)
    run = kc.keys_at_slice_end(rng, chain, lg, s)
    bk = np.concatenate([bk, run])
    bv = np.concatenate([bv, rng.integers(-2**62, 2**62, size=chain, dtype=np.int64)])
    assert kc.join_lg_cap(bk.shape[0]) == lg
    homes = kc.join_home(bk, lg)
    lo = s * kc.SLICE_CELLS
    occ = kc.linear_probe_cells(homes[(homes >= np.uint64(lo - 1024)) & (homes < np.uint64(lo + 3 * kc.SLICE_CELLS))], 1 << lg)
    end = lo + kc.SLICE_CELLS - 1 + chain                                        # the first empty cell behind the run
    assert occ[lo + kc.SLICE_CELLS - 1:end].all() and not occ[end]
    assert (end < lo + kc.SLICE_CELLS + kc.SLICE_TAIL) == (plan == "lds")
    misses = kc.keys_at_slice_end(rng, 500, lg, s)                               # absent keys that walk the whole run
    pk = _probe_mix(rng, bk, NP, extra=np.concatenate([np.repeat(run, 20), misses]))
    opts = dict(LOW_ROWS, tune_join_no_radix=1, tune_join_no_prefilter=1)
    if plan == "lds":
        _check_fused(ch, capfd, bk, bv, pk, VARIANTS, _expect("lds", lg_cap=lg), **opts)
    else:
        _check_fused(ch, capfd, bk, bv, pk, VARIANTS, _expect(plan, "stray", "join probe lds", lg_cap=lg), **opts)
        _check_fused(ch, capfd, bk, bv, pk, VARIANTS, _expect(plan, "shape", "join probe lds"), tune_join_no_lds_probe=1, **opts)


@pytest.mark.parametrize("placement", ["radix", "hash"])
def test_probe_keys_in_partitions_p_and_p_plus_2(ch, capfd, placement):
    """case 6: 1000 probe keys in first-level partition 10, the rest in 12, none in 11: the first tile spans three partitions (stray);
    radix join (placement 'radix') or LDS-staged probe ('hash') declines, and the table plans answer"""
    rng, bk, bv = _build(30)
    slot = (lambda k: kc.radix_slot(k, LG)) if placement == "radix" else (lambda k: kc.join_home(k, LG))
    part = kc.partition_of_slot(slot(bk), LG)
    hits10, hits12 = bk[part == 10], bk[part == 12]
    pk = kc.keys_in_partitions(rng, {10: 500, 12: NP // 2}, LG, placement)
    pk = np.concatenate([pk, hits10[:500], hits12[rng.integers(0, hits12.shape[0], size=NP // 2)], np.zeros(5, dtype=np.uint64), np.full(5, TOP)])
    pk = rng.permutation(pk)
    if placement == "radix":
        _check_fused(ch, capfd, bk, bv, pk, VARIANTS, _expect("regions", "stray"), **LOW_ROWS)
        _check_fused(ch, capfd, bk, bv, pk, VARIANTS, _expect("regions", "shape"), tune_join_no_radix=1, **LOW_ROWS)
    else:
        opts = dict(LOW_ROWS, tune_join_no_radix=1, tune_join_no_prefilter=1)
        _check_fused(ch, capfd, bk, bv, pk, VARIANTS, _expect("regions", "stray", "join probe lds"), **opts)
        _check_fused(ch, capfd, bk, bv, pk, VARIANTS, _expect("regions", "shape", "join probe lds"), tune_join_no_lds_probe=1, **opts)


@pytest.mark.parametrize("region_kib,regions", [(1024, 64), (64, kc.MAX_REGIONS)])
def test_region_probe_with_every_probe_key_in_one_region(ch, capfd, region_kib, regions):
    """case 7: all probe keys (but the zero key and 2^64 - 1) in one table region; R = 64, and R = JPR_MAX_REGIONS"""
    rng, bk, bv = _build(40 + regions)
    assert kc.region_count(LG, region_kib) == regions
    lg_r = regions.bit_length() - 1
    reg = kc.partition_of_slot(kc.join_home(bk, LG), LG, lg_r)
    inr = bk[reg == 3]
    pk = np.concatenate([inr[rng.integers(0, inr.shape[0], size=NP // 2)], kc.keys_in_region(rng, NP // 2, LG, 3, regions),
                         np.zeros(7, dtype=np.uint64), np.full(7, TOP)])
    pk = rng.permutation(pk)
    opts = dict(LOW_ROWS, tune_join_no_radix=1, tune_join_no_lds_probe=1, tune_join_region_kib=region_kib)
    _check_fused(ch, capfd, bk, bv, pk, VARIANTS, _expect("regions", lg_cap=LG, regions=regions), **opts)
    _check_fused(ch, capfd, bk, bv, pk, VARIANTS[:2], _expect("one_pass", "shape", "join probe regions"), tune_join_no_regions=1, **opts)


# ---- the slice build, through the ordered joinBlock -------------------------------------------------------------------------
def _probe_columns(ch, capfd, bk, left, **opts):
    ctx = ch.Context(0)
    try:
        for name, value in opts.items():
            ctx.set_option(name, value)
        ctx.set_option("debug", 1)
        j = ch.HashJoin(ch.JOIN_INNER, ch.STRICT_ALL, ctx=ctx)
        j.add_block(bk)
        capfd.readouterr()
        r = j.probe_columns(left)
        err = capfd.readouterr().err
        out = (r["consumed"], r["n_out"], r["offsets"].numpy().astype(np.int64), r["right_rowid"].numpy(), j.n_keys)
        del j, r
    finally:
        ctx.close()
    return out, err


def _check_probe_columns(bk, left, out):
    consumed, n_out, off, rid, n_keys = out
    assert consumed == left.shape[0]
    counts = np.diff(np.concatenate([[0], off]))
    order = np.argsort(bk, kind="stable")
    lo = np.searchsorted(bk[order], left, side="left")
    hi = np.searchsorted(bk[order], left, side="right")
    assert np.array_equal(counts, hi - lo)
    assert n_out == int((hi - lo).sum())
    rows = (rid & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert np.all((rid >> np.uint64(32)) == 0) and np.array_equal(bk[rows], np.repeat(left, counts))
    assert n_keys == np.unique(bk).shape[0]


def _slice_build_case(ch, capfd, bk, left, expect_slices):
    out, err = _probe_columns(ch, capfd, bk, left)
    _check_probe_columns(bk, left, out)
    p = _plan(err, "join build")
    if expect_slices:
        assert p["plan"] == "slices" and int(p["overflow"]) > 0, err
    else:
        assert p["plan"] == "generic" and _declined(err, "join build slices") == ["overflow_list_full"], err
    out2, err2 = _probe_columns(ch, capfd, bk, left, tune_join_no_slice_build=1)
    assert _plan(err2, "join build")["plan"] == "generic", err2
    _check_probe_columns(bk, left, out2)
    assert out2[1] == out[1] and np.array_equal(out2[2], out[2]) and np.array_equal(out2[3], out[3])


def _left_of(rng, bk, extra):
    return rng.permutation(np.concatenate([bk[rng.integers(0, bk.shape[0], size=300_000)], rng.integers(0, 2**64 - 1, size=300_000, dtype=np.uint64, endpoint=True),
                                           extra, np.zeros(3, dtype=np.uint64), np.full(3, TOP)]))


def test_slice_build_overflow_list_answers(ch, capfd):
    """case 8: 6000 extra keys homed in one 4096-cell slice: the rows that do not fit go through the overflow list, the slice build answers"""
    rng, bk, _ = _build(50)
    crowd = kc.keys_in_slice(rng, 6000, LG, 200)
    bk = rng.permutation(np.concatenate([bk, crowd]))
    assert kc.join_lg_cap(bk.shape[0]) == LG
    _slice_build_case(ch, capfd, bk, _left_of(rng, bk, crowd), True)


def test_slice_build_overflow_list_full_falls_back(ch, capfd):
    """case 9: 280 slices with 8096 keys each (spread over every first-level partition; the two slices behind each take the spill and
    hold no key of their own) send more than JBS_MAX_OVERFLOW rows to the overflow list: overflow_list_full -- and nothing else, every
    partition is longer than a build tile -- and the generic build answers"""
    rng = _rng(60)
    nb = 2_500_000
    lg = kc.join_lg_cap(nb)
    assert lg == 23
    n_slices = 1 << (lg - kc.LG_SLICE_CELLS)
    groups, per = 280, 2 * kc.SLICE_CELLS - 96
    assert groups * (per - kc.SLICE_CELLS) > kc.MAX_OVERFLOW
    base = np.arange(groups, dtype=np.uint64) * np.uint64(n_slices) // np.uint64(groups)
    slots = np.concatenate([np.uint64(b * kc.SLICE_CELLS) + rng.integers(0, kc.SLICE_CELLS, size=per, dtype=np.uint64) for b in base.tolist()])
    crowd = kc.keys_at_slots(rng, slots, lg)
    taken = np.concatenate([base, base + np.uint64(1), base + np.uint64(2)])
    rest = _unique_keys(rng, nb - 2 - crowd.shape[0], lambda k: np.isin(kc.join_home(k, lg) >> np.uint64(kc.LG_SLICE_CELLS), taken))
    bk = rng.permutation(_with_edges(np.unique(np.concatenate([crowd, rest]))))
    assert bk.shape[0] == nb and kc.join_lg_cap(bk.shape[0]) == lg
    assert np.bincount(kc.partition_of_slot(kc.join_home(bk, lg), lg).astype(np.int64), minlength=1 << kc.LG_P1).min() > kc.BUILD_TILE
    _slice_build_case(ch, capfd, bk, _left_of(rng, bk, crowd[:1000]), False)


# ---- GROUP BY -----------------------------------------------------------------------------------------------------------------
def _gb_ref(keys, v, f):
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    starts = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))
    cnt = np.diff(np.concatenate([starts, [keys.shape[0]]])).astype(np.uint64)
    vs = v[order]
    return dict(keys=sk[starts], count=cnt, sum=np.add.reduceat(vs.astype(np.uint64), starts), min=np.minimum.reduceat(vs, starts),
                max=np.maximum.reduceat(vs, starts), avg=np.add.reduceat(f[order], starts) / cnt)


AGG_SETS = {"count_sum": ["count", "sum"], "avg": ["avg"], "min_max": ["min", "max"]}


def _group_by(ch, capfd, keys, v, f, aggs, hint, pack=None, **opts):
    ctx = ch.Context(0)
    try:
        for name, value in opts.items():
            ctx.set_option(name, value)
        ctx.set_option("debug", 1)
        kinds = {"count": (ch.AGG_COUNT, None), "sum": (ch.AGG_SUM, np.int64), "avg": (ch.AGG_AVG, np.float64), "min": (ch.AGG_MIN, np.int64),
                 "max": (ch.AGG_MAX, np.int64)}
        A = ch.Aggregator(np.uint64 if pack is not None else keys.dtype, [kinds[a] for a in aggs], size_hint=hint, ctx=ctx)
        if pack is not None:
            kcol = ch.pack_fixed_keys([ctx.upload(pack[0]), ctx.upload(pack[1])])
        else:
            kcol = ctx.upload(keys)
        vcol, fcol = ctx.upload(v), ctx.upload(f)
        capfd.readouterr()
        A.execute_on_block(kcol, [None if a == "count" else (fcol if a == "avg" else vcol) for a in aggs])
        gk, res = A.convert_to_block()
        err = capfd.readouterr().err
        del A, kcol, vcol, fcol
    finally:
        ctx.close()
    return gk, res, err


def _check_gb(ref, gk, res, aggs):
    order = np.argsort(gk)
    assert np.array_equal(gk[order].astype(np.uint64), ref["keys"].astype(np.uint64))
    for a, r in zip(aggs, res):
        r = r[order]
        if a == "avg":
            assert np.allclose(r, ref["avg"], rtol=1e-6, atol=0)
        elif a in ("count", "sum"):
            assert np.array_equal(r.view(np.uint64), ref[a].astype(np.uint64)), a
        else:
            assert np.array_equal(r, ref[a]), a


def _gb_plan(err):
    if _lines(err, "tile-sorted GROUP BY"):
        return "tiled"
    if _lines(err, "partitioned GROUP BY"):
        return "partitioned"
    if _lines(err, "ranged GROUP BY"):
        return "ranged"
    if _lines(err, "direct GROUP BY"):
        return "direct"
    return None


def _rounds(err):
    return [int(_fields(ln)["rounds"]) for ln in _lines(err, "GROUP BY finish rounds=")]


def _run_gb(ch, capfd, keys, v, f, hint, plan, ref, pack=None, aggs_sets=("count_sum",), **opts):
    errs = []
    for name in aggs_sets:
        aggs = AGG_SETS[name]
        gk, res, err = _group_by(ch, capfd, keys, v, f, aggs, hint, pack, **opts)
        _check_gb(ref, gk, res, aggs)
        assert _gb_plan(err) == (plan if name != "min_max" else "direct"), err
        assert _rounds(err), err
        errs.append(err)
    return errs


def _args(rng, n):
    return rng.integers(-2**62, 2**62, size=n, dtype=np.int64), rng.random(n) * 1000.0


@pytest.mark.parametrize("plan", ["tiled", "partitioned", "ranged"])
def test_group_by_packed_uint32_pair_with_a_low_cardinality_first_column(ch, capfd, plan):
    """case 10: GROUP BY a, b over two UInt32 columns, a of four values: packed, a sits in the low half, and bits 20..32 of
    key * GBP_MULT -- the LDS home cell -- see only a and b's lowest bit.  Eight home cells for ~3 M groups: nearly every row gives up
    after 64 probes.  The tile-sorted plan leaves them pending for the finish rounds; the partitioned and RANGE plans send them to the
    HBM table, whose growth the finish rounds then do (RANGE, no size hint: the table starts at its minimum).  The tile-sorted and
    partitioned plans get ~1.2 M groups (one level, P = 512), RANGE ~3 M (beyond the minimum table's max fill)."""
    rng = _rng(70)
    n = 6_000_000
    a = rng.integers(0, 4, size=n).astype(np.uint32)
    a[:1000] = 2**32 - 1
    b = rng.integers(0, 1_000_000 if plan == "ranged" else 300_000, size=n).astype(np.uint32)
    b[:1000] = 2**32 - 1
    a[1000:1010] = 0
    b[1000:1010] = 0                                                              # the zero key
    keys = a.astype(np.uint64) | (b.astype(np.uint64) << np.uint64(32))
    v, f = _args(rng, n)
    ref = _gb_ref(keys, v, f)
    groups = ref["keys"].shape[0]
    assert (groups > 2**21) == (plan == "ranged")                                 # more than the minimum table's max fill
    hint = 0 if plan == "ranged" else groups
    opts = {"tune_gb_no_tiled": 1} if plan == "partitioned" else {}
    sets = ("count_sum", "avg", "min_max") if plan == "tiled" else ("count_sum",)
    errs = _run_gb(ch, capfd, keys, v, f, hint, plan, ref, pack=(a, b), aggs_sets=sets, **opts)
    if plan in ("tiled", "ranged"):
        assert max(_rounds(errs[0])) >= 1, errs[0]
    if plan != "partitioned":
        return
    _run_gb(ch, capfd, keys, v, f, hint, "direct", ref, pack=(a, b), agg_no_partition=1)   # no partitioning at all: the DIRECT kernel


@pytest.mark.parametrize("plan", ["tiled", "partitioned"])
def test_group_by_64bit_keys_on_one_partition(ch, capfd, plan):
    """case 11: ~1 M distinct 64-bit keys with one GBP_MULT partition for every P: far more than one partition's LDS table"""
    rng = _rng(80)
    uk = np.concatenate([kc.gb_keys64_top(rng, 1_000_000, 12, 0x9A5), np.array([0, 2**64 - 1], dtype=np.uint64)])
    n = 5_000_000
    keys = uk[rng.integers(0, uk.shape[0], size=n)]
    keys[:uk.shape[0]] = uk
    v, f = _args(rng, n)
    ref = _gb_ref(keys, v, f)
    opts = {"tune_gb_no_tiled": 1} if plan == "partitioned" else {}
    errs = _run_gb(ch, capfd, keys, v, f, ref["keys"].shape[0], plan, ref, aggs_sets=("count_sum", "avg") if plan == "tiled" else ("count_sum",), **opts)
    p = _fields(_lines(errs[0], "tile-sorted GROUP BY" if plan == "tiled" else "partitioned GROUP BY")[0])
    assert np.unique(kc.gbp_part64(uk[:-2], int(p["P"]))).shape[0] == 1
    if plan == "tiled":
        assert max(_rounds(errs[0])) >= 1, errs[0]
        _run_gb(ch, capfd, keys, v, f, 0, "ranged", ref)                         # no size hint, fewer than 8 Mi rows: RANGE mode


def test_group_by_two_level_with_one_first_level_partition(ch, capfd):
    """case 11: 7 M distinct keys on one GBP_MULT1 partition: the two-level plan's first level puts every row in one big partition"""
    rng = _rng(81)
    uk = np.concatenate([kc.gb_keys64_top(rng, 7_000_000, 12, 0x123, kc.GBP_MULT1), np.array([0, 2**64 - 1], dtype=np.uint64)])
    n = 9_000_000
    keys = np.concatenate([uk, uk[rng.integers(0, uk.shape[0], size=n - uk.shape[0])]])
    v, f = _args(rng, n)
    ref = _gb_ref(keys, v, f)
    errs = _run_gb(ch, capfd, keys, v, f, ref["keys"].shape[0], "partitioned", ref)
    lv = [_fields(ln) for ln in _lines(errs[0], "partitioned GROUP BY")]
    assert [d["level"] for d in lv][0] == "1", errs[0]
    big = [d for d in lv if d["level"] == "2" and int(d["n"]) >= n - 100]
    assert len(big) == 1, errs[0]


@pytest.mark.parametrize("plan", ["tiled", "partitioned", "ranged"])
def test_group_by_uint32_keys_on_one_partition_and_one_cell(ch, capfd, plan):
    """case 12: UInt32 keys through the 32-bit multiplier: 256 keys on one partition and one LDS cell (top 24 product bits fixed) and,
    for the partitioned plans, 300 k more on that partition (top 10 bits)"""
    rng = _rng(90)
    cell = kc.gb_keys32_top(rng, 256, 24, 0x5A5A5A)
    if plan == "ranged":
        uk = np.concatenate([cell, np.array([0, 2**32 - 1], dtype=np.uint32)])
        n = 2_000_000
    else:
        part = kc.gb_keys32_top(rng, 300_000, 10, 0x5A5A5A >> 14)
        uk = np.unique(np.concatenate([cell, part, np.array([0, 2**32 - 1], dtype=np.uint32)]))
        n = 4_500_000
    keys = np.concatenate([uk, uk[rng.integers(0, uk.shape[0], size=n - uk.shape[0])]])
    v, f = _args(rng, n)
    ref = _gb_ref(keys, v, f)
    opts = {"tune_gb_no_tiled": 1} if plan == "partitioned" else {}
    hints = (ref["keys"].shape[0], 0) if plan == "ranged" else (ref["keys"].shape[0],)
    for hint in hints:
        _run_gb(ch, capfd, keys, v, f, hint, plan, ref, aggs_sets=("count_sum", "min_max"), **opts)
    if plan == "tiled":
        _run_gb(ch, capfd, keys, v, f, ref["keys"].shape[0], "partitioned", ref, tune_gb_no_tiled=1)
