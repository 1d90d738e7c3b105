"""tests/chain_cases.py checked without a device: its constants against join_chain.h, its numpy reference against oracle.HashJoin run join
by join, and every generator against what it promises (slice counts, alive rows per unit and quarter)."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_cases as cc  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "clickhouse_amd", "csrc", "join_chain.h")


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _header():
    with open(HEADER) as f:
        return f.read()


def _const(text, name):
    m = re.search(r"static constexpr u32 (?:\w+ = [^;,]+, )*?" + name + r" = ([^;,]+)[;,]", text)
    assert m, name
    expr = re.sub(r"(\d+)u\b", r"\1", m.group(1))
    names = {n: _const(text, n) for n in re.findall(r"\b(JCT?_[A-Z_]+)\b", expr)}
    return int(eval(expr.replace("/", "//"), {"__builtins__": {}}, names))


def test_constants_match_the_header():
    text = _header()
    for name in ["JC_MAX_STEPS", "JC_MAX_CARRY", "JC_SLICE_BYTES", "JC_SLICE_BITS", "JC_MAX_SLICES", "JC_QPT", "JC_THREADS", "JCT_QUEUE", "JCT_COAL_MIN", "JCT_WAVES"]:
        assert _const(text, name) == getattr(cc, name), name
    assert _const(text, "JC_PART_ROWS") == cc.PART_ROWS
    assert _const(text, "JC_UNIT_ROWS") == cc.UNIT_ROWS
    assert _const(text, "JC_UNITS_PER_PART") == cc.UNITS_PER_PART
    # the row threshold of the LDS sweep and the key-set limit are literals (the threshold sits in the gate the chain shares with the
    # filter-only probe, beside the join's kernels)
    with open(os.path.join(os.path.dirname(HEADER), "join_kernels.hip")) as f:
        gate = re.search(r"static bool join_lds_filter_fits\(.*?\n}\n", f.read(), re.S).group(0)
    assert "join_lds_filter_fits(" in text and "JC_SLICE_BITS, JC_MAX_SLICES)" in text
    assert re.search(r"n >= \(1u << (\d+)\)", gate).group(1) == str(cc.LDS_MIN_ROWS.bit_length() - 1)
    assert re.search(r"r\[0\] >= \(1ull << (\d+)\)", text).group(1) == str(cc.KEYSET_LIMIT.bit_length() - 1)
    # the grid caps the many-turn case derives its row count from, and the row mapping of the alive words
    assert "(u64)ctx->num_cus * 4" in text and "(u64)ctx->num_cus * 8" in text and "(u64)ctx->num_cus)" in text
    assert "((bit >> 2) * 64 + lane) * 4 + (bit & 3)" in text and "(((b >> 2) * 64 + lane) * 4 + (b & 3))" in text


def test_geometry():
    assert cc.PART_ROWS == 65536 and cc.UNIT_ROWS == 4096 and cc.QUARTER_ROWS == 1024
    assert cc.dense_bits(0) == 32 and cc.dense_bits(31) == 32 and cc.dense_bits(32) == 64
    assert cc.n_slices(cc.JC_SLICE_BITS - 32) == 1 and cc.n_slices(cc.JC_SLICE_BITS - 1) == 1 and cc.n_slices(cc.JC_SLICE_BITS) == 2
    assert cc.slice_ranges(cc.JC_SLICE_BITS) == [(0, cc.JC_SLICE_BITS), (cc.JC_SLICE_BITS, 32)]          # a last slice of one word
    assert cc.fits_lds(cc.LDS_MAX_KEY) and not cc.fits_lds(cc.LDS_MAX_KEY + 1) and cc.n_slices(cc.LDS_MAX_KEY) == 4
    assert cc.LDS_MAX_KEY < cc.KEYSET_LIMIT
    rows = cc.unit_row(np.arange(64)[:, None], np.arange(64)[None, :])
    assert sorted(rows.ravel().tolist()) == list(range(cc.UNIT_ROWS))                                      # a bijection lanes x bits -> rows
    lane, bit = cc.unit_lane_bit(rows)
    assert np.array_equal(lane, np.broadcast_to(np.arange(64)[:, None], rows.shape)) and np.array_equal(bit, np.broadcast_to(np.arange(64)[None, :], rows.shape))
    for q in range(4):
        assert np.array_equal(cc.quarter_rows(q), np.arange(q * 1024, q * 1024 + 1024))                    # a queue pass takes 1024 consecutive rows
    assert cc.locate(3 * cc.PART_ROWS + 5 * cc.UNIT_ROWS + 1029) == dict(row=3 * 65536 + 5 * 4096 + 1029, part=3, unit=53, wave=5, lane=1, bit=17, quarter=1)


# ---- the reference against the oracle -------------------------------------------------------------------------------------------
def oracle_chain(O, steps):
    """oracle.HashJoin join by join: the AND of the filters; per step the rows joinBlock adds for the survivors"""
    n = steps[0].probe.shape[0]
    flt = np.ones(n, dtype=bool)
    joins = []
    for st in steps:
        j = O.HashJoin(st.kind, st.strictness)
        for keys, nm, jm in st.build:
            j.add_block(cc.canon(np.asarray(keys, dtype=st.dtype)).astype(np.uint64), nm, jm)
        joins.append(j)
        r = j.probe(cc.canon(st.probe).astype(np.uint64), st.null_map)
        if r["filter"] is not None:
            flt &= r["filter"].astype(bool)
        elif r["offsets"] is not None:
            f = np.diff(np.concatenate([[0], r["offsets"].astype(np.int64)])) > 0
            assert st.filters or f.all()
            flt &= f
    idx = np.flatnonzero(flt)
    rowids = []
    for st, j in zip(steps, joins):
        o = j.probe(cc.canon(st.probe).astype(np.uint64)[idx], st.null_map[idx] if st.null_map is not None else None)
        assert o["added_row"].shape[0] == idx.shape[0]
        rowids.append(np.where(o["added_row"] < 0, cc.NO_ROW, (o["added_block"].astype(np.uint64) << np.uint64(32)) | o["added_row"].astype(np.uint64)))
    return flt, idx, rowids


def assert_reference_equals_oracle(O, steps):
    ref = cc.chain_reference(steps)
    flt, idx, rowids = oracle_chain(O, steps)
    assert np.array_equal(ref["filter"], flt)
    assert ref["kept"] == idx.shape[0] and np.array_equal(ref["indexes"], idx.astype(np.uint64))
    for s, (a, b) in enumerate(zip(ref["rowids"], rowids)):
        assert np.array_equal(a, b), s


DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]
FORMS = [(cc.JOIN_LEFT, cc.STRICT_SEMI, True), (cc.JOIN_LEFT, cc.STRICT_ANTI, True), (cc.JOIN_INNER, cc.STRICT_ALL, False),
         (cc.JOIN_LEFT, cc.STRICT_ANY, True), (cc.JOIN_LEFT, cc.STRICT_ALL, False)]          # (kind, strictness, duplicates allowed)


def _random_step(rng, n, dt, form):
    kind, strictness, dups_ok = form
    info = np.iinfo(dt)
    span = min(int(info.max), 300)
    low = max(int(info.min), -span)
    domain = np.arange(low, span + 1).astype(dt)
    blocks = []
    pool = rng.permutation(domain)
    at = 0
    for _ in range(int(rng.integers(0, 4))):
        rows = int(rng.integers(0, 60))
        keys = pool[at:at + rows]
        at += rows
        if dups_ok and keys.shape[0] > 4:
            keys = np.concatenate([keys, keys[:3], blocks[0][0][:2] if blocks else keys[:1]])
        nm = (rng.random(keys.shape[0]) < 0.2).astype(np.uint8) if rng.random() < 0.5 else None
        jm = (rng.random(keys.shape[0]) < 0.8).astype(np.uint8) if rng.random() < 0.5 else None
        blocks.append((keys, nm, jm))
    probe = rng.choice(domain, size=n)
    nm = (rng.random(n) < 0.1).astype(np.uint8) if rng.random() < 0.5 else None
    return cc.Step(kind, strictness, blocks, probe, nm)


@pytest.mark.parametrize("seed", range(12))
def test_reference_equals_the_oracle_on_small_chains(oracle_mod, seed):
    rng = _rng(seed)
    n = int(rng.integers(0, 700))
    steps = [_random_step(rng, n, DTYPES[int(rng.integers(0, len(DTYPES)))], FORMS[int(rng.integers(0, len(FORMS)))]) for _ in range(int(rng.integers(1, 6)))]
    assert_reference_equals_oracle(oracle_mod, steps)


def test_reference_treats_the_edges_like_the_oracle(oracle_mod):
    # negative keys match themselves only; a masked-out build row does not count; duplicates: the first valid row; empty build sides
    i32 = np.array([-1, -2**31, 5, 0, 7, 2**31 - 1], dtype=np.int32)
    st = [cc.Step(cc.JOIN_LEFT, cc.STRICT_SEMI, [np.array([-1, 5, 5, 0, -2**31], dtype=np.int32)], i32),
          cc.Step(cc.JOIN_LEFT, cc.STRICT_ANY, [(np.array([7, 7, 5], dtype=np.int32), np.array([1, 0, 0], dtype=np.uint8), None),
                                                (np.array([7, 0], dtype=np.int32), None, np.array([1, 0], dtype=np.uint8))], i32)]
    ref = cc.chain_reference(st)
    assert ref["filter"].tolist() == [True, True, True, True, False, False]
    assert ref["rowids"][0].tolist() == [0, 4, 1, 3] and ref["rowids"][1].tolist() == [int(cc.NO_ROW), int(cc.NO_ROW), 2, int(cc.NO_ROW)]
    assert cc.build_stats(st[1]) == (7, False) and cc.build_stats(st[0]) == (0xFFFFFFFF, True)
    assert_reference_equals_oracle(oracle_mod, st)
    for form in FORMS[:3]:
        for build in ([], [np.zeros(0, dtype=np.uint32)]):
            assert_reference_equals_oracle(oracle_mod, [cc.Step(form[0], form[1], build, np.arange(9, dtype=np.uint32))])


# ---- the generators -------------------------------------------------------------------------------------------------------------
EDGE_MAX_KEYS = [1, 31, 32, cc.JC_SLICE_BITS - 33, cc.JC_SLICE_BITS - 32, cc.JC_SLICE_BITS - 1, cc.JC_SLICE_BITS, 256 * 32 * 8 - 1, 2 * cc.JC_SLICE_BITS - 1,
                 3 * cc.JC_SLICE_BITS + 12345, cc.LDS_MAX_KEY, cc.LDS_MAX_KEY + 1, cc.KEYSET_LIMIT - 1, cc.KEYSET_LIMIT]


@pytest.mark.parametrize("max_key", EDGE_MAX_KEYS)
@pytest.mark.parametrize("with_zero", [False, True])
def test_build_sides_have_the_promised_geometry(oracle_mod, max_key, with_zero):
    rng = _rng(max_key + with_zero)
    bk = cc.alternating_edge_build(rng, max_key, min(3000, max_key), with_zero).astype(np.uint32)
    assert np.unique(bk).shape[0] == bk.shape[0]
    edges = cc.slice_edge_keys(max_key)
    inner = [int(k) for k in edges if 0 < k < max_key]
    assert np.isin(np.array(inner[0::2], dtype=np.uint32), bk).all() and not np.isin(np.array(inner[1::2], dtype=np.uint32), bk).any()
    probe = cc.probe_mix(rng, 5000, bk, 0.5, min(2 * max_key + 64, 0xFFFFFFFF))
    rows = cc.plant(rng, probe, edges, copies=2)
    assert set(probe[rows].tolist()) == set(edges.tolist())
    st = cc.Step(cc.JOIN_LEFT, cc.STRICT_SEMI, [bk], probe)
    assert cc.build_stats(st) == (max_key, with_zero)
    for lo, nb in cc.slice_ranges(max_key):
        for k in (lo - 1, lo, lo + nb - 1, lo + nb):
            assert k < 0 or k in edges
    assert sum(nb for _, nb in cc.slice_ranges(max_key)) == cc.dense_bits(max_key) > max_key
    found = cc.step_found(st)
    assert np.array_equal(found, np.isin(probe, bk))
    assert found[rows].any() and not found[rows].all()
    for anti in (cc.STRICT_SEMI, cc.STRICT_ANTI):
        assert_reference_equals_oracle(oracle_mod, [cc.Step(cc.JOIN_LEFT, anti, [bk], probe)])


def test_slice_counts_of_the_edge_key_sets():
    want = {1: 1, cc.JC_SLICE_BITS - 33: 1, cc.JC_SLICE_BITS - 32: 1, cc.JC_SLICE_BITS - 1: 1, cc.JC_SLICE_BITS: 2, 2 * cc.JC_SLICE_BITS - 1: 2,
            3 * cc.JC_SLICE_BITS + 12345: 4, cc.LDS_MAX_KEY: 4, cc.LDS_MAX_KEY + 1: 5}
    for mk, s in want.items():
        assert cc.n_slices(mk) == s, mk
    assert cc.slice_ranges(256 * 32 * 8 - 1)[0][1] // 32 % 256 == 0           # a slice whose word count is a multiple of 256
    assert cc.slice_ranges(cc.LDS_MAX_KEY)[-1] == (3 * cc.JC_SLICE_BITS, cc.JC_SLICE_BITS)


@pytest.mark.parametrize("plan", [
    {0: 0, 1: 1, 2: 95, 3: 96, 4: 1024, 5: 1025, 6: 4096, 7: 97},
    {2: (1024, 0, 0, 0), 3: (0, 0, 0, 1024), 5: (1024, 1, 0, 0), 9: (0, 1024, 1024, 0), 10: (256, 256, 256, 256), 11: (257, 256, 256, 256), 15: (24, 24, 24, 23)},
])
def test_unit_alive_column_places_the_promised_counts(plan):
    rng = _rng(5)
    n = 16 * cc.UNIT_ROWS + 777
    col = cc.unit_alive_column(rng, n, hit_key=11, miss_key=12, plan=plan)
    st = cc.Step(cc.JOIN_LEFT, cc.STRICT_SEMI, [np.array([11, 3], dtype=np.uint32)], col)
    got = cc.alive_per_unit_quarter(cc.chain_reference([st])["filter"])
    assert got.shape == (17, 4)
    for unit, want in plan.items():
        if np.isscalar(want):
            assert got[unit].sum() == want, unit
        else:
            assert tuple(got[unit]) == tuple(want), unit
    others = [u for u in range(16) if u not in plan]
    assert all(1500 < got[u].sum() < 2600 for u in others)
    # the same through the lane words of k_chain_lds: bit 4 * kb + b of lane l = row (kb * 64 + l) * 4 + b
    alive = cc.chain_reference([st])["filter"]
    for unit, want in plan.items():
        u = alive[unit * cc.UNIT_ROWS:(unit + 1) * cc.UNIT_ROWS]
        words = u[cc.unit_row(np.arange(64)[:, None], np.arange(64)[None, :])]          # [lane, bit]
        per_quarter = [int(words[:, 16 * q:16 * q + 16].sum()) for q in range(4)]
        assert per_quarter == got[unit].tolist()


def test_per_part_rates_differ_between_parts_a_grid_apart():
    n = 600 * cc.PART_ROWS + 5
    r = cc.per_part_rates(n)
    per_part = r[::cc.PART_ROWS]
    for grid in (1, 2, 8, 104, 256, 304):
        assert (np.abs(per_part[grid:] - per_part[:-grid]) > 1e-3).mean() > 0.99, grid
    assert r.shape[0] == n and 0.1 < r.min() and r.max() < 1.0
    assert np.array_equal(cc.kept_per_part(np.ones(n, dtype=bool)), np.array([cc.PART_ROWS] * 600 + [5]))
