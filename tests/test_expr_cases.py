"""CPU only: the cases of the expression compiler's matrix (tests/expr_cases.py) are complete and well formed, and the scalar
reference -- Python integers, IEEE Float64 and exact rationals, one function per family -- agrees with the numpy oracle
(oracle/expr_dag.py) for every accepted (function, operand types) combination over the full cross product of the adversarial values.
The two share no structure: the first check of the oracle's arithmetic, casts, if and logic that does not restate them the same way."""
import numpy as np
import pytest

import expr_cases as XC
from oracle import expr_dag as OE


def test_value_sets_hold_the_values_the_conversions_turn_on():
    for t in XC.TAGS:
        assert len(XC.VALUES[t]) <= 48 and len(XC.VALUES[t]) >= 8
        assert XC.column(t).tolist() == XC.VALUES[t] or XC.is_float(t)  # every integer fits its type
    big = (1 << 60) + (1 << 36) + 1
    assert big in XC.VALUES[XC.I64] and -big in XC.VALUES[XC.I64] and big in XC.VALUES[XC.U64]
    # integer -> Float32 in one rounding against two: 2^60 + 2^37 against 2^60
    assert XC.convert(big, XC.I64, XC.F32) == float(2**60 + 2**37) and XC.round_f32(XC.Fraction(float(big))) == float(2**60)
    f32 = XC.VALUES[XC.F32]
    assert any(0 < x < 2.0**-126 for x in f32) and 2.0**-149 in f32  # Float32 subnormals: 1e-40 and the rounding of 1e-45
    assert XC.convert(1e-45, XC.F64, XC.F32) == 2.0**-149 and XC.convert(3.5e38, XC.F64, XC.F32) == float("inf")
    assert XC.convert(3.4028235e38, XC.F64, XC.F32) == float(np.finfo(np.float32).max)
    assert str(XC.convert(-1e-300, XC.F64, XC.F32)) == "-0.0"


def test_plan_covers_every_accepted_combination_exactly_once():
    per, table = XC.plan()
    accepted = XC.accepted_combinations()
    assert len(accepted) == len(set(accepted)) == XC.N_COMBINATIONS == 1680
    assert set(table) == set(accepted)  # a dict: each combination once
    direct = [k for k, s in table.items() if not s.mirror]
    print(f"combinations: {len(table)} accepted, {len(direct)} computed as written, {len(table) - len(direct)} folded into the other operand order")
    assert len(table) - len(direct) == XC.N_MIRRORED == 174 and len(direct) == 1506
    # a folded combination is a commutative function of a mixed pair and points at its mirror image's slot
    for (fn, ty), s in table.items():
        if s.mirror:
            assert fn in (XC.FN["plus"], XC.FN["multiply"]) + tuple(XC.BIT_FNS) and ty[0] != ty[1]
            assert table[(fn, ty[::-1])] == s._replace(mirror=False)
    # every direct combination is a field of exactly one output
    seen = {}
    assert len(per) == 55
    for (a, b), kernels in per.items():
        assert 1 <= len(kernels) <= 2
        for ki, k in enumerate(kernels):
            assert len(k.nodes) <= 256 and 1 <= len(k.out_nodes) <= 8
            for o, fs in enumerate(k.fields):
                for f in fs:
                    assert (f.fn, f.types) not in seen
                    seen[(f.fn, f.types)] = (XC.pair_id(a, b), ki, o)
                    s = table[(f.fn, f.types)]
                    assert (s.pair, s.kernel, s.output) == (XC.pair_id(a, b), ki, o) and s.bit == (f.shift if f.width else None)
                    assert k.nodes[f.node][1] == f.fn and tuple(k.types[j] for j in k.nodes[f.node][3] if j >= 0) == f.types
    assert set(seen) == set(direct)
    n_kernels = sum(len(k) for k in per.values())
    print(f"kernels: {n_kernels}")
    assert n_kernels == 106


def test_every_planned_dag_compiles_with_the_plans_types():
    """chgpu_expr_compile needs no device"""
    import clickhouse_amd as ch
    per, _ = XC.plan()
    dags = [k.nodes for ks in per.values() for k in ks] + [XC.calendar_nodes()] + [c.nodes for c in XC.shape_cases()]
    types = [k.types for ks in per.values() for k in ks] + [None] * (len(dags) - sum(len(ks) for ks in per.values()))
    for nodes, want in zip(dags, types):
        d = ch.ActionsDAG()
        d.nodes = list(nodes)
        ex = d.compile()
        got = [ex.node_type(k) for k in range(len(nodes))]
        assert got == (want if want is not None else XC._types_of(nodes))


def _oracle_and_reference(fn, ty):
    rt = OE.result_type(fn, *ty)
    assert rt is not None
    if fn == XC.FN["if"]:
        a, b, cond = XC.cross_columns(ty[1], ty[2], 3 * len(XC.VALUES[ty[1]]) * len(XC.VALUES[ty[2]]))
        cols = [cond, a, b]
    elif len(ty) == 2:
        cols = list(XC.cross_columns(ty[0], ty[1])[:2])
    else:
        cols = [XC.column(ty[0])]
    with np.errstate(all="ignore"):  # 3.5e38 -> Float32 overflows on purpose
        got = OE.apply_function(fn, cols, list(ty))
    return got, XC.ref_column(fn, cols, ty, rt), cols


def test_scalar_reference_equals_the_oracle_for_every_combination():
    n = rows = 0
    bad = []
    for fn, ty in XC.accepted_combinations():
        got, want, cols = _oracle_and_reference(fn, ty)
        assert got.dtype == want.dtype == np.dtype(XC.NP_OF[OE.result_type(fn, *ty)])
        if not XC.same(got, want):
            i = int(np.flatnonzero(~((got == want) | ((got != got) & (want != want))))[:1].sum())
            bad.append((XC.fn_name(fn), [XC.NAME[t] for t in ty], [c[i] for c in cols], got[i], want[i]))
        n += 1
        rows += got.shape[0]
    print(f"{n} combinations, {rows} rows")
    assert not bad, bad[:10]
    assert n == 1680 and rows > 500_000


def test_if_meets_every_condition_for_every_value_pair():
    a, b, cond = XC.cross_columns(XC.U8, XC.I8, 3 * len(XC.VALUES[XC.U8]) * len(XC.VALUES[XC.I8]))
    seen = {(int(x), int(y), int(c)) for x, y, c in zip(a, b, cond)}
    assert len(seen) == 3 * len(XC.VALUES[XC.U8]) * len(XC.VALUES[XC.I8])
    # and a window one row in sees the same rows shifted
    a1, b1, c1 = XC.cross_columns(XC.U8, XC.I8, 100, offset=1)
    assert np.array_equal(a1, a[1:101]) and np.array_equal(b1, b[1:101]) and np.array_equal(c1, cond[1:101])


def test_calendar_reference_equals_the_oracle_on_every_day_number():
    days = np.arange(65536, dtype=np.uint16)
    nodes = XC.calendar_nodes()
    vals, types = OE.evaluate(nodes, [days])
    ref = XC.calendar_reference()
    for k, f in enumerate(XC.CALENDAR, start=1):
        assert types[k] == OE.result_type(XC.FN[f], XC.U16)
        assert vals[k].tolist() == ref[f], f
    assert ref["toYYYYMMDD"][0] == 19700101 and ref["toYYYYMMDD"][65535] == 21490606 and ref["toDayOfWeek"][0] == 4  # a Thursday


@pytest.mark.parametrize("pair", XC.pairs(), ids=lambda p: XC.pair_id(*p))
def test_bit_packing_round_trip(pair):
    """unpacking the oracle's packed outputs gives the oracle's values of the packed functions' own nodes"""
    a, b = pair
    xa, xb, cond = XC.cross_columns(a, b, 3 * len(XC.VALUES[a]) * len(XC.VALUES[b]))
    n_fields = 0
    for k in XC.plan()[0][pair]:
        with np.errstate(all="ignore"):
            vals, types = OE.evaluate(k.nodes, [xa, xb, cond])
        assert types == k.types
        for o, node in enumerate(k.out_nodes):
            fields = XC.unpack(k, o, vals[node])
            assert len(fields) == len(k.fields[o])
            for f, col in fields:
                assert XC.same(col, vals[f.node]), (XC.fn_name(f.fn), f.types)
                n_fields += 1
            assert XC.mismatches(k, o, vals[node], vals[node]) == []
            if k.fields[o][0].width:  # a flipped bit of a packed word names its function
                flipped = vals[node].copy()
                f = k.fields[o][-1]
                flipped[0] ^= flipped.dtype.type(1 << f.shift)
                names = XC.mismatches(k, o, flipped, vals[node])
                assert len(names) == 1 and names[0].startswith(XC.fn_name(f.fn)), names
    assert n_fields >= 9


def test_shape_cases_pin_every_vector_width():
    cases = XC.shape_cases()
    assert sorted({c.v for c in cases}) == [2, 4, 8, 16]
    assert sum(c.transposed >= 2 for c in cases) == 2  # two one-byte outputs through the LDS transpose, twice
    kinds = {cases[0].nodes[k][0] for k in cases[0].out_nodes}
    assert kinds == {XC.EX_INPUT, XC.EX_CONST, XC.EX_FUNC}
    for c in cases:
        r = XC.chunk_rows(c.v)
        assert XC.shape_sizes(c.v) == [1, 63, 64, 65, r - 1, r, r + 1, 2 * r + 64 * c.v + 3]
