"""TEST INFRASTRUCTURE ONLY -- the cases of the expression compiler's matrix (tests/test_expr_cases.py on the CPU,
tests/test_gpu_expr_matrix.py on the device).  Importable without a GPU.

Four parts:
  values      adversarial values per type (VALUES): the ends of every integer range, powers of two and their neighbours, the
              Float64 / Float32 values at which conversions and comparisons change their answer (2^24+1, 2^53+2, 2^63, 2^64,
              subnormal Float32, overflow to inf), 2^60+2^36+1 (integer -> Float32 through Float64 rounds twice: 2^60 instead of 2^60+2^37)
  reference   ref_apply: one scalar function per function family on Python integers, Python floats (IEEE Float64) and exact
              rationals (fractions.Fraction).  It shares nothing with oracle/expr_dag.py: no numpy, no long double, no whole-column
              casts.  The result TYPE is an argument (types are pinned elsewhere, against NumberTraits.h compiled in place).
  plan        plan_pair: for every unordered pair of the 10 types at most two DAGs of at most 8 outputs each that hold every accepted
              (function, operand types) combination of the pair; one-bit results are packed into a UInt32 inside the DAG
              (if(bit, 2^k, 0) folded by bitOr), the six narrow casts into two Int64 (multiply by 2^k, plus).  TABLE maps
              (function code, operand types) -> Slot so that a mismatch names its function.
  shapes      the small DAGs that pin the vector width V of the generated kernel, and the row counts around its chunk size.
"""
from __future__ import annotations

import datetime
import math
import struct
from collections import namedtuple
from fractions import Fraction

import numpy as np

from oracle import expr_dag as OE  # type tags, function codes, result types (the plan's types; the reference below does not use it)

I64, U32, U64, F64, U8, I32, U16, I16, I8, F32 = range(10)
TAGS = list(range(10))
NAME = {I64: "Int64", U32: "UInt32", U64: "UInt64", F64: "Float64", U8: "UInt8", I32: "Int32", U16: "UInt16", I16: "Int16", I8: "Int8",
        F32: "Float32"}
NP_OF = {I64: np.int64, U32: np.uint32, U64: np.uint64, F64: np.float64, U8: np.uint8, I32: np.int32, U16: np.uint16, I16: np.int16,
         I8: np.int8, F32: np.float32}
BITS = {I64: 64, U32: 32, U64: 64, F64: 64, U8: 8, I32: 32, U16: 16, I16: 16, I8: 8, F32: 32}
SIGNED_INT = (I64, I32, I16, I8)
FLOATS = (F64, F32)
INTS = [t for t in TAGS if t not in FLOATS]
EX_INPUT, EX_CONST, EX_FUNC = 0, 1, 2
FN = dict(OE.FN)
FN_CAST = OE.FN_CAST
FN_NAME = {v: k for k, v in FN.items()}
CMP_FNS = [FN[f] for f in ("equals", "notEquals", "less", "greater", "lessOrEquals", "greaterOrEquals")]
LOGIC_FNS = [FN[f] for f in ("and", "or", "xor")]
BIT_FNS = [FN[f] for f in ("bitAnd", "bitOr", "bitXor")]
CALENDAR = ["toYear", "toMonth", "toDayOfMonth", "toYYYYMM", "toYYYYMMDD", "toDayOfWeek", "toQuarter", "toStartOfMonth"]


def fn_name(fn):
    return "to" + NAME[fn - FN_CAST] if fn >= FN_CAST else FN_NAME[fn]


def is_float(t):
    return t in FLOATS


# ----------------------------------------------------------------------------------------------------------------------
# values
# ----------------------------------------------------------------------------------------------------------------------
def _int_values(t):
    bits, sg = BITS[t], t in SIGNED_INT
    lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if sg else (0, (1 << bits) - 1)
    v = [0, 1, -1, 2, -2, lo, lo + 1, hi, hi - 1]
    for k in (7, 8, 15, 16, 24, 31, 32, 53, 63):
        v += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    for k in (7, 8, 15, 16, 24, 31, 32, 53):
        v.append(-(1 << k))
    v += [-(1 << 7) - 1, -(1 << 15) - 1, -(1 << 31) - 1]  # one below the narrower types' minimum: sign extension
    if bits == 64:
        v += [(1 << 60) + (1 << 36) + 1, -((1 << 60) + (1 << 36) + 1), (1 << 53) + 1]
    out = []
    for x in v:
        if lo <= x <= hi and x not in out:
            out.append(x)
    return out


_F64_VALUES = [0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 2.5, math.nan, math.inf, -math.inf,
               2.0**24, 2.0**24 + 1, 2.0**53, 2.0**53 + 2,
               2.0**63, -(2.0**63), 2.0**63 + 2048, 2.0**64, 4294967295.5, -2147483648.5,
               1e300, 1e-300, 1e-40, 1e-45, 3.4028235e38, 3.5e38,
               # the neighbours of the integer types' ends, the largest Float64 below 2^63 and below 2^64
               -2.5, 1.5, 255.0, 256.0, -128.0, -129.0, 32767.0, -32769.0, 65535.0, 16777215.0, 2147483648.0, 4294967296.0,
               2.0**63 - 1024, 2.0**64 - 2048, -1e300]


def _float_values(t):
    if t == F64:
        return list(_F64_VALUES)
    out, seen = [], set()
    with np.errstate(over="ignore"):
        for x in _F64_VALUES:  # the value where Float32 holds it, else its rounding (1e300 -> inf, 1e-45 -> the smallest subnormal, 1e-300 -> 0)
            y = np.float32(x)
            key = "nan" if y != y else y.tobytes()
            if key not in seen:
                seen.add(key)
                out.append(float(y))
    return out


VALUES = {t: (_float_values(t) if is_float(t) else _int_values(t)) for t in TAGS}
assert all(len(v) <= 48 for v in VALUES.values())


def column(t):
    return np.array(VALUES[t], dtype=NP_OF[t])


def cross_columns(a, b, n=None, offset=0):
    """rows offset .. offset+n-1 of the endlessly tiled cross product of VALUES[a] x VALUES[b] and the condition column 0 / 1 / 255;
    the condition shifts by one from tile to tile, so every value pair meets every condition within three tiles"""
    va, vb = column(a), column(b)
    period = va.shape[0] * vb.shape[0]
    n = period if n is None else n
    i = np.arange(offset, offset + n, dtype=np.int64)
    j = i % period
    cond = np.array([0, 1, 255], dtype=np.uint8)[(i + i // period) % 3]
    return va[j // vb.shape[0]], vb[j % vb.shape[0]], cond


# ----------------------------------------------------------------------------------------------------------------------
# the scalar reference
# ----------------------------------------------------------------------------------------------------------------------
def wrap(v: int, t) -> int:
    """the exact integer reduced modulo 2^bits into the range of t"""
    bits = BITS[t]
    v &= (1 << bits) - 1
    if t in SIGNED_INT and v >> (bits - 1):
        v -= 1 << bits
    return v


def round_f32(q: Fraction) -> float:
    """the exact rational q -> the nearest Float32 (ties to even) in ONE rounding: gradual underflow, overflow to infinity"""
    if q == 0:
        return 0.0
    sign, q = (-1.0, -q) if q < 0 else (1.0, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    elif Fraction(2) ** (e + 1) <= q:
        e += 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1)
    e = max(e, -126)  # subnormals keep the spacing of the smallest normal
    ulp = Fraction(2) ** (e - 23)
    m = q / ulp
    n = m.numerator // m.denominator
    r = m - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n & 1):
        n += 1
    val = n * ulp
    if val >= Fraction(2) ** 128:
        return sign * math.inf
    return sign * float(val)  # exact: at most 24 significant bits


def round_f64(v: int) -> float:
    """integer -> nearest Float64, ties to even (what Python's int -> float conversion is specified to do)"""
    return float(v)


def convert(v, tf, tt):
    """static_cast<tt>(v) for v of type tf; Float -> integer is not carried"""
    if is_float(tt):
        if is_float(tf):
            if tt == F64 or tf == F32 or v != v or v in (math.inf, -math.inf) or v == 0:
                return v  # widening is exact; NaN, infinities and signed zeros pass through
            return round_f32(Fraction(v))
        return round_f64(v) if tt == F64 else round_f32(Fraction(v))
    if is_float(tf):
        raise NotImplementedError("Float -> integer")
    return wrap(v, tt)


def _fdiv(x: float, y: float) -> float:
    if y == 0:  # IEEE 754: x / 0 is an infinity of the product of the signs, 0 / 0 and NaN / 0 are NaN
        if x != x or x == 0:
            return math.nan
        return math.copysign(math.inf, x) * math.copysign(1.0, y)
    return x / y


def _truth(v) -> bool:
    return v != 0  # NaN != 0 is true, -0.0 != 0 is false


def _date(days: int) -> datetime.date:
    return datetime.date(1970, 1, 1) + datetime.timedelta(days=days)


def ref_apply(fn, args, types, rt):
    """the value of fn(args) -- args of the given types -- in the result type rt, as a Python int or float"""
    a, ta = args[0], types[0]
    if fn in CMP_FNS:  # Python compares int with float, int with int and float with float mathematically exactly
        b = args[1]
        if a != a or b != b:
            return int(fn == FN["notEquals"])
        return int({FN["equals"]: a == b, FN["notEquals"]: a != b, FN["less"]: a < b, FN["greater"]: a > b, FN["lessOrEquals"]: a <= b,
                    FN["greaterOrEquals"]: a >= b}[fn])
    if fn in (FN["plus"], FN["minus"], FN["multiply"]):
        b, tb = args[1], types[1]
        if is_float(rt):
            x, y = convert(a, ta, F64), convert(b, tb, F64)
            return convert(x + y if fn == FN["plus"] else x - y if fn == FN["minus"] else x * y, F64, rt)
        return wrap(a + b if fn == FN["plus"] else a - b if fn == FN["minus"] else a * b, rt)
    if fn == FN["divide"]:
        return _fdiv(convert(a, ta, F64), convert(args[1], types[1], F64))
    if fn == FN["negate"]:
        return -a if is_float(rt) else wrap(-a, rt)
    if fn in LOGIC_FNS:
        x, y = _truth(a), _truth(args[1])
        return int(x and y if fn == FN["and"] else x or y if fn == FN["or"] else x != y)
    if fn == FN["not"]:
        return int(not _truth(a))
    if fn in BIT_FNS:  # Python's & | ^ on negative integers act on the infinitely sign-extended two's complement
        b = args[1]
        return wrap(a & b if fn == FN["bitAnd"] else a | b if fn == FN["bitOr"] else a ^ b, rt)
    if fn == FN["if"]:
        return convert(args[1], types[1], rt) if _truth(a) else convert(args[2], types[2], rt)
    if fn >= FN_CAST:
        return convert(a, ta, rt)
    d = _date(a)
    return {"toYear": d.year, "toMonth": d.month, "toDayOfMonth": d.day, "toYYYYMM": d.year * 100 + d.month,
            "toYYYYMMDD": d.year * 10000 + d.month * 100 + d.day, "toDayOfWeek": d.isoweekday(), "toQuarter": (d.month - 1) // 3 + 1,
            "toStartOfMonth": (d.replace(day=1) - datetime.date(1970, 1, 1)).days}[FN_NAME[fn]]


def ref_column(fn, cols, types, rt):
    """ref_apply over rows of numpy columns -> a numpy column of the result type (the conversions to and from Python scalars are exact)"""
    lists = [c.tolist() for c in cols]
    out = [ref_apply(fn, row, types, rt) for row in zip(*lists)]
    if rt == F32:
        return np.array([struct.unpack("<I", struct.pack("<f", x))[0] for x in out], dtype=np.uint32).view(np.float32)
    return np.array(out, dtype=NP_OF[rt])


def same(a, b):
    """integers equal; floats bit for bit, the sign of zero included, NaN == NaN (the rule of tests/test_expr_dag.py)"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))) and np.all(np.signbit(a[~np.isnan(a)]) == np.signbit(b[~np.isnan(b)])))
    return bool(np.array_equal(a, b))


# ----------------------------------------------------------------------------------------------------------------------
# the matrix plan
# ----------------------------------------------------------------------------------------------------------------------
Slot = namedtuple("Slot", "pair kernel output bit mirror")       # bit: the bit of a packed UInt32 / the field of a packed Int64 / None
Field = namedtuple("Field", "fn types node shift width signed")  # one function's result inside an output; width 0: the whole output
Kernel = namedtuple("Kernel", "nodes types out_nodes fields")    # fields[o]: the Fields of output o (one for an unpacked output)
NARROW = [[(U8, 0), (I8, 8), (U16, 16), (I16, 32)], [(U32, 0), (I32, 32)]]  # the casts packed into two Int64: sum of value * 2^shift


class _Dag:
    def __init__(self, in_types):
        self.nodes, self.types, self.in_types, self.inputs, self.consts = [], [], in_types, {}, {}

    def inp(self, j):
        if j not in self.inputs:
            self.nodes.append((EX_INPUT, j, self.in_types[j], (-1, -1, -1), 0))
            self.types.append(self.in_types[j])
            self.inputs[j] = len(self.nodes) - 1
        return self.inputs[j]

    def const(self, v, t):
        if (v, t) not in self.consts:
            bits = int.from_bytes(np.array([v], dtype=NP_OF[t]).tobytes().ljust(8, b"\0"), "little")
            self.nodes.append((EX_CONST, 0, t, (-1, -1, -1), bits))
            self.types.append(t)
            self.consts[(v, t)] = len(self.nodes) - 1
        return self.consts[(v, t)]

    def fn(self, code, *args):
        rt = OE.result_type(code, *[self.types[k] for k in args])
        assert rt is not None, (code, [self.types[k] for k in args])
        self.nodes.append((EX_FUNC, code, 0, tuple(args) + (-1,) * (3 - len(args)), 0))
        self.types.append(rt)
        return len(self.nodes) - 1


def pairs():
    return [(a, b) for i, a in enumerate(TAGS) for b in TAGS[i:]]


def pair_id(a, b):
    return f"{NAME[a]}-{NAME[b]}"


def _pair_items(a, b):
    """(value items, packs of (narrow cast item, shift), bit items, mirrors): an item is (fn, operand types, input positions); input 0 has type a, 1 type b,
    2 is the UInt8 condition.  mirrors: (fn, types) -> the item that computes it with its operands exchanged."""
    both_int = not is_float(a) and not is_float(b)
    values, narrow, bits, mirrors = [], [], [], {}
    orders = [((a, b), (0, 1))] + ([((b, a), (1, 0))] if a != b else [])
    for name in ("plus", "multiply"):
        values.append((FN[name], (a, b), (0, 1)))
        if a != b:
            mirrors[(FN[name], (b, a))] = (FN[name], (a, b))
    for name in ("minus", "divide"):
        for ty, pos in orders:
            values.append((FN[name], ty, pos))
    for ty, pos in orders:
        if OE.result_type(FN["if"], U8, *ty) is not None:
            values.append((FN["if"], (U8,) + ty, (2,) + pos))
    if both_int:
        for f in BIT_FNS:
            values.append((f, (a, b), (0, 1)))
            if a != b:
                mirrors[(f, (b, a))] = (f, (a, b))
    for ty, pos in orders:
        for f in CMP_FNS + LOGIC_FNS:
            bits.append((f, ty, pos))
    if a == b:
        bits.append((FN["not"], (a,), (0,)))
        values.append((FN["negate"], (a,), (0,)))
        for to in TAGS:
            if OE.result_type(FN_CAST + to, a) is None:
                continue
            if is_float(a) or to not in [t for pack in NARROW for t, _ in pack]:
                values.append((FN_CAST + to, (a,), (0,)))
        if not is_float(a):
            narrow = [[((FN_CAST + to, (a,), (0,)), shift) for to, shift in pack] for pack in NARROW]
    return values, narrow, bits, mirrors


def _build_kernel(in_types, outputs):
    """outputs: ("value", item) | ("narrow", [(item, shift)]) | ("bits", items) -> Kernel"""
    d = _Dag(in_types)
    out_nodes, fields = [], []
    for kind, what in outputs:
        if kind == "value":
            fn, ty, pos = what
            k = d.fn(fn, *[d.inp(j) for j in pos])
            out_nodes.append(k)
            fields.append([Field(fn, ty, k, 0, 0, False)])
        elif kind == "narrow":
            acc, fs = None, []
            for (fn, ty, pos), shift in what:
                to = fn - FN_CAST
                k = d.fn(fn, *[d.inp(j) for j in pos])
                term = d.fn(FN["multiply"], k, d.const(1 << shift, U64))  # UInt64 or Int64: value * 2^shift modulo 2^64
                acc = term if acc is None else d.fn(FN["plus"], acc, term)
                fs.append(Field(fn, ty, k, shift, BITS[to], to in SIGNED_INT))
            assert d.types[acc] == I64
            out_nodes.append(acc)
            fields.append(fs)
        else:
            acc, fs = None, []
            zero = d.const(0, U32)
            for bit, (fn, ty, pos) in enumerate(what):
                k = d.fn(fn, *[d.inp(j) for j in pos])
                assert d.types[k] == U8
                term = d.fn(FN["if"], k, d.const(1 << bit, U32), zero)
                acc = term if acc is None else d.fn(FN["bitOr"], acc, term)
                fs.append(Field(fn, ty, k, bit, 1, False))
            assert d.types[acc] == U32 and len(what) <= 32
            out_nodes.append(acc)
            fields.append(fs)
    return Kernel(d.nodes, d.types, out_nodes, fields)


def plan_pair(a, b):
    """-> (kernels, table): at most two kernels of at most 8 outputs; table: (fn, operand types) -> Slot"""
    values, narrow, bits, mirrors = _pair_items(a, b)
    outputs = [("value", v) for v in values] + [("narrow", pack) for pack in narrow] + [("bits", bits)]
    assert len(outputs) <= 16, (a, b, len(outputs))
    in_types = [a, b, U8]
    kernels = [_build_kernel(in_types, outputs[lo:lo + 8]) for lo in range(0, len(outputs), 8)]
    table = {}
    pid = pair_id(a, b)
    for ki, k in enumerate(kernels):
        for o, fs in enumerate(k.fields):
            for f in fs:
                assert (f.fn, f.types) not in table
                table[(f.fn, f.types)] = Slot(pid, ki, o, f.shift if f.width else None, False)
    for key, of in mirrors.items():
        assert key not in table
        table[key] = table[of]._replace(mirror=True)
    return kernels, table


_PLAN = None


def plan():
    """{(a, b): kernels}, TABLE over all 55 pairs"""
    global _PLAN
    if _PLAN is None:
        per, table = {}, {}
        for a, b in pairs():
            ks, t = plan_pair(a, b)
            per[(a, b)] = ks
            assert not (set(t) & set(table))
            table.update(t)
        _PLAN = (per, table)
    return _PLAN


def accepted_combinations():
    """every (fn, operand types) the compiler accepts, intDiv / modulo (constant divisors only: their own test) and the calendar
    (Date only: its own kernel) apart"""
    out = []
    for name, fn in FN.items():
        if name in ("intDiv", "modulo") or name in CALENDAR:
            continue
        if name in ("negate", "not"):
            cases = [(a,) for a in TAGS]
        elif name == "if":
            cases = [(U8, b, c) for b in TAGS for c in TAGS]
        else:
            cases = [(a, b) for a in TAGS for b in TAGS]
        out += [(fn, ty) for ty in cases if OE.result_type(fn, *ty) is not None]
    out += [(FN_CAST + to, (a,)) for to in TAGS for a in TAGS if OE.result_type(FN_CAST + to, a) is not None]
    return out


N_COMBINATIONS = 1680          # 6 comparisons, plus, minus, multiply, divide, and, or, xor at 100; bit* at 64; if 84; casts 84; negate, not 10
N_MIRRORED = 2 * 45 + 3 * 28   # plus, multiply of the 45 mixed pairs and bitAnd, bitOr, bitXor of the 28 mixed integer pairs: one operand order


def unpack(kernel, o, arr):
    """the output column o of a kernel -> [(Field, its column)]"""
    fs = kernel.fields[o]
    if fs[0].width == 0:
        return [(fs[0], arr)]
    if fs[0].width == 1:
        return [(f, ((arr >> np.uint32(f.shift)) & np.uint32(1)).astype(np.uint8)) for f in fs]
    out, rem = [], arr.view(np.uint64).copy()
    for f in fs:  # lowest field first: take the digit, remove it (a negative digit borrows from the fields above)
        digit = (rem >> np.uint64(f.shift)) & np.uint64((1 << f.width) - 1)
        t = f.fn - FN_CAST
        v = digit.astype(np.dtype(NP_OF[t]).str.replace("i", "u")).view(NP_OF[t])
        out.append((f, v))
        with np.errstate(over="ignore"):
            rem = rem - (v.astype(np.int64).view(np.uint64) << np.uint64(f.shift))
    assert not rem.any()
    return out


def mismatches(kernel, o, got, want):
    """names of the functions whose results differ between two columns of output o"""
    bad = []
    try:
        g, w = unpack(kernel, o, got), unpack(kernel, o, want)
    except AssertionError:
        return [f"{fn_name(f.fn)}{tuple(NAME[t] for t in f.types)}?" for f in kernel.fields[o]]
    for (f, x), (_, y) in zip(g, w):
        if not same(x, y):
            differ = ~((x == y) | ((x != x) & (y != y)))
            if x.dtype.kind == "f":
                differ |= (np.signbit(x) != np.signbit(y)) & ~(x != x)
            i = int(np.flatnonzero(differ)[0])
            bad.append(f"{fn_name(f.fn)}{tuple(NAME[t] for t in f.types)} row {i}: got {x[i]!r}, want {y[i]!r}")
    return bad


def calendar_nodes():
    """one DAG with the eight calendar functions of a Date (UInt16 day number); outputs = nodes 1..8"""
    return [(EX_INPUT, 0, U16, (-1, -1, -1), 0)] + [(EX_FUNC, FN[f], 0, (0, -1, -1), 0) for f in CALENDAR]


def calendar_reference():
    """{function: its 65536 values from datetime.date}"""
    days = range(65536)
    return {f: [ref_apply(FN[f], (d,), (U16,), None) for d in days] for f in CALENDAR}


# ----------------------------------------------------------------------------------------------------------------------
# kernel shapes
# ----------------------------------------------------------------------------------------------------------------------
def vec_rows(types):
    """rows per lane and vector of the generated kernel (expr_jit.hip, vec_rows): 16-byte loads of the widest column among the inputs
    and outputs, at least 4 bytes of the narrowest"""
    w = [BITS[t] // 8 for t in types]
    return min(16, max(1, 16 // max(w), 4 // min(w)))


UNROLL = 4  # vectors in flight per lane and column (tune_jit_unroll's default)


def chunk_rows(v):
    """rows one workgroup takes per turn of its chunk loop"""
    return 256 * UNROLL * v


def shape_sizes(v):
    r = chunk_rows(v)
    return [1, 63, 64, 65, r - 1, r, r + 1, 2 * r + 64 * v + 3]


ShapeCase = namedtuple("ShapeCase", "name v in_types nodes out_nodes transposed")


def shape_cases():
    """one small DAG per vector width; the out_nodes of the first hold an INPUT and a CONST node"""
    cases = []
    d = _Dag([I64])
    p = d.fn(FN["plus"], d.inp(0), d.const(-3, I64))
    cases.append(ShapeCase("v2_int64", 2, [I64], d.nodes, [p, d.inp(0), d.const(-3, I64)], 0))
    d = _Dag([U32])
    outs = [d.fn(FN["less"], d.inp(0), d.const(2**31, U32)), d.fn(FN["bitXor"], d.inp(0), d.const(0xA5A5A5A5, U32)),
            d.fn(FN["greaterOrEquals"], d.inp(0), d.const(2**30, U32))]
    cases.append(ShapeCase("v4_uint32_bytes_transposed", 4, [U32], d.nodes, outs, 2))
    d = _Dag([I64, U8])
    outs = [d.fn(FN["bitAnd"], d.inp(1), d.const(0x5A, U8)), d.fn(FN["plus"], d.inp(0), d.inp(1)), d.fn(FN["less"], d.inp(0), d.inp(1))]
    cases.append(ShapeCase("v4_int64_uint8_bytes_transposed", 4, [I64, U8], d.nodes, outs, 2))
    d = _Dag([U16])
    outs = [d.fn(FN["bitXor"], d.inp(0), d.const(0x0FF0, U16)), d.fn(FN["toStartOfMonth"], d.inp(0))]
    cases.append(ShapeCase("v8_uint16", 8, [U16], d.nodes, outs, 0))
    d = _Dag([U8])
    outs = [d.fn(FN["and"], d.inp(0), d.const(1, U8)), d.fn(FN["not"], d.inp(0)), d.fn(FN["bitAnd"], d.inp(0), d.const(0x3C, U8))]
    cases.append(ShapeCase("v16_uint8", 16, [U8], d.nodes, outs, 0))
    for c in cases:
        ty = _types_of(c.nodes)
        assert vec_rows(list(c.in_types) + [ty[k] for k in c.out_nodes]) == c.v, c.name
        one_byte = sum(BITS[ty[k]] == 8 for k in c.out_nodes)
        assert c.transposed == (one_byte if c.v * UNROLL == 16 else 0), c.name
    return cases


def _types_of(nodes):
    ty = []
    for kind, code, t, args, _ in nodes:
        if kind == EX_FUNC:
            ar = 3 if code == FN["if"] else 1 if (code in (FN["negate"], FN["not"]) or 50 <= code <= 57 or code >= FN_CAST) else 2
            t = OE.result_type(code, *[ty[args[j]] for j in range(ar)])
        ty.append(t)
    return ty


def random_column(rng, t, n):
    """full-range integers / finite floats with the type's ends sprinkled in"""
    if is_float(t):
        return (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 12, size=n)).astype(NP_OF[t])
    info = np.iinfo(NP_OF[t])
    x = rng.integers(info.min, info.max, size=n, dtype=NP_OF[t], endpoint=True)
    x[rng.integers(0, n, size=max(1, n // 16))] = rng.choice(np.array([info.min, info.max, 0, 1], dtype=NP_OF[t]), size=max(1, n // 16))
    return x
