"""Case generators, kernel geometry and plain references for the streaming kernels' test matrix
(tests/test_gpu_streaming_matrix.py runs them on the device, tests/test_streaming_cases.py checks them without one).

Geometry: R = rows one workgroup consumes per main-loop iteration, G = grid cap, both read off the dispatch code; each
function names the line it mirrors.  If a later change moves R the seeded ragged sizes keep the lists meaningful, and the
CPU companion fails until the table here is brought back in line with the source.
"""
import math

import numpy as np

INT_DTYPES = [np.int64, np.uint64, np.uint32, np.int32, np.uint8, np.uint16, np.int16, np.int8]
FLOAT_DTYPES = [np.float64, np.float32]
ALL_DTYPES = INT_DTYPES + FLOAT_DTYPES
EXPR_DTYPES = [np.int64, np.uint64, np.uint32, np.int32, np.uint8]   # what chgpu_expr_filter_sum takes
THREADS = 256                                                        # FS_THREADS / every launch here uses 256 lanes
FLOAT_EXACT_MAX = 2 ** 20                                            # |x| of the exactly summable float columns
FLOAT_EXACT_MAX_ROWS = 2 ** 25


def name(dtype) -> str:
    return np.dtype(dtype).name


def vecw(dtype) -> int:
    """elements of a 16-byte vector (launch_filter_sum_t / launch_cmp_t: VECW = 16 / sizeof(T))"""
    return 16 // np.dtype(dtype).itemsize


# ----------------------------------------------------------------------------------------------------------------
# geometry: (R, G, VEC)
# ----------------------------------------------------------------------------------------------------------------
def filter_sum_geometry(dtype, same: bool, aligned: bool, cus: int):
    """k_filter_sum: UNROLL = SAME ? FS_UNROLL_SAME (4) : (4 + 1) / 2; CHUNK = UNROLL * FS_THREADS vectors of VEC rows;
    grid cap FS_WG_PER_CU (2) workgroups per CU (launch_filter_sum_t)"""
    vec = vecw(dtype) if aligned else 1
    return (4 if same else 2) * THREADS * vec, 2 * cus, vec


def cmp_mask_geometry(dtype, aligned: bool, cus: int):
    """k_cmp_mask: UNROLL = 4, CHUNK = UNROLL * 256 vectors; tune_cmp_wg default 2 (launch_cmp_t)"""
    vec = vecw(dtype) if aligned else 1
    return 4 * THREADS * vec, 2 * cus, vec


def expr_same_geometry(dtype, cus: int):
    """k_expr_filter_sum<T>: EX_UNROLL = 4 vectors of 16 / sizeof(T) rows per lane; tune_expr_wg default 3"""
    vec = vecw(dtype)
    return 4 * THREADS * vec, 3 * cus, vec


def expr_narrow_geometry(cus: int):
    """k_expr_filter_sum_narrow: EXN_UNROLL = 2 units of 4 rows per lane; tune_exprn_wg default 6"""
    return 2 * THREADS * 4, 6 * cus, 4


def expr_mixed_geometry(cus: int):
    """k_expr_filter_sum_mixed: one row per lane and step (EXM_UNROLL = 4 steps in flight, each a whole grid apart);
    tune_expr_wg default 3; the grid is sized for 4 rows per lane (vecw = 4 in chgpu_expr_filter_sum)"""
    return THREADS, 3 * cus, 1


def jit_vec_rows(dtypes) -> int:
    """vec_rows() of expr_jit.hip: 16-byte loads of the widest touched column, at least 4 bytes of the narrowest"""
    sizes = [np.dtype(d).itemsize for d in dtypes]
    return min(16, max(1, max(16 // max(sizes), 4 // min(sizes))))


def jit_sum_geometry(dtypes, aligned: bool, cus: int):
    """generated k_run (sum): 256 lanes x JIT_UNROLL (4) x vec rows; tune_jit_wg_sum default 2; vec = 1 for a view that
    is not 64-byte aligned (cols_aligned)"""
    vec = jit_vec_rows(dtypes) if aligned else 1
    return THREADS * 4 * vec, 2 * cus, vec


def size_list(R: int, G: int, vec: int, seed: int = 0, zero: bool = True, n_random: int = 3):
    """the issue's row counts for one kernel: around the vector, around one chunk, around the whole grid"""
    sizes = {1, vec - 1, vec, vec + 1, R - 1, R, R + 1, R + vec + 1, 3 * R + R // 2 + 3, (G - 1) * R + 5, G * R, G * R + 1,
             (2 * G + 1) * R + vec + 3}
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    sizes |= {int(x) for x in rng.integers(2, (2 * G + 1) * R, size=n_random)}
    sizes.discard(0)
    if zero:
        sizes.add(0)
    return sorted(sizes)


def mid_size(R: int) -> int:
    return 3 * R + R // 2 + 3


def max_rows(cus: int, dtype) -> int:
    """rows to generate per column so that every size list of every family fits, plus a few for views at row 1..3"""
    worst = 0
    for same in (True, False):
        for aligned in (True, False):
            R, G, vec = filter_sum_geometry(dtype, same, aligned, cus)
            worst = max(worst, (2 * G + 1) * R + vec + 3)
    for aligned in (True, False):
        R, G, vec = cmp_mask_geometry(dtype, aligned, cus)
        worst = max(worst, (2 * G + 1) * R + vec + 3)
    return worst + 4


def edge_rows(n: int, R: int, vec: int):
    """row 0, the last row, the last row of the main loop, the first row of the remainder loop, the first of the scalar tail"""
    if n == 0:
        return []
    main_end = (n // R) * R
    tail = (n // vec) * vec
    return sorted({r for r in (0, n - 1, main_end - 1, main_end, tail) if 0 <= r < n})


# ----------------------------------------------------------------------------------------------------------------
# columns
# ----------------------------------------------------------------------------------------------------------------
def limits(dtype):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return -FLOAT_EXACT_MAX, FLOAT_EXACT_MAX
    info = np.iinfo(dt)
    return int(info.min), int(info.max)


def threshold(dtype) -> int:
    """about the median of a uniform column, never at the ends of the range"""
    lo, hi = limits(dtype)
    return (lo + hi) // 2 + 3


def planted_values(dtype):
    lo, hi = limits(dtype)
    t = threshold(dtype)
    return [lo, hi, t - 1, t, t + 1]


def uniform_column(dtype, n: int, seed: int) -> np.ndarray:
    """integers: uniform over the whole range of the type; floats: integer-valued, |x| <= 2^20 (exactly summable)"""
    dt = np.dtype(dtype)
    rng = np.random.Generator(np.random.PCG64(seed))
    lo, hi = limits(dt)
    if dt.kind == "f":
        assert n <= FLOAT_EXACT_MAX_ROWS
        return rng.integers(lo, hi, size=n, endpoint=True).astype(dt)
    return rng.integers(lo, hi, size=n, dtype=dt, endpoint=True)


def plant(col: np.ndarray, rows, shift: int = 0) -> np.ndarray:
    """min, max, thr - 1, thr, thr + 1 in turn at the given rows (in place)"""
    vals = planted_values(col.dtype)
    for k, r in enumerate(sorted(set(int(r) for r in rows))):
        if 0 <= r < col.shape[0]:
            col[r] = vals[(k + shift) % len(vals)]
    return col


def all_edge_rows(geometries, sizes_of, starts=(0, 1)):
    """every edge row, over every (R, G, vec) of `geometries`, every size of sizes_of(R, G, vec) and every view start"""
    rows = set()
    for R, G, vec in geometries:
        for n in sizes_of(R, G, vec):
            for s in starts:
                rows |= {s + r for r in edge_rows(n, R, vec)}
    return rows


def mask_column(n: int, seed: int, keep_one_in: int = 3) -> np.ndarray:
    """IColumn::Filter bytes: zero or any non-zero byte (1, 2, 7, 128, 255 ...)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    nz = rng.choice(np.array([1, 2, 7, 128, 255], dtype=np.uint8), size=n)
    return np.where(rng.integers(0, keep_one_in, size=n) == 0, nz, np.uint8(0)).astype(np.uint8)


def rough_float_column(dtype, n: int, seed: int) -> np.ndarray:
    """general values of mixed sign and magnitude (the rounding path)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 6, size=n)).astype(dtype)


# ----------------------------------------------------------------------------------------------------------------
# plain references (Python integers / math.fsum): the second witness next to the C oracle
# ----------------------------------------------------------------------------------------------------------------
OPS = {0: lambda a, s: a == s, 1: lambda a, s: a != s, 2: lambda a, s: a < s, 3: lambda a, s: a > s, 4: lambda a, s: a <= s,
       5: lambda a, s: a >= s}
OP_NAMES = {0: "EQ", 1: "NE", 2: "LT", 3: "GT", 4: "LE", 5: "GE"}


def py_scalar(x):
    """numpy scalar -> Python int / float (Python compares int with float mathematically, as accurate::lessOp does)"""
    return x.item() if isinstance(x, np.generic) else x


def py_pass(col: np.ndarray, op: int, scalar) -> list:
    s = py_scalar(scalar)
    f = OPS[op]
    return [bool(f(a, s)) for a in col.tolist()]


def wrap64(v: int, signed: bool) -> int:
    v %= 2 ** 64
    return v - 2 ** 64 if signed and v >= 2 ** 63 else v


def py_filter_sum(pred: np.ndarray, op: int, scalar, val: np.ndarray, mask: np.ndarray = None):
    """(sum, count) with Python arithmetic: integers modulo 2^64 in the sum's signedness, floats by math.fsum"""
    keep = py_pass(pred, op, scalar) if op is not None else [True] * val.shape[0]
    if mask is not None:
        keep = [k and m != 0 for k, m in zip(keep, mask.tolist())]
    sel = [v for v, k in zip(val.tolist(), keep) if k]
    if val.dtype.kind == "f":
        return math.fsum(sel), len(sel)
    return wrap64(sum(sel), val.dtype.kind == "i"), len(sel)


VAL_COL, VAL_MUL, VAL_PLUS, VAL_MINUS = 0, 1, 2, 3
VAL_NAMES = {0: "col", 1: "mul", 2: "plus", 3: "minus"}


def expr_result_signed(value_op: int, dt_a, dt_b) -> bool:
    """NumberTraits (NumberTraits.h:73-87) for integer operands of <= 8 bytes: minus is always signed, multiply / plus are
    signed when either operand is; a bare column sums in its own signedness"""
    sa, sb = np.dtype(dt_a).kind == "i", np.dtype(dt_b).kind == "i"
    if value_op == VAL_COL:
        return sa
    return True if value_op == VAL_MINUS else (sa or sb)


def py_expr_filter_sum(cols, preds, value_op: int, val_a: int, val_b: int = 0):
    """(sum, count, signed) of the fused expression in Python integers: every row's value wraps to 64 bits, then the sum does"""
    n = cols[0].shape[0]
    keep = [True] * n
    for p in preds:
        keep = [k and q for k, q in zip(keep, py_pass(cols[p[0]], p[1], p[2]))]
    a = cols[val_a].tolist()
    b = cols[val_b].tolist() if value_op != VAL_COL else a
    f = {VAL_COL: lambda x, y: x, VAL_MUL: lambda x, y: x * y, VAL_PLUS: lambda x, y: x + y, VAL_MINUS: lambda x, y: x - y}[value_op]
    signed = expr_result_signed(value_op, cols[val_a].dtype, cols[val_b if value_op != VAL_COL else val_a].dtype)
    total = sum(wrap64(f(x, y), signed) for x, y, k in zip(a, b, keep) if k)
    return wrap64(total, signed), sum(keep), signed


def fold_constants(dtype):
    """(scalar, dtype of the scalar) pairs for one integer column type: inside the range, at its ends, outside on both sides,
    typed as the column, as Int64, as UInt64 and as a fractional Float64"""
    lo, hi = limits(dtype)
    t = threshold(dtype)
    out = [(t, dtype), (lo, dtype), (hi, dtype)]
    out += [(v, np.int64) for v in (t, lo, hi, lo - 1, max(lo - 2 ** 40, -2 ** 63), -1, -2 ** 63) if -2 ** 63 <= v < 2 ** 63]
    out += [(v, np.int64) for v in (hi + 1, min(hi + 2 ** 40, 2 ** 63 - 1)) if v < 2 ** 63]
    out += [(v, np.uint64) for v in (max(t, 0), max(hi, 0), hi + 1, 2 ** 63, 2 ** 64 - 1) if 0 <= v < 2 ** 64]
    out += [(float(v), np.float64) for v in (t + 0.5, lo - 0.5, hi + 0.5, -0.5, lo + 0.0, 1e30, -1e30) if abs(v) < 2 ** 53 or abs(v) >= 1e30]
    seen, uniq = set(), []
    for v, d in out:
        if (v, np.dtype(d).name) not in seen:
            seen.add((v, np.dtype(d).name))
            uniq.append((v, d))
    return uniq
