// expr_jit.hip — SURVEY §8(f) rank 1: the expression DAG of a query step compiled at run time into ONE HIP kernel.
//
// Replaces ExpressionActions::execute (src/Interpreters/ExpressionActions.cpp:595-747), which runs every action of the DAG as a
// separate IFunction::executeImpl and materialises every intermediate column, and stands where the reference's own run-time
// compiler stands (setting compile_expressions: src/Interpreters/JIT/CHJIT.cpp, src/Interpreters/JIT/compileFunction.cpp,
// ExpressionJIT.cpp — LLVM IR per fused sub-DAG, cached by DAG hash).  Here the DAG becomes the body of a hand-written
// streaming kernel skeleton (contiguous chunk per workgroup iteration, 16..64-byte nontemporal loads issued before first use,
// wave64 shuffle reduction — the geometry of k_filter_sum), compiled for gfx950 with hiprtc and cached by source text.
//   k_run             : any set of DAG nodes -> materialised columns (ActionsDAG outputs)
//   k_run + k_fin     : WHERE <node> + sum(<node>), count() in one pass, nothing materialised (FilterTransform + AggregatingTransform
//                       without key fused behind the expression)
//   k_fcount + k_femit: WHERE <node> + the surviving rows of any set of DAG nodes
//   k_mm + k_mm_fin   : WHERE <node> + min(<node>), max(<node>), count()
// Each thing is written once:
//   FUNCTIONS   one row per function: code, arity, result-type rule, right-hand side, compile-time gate.  Semantics restated per
//               row (types: src/DataTypes/NumberTraits.h:40-215; comparisons: src/Core/AccurateComparison.h:20-204; logical:
//               src/Functions/FunctionsLogical.h:82-140; arithmetic: src/Functions/FunctionBinaryArithmetic.h; dates:
//               DateTimeTransforms.h ToYearImpl/ToMonthImpl/ToYYYYMMImpl/ToDayOfMonthImpl over DayNum).
//   gen_frame   what every generated program starts with: prelude, Args (ARGS_DECL, beside the host's JitArgs), Row, Res, eval();
//               row_load and out_store are the row's way in and out.  The four kernel bodies are different algorithms and stay apart.
//   launch path make_spec (what to generate, validated), bind_inputs, jit_functions, launch, run_reduction (the two reductions),
//               OutCols (the owner of the result columns until the caller has them).
#include "chgpu_internal.h"

#include <dlfcn.h>

#include <mutex>
#include <string>

namespace
{

// ---- hiprtc, resolved at first use (no link-time dependency: the process may already hold PyTorch's copy of the library) ----
struct Rtc
{
    void * h = nullptr;
    int (*create)(void **, const char *, const char *, int, const char * const *, const char * const *) = nullptr;
    int (*compile)(void *, int, const char * const *) = nullptr;
    int (*log_size)(void *, size_t *) = nullptr;
    int (*log)(void *, char *) = nullptr;
    int (*code_size)(void *, size_t *) = nullptr;
    int (*code)(void *, char *) = nullptr;
    int (*destroy)(void **) = nullptr;
};
Rtc g_rtc;
std::mutex g_jit_mutex;
std::map<std::string, std::vector<char>> g_code_cache;                    // source text -> code object
std::map<std::pair<int, std::string>, hipModule_t> g_module_cache;        // (device, source text) -> loaded module

int rtc_load()
{
    if (g_rtc.h)
        return CHGPU_OK;
    const char * names[] = {"libhiprtc.so.7", "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so"};
    void * h = nullptr;
    for (const char * n : names)
        if ((h = dlopen(n, RTLD_NOW | RTLD_LOCAL)))
            break;
    if (!h)
        return chgpu_set_error(CHGPU_ERR_NOT_IMPLEMENTED, "cannot load libhiprtc (%s): expressions stay on the CPU", dlerror());
#define SYM(field, name)                                              \
    *(void **)&g_rtc.field = dlsym(h, name);                          \
    if (!g_rtc.field)                                                 \
        return chgpu_set_error(CHGPU_ERR_DEVICE, "libhiprtc lacks %s", name);
    SYM(create, "hiprtcCreateProgram")
    SYM(compile, "hiprtcCompileProgram")
    SYM(log_size, "hiprtcGetProgramLogSize")
    SYM(log, "hiprtcGetProgramLog")
    SYM(code_size, "hiprtcGetCodeSize")
    SYM(code, "hiprtcGetCode")
    SYM(destroy, "hiprtcDestroyProgram")
#undef SYM
    g_rtc.h = h;
    return CHGPU_OK;
}

const char * ctype(int t)
{
    switch (t)
    {
        case CHGPU_I64: return "i64";
        case CHGPU_U64: return "u64";
        case CHGPU_I32: return "i32";
        case CHGPU_U32: return "u32";
        case CHGPU_I16: return "i16";
        case CHGPU_U16: return "u16";
        case CHGPU_I8: return "i8";
        case CHGPU_U8: return "u8";
        case CHGPU_F64: return "f64";
        case CHGPU_F32: return "f32";
        default: return nullptr;
    }
}

// NumberTraits::Construct<is_signed, is_floating, size> (NumberTraits.h:40-63); -1 = a type this path does not carry
int construct(bool sgn, bool flt, size_t size)
{
    if (flt)
        return size == 8 ? CHGPU_F64 : size == 4 ? CHGPU_F32 : -1;
    switch (size)
    {
        case 1: return sgn ? CHGPU_I8 : CHGPU_U8;
        case 2: return sgn ? CHGPU_I16 : CHGPU_U16;
        case 4: return sgn ? CHGPU_I32 : CHGPU_U32;
        case 8: return sgn ? CHGPU_I64 : CHGPU_U64;
        default: return -1;
    }
}
size_t next_size(size_t s) { return s < 8 ? s * 2 : s; } // NumberTraits.h:32-37
bool is_sgn(int t) { return chgpu_type_is_signed(t) || chgpu_type_is_float(t); } // is_signed_v<Float> is true

// ---- the functions: one row each, or one per family whose members differ in an operator only ----
struct FnRow;
struct Operands
{
    int rt;           // result type
    int t[3];         // operand types
    std::string n[3]; // operand names (n<node>)
};
typedef int (*TypeRule)(const FnRow & f, int fn, int a, int b, int c); // result type over the operand types; -1 = not carried / illegal
typedef std::string (*Emitter)(const Operands & x);
typedef const char * (*Gate)(const chgpu_expr_node * nodes, const chgpu_expr_node & nd, const int * at); // nullptr: compile it; else why not

struct FnRow
{
    int code, n_codes;       // the codes [code, code + n_codes)
    int arity;
    TypeRule type;
    int result;              // the rules with a fixed result: that type
    const char * text;       // right-hand side: $0 $1 $2 the operands, $W0 $W1 the operands widened for the comparison helpers, $T the result's C type
    const char * text_float; // the same for a Float result, where it differs
    Emitter emit;            // in place of text
    Gate gate;               // compile-time condition beyond the types
};

// every operand is a type -> the row's result
int ty_fixed(const FnRow & f, int, int a, int b, int)
{
    return chgpu_type_size(a) && (f.arity < 2 || chgpu_type_size(b)) ? f.result : -1;
}
int ty_date(const FnRow & f, int, int a, int, int) { return a == CHGPU_U16 ? f.result : -1; } // a Date is its day number
bool both_int(int a, int b) { return chgpu_type_is_int(a) && chgpu_type_is_int(b); }
int ty_add_mul(const FnRow &, int, int a, int b, int) // ResultOfAdditionMultiplication
{
    const size_t sa = chgpu_type_size(a), sb = chgpu_type_size(b);
    return (sa && sb) ? construct(is_sgn(a) || is_sgn(b), chgpu_type_is_float(a) || chgpu_type_is_float(b), next_size(sa > sb ? sa : sb)) : -1;
}
int ty_minus(const FnRow &, int, int a, int b, int) // ResultOfSubtraction
{
    const size_t sa = chgpu_type_size(a), sb = chgpu_type_size(b);
    return (sa && sb) ? construct(true, chgpu_type_is_float(a) || chgpu_type_is_float(b), next_size(sa > sb ? sa : sb)) : -1;
}
int ty_negate(const FnRow &, int, int a, int, int) // ResultOfNegate
{
    const size_t sa = chgpu_type_size(a);
    return sa ? construct(true, chgpu_type_is_float(a), is_sgn(a) ? sa : next_size(sa)) : -1;
}
int ty_bit(const FnRow &, int, int a, int b, int) // ResultOfBit, integers only here
{
    return both_int(a, b) ? construct(is_sgn(a) || is_sgn(b), false, std::max(chgpu_type_size(a), chgpu_type_size(b))) : -1;
}
int ty_int_div(const FnRow &, int, int a, int b, int) // ResultOfIntegerDivision; integers only here (the float forms throw on NaN / infinities)
{
    return both_int(a, b) ? construct(is_sgn(a) || is_sgn(b), false, chgpu_type_size(a)) : -1;
}
int ty_modulo(const FnRow &, int, int a, int b, int) // ResultOfModulo; integers only here
{
    return both_int(a, b) ? construct(is_sgn(a), false, is_sgn(a) ? next_size(chgpu_type_size(b)) : chgpu_type_size(b)) : -1;
}
int ty_if(const FnRow &, int, int a, int b, int c) // ResultOfIf (NumberTraits.h:159-199) for the branches b, c; condition a is an integer
{
    const size_t sb = chgpu_type_size(b), sc = chgpu_type_size(c);
    if (!chgpu_type_is_int(a) || !sb || !sc)
        return -1;
    if (b == c)
        return b;
    const bool fb = chgpu_type_is_float(b), fc = chgpu_type_is_float(c);
    const bool has_float = fb || fc, has_integer = !fb || !fc, has_signed = is_sgn(b) || is_sgn(c), has_unsigned = !is_sgn(b) || !is_sgn(c);
    const size_t max_u = std::max(is_sgn(b) ? (size_t)0 : sb, is_sgn(c) ? (size_t)0 : sc);
    const size_t max_s = std::max(is_sgn(b) ? sb : (size_t)0, is_sgn(c) ? sc : (size_t)0);
    const size_t max_i = std::max(fb ? (size_t)0 : sb, fc ? (size_t)0 : sc);
    const size_t max_f = std::max(fb ? sb : (size_t)0, fc ? sc : (size_t)0);
    const size_t m = std::max(sb, sc);
    const bool dbl = (has_float && has_integer && max_i >= max_f) || (has_signed && has_unsigned && max_u >= max_s);
    return construct(has_signed, has_float, dbl ? m * 2 : m); // UInt64 with Int<x>, Float<x> with [U]Int64 -> size 16 -> -1 (Error)
}
int ty_cast(const FnRow & f, int fn, int a, int, int)
{
    const int to = fn - f.code;
    if (!chgpu_type_size(a) || !chgpu_type_size(to))
        return -1;
    if (chgpu_type_is_float(a) && !chgpu_type_is_float(to))
        return -1; // Float -> integer: out-of-range values are target-defined in the reference (x86 cvttsd2si); not carried
    return to;
}

// intDiv / modulo throw ILLEGAL_DIVISION on a zero divisor and on min / -1 (throwIfDivisionLeadsToFPE, DivisionUtils.h:15-26): a
// kernel cannot throw per row, so only constant divisors that can never throw are compiled; everything else stays on the CPU.
const char * const NO_SAFE_DIVISOR = "intDiv / modulo need a constant integer divisor that cannot raise ILLEGAL_DIVISION";
// a constant, nonzero integer divisor of an integer: its bits and the all-ones mask of its width
bool constant_divisor(const chgpu_expr_node * nodes, const chgpu_expr_node & nd, const int * at, u64 * bits, u64 * mask)
{
    const chgpu_expr_node & dn = nodes[nd.args[1]];
    if (dn.kind != CHGPU_EX_CONST || !both_int(at[0], at[1]))
        return false;
    const size_t sb = chgpu_type_size(at[1]);
    *mask = sb == 8 ? ~0ull : ((1ull << (8 * sb)) - 1);
    *bits = dn.bits & *mask;
    return *bits != 0; // division by zero
}
const char * gate_int_div(const chgpu_expr_node * nodes, const chgpu_expr_node & nd, const int * at)
{
    u64 bits = 0, mask = 0;
    if (!constant_divisor(nodes, nd, at, &bits, &mask))
        return NO_SAFE_DIVISOR;
    // all-ones divisor: -1 once it is (or is cast to) a signed type of its own width -- min / -1 would throw
    const bool cast_to_signed = chgpu_type_is_signed(at[0]) && chgpu_type_size(at[0]) <= chgpu_type_size(at[1]);
    return bits == mask && (chgpu_type_is_signed(at[1]) || cast_to_signed) ? NO_SAFE_DIVISOR : nullptr;
}
const char * gate_modulo(const chgpu_expr_node * nodes, const chgpu_expr_node & nd, const int * at)
{
    u64 bits = 0, mask = 0;
    if (!constant_divisor(nodes, nd, at, &bits, &mask))
        return NO_SAFE_DIVISOR;
    if (!chgpu_type_is_signed(at[1]))
        return nullptr;
    // all-ones: -1, min % -1 would throw.  The most negative value of a signed divisor type: the reference's constant-divisor path
    // (ModuloByConstantImpl::vectorConstant, src/Functions/modulo.cpp:56-80) throws ILLEGAL_DIVISION "Division by the most negative number"
    // where ModuloImpl::apply would compute a % b -- e.g. Int64 % toInt64(-9223372036854775808), Int32 % toInt8(-128).  Refused for every
    // operand pair (a superset).  (intDiv by that constant does not throw: DivideIntegralByConstantImpl, src/Functions/intDiv.cpp:55-78)
    return bits == mask || bits == (mask >> 1) + 1 ? NO_SAFE_DIVISOR : nullptr;
}

// the operand widened without loss to the 64-bit class the exact comparison helpers take
std::string wide(int t, const std::string & e)
{
    if (chgpu_type_is_float(t))
        return "(f64)" + e;
    return (chgpu_type_is_signed(t) ? "(i64)" : "(u64)") + e;
}

std::string subst(const std::string & text, const Operands & x)
{
    std::string s;
    for (size_t i = 0; i < text.size(); ++i)
    {
        if (text[i] != '$')
            s += text[i];
        else if (text[++i] == 'T')
            s += ctype(x.rt);
        else if (text[i] == 'W')
        {
            ++i;
            s += wide(x.t[text[i] - '0'], x.n[text[i] - '0']);
        }
        else
            s += x.n[text[i] - '0'];
    }
    return s;
}

// DivideIntegralImpl::apply (src/Functions/DivisionUtils.h:66-105).  The operands keep their exact C types, so the division is
// performed in the same promoted type as on the host (usual arithmetic conversions, LP64).
std::string emit_int_div(const Operands & x)
{
    const int ta = x.t[0], tb = x.t[1];
    if (!chgpu_type_is_signed(ta) && !chgpu_type_is_signed(tb))
        return subst("($T)($0 / $1)", x);
    const int sa_t = construct(true, false, chgpu_type_size(ta));
    const int sb_t = chgpu_type_size(ta) <= chgpu_type_size(tb) ? construct(true, false, chgpu_type_size(tb)) : sa_t;
    return subst(std::string("($T)((") + ctype(sa_t) + ")$0 / (" + ctype(sb_t) + ")$1)", x);
}

const FnRow FUNCTIONS[] = {
    // accurate::equalsOp / lessOp (AccurateComparison.h:20-204) on the widened operands
    {CHGPU_FN_EQUALS, 1, 2, ty_fixed, CHGPU_U8, "(u8)(eq_($W0, $W1))"},
    {CHGPU_FN_NOT_EQUALS, 1, 2, ty_fixed, CHGPU_U8, "(u8)(!eq_($W0, $W1))"},
    {CHGPU_FN_LESS, 1, 2, ty_fixed, CHGPU_U8, "(u8)(lt_($W0, $W1))"},
    {CHGPU_FN_GREATER, 1, 2, ty_fixed, CHGPU_U8, "(u8)(lt_($W1, $W0))"},
    {CHGPU_FN_LESS_OR_EQUALS, 1, 2, ty_fixed, CHGPU_U8, "(u8)(le_($W0, $W1))"},
    {CHGPU_FN_GREATER_OR_EQUALS, 1, 2, ty_fixed, CHGPU_U8, "(u8)(ge_($W0, $W1))"},
    // FunctionBinaryArithmetic.h, `static_cast<Result>(a) OP b`.  An integer result type holds both operands: two's complement
    // arithmetic in 64 bits, truncated, is exact.  A Float result is always Float64: nextSize of a >= 4-byte operand.
    {CHGPU_FN_PLUS, 1, 2, ty_add_mul, -1, "($T)((u64)$0 + (u64)$1)", "(f64)$0 + (f64)$1"},
    {CHGPU_FN_MINUS, 1, 2, ty_minus, -1, "($T)((u64)$0 - (u64)$1)", "(f64)$0 - (f64)$1"},
    {CHGPU_FN_MULTIPLY, 1, 2, ty_add_mul, -1, "($T)((u64)$0 * (u64)$1)", "(f64)$0 * (f64)$1"},
    {CHGPU_FN_DIVIDE, 1, 2, ty_fixed, CHGPU_F64, "(f64)$0 / (f64)$1"}, // ResultOfFloatingPointDivision
    {CHGPU_FN_NEGATE, 1, 1, ty_negate, -1, "($T)(0ull - (u64)$0)", "-$0"},
    {CHGPU_FN_INT_DIV, 1, 2, ty_int_div, -1, nullptr, nullptr, emit_int_div, gate_int_div},
    // ModuloImpl::apply (DivisionUtils.h:126-170): IntegerAType(a) % IntegerBType(b), then the cast
    {CHGPU_FN_MODULO, 1, 2, ty_modulo, -1, "($T)($0 % $1)", nullptr, nullptr, gate_modulo},
    // FunctionsLogical.h:82-140 on static_cast<bool>
    {CHGPU_FN_AND, 1, 2, ty_fixed, CHGPU_U8, "(u8)(($0 != 0) & ($1 != 0))"},
    {CHGPU_FN_OR, 1, 2, ty_fixed, CHGPU_U8, "(u8)(($0 != 0) | ($1 != 0))"},
    {CHGPU_FN_XOR, 1, 2, ty_fixed, CHGPU_U8, "(u8)(($0 != 0) ^ ($1 != 0))"},
    {CHGPU_FN_NOT, 1, 1, ty_fixed, CHGPU_U8, "(u8)!($0 != 0)"},
    {CHGPU_FN_IF, 1, 3, ty_if, -1, "($0 != 0) ? ($T)$1 : ($T)$2"},
    {CHGPU_FN_BIT_AND, 1, 2, ty_bit, -1, "($T)((u64)$0 & (u64)$1)"},
    {CHGPU_FN_BIT_OR, 1, 2, ty_bit, -1, "($T)((u64)$0 | (u64)$1)"},
    {CHGPU_FN_BIT_XOR, 1, 2, ty_bit, -1, "($T)((u64)$0 ^ (u64)$1)"},
    // DateTimeTransforms.h ToYearImpl ... over DayNum: the argument is a Date
    {CHGPU_FN_TO_YEAR, 1, 1, ty_date, CHGPU_U16, "(u16)civil_($0).y"},
    {CHGPU_FN_TO_MONTH, 1, 1, ty_date, CHGPU_U8, "(u8)civil_($0).m"},
    {CHGPU_FN_TO_DAY_OF_MONTH, 1, 1, ty_date, CHGPU_U8, "(u8)civil_($0).d"},
    {CHGPU_FN_TO_YYYYMM, 1, 1, ty_date, CHGPU_U32, "(u32)(civil_($0).y * 100u + civil_($0).m)"},
    {CHGPU_FN_TO_YYYYMMDD, 1, 1, ty_date, CHGPU_U32, "(u32)(civil_($0).y * 10000u + civil_($0).m * 100u + civil_($0).d)"},
    {CHGPU_FN_TO_DAY_OF_WEEK, 1, 1, ty_date, CHGPU_U8, "(u8)(((u32)$0 + 3u) % 7u + 1u)"}, // ToDayOfWeekImpl, mode 0: Monday = 1 ... Sunday = 7; 1970-01-01 was a Thursday
    {CHGPU_FN_TO_QUARTER, 1, 1, ty_date, CHGPU_U8, "(u8)((civil_($0).m - 1u) / 3u + 1u)"},
    {CHGPU_FN_TO_START_OF_MONTH, 1, 1, ty_date, CHGPU_U16, "(u16)((u32)$0 - (civil_($0).d - 1u))"}, // a Date again
    {CHGPU_FN_CAST, 16, 1, ty_cast, -1, "($T)$0"}, // CHGPU_FN_CAST + target type
};

const FnRow * fn_row(int fn)
{
    for (const FnRow & f : FUNCTIONS)
        if (fn >= f.code && fn < f.code + f.n_codes)
            return &f;
    return nullptr;
}

const char * PRELUDE = R"SRC(
typedef unsigned long long u64; typedef long long i64; typedef unsigned int u32; typedef int i32;
typedef unsigned short u16; typedef short i16; typedef unsigned char u8; typedef signed char i8;
typedef float f32; typedef double f64;
#define DEV static __device__ __forceinline__
// accurate::lessOp / equalsOp (AccurateComparison.h:20-204) on operands widened to i64 / u64 / f64: mathematically exact
DEV bool nan_(i64) { return false; }
DEV bool nan_(u64) { return false; }
DEV bool nan_(f64 x) { return x != x; }
DEV bool lt_(i64 a, i64 b) { return a < b; }
DEV bool lt_(u64 a, u64 b) { return a < b; }
DEV bool lt_(f64 a, f64 b) { return a < b; }
DEV bool lt_(i64 a, u64 b) { return a < 0 || (u64)a < b; }
DEV bool lt_(u64 a, i64 b) { return b >= 0 && a < (u64)b; }
DEV bool lt_(i64 a, f64 b)
{
    if (b != b) return false;
    if (b >= 9223372036854775808.0) return true;
    if (b < -9223372036854775808.0) return false;
    const i64 t = (i64)b; // truncation, exact in range
    if (a != t) return a < t;
    return b - (f64)t > 0;
}
DEV bool lt_(f64 a, i64 b)
{
    if (a != a) return false;
    if (a >= 9223372036854775808.0) return false;
    if (a < -9223372036854775808.0) return true;
    const i64 t = (i64)a;
    if (t != b) return t < b;
    return a - (f64)t < 0;
}
DEV bool lt_(u64 a, f64 b)
{
    if (b != b) return false;
    if (b >= 18446744073709551616.0) return true;
    if (b <= 0) return false;
    const u64 t = (u64)b;
    if (a != t) return a < t;
    return b - (f64)t > 0;
}
DEV bool lt_(f64 a, u64 b)
{
    if (a != a) return false;
    if (a >= 18446744073709551616.0) return false;
    if (a < 0) return true;
    const u64 t = (u64)a;
    if (t != b) return t < b;
    return a - (f64)t < 0;
}
DEV bool eq_(i64 a, i64 b) { return a == b; }
DEV bool eq_(u64 a, u64 b) { return a == b; }
DEV bool eq_(f64 a, f64 b) { return a == b; }
DEV bool eq_(i64 a, u64 b) { return a >= 0 && (u64)a == b; }
DEV bool eq_(u64 a, i64 b) { return b >= 0 && a == (u64)b; }
DEV bool eq_(i64 a, f64 b)
{
    if (!(b >= -9223372036854775808.0 && b < 9223372036854775808.0)) return false;
    const i64 t = (i64)b;
    return t == a && (f64)t == b;
}
DEV bool eq_(f64 a, i64 b) { return eq_(b, a); }
DEV bool eq_(u64 a, f64 b)
{
    if (!(b >= 0 && b < 18446744073709551616.0)) return false;
    const u64 t = (u64)b;
    return t == a && (f64)t == b;
}
DEV bool eq_(f64 a, u64 b) { return eq_(b, a); }
template <typename A, typename B> DEV bool le_(A a, B b) { return !nan_(a) && !nan_(b) && !lt_(b, a); }
template <typename A, typename B> DEV bool ge_(A a, B b) { return !nan_(a) && !nan_(b) && !lt_(a, b); }
// DayNum -> civil date (proleptic Gregorian; what DateLUTImpl's day table holds for DayNum, Common/DateLUTImpl.h)
struct Civil { u32 y, m, d; };
DEV Civil civil_(u32 days)
{
    const u32 z = days + 719468u;
    const u32 era = z / 146097u;
    const u32 doe = z - era * 146097u;
    const u32 yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;
    const u32 doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);
    const u32 mp = (5u * doy + 2u) / 153u;
    Civil c;
    c.d = doy - (153u * mp + 2u) / 5u + 1u;
    c.m = mp < 10u ? mp + 3u : mp - 9u;
    c.y = yoe + era * 400u + (c.m <= 2u ? 1u : 0u);
    return c;
}
)SRC";

} // namespace

struct chgpu_expr
{
    std::vector<chgpu_expr_node> nodes;
    std::vector<int> types;       // resolved type of every node
    std::vector<int> input_types; // type of cols[j] (from the INPUT nodes), -1 = unused slot
    std::string body;             // statements computing n0..nK from `r`
};


namespace
{

int build_body(chgpu_expr * e)
{
    std::string s;
    char buf[256];
    for (size_t k = 0; k < e->nodes.size(); ++k)
    {
        const chgpu_expr_node & nd = e->nodes[k];
        const int t = e->types[k];
        const char * ct = ctype(t);
        std::string rhs;
        if (nd.kind == CHGPU_EX_INPUT)
            rhs = "r.c" + std::to_string(nd.code);
        else if (nd.kind == CHGPU_EX_CONST)
        {
            if (t == CHGPU_F64)
                snprintf(buf, sizeof(buf), "__longlong_as_double((long long)0x%llxull)", (unsigned long long)nd.bits);
            else if (t == CHGPU_F32)
                snprintf(buf, sizeof(buf), "__uint_as_float(0x%xu)", (unsigned)(nd.bits & 0xffffffffu));
            else
                snprintf(buf, sizeof(buf), "(%s)0x%llxull", ct, (unsigned long long)nd.bits);
            rhs = buf;
        }
        else
        {
            const FnRow & f = *fn_row(nd.code); // a code without a row got no type and never comes here
            Operands x;
            x.rt = t;
            for (int j = 0; j < f.arity; ++j)
            {
                x.t[j] = e->types[nd.args[j]];
                x.n[j] = "n" + std::to_string(nd.args[j]);
            }
            rhs = f.emit ? f.emit(x) : subst(f.text_float && chgpu_type_is_float(t) ? f.text_float : f.text, x);
        }
        s += std::string("    const ") + ct + " n" + std::to_string(k) + " = " + rhs + ";\n";
    }
    e->body = s;
    return CHGPU_OK;
}

// rows per lane and vector: 16-byte loads of the widest column, at least 4 bytes of the narrowest
u32 vec_rows(const std::vector<int> & types)
{
    size_t wmax = 1, wmin = 8;
    for (int t : types)
    {
        const size_t w = chgpu_type_size(t);
        wmax = std::max(wmax, w);
        wmin = std::min(wmin, w);
    }
    u32 v = (u32)std::max((size_t)16 / wmax, (size_t)4 / wmin);
    return v < 1 ? 1 : v > 16 ? 16 : v;
}

enum Form
{
    FORM_MAP,       // k_run: DAG nodes -> materialised columns
    FORM_SUM,       // k_run + k_fin: WHERE <node> + sum(<node>), count()
    FORM_WHERE_MAP, // k_fcount + k_femit: WHERE <node> + the surviving rows of DAG nodes
};

struct KernelSpec
{
    Form form = FORM_MAP;
    std::vector<u32> out_nodes; // map, WHERE + projection
    int filter_node = -1;       // sum (-1: every row), WHERE + projection
    int value_node = -1;        // sum (-1: count only)
    u32 vec = 1;                // map, sum: rows per lane and vector
};

static int jit_env(const chgpu_ctx * ctx, const char * name, int dflt) { return (int)chgpu_opt(ctx, name, dflt); } // developer knobs (chgpu_ctx_set_option)
// vectors in flight per lane and column / workgroups per CU: developer overrides for A/B runs (CHGPU_TUNE_JIT_UNROLL, _WG_MAP, _WG_SUM)
// (the source generator has no context: the process-wide default, chgpu_ctx_set_option(NULL, ...), fixed at the first compilation)
static int jit_unroll()
{
    static const int v = jit_env(nullptr, "tune_jit_unroll", 4);
    return v;
}
#define JIT_UNROLL jit_unroll()
constexpr u32 JIT_MAX_COLS = 8;

struct JitArgs
{
    const void * in[JIT_MAX_COLS];
    void * out[JIT_MAX_COLS];
    u64 n;
    u64 * part; // per-workgroup partials of the reductions; WHERE + projection: the chunk counts, then their offsets
    u32 n_parts;
    u32 pad;
};
// the same struct as the generated program declares it
const char * const ARGS_DECL = "struct Args { const void * in[8]; void * out[8]; u64 n; u64 * part; u32 n_parts; u32 pad; };\n";
static_assert(JIT_MAX_COLS == 8 && sizeof(JitArgs) == 2 * 8 * 8 + 8 + 8 + 4 + 4, "ARGS_DECL restates JitArgs");

// ---- the frame of every generated program ----
struct ResField
{
    std::string type, name, value; // a field of Res and the expression eval() assigns to it
};

std::vector<ResField> out_fields(const chgpu_expr * e, const std::vector<u32> & out_nodes)
{
    std::vector<ResField> fields;
    for (size_t o = 0; o < out_nodes.size(); ++o)
        fields.push_back({ctype(e->types[out_nodes[o]]), "o" + std::to_string(o), "n" + std::to_string(out_nodes[o])});
    return fields;
}

// prelude, `decls`, Args, Row (a field per input column), Res (`keep` for the forms with a WHERE, then `fields`) and eval(): the DAG's
// statements, then the assignments to Res.  filter_node -1: every row is kept.
std::string gen_frame(const chgpu_expr * e, const std::string & decls, bool keep, int filter_node, const std::vector<ResField> & fields)
{
    std::string s = PRELUDE + decls + ARGS_DECL + "struct Row {";
    for (size_t j = 0; j < e->input_types.size(); ++j)
        if (e->input_types[j] >= 0)
            s += std::string(" ") + ctype(e->input_types[j]) + " c" + std::to_string(j) + ";";
    s += " };\nstruct Res {";
    if (keep)
        s += " bool keep;";
    for (const ResField & f : fields)
        s += " " + f.type + " " + f.name + ";";
    s += " };\nDEV void eval(const Row & r, Res & o)\n{\n" + e->body;
    if (keep)
        s += filter_node >= 0 ? "    o.keep = n" + std::to_string(filter_node) + " != 0;\n" : std::string("    o.keep = true;\n");
    for (const ResField & f : fields)
        s += "    o." + f.name + " = " + f.value + ";\n";
    return s + "}\n";
}

// `Row r` filled from row `index` of the input columns
std::string row_load(const chgpu_expr * e, const std::string & indent, const std::string & index)
{
    std::string s;
    for (size_t j = 0; j < e->input_types.size(); ++j)
        if (e->input_types[j] >= 0)
            s += indent + "r.c" + std::to_string(j) + " = ((const " + ctype(e->input_types[j]) + " *)a.in[" + std::to_string(j) + "])[" + index + "];\n";
    return s;
}

std::string out_store(const std::string & indent, const std::string & type, size_t o, const std::string & index, const std::string & value)
{
    return indent + "((" + type + " *)a.out[" + std::to_string(o) + "])[" + index + "] = " + value + ";\n";
}

std::string gen_source(const chgpu_expr * e, const KernelSpec & ks)
{
    const bool fsum = ks.form == FORM_SUM;
    const u32 V = ks.vec;
    auto vtype = [&](int t) { return std::string("v") + ctype(t) + "_t"; };
    auto otype = [&](size_t o) { return e->types[ks.out_nodes[o]]; };
    const size_t n_out = ks.out_nodes.size(); // 0 for the sum
    std::string vdefs; // vector typedefs for every element type
    for (int t = 0; t <= CHGPU_F32; ++t)
        vdefs += std::string("typedef ") + ctype(t) + " " + vtype(t) + " __attribute__((ext_vector_type(" + std::to_string(V) + ")));\n";
    std::vector<ResField> fields = out_fields(e, ks.out_nodes);
    if (fsum && ks.value_node >= 0)
        fields.push_back({ctype(e->types[ks.value_node]), "val", "n" + std::to_string(ks.value_node)});
    std::string s = gen_frame(e, vdefs, fsum, ks.filter_node, fields);

    const bool facc = fsum && ks.value_node >= 0 && chgpu_type_is_float(e->types[ks.value_node]);
    // the sum's statements per evaluated row
    auto accumulate = [&](const std::string & indent) {
        std::string t;
        if (ks.value_node >= 0)
            t += indent + (facc ? "acc += o.keep ? (f64)o.val : 0.0;\n" : "acc += o.keep ? (u64)o.val : 0ull;\n");
        return t + indent + "cnt += o.keep ? 1u : 0u;\n";
    };
    const std::string U = std::to_string(JIT_UNROLL), VS = std::to_string(V);
    s += "extern \"C\" __global__ __launch_bounds__(256) void k_run(Args a)\n{\n";
    if (fsum)
        s += facc ? "    f64 acc = 0; u64 cnt = 0;\n" : "    u64 acc = 0; u64 cnt = 0;\n";
    s += "    const u64 nvec = a.n / " + VS + ";\n    constexpr u64 CH = 256ull * " + U + ";\n    const u64 nch = nvec / CH;\n";
    // every wave owns a contiguous strip of U * 64 vectors of the chunk.  One-byte outputs (masks) whose V * U bytes per lane make 16
    // are transposed through a wave-private LDS strip so that each lane stores 16 CONTIGUOUS bytes once per chunk instead of U
    // narrow vectors (k_cmp_mask's scheme: the 4-byte stores cost the generated mask kernel 0.57 of peak against 0.72).
    const bool tr_ok = !fsum && V * (u32)JIT_UNROLL == 16;
    std::vector<int> tr_slot(n_out, -1);
    int n_tr = 0;
    if (tr_ok)
        for (size_t o = 0; o < n_out; ++o)
            if (chgpu_type_size(otype(o)) == 1)
                tr_slot[o] = n_tr++;
    if (n_tr)
        s += "    typedef u8 v16b_t __attribute__((ext_vector_type(16)));\n    __shared__ __attribute__((aligned(16))) u8 tr[" + std::to_string(n_tr) + "][4][1024];\n";
    s += "    for (u64 ch = blockIdx.x; ch < nch; ch += gridDim.x)\n    {\n        const u64 sb = ch * CH + (u64)(threadIdx.x >> 6) * (64 * " + U +
         ");\n        const u64 vb = sb + (threadIdx.x & 63);\n";
    for (size_t j = 0; j < e->input_types.size(); ++j)
        if (e->input_types[j] >= 0)
        {
            const std::string vt = vtype(e->input_types[j]), J = std::to_string(j);
            s += "        " + vt + " x" + J + "[" + U + "];\n";
            s += "#pragma unroll\n        for (int k = 0; k < " + U + "; ++k) x" + J + "[k] = __builtin_nontemporal_load((const " + vt + " *)a.in[" + J + "] + vb + (u64)k * 64);\n";
        }
    s += "#pragma unroll\n        for (int k = 0; k < " + U + "; ++k)\n        {\n";
    for (size_t o = 0; o < n_out; ++o)
        s += "            " + vtype(otype(o)) + " y" + std::to_string(o) + ";\n";
    s += "#pragma unroll\n            for (int q = 0; q < " + VS + "; ++q)\n            {\n                Row r; Res o;\n";
    for (size_t j = 0; j < e->input_types.size(); ++j) // from the vectors already loaded, not from memory
        if (e->input_types[j] >= 0)
            s += "                r.c" + std::to_string(j) + " = x" + std::to_string(j) + "[k][q];\n";
    s += "                eval(r, o);\n";
    if (fsum)
        s += accumulate("                ");
    for (size_t o = 0; o < n_out; ++o)
        s += "                y" + std::to_string(o) + "[q] = o.o" + std::to_string(o) + ";\n";
    s += "            }\n";
    for (size_t o = 0; o < n_out; ++o)
    {
        if (tr_slot[o] >= 0)
            s += "            *(" + vtype(otype(o)) + " *)&tr[" + std::to_string(tr_slot[o]) + "][threadIdx.x >> 6][(k * 64 + (threadIdx.x & 63)) * " + VS +
                 "] = y" + std::to_string(o) + ";\n";
        else
            s += out_store("            ", vtype(otype(o)), o, "vb + (u64)k * 64", "y" + std::to_string(o));
    }
    s += "        }\n";
    if (n_tr)
    {
        s += "        __builtin_amdgcn_wave_barrier();\n"; // LDS operations of one wave complete in order
        for (size_t o = 0; o < n_out; ++o)
            if (tr_slot[o] >= 0)
                s += "        *((v16b_t *)((u8 *)a.out[" + std::to_string(o) + "] + sb * " + VS + ") + (threadIdx.x & 63)) = *(const v16b_t *)&tr[" +
                     std::to_string(tr_slot[o]) + "][threadIdx.x >> 6][(threadIdx.x & 63) * 16];\n";
        s += "        __builtin_amdgcn_wave_barrier();\n";
    }
    s += "    }\n";
    // ragged tail, one row per lane
    s += "    for (u64 i = nch * CH * " + VS + " + (u64)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (u64)gridDim.x * 256)\n    {\n        Row r; Res o;\n";
    s += row_load(e, "        ", "i") + "        eval(r, o);\n";
    if (fsum)
        s += accumulate("        ");
    for (size_t o = 0; o < n_out; ++o)
        s += out_store("        ", ctype(otype(o)), o, "i", "o.o" + std::to_string(o));
    s += "    }\n";
    if (fsum)
    {
        // wave64 shuffle reduce -> LDS -> one partial per workgroup; k_fin adds the partials in a fixed order
        s += R"SRC(
    __shared__ u64 sh_a[4], sh_c[4];
    u64 ab = ACC_BITS(acc);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
    {
        const u64 oa = ((u64)__shfl_down((u32)(ab >> 32), d, 64) << 32) | __shfl_down((u32)ab, d, 64);
        const u64 oc = ((u64)__shfl_down((u32)(cnt >> 32), d, 64) << 32) | __shfl_down((u32)cnt, d, 64);
        ab = ACC_ADD(ab, oa);
        cnt += oc;
    }
    if ((threadIdx.x & 63) == 0) { sh_a[threadIdx.x >> 6] = ab; sh_c[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        u64 ta = sh_a[0], tc = sh_c[0];
        for (int w = 1; w < 4; ++w) { ta = ACC_ADD(ta, sh_a[w]); tc += sh_c[w]; }
        a.part[2 * blockIdx.x] = ta;
        a.part[2 * blockIdx.x + 1] = tc;
    }
}
extern "C" __global__ __launch_bounds__(64) void k_fin(Args a)
{
    if (threadIdx.x != 0) return;
    u64 ta = ACC_ZERO, tc = 0;
    for (u32 p = 0; p < a.n_parts; ++p) { ta = ACC_ADD(ta, a.part[2 * p]); tc += a.part[2 * p + 1]; }
    a.part[2 * a.n_parts] = ta;
    a.part[2 * a.n_parts + 1] = tc;
}
)SRC";
        const std::string defs = facc ? "#define ACC_BITS(x) ((u64)__double_as_longlong(x))\n#define ACC_ADD(x, y) ((u64)__double_as_longlong(__longlong_as_double((long long)(x)) + __longlong_as_double((long long)(y))))\n#define ACC_ZERO 0ull\n"
                                      : "#define ACC_BITS(x) (x)\n#define ACC_ADD(x, y) ((x) + (y))\n#define ACC_ZERO 0ull\n";
        s = defs + s;
    }
    else
        s += "}\n";
    return s;
}

// WHERE + projection in one step (FilterTransform behind an ExpressionTransform): k_fcount evaluates the filter node and counts
// the surviving rows of every 1024-row chunk (one wave per chunk, 64 consecutive rows per step); after the scan of the counts
// k_femit evaluates filter and outputs again and writes the survivors compacted, in order (rank inside a step from the wave
// ballot).  The inputs are read twice; no mask, no unfiltered intermediate column is ever written.
constexpr u32 FE_CHUNK = 1024;

std::string gen_filter_source(const chgpu_expr * e, const KernelSpec & ks)
{
    std::string s = gen_frame(e, "", true, ks.filter_node, out_fields(e, ks.out_nodes));
    const std::string load = row_load(e, "            ", "in ? i : 0");
    const std::string C = std::to_string(FE_CHUNK);
    // a.part: u32 counts[n_chunks] (k_fcount writes), then const u64 offsets[n_chunks] (k_femit reads)
    s += "extern \"C\" __global__ __launch_bounds__(256) void k_fcount(Args a)\n{\n"
         "    const u32 lane = threadIdx.x & 63;\n"
         "    const u64 n_chunks = (a.n + " + C + " - 1) / " + C + ";\n"
         "    for (u64 ch = ((u64)blockIdx.x * 256 + threadIdx.x) >> 6; ch < n_chunks; ch += ((u64)gridDim.x * 256) >> 6)\n    {\n"
         "        u32 cnt = 0;\n"
         "#pragma unroll 4\n"
         "        for (u32 st = 0; st < " + C + " / 64; ++st)\n        {\n"
         "            const u64 i = ch * " + C + " + st * 64 + lane;\n            const bool in = i < a.n;\n            Row r; Res o;\n" + load +
         "            eval(r, o);\n            cnt += (u32)__popcll(__ballot(in && o.keep));\n        }\n"
         "        if (lane == 0) ((u32 *)a.part)[ch] = cnt;\n    }\n}\n";
    s += "extern \"C\" __global__ __launch_bounds__(256) void k_femit(Args a)\n{\n"
         "    const u32 lane = threadIdx.x & 63;\n"
         "    const u64 n_chunks = (a.n + " + C + " - 1) / " + C + ";\n"
         "    const u64 * offsets = (const u64 *)a.part;\n"
         "    for (u64 ch = ((u64)blockIdx.x * 256 + threadIdx.x) >> 6; ch < n_chunks; ch += ((u64)gridDim.x * 256) >> 6)\n    {\n"
         "        u64 pos = offsets[ch];\n"
         "#pragma unroll 4\n"
         "        for (u32 st = 0; st < " + C + " / 64; ++st)\n        {\n"
         "            const u64 i = ch * " + C + " + st * 64 + lane;\n            const bool in = i < a.n;\n            Row r; Res o;\n" + load +
         "            eval(r, o);\n            const bool keep = in && o.keep;\n            const u64 b = __ballot(keep);\n"
         "            const u64 dst = pos + __builtin_amdgcn_mbcnt_hi((u32)(b >> 32), __builtin_amdgcn_mbcnt_lo((u32)b, 0u));\n"
         "            if (keep)\n            {\n";
    for (size_t o = 0; o < ks.out_nodes.size(); ++o)
        s += out_store("                ", ctype(e->types[ks.out_nodes[o]]), o, "dst", "o.o" + std::to_string(o));
    s += "            }\n            pos += (u64)__popcll(b);\n        }\n    }\n}\n";
    return s;
}

// min(value), max(value), count() over the rows that pass the filter (executeWithoutKeyImpl with AggregateFunctionMin / Max,
// src/AggregateFunctions/AggregateFunctionMinMax.h; SingleValueDataFixed::setIfSmaller / setIfGreater) for INTEGER values: the value is
// widened to 64 bits and mapped to an order-preserving unsigned key, lanes keep a running (lowest, highest), waves reduce by shuffles.
// Float values are not carried: the reference keeps a NaN that arrives first (setIfSmaller compares with <), an order-dependent result.
std::string gen_minmax_source(const chgpu_expr * e, int filter_node, int value_node)
{
    const std::string v = "n" + std::to_string(value_node);
    const std::string key = chgpu_type_is_signed(e->types[value_node]) ? "(u64)(i64)" + v + " ^ 0x8000000000000000ull" : "(u64)" + v;
    std::string s = gen_frame(e, "", true, filter_node, {{"u64", "key", key}});
    s += R"SRC(
DEV u64 shfl_u64(u64 v, int d) { return ((u64)__shfl_down((u32)(v >> 32), d, 64) << 32) | __shfl_down((u32)v, d, 64); }
extern "C" __global__ __launch_bounds__(256) void k_mm(Args a)
{
    u64 lo = ~0ull, hi = 0ull, cnt = 0;
    const u64 stride = (u64)gridDim.x * 256;
    for (u64 i0 = (u64)blockIdx.x * 256 + threadIdx.x; i0 < a.n; i0 += stride * 4)
    {
#pragma unroll
        for (int q = 0; q < 4; ++q)
        {
            const u64 i = i0 + (u64)q * stride;
            const bool in = i < a.n;
            Row r; Res o;
)SRC" + row_load(e, "            ", "in ? i : 0") + R"SRC(
            eval(r, o);
            if (in && o.keep) { lo = o.key < lo ? o.key : lo; hi = o.key > hi ? o.key : hi; ++cnt; }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
    {
        const u64 l2 = shfl_u64(lo, d), h2 = shfl_u64(hi, d), c2 = shfl_u64(cnt, d);
        lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi; cnt += c2;
    }
    __shared__ u64 sl[4], sh[4], sc[4];
    if ((threadIdx.x & 63) == 0) { sl[threadIdx.x >> 6] = lo; sh[threadIdx.x >> 6] = hi; sc[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        for (int w = 1; w < 4; ++w) { lo = sl[w] < lo ? sl[w] : lo; hi = sh[w] > hi ? sh[w] : hi; cnt += sc[w]; }
        a.part[3 * blockIdx.x] = lo; a.part[3 * blockIdx.x + 1] = hi; a.part[3 * blockIdx.x + 2] = cnt;
    }
}
extern "C" __global__ __launch_bounds__(64) void k_mm_fin(Args a)
{
    if (threadIdx.x != 0) return;
    u64 lo = ~0ull, hi = 0ull, cnt = 0;
    for (u32 p = 0; p < a.n_parts; ++p)
    {
        const u64 l2 = a.part[3 * p], h2 = a.part[3 * p + 1];
        lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi; cnt += a.part[3 * p + 2];
    }
    a.part[3 * a.n_parts] = lo; a.part[3 * a.n_parts + 1] = hi; a.part[3 * a.n_parts + 2] = cnt;
}
)SRC";
    return s;
}

int jit_compile(const std::string & src, const std::vector<char> ** code_out)
{
    std::lock_guard<std::mutex> g(g_jit_mutex);
    auto it = g_code_cache.find(src);
    if (it == g_code_cache.end())
    {
        CHGPU_TRY(rtc_load());
        void * prog = nullptr;
        if (g_rtc.create(&prog, src.c_str(), "chgpu_expr.hip", 0, nullptr, nullptr) != 0)
            return chgpu_set_error(CHGPU_ERR_DEVICE, "hiprtcCreateProgram failed");
        const char * opts[] = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off"};
        const int rc = g_rtc.compile(prog, 3, opts);
        if (rc != 0)
        {
            size_t ls = 0;
            g_rtc.log_size(prog, &ls);
            std::string log(ls + 1, '\0');
            if (ls)
                g_rtc.log(prog, &log[0]);
            g_rtc.destroy(&prog);
            if (getenv("CHGPU_JIT_DUMP"))
                fprintf(stderr, "%s\n", src.c_str());
            return chgpu_set_error(CHGPU_ERR_LOGICAL, "hiprtc compile failed (%d): %.400s", rc, log.c_str());
        }
        size_t cs = 0;
        g_rtc.code_size(prog, &cs);
        std::vector<char> code(cs);
        g_rtc.code(prog, code.data());
        g_rtc.destroy(&prog);
        it = g_code_cache.emplace(src, std::move(code)).first;
    }
    *code_out = &it->second;
    return CHGPU_OK;
}

int jit_module(chgpu_ctx * ctx, const std::string & src, hipModule_t * mod)
{
    const std::vector<char> * code = nullptr;
    CHGPU_TRY(jit_compile(src, &code));
    std::lock_guard<std::mutex> g(g_jit_mutex);
    auto key = std::make_pair(ctx->device, src);
    auto it = g_module_cache.find(key);
    if (it == g_module_cache.end())
    {
        hipModule_t m = nullptr;
        CHGPU_HIP(hipModuleLoadData(&m, code->data()));
        it = g_module_cache.emplace(key, m).first;
    }
    *mod = it->second;
    return CHGPU_OK;
}

int check_spec(const chgpu_expr * e, uint32_t n_cols, const chgpu_col * const * cols, u64 * rows_out)
{
    CHGPU_REQUIRE(n_cols >= e->input_types.size(), CHGPU_ERR_BAD_ARGUMENTS, "expression reads column %zu, %u columns given", e->input_types.size() - 1, n_cols);
    u64 rows = 0;
    bool first = true;
    for (size_t j = 0; j < e->input_types.size(); ++j)
    {
        if (e->input_types[j] < 0)
            continue;
        CHGPU_REQUIRE(cols[j], CHGPU_ERR_BAD_ARGUMENTS, "column %zu is NULL", j);
        CHGPU_REQUIRE(cols[j]->type == e->input_types[j], CHGPU_ERR_BAD_ARGUMENTS, "column %zu has type %d, the expression was compiled for %d", j, cols[j]->type, e->input_types[j]);
        if (first)
            rows = cols[j]->rows, first = false;
        CHGPU_REQUIRE(cols[j]->rows == rows, CHGPU_ERR_SIZES_MISMATCH, "Sizes of columns doesn't match: %llu and %llu", (unsigned long long)cols[j]->rows, (unsigned long long)rows);
    }
    CHGPU_REQUIRE(!first, CHGPU_ERR_BAD_ARGUMENTS, "an expression without input columns has no row count");
    *rows_out = rows;
    return CHGPU_OK;
}

// FilterDescription's condition on the filter column; -1 = no WHERE, for the forms that have one without
int check_filter_node(const chgpu_expr * e, int filter_node, bool required)
{
    CHGPU_REQUIRE(filter_node < (int)e->types.size() && (filter_node >= 0 || !required), CHGPU_ERR_BAD_ARGUMENTS, "bad node");
    CHGPU_REQUIRE(filter_node < 0 || chgpu_type_is_int(e->types[filter_node]), CHGPU_ERR_BAD_ARGUMENTS,
                  "Illegal type for filter: the WHERE node must be an integer (FilterDescription.cpp:86-92)");
    return CHGPU_OK;
}

int make_spec(const chgpu_expr * e, Form form, uint32_t n_outputs, const uint32_t * out_nodes, int filter_node, int value_node, bool aligned, KernelSpec * ks)
{
    ks->form = form;
    std::vector<int> touched;
    for (int t : e->input_types)
        if (t >= 0)
            touched.push_back(t);
    if (form == FORM_SUM)
    {
        CHGPU_REQUIRE(value_node < (int)e->types.size(), CHGPU_ERR_BAD_ARGUMENTS, "bad node");
        ks->value_node = value_node;
    }
    else
    {
        const uint32_t most = form == FORM_WHERE_MAP ? JIT_MAX_COLS - 1 : JIT_MAX_COLS; // chgpu_expr_filter_execute takes 7
        CHGPU_REQUIRE(n_outputs > 0 && n_outputs <= most && out_nodes, CHGPU_ERR_BAD_ARGUMENTS, "1..%u outputs", most);
        for (uint32_t o = 0; o < n_outputs; ++o)
        {
            CHGPU_REQUIRE(out_nodes[o] < e->types.size(), CHGPU_ERR_BAD_ARGUMENTS, "bad output node");
            ks->out_nodes.push_back(out_nodes[o]);
            touched.push_back(e->types[out_nodes[o]]);
        }
    }
    if (form != FORM_MAP)
    {
        CHGPU_TRY(check_filter_node(e, filter_node, form == FORM_WHERE_MAP));
        ks->filter_node = filter_node;
    }
    ks->vec = aligned ? vec_rows(touched) : 1;
    return CHGPU_OK;
}

bool cols_aligned(const chgpu_expr * e, const chgpu_col * const * cols)
{
    for (size_t j = 0; j < e->input_types.size(); ++j)
        if (e->input_types[j] >= 0 && ((uintptr_t)cols[j]->data & 63) != 0)
            return false;
    return true;
}

// ---- the launch path ----
// the arguments with the input columns (checked by check_spec) and the row count in place
JitArgs bind_inputs(const chgpu_expr * e, const chgpu_col * const * cols, u64 rows)
{
    JitArgs a;
    memset(&a, 0, sizeof(a));
    for (size_t j = 0; j < e->input_types.size(); ++j)
        a.in[j] = e->input_types[j] >= 0 ? cols[j]->data : nullptr;
    a.n = rows;
    return a;
}

struct NamedFn
{
    const char * name;
    hipFunction_t * fn;
};
// the source's module on the context's device (compiled and loaded once per text) and its kernels by name
int jit_functions(chgpu_ctx * ctx, const std::string & src, std::initializer_list<NamedFn> fns)
{
    hipModule_t mod = nullptr;
    CHGPU_TRY(jit_module(ctx, src, &mod));
    for (const NamedFn & f : fns)
        CHGPU_HIP(hipModuleGetFunction(f.fn, mod, f.name));
    return CHGPU_OK;
}

int launch(chgpu_ctx * ctx, hipFunction_t fn, u32 grid, u32 block, JitArgs & a)
{
    void * params[] = {&a};
    CHGPU_HIP(hipModuleLaunchKernel(fn, grid, 1, 1, block, 1, 1, 0, ctx->stream, params, nullptr));
    return CHGPU_OK;
}

// work items of k_run, map and sum: one per `vec` rows of each of the JIT_UNROLL vectors a lane holds
u64 run_items(u64 rows, const KernelSpec & ks)
{
    return (rows + ks.vec * JIT_UNROLL - 1) / (ks.vec * JIT_UNROLL);
}

// A reduction to `words` u64: `kernel` leaves `words` per workgroup in the scratch, `fin` (one lane) folds them in a fixed order into
// the slot after the last workgroup's, which is read back.
int run_reduction(chgpu_ctx * ctx, const chgpu_expr * e, const chgpu_col * const * cols, u64 rows, const std::string & src, const char * kernel,
                  const char * fin, u64 items, int wg_per_cu, u32 words, u64 * res)
{
    hipFunction_t fn = nullptr, ffin = nullptr;
    CHGPU_TRY(jit_functions(ctx, src, {{kernel, &fn}, {fin, &ffin}}));
    const u32 grid = chgpu_grid_for(ctx, items, 256, wg_per_cu);
    void * scratch = nullptr;
    CHGPU_TRY(chgpu_scratch(ctx, ((size_t)grid + 1) * words * sizeof(u64), &scratch));
    JitArgs a = bind_inputs(e, cols, rows);
    a.part = (u64 *)scratch;
    a.n_parts = grid;
    CHGPU_TRY(launch(ctx, fn, grid, 256, a));
    CHGPU_TRY(launch(ctx, ffin, 1, 64, a));
    ctx->counters[6] += 2;
    return chgpu_read_back(ctx, a.part + (size_t)words * grid, res, words * sizeof(u64));
}

// The output columns of a call until the caller has them: whatever is still held when the call returns is freed.
struct OutCols
{
    std::vector<chgpu_col *> cols;
    ~OutCols()
    {
        for (chgpu_col * c : cols)
            chgpu_col_free(c);
    }
    // a new column of `rows` rows per output node, bound to a.out
    int alloc(chgpu_ctx * ctx, const chgpu_expr * e, const std::vector<u32> & out_nodes, u64 rows, JitArgs & a)
    {
        for (size_t o = 0; o < out_nodes.size(); ++o)
        {
            chgpu_col * c = nullptr;
            CHGPU_TRY(chgpu_col_new(ctx, e->types[out_nodes[o]], rows, &c));
            cols.push_back(c);
            a.out[o] = c->data;
        }
        return CHGPU_OK;
    }
    void hand_over(chgpu_col ** outs)
    {
        std::copy(cols.begin(), cols.end(), outs);
        cols.clear();
    }
};

} // namespace

extern "C" int chgpu_expr_compile(uint32_t n_nodes, const chgpu_expr_node * nodes, chgpu_expr ** out)
{
    CHGPU_REQUIRE(nodes && out && n_nodes > 0, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(n_nodes <= 256, CHGPU_ERR_NOT_IMPLEMENTED, "expression of %u nodes", n_nodes);
    chgpu_expr * e = new chgpu_expr;
    e->nodes.assign(nodes, nodes + n_nodes);
    e->types.assign(n_nodes, -1);
    int rc = CHGPU_OK;
    for (uint32_t k = 0; k < n_nodes && rc == CHGPU_OK; ++k)
    {
        const chgpu_expr_node & nd = nodes[k];
        if (nd.kind == CHGPU_EX_INPUT)
        {
            if (nd.code < 0 || (u32)nd.code >= JIT_MAX_COLS || !chgpu_type_size(nd.type))
                rc = chgpu_set_error(CHGPU_ERR_BAD_ARGUMENTS, "node %u: input column %d of type %d", k, nd.code, nd.type);
            else
            {
                if (e->input_types.size() <= (size_t)nd.code)
                    e->input_types.resize(nd.code + 1, -1);
                if (e->input_types[nd.code] >= 0 && e->input_types[nd.code] != nd.type)
                    rc = chgpu_set_error(CHGPU_ERR_BAD_ARGUMENTS, "node %u: column %d declared with two types", k, nd.code);
                e->input_types[nd.code] = nd.type;
                e->types[k] = nd.type;
            }
        }
        else if (nd.kind == CHGPU_EX_CONST)
        {
            if (!chgpu_type_size(nd.type))
                rc = chgpu_set_error(CHGPU_ERR_BAD_ARGUMENTS, "node %u: constant of type %d", k, nd.type);
            e->types[k] = nd.type;
        }
        else if (nd.kind == CHGPU_EX_FUNC)
        {
            // a code without a row is refused below, as "function %d over types", once its two operands have been found in place
            const FnRow * f = fn_row(nd.code);
            const int ar = f ? f->arity : 2;
            int at[3] = {-1, -1, -1};
            for (int j = 0; j < ar && rc == CHGPU_OK; ++j)
            {
                if (nd.args[j] < 0 || (u32)nd.args[j] >= k)
                    rc = chgpu_set_error(CHGPU_ERR_BAD_ARGUMENTS, "node %u: operand %d is not an earlier node", k, j);
                else
                    at[j] = e->types[nd.args[j]];
            }
            if (rc == CHGPU_OK && f && f->gate)
                if (const char * why_not = f->gate(nodes, nd, at))
                    rc = chgpu_set_error(CHGPU_ERR_NOT_IMPLEMENTED, "node %u: %s", k, why_not);
            if (rc == CHGPU_OK)
            {
                e->types[k] = f ? f->type(*f, nd.code, at[0], at[1], at[2]) : -1;
                if (e->types[k] < 0)
                    rc = chgpu_set_error(CHGPU_ERR_NOT_IMPLEMENTED, "node %u: function %d over types (%d, %d, %d)", k, nd.code, at[0], at[1], at[2]);
            }
        }
        else
            rc = chgpu_set_error(CHGPU_ERR_BAD_ARGUMENTS, "node %u: kind %d", k, nd.kind);
    }
    if (rc == CHGPU_OK)
        rc = build_body(e);
    if (rc != CHGPU_OK)
    {
        delete e;
        return rc;
    }
    *out = e;
    return CHGPU_OK;
}

extern "C" int chgpu_expr_node_type(const chgpu_expr * e, uint32_t node, int * type_out)
{
    CHGPU_REQUIRE(e && type_out && node < e->types.size(), CHGPU_ERR_BAD_ARGUMENTS, "bad node");
    *type_out = e->types[node];
    return CHGPU_OK;
}

extern "C" int chgpu_expr_free(chgpu_expr * e)
{
    delete e;
    return CHGPU_OK;
}

/* run hiprtc only (no device needed): the "does it compile for gfx950" check of a DAG */
extern "C" int chgpu_expr_precompile(const chgpu_expr * e, uint32_t n_outputs, const uint32_t * out_nodes, int filter_node, int value_node,
                                     uint64_t * code_bytes_out)
{
    CHGPU_REQUIRE(e, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    KernelSpec ks;
    CHGPU_TRY(make_spec(e, n_outputs == 0 ? FORM_SUM : filter_node >= 0 ? FORM_WHERE_MAP : FORM_MAP, n_outputs, out_nodes, filter_node, value_node, true, &ks));
    const std::vector<char> * code = nullptr;
    CHGPU_TRY(jit_compile(ks.form == FORM_WHERE_MAP ? gen_filter_source(e, ks) : gen_source(e, ks), &code));
    if (code_bytes_out)
        *code_bytes_out = code->size();
    return CHGPU_OK;
}

extern "C" int chgpu_expr_execute(chgpu_ctx * ctx, const chgpu_expr * e, uint32_t n_cols, const chgpu_col * const * cols, uint32_t n_outputs,
                                  const uint32_t * out_nodes, chgpu_col ** outs)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    CHGPU_REQUIRE(ctx && e && cols && outs, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    u64 rows = 0;
    CHGPU_TRY(check_spec(e, n_cols, cols, &rows));
    KernelSpec ks;
    CHGPU_TRY(make_spec(e, FORM_MAP, n_outputs, out_nodes, -1, -1, cols_aligned(e, cols), &ks));
    hipFunction_t fn = nullptr;
    CHGPU_TRY(jit_functions(ctx, gen_source(e, ks), {{"k_run", &fn}}));
    JitArgs a = bind_inputs(e, cols, rows);
    OutCols res;
    CHGPU_TRY(res.alloc(ctx, e, ks.out_nodes, rows, a));
    if (rows)
    {
        CHGPU_TRY(launch(ctx, fn, chgpu_grid_for(ctx, run_items(rows, ks), 256, jit_env(ctx, "tune_jit_wg_map", 4)), 256, a));
        ctx->counters[6] += 1;
    }
    res.hand_over(outs);
    return CHGPU_OK;
}

extern "C" int chgpu_expr_filter_sum_node(chgpu_ctx * ctx, const chgpu_expr * e, uint32_t n_cols, const chgpu_col * const * cols, int filter_node,
                                          int value_node, int * result_type_out, void * sum_out, uint64_t * count_out)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    CHGPU_REQUIRE(ctx && e && cols, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    u64 rows = 0;
    CHGPU_TRY(check_spec(e, n_cols, cols, &rows));
    KernelSpec ks;
    CHGPU_TRY(make_spec(e, FORM_SUM, 0, nullptr, filter_node, value_node, cols_aligned(e, cols), &ks));
    if (result_type_out)
        *result_type_out = value_node >= 0 ? chgpu_sum_result_type(e->types[value_node]) : CHGPU_U64;
    u64 res[2] = {0, 0}; // sum bits, count
    if (rows)
        CHGPU_TRY(run_reduction(ctx, e, cols, rows, gen_source(e, ks), "k_run", "k_fin", run_items(rows, ks), jit_env(ctx, "tune_jit_wg_sum", 2), 2, res));
    if (sum_out)
        memcpy(sum_out, &res[0], 8);
    if (count_out)
        *count_out = res[1];
    return CHGPU_OK;
}

extern "C" int chgpu_expr_filter_execute(chgpu_ctx * ctx, const chgpu_expr * e, uint32_t n_cols, const chgpu_col * const * cols, uint32_t filter_node,
                                         uint32_t n_outputs, const uint32_t * out_nodes, chgpu_col ** outs, uint64_t * rows_out)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    CHGPU_REQUIRE(ctx && e && cols && outs && rows_out && out_nodes, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    KernelSpec ks;
    CHGPU_TRY(make_spec(e, FORM_WHERE_MAP, n_outputs, out_nodes, (int)filter_node, -1, false, &ks)); // one row per lane, whatever the alignment
    u64 rows = 0;
    CHGPU_TRY(check_spec(e, n_cols, cols, &rows));
    JitArgs a = bind_inputs(e, cols, rows);
    OutCols res;
    u64 total = 0;
    if (rows)
    {
        hipFunction_t fcount = nullptr, femit = nullptr;
        CHGPU_TRY(jit_functions(ctx, gen_filter_source(e, ks), {{"k_fcount", &fcount}, {"k_femit", &femit}}));
        const u64 n_chunks = (rows + FE_CHUNK - 1) / FE_CHUNK;
        auto al = [](size_t b) { return (b + 255) / 256 * 256; };
        const size_t b_cnt = al(n_chunks * 4), b_off = al(n_chunks * 8), b_tmp = chgpu_scan_tmp_bytes(n_chunks);
        void * scratch = nullptr;
        CHGPU_TRY(chgpu_scratch(ctx, b_cnt + b_off + 256 + b_tmp, &scratch));
        u32 * counts = (u32 *)scratch;
        u64 * offsets = (u64 *)((char *)scratch + b_cnt);
        u64 * total_dev = (u64 *)((char *)scratch + b_cnt + b_off);
        void * tmp = (char *)scratch + b_cnt + b_off + 256;
        a.part = (u64 *)counts;
        const u32 grid = chgpu_grid_for(ctx, n_chunks * 64, 256, 8);
        CHGPU_TRY(launch(ctx, fcount, grid, 256, a));
        CHGPU_TRY(chgpu_scan_exclusive_u32_u64(ctx, counts, offsets, n_chunks, total_dev, tmp, b_tmp));
        CHGPU_TRY(chgpu_read_back(ctx, total_dev, &total, sizeof(total)));
        CHGPU_TRY(res.alloc(ctx, e, ks.out_nodes, total, a));
        if (total)
        {
            a.part = offsets;
            CHGPU_TRY(launch(ctx, femit, grid, 256, a));
        }
        ctx->counters[6] += 2;
        ctx->counters[0] += total; // FilterTransformPassedRows
    }
    else
        CHGPU_TRY(res.alloc(ctx, e, ks.out_nodes, 0, a));
    res.hand_over(outs);
    *rows_out = total;
    return CHGPU_OK;
}

extern "C" int chgpu_expr_filter_minmax_node(chgpu_ctx * ctx, const chgpu_expr * e, uint32_t n_cols, const chgpu_col * const * cols, int filter_node,
                                             uint32_t value_node, int * value_type_out, void * min_out, void * max_out, uint64_t * count_out)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    CHGPU_REQUIRE(ctx && e && cols, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(value_node < e->types.size(), CHGPU_ERR_BAD_ARGUMENTS, "bad node");
    CHGPU_TRY(check_filter_node(e, filter_node, false));
    const int vt = e->types[value_node];
    CHGPU_REQUIRE(chgpu_type_is_int(vt), CHGPU_ERR_NOT_IMPLEMENTED,
                  "min / max of a Float column keep a NaN that arrives first (SingleValueDataFixed::setIfSmaller): order-dependent, CPU path");
    u64 rows = 0;
    CHGPU_TRY(check_spec(e, n_cols, cols, &rows));
    if (value_type_out)
        *value_type_out = vt;
    u64 res[3] = {~0ull, 0, 0}; // lowest key, highest key, count
    if (rows)
        CHGPU_TRY(run_reduction(ctx, e, cols, rows, gen_minmax_source(e, filter_node, (int)value_node), "k_mm", "k_mm_fin", (rows + 3) / 4, 8, 3, res));
    // no row passed: the aggregate of an empty set is the type's default (AggregateFunctionMin on non-Nullable arguments: 0)
    const u64 sign = chgpu_type_is_signed(vt) ? 0x8000000000000000ull : 0;
    const u64 vmin = res[2] ? (res[0] ^ sign) : 0, vmax = res[2] ? (res[1] ^ sign) : 0;
    const size_t es = chgpu_type_size(vt);
    if (min_out)
        memcpy(min_out, &vmin, es); // little endian: the low bytes are the value in its own width
    if (max_out)
        memcpy(max_out, &vmax, es);
    if (count_out)
        *count_out = res[2];
    return CHGPU_OK;
}
