// string_column.h — what a kernel or an entry point of string_kernels.hip, string_sort_kernels.hip and string_func_kernels.hip needs to
// know about a ColumnString (src/Columns/ColumnString.h:40-52: `chars` with a terminating zero after every value, `offsets[i]` = end of
// value i including that zero), written once.
// Device: str_load8, str_value, str_copy_value, str_size_u32; the constant a kernel argument carries (StrConst, str_stage_const) and the
// word tests made against it (str_tail_mask, str_zero_bytes); the two loops over a value's 8-byte words, which take one callable per
// side that gives the word at a byte offset (global memory, the constant in LDS, a shifted LDS tile): str_compare with str_cmp_holds,
// and str_equals_words; the 16-byte grid of the chars ADDRESS (StrGrid, str_load_chunk).
// Host: the entry points' prologue (str_column_begin) and a further column argument (str_column_also_checks, str_column_also), the
// call's numbered allocations (str_call: pair_pool.h with `test_string_fail_alloc`) and its one pool allocation divided by a layout of
// string_host.h (str_carve), the guard of a call's columns (StrCols), the check behind a call's launches (str_launched), and the two
// shapes of an entry point: one result column with one value per row (str_one_column), and a new ColumnString built by a sizes kernel,
// the layout pass (str_layout_values) and a move kernel (str_build_values).
#pragma once

#include "chgpu_internal.h"
#include "pair_pool.h"
#include "string_host.h"

__device__ __forceinline__ u64 str_load8(const u8 * p)
{
    u64 v;
    __builtin_memcpy(&v, p, 8); // unaligned: global memory allows it; the column's 64-byte pad covers the over-read
    return v;
}

struct StrValue
{
    u64 begin; // of its first byte in chars
    u64 size;  // its bytes and the terminating zero
};

__device__ __forceinline__ StrValue str_value(const u64 * __restrict__ offsets, u64 r)
{
    const u64 begin = r ? offsets[r - 1] : 0;
    return {begin, offsets[r] - begin};
}

// 8 bytes a step while 8 whole bytes are left, then byte by byte: the zero travels with the value, nothing is written behind it
__device__ __forceinline__ void str_copy_value(u8 * __restrict__ dst, const u8 * __restrict__ src, u64 sz)
{
    u64 k = 0;
    for (; k + 8 <= sz; k += 8)
    {
        const u64 v = str_load8(src + k);
        __builtin_memcpy(dst + k, &v, 8);
    }
    for (; k < sz; ++k)
        dst[k] = src[k];
}

// a value's size as the layout pass scans it; 4 GiB or more raises the flag and takes no bytes (the call fails)
__device__ __forceinline__ u32 str_size_u32(u64 sz, u32 * __restrict__ too_long)
{
    if (sz >= (1ull << 32))
        *too_long = 1, sz = 0;
    return (u32)sz;
}

// A constant (a value, a needle, a LIKE pattern, the constant parts of a concat) travels in the kernel argument -- no device allocation,
// no upload -- and is staged into LDS once per workgroup, where every lane reads it at its own index.
static constexpr u32 SM_MAX = CHGPU_STR_CONST_MAX; // bytes of a constant / tokens of a pattern a kernel argument carries

struct StrConst
{
    u64 w[SM_MAX / 8];     // the bytes (little endian words), zero padded
    u32 meta[SM_MAX / 32]; // k_str_like: bit i set = token i is a wildcard
    u32 len;
    u32 pad;
};

// kernel argument -> LDS with constant indices only (a lane-indexed read of the argument itself would go through scratch)
__device__ __forceinline__ void str_stage_const(u64 * s_w, const StrConst & c)
{
    if (threadIdx.x == 0)
    {
#pragma unroll
        for (u32 k = 0; k < SM_MAX / 8; ++k)
            s_w[k] = c.w[k];
    }
}

__device__ __forceinline__ u64 str_tail_mask(u64 bytes) // 1 <= bytes <= 7
{
    return ~0ull >> (8 * (8 - bytes));
}

// bit k set = byte k of x is zero
__device__ __forceinline__ u32 str_zero_bytes(u64 x)
{
    const u64 l = 0x7F7F7F7F7F7F7F7Full;
    const u64 z = ~(((x & l) + l) | x | l); // 0x80 in every zero byte, exact
    return (u32)(((z >> 7) * 0x0102040810204080ull) >> 56);
}

// The order of two values (memcmpSmallAllowOverflow15, then the lengths): the common prefix as unsigned bytes, 8 bytes a step with the
// tail masked, the first differing words ordered by one compare of the byte-swapped words; equal prefixes: the shorter value is the
// smaller.  `word_a(j)` / `word_b(j)`: the 8 bytes at byte offset j of a side; what lies behind the common prefix is masked off.
template <class WordA, class WordB>
__device__ __forceinline__ int str_compare(WordA && word_a, WordB && word_b, u64 la, u64 lb)
{
    const u64 k = la < lb ? la : lb;
    int cmp = 0;
    for (u64 j = 0; j < k; j += 8)
    {
        u64 a = word_a(j), b = word_b(j);
        if (k - j < 8)
        {
            const u64 tm = str_tail_mask(k - j);
            a &= tm, b &= tm;
        }
        if (a != b)
        {
            cmp = __builtin_bswap64(a) < __builtin_bswap64(b) ? -1 : 1; // the first byte is the most significant one
            break;
        }
    }
    if (cmp == 0)
        cmp = la < lb ? -1 : la > lb ? 1 : 0;
    return cmp;
}

__device__ __forceinline__ bool str_cmp_holds(int op, int cmp) // CHGPU_EQ .. CHGPU_GE over str_compare's answer
{
    return op == CHGPU_EQ ? cmp == 0 : op == CHGPU_NE ? cmp != 0 : op == CHGPU_LT ? cmp < 0 : op == CHGPU_GT ? cmp > 0 : op == CHGPU_LE ? cmp <= 0 : cmp >= 0;
}

// the m bytes of both sides are equal; words as in str_compare; `Len` is the caller's index type (u32 where m is a constant's length)
template <class WordA, class WordB, class Len>
__device__ __forceinline__ bool str_equals_words(WordA && word_a, WordB && word_b, Len m)
{
    for (Len k = 0; k < m; k += 8)
    {
        u64 x = word_a(k) ^ word_b(k);
        if (m - k < 8)
            x &= str_tail_mask(m - k);
        if (x)
            return false;
    }
    return true;
}

// The 16-byte grid of the chars ADDRESS: a flat sweep over chars cuts its chunks (and its tiles of chunks) there, so that a view that
// starts anywhere loads aligned.  Grid position q is byte q - a0 of chars; only [a0, end) belongs to chars.
struct StrGrid
{
    u64 a0;          // grid position of chars' first byte, < 16
    const u8 * grid; // 16-byte aligned
    u64 end;
    __host__ __device__ StrGrid(const u8 * chars, u64 size) : a0((u64)(uintptr_t)chars & 15), grid(chars - a0), end(a0 + size) {}
};

static inline u64 str_grid_chunks(const StrGrid & g) // the 16-byte chunks that hold a byte of chars
{
    return (g.end + 15) / 16;
}

// the 16 bytes at grid position q (a multiple of 16), zeros where they lie outside chars: nothing outside is read
__device__ __forceinline__ uint4 str_load_chunk(const StrGrid & g, u64 q)
{
    if (q >= g.a0 && q + 16 <= g.end)
        return *(const uint4 *)(g.grid + q);
    u64 lo = 0, hi = 0;
    if (q + 16 > g.a0 && q < g.end)
    {
#pragma unroll
        for (u32 k = 0; k < 16; ++k)
            if (q + k >= g.a0 && q + k < g.end)
            {
                const u64 b = g.grid[q + k];
                if (k < 8)
                    lo |= b << (8 * k);
                else
                    hi |= b << (8 * (k - 8));
            }
    }
    return make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
}

static StrConst str_const_of(const void * bytes, u64 n)
{
    StrConst c;
    memset(&c, 0, sizeof(c));
    if (n)
        memcpy(c.w, bytes, n);
    c.len = (u32)n;
    return c;
}

struct StrColumn // a validated ColumnString
{
    const u64 * offsets;
    const u8 * chars;
    u64 rows;
};

// `others_present`: the entry point's other pointers are not NULL.  `own_checks() -> int` holds the checks the entry point makes
// between the type check and the walk over the offsets (it may use the columns: they are not NULL there).
template <class OwnChecks>
static int str_column_begin(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, bool others_present, OwnChecks && own_checks, StrColumn * col)
{
    CHGPU_REQUIRE(ctx && offsets_u64 && chars_u8 && others_present, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(offsets_u64->type == CHGPU_U64 && chars_u8->type == CHGPU_U8, CHGPU_ERR_BAD_ARGUMENTS, "ColumnString = UInt64 offsets + UInt8 chars");
    CHGPU_TRY(own_checks());
    CHGPU_TRY(str_validate_offsets(ctx, offsets_u64, chars_u8));
    *col = StrColumn{(const u64 *)offsets_u64->data, (const u8 *)chars_u8->data, offsets_u64->rows};
    return CHGPU_OK;
}

// A column argument behind the first one.  Its checks that need no device belong into the first column's `own_checks` (every such check
// of a call is made in front of the first walk); `arg_no` counts the call's arguments from 0 ...
static int str_column_also_checks(const chgpu_col * first_offsets_u64, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, u32 arg_no)
{
    CHGPU_REQUIRE(offsets_u64->type == CHGPU_U64 && chars_u8->type == CHGPU_U8, CHGPU_ERR_BAD_ARGUMENTS, "ColumnString = UInt64 offsets + UInt8 chars");
    CHGPU_REQUIRE(offsets_u64->rows == first_offsets_u64->rows, CHGPU_ERR_SIZES_MISMATCH, "argument %u has %llu rows, not %llu", arg_no,
                  (unsigned long long)offsets_u64->rows, (unsigned long long)first_offsets_u64->rows);
    return CHGPU_OK;
}

// ... and its walk over the offsets, behind the first column's: a column that was walked (the first one) and is given again is not
// walked again
static int str_column_also(chgpu_ctx * ctx, const chgpu_col * walked_offsets_u64, const chgpu_col * walked_chars_u8, const chgpu_col * offsets_u64,
                           const chgpu_col * chars_u8, StrColumn * col)
{
    if (offsets_u64 != walked_offsets_u64 || chars_u8 != walked_chars_u8)
        CHGPU_TRY(str_validate_offsets(ctx, offsets_u64, chars_u8));
    *col = StrColumn{(const u64 *)offsets_u64->data, (const u8 *)chars_u8->data, offsets_u64->rows};
    return CHGPU_OK;
}

static inline PairAllocs str_call(chgpu_ctx * ctx, const char * op)
{
    PairAllocs mem{ctx, op, "test_string_fail_alloc"};
    mem.begin_call();
    return mem;
}

// one pool allocation of the call, divided by `lay(base) -> bytes` (a layout of string_host.h with its arguments bound); its first
// sub-buffer is the allocation itself, which is what PairTemps::release takes
template <class Lay>
static int str_carve(PairTemps & tmp, Lay && lay)
{
    void * mem = nullptr;
    CHGPU_TRY(tmp.alloc(lay(0), &mem));
    lay((uintptr_t)mem);
    return CHGPU_OK;
}

template <int N = 2> // >= 2
struct StrCols // columns a call made, freed unless given to the caller
{
    chgpu_col * v[N] = {};
    ~StrCols() { drop(); }
    void drop()
    {
        for (chgpu_col *& c : v)
            if (c) chgpu_col_free(c), c = nullptr;
    }
    void give(chgpu_col ** a, chgpu_col ** b = nullptr)
    {
        *a = v[0];
        if (b)
            *b = v[1], v[1] = nullptr;
        v[0] = nullptr;
    }
};

// The layout pass of an operator that builds a ColumnString of n values: l.sizes (the caller's sizes kernel wrote them and raised
// the flags in l.words, zeroed before) -> l.pos, the words on the host in one read-back, the flags as their errors, the result's
// offsets and chars columns.  The result has n rows, or words->rows when `rows_scanned` (the caller's kept-row scan left them there).
static int str_layout_values(chgpu_ctx * ctx, PairAllocs & mem, const StrValuesLayout & l, u64 n, bool rows_scanned, u64 src_rows, StrLayoutWords * words, StrCols<> * out)
{
    *words = StrLayoutWords{};
    if (n)
    {
        CHGPU_TRY(chgpu_scan_exclusive_u32_u64(ctx, l.sizes, l.pos, n, &l.words->bytes, l.scan_tmp, chgpu_scan_tmp_bytes(n)));
        CHGPU_TRY(chgpu_read_back(ctx, l.words, words, sizeof(*words)));
        CHGPU_REQUIRE(!words->bad_index, CHGPU_ERR_BAD_ARGUMENTS, "an index is not below the column's %llu rows", (unsigned long long)src_rows);
        CHGPU_REQUIRE(!words->too_long, CHGPU_ERR_NOT_IMPLEMENTED, "a value of 4 GiB or more");
    }
    if (!rows_scanned)
        words->rows = n;
    CHGPU_TRY(mem.col_new(CHGPU_U64, words->rows, &out->v[0]));
    return mem.col_new(CHGPU_U8, words->bytes, &out->v[1]);
}

static int str_launched(const char * op) // behind the launches of a call
{
    CHGPU_REQUIRE(hipGetLastError() == hipSuccess, CHGPU_ERR_DEVICE, "%s kernels failed to launch", op);
    return CHGPU_OK;
}

// An entry point with one result column of `type` and one value per row of a column of n rows: `launch(data) -> int` fills it (and
// counts its kernels); it is not called for n == 0.
template <class Launch>
static int str_one_column(chgpu_ctx * ctx, const char * op, int type, u64 n, Launch && launch, chgpu_col ** out)
{
    PairAllocs mem = str_call(ctx, op);
    StrCols<> res;
    CHGPU_TRY(mem.col_new(type, n, &res.v[0]));
    if (n)
    {
        CHGPU_TRY(launch(res.v[0]->data));
        CHGPU_TRY(str_launched(op));
    }
    res.give(out);
    return CHGPU_OK;
}

// An entry point that builds a ColumnString of n values: `sizes(l)` launches the kernel that writes l.sizes and raises the flags of
// l.words, the layout pass follows, `move(l, res)` launches the kernel that writes the result's offsets and chars.  `rows_out` is
// the filter's: its sizes kernel also wrote l.flag over the n rows of the source, a scan of them gives every kept row its row in the
// result, the result has that many rows, and an empty result needs no move.  KernelLaunches: one per kernel; the filter counts both of
// its own behind the move, launched or not, and its kept rows as RowsProduced.
template <class Sizes, class Move>
static int str_build_values(chgpu_ctx * ctx, const char * op, u64 n, u64 src_rows, Sizes && sizes, Move && move, chgpu_col ** out_offsets_u64,
                            chgpu_col ** out_chars_u8, uint64_t * rows_out = nullptr)
{
    const bool kept = rows_out != nullptr;
    PairAllocs mem = str_call(ctx, op);
    PairTemps tmp(mem);
    StrValuesLayout l{};
    if (n)
    {
        CHGPU_TRY(str_carve(tmp, [&](uintptr_t base) { return str_values_lay(base, n, kept, chgpu_scan_tmp_bytes(n), &l); }));
        CHGPU_HIP(hipMemsetAsync(l.words, 0, sizeof(StrLayoutWords), ctx->stream));
        sizes(l);
        if (kept)
            CHGPU_TRY(chgpu_scan_exclusive_u32_u64(ctx, l.flag, l.row_pos, n, &l.words->rows, l.scan_tmp, chgpu_scan_tmp_bytes(n)));
        else
            ctx->counters[6] += 1;
    }
    StrLayoutWords words;
    StrCols<> res;
    CHGPU_TRY(str_layout_values(ctx, mem, l, n, kept, src_rows, &words, &res));
    if (n)
    {
        if (words.rows)
            move(l, res);
        ctx->counters[6] += kept ? 2 : 1;
        if (kept)
            ctx->counters[0] += words.rows;
        CHGPU_TRY(str_launched(op));
    }
    res.give(out_offsets_u64, out_chars_u8);
    if (kept)
        *rows_out = words.rows;
    return CHGPU_OK;
}
