// string_column.h — what a kernel or an entry point of string_kernels.hip, string_sort_kernels.hip and string_func_kernels.hip needs to
// know about a ColumnString (src/Columns/ColumnString.h:40-52: `chars` with a terminating zero after every value, `offsets[i]` = end of
// value i including that zero), written once.  Device: str_load8, str_value, str_copy_value, str_size_u32, and the constant a kernel
// argument carries (StrConst, str_stage_const) with the two word tests made against it (str_tail_mask, str_zero_bytes).  Host: the entry points' prologue
// (str_column_begin), the call's numbered allocations (str_call: pair_pool.h with `test_string_fail_alloc`) and its one pool
// allocation divided by a layout of string_host.h (str_carve), the guard of a call's columns (StrCols), the layout pass.
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
