// string_func_kernels.hip — functions that compute a new column from a ColumnString (src/Columns/ColumnString.h:40-52): length, lengthUTF8,
// empty / notEmpty (FunctionStringOrArrayToT over LengthImpl / LengthUTF8Impl / EmptyImpl), lower / upper (LowerUpperImpl, the ASCII
// forms), column-versus-column comparison (FunctionsComparison.h StringComparisonImpl::string_vector_string_vector), substring with
// constant arguments (FunctionsStringSubstring: SubstringImpl, GatherUtils sliceFromLeft/RightConstantOffset*), concat (ConcatImpl) and
// position with a constant needle (PositionImpl::vectorConstant).  Every byte-level rule is stated in include/chgpu.h.
//
//   k_sf_length<KIND>   length / empty / notEmpty: the offsets alone.  lengthUTF8: one lane per row, 8 bytes a step, the popcount of
//                       the bytes that are no continuation byte (10xxxxxx), the tail masked.
//   k_sf_map_case       lower / upper walk no rows: a flat sweep over chars[0, offsets.back()) in 16-byte chunks cut on the grid of the
//                       chars ADDRESS (as k_str_contains_flat cuts its tiles), so that a view that starts anywhere loads aligned.  The
//                       flip is SWAR on the two 8-byte words: a per-byte range mask, shifted to bit 0x20.  The two edge chunks go byte
//                       by byte; nothing in front of the view or behind offsets.back() is read or written.  The offsets are copied.
//   k_sf_cmp_columns    one lane per row, 8 bytes a step from both sides; differing words are ordered by one compare of the
//                       byte-swapped words (as k_str_row_const), then the shorter value is the smaller.
//   k_sf_substring_sizes / _move, k_sf_concat_sizes / _move
//                       the shape of chgpu_string_filter: sizes from the offsets alone (too_long through str_size_u32), the layout
//                       pass of string_column.h, then str_copy_value per part and the zero, which the move writes itself.
//                       concat's constant parts are staged into LDS once per workgroup from the kernel argument.
//   k_sf_position       one lane per row: candidates for the needle's first byte 8 bytes a step (SWAR zero-byte test), the rest of the
//                       needle verified against the constant in LDS, stop at the first hit.  Start positions behind size - needle are
//                       masked off, so an occurrence never takes in the terminating zero or the next row.
// What these share with the other String operators (a value's begin and size, the copy loop, the prologue, the call's allocations, the
// layout pass) is string_column.h; the one pool allocation of substring / concat is divided by str_values_lay of string_host.h.
#include "string_column.h"

static constexpr u32 SF_ARGS = 8; // arguments of one concat
static constexpr u64 SF_HI = 0x8080808080808080ull, SF_LO7 = 0x7F7F7F7F7F7F7F7Full;

// ---------------------------------------------------------------------------------------------
// length, lengthUTF8, empty, notEmpty.  Bytes per row: 8 B offset + 8 B (1 B) result; lengthUTF8 reads the value once on top.
// ---------------------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(256) void k_sf_length(const u64 * __restrict__ offsets, const u8 * __restrict__ chars, u64 n, void * __restrict__ out)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        const StrValue v = str_value(offsets, i);
        const u64 len = v.size - 1;
        if (KIND == CHGPU_STR_LENGTH)
            ((u64 *)out)[i] = len;
        else if (KIND == CHGPU_STR_EMPTY)
            ((u8 *)out)[i] = len == 0;
        else if (KIND == CHGPU_STR_NOT_EMPTY)
            ((u8 *)out)[i] = len != 0;
        else
        {
            // UTF8::countCodePoints: every byte that is not 10xxxxxx, on valid and invalid UTF-8 alike
            const u8 * p = chars + v.begin;
            u64 count = 0;
            for (u64 j = 0; j < len; j += 8)
            {
                const u64 x = str_load8(p + j);
                u64 not_cont = ~(x & ~(x << 1)) & SF_HI; // 0x80 in every byte that has bit 7 clear or bit 6 set
                if (len - j < 8)
                    not_cont &= str_tail_mask(len - j);
                count += __builtin_popcountll(not_cont);
            }
            ((u64 *)out)[i] = count;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// lower / upper.  Bytes: chars read once and written once + 16 B per row of offsets (copied).
// ---------------------------------------------------------------------------------------------
// bit 0x20 of every byte of x in [first, first + 25]; `add_ge` = 0x80 - first, `add_gt` = 0x80 - (first + 26), in every byte
__device__ __forceinline__ u64 sf_flip_word(u64 x, u64 add_ge, u64 add_gt)
{
    const u64 h = x & SF_LO7; // no carry leaves a byte: 0x7F + 0x3F < 0x100
    const u64 in_range = (h + add_ge) & ~(h + add_gt) & ~x & SF_HI;
    return x ^ (in_range >> 2);
}

__global__ __launch_bounds__(256) void k_sf_map_case(const u8 * __restrict__ chars, u64 size, u32 upper, u8 * __restrict__ out)
{
    const u32 first = upper ? 'a' : 'A';
    const u64 add_ge = 0x0101010101010101ull * (0x80 - first), add_gt = 0x0101010101010101ull * (0x80 - first - 26);
    const u64 a0 = (u64)chars & 15;
    const u8 * grid = chars - a0; // 16-byte aligned; only [a0, end) is read
    const u64 end = a0 + size;
    for (u64 q = ((u64)blockIdx.x * 256 + threadIdx.x) * 16; q < end; q += (u64)gridDim.x * 256 * 16)
    {
        if (q >= a0 && q + 16 <= end)
        {
            const uint4 v = *(const uint4 *)(grid + q);
            const u64 lo = sf_flip_word((u64)v.x | ((u64)v.y << 32), add_ge, add_gt), hi = sf_flip_word((u64)v.z | ((u64)v.w << 32), add_ge, add_gt);
            const uint4 r = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
            __builtin_memcpy(out + (q - a0), &r, 16); // the result starts on its own grid: this store is unaligned when the view is
        }
        else
        {
            for (u32 k = 0; k < 16; ++k) // the chunk holding the view's first byte, and the one holding its last
                if (q + k >= a0 && q + k < end)
                {
                    const u32 b = grid[q + k];
                    out[q + k - a0] = (u8)(b - first < 26u ? b ^ 0x20u : b);
                }
        }
    }
}

__global__ __launch_bounds__(256) void k_sf_copy_u64(const u64 * __restrict__ in, u64 n, u64 * __restrict__ out)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
        out[i] = in[i];
}

// ---------------------------------------------------------------------------------------------
// a <op> b, row by row.  Bytes per row: 16 B offsets + up to min(len_a, len_b) bytes of both + 1 B.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sf_cmp_columns(const u64 * __restrict__ a_offsets, const u8 * __restrict__ a_chars, const u64 * __restrict__ b_offsets,
                                                        const u8 * __restrict__ b_chars, u64 n, int op, u8 * __restrict__ out)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        const StrValue va = str_value(a_offsets, i), vb = str_value(b_offsets, i);
        const u64 la = va.size - 1, lb = vb.size - 1;
        const u64 k = la < lb ? la : lb;
        const u8 * pa = a_chars + va.begin, * pb = b_chars + vb.begin;
        int cmp = 0;
        for (u64 j = 0; j < k; j += 8)
        {
            u64 a = str_load8(pa + j), b = str_load8(pb + j);
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
        const bool res = op == CHGPU_EQ ? cmp == 0 : op == CHGPU_NE ? cmp != 0 : op == CHGPU_LT ? cmp < 0 : op == CHGPU_GT ? cmp > 0 : op == CHGPU_LE ? cmp <= 0 : cmp >= 0;
        out[i] = res ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------
// substring(s, offset[, length]), constant arguments, bytes.  Bytes per row: 8 B offset + 4 B size + 8 B position (written, read) +
// 8 B new offset + the window's bytes read and written.
// ---------------------------------------------------------------------------------------------
struct SfWindow
{
    u64 begin, count; // bytes [begin, begin + count) of the value
};

// The window of include/chgpu.h over a value of `len` bytes, clipped to [0, len); offset != 0.  Every sum saturates: offset may be
// INT64_MIN and length 2^64 - 1.
__device__ __forceinline__ SfWindow sf_window(u64 len, i64 offset, u32 has_length, u64 length)
{
    u64 start; // index of the window's first byte when it is not negative
    if (offset > 0)
        start = (u64)offset - 1;
    else
    {
        const u64 back = 0 - (u64)offset; // |offset|, 2^63 for INT64_MIN
        if (back > len)
        {
            // the window starts back - len indexes in front of the value: what is left of `length` behind them starts at byte 0
            const u64 before = back - len;
            if (!has_length)
                return {0, len};
            if (length <= before)
                return {0, 0};
            const u64 rest = length - before;
            return {0, rest < len ? rest : len};
        }
        start = len - back;
    }
    if (start >= len)
        return {len, 0};
    const u64 room = len - start;
    return {start, !has_length || length > room ? room : length};
}

__global__ __launch_bounds__(256) void k_sf_substring_sizes(const u64 * __restrict__ offsets, u64 n, i64 offset, u32 has_length, u64 length, u32 * __restrict__ sizes,
                                                            u32 * __restrict__ too_long)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
        sizes[i] = str_size_u32(sf_window(str_value(offsets, i).size - 1, offset, has_length, length).count + 1, too_long);
}

__global__ __launch_bounds__(256) void k_sf_substring_move(const u64 * __restrict__ offsets, const u8 * __restrict__ chars, const u64 * __restrict__ byte_pos, u64 n,
                                                           i64 offset, u32 has_length, u64 length, u64 * __restrict__ out_offsets, u8 * __restrict__ out_chars)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        const StrValue v = str_value(offsets, i);
        const SfWindow w = sf_window(v.size - 1, offset, has_length, length);
        const u64 dst = byte_pos[i];
        out_offsets[i] = dst + w.count + 1;
        str_copy_value(out_chars + dst, chars + v.begin + w.begin, w.count);
        out_chars[dst + w.count] = 0; // the source's byte behind the window is not a zero in general
    }
}

// ---------------------------------------------------------------------------------------------
// concat(a, b, ...).  Bytes per row: 8 B offset per column argument (read by both kernels) + 4 B size + 8 B position (written, read) +
// 8 B new offset + the columns' bytes read + the result's bytes written.
// ---------------------------------------------------------------------------------------------
struct SfConcat
{
    const u64 * offsets[SF_ARGS]; // NULL: the argument is a constant
    const u8 * chars[SF_ARGS];
    u32 const_at[SF_ARGS]; // a constant's first byte in c, and its bytes
    u32 const_len[SF_ARGS];
    u32 n_args;
    StrConst c; // the constants one after another; c.len: their bytes together
};

__global__ __launch_bounds__(256) void k_sf_concat_sizes(const SfConcat a, u64 n, u32 * __restrict__ sizes, u32 * __restrict__ too_long)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        u64 total = (u64)a.c.len + 1;
#pragma unroll
        for (u32 p = 0; p < SF_ARGS; ++p)
            if (p < a.n_args && a.offsets[p])
            {
                const u64 len = str_value(a.offsets[p], i).size - 1;
                total = total + len < total ? ~0ull : total + len; // saturating
            }
        sizes[i] = str_size_u32(total, too_long);
    }
}

__global__ __launch_bounds__(256) void k_sf_concat_move(const SfConcat a, const u64 * __restrict__ byte_pos, u64 n, u64 * __restrict__ out_offsets,
                                                        u8 * __restrict__ out_chars)
{
    __shared__ u64 s_w[SM_MAX / 8];
    str_stage_const(s_w, a.c);
    __syncthreads();
    const u8 * s_bytes = (const u8 *)s_w;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        u64 dst = byte_pos[i];
#pragma unroll
        for (u32 p = 0; p < SF_ARGS; ++p)
            if (p < a.n_args)
            {
                if (a.offsets[p])
                {
                    const StrValue v = str_value(a.offsets[p], i);
                    str_copy_value(out_chars + dst, a.chars[p] + v.begin, v.size - 1);
                    dst += v.size - 1;
                }
                else
                {
                    str_copy_value(out_chars + dst, s_bytes + a.const_at[p], a.const_len[p]);
                    dst += a.const_len[p];
                }
            }
        out_chars[dst] = 0;
        out_offsets[i] = dst + 1;
    }
}

// ---------------------------------------------------------------------------------------------
// position(haystack, needle), constant needle.  Bytes per row: 8 B offset + the value up to its first occurrence + 8 B result.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sf_position(const u64 * __restrict__ offsets, const u8 * __restrict__ chars, u64 n, const StrConst c, u64 * __restrict__ out)
{
    __shared__ u64 s_w[SM_MAX / 8];
    str_stage_const(s_w, c);
    __syncthreads();
    const u64 first = 0x0101010101010101ull * (c.w[0] & 0xFF);
    const u32 m = c.len;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        const StrValue v = str_value(offsets, i);
        const u64 len = v.size - 1;
        const u8 * p = chars + v.begin;
        u64 res = m == 0; // the empty needle is found at 1
        if (m && m <= len)
        {
            const u64 starts = len - m + 1; // start positions at which the needle lies wholly inside the value
            for (u64 j = 0; j < starts && !res; j += 8)
            {
                u32 cand = str_zero_bytes(str_load8(p + j) ^ first);
                if (starts - j < 8)
                    cand &= (1u << (starts - j)) - 1;
                while (cand)
                {
                    const u64 s = j + __builtin_ctz(cand);
                    cand &= cand - 1;
                    bool eq = true;
                    for (u32 k = 0; k < m; k += 8)
                    {
                        u64 x = str_load8(p + s + k) ^ s_w[k >> 3];
                        if (m - k < 8)
                            x &= str_tail_mask(m - k);
                        if (x)
                        {
                            eq = false;
                            break;
                        }
                    }
                    if (eq)
                    {
                        res = s + 1;
                        break;
                    }
                }
            }
        }
        out[i] = res;
    }
}

// ---------------------------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------------------------
static int sf_end(const char * what)
{
    CHGPU_REQUIRE(hipGetLastError() == hipSuccess, CHGPU_ERR_DEVICE, "string %s kernels failed to launch", what);
    return CHGPU_OK;
}

extern "C" int chgpu_string_length(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, int kind, chgpu_col ** out)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    StrColumn col;
    CHGPU_TRY(str_column_begin(ctx, offsets_u64, chars_u8, out != nullptr, [&] {
        CHGPU_REQUIRE(kind >= CHGPU_STR_LENGTH && kind <= CHGPU_STR_NOT_EMPTY, CHGPU_ERR_BAD_ARGUMENTS, "unknown string length kind %d", kind);
        return (int)CHGPU_OK;
    }, &col));
    const u64 n = col.rows;
    const bool wide = kind == CHGPU_STR_LENGTH || kind == CHGPU_STR_LENGTH_UTF8;
    PairAllocs mem = str_call(ctx, "string length");
    StrCols<> res;
    CHGPU_TRY(mem.col_new(wide ? CHGPU_U64 : CHGPU_U8, n, &res.v[0]));
    if (n)
    {
        const dim3 grid(chgpu_grid_for(ctx, n, 256, 8)), block(256);
        void * dst = res.v[0]->data;
        if (kind == CHGPU_STR_LENGTH)
            hipLaunchKernelGGL(k_sf_length<CHGPU_STR_LENGTH>, grid, block, 0, ctx->stream, col.offsets, col.chars, n, dst);
        else if (kind == CHGPU_STR_LENGTH_UTF8)
            hipLaunchKernelGGL(k_sf_length<CHGPU_STR_LENGTH_UTF8>, grid, block, 0, ctx->stream, col.offsets, col.chars, n, dst);
        else if (kind == CHGPU_STR_EMPTY)
            hipLaunchKernelGGL(k_sf_length<CHGPU_STR_EMPTY>, grid, block, 0, ctx->stream, col.offsets, col.chars, n, dst);
        else
            hipLaunchKernelGGL(k_sf_length<CHGPU_STR_NOT_EMPTY>, grid, block, 0, ctx->stream, col.offsets, col.chars, n, dst);
        ctx->counters[6] += 1;
        CHGPU_TRY(sf_end("length"));
    }
    res.give(out);
    return CHGPU_OK;
}

extern "C" int chgpu_string_map_case(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, int kind, chgpu_col ** out_offsets_u64,
                                     chgpu_col ** out_chars_u8)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    StrColumn col;
    CHGPU_TRY(str_column_begin(ctx, offsets_u64, chars_u8, out_offsets_u64 && out_chars_u8, [&] {
        CHGPU_REQUIRE(kind == CHGPU_STR_LOWER || kind == CHGPU_STR_UPPER, CHGPU_ERR_BAD_ARGUMENTS, "unknown string case kind %d (lowerUTF8 / upperUTF8: CPU path)", kind);
        return (int)CHGPU_OK;
    }, &col));
    const u64 n = col.rows;
    u64 size = 0; // offsets.back(): bytes of a wrapped chars buffer behind it belong to no value
    if (n)
        CHGPU_TRY(chgpu_read_back(ctx, col.offsets + (n - 1), &size, sizeof(size)));
    PairAllocs mem = str_call(ctx, "string map_case");
    StrCols<> res;
    CHGPU_TRY(mem.col_new(CHGPU_U64, n, &res.v[0]));
    CHGPU_TRY(mem.col_new(CHGPU_U8, size, &res.v[1]));
    if (n)
    {
        hipLaunchKernelGGL(k_sf_copy_u64, dim3(chgpu_grid_for(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, col.offsets, n, (u64 *)res.v[0]->data);
        const u64 chunks = (((u64)(uintptr_t)col.chars & 15) + size + 15) / 16;
        hipLaunchKernelGGL(k_sf_map_case, dim3(chgpu_grid_for(ctx, chunks, 256, 8)), dim3(256), 0, ctx->stream, col.chars, size, (u32)(kind == CHGPU_STR_UPPER),
                           (u8 *)res.v[1]->data);
        ctx->counters[6] += 2;
        CHGPU_TRY(sf_end("map_case"));
    }
    res.give(out_offsets_u64, out_chars_u8);
    return CHGPU_OK;
}

extern "C" int chgpu_string_cmp_columns(chgpu_ctx * ctx, const chgpu_col * a_offsets_u64, const chgpu_col * a_chars_u8, const chgpu_col * b_offsets_u64,
                                        const chgpu_col * b_chars_u8, int op, chgpu_col ** out_u8)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    StrColumn a;
    CHGPU_TRY(str_column_begin(ctx, a_offsets_u64, a_chars_u8, b_offsets_u64 && b_chars_u8 && out_u8, [&] {
        CHGPU_REQUIRE(b_offsets_u64->type == CHGPU_U64 && b_chars_u8->type == CHGPU_U8, CHGPU_ERR_BAD_ARGUMENTS, "ColumnString = UInt64 offsets + UInt8 chars");
        CHGPU_REQUIRE(op >= CHGPU_EQ && op <= CHGPU_GE, CHGPU_ERR_BAD_ARGUMENTS, "unknown comparison %d", op);
        CHGPU_REQUIRE(a_offsets_u64->rows == b_offsets_u64->rows, CHGPU_ERR_SIZES_MISMATCH, "the columns have %llu and %llu rows",
                      (unsigned long long)a_offsets_u64->rows, (unsigned long long)b_offsets_u64->rows);
        return (int)CHGPU_OK;
    }, &a));
    if (b_offsets_u64 != a_offsets_u64 || b_chars_u8 != a_chars_u8)
        CHGPU_TRY(str_validate_offsets(ctx, b_offsets_u64, b_chars_u8));
    const u64 n = a.rows;
    PairAllocs mem = str_call(ctx, "string cmp_columns");
    StrCols<> res;
    CHGPU_TRY(mem.col_new(CHGPU_U8, n, &res.v[0]));
    if (n)
    {
        hipLaunchKernelGGL(k_sf_cmp_columns, dim3(chgpu_grid_for(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, a.offsets, a.chars, (const u64 *)b_offsets_u64->data,
                           (const u8 *)b_chars_u8->data, n, op, (u8 *)res.v[0]->data);
        ctx->counters[6] += 1;
        CHGPU_TRY(sf_end("cmp_columns"));
    }
    res.give(out_u8);
    return CHGPU_OK;
}

// the shape substring and concat share with filter and index: `sizes(l)` launches the sizes kernel, `move(l, out)` the move kernel
template <class Sizes, class Move>
static int sf_build_values(chgpu_ctx * ctx, const char * op, u64 n, Sizes && sizes, Move && move, chgpu_col ** out_offsets_u64, chgpu_col ** out_chars_u8)
{
    PairAllocs mem = str_call(ctx, op);
    PairTemps tmp(mem);
    StrValuesLayout l{};
    if (n)
    {
        CHGPU_TRY(str_carve(tmp, [&](uintptr_t base) { return str_values_lay(base, n, false, chgpu_scan_tmp_bytes(n), &l); }));
        CHGPU_HIP(hipMemsetAsync(l.words, 0, sizeof(StrLayoutWords), ctx->stream));
        sizes(l);
        ctx->counters[6] += 1;
    }
    StrLayoutWords words;
    StrCols<> res;
    CHGPU_TRY(str_layout_values(ctx, mem, l, n, false, n, &words, &res));
    if (n)
    {
        move(l, res);
        ctx->counters[6] += 1;
        CHGPU_TRY(sf_end(op));
    }
    res.give(out_offsets_u64, out_chars_u8);
    return CHGPU_OK;
}

extern "C" int chgpu_string_substring(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, int64_t offset, int has_length, uint64_t length,
                                      chgpu_col ** out_offsets_u64, chgpu_col ** out_chars_u8)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    StrColumn col;
    CHGPU_TRY(str_column_begin(ctx, offsets_u64, chars_u8, out_offsets_u64 && out_chars_u8, [&] {
        CHGPU_REQUIRE(offset != 0, CHGPU_ERR_NOT_IMPLEMENTED, "substring with offset 0 (the reference's answer has changed between versions): CPU path");
        return (int)CHGPU_OK;
    }, &col));
    const u64 n = col.rows;
    const dim3 grid(chgpu_grid_for(ctx, n, 256, 8)), block(256);
    const u32 has = has_length != 0;
    return sf_build_values(ctx, "substring", n,
        [&](const StrValuesLayout & l) {
            hipLaunchKernelGGL(k_sf_substring_sizes, grid, block, 0, ctx->stream, col.offsets, n, (i64)offset, has, (u64)length, l.sizes, (u32 *)&l.words->too_long);
        },
        [&](const StrValuesLayout & l, StrCols<> & res) {
            hipLaunchKernelGGL(k_sf_substring_move, grid, block, 0, ctx->stream, col.offsets, col.chars, (const u64 *)l.pos, n, (i64)offset, has, (u64)length,
                               (u64 *)res.v[0]->data, (u8 *)res.v[1]->data);
        },
        out_offsets_u64, out_chars_u8);
}

extern "C" int chgpu_string_concat(chgpu_ctx * ctx, const chgpu_string_arg * args, uint32_t n_args, chgpu_col ** out_offsets_u64, chgpu_col ** out_chars_u8)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    CHGPU_REQUIRE(ctx && args && out_offsets_u64 && out_chars_u8, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(n_args >= 2 && n_args <= SF_ARGS, CHGPU_ERR_BAD_ARGUMENTS, "concat takes 2 to %u arguments, not %u", SF_ARGS, n_args);
    const chgpu_string_arg * first = nullptr; // the first column among the arguments
    for (u32 p = 0; p < n_args && !first; ++p)
        if (args[p].offsets)
            first = &args[p];
    CHGPU_REQUIRE(first, CHGPU_ERR_BAD_ARGUMENTS, "concat of constants only: at least one argument is a column");
    SfConcat a;
    memset(&a, 0, sizeof(a));
    a.n_args = n_args;
    StrColumn col;
    CHGPU_TRY(str_column_begin(ctx, first->offsets, first->chars, true, [&] {
        u64 const_total = 0;
        for (u32 p = 0; p < n_args; ++p)
        {
            const chgpu_string_arg & g = args[p];
            if (g.offsets)
            {
                CHGPU_REQUIRE(g.chars, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument (chars of argument %u)", p);
                CHGPU_REQUIRE(g.offsets->type == CHGPU_U64 && g.chars->type == CHGPU_U8, CHGPU_ERR_BAD_ARGUMENTS, "ColumnString = UInt64 offsets + UInt8 chars");
                CHGPU_REQUIRE(g.offsets->rows == first->offsets->rows, CHGPU_ERR_SIZES_MISMATCH, "argument %u has %llu rows, not %llu", p,
                              (unsigned long long)g.offsets->rows, (unsigned long long)first->offsets->rows);
                continue;
            }
            CHGPU_REQUIRE(g.value || !g.value_bytes, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument (value of argument %u)", p);
            CHGPU_REQUIRE(g.value_bytes <= SM_MAX - const_total, CHGPU_ERR_NOT_IMPLEMENTED, "more than %u constant bytes in one concat: CPU path", SM_MAX);
            a.const_at[p] = (u32)const_total, a.const_len[p] = (u32)g.value_bytes;
            if (g.value_bytes)
                memcpy((u8 *)a.c.w + const_total, g.value, g.value_bytes);
            const_total += g.value_bytes;
        }
        a.c.len = (u32)const_total;
        return (int)CHGPU_OK;
    }, &col));
    for (u32 p = 0; p < n_args; ++p)
    {
        const chgpu_string_arg & g = args[p];
        if (!g.offsets)
            continue;
        bool seen = false; // the same column may appear several times: its offsets are walked once
        for (u32 q = 0; q < p; ++q)
            seen = seen || (args[q].offsets == g.offsets && args[q].chars == g.chars);
        if (!seen && &g != first)
            CHGPU_TRY(str_validate_offsets(ctx, g.offsets, g.chars));
        a.offsets[p] = (const u64 *)g.offsets->data, a.chars[p] = (const u8 *)g.chars->data;
    }
    const u64 n = col.rows;
    const dim3 grid(chgpu_grid_for(ctx, n, 256, 8)), block(256);
    return sf_build_values(ctx, "concat", n,
        [&](const StrValuesLayout & l) { hipLaunchKernelGGL(k_sf_concat_sizes, grid, block, 0, ctx->stream, a, n, l.sizes, (u32 *)&l.words->too_long); },
        [&](const StrValuesLayout & l, StrCols<> & res) {
            hipLaunchKernelGGL(k_sf_concat_move, grid, block, 0, ctx->stream, a, (const u64 *)l.pos, n, (u64 *)res.v[0]->data, (u8 *)res.v[1]->data);
        },
        out_offsets_u64, out_chars_u8);
}

extern "C" int chgpu_string_position_const(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, const void * needle, uint64_t needle_bytes,
                                           chgpu_col ** out_u64)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    StrColumn col;
    CHGPU_TRY(str_column_begin(ctx, offsets_u64, chars_u8, out_u64 && (needle || !needle_bytes), [&] {
        CHGPU_REQUIRE(needle_bytes <= SM_MAX, CHGPU_ERR_NOT_IMPLEMENTED, "a needle of %llu bytes (the kernels carry %u): CPU path", (unsigned long long)needle_bytes, SM_MAX);
        return (int)CHGPU_OK;
    }, &col));
    const u64 n = col.rows;
    PairAllocs mem = str_call(ctx, "string position");
    StrCols<> res;
    CHGPU_TRY(mem.col_new(CHGPU_U64, n, &res.v[0]));
    if (n)
    {
        hipLaunchKernelGGL(k_sf_position, dim3(chgpu_grid_for(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, col.offsets, col.chars, n,
                           str_const_of(needle, needle_bytes), (u64 *)res.v[0]->data);
        ctx->counters[6] += 1;
        CHGPU_TRY(sf_end("position"));
    }
    res.give(out_u64);
    return CHGPU_OK;
}
