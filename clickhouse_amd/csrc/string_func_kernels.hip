// string_func_kernels.hip — functions that compute a new column from a ColumnString (src/Columns/ColumnString.h:40-52): length, lengthUTF8,
// empty / notEmpty (FunctionStringOrArrayToT over LengthImpl / LengthUTF8Impl / EmptyImpl), lower / upper (LowerUpperImpl, the ASCII
// forms), column-versus-column comparison (FunctionsComparison.h StringComparisonImpl::string_vector_string_vector), substring with
// constant arguments (FunctionsStringSubstring: SubstringImpl, GatherUtils sliceFromLeft/RightConstantOffset*), concat (ConcatImpl) and
// position with a constant needle (PositionImpl::vectorConstant).  Every byte-level rule is stated in include/chgpu.h.
//
//   k_sf_length<KIND>   length / empty / notEmpty: the offsets alone.  lengthUTF8: one lane per row, 8 bytes a step, the popcount of
//                       the bytes that are no continuation byte (10xxxxxx), the tail masked.
//   k_sf_map_case       lower / upper walk no rows: a flat sweep over chars[0, offsets.back()) in the 16-byte chunks of StrGrid, loaded
//                       through str_load_chunk.  The flip is SWAR on the two 8-byte words: a per-byte range mask, shifted to bit 0x20.
//                       A whole chunk is stored in one piece, the two edge chunks byte by byte; nothing in front of the view or behind
//                       offsets.back() is read or written.  The offsets are copied.
//   k_sf_cmp_columns    one lane per row: str_compare over both values in global memory, str_cmp_holds.
//   k_sf_substring_sizes / _move, k_sf_concat_sizes / _move
//                       sizes from the offsets alone (too_long through str_size_u32), then str_copy_value per part and the zero,
//                       which the move writes itself.  concat's constant parts are staged into LDS once per workgroup from the kernel
//                       argument.  Between the two kernels: str_build_values, as for filter and index.
//   k_sf_position       one lane per row: candidates for the needle's first byte 8 bytes a step (SWAR zero-byte test), the rest of the
//                       needle verified against the constant in LDS (str_equals_words), stop at the first hit.  Start positions behind
//                       size - needle are masked off, so an occurrence never takes in the terminating zero or the next row.
// Everything these share with the other String operators is string_column.h: a value's begin and size, the copy loop, the compare and
// equality loops, the grid; the prologue and a second column argument; the entry point of one result column (str_one_column: length,
// cmp_columns, position) and the one that builds a ColumnString (str_build_values: substring, concat -- the call's allocations of
// str_call, its one pool allocation divided by str_carve over str_values_lay of string_host.h, the layout pass str_layout_values).
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
    const StrGrid g(chars, size);
    for (u64 q = ((u64)blockIdx.x * 256 + threadIdx.x) * 16; q < g.end; q += (u64)gridDim.x * 256 * 16)
    {
        const uint4 v = str_load_chunk(g, q);
        const u64 lo = sf_flip_word((u64)v.x | ((u64)v.y << 32), add_ge, add_gt), hi = sf_flip_word((u64)v.z | ((u64)v.w << 32), add_ge, add_gt);
        if (q >= g.a0 && q + 16 <= g.end)
        {
            const uint4 r = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
            __builtin_memcpy(out + (q - g.a0), &r, 16); // the result starts on its own grid: this store is unaligned when the view is
        }
        else
        {
            for (u32 k = 0; k < 16; ++k) // the chunk holding the view's first byte, and the one holding its last
                if (q + k >= g.a0 && q + k < g.end)
                    out[q + k - g.a0] = (u8)((k < 8 ? lo : hi) >> (8 * (k & 7)));
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
        const u8 * pa = a_chars + va.begin, * pb = b_chars + vb.begin;
        const int cmp = str_compare([&](u64 j) { return str_load8(pa + j); }, [&](u64 j) { return str_load8(pb + j); }, va.size - 1, vb.size - 1);
        out[i] = str_cmp_holds(op, cmp) ? 1 : 0;
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
                    if (str_equals_words([&](u32 k) { return str_load8(p + s + k); }, [&](u32 k) { return s_w[k >> 3]; }, m))
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
    return str_one_column(ctx, "string length", wide ? CHGPU_U64 : CHGPU_U8, n, [&](void * dst) {
        const dim3 grid(chgpu_grid_for(ctx, n, 256, 8)), block(256);
        if (kind == CHGPU_STR_LENGTH)
            hipLaunchKernelGGL(k_sf_length<CHGPU_STR_LENGTH>, grid, block, 0, ctx->stream, col.offsets, col.chars, n, dst);
        else if (kind == CHGPU_STR_LENGTH_UTF8)
            hipLaunchKernelGGL(k_sf_length<CHGPU_STR_LENGTH_UTF8>, grid, block, 0, ctx->stream, col.offsets, col.chars, n, dst);
        else if (kind == CHGPU_STR_EMPTY)
            hipLaunchKernelGGL(k_sf_length<CHGPU_STR_EMPTY>, grid, block, 0, ctx->stream, col.offsets, col.chars, n, dst);
        else
            hipLaunchKernelGGL(k_sf_length<CHGPU_STR_NOT_EMPTY>, grid, block, 0, ctx->stream, col.offsets, col.chars, n, dst);
        ctx->counters[6] += 1;
        return (int)CHGPU_OK;
    }, out);
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
        hipLaunchKernelGGL(k_sf_map_case, dim3(chgpu_grid_for(ctx, str_grid_chunks(StrGrid(col.chars, size)), 256, 8)), dim3(256), 0, ctx->stream, col.chars, size,
                           (u32)(kind == CHGPU_STR_UPPER), (u8 *)res.v[1]->data);
        ctx->counters[6] += 2;
        CHGPU_TRY(str_launched("string map_case"));
    }
    res.give(out_offsets_u64, out_chars_u8);
    return CHGPU_OK;
}

extern "C" int chgpu_string_cmp_columns(chgpu_ctx * ctx, const chgpu_col * a_offsets_u64, const chgpu_col * a_chars_u8, const chgpu_col * b_offsets_u64,
                                        const chgpu_col * b_chars_u8, int op, chgpu_col ** out_u8)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    StrColumn a, b;
    CHGPU_TRY(str_column_begin(ctx, a_offsets_u64, a_chars_u8, b_offsets_u64 && b_chars_u8 && out_u8, [&] {
        CHGPU_REQUIRE(op >= CHGPU_EQ && op <= CHGPU_GE, CHGPU_ERR_BAD_ARGUMENTS, "unknown comparison %d", op);
        return str_column_also_checks(a_offsets_u64, b_offsets_u64, b_chars_u8, 1);
    }, &a));
    CHGPU_TRY(str_column_also(ctx, a_offsets_u64, a_chars_u8, b_offsets_u64, b_chars_u8, &b));
    const u64 n = a.rows;
    return str_one_column(ctx, "string cmp_columns", CHGPU_U8, n, [&](void * dst) {
        hipLaunchKernelGGL(k_sf_cmp_columns, dim3(chgpu_grid_for(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, a.offsets, a.chars, b.offsets, b.chars, n, op, (u8 *)dst);
        ctx->counters[6] += 1;
        return (int)CHGPU_OK;
    }, out_u8);
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
    return str_build_values(ctx, "substring", n, n,
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
                CHGPU_TRY(str_column_also_checks(first->offsets, g.offsets, g.chars, p));
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
        const chgpu_string_arg * walked = first; // the same column may appear several times: its offsets are walked once
        for (u32 q = 0; q < p; ++q)
            if (args[q].offsets == g.offsets && args[q].chars == g.chars)
                walked = &args[q];
        StrColumn also;
        CHGPU_TRY(str_column_also(ctx, walked->offsets, walked->chars, g.offsets, g.chars, &also));
        a.offsets[p] = also.offsets, a.chars[p] = also.chars;
    }
    const u64 n = col.rows;
    const dim3 grid(chgpu_grid_for(ctx, n, 256, 8)), block(256);
    return str_build_values(ctx, "concat", n, n,
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
    return str_one_column(ctx, "string position", CHGPU_U64, n, [&](void * dst) {
        hipLaunchKernelGGL(k_sf_position, dim3(chgpu_grid_for(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, col.offsets, col.chars, n, str_const_of(needle, needle_bytes),
                           (u64 *)dst);
        ctx->counters[6] += 1;
        return (int)CHGPU_OK;
    }, out_u64);
}
