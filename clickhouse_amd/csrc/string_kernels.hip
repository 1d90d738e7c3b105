// string_kernels.hip — SURVEY §8(f) rank 2: String keys.  A ColumnString (src/Columns/ColumnString.h:40-49: `chars` with a
// terminating zero after every value, `offsets[i]` = end of value i including that zero) is dictionary-encoded on the device:
// every row gets the dense id of its value, ids numbered by first appearance — what ColumnUnique::uniqueInsertRangeFrom builds
// when a String column is turned into a LowCardinality one (src/Columns/ColumnUnique.h:520-620), and what the reference's
// key_string / StringHashMap aggregation (AggregatedDataVariants.h:96, Common/HashTable/StringHashTable.h) achieves per row with
// a CPU hash table keyed by the bytes.  The ids then take the ordinary UInt32 GROUP BY / join path (through
// LowCardinalityDictionary when several stripes or Blocks must agree on ids).
//
//   k_str_hash      64-bit hash of every value (8 bytes per step, unaligned loads inside the column's padding)
//   k_str_insert    open-addressing table of hash tags; every row lowers `first_row` of its tag's cell (atomicMin): the
//                   representative of a value is its FIRST row, independent of scheduling
//   k_str_resolve   every row compares its bytes with its representative's (length + content): equal -> it belongs to that value;
//                   different bytes under one 64-bit tag -> the collision flag (the call answers NOT_IMPLEMENTED: exactness is
//                   never traded; the reference's `hashed` method accepts 128-bit collisions, this path accepts none)
//   scan of the "I am a first row" flags -> dense ids in order of first appearance; k_str_ids gathers them per row
// The hash is internal (placement only).  Algorithmic bytes: chars once + 8 B offsets + 4 B id per row; the table traffic is
// random 16-byte cells, two touches per row.
// Further down: ColumnString::filter and the predicates against a constant.  What the String kernels and entry points share is
// string_column.h: a value's begin and size, the copy loop, the ordered compare and the equality test of two byte ranges, the grid of
// the chars address; the prologue, the call's allocations, the entry point of one result column (every predicate) and the one that
// builds a ColumnString (filter).  The buffer layouts are string_host.h.
#include "string_column.h"

__device__ __forceinline__ u64 str_hash_bytes(const u8 * p, u64 len)
{
    u64 h = 0x9E3779B97F4A7C15ull ^ (len * 0xff51afd7ed558ccdull);
    u64 i = 0;
    for (; i + 8 <= len; i += 8)
    {
        h = (h ^ str_load8(p + i)) * 0xc4ceb9fe1a85ec53ull;
        h ^= h >> 29;
    }
    if (i < len)
    {
        const u64 tail = str_load8(p + i) & (~0ull >> (8 * (8 - (len - i)))); // (str_tail_mask, spelled out: tests/keycraft.py restates this function)
        h = (h ^ tail) * 0xc4ceb9fe1a85ec53ull;
        h ^= h >> 29;
    }
    h = dev_intHash64(h);
    return h | 1ull; // 0 marks an empty cell
}

// ColumnString invariant (ColumnString.h:40-52): offsets strictly increase (every value has at least its terminating zero) and end inside
// chars.  The kernels below compute `offsets[i] - begin - 1` bytes per value and read that many: an offset column that breaks the
// invariant (corrupted or hostile input) would turn into a 2^64-byte walk -- a hang or a fault, not an error code.
__global__ __launch_bounds__(256) void k_str_check_offsets(const u64 * __restrict__ offsets, u64 n, u64 chars_size, u32 * __restrict__ bad)
{
    bool b = false;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        const u64 begin = i ? offsets[i - 1] : 0, end = offsets[i];
        b = b || !(begin < end && end <= chars_size);
    }
    if (b)
        *bad = 1;
}

int str_validate_offsets(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8) // (called by str_column_begin, string_column.h)
{
    const u64 n = offsets_u64->rows;
    if (!n)
        return CHGPU_OK;
    void * scratch = nullptr;
    CHGPU_TRY(chgpu_scratch(ctx, 256, &scratch));
    CHGPU_HIP(hipMemsetAsync(scratch, 0, 4, ctx->stream));
    hipLaunchKernelGGL(k_str_check_offsets, dim3(chgpu_grid_for(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, (const u64 *)offsets_u64->data, n, (u64)chars_u8->rows, (u32 *)scratch);
    ctx->counters[6] += 1;
    u32 bad = 0;
    CHGPU_TRY(chgpu_read_back(ctx, scratch, &bad, 4));
    CHGPU_REQUIRE(!bad, CHGPU_ERR_BAD_ARGUMENTS, "ColumnString offsets must strictly increase and stay inside chars (%llu bytes)", (unsigned long long)chars_u8->rows);
    return CHGPU_OK;
}

__global__ __launch_bounds__(256) void k_str_hash(const u64 * __restrict__ offsets, const u8 * __restrict__ chars, u64 n, u64 * __restrict__ hash)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        const StrValue v = str_value(offsets, i);
        hash[i] = str_hash_bytes(chars + v.begin, v.size - 1); // without the terminating zero (ColumnString.h:48-52)
    }
}

__global__ __launch_bounds__(256) void k_str_insert(const u64 * __restrict__ hash, u64 n, u64 * __restrict__ tags, unsigned long long * __restrict__ first_row, u64 mask,
                                                    u32 * __restrict__ fail)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        const u64 h = hash[i];
        u64 s = (h >> 1) & mask;
        bool placed = false;
        for (u64 probe = 0; probe <= mask; ++probe) // bounded: the table has >= 2 cells per row
        {
            u64 t = tags[s];
            if (t == 0)
            {
                t = atomicCAS((unsigned long long *)&tags[s], 0ull, (unsigned long long)h);
                if (t == 0)
                    t = h;
            }
            if (t == h)
            {
                // first_row only ever decreases, so a (possibly stale) value <= i proves the atomic would change nothing; without
                // this test a low-cardinality column sends every row's atomic to a few thousand addresses (same-address atomics
                // serialise: 1e8 rows over 2500 values took 414 ms, all of it here)
                if (__builtin_nontemporal_load(&first_row[s]) > (unsigned long long)i)
                    atomicMin(&first_row[s], (unsigned long long)i);
                placed = true;
                break;
            }
            s = (s + 1) & mask;
        }
        if (!placed)
            *fail = 1;
    }
}

__global__ __launch_bounds__(256) void k_str_resolve(const u64 * __restrict__ offsets, const u8 * __restrict__ chars, const u64 * __restrict__ hash, u64 n,
                                                     const u64 * __restrict__ tags, const unsigned long long * __restrict__ first_row, u64 mask,
                                                     u64 * __restrict__ rep_row, u32 * __restrict__ is_first, u32 * __restrict__ fail)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        const u64 h = hash[i];
        u64 s = (h >> 1) & mask;
        u64 r = ~0ull;
        for (u64 probe = 0; probe <= mask; ++probe)
        {
            const u64 t = tags[s];
            if (t == h)
            {
                r = first_row[s];
                break;
            }
            if (t == 0)
                break;
            s = (s + 1) & mask;
        }
        if (r >= n)
        {
            *fail = 1;
            r = i;
        }
        if (r != i)
        {
            const StrValue v0 = str_value(offsets, i), v1 = str_value(offsets, r);
            const u8 * p0 = chars + v0.begin, * p1 = chars + v1.begin;
            if (v0.size != v1.size || !str_equals_words([&](u64 k) { return str_load8(p0 + k); }, [&](u64 k) { return str_load8(p1 + k); }, v0.size - 1))
                *fail = 2; // two different values under one 64-bit tag
        }
        rep_row[i] = r;
        is_first[i] = r == i ? 1u : 0u;
    }
}

__global__ __launch_bounds__(256) void k_str_ids(const u64 * __restrict__ rep_row, const u32 * __restrict__ is_first, const u64 * __restrict__ prefix, u64 n,
                                                 u32 * __restrict__ ids, u64 * __restrict__ dict_rows)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        ids[i] = (u32)prefix[rep_row[i]]; // exclusive prefix of the first-row flags = number of values that appeared earlier
        if (is_first[i])
            dict_rows[prefix[i]] = i;
    }
}

extern "C" int chgpu_string_dictionary_encode(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, chgpu_col ** ids_u32,
                                              chgpu_col ** first_rows_u64, uint64_t * n_distinct)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    StrColumn col;
    CHGPU_TRY(str_column_begin(ctx, offsets_u64, chars_u8, ids_u32 && first_rows_u64 && n_distinct, [&] {
        const u64 n = offsets_u64->rows;
        CHGPU_REQUIRE(n < (1ull << 32), CHGPU_ERR_NOT_IMPLEMENTED, "more than 2^32 rows per call");
        *n_distinct = 0;
        if (n == 0)
            return (int)CHGPU_OK;
        // the last offset must equal the size of chars (ColumnString invariant); checked with one read-back
        u64 last = 0;
        CHGPU_TRY(chgpu_read_back(ctx, (const u64 *)offsets_u64->data + (n - 1), &last, sizeof(last)));
        CHGPU_REQUIRE(last == chars_u8->rows, CHGPU_ERR_SIZES_MISMATCH, "offsets.back() (%llu) != chars.size() (%llu)", (unsigned long long)last,
                      (unsigned long long)chars_u8->rows);
        return (int)CHGPU_OK;
    }, &col));
    const u64 n = col.rows;
    const u32 grid = chgpu_grid_for(ctx, n, 256, 8);
    PairAllocs mem = str_call(ctx, "string dictionary_encode");
    PairTemps tmp(mem);
    StrDictLayout l;
    u64 total = 0;
    if (n)
    {
        u64 cap = 1024;
        while (cap < 2 * n)
            cap <<= 1; // cells of the table: a power of two, at least two per row
        const size_t b_tmp = chgpu_scan_tmp_bytes(n);
        CHGPU_TRY(str_carve(tmp, [&](uintptr_t base) { return str_dict_lay(base, n, cap, b_tmp, &l); }));
        CHGPU_HIP(hipMemsetAsync(l.tags, 0, cap * 8, ctx->stream));
        CHGPU_HIP(hipMemsetAsync(l.first_row, 0xFF, cap * 8, ctx->stream));
        CHGPU_HIP(hipMemsetAsync(l.fail, 0, 256, ctx->stream));
        hipLaunchKernelGGL(k_str_hash, dim3(grid), dim3(256), 0, ctx->stream, col.offsets, col.chars, n, l.hash);
        hipLaunchKernelGGL(k_str_insert, dim3(grid), dim3(256), 0, ctx->stream, (const u64 *)l.hash, n, l.tags, l.first_row, cap - 1, l.fail);
        hipLaunchKernelGGL(k_str_resolve, dim3(grid), dim3(256), 0, ctx->stream, col.offsets, col.chars, (const u64 *)l.hash, n, (const u64 *)l.tags,
                           (const unsigned long long *)l.first_row, cap - 1, l.rep_row, l.is_first, l.fail);
        ctx->counters[6] += 3;
        CHGPU_TRY(chgpu_scan_exclusive_u32_u64(ctx, l.is_first, l.prefix, n, l.total, l.scan_tmp, b_tmp));
        CHGPU_TRY(chgpu_read_back(ctx, l.total, &total, sizeof(total)));
        u32 failed = 0;
        CHGPU_TRY(chgpu_read_back(ctx, l.fail, &failed, sizeof(failed)));
        CHGPU_REQUIRE(failed != 2, CHGPU_ERR_NOT_IMPLEMENTED, "two different strings share a 64-bit hash tag in this block: CPU path");
        CHGPU_REQUIRE(!failed, CHGPU_ERR_LOGICAL, "string table probe did not terminate");
    }
    StrCols<> out; // ids, first rows
    CHGPU_TRY(mem.col_new(CHGPU_U32, n, &out.v[0]));
    CHGPU_TRY(mem.col_new(CHGPU_U64, total, &out.v[1]));
    if (n)
    {
        hipLaunchKernelGGL(k_str_ids, dim3(grid), dim3(256), 0, ctx->stream, (const u64 *)l.rep_row, (const u32 *)l.is_first, (const u64 *)l.prefix, n,
                           (u32 *)out.v[0]->data, (u64 *)out.v[1]->data);
        ctx->counters[6] += 1;
        CHGPU_TRY(str_launched("string dictionary"));
    }
    out.give(ids_u32, first_rows_u64);
    *n_distinct = total;
    return CHGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// ColumnString::filter (src/Columns/ColumnString.cpp:270-290 -> filterArraysImpl<UInt8>, src/Columns/ColumnsCommon.cpp:191-286):
// the kept values' bytes are moved together and the offsets rebuilt.  The reference walks the mask 64 rows at a time and memcpy's
// runs of kept values; here two scans (kept rows, kept bytes) give every surviving value its new row and its new byte position,
// and one pass copies the values (8 bytes per step per lane, unaligned; the terminating zero travels with the value).
//   k_str_filter_sizes   flag[i] = mask[i] != 0, bytes[i] = flag ? size of value i incl. its zero : 0
//   k_str_filter_move    out_offsets[row'] = pos' + size;  out_chars[pos' ..] = chars[begin ..]
// Algorithmic bytes: 8 (offset) + 1 (mask) per row + kept bytes read and written + 8 per kept row.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_str_filter_sizes(const u64 * __restrict__ offsets, const u8 * __restrict__ mask, u64 n, u32 * __restrict__ flag,
                                                          u32 * __restrict__ bytes, u32 * __restrict__ too_long)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        const u32 f = mask[i] != 0;
        const StrValue v = str_value(offsets, i);
        flag[i] = f;
        bytes[i] = f ? str_size_u32(v.size, too_long) : 0u;
    }
}

__global__ __launch_bounds__(256) void k_str_filter_move(const u64 * __restrict__ offsets, const u8 * __restrict__ chars, const u32 * __restrict__ flag,
                                                         const u64 * __restrict__ row_pos, const u64 * __restrict__ byte_pos, u64 n,
                                                         u64 * __restrict__ out_offsets, u8 * __restrict__ out_chars)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        if (!flag[i])
            continue;
        const StrValue v = str_value(offsets, i);
        const u64 dst = byte_pos[i];
        out_offsets[row_pos[i]] = dst + v.size;
        str_copy_value(out_chars + dst, chars + v.begin, v.size);
    }
}

extern "C" int chgpu_string_filter(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, const chgpu_col * filter_u8,
                                   chgpu_col ** out_offsets_u64, chgpu_col ** out_chars_u8, uint64_t * rows_out)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    StrColumn col;
    CHGPU_TRY(str_column_begin(ctx, offsets_u64, chars_u8, filter_u8 && out_offsets_u64 && out_chars_u8 && rows_out, [&] {
        CHGPU_REQUIRE(filter_u8->type == CHGPU_U8, CHGPU_ERR_BAD_ARGUMENTS, "the filter is a UInt8 column");
        CHGPU_REQUIRE(filter_u8->rows == offsets_u64->rows, CHGPU_ERR_SIZES_MISMATCH, "Size of filter (%llu) doesn't match size of column (%llu)",
                      (unsigned long long)filter_u8->rows, (unsigned long long)offsets_u64->rows); // ColumnsCommon.cpp:199-200
        return (int)CHGPU_OK;
    }, &col));
    const u64 n = col.rows;
    const dim3 grid(chgpu_grid_for(ctx, n, 256, 8)), block(256);
    return str_build_values(ctx, "string filter", n, n,
        [&](const StrValuesLayout & l) {
            hipLaunchKernelGGL(k_str_filter_sizes, grid, block, 0, ctx->stream, col.offsets, (const u8 *)filter_u8->data, n, l.flag, l.sizes, (u32 *)&l.words->too_long);
        },
        [&](const StrValuesLayout & l, StrCols<> & out) {
            hipLaunchKernelGGL(k_str_filter_move, grid, block, 0, ctx->stream, col.offsets, col.chars, (const u32 *)l.flag, (const u64 *)l.row_pos, (const u64 *)l.pos, n,
                               (u64 *)out.v[0]->data, (u8 *)out.v[1]->data);
        },
        out_offsets_u64, out_chars_u8, rows_out);
}

// ---------------------------------------------------------------------------------------------
// String predicates against a constant: the WHERE clause over a ColumnString (FunctionsComparison.h StringComparisonImpl::
// string_vector_constant; FunctionsStringSearch.h / MatchImpl.h for like, position, startsWith, endsWith).  (offsets, chars, constant) -> one
// 0/1 byte per row.  The constant travels in the kernel argument (no device allocation, no upload) and is staged into LDS once per
// workgroup, where every lane reads it at its own index.  Three kernels:
//   k_str_row_const<MODE>   one lane per row: comparison (str_compare, str_cmp_holds), startsWith, endsWith (str_equals_words) of the value
//                           in global memory and the constant in LDS; at most min(len, constant) bytes of the value matter.
//                           Algorithmic bytes: 8 B offset + <= constant bytes + 1 B per row.
//   k_str_contains_flat     substring search that never walks rows: the chars buffer is swept in tiles of SM_TILE bytes of StrGrid (one
//                           16-byte str_load_chunk per lane into LDS + a halo of needle - 1 bytes of the next tile); every lane tests its
//                           16 start positions (first byte in registers, the rest out of LDS through str_equals_words, whose tile side
//                           shifts two LDS words together).  A hit at byte p belongs to the first row r with offsets[r] > p
//                           and counts when p + needle <= offsets[r] - 1.  k_str_tile_rows resolves the first row of every tile beforehand
//                           (one binary search per TILE); the tile's own offsets are staged in LDS, so a hit costs an LDS search over the
//                           tile's rows.  Result bytes are idempotent plain stores into a mask pre-filled with `negate`.
//                           Algorithmic bytes: chars once + 1 B per row (+ 8 B per row of offsets, read tile-wise).
//   k_str_like              any pattern with `_` or an inner `%`: one lane per row, the two-pointer wildcard match (the last `%` and the
//                           haystack mark are remembered; a mismatch resumes after that `%` with the mark advanced by one byte).
// ---------------------------------------------------------------------------------------------
static constexpr u32 SM_TILE = 4096;     // bytes of chars per workgroup step: 256 lanes x 16 B
static constexpr u32 SM_ROWS_LDS = 1024; // a tile with more rows than this searches its offsets in global memory
enum { SM_CMP = 0, SM_STARTS = 1, SM_ENDS = 2 };

template <int MODE>
__global__ __launch_bounds__(256) void k_str_row_const(const u64 * __restrict__ offsets, const u8 * __restrict__ chars, u64 n, const StrConst c, int op, u32 negate,
                                                       u8 * __restrict__ out)
{
    __shared__ u64 s_w[SM_MAX / 8];
    str_stage_const(s_w, c);
    __syncthreads();
    const u64 m = c.len;
    const auto constant = [&](u64 j) { return s_w[j >> 3]; };
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        const StrValue v = str_value(offsets, i);
        const u64 len = v.size - 1;
        const u8 * p = chars + v.begin + (MODE == SM_ENDS && len >= m ? len - m : 0);
        const auto value = [&](u64 j) { return str_load8(p + j); };
        bool res;
        if (MODE == SM_CMP)
            res = str_cmp_holds(op, str_compare(value, constant, len, m));
        else
            res = (len >= m && str_equals_words(value, constant, m)) != (negate != 0);
        out[i] = res ? 1 : 0;
    }
}

// `_`: one UTF-8 sequence.  The lead byte gives the length; every continuation byte must be 10xxxxxx and lie inside the value.  0 = no match here.
__device__ __forceinline__ u32 str_utf8_step(const u8 * __restrict__ p, u64 avail)
{
    const u32 b = p[0];
    const u32 l = b < 0x80 ? 1 : (b & 0xE0) == 0xC0 ? 2 : (b & 0xF0) == 0xE0 ? 3 : (b & 0xF8) == 0xF0 ? 4 : 0;
    if (l == 0 || l > avail)
        return 0;
    for (u32 k = 1; k < l; ++k)
        if ((p[k] & 0xC0) != 0x80)
            return 0;
    return l;
}

__global__ __launch_bounds__(256) void k_str_like(const u64 * __restrict__ offsets, const u8 * __restrict__ chars, u64 n, const StrConst c, u32 negate,
                                                  u8 * __restrict__ out)
{
    __shared__ u64 s_w[SM_MAX / 8];
    __shared__ u32 s_meta[SM_MAX / 32];
    str_stage_const(s_w, c);
    if (threadIdx.x == 0)
    {
#pragma unroll
        for (u32 k = 0; k < SM_MAX / 32; ++k)
            s_meta[k] = c.meta[k];
    }
    __syncthreads();
    const u8 * s_tok = (const u8 *)s_w;
    const u32 plen = c.len;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        const StrValue v = str_value(offsets, i);
        const u64 len = v.size - 1;
        const u8 * s = chars + v.begin;
        u64 h = 0, mark = 0;
        u32 p = 0;
        int star = -1;
        bool res = false;
        for (;;)
        {
            if (p < plen)
            {
                const u32 tok = s_tok[p];
                const bool meta = (s_meta[p >> 5] >> (p & 31)) & 1;
                if (meta && tok == '%')
                {
                    if (p + 1 == plen) // a trailing % takes whatever is left
                    {
                        res = true;
                        break;
                    }
                    star = (int)p, mark = h, ++p;
                    continue;
                }
                if (h >= len)
                    break; // the value is used up and the pattern still needs a character: a later mark only leaves less
                if (meta)
                {
                    const u32 step = str_utf8_step(s + h, len - h);
                    if (step)
                    {
                        h += step, ++p;
                        continue;
                    }
                }
                else if (s[h] == tok)
                {
                    ++h, ++p;
                    continue;
                }
            }
            else if (h == len)
            {
                res = true;
                break;
            }
            // mismatch: resume after the last %, which takes one byte more
            if (star < 0 || ++mark > len)
                break;
            h = mark, p = (u32)star + 1;
        }
        out[i] = (res != (negate != 0)) ? 1 : 0;
    }
}

// tile_row[t] = the first row r with offsets[r] > (first chars position of tile t), t = 0 .. ntiles (n when there is none).  Tiles are cut
// on the 16-byte grid of the chars ADDRESS: tile t covers chars positions [t * SM_TILE - a0, (t + 1) * SM_TILE - a0), a0 = address & 15.
__global__ __launch_bounds__(256) void k_str_tile_rows(const u64 * __restrict__ offsets, u64 n, u64 a0, u64 ntiles, u64 * __restrict__ tile_row)
{
    for (u64 t = (u64)blockIdx.x * 256 + threadIdx.x; t <= ntiles; t += (u64)gridDim.x * 256)
    {
        const u64 pos = t ? t * SM_TILE - a0 : 0;
        u64 lo = 0, hi = n;
        while (lo < hi)
        {
            const u64 mid = lo + ((hi - lo) >> 1);
            if (offsets[mid] > pos)
                hi = mid;
            else
                lo = mid + 1;
        }
        tile_row[t] = lo;
    }
}

__global__ __launch_bounds__(256) void k_str_contains_flat(const u64 * __restrict__ offsets, const u8 * __restrict__ chars, u64 n, u64 size,
                                                           const u64 * __restrict__ tile_row, u64 ntiles, const StrConst c, u8 hit_value, u8 * __restrict__ out)
{
    __shared__ uint4 s_tile4[(SM_TILE + SM_MAX + 16) / 16]; // the tile, the halo, 16 zero bytes for the last 8-byte read
    __shared__ u64 s_w[SM_MAX / 8];
    __shared__ u32 s_off[SM_ROWS_LDS];
    str_stage_const(s_w, c);
    const u32 m = c.len; // >= 1
    const u32 tid = threadIdx.x;
    const StrGrid g(chars, size);
    const u64 a0 = g.a0;
    const u64 first = 0x0101010101010101ull * (c.w[0] & 0xFF);
    const u64 * s_tile8 = (const u64 *)s_tile4;
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x)
    {
        const u64 r_lo = tile_row[t];
        if (r_lo >= n) // bytes after the last value
            break;
        const u64 r_next = tile_row[t + 1];
        const u64 r_hi = r_next < n ? r_next : n - 1; // the last row a start position of this tile can belong to
        const u64 cnt = r_hi - r_lo + 1;
        const u64 q0 = t * SM_TILE;
        const u64 pos0 = t ? q0 - a0 : 0;
        __syncthreads(); // the previous tile's readers are done (and the staged constant is visible)
        const uint4 v = str_load_chunk(g, q0 + tid * 16);
        s_tile4[tid] = v;
        if (tid <= SM_MAX / 16)
            s_tile4[SM_TILE / 16 + tid] = tid * 16 + 1 < m ? str_load_chunk(g, q0 + SM_TILE + tid * 16) : make_uint4(0, 0, 0, 0);
        const bool rows_in_lds = cnt <= SM_ROWS_LDS;
        if (rows_in_lds)
            for (u32 k = tid; k < cnt; k += 256)
            {
                const u64 d = offsets[r_lo + k] - pos0;
                s_off[k] = d > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)d;
            }
        __syncthreads();
        u32 cand = str_zero_bytes(((u64)v.x | ((u64)v.y << 32)) ^ first) | (str_zero_bytes(((u64)v.z | ((u64)v.w << 32)) ^ first) << 8);
        while (cand)
        {
            const u32 j = __builtin_ctz(cand);
            cand &= cand - 1;
            const u32 o = tid * 16 + j;
            if (q0 + o < a0)
                continue; // in front of chars
            const auto tile = [&](u32 k) { // the 8 bytes at byte o + k of the tile: two words of LDS, shifted together
                const u32 oo = o + k, sh = (oo & 7) * 8;
                const u64 lo = s_tile8[oo >> 3], hi = s_tile8[(oo >> 3) + 1];
                return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
            };
            if (!str_equals_words(tile, [&](u32 k) { return s_w[k >> 3]; }, m))
                continue;
            // the row of the hit: first row of this tile's rows whose end lies behind the hit
            const u64 rel = q0 + o - a0 - pos0; // < SM_TILE
            u64 lo = 0, hi = cnt;
            u64 row_end_rel = 0;
            if (rows_in_lds)
            {
                while (lo < hi)
                {
                    const u64 mid = (lo + hi) >> 1;
                    if (s_off[mid] > rel)
                        hi = mid;
                    else
                        lo = mid + 1;
                }
                if (lo < cnt)
                    row_end_rel = s_off[lo]; // saturated at 2^32 - 1: such a row ends far behind the hit
            }
            else
            {
                while (lo < hi)
                {
                    const u64 mid = (lo + hi) >> 1;
                    if (offsets[r_lo + mid] - pos0 > rel)
                        hi = mid;
                    else
                        lo = mid + 1;
                }
                if (lo < cnt)
                    row_end_rel = offsets[r_lo + lo] - pos0;
            }
            if (lo < cnt && rel + m + 1 <= row_end_rel) // wholly inside the value: not its terminating zero, not the next row
                out[r_lo + lo] = hit_value;
        }
    }
}

extern "C" int chgpu_like_compile(const void * pattern, uint64_t pattern_bytes, chgpu_like_plan * out)
{
    CHGPU_REQUIRE(out && (pattern || !pattern_bytes), CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    memset(out, 0, sizeof(*out));
    CHGPU_REQUIRE(pattern_bytes <= CHGPU_STR_CONST_MAX, CHGPU_ERR_NOT_IMPLEMENTED, "a LIKE pattern of %llu bytes (the kernels carry %d): CPU path",
                  (unsigned long long)pattern_bytes, CHGPU_STR_CONST_MAX);
    const u8 * p = (const u8 *)pattern;
    u32 nt = 0;
    auto push = [&](u8 byte, bool meta) {
        out->tokens[nt] = byte;
        if (meta)
            out->token_meta[nt >> 5] |= 1u << (nt & 31);
        ++nt;
    };
    auto is_meta = [&](u32 k) { return (out->token_meta[k >> 5] >> (k & 31)) & 1u; };
    for (u64 i = 0; i < pattern_bytes; ++i)
    {
        const u8 ch = p[i];
        if (ch == '\\')
        {
            // likePatternToRegexp: a pattern may not end in a lone backslash (CANNOT_PARSE_ESCAPE_SEQUENCE)
            CHGPU_REQUIRE(i + 1 < pattern_bytes, CHGPU_ERR_BAD_ARGUMENTS, "LIKE pattern ends in a lone backslash (an escape sequence is expected after it)");
            const u8 d = p[i + 1];
            if (d == '%' || d == '_' || d == '\\')
                push(d, false), ++i;
            else
                push('\\', false); // a literal backslash; the next byte is read as usual
        }
        else if (ch == '%')
        {
            ++out->n_percent;
            if (!(nt && is_meta(nt - 1) && out->tokens[nt - 1] == '%'))
                push('%', true);
        }
        else if (ch == '_')
            ++out->n_underscore, push('_', true);
        else
            push(ch, false);
    }
    out->n_tokens = nt;
    const bool lead = nt && is_meta(0) && out->tokens[0] == '%';
    u32 b = lead ? 1 : 0, e = nt;
    const bool trail = e > b && is_meta(e - 1) && out->tokens[e - 1] == '%';
    if (trail)
        --e;
    for (u32 k = b; k < e; ++k)
        if (is_meta(k))
        {
            out->route = CHGPU_STR_ROUTE_GENERAL;
            return CHGPU_OK;
        }
    out->literal_bytes = e - b;
    memcpy(out->literal, out->tokens + b, e - b);
    if (b == e && (lead || trail))
        out->route = CHGPU_STR_ROUTE_CONTAINS; // `%`, `%%`: contains the empty string
    else
        out->route = lead && trail ? CHGPU_STR_ROUTE_CONTAINS : lead ? CHGPU_STR_ROUTE_ENDS_WITH : trail ? CHGPU_STR_ROUTE_STARTS_WITH : CHGPU_STR_ROUTE_EQUALS;
    return CHGPU_OK;
}

// A predicate: the arguments all of them share, then `own_checks` (the entry point's), the walk over the offsets, and a UInt8 column of
// one byte per row, which `launch(col, mask) -> int` fills
template <class OwnChecks, class Launch>
static int str_predicate(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, const void * constant, u64 constant_bytes, OwnChecks && own_checks,
                         Launch && launch, chgpu_col ** out_u8)
{
    StrColumn col;
    CHGPU_TRY(str_column_begin(ctx, offsets_u64, chars_u8, out_u8 && (constant || !constant_bytes), [&] {
        CHGPU_REQUIRE(constant_bytes <= CHGPU_STR_CONST_MAX, CHGPU_ERR_NOT_IMPLEMENTED, "a string constant of %llu bytes (the kernels carry %d): CPU path",
                      (unsigned long long)constant_bytes, CHGPU_STR_CONST_MAX);
        return own_checks();
    }, &col));
    return str_one_column(ctx, "string predicate", CHGPU_U8, col.rows, [&](void * mask) { return launch(col, (u8 *)mask); }, out_u8);
}

static int str_launch_row(chgpu_ctx * ctx, const StrColumn & col, int mode, int op, const StrConst & c, int negate, u8 * out)
{
    const u64 n = col.rows;
    const dim3 grid(chgpu_grid_for(ctx, n, 256, 8)), block(256);
    if (mode == SM_CMP)
        hipLaunchKernelGGL(k_str_row_const<SM_CMP>, grid, block, 0, ctx->stream, col.offsets, col.chars, n, c, op, 0u, out);
    else if (mode == SM_STARTS)
        hipLaunchKernelGGL(k_str_row_const<SM_STARTS>, grid, block, 0, ctx->stream, col.offsets, col.chars, n, c, 0, (u32)(negate != 0), out);
    else
        hipLaunchKernelGGL(k_str_row_const<SM_ENDS>, grid, block, 0, ctx->stream, col.offsets, col.chars, n, c, 0, (u32)(negate != 0), out);
    ctx->counters[6] += 1;
    return CHGPU_OK;
}

static int str_launch_contains(chgpu_ctx * ctx, const StrColumn & col, u64 size, const StrConst & c, int negate, u8 * out)
{
    const u64 n = col.rows;
    CHGPU_HIP(hipMemsetAsync(out, (negate != 0) != (c.len == 0) ? 1 : 0, n, ctx->stream));
    if (c.len == 0) // the empty needle is found in every row
        return CHGPU_OK;
    const StrGrid g(col.chars, size);
    const u64 ntiles = (str_grid_chunks(g) + SM_TILE / 16 - 1) / (SM_TILE / 16);
    void * tile_row = nullptr;
    CHGPU_TRY(chgpu_scratch(ctx, (ntiles + 1) * sizeof(u64), &tile_row));
    hipLaunchKernelGGL(k_str_tile_rows, dim3(chgpu_grid_for(ctx, ntiles + 1, 256, 8)), dim3(256), 0, ctx->stream, col.offsets, n, g.a0, ntiles, (u64 *)tile_row);
    hipLaunchKernelGGL(k_str_contains_flat, dim3(chgpu_grid_for(ctx, ntiles * 256, 256, 8)), dim3(256), 0, ctx->stream, col.offsets, col.chars, n, size,
                       (const u64 *)tile_row, ntiles, c, (u8)(negate ? 0 : 1), out);
    ctx->counters[6] += 2;
    return CHGPU_OK;
}

static int str_launch_like(chgpu_ctx * ctx, const StrColumn & col, const StrConst & c, int negate, u8 * out)
{
    hipLaunchKernelGGL(k_str_like, dim3(chgpu_grid_for(ctx, col.rows, 256, 8)), dim3(256), 0, ctx->stream, col.offsets, col.chars, col.rows, c, (u32)(negate != 0), out);
    ctx->counters[6] += 1;
    return CHGPU_OK;
}

extern "C" int chgpu_string_cmp_const(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, int op, const void * value, uint64_t value_bytes,
                                      chgpu_col ** out_u8)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    return str_predicate(ctx, offsets_u64, chars_u8, value, value_bytes, [&] {
        CHGPU_REQUIRE(op >= CHGPU_EQ && op <= CHGPU_GE, CHGPU_ERR_BAD_ARGUMENTS, "unknown comparison %d", op);
        return (int)CHGPU_OK;
    }, [&](const StrColumn & col, u8 * mask) { return str_launch_row(ctx, col, SM_CMP, op, str_const_of(value, value_bytes), 0, mask); }, out_u8);
}

// every kind is a route of the LIKE plan; a needle is its own literal
static int str_match_plan(chgpu_ctx * ctx, int kind, const void * pattern, u64 pattern_bytes, chgpu_like_plan & plan)
{
    CHGPU_REQUIRE(kind >= CHGPU_STR_LIKE && kind <= CHGPU_STR_ENDS_WITH, CHGPU_ERR_BAD_ARGUMENTS, "unknown string predicate %d", kind);
    if (kind == CHGPU_STR_LIKE)
        CHGPU_TRY(chgpu_like_compile(pattern, pattern_bytes, &plan));
    else
    {
        memset(&plan, 0, sizeof(plan));
        plan.route = kind == CHGPU_STR_CONTAINS ? CHGPU_STR_ROUTE_CONTAINS : kind == CHGPU_STR_STARTS_WITH ? CHGPU_STR_ROUTE_STARTS_WITH : CHGPU_STR_ROUTE_ENDS_WITH;
        plan.literal_bytes = (u32)pattern_bytes;
        if (pattern_bytes)
            memcpy(plan.literal, pattern, pattern_bytes);
    }
    // developer option: a contains goes down the general matcher as %needle% (the measurement the router's choice rests on)
    if (plan.route == CHGPU_STR_ROUTE_CONTAINS && plan.literal_bytes && plan.literal_bytes + 2 <= CHGPU_STR_CONST_MAX && chgpu_opt(ctx, "tune_str_contains_general", 0))
    {
        memset(plan.token_meta, 0, sizeof(plan.token_meta));
        plan.n_tokens = plan.literal_bytes + 2;
        plan.tokens[0] = plan.tokens[plan.n_tokens - 1] = '%';
        memcpy(plan.tokens + 1, plan.literal, plan.literal_bytes);
        plan.token_meta[0] |= 1u;
        plan.token_meta[(plan.n_tokens - 1) >> 5] |= 1u << ((plan.n_tokens - 1) & 31);
        plan.route = CHGPU_STR_ROUTE_GENERAL;
    }
    return CHGPU_OK;
}

extern "C" int chgpu_string_match_const(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, int kind, const void * pattern,
                                        uint64_t pattern_bytes, int negate, chgpu_col ** out_u8)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    chgpu_like_plan plan;
    return str_predicate(ctx, offsets_u64, chars_u8, pattern, pattern_bytes, [&] { return str_match_plan(ctx, kind, pattern, pattern_bytes, plan); },
        [&](const StrColumn & col, u8 * mask) {
            if (plan.route == CHGPU_STR_ROUTE_GENERAL)
            {
                StrConst c = str_const_of(plan.tokens, plan.n_tokens);
                memcpy(c.meta, plan.token_meta, sizeof(c.meta));
                return str_launch_like(ctx, col, c, negate, mask);
            }
            const StrConst c = str_const_of(plan.literal, plan.literal_bytes);
            if (plan.route == CHGPU_STR_ROUTE_CONTAINS)
                return str_launch_contains(ctx, col, chars_u8->rows, c, negate, mask);
            if (plan.route == CHGPU_STR_ROUTE_EQUALS)
                return str_launch_row(ctx, col, SM_CMP, negate ? CHGPU_NE : CHGPU_EQ, c, 0, mask);
            return str_launch_row(ctx, col, plan.route == CHGPU_STR_ROUTE_STARTS_WITH ? SM_STARTS : SM_ENDS, 0, c, negate, mask);
        }, out_u8);
}
