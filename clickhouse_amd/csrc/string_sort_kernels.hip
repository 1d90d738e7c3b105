// string_sort_kernels.hip — SURVEY §8(f) rank 4 over Strings: ColumnString::getPermutation (src/Columns/ColumnString.cpp, the
// comparison sort over memcmpSmallAllowOverflow15 + length) and ColumnString::permute / index (ColumnString.cpp indexImpl), the two
// pieces sortBlock needs to order a Block by, or with, a String column.
//
// chgpu_string_sort_permutation is an MSD sort in 8-byte words whose every round is the stable LSD radix machinery of the numeric sort
// (chgpu_partition_by_key_byte) over the rows still undecided:
//   key of a row at word depth d = (word, c): word = bytes [8d, 8d+8) of the value read big-endian, bytes past the end as 0;
//                   c = min(9, max(0, len - 8d)).  Equal (word, c) with c <= 8 are equal strings: decided, incoming order kept.
//                   Equal word with c == 9 goes on to the next round.  c keeps "ab" apart from "ab\0", which a zero-padded word alone
//                   cannot.  Descending complements both parts (the comparison is reversed, never the row order among ties).
//   segment         a run of rows that were equal in every earlier round.  It owns a range of the output (start) and of the active arrays
//                   (first), and its own depth.  Round 0 has one segment: all rows.
//   k_ss_lcp        before a round, every active row counts the whole words it shares with its predecessor in the segment from the
//                   segment's depth on; the segment's minimum (one atomicMin per wave and segment) is skipped: the number of rounds does not grow with a prefix a
//                   whole segment shares (10^6 equal 1 KiB values: one round, not 128).
//   k_ss_keys       the unaligned 8-byte gather from chars (inside the column's pad at the last value) -> word, c
//   partition       stable passes over (word, c, segment, row): c, the 8 bytes of word, then as many bytes of the segment id as the
//                   segment count needs (none in round 0) -- the active rows end up ordered by (segment, word, c)
//   k_ss_heads      every active row goes to its final position, start + rank inside its segment; heads of runs of equal
//                   (segment, word, c) with c == 9 and more than one row (and a start below the limit) are the next segments
//   k_ss_segs / k_ss_active / k_ss_compact   two scans number the new segments and their rows; everything else has left the active set
// One read-back per round: (active rows, segments) of the next one.
// Algorithmic bytes per round over m active rows: 2 value gathers (lcp, keys) + (9 + segment-id bytes) passes x 21 B read and written
// + ~50 B per row of flags and scans.
//
// chgpu_string_index is a str_build_values of string_column.h, as filter, substring and concat are: sizes gathered through the indexes,
// the layout pass, one move pass.  (SsSegs and the layouts of a round's pool allocations are string_host.h's.)
#include "block_scan.h"
#include "string_column.h"

#include <algorithm>

static constexpr u64 SS_NONE = ~0ull;

__device__ __forceinline__ u64 ss_adv(const SsSegs & t, u32 s)
{
    const u64 a = t.adv[s];
    return a == SS_NONE ? 0 : a;
}

__global__ __launch_bounds__(256) void k_ss_init(const u64 * __restrict__ perm_in, u64 rows, u64 n, u64 * __restrict__ row, u32 * __restrict__ seg)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        u64 src = perm_in ? perm_in[i] : i;
        if (src >= rows)
            src = 0; // as k_sort_keys: a caller bug, no fault
        row[i] = src;
        seg[i] = 0;
    }
}

// Every wave folds what its lanes found for one segment into ONE atomicMin: in round 0 all rows belong to one segment, and a lane-wise
// atomicMin would queue every resident lane of the first sweep on a single address.
__global__ __launch_bounds__(256) void k_ss_lcp(const u64 * __restrict__ offsets, const u8 * __restrict__ chars, const u64 * __restrict__ row,
                                                const u32 * __restrict__ seg, u64 m, const SsSegs t)
{
    const u32 lane = lane_id();
    for (u64 base = (u64)blockIdx.x * 256; base < m; base += (u64)gridDim.x * 256) // uniform over the workgroup: the wave operations below see every lane
    {
        const u64 j = base + threadIdx.x;
        u32 s = 0;
        u64 k = 0;
        bool lower = false;
        if (j < m)
        {
            s = seg[j];
            const u64 cap = j == t.first[s] ? 0 : __hip_atomic_load(&t.adv[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cap) // a pair that shares `cap` words or more cannot lower the minimum
            {
                // (begin and length by hand, not through str_value: with it the kernel came out two instructions longer and the
                // two-round shape of tools/bench_string_sort.py 5 to 8 % slower in two sessions out of two)
                const u64 ra = row[j - 1], rb = row[j];
                const u64 ba = ra ? offsets[ra - 1] : 0, bb = rb ? offsets[rb - 1] : 0;
                const u64 la = offsets[ra] - ba - 1, lb = offsets[rb] - bb - 1;
                const u64 words = (la < lb ? la : lb) / 8; // whole words both values have
                const u64 d = t.depth[s];
                while (k < cap && d + k < words && str_load8(chars + ba + 8 * (d + k)) == str_load8(chars + bb + 8 * (d + k)))
                    ++k;
                lower = k < cap;
            }
        }
        u64 todo = __ballot(lower);
        for (u32 turn = 0; todo && turn < 4; ++turn)
        {
            const u32 leader = (u32)__ffsll((unsigned long long)todo) - 1;
            const u32 ls = __shfl(s, leader, WAVE);
            const bool mine = lower && s == ls;
            const u64 least = wave_reduce_all<MinU64>(mine ? k : SS_NONE);
            if (lane == leader)
                atomicMin((unsigned long long *)&t.adv[ls], (unsigned long long)least);
            lower = lower && !mine;
            todo = __ballot(lower);
        }
        if (lower) // a wave over more than four segments: they are short, and their minima live at different addresses
            atomicMin((unsigned long long *)&t.adv[s], (unsigned long long)k);
    }
}

__global__ __launch_bounds__(256) void k_ss_keys(const u64 * __restrict__ offsets, const u8 * __restrict__ chars, const u64 * __restrict__ row,
                                                 const u32 * __restrict__ seg, u64 m, const SsSegs t, int descending, u64 * __restrict__ word,
                                                 u8 * __restrict__ c)
{
    for (u64 j = (u64)blockIdx.x * 256 + threadIdx.x; j < m; j += (u64)gridDim.x * 256)
    {
        const u32 s = seg[j];
        const u64 d = t.depth[s] + ss_adv(t, s);
        const StrValue v = str_value(offsets, row[j]);
        const u64 begin = v.begin, len = v.size - 1;
        const u64 rem = len > 8 * d ? len - 8 * d : 0;
        u64 w = 0;
        if (rem)
        {
            // at least one byte of the value is left, so the load ends at most 7 bytes behind it: the terminating zero + the 8-byte pad
            w = __builtin_bswap64(str_load8(chars + begin + 8 * d));
            if (rem < 8)
                w &= ~0ull << (8 * (8 - rem));
        }
        const u32 cc = rem < 9 ? (u32)rem : 9u;
        word[j] = descending ? ~w : w;
        c[j] = (u8)(descending ? 9u - cc : cc);
    }
}

__global__ __launch_bounds__(256) void k_ss_heads(const u64 * __restrict__ word, const u8 * __restrict__ c, const u32 * __restrict__ seg,
                                                  const u64 * __restrict__ row, u64 m, const SsSegs t, u32 cont, u64 limit, u64 n_out,
                                                  u64 * __restrict__ out, u32 * __restrict__ new_head)
{
    for (u64 j = (u64)blockIdx.x * 256 + threadIdx.x; j < m; j += (u64)gridDim.x * 256)
    {
        const u32 s = seg[j];
        const u64 w = word[j];
        const u32 cc = c[j];
        const u64 pos = t.start[s] + (j - t.first[s]);
        if (pos < n_out)
            out[pos] = row[j];
        const bool head = j == 0 || seg[j - 1] != s || word[j - 1] != w || c[j - 1] != cc;
        const bool more = j + 1 < m && seg[j + 1] == s && word[j + 1] == w && c[j + 1] == cc;
        new_head[j] = head && more && cc == cont && pos < limit;
    }
}

// ns: the next round's segments, numbered by the inclusive scan of new_head
__global__ __launch_bounds__(256) void k_ss_segs(const u32 * __restrict__ new_head, const u64 * __restrict__ seg_no, const u32 * __restrict__ seg, u64 m,
                                                 const SsSegs t, const SsSegs ns)
{
    for (u64 j = (u64)blockIdx.x * 256 + threadIdx.x; j < m; j += (u64)gridDim.x * 256)
    {
        if (!new_head[j])
            continue;
        const u32 s = seg[j];
        const u64 k = seg_no[j] - 1;
        ns.start[k] = t.start[s] + (j - t.first[s]);
        ns.depth[k] = t.depth[s] + ss_adv(t, s) + 1;
        ns.adv[k] = SS_NONE;
        ns.head[k] = j;
    }
}

// a row stays active when the last new segment head at or before it heads its own run
__global__ __launch_bounds__(256) void k_ss_active(const u64 * __restrict__ word, const u8 * __restrict__ c, const u32 * __restrict__ seg,
                                                   const u64 * __restrict__ seg_no, u64 m, const SsSegs ns, u32 cont, u32 * __restrict__ active)
{
    for (u64 j = (u64)blockIdx.x * 256 + threadIdx.x; j < m; j += (u64)gridDim.x * 256)
    {
        const u64 k = seg_no[j];
        bool a = false;
        if (k && c[j] == cont)
        {
            const u64 h = ns.head[k - 1];
            a = h <= j && seg[h] == seg[j] && word[h] == word[j];
        }
        active[j] = a;
    }
}

__global__ __launch_bounds__(256) void k_ss_compact(const u32 * __restrict__ active, const u64 * __restrict__ slot, const u32 * __restrict__ new_head,
                                                    const u64 * __restrict__ seg_no, const u64 * __restrict__ row, u64 m, const SsSegs ns,
                                                    u64 * __restrict__ row_out, u32 * __restrict__ seg_out)
{
    for (u64 j = (u64)blockIdx.x * 256 + threadIdx.x; j < m; j += (u64)gridDim.x * 256)
    {
        if (!active[j])
            continue;
        const u64 k = slot[j];
        row_out[k] = row[j];
        seg_out[k] = (u32)(seg_no[j] - 1);
        if (new_head[j])
            ns.first[seg_no[j] - 1] = k;
    }
}

typedef StrCols<4> SsCols; // the active rows: word, c, segment, row

// one stable pass over all four columns by a byte of column `key`
static int ss_pass(PairAllocs & mem, SsCols & a, int key, u32 shift)
{
    chgpu_col * out[4] = {nullptr, nullptr, nullptr, nullptr};
    CHGPU_TRY(mem.refused()); // the pass allocates inside: one number for all of it
    CHGPU_TRY(chgpu_partition_by_key_byte(mem.ctx, a.v[key], shift, 4, a.v, out));
    a.drop();
    for (int i = 0; i < 4; ++i)
        a.v[i] = out[i];
    return CHGPU_OK;
}

extern "C" int chgpu_string_sort_permutation(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, const chgpu_col * perm_in_u64,
                                             int descending, uint64_t limit, chgpu_col ** perm_out_u64)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    StrColumn col;
    CHGPU_TRY(str_column_begin(ctx, offsets_u64, chars_u8, perm_out_u64 != nullptr, [&] {
        CHGPU_REQUIRE(!perm_in_u64 || perm_in_u64->type == CHGPU_U64, CHGPU_ERR_BAD_ARGUMENTS, "a permutation is a UInt64 column (IColumn::Permutation)");
        CHGPU_REQUIRE(!perm_in_u64 || perm_in_u64->rows <= offsets_u64->rows, CHGPU_ERR_SIZES_MISMATCH, "Size of permutation (%llu) is greater than the column (%llu)",
                      (unsigned long long)(perm_in_u64 ? perm_in_u64->rows : 0), (unsigned long long)offsets_u64->rows);
        CHGPU_REQUIRE((perm_in_u64 ? perm_in_u64->rows : offsets_u64->rows) < (1ull << 32), CHGPU_ERR_NOT_IMPLEMENTED, "2^32 rows or more in one String sort");
        return (int)CHGPU_OK;
    }, &col));
    const u64 n = perm_in_u64 ? perm_in_u64->rows : col.rows;
    const u64 lim = limit && limit < n ? limit : SS_NONE;
    const u32 cont = descending ? 0u : 9u;

    PairAllocs mem = str_call(ctx, "string sort");
    PairTemps hold(mem);
    StrCols<> out_guard; // the permutation
    chgpu_col *& out = out_guard.v[0];
    CHGPU_TRY(mem.col_new(CHGPU_U64, n, &out));
    if (n == 0)
    {
        out_guard.give(perm_out_u64);
        return CHGPU_OK;
    }

    SsCols act;
    SsSegs segs;
    CHGPU_TRY(str_carve(hold, [&](uintptr_t base) { return ss_segs_lay(base, 1, &segs); }));
    CHGPU_HIP(hipMemsetAsync(segs.start, 0, 256 * 3, ctx->stream));              // start = first = depth = 0
    CHGPU_HIP(hipMemsetAsync(segs.adv, 0xFF, 8, ctx->stream));
    u64 m = n, n_segs = 1;
    CHGPU_TRY(mem.col_new(CHGPU_U64, m, &act.v[3]));
    CHGPU_TRY(mem.col_new(CHGPU_U32, m, &act.v[2]));
    hipLaunchKernelGGL(k_ss_init, dim3(chgpu_grid_for(ctx, m, 256, 8)), dim3(256), 0, ctx->stream, perm_in_u64 ? (const u64 *)perm_in_u64->data : nullptr, col.rows, m,
                       (u64 *)act.v[3]->data, (u32 *)act.v[2]->data);
    ctx->counters[6] += 1;

    while (m)
    {
        const u32 grid = chgpu_grid_for(ctx, m, 256, 8);
        CHGPU_TRY(mem.col_new(CHGPU_U64, m, &act.v[0]));
        CHGPU_TRY(mem.col_new(CHGPU_U8, m, &act.v[1]));
        hipLaunchKernelGGL(k_ss_lcp, dim3(grid), dim3(256), 0, ctx->stream, col.offsets, col.chars, (const u64 *)act.v[3]->data, (const u32 *)act.v[2]->data, m, segs);
        hipLaunchKernelGGL(k_ss_keys, dim3(grid), dim3(256), 0, ctx->stream, col.offsets, col.chars, (const u64 *)act.v[3]->data, (const u32 *)act.v[2]->data, m, segs,
                           descending, (u64 *)act.v[0]->data, (u8 *)act.v[1]->data);
        ctx->counters[6] += 2;
        CHGPU_TRY(ss_pass(mem, act, 1, 0));
        for (u32 b = 0; b < 8; ++b)
            CHGPU_TRY(ss_pass(mem, act, 0, b * 8));
        for (u32 b = 0; b < 4 && ((n_segs - 1) >> (8 * b)); ++b)
            CHGPU_TRY(ss_pass(mem, act, 2, b * 8));

        // flags, scans and the next round's segment table
        const size_t b_tmp = chgpu_scan_tmp_bytes(m);
        SsRoundLayout l;
        CHGPU_TRY(str_carve(hold, [&](uintptr_t base) { return ss_round_lay(base, m, b_tmp, &l); }));
        SsSegs next;
        CHGPU_TRY(str_carve(hold, [&](uintptr_t base) { return ss_segs_lay(base, m / 2 + 1, &next); }));
        const u64 * word = (const u64 *)act.v[0]->data;
        const u8 * c = (const u8 *)act.v[1]->data;
        const u32 * seg = (const u32 *)act.v[2]->data;
        const u64 * row = (const u64 *)act.v[3]->data;
        hipLaunchKernelGGL(k_ss_heads, dim3(grid), dim3(256), 0, ctx->stream, word, c, seg, row, m, segs, cont, lim, n, (u64 *)out->data, l.new_head);
        CHGPU_TRY(chgpu_scan_inclusive_u32_u64(ctx, l.new_head, l.seg_no, m, l.totals, l.scan_tmp, b_tmp));
        hipLaunchKernelGGL(k_ss_segs, dim3(grid), dim3(256), 0, ctx->stream, (const u32 *)l.new_head, (const u64 *)l.seg_no, seg, m, segs, next);
        hipLaunchKernelGGL(k_ss_active, dim3(grid), dim3(256), 0, ctx->stream, word, c, seg, (const u64 *)l.seg_no, m, next, cont, l.active);
        CHGPU_TRY(chgpu_scan_exclusive_u32_u64(ctx, l.active, l.slot, m, l.totals + 1, l.scan_tmp, b_tmp));
        ctx->counters[6] += 3;
        u64 host_totals[2] = {0, 0};
        CHGPU_TRY(chgpu_read_back(ctx, l.totals, host_totals, sizeof(host_totals)));
        CHGPU_HIP(hipGetLastError());
        const u64 m_next = host_totals[1];
        CHGPU_REQUIRE(m_next <= m && host_totals[0] <= m / 2, CHGPU_ERR_LOGICAL, "string sort: a round grew its active set");
        if (m_next)
        {
            StrCols<> next_rows; // row, segment
            CHGPU_TRY(mem.col_new(CHGPU_U64, m_next, &next_rows.v[0]));
            CHGPU_TRY(mem.col_new(CHGPU_U32, m_next, &next_rows.v[1]));
            hipLaunchKernelGGL(k_ss_compact, dim3(grid), dim3(256), 0, ctx->stream, (const u32 *)l.active, (const u64 *)l.slot, (const u32 *)l.new_head,
                               (const u64 *)l.seg_no, row, m, next, (u64 *)next_rows.v[0]->data, (u32 *)next_rows.v[1]->data);
            ctx->counters[6] += 1;
            act.drop(); // back to the pool; reuse is ordered behind the kernel above on this stream
            next_rows.give(&act.v[3], &act.v[2]);
        }
        else
            act.drop();
        hold.release(l.new_head);
        hold.release(segs.start);
        segs = next;
        n_segs = host_totals[0];
        m = m_next;
    }
    if (lim != SS_NONE)
        out->rows = lim; // IColumn::Permutation is simply cut (the buffer keeps its size class)
    out_guard.give(perm_out_u64);
    return CHGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// ColumnString::permute / index (ColumnString.cpp:300-360, indexImpl): out[i] = value[indexes[i]] as a new ColumnString.
//   k_str_index_sizes   bytes[i] = size of value indexes[i] incl. its zero; an index >= rows raises a flag and takes no bytes
//   k_str_index_move    out_offsets[i] = pos + size; the value travels 8 bytes per step while 8 whole bytes are left, the rest byte by
//                       byte: nothing is written behind the value's own terminating zero
// Algorithmic bytes: 8 (index) + 16 (two offsets, gathered) per row + the values read and written + 8 per row.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_str_index_sizes(const u64 * __restrict__ offsets, u64 rows, const u64 * __restrict__ indexes, u64 n,
                                                         u32 * __restrict__ bytes, u32 * __restrict__ bad_index, u32 * __restrict__ too_long)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        const u64 r = indexes[i];
        u64 sz = 0;
        if (r >= rows)
            *bad_index = 1;
        else
            sz = str_value(offsets, r).size;
        bytes[i] = str_size_u32(sz, too_long);
    }
}

__global__ __launch_bounds__(256) void k_str_index_move(const u64 * __restrict__ offsets, const u8 * __restrict__ chars, const u64 * __restrict__ indexes,
                                                        const u32 * __restrict__ bytes, const u64 * __restrict__ byte_pos, u64 n,
                                                        u64 * __restrict__ out_offsets, u8 * __restrict__ out_chars)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        const u64 sz = bytes[i]; // 0 only for an index the sizes pass flagged: the call fails, nothing is read through it
        const u64 dst = byte_pos[i];
        out_offsets[i] = dst + sz;
        if (sz)
            str_copy_value(out_chars + dst, chars + str_value(offsets, indexes[i]).begin, sz);
    }
}

extern "C" int chgpu_string_index(chgpu_ctx * ctx, const chgpu_col * offsets_u64, const chgpu_col * chars_u8, const chgpu_col * indexes_u64, uint64_t limit,
                                  chgpu_col ** out_offsets_u64, chgpu_col ** out_chars_u8)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    StrColumn col;
    CHGPU_TRY(str_column_begin(ctx, offsets_u64, chars_u8, indexes_u64 && out_offsets_u64 && out_chars_u8, [&] {
        CHGPU_REQUIRE(indexes_u64->type == CHGPU_U64, CHGPU_ERR_BAD_ARGUMENTS, "the indexes are a UInt64 column");
        return (int)CHGPU_OK;
    }, &col));
    const u64 n = limit && limit < indexes_u64->rows ? limit : indexes_u64->rows;
    const dim3 grid(chgpu_grid_for(ctx, n, 256, 8)), block(256);
    const u64 * indexes = (const u64 *)indexes_u64->data;
    return str_build_values(ctx, "string index", n, col.rows,
        [&](const StrValuesLayout & l) {
            hipLaunchKernelGGL(k_str_index_sizes, grid, block, 0, ctx->stream, col.offsets, col.rows, indexes, n, l.sizes, (u32 *)&l.words->bad_index,
                               (u32 *)&l.words->too_long);
        },
        [&](const StrValuesLayout & l, StrCols<> & out) {
            hipLaunchKernelGGL(k_str_index_move, grid, block, 0, ctx->stream, col.offsets, col.chars, indexes, (const u32 *)l.sizes, (const u64 *)l.pos, n,
                               (u64 *)out.v[0]->data, (u8 *)out.v[1]->data);
        },
        out_offsets_u64, out_chars_u8);
}
