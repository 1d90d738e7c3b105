// merge_versioned_kernels.hip — the merge of VersionedCollapsingMergeTree (src/Processors/Merges/Algorithms/VersionedCollapsingAlgorithm.cpp):
// within a group of equal sort columns, the version included, a row of one sign cancels the nearest unmatched earlier row of the other, and
// every unmatched row survives -- any number of rows of a group, each living or dying on its own.  In front of it everything is the folding
// merges', through their call frame (FoldCall of merge_keys.h): the merged order M as (key word, row) pairs (merge_kernels.hip), the sign
// check, the group heads (merge_fold_kernels.hip); so are the offsets step behind the tile counts and the tail of the emit.
// Behind the heads, over the tiles of FOLD_TILE positions, a thread owning FOLD_ITEMS consecutive ones:
//   k_vc_tile     the signs of the tile's rows gathered ONCE in position order (a wave's lanes read consecutive row numbers, and a ballot
//                 turns their signs into 64 bits in LDS), kept as one bit a position for the pass below; the tile as one element of the
//                 forward scan (VcSum: the balance since the last head) and one of the backward scan (VcAfter: the sum and the extreme
//                 prefix sums of the part in front of the first head)
//   k_vc_carry    one workgroup per scan, FOLD_THREADS tiles a pass with the carry of the passes in LDS: VcSum of the tiles in front of
//                 every tile, VcAfter of those behind it
//   k_vc_decide   the tile again between its two carries: every position's balance and what follows it in its group give the survive
//                 rule; one mask byte a thread, the tile's survivor count and its largest |balance|
//   (k_fold_offsets of merge_fold_kernels.hip: the exclusive sum of the tile counts, the total, and the maximum of the tiles' |balance|)
//   k_vc_emit     the surviving row numbers of a tile, compacted through LDS and stored coalesced as UInt64 at the tile's offset
// The states, the combines, the survive rule and the threads' walks are merge_versioned_host.h's; the scans inside a workgroup are
// block_scan.h's.  No atomics; nothing depends on which workgroup runs first.
// Algorithmic bytes per row behind the heads: tile 4 (row number) + 1 (sign, gathered) + 1 (head) + 1/8; decide 1 + 1/8 + 1/8; emit 1/8 +
// 4 where a thread has a survivor + 8 per survivor: 11.5 + 8 per survivor.  Storing the balance as a column instead (8 bytes written, then
// read by the backward scan's tile pass and again by its apply pass) would add 24 bytes a row, which is why the backward scan carries
// prefix sums and the balance is recomputed inside the tile from the tile's carry.
#include "merge_versioned_host.h"
#include "merge_keys.h"

// ---------------------------------------------------------------------------------------------
// the two scans as block_scan.h Ops
// ---------------------------------------------------------------------------------------------
struct VcSumOp
{
    typedef VcSum T;
    static __device__ __forceinline__ T id() { return vc_sum_id(); }
    static __device__ __forceinline__ T comb(T a, T b) { return vc_sum_combine(a, b); }
};
// scanned from the far end of M: what the scan met earlier lies LATER in M
struct VcAfterBackOp
{
    typedef VcAfter T;
    static __device__ __forceinline__ T id() { return vc_after_id(); }
    static __device__ __forceinline__ T comb(T a, T b) { return vc_after_combine(b, a); }
};
__device__ __forceinline__ VcSum shfl_up(VcSum v, int d) { return VcSum{(i64)shfl_up((u64)v.sum, d), shfl_up(v.head, d)}; }
__device__ __forceinline__ VcAfter shfl_up(VcAfter v, int d)
{
    return VcAfter{(i64)shfl_up((u64)v.sum, d), (i64)shfl_up((u64)v.mn, d), (i64)shfl_up((u64)v.mx, d), shfl_up(v.closed, d)};
}

struct VcScanLds
{
    VcSum f[FOLD_THREADS / WAVE];
    VcAfter g[FOLD_THREADS / WAVE];
    VcAfter turn[FOLD_THREADS];
};

// From every thread's two elements: before = VcSum of the tile's positions in front of the thread's, after = VcAfter of those behind them,
// and the tile's own two elements.  The backward scan is the forward one over the threads in reverse: thread t scans for thread
// FOLD_THREADS - 1 - t, and the elements change hands through LDS.
__device__ __forceinline__ void vc_block_scans(const VcSum & f, const VcAfter & g, VcScanLds & lds, VcSum & before, VcAfter & after, VcSum & tile_f, VcAfter & tile_g)
{
    before = block_scan_exclusive<VcSumOp>(f, lds.f, &tile_f);
    const u32 t = threadIdx.x, r = FOLD_THREADS - 1 - t;
    lds.turn[t] = g;
    __syncthreads();
    const VcAfter theirs = lds.turn[r];
    const VcAfter behind = block_scan_exclusive<VcAfterBackOp>(theirs, lds.g, &tile_g);  // (its barriers stand between the reads above and the writes below)
    lds.turn[r] = behind;
    __syncthreads();
    after = lds.turn[t];
}

// the thread's positions [p0, p0 + FOLD_ITEMS) cut at n: the head bytes as one word, and how many positions are real
__device__ __forceinline__ VcItems vc_items_heads(const u8 * __restrict__ heads, u32 n)
{
    u64 p0, p1;
    fold_thread_range(blockIdx.x, threadIdx.x, n, p0, p1);
    VcItems it{0, 0, (u32)(p1 - p0)};
    if (it.count == FOLD_ITEMS)
        it.heads = *(const u64 *)(heads + p0);  // p0 is a multiple of 8 and the array begins a pool allocation
    else
        for (u32 i = 0; i < it.count; ++i)
            it.heads |= (u64)heads[p0 + i] << (8 * i);
    return it;
}

__global__ __launch_bounds__(FOLD_THREADS) void k_vc_tile(const i8 * __restrict__ sign, const u8 * __restrict__ heads, const u32 * __restrict__ rows, u32 n,
                                                          u8 * __restrict__ positive, VcSum * __restrict__ agg_f, VcAfter * __restrict__ agg_g)
{
    __shared__ u64 lbits[FOLD_TILE / WAVE];  // bit e: position base + e is a +1 row
    __shared__ VcScanLds lds;
    const u64 base = (u64)blockIdx.x * FOLD_TILE;
    for (u32 k = 0; k < FOLD_ITEMS; ++k)
    {
        const u32 e = k * FOLD_THREADS + threadIdx.x;  // a wave: 64 consecutive positions
        const bool plus = base + e < n && sign[rows[base + e]] == 1;
        const u64 ballot = __ballot(plus);
        if ((threadIdx.x & (WAVE - 1)) == 0)
            lbits[e / WAVE] = ballot;
    }
    __syncthreads();
    VcItems it = vc_items_heads(heads, n);
    it.positive = ((const u8 *)lbits)[threadIdx.x];  // positions 8 t .. 8 t + 7
    positive[(u64)blockIdx.x * FOLD_THREADS + threadIdx.x] = (u8)it.positive;
    VcSum f, before, tile_f;
    VcAfter g, after, tile_g;
    vc_aggregate(it, f, g);
    vc_block_scans(f, g, lds, before, after, tile_f, tile_g);
    if (threadIdx.x == 0)
    {
        agg_f[blockIdx.x] = tile_f;
        agg_g[blockIdx.x] = tile_g;
    }
}

// in place: f[t] := VcSum of the tiles in front of t, g[t] := VcAfter of the tiles behind t.  Two workgroups, one scan each: the two
// share nothing, and a scan of one workgroup is a chain of passes that wait on each other
__global__ __launch_bounds__(FOLD_THREADS) void k_vc_carry(VcSum * __restrict__ f, VcAfter * __restrict__ g, u32 n_tiles)
{
    if (blockIdx.x == 0)
        block_scan_array<VcSumOp, false>(f, f, n_tiles, vc_sum_id());
    else
        block_scan_array<VcAfterBackOp, true>(g, g, n_tiles, vc_after_id());
}

__global__ __launch_bounds__(FOLD_THREADS) void k_vc_decide(const u8 * __restrict__ heads, const u8 * __restrict__ positive, u32 n, const VcSum * __restrict__ carry_f,
                                                            const VcAfter * __restrict__ carry_g, u8 * __restrict__ masks, u32 * __restrict__ tile_counts,
                                                            u64 * __restrict__ tile_max)
{
    __shared__ VcScanLds lds;
    __shared__ u32 lcount[FOLD_THREADS / WAVE];
    __shared__ u64 lmax[FOLD_THREADS / WAVE];
    const u64 slot = (u64)blockIdx.x * FOLD_THREADS + threadIdx.x;
    VcItems it = vc_items_heads(heads, n);
    it.positive = positive[slot];
    VcSum f, before, tile_f;
    VcAfter g, after, tile_g;
    vc_aggregate(it, f, g);
    vc_block_scans(f, g, lds, before, after, tile_f, tile_g);
    before = vc_sum_combine(carry_f[blockIdx.x], before);
    after = vc_after_combine(after, carry_g[blockIdx.x]);
    u64 max_abs = 0;
    const u32 mask = vc_decide(it, before, after, &max_abs);
    masks[slot] = (u8)mask;
    const u32 total = block_reduce<AddU32>((u32)__popc(mask), lcount);
    max_abs = block_reduce<MaxU64>(max_abs, lmax);
    if (threadIdx.x == 0)
    {
        tile_counts[blockIdx.x] = total;
        tile_max[blockIdx.x] = max_abs;
    }
}

__global__ __launch_bounds__(FOLD_THREADS) void k_vc_emit(const u8 * __restrict__ masks, const u32 * __restrict__ rows, u32 n, const u64 * __restrict__ tile_offsets,
                                                          u64 * __restrict__ out)
{
    __shared__ u32 stage[FOLD_TILE];
    __shared__ u32 lcount[FOLD_THREADS / WAVE];
    const u32 mask = masks[(u64)blockIdx.x * FOLD_THREADS + threadIdx.x];
    u32 total = 0;
    u32 at = block_scan_exclusive<AddU32>((u32)__popc(mask), lcount, &total);
    if (mask)
    {
        u64 p0, p1;
        fold_thread_range(blockIdx.x, threadIdx.x, n, p0, p1);
        u32 r[FOLD_ITEMS] = {};
        if (p1 - p0 == FOLD_ITEMS)
        {
            const uint4 lo = *(const uint4 *)(rows + p0), hi = *(const uint4 *)(rows + p0 + 4);  // 32-byte aligned: p0 is a multiple of 8
            r[0] = lo.x, r[1] = lo.y, r[2] = lo.z, r[3] = lo.w, r[4] = hi.x, r[5] = hi.y, r[6] = hi.z, r[7] = hi.w;
        }
        else
            for (u32 i = 0; i < FOLD_ITEMS; ++i)  // a mask bit is only ever set below n
                if (p0 + i < p1)
                    r[i] = rows[p0 + i];
        for (u32 i = 0; i < FOLD_ITEMS; ++i)
            if ((mask >> i) & 1)
                stage[at++] = r[i];  // at < total <= FOLD_TILE
    }
    fold_store_staged(stage, total, out, tile_offsets[blockIdx.x], true);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
extern "C" int chgpu_merge_versioned_collapsing(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const int32_t * descending, const int32_t * nan_direction_hint,
                                                uint32_t n_keys, const uint64_t * run_offsets, uint32_t n_runs, uint32_t flags, const chgpu_col * sign_i8,
                                                chgpu_col ** rows_out_u64, uint64_t * max_balance)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    CHGPU_REQUIRE(rows_out_u64 && sign_i8, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    FoldPrefix px;
    CHGPU_TRY(fold_validate(ctx, key_cols, descending, nan_direction_hint, n_keys, run_offsets, n_runs, flags, &px));
    CHGPU_TRY(fold_check_column(sign_i8, "sign", CHGPU_I8, "Int8", px.rows));
    FoldCall call(ctx, "merge_versioned_collapsing");
    const u32 n = (u32)px.rows;
    const int sign_mode = 0;
    CHGPU_TRY(call.open(key_cols, px, run_offsets, n_runs, flags, &sign_i8, &sign_mode, 1));
    const u32 tiles = call.tiles;
    u64 result[2] = {0, 0};  // the survivors, the greatest |balance|
    const u64 * tile_off = nullptr;
    void * masks = nullptr;
    if (n)
    {
        void * positive = nullptr, * agg_f = nullptr, * agg_g = nullptr, * counts = nullptr, * tile_max = nullptr;
        CHGPU_TRY(call.tmp.alloc((size_t)tiles * FOLD_THREADS, &positive));
        CHGPU_TRY(call.tmp.alloc((size_t)tiles * FOLD_THREADS, &masks));
        CHGPU_TRY(call.tmp.alloc((size_t)tiles * sizeof(VcSum), &agg_f));
        CHGPU_TRY(call.tmp.alloc((size_t)tiles * sizeof(VcAfter), &agg_g));
        CHGPU_TRY(call.tmp.alloc((size_t)tiles * sizeof(u32), &counts));
        CHGPU_TRY(call.tmp.alloc((size_t)tiles * sizeof(u64), &tile_max));
        hipLaunchKernelGGL(k_vc_tile, dim3(tiles), dim3(FOLD_THREADS), 0, ctx->stream, (const i8 *)sign_i8->data, (const u8 *)call.heads, call.rows, n, (u8 *)positive,
                           (VcSum *)agg_f, (VcAfter *)agg_g);
        hipLaunchKernelGGL(k_vc_carry, dim3(2), dim3(FOLD_THREADS), 0, ctx->stream, (VcSum *)agg_f, (VcAfter *)agg_g, tiles);
        hipLaunchKernelGGL(k_vc_decide, dim3(tiles), dim3(FOLD_THREADS), 0, ctx->stream, (const u8 *)call.heads, (const u8 *)positive, n, (const VcSum *)agg_f,
                           (const VcAfter *)agg_g, (u8 *)masks, (u32 *)counts, (u64 *)tile_max);
        ctx->counters[6] += 3;
        CHGPU_TRY(fold_offsets(ctx, call.tmp, (const u32 *)counts, (const u64 *)tile_max, tiles, &tile_off, result));
    }
    chgpu_col * out = nullptr;
    int rc = chgpu_col_new(ctx, CHGPU_U64, result[0], &out);
    if (rc == CHGPU_OK && result[0])
    {
        hipLaunchKernelGGL(k_vc_emit, dim3(tiles), dim3(FOLD_THREADS), 0, ctx->stream, (const u8 *)masks, call.rows, n, tile_off, (u64 *)out->data);
        ctx->counters[6] += 1;
    }
    CHGPU_TRY(call.close(rc, &out, 1));
    *rows_out_u64 = out;
    if (max_balance)
        *max_balance = result[1];
    return CHGPU_OK;
}
