// merge_fold_kernels.hip — the merges of MergeTree that fold rows of equal sorting key while they merge: ReplacingSortedAlgorithm,
// CollapsingSortedAlgorithm, SummingSortedAlgorithm and AggregatingSortedAlgorithm over SimpleAggregateFunction columns
// (src/Processors/Merges/Algorithms/{ReplacingSorted,CollapsingSorted,SummingSorted,AggregatingSorted}Algorithm.cpp).  One operator:
// merge (merge_kernels.hip gives the merged order M as (key word, row) pairs), find the groups of equal key, fold each group by the
// algorithm's rule, write the surviving rows compacted and still in order.
//   k_fold_bad      sign / is_deleted: per-tile minimum of the row that holds a value outside the domain (then k_merge_min)
//   k_fold_heads    one flag per position of M: the first key's word against its predecessor's; the further key columns are gathered
//                   through the row numbers only where the words tie
//   k_fold_tile     a tile's positions as ONE scan element {flags, state}: the states are loaded in position order into LDS (states of at
//                   most 16 bytes, Collapsing's excepted; the others are read in place), thread-local fold, then a segmented scan over the workgroup
//   k_fold_carry    one workgroup: the segmented scan of the tile elements -> the state of the group open at every tile's start
//   k_fold_apply    the tile again behind its carry; a group's result is known at its TAIL, which emits 0, 1 or 2 outputs.
//                   EMIT = false: the tile's and its threads' output counts.  EMIT = true: the outputs, compacted through LDS, stored
//                   coalesced at the tile's offset; the folding form stores its result columns through the same offsets
//   k_fold_offsets  one workgroup: the exclusive sum of the tile counts, the total and, where the caller has per-tile maxima
//                   (merge_versioned_kernels.hip), their maximum
// The states, the combine operators, the walks and a thread's positions are merge_fold_host.h's.  No atomics; nothing depends on which
// workgroup runs first.  Host side: FoldCall (merge_keys.h) is the frame of a call -- the checks, the merged order, the heads, the
// epilogue -- for fold_run here and for the VersionedCollapsing merge, and fold_offsets the step behind the tile counts.
// Algorithmic bytes per row behind the merge: heads 12 + 1; tile 1 + 4 + the gathered columns; apply twice the same (+ 1 / 8 for the
// threads' counts); outputs 8 per row number and the value widths per surviving group.
#include "merge_fold_host.h"
#include "merge_keys.h"

// mode 0: Int8 sign, bad unless +1 or -1; mode 1: UInt8 is_deleted, bad unless 0 or 1
__global__ __launch_bounds__(FOLD_THREADS) void k_fold_bad(const u8 * __restrict__ col, int mode, u32 n, u64 * __restrict__ partial)
{
    __shared__ u64 lds[FOLD_THREADS / WAVE];
    u64 found = ~0ull;
    for (u32 t = 0; t < FOLD_ITEMS; ++t)
    {
        const u64 i = (u64)blockIdx.x * FOLD_TILE + (u64)t * FOLD_THREADS + threadIdx.x;
        if (i >= n)
            break;
        const u8 v = col[i];
        const bool bad = mode == 0 ? (v != 1 && v != 0xFF) : v > 1;
        if (bad && found == ~0ull)
            found = i;
    }
    const u64 m = block_reduce<MinU64>(found, lds);
    if (threadIdx.x == 0)
        partial[blockIdx.x] = m;
}

__global__ __launch_bounds__(256) void k_fold_heads(MergeKeys keys, const u64 * __restrict__ words, const u32 * __restrict__ rows, u32 n, u8 * __restrict__ heads)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        bool head = i == 0 || words[i] != words[i - 1];
        if (!head && keys.n > 1)
        {
            const u32 r = rows[i], q = rows[i - 1];
            for (u32 j = 1; j < keys.n && !head; ++j)
                head = mrg_key(keys, j, r) != mrg_key(keys, j, q);
        }
        heads[i] = head ? 1 : 0;
    }
}

// inclusive segmented scan of the threads' elements; afterwards ls / lf hold every thread's inclusive element
// (not block_scan.h's: a state reaches 72 bytes, too wide for shuffles, and the callers read their neighbour's element from ls / lf)
template <class A>
__device__ __forceinline__ void fold_block_scan(const A & a, typename A::State & s, u8 & fl, typename A::State * ls, u8 * lf)
{
    const u32 t = threadIdx.x;
    ls[t] = s;
    lf[t] = fl;
    __syncthreads();
    for (u32 d = 1; d < FOLD_THREADS; d <<= 1)
    {
        typename A::State ps = s;
        u8 pf = 0;
        if (t >= d)
        {
            ps = ls[t - d];
            pf = lf[t - d];
        }
        __syncthreads();
        if (t >= d)
        {
            fold_seg_combine(a, ps, pf, s, fl);
            s = ps;
            fl = pf;
            ls[t] = s;
            lf[t] = fl;
        }
        __syncthreads();
    }
}

// A tile's states are loaded ONCE in the order the positions lie -- a wave's lanes read consecutive positions, so the row numbers are
// read coalesced and the gathers through them walk the K runs as K dense streams -- and wait in LDS for the threads, each of which then
// folds FOLD_ITEMS consecutive positions (in padded slots: fold_stage_slot of merge_fold_host.h).  States wider than FOLD_STAGE_BYTES would not fit beside the scan and the output stage:
// those algorithms read every position where it lies.  So does Collapsing: its argument is one byte a row, the runs' sign bytes of a
// tile are a few cache lines, and staging its 16-byte state measured slower than reading them in place.
static constexpr u32 FOLD_STAGE_BYTES = 16;
template <class A>
struct FoldStages
{
    static constexpr bool value = sizeof(typename A::State) <= FOLD_STAGE_BYTES;
};
template <>
struct FoldStages<CollapsingFold>
{
    static constexpr bool value = false;
};
template <class A>
struct FoldTileSrc
{
    static constexpr bool STAGED = FoldStages<A>::value;
    FoldColumns<A> g;
    const typename A::State * staged;  // the tile's states, from position `base`
    u64 base;
    __device__ __forceinline__ u8 head(u64 p) const { return g.head(p); }
    __device__ __forceinline__ u32 row(u64 p) const { return g.row(p); }
    __device__ __forceinline__ bool tail(u64 p) const { return g.tail(p); }
    __device__ __forceinline__ typename A::State state(u64 p) const
    {
        if constexpr (STAGED)
            return staged[fold_stage_slot((u32)(p - base))];
        else
            return g.state(p);
    }
};

// lds: FOLD_STAGE_SLOTS states when FoldTileSrc<A>::STAGED (else unused)
template <class A>
__device__ __forceinline__ FoldTileSrc<A> fold_tile_src(const A & a, const u8 * heads, const u32 * rows, u32 n, typename A::State * lds)
{
    const u64 base = (u64)blockIdx.x * FOLD_TILE;
    if constexpr (FoldTileSrc<A>::STAGED)
    {
        for (u32 e = threadIdx.x; e < FOLD_TILE && base + e < n; e += FOLD_THREADS)
            lds[fold_stage_slot(e)] = a.load(rows[base + e]);
        __syncthreads();
    }
    return FoldTileSrc<A>{FoldColumns<A>{a, heads, rows, n}, lds, base};
}

template <class A>
__global__ __launch_bounds__(FOLD_THREADS) void k_fold_tile(A a, const u8 * __restrict__ heads, const u32 * __restrict__ rows, u32 n, typename A::State * __restrict__ agg_s,
                                                            u8 * __restrict__ agg_f)
{
    __shared__ typename A::State ls[FOLD_THREADS];
    __shared__ u8 lf[FOLD_THREADS];
    __shared__ typename A::State lstage[FoldTileSrc<A>::STAGED ? FOLD_STAGE_SLOTS : 1];
    const FoldTileSrc<A> src = fold_tile_src(a, heads, rows, n, lstage);
    u64 p0, p1;
    fold_thread_range(blockIdx.x, threadIdx.x, n, p0, p1);
    typename A::State s = {};
    u8 fl = 0;
    fold_aggregate(a, src, p0, p1, s, fl);
    fold_block_scan(a, s, fl, ls, lf);
    if (threadIdx.x == FOLD_THREADS - 1)
    {
        agg_s[blockIdx.x] = s;
        agg_f[blockIdx.x] = fl;
    }
}

template <class A>
__global__ __launch_bounds__(FOLD_THREADS) void k_fold_carry(A a, const typename A::State * __restrict__ agg_s, const u8 * __restrict__ agg_f, u32 n_tiles,
                                                             typename A::State * __restrict__ carry)
{
    __shared__ typename A::State ls[FOLD_THREADS];
    __shared__ u8 lf[FOLD_THREADS];
    const u32 t0 = fold_chunk_begin(threadIdx.x, n_tiles), t1 = fold_chunk_begin(threadIdx.x + 1, n_tiles);
    typename A::State s = {};
    u8 fl = 0;
    fold_chunk_aggregate(a, agg_s, agg_f, t0, t1, s, fl);
    fold_block_scan(a, s, fl, ls, lf);
    typename A::State ps = {};
    u8 pf = 0;
    if (threadIdx.x)
    {
        ps = ls[threadIdx.x - 1];
        pf = lf[threadIdx.x - 1];
    }
    fold_chunk_carries(a, agg_s, agg_f, t0, t1, ps, pf, carry);
}

// Exclusive sum of the threads' counts, through LDS and not block_scan.h's block_scan_exclusive<AddU32>: with the shuffle scan the
// Summing fold measured 2.4-5.6 % slower at 10^8 rows, so this site keeps the form it had.
__device__ __forceinline__ u32 fold_block_exclusive_u32(u32 v, u32 * lds /* FOLD_THREADS */, u32 * total)
{
    const u32 t = threadIdx.x;
    u32 x = v;
    lds[t] = x;
    __syncthreads();
    for (u32 d = 1; d < FOLD_THREADS; d <<= 1)
    {
        const u32 o = t >= d ? lds[t - d] : 0;
        __syncthreads();
        x += o;
        lds[t] = x;
        __syncthreads();
    }
    *total = lds[FOLD_THREADS - 1];
    return x - v;
}

// EMIT = false: tile_counts[tile] = the tile's outputs and thread_counts[tile * FOLD_THREADS + thread] = the thread's (at most
// FOLD_MAX_OUT * FOLD_ITEMS).  EMIT = true: tile_offsets[tile] is where they go in out0 (and out1: the second column of a PAIRED
// algorithm); the threads' counts are read back, so the tile is walked once.
template <class A, bool EMIT>
__global__ __launch_bounds__(FOLD_THREADS) void k_fold_apply(A a, const u8 * __restrict__ heads, const u32 * __restrict__ rows, u32 n,
                                                             const typename A::State * __restrict__ carry, u32 * __restrict__ tile_counts,
                                                             u8 * __restrict__ thread_counts, const u64 * __restrict__ tile_offsets, u64 * __restrict__ out0,
                                                             u64 * __restrict__ out1)
{
    __shared__ typename A::State ls[FOLD_THREADS];
    __shared__ u8 lf[FOLD_THREADS];
    __shared__ u32 lcount[FOLD_THREADS];
    __shared__ u32 stage0[EMIT ? (A::PAIRED ? 1 : FOLD_MAX_OUT) * FOLD_TILE : 1];  // a PAIRED tail emits at most one pair
    __shared__ u32 stage1[EMIT && A::PAIRED ? FOLD_TILE : 1];
    __shared__ typename A::State lstage[FoldTileSrc<A>::STAGED ? FOLD_STAGE_SLOTS : 1];
    const FoldTileSrc<A> src = fold_tile_src(a, heads, rows, n, lstage);
    u64 p0, p1;
    fold_thread_range(blockIdx.x, threadIdx.x, n, p0, p1);
    typename A::State s = {};
    u8 fl = 0;
    fold_aggregate(a, src, p0, p1, s, fl);
    fold_block_scan(a, s, fl, ls, lf);
    // the prefix of this thread: the tile's carry, then the threads before it
    typename A::State ps = {};
    u8 pf = 0;
    if (blockIdx.x)
    {
        ps = carry[blockIdx.x];
        pf = FOLD_ANY;
    }
    if (threadIdx.x)
        fold_seg_combine(a, ps, pf, ls[threadIdx.x - 1], lf[threadIdx.x - 1]);
    const u64 thread_slot = (u64)blockIdx.x * FOLD_THREADS + threadIdx.x;
    u32 count = 0;
    if constexpr (EMIT)
        count = thread_counts[thread_slot];
    else
        fold_apply(a, src, p0, p1, ps, pf, [&](u64, const typename A::State &, u32 c, const u32 *) { count += c; });
    u32 total = 0;
    const u32 off = fold_block_exclusive_u32(count, lcount, &total);
    if constexpr (!EMIT)
    {
        thread_counts[thread_slot] = (u8)count;
        if (threadIdx.x == 0)
            tile_counts[blockIdx.x] = total;
    }
    else
    {
        const u64 base = tile_offsets[blockIdx.x];
        u32 at = off;
        fold_apply(a, src, p0, p1, ps, pf, [&](u64, const typename A::State & st, u32 c, const u32 * o) {
            if (!c)
                return;
            if constexpr (A::PAIRED)
            {
                stage0[at] = o[0];
                stage1[at] = o[1];
                a.store(st, base + at);
                at += 1;
            }
            else
                for (u32 j = 0; j < c; ++j)
                    stage0[at++] = o[j];
        });
        fold_store_staged(stage0, total, out0, base, true);
        if constexpr (A::PAIRED)
            fold_store_staged(stage1, total, out1, base, false);
    }
}

// off[t] = counts[0] + .. + counts[t - 1]; off[n_tiles] = the total; with tile_max, off[n_tiles + 1] = the greatest of tile_max
// (FOLD_THREADS tile counts a pass: the launch is the one it was)
__global__ __launch_bounds__(FOLD_THREADS) void k_fold_offsets(const u32 * __restrict__ counts, const u64 * __restrict__ tile_max /* NULL: none */, u32 n_tiles,
                                                               u64 * __restrict__ off)
{
    __shared__ u64 lmax[FOLD_THREADS / WAVE];
    const u64 total = block_scan_array<AddU64, false>(counts, off, n_tiles, 0);
    if (threadIdx.x == 0)
        off[n_tiles] = total;
    if (tile_max)
    {
        u64 m = 0;
        for (u32 t = threadIdx.x; t < n_tiles; t += FOLD_THREADS)
            m = tile_max[t] > m ? tile_max[t] : m;
        m = block_reduce<MaxU64>(m, lmax);
        if (threadIdx.x == 0)
            off[n_tiles + 1] = m;
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// (fold_validate, fold_check_column, FoldCall and fold_offsets are declared in merge_keys.h: merge_versioned_kernels.hip takes them)
// the shared argument prefix, in front of the device
int fold_validate(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const int32_t * descending, const int32_t * nan_direction_hint, u32 n_keys,
                  const uint64_t * run_offsets, u32 n_runs, u32 flags, FoldPrefix * px)
{
    CHGPU_TRY(merge_validate(ctx, key_cols, descending, nan_direction_hint, n_keys, run_offsets, n_runs, &px->keys, &px->rows));
    CHGPU_REQUIRE(n_runs >= 1, CHGPU_ERR_BAD_ARGUMENTS, "no runs: a folding merge takes at least one");
    return merge_check_flags(flags);
}

int fold_check_column(const chgpu_col * c, const char * what, int want_type, const char * type_name, u64 rows)
{
    CHGPU_REQUIRE(c->type == want_type, CHGPU_ERR_BAD_ARGUMENTS, "the %s column has the type %d: it is %s", what, c->type, type_name);
    CHGPU_REQUIRE(c->rows == rows, CHGPU_ERR_SIZES_MISMATCH, "the %s column has %llu rows, the run offsets end at %llu", what, (unsigned long long)c->rows,
                  (unsigned long long)rows);
    return CHGPU_OK;
}

// BAD_ARGUMENTS naming the lowest concatenated row whose value is outside the column's domain (mode 0: Int8 sign, 1: UInt8 is_deleted)
static int fold_require_domain(chgpu_ctx * ctx, PairTemps & tmp, const chgpu_col * c, int mode, u64 rows)
{
    const u32 tiles = merge_tiles((u32)rows);
    u64 bad = ~0ull;
    CHGPU_TRY(merge_lowest_row(ctx, tmp, tiles, [&](u64 * partial) {
        hipLaunchKernelGGL(k_fold_bad, dim3(tiles), dim3(FOLD_THREADS), 0, ctx->stream, (const u8 *)c->data, mode, (u32)rows, partial);
    }, &bad));
    if (mode == 0)
        CHGPU_REQUIRE(bad == ~0ull, CHGPU_ERR_BAD_ARGUMENTS, "the sign of row %llu is neither 1 nor -1", (unsigned long long)bad);
    CHGPU_REQUIRE(bad == ~0ull, CHGPU_ERR_BAD_ARGUMENTS, "is_deleted of row %llu is neither 0 nor 1", (unsigned long long)bad);
    return CHGPU_OK;
}

int FoldCall::open(const chgpu_col * const * key_cols, const FoldPrefix & px, const uint64_t * run_offsets, u32 n_runs, u32 flags, const chgpu_col * const * domain,
                   const int * domain_mode, u32 n_domain)
{
    chgpu_ctx * ctx = mem.ctx;
    const u64 n = px.rows;
    tiles = merge_tiles((u32)n);
    if (!n)
        return CHGPU_OK;
    if ((flags & CHGPU_MERGE_CHECK_SORTED) && n >= 2)
        CHGPU_TRY(merge_require_sorted(ctx, px.keys, run_offsets, n_runs, n));
    for (u32 i = 0; i < n_domain; ++i)
        CHGPU_TRY(fold_require_domain(ctx, tmp, domain[i], domain_mode[i], n));
    CHGPU_TRY(merge_order(ctx, key_cols, px.keys, run_offsets, n_runs, n, tmp, &words, &rows));
    void * h = nullptr;
    CHGPU_TRY(tmp.alloc(n, &h));
    heads = (u8 *)h;
    hipLaunchKernelGGL(k_fold_heads, dim3(chgpu_grid_for(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, px.keys, words, rows, (u32)n, heads);
    ctx->counters[6] += 1;
    return CHGPU_OK;
}

int FoldCall::close(int rc, chgpu_col ** outs, u32 n_outs)
{
    if (rc == CHGPU_OK)
    {
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            rc = chgpu_set_error(CHGPU_ERR_DEVICE, "%s: %s", mem.op, hipGetErrorString(e));
    }
    if (rc != CHGPU_OK)
        for (u32 i = 0; i < n_outs; ++i)
            if (outs[i])
            {
                chgpu_col_free(outs[i]);
                outs[i] = nullptr;
            }
    return rc;
}

int fold_offsets(chgpu_ctx * ctx, PairTemps & tmp, const u32 * counts, const u64 * tile_max, u32 tiles, const u64 ** tile_off, u64 * result)
{
    const u32 n_results = tile_max ? 2 : 1;
    void * off = nullptr;
    CHGPU_TRY(tmp.alloc(((size_t)tiles + n_results) * sizeof(u64), &off));
    hipLaunchKernelGGL(k_fold_offsets, dim3(1), dim3(FOLD_THREADS), 0, ctx->stream, counts, tile_max, tiles, (u64 *)off);
    ctx->counters[6] += 1;
    *tile_off = (const u64 *)off;
    return chgpu_read_back(ctx, *tile_off + tiles, result, n_results * sizeof(u64));
}

// Everything behind the validation.  domain[0..n_domain): the columns to check with their modes.  outs: the row-number columns (one, or
// two for a PAIRED algorithm) followed by the result columns of the folding form.
template <class A>
static int fold_run(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const FoldPrefix & px, const uint64_t * run_offsets, u32 n_runs, u32 flags, A a,
                    const chgpu_col * const * domain, const int * domain_mode, u32 n_domain, chgpu_col ** outs)
{
    typedef typename A::State State;
    u32 n_outs = A::PAIRED ? 2 : 1;
    if constexpr (A::PAIRED)
        n_outs += a.d.n;
    for (u32 i = 0; i < n_outs; ++i)
        outs[i] = nullptr;
    FoldCall call(ctx, "merge_fold");
    const u32 n = (u32)px.rows;
    u64 total = 0;
    const u64 * tile_off = nullptr;
    void * carry = nullptr, * thread_counts = nullptr;
    CHGPU_TRY(call.open(key_cols, px, run_offsets, n_runs, flags, domain, domain_mode, n_domain));
    const u32 tiles = call.tiles;
    if (n)
    {
        void * agg_s = nullptr, * agg_f = nullptr, * counts = nullptr;
        CHGPU_TRY(call.tmp.alloc((size_t)tiles * FOLD_THREADS, &thread_counts));
        CHGPU_TRY(call.tmp.alloc((size_t)tiles * sizeof(State), &agg_s));
        CHGPU_TRY(call.tmp.alloc(tiles, &agg_f));
        CHGPU_TRY(call.tmp.alloc((size_t)tiles * sizeof(State), &carry));
        CHGPU_TRY(call.tmp.alloc((size_t)tiles * sizeof(u32), &counts));
        hipLaunchKernelGGL(k_fold_tile<A>, dim3(tiles), dim3(FOLD_THREADS), 0, ctx->stream, a, (const u8 *)call.heads, call.rows, n, (State *)agg_s, (u8 *)agg_f);
        hipLaunchKernelGGL(k_fold_carry<A>, dim3(1), dim3(FOLD_THREADS), 0, ctx->stream, a, (const State *)agg_s, (const u8 *)agg_f, tiles, (State *)carry);
        hipLaunchKernelGGL((k_fold_apply<A, false>), dim3(tiles), dim3(FOLD_THREADS), 0, ctx->stream, a, (const u8 *)call.heads, call.rows, n, (const State *)carry,
                           (u32 *)counts, (u8 *)thread_counts, (const u64 *)nullptr, (u64 *)nullptr, (u64 *)nullptr);
        ctx->counters[6] += 3;
        CHGPU_TRY(fold_offsets(ctx, call.tmp, (const u32 *)counts, nullptr, tiles, &tile_off, &total));
    }
    int rc = CHGPU_OK;
    for (u32 i = 0; i < n_outs && rc == CHGPU_OK; ++i)
    {
        int type = CHGPU_U64;
        if constexpr (A::PAIRED)
            if (i >= 2)
                type = a.d.type[i - 2];
        rc = chgpu_col_new(ctx, type, total, &outs[i]);
    }
    if (rc == CHGPU_OK && total)
    {
        if constexpr (A::PAIRED)
            for (u32 k = 0; k < a.d.n; ++k)
                a.d.out[k] = outs[2 + k]->data;
        hipLaunchKernelGGL((k_fold_apply<A, true>), dim3(tiles), dim3(FOLD_THREADS), 0, ctx->stream, a, (const u8 *)call.heads, call.rows, n, (const State *)carry,
                           (u32 *)nullptr, (u8 *)thread_counts, tile_off, (u64 *)outs[0]->data, A::PAIRED ? (u64 *)outs[1]->data : (u64 *)nullptr);
        ctx->counters[6] += 1;
    }
    return call.close(rc, outs, n_outs);
}

extern "C" int chgpu_merge_replacing(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const int32_t * descending, const int32_t * nan_direction_hint,
                                     uint32_t n_keys, const uint64_t * run_offsets, uint32_t n_runs, uint32_t flags, const chgpu_col * version,
                                     const chgpu_col * is_deleted_u8, int32_t cleanup, chgpu_col ** rows_out_u64)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    CHGPU_REQUIRE(rows_out_u64, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    FoldPrefix px;
    CHGPU_TRY(fold_validate(ctx, key_cols, descending, nan_direction_hint, n_keys, run_offsets, n_runs, flags, &px));
    ReplacingFold a;
    if (version)
    {
        CHGPU_REQUIRE(chgpu_type_size(version->type), CHGPU_ERR_BAD_ARGUMENTS, "the version column has the unknown type %d", version->type);
        CHGPU_REQUIRE(fold_type_is_int(version->type), CHGPU_ERR_NOT_IMPLEMENTED, "a Float version column is not implemented: versions are integers");
        CHGPU_TRY(fold_check_column(version, "version", version->type, "", px.rows));
        a.version = version->data;
        a.version_type = version->type;
    }
    if (is_deleted_u8)
    {
        CHGPU_REQUIRE(version, CHGPU_ERR_NOT_IMPLEMENTED, "is_deleted without a version column is not implemented");
        CHGPU_TRY(fold_check_column(is_deleted_u8, "is_deleted", CHGPU_U8, "UInt8", px.rows));
        a.is_deleted = (const u8 *)is_deleted_u8->data;
    }
    a.cleanup = cleanup ? 1 : 0;
    const chgpu_col * domain[1] = {is_deleted_u8};
    const int mode[1] = {1};
    return fold_run(ctx, key_cols, px, run_offsets, n_runs, flags, a, domain, mode, is_deleted_u8 ? 1 : 0, rows_out_u64);
}

extern "C" int chgpu_merge_collapsing(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const int32_t * descending, const int32_t * nan_direction_hint,
                                      uint32_t n_keys, const uint64_t * run_offsets, uint32_t n_runs, uint32_t flags, const chgpu_col * sign_i8,
                                      chgpu_col ** rows_out_u64)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    CHGPU_REQUIRE(rows_out_u64 && sign_i8, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    FoldPrefix px;
    CHGPU_TRY(fold_validate(ctx, key_cols, descending, nan_direction_hint, n_keys, run_offsets, n_runs, flags, &px));
    CHGPU_TRY(fold_check_column(sign_i8, "sign", CHGPU_I8, "Int8", px.rows));
    CollapsingFold a;
    a.sign = (const i8 *)sign_i8->data;
    const chgpu_col * domain[1] = {sign_i8};
    const int mode[1] = {0};
    return fold_run(ctx, key_cols, px, run_offsets, n_runs, flags, a, domain, mode, 1, rows_out_u64);
}

extern "C" int chgpu_merge_folding(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const int32_t * descending, const int32_t * nan_direction_hint,
                                   uint32_t n_keys, const uint64_t * run_offsets, uint32_t n_runs, uint32_t flags, const chgpu_col * const * value_cols,
                                   const int32_t * kinds, uint32_t n_values, int32_t drop_zero, chgpu_col ** first_rows_u64, chgpu_col ** last_rows_u64,
                                   chgpu_col ** res_cols)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    CHGPU_REQUIRE(first_rows_u64 && last_rows_u64 && (n_values == 0 || (value_cols && kinds && res_cols)), CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    FoldPrefix px;
    CHGPU_TRY(fold_validate(ctx, key_cols, descending, nan_direction_hint, n_keys, run_offsets, n_runs, flags, &px));
    CHGPU_REQUIRE(n_values <= FOLD_MAX_VALUES, CHGPU_ERR_NOT_IMPLEMENTED, "%u value columns: one folding call takes at most %u", n_values, FOLD_MAX_VALUES);
    FoldValues d = {};
    d.n = n_values;
    d.drop_zero = drop_zero ? 1 : 0;
    for (u32 k = 0; k < n_values; ++k)
    {
        CHGPU_REQUIRE(value_cols[k], CHGPU_ERR_BAD_ARGUMENTS, "value column %u is NULL", k);
        CHGPU_REQUIRE(kinds[k] == CHGPU_FOLD_SUM || kinds[k] == CHGPU_FOLD_MIN || kinds[k] == CHGPU_FOLD_MAX, CHGPU_ERR_BAD_ARGUMENTS,
                      "value column %u has the unknown fold kind %d", k, kinds[k]);
        CHGPU_REQUIRE(chgpu_type_size(value_cols[k]->type), CHGPU_ERR_BAD_ARGUMENTS, "value column %u has the unknown type %d", k, value_cols[k]->type);
        CHGPU_REQUIRE(fold_type_is_int(value_cols[k]->type), CHGPU_ERR_NOT_IMPLEMENTED,
                      "value column %u is a Float column: the reference adds a group's rows one after another and a parallel scan rounds differently", k);
        CHGPU_REQUIRE(value_cols[k]->rows == px.rows, CHGPU_ERR_SIZES_MISMATCH, "value column %u has %llu rows, the run offsets end at %llu", k,
                      (unsigned long long)value_cols[k]->rows, (unsigned long long)px.rows);
        d.data[k] = value_cols[k]->data;
        d.type[k] = value_cols[k]->type;
        d.kind[k] = kinds[k];
    }
    chgpu_col * outs[2 + FOLD_MAX_VALUES];
    int rc = CHGPU_OK;
    dispatch_const<0, (int)FOLD_MAX_VALUES>(n_values, [&](auto nv) {
        FoldingFold<(u32)decltype(nv)::value> a;
        a.d = d;
        rc = fold_run(ctx, key_cols, px, run_offsets, n_runs, flags, a, nullptr, nullptr, 0, outs);
    });
    CHGPU_TRY(rc);
    *first_rows_u64 = outs[0];
    *last_rows_u64 = outs[1];
    for (u32 k = 0; k < n_values; ++k)
        res_cols[k] = outs[2 + k];
    return CHGPU_OK;
}
