// merge_kernels.hip — the other half of ORDER BY: the stable merge of runs that are already sorted.  MergingSortedAlgorithm
// (src/Processors/Merges/Algorithms/MergingSortedAlgorithm.cpp) over SortCursor (src/Core/SortCursor.h: column by column, ties by the
// cursor's `order`), which is what MergeSortingTransform (src/Processors/Transforms/MergeSortingTransform.cpp) does with the chunks
// PartialSortingTransform sorted and MergingSortedTransform with the streams; and isAlreadySorted (src/Interpreters/sortBlock.cpp).
// The key columns are the runs glued end to end; the result is the permutation of concatenated row numbers, bit-equal to what the
// stable sort of the concatenation gives (sort_kernels.hip), because both compare the SortKey words of sort_key.h.
//   k_merge_pairs      first key column -> (order-preserving u64 word, u32 row number) for the source row of every entry, ONE kernel
//                      over where that row comes from: the runs cut to the limit (MergeCutRows), a merged order known as a permutation
//                      (MergePermRows: what merge_order hands the folding merges where the plan is the sort chain) or the identity
//   k_merge_split      per round, ONE launch: for every tile edge of every pair, the merge-path crossing of its diagonal (binary search
//                      over the pair's two runs in HBM)
//   k_merge_tiles      per round, ONE launch: a workgroup stages its tile's two input pieces in LDS, every thread finds its own diagonal
//                      there and merges MRG_ITEMS consecutive outputs, the tile goes out coalesced
//   k_merge_perm       the last round's row numbers widened to the UInt64 permutation
//   k_merge_is_sorted  adjacent rows compared under the same order, never across a run boundary; per-tile minimum of the violating row
//   k_merge_min        one workgroup folds the tile minima: the LOWEST violating row, the same in every run
// The comparator reads the words first; on equal words (and n_keys > 1) the remaining columns through the row numbers; all equal: the
// left run's element first (merge_host.h keeps the invariant).  No atomics anywhere.
// Host side, each written once: merge_pairs launches the pair build for the tree and for merge_order, merge_plan_of
// holds the plan's choice, merge_new_perm the UInt64 permutation, merge_lowest_row the "lowest offending row" of a check (also the
// folds' domain check), merge_check_flags the flag check.
// Algorithmic bytes per row: key build sizeof(T) + 12; a round 2 x 12; the permutation 4 + 8.  is_sorted: the key columns once.
#include "merge_keys.h"

// Does (wb, rb) order STRICTLY before (wa, ra)?  Equal on every column answers false: the caller then takes the left run's element.
__device__ __forceinline__ bool mrg_before(const MergeKeys & keys, u64 wb, u32 rb, u64 wa, u32 ra)
{
    if (wb != wa)
        return wb < wa;
    for (u32 j = 1; j < keys.n; ++j)
    {
        const u64 x = mrg_key(keys, j, rb), y = mrg_key(keys, j, ra);
        if (x != y)
            return x < y;
    }
    return false;
}

// The source row of entry i of the pair arrays, three ways.
// cut_off[n_runs + 1]: where each (cut) run starts in the arrays; src_off[n_runs]: its first row in the columns
struct MergeCutRows
{
    const u32 * __restrict__ cut_off, * __restrict__ src_off;
    u32 n_runs;
    __device__ __forceinline__ u32 operator()(u32 i) const
    {
        u32 lo = 0, hi = n_runs; // cut_off[lo] <= i < cut_off[hi]
        while (hi - lo > 1)
        {
            const u32 mid = lo + (hi - lo) / 2;
            if (cut_off[mid] <= i)
                lo = mid;
            else
                hi = mid;
        }
        return src_off[lo] + (i - cut_off[lo]);
    }
};
struct MergePermRows
{
    const u64 * __restrict__ perm;
    __device__ __forceinline__ u32 operator()(u32 i) const { return (u32)perm[i]; }
};
struct MergeIdentityRows
{
    __device__ __forceinline__ u32 operator()(u32 i) const { return i; }
};

template <class Source>
__global__ __launch_bounds__(256) void k_merge_pairs(MergeKeys keys, Source source, u32 n, u64 * __restrict__ words, u32 * __restrict__ rows)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
    {
        const u32 src = source((u32)i);
        words[i] = mrg_key(keys, 0, src);
        rows[i] = src;
    }
}

__global__ __launch_bounds__(256) void k_merge_split(MergeKeys keys, const MergePair * __restrict__ pairs, u32 n_pairs, u32 n_splits, const u64 * __restrict__ words,
                                                     const u32 * __restrict__ rows, u32 * __restrict__ splits)
{
    const u32 s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n_splits)
        return;
    const MergePair p = pairs[merge_pair_of<&MergePair::split_begin>(pairs, n_pairs, s)];
    const u64 edge = (u64)(s - p.split_begin) * MRG_TILE;
    const u32 diag = edge < p.out_len ? (u32)edge : p.out_len;
    const u64 * wa = words + p.a_begin, * wb = words + p.b_begin;
    const u32 * ra = rows + p.a_begin, * rb = rows + p.b_begin;
    splits[s] = merge_path(diag, p.a_len, p.b_len, [&](u32 bi, u32 ai) { return mrg_before(keys, wb[bi], rb[bi], wa[ai], ra[ai]); });
}

__global__ __launch_bounds__(MRG_THREADS) void k_merge_tiles(MergeKeys keys, const MergePair * __restrict__ pairs, u32 n_pairs, const u32 * __restrict__ splits,
                                                             const u64 * __restrict__ words_in, const u32 * __restrict__ rows_in, u64 * __restrict__ words_out,
                                                             u32 * __restrict__ rows_out)
{
    __shared__ u64 sw[MRG_TILE];
    __shared__ u32 sr[MRG_TILE];
    const u32 tid = threadIdx.x;
    const MergePair p = pairs[merge_pair_of<&MergePair::tile_begin>(pairs, n_pairs, blockIdx.x)];
    const u32 k = blockIdx.x - p.tile_begin;
    const u32 d0 = k * MRG_TILE; // < out_len: the pair has this tile
    const u32 n = p.out_len - d0 < MRG_TILE ? p.out_len - d0 : MRG_TILE;
    const u32 a0 = splits[p.split_begin + k];
    u32 a1 = splits[p.split_begin + k + 1];
    // Sorted runs give a0 <= a1 <= a0 + n.  Runs that are not sorted (the caller's error without CHGPU_MERGE_CHECK_SORTED) may not: the
    // order is then unspecified, but every index stays inside the pair
    a1 = a1 < a0 ? a0 : a1 - a0 > n ? a0 + n : a1;
    const u32 b0 = d0 - a0;
    const u32 na = a1 - a0, nb = n - na;
    for (u32 e = tid; e < n; e += MRG_THREADS)
    {
        const u32 src = e < na ? p.a_begin + a0 + e : p.b_begin + b0 + (e - na);
        sw[e] = words_in[src];
        sr[e] = rows_in[src];
    }
    __syncthreads();
    const u32 d = tid * MRG_ITEMS < n ? tid * MRG_ITEMS : n;
    const u32 count = n - d < MRG_ITEMS ? n - d : MRG_ITEMS;
    const u64 * la = sw, * lb = sw + na;
    const u32 * lra = sr, * lrb = sr + na;
    u32 ai = merge_path(d, na, nb, [&](u32 bi, u32 ai_) { return mrg_before(keys, lb[bi], lrb[bi], la[ai_], lra[ai_]); });
    u32 bi = d - ai;
    u64 ow[MRG_ITEMS];
    u32 orow[MRG_ITEMS];
#pragma unroll
    for (u32 i = 0; i < MRG_ITEMS; ++i)
    {
        if (i < count)
        {
            // all equal: the left run's element goes first (the invariant of merge_host.h)
            const bool take_b = bi < nb && (ai >= na || mrg_before(keys, lb[bi], lrb[bi], la[ai], lra[ai]));
            ow[i] = take_b ? lb[bi] : la[ai];
            orow[i] = take_b ? lrb[bi] : lra[ai];
            bi += take_b ? 1 : 0;
            ai += take_b ? 0 : 1;
        }
    }
    __syncthreads(); // every thread has read its inputs: the tile's LDS now takes the outputs
#pragma unroll
    for (u32 i = 0; i < MRG_ITEMS; ++i)
        if (i < count)
        {
            sw[d + i] = ow[i];
            sr[d + i] = orow[i];
        }
    __syncthreads();
    const u32 out = p.out_begin + d0;
    for (u32 e = tid; e < n; e += MRG_THREADS)
    {
        words_out[out + e] = sw[e];
        rows_out[out + e] = sr[e];
    }
}

// rows == NULL: the identity
__global__ __launch_bounds__(256) void k_merge_perm(const u32 * __restrict__ rows, u64 n, u64 * __restrict__ perm)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
        perm[i] = rows ? rows[i] : i;
}

// run_off[n_runs + 1]; partial[blockIdx.x] = the lowest row i of this tile that is no run's first row and orders strictly before
// row i - 1, or ~0
__global__ __launch_bounds__(MRG_THREADS) void k_merge_is_sorted(MergeKeys keys, const u32 * __restrict__ run_off, u32 n_runs, u32 n, u64 * __restrict__ partial)
{
    __shared__ u64 lds[MRG_THREADS / WAVE];
    // a thread's rows are MRG_THREADS apart, so that a wave reads consecutive rows
    const u64 first = (u64)blockIdx.x * MRG_TILE + threadIdx.x;
    u64 found = ~0ull;
    if (first < n)
    {
        u32 lo = 0, hi = n_runs + 1; // the first offset >= first (run_off[n_runs] == n > first: it exists)
        while (lo < hi)
        {
            const u32 mid = lo + (hi - lo) / 2;
            if (run_off[mid] < (u32)first)
                lo = mid + 1;
            else
                hi = mid;
        }
        u32 pos = lo;
        for (u32 t = 0; t < MRG_ITEMS && found == ~0ull; ++t)
        {
            const u64 i = first + (u64)t * MRG_THREADS;
            if (i >= n)
                break;
            while (pos <= n_runs && run_off[pos] < (u32)i)
                pos += 1;
            if (pos <= n_runs && run_off[pos] == (u32)i)
                continue; // the first row of a run: nothing before it to compare with
            for (u32 j = 0; j < keys.n; ++j)
            {
                const u64 x = mrg_key(keys, j, i), y = mrg_key(keys, j, i - 1);
                if (x != y)
                {
                    if (x < y)
                        found = i;
                    break;
                }
            }
        }
    }
    const u64 m = block_reduce<MinU64>(found, lds);
    if (threadIdx.x == 0)
        partial[blockIdx.x] = m;
}

__global__ __launch_bounds__(MRG_THREADS) void k_merge_min(const u64 * __restrict__ partial, u32 n, u64 * __restrict__ out)
{
    __shared__ u64 lds[MRG_THREADS / WAVE];
    u64 v = ~0ull;
    for (u32 i = threadIdx.x; i < n; i += MRG_THREADS)
        v = partial[i] < v ? partial[i] : v;
    const u64 m = block_reduce<MinU64>(v, lds);
    if (threadIdx.x == 0)
        out[0] = m;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
int merge_validate(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const int32_t * descending, const int32_t * nan_direction_hint, u32 n_keys,
                   const uint64_t * run_offsets, u32 n_runs, MergeKeys * keys, u64 * rows)
{
    CHGPU_REQUIRE(ctx && key_cols && descending && nan_direction_hint && run_offsets, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(n_keys >= 1 && n_keys <= MRG_MAX_KEYS, CHGPU_ERR_BAD_ARGUMENTS, "%u key columns: a sort description has 1 to %u", n_keys, MRG_MAX_KEYS);
    const char * msg = nullptr;
    const int rc = merge_check_offsets(run_offsets, n_runs, rows, &msg);
    CHGPU_REQUIRE(rc == CHGPU_OK, rc, "%s", msg);
    *keys = MergeKeys{};
    keys->n = n_keys;
    for (u32 j = 0; j < n_keys; ++j)
    {
        CHGPU_REQUIRE(key_cols[j], CHGPU_ERR_BAD_ARGUMENTS, "key column %u is NULL", j);
        CHGPU_REQUIRE(chgpu_type_size(key_cols[j]->type), CHGPU_ERR_BAD_ARGUMENTS, "key column %u has the unknown type %d", j, key_cols[j]->type);
        CHGPU_REQUIRE(key_cols[j]->rows == *rows, CHGPU_ERR_SIZES_MISMATCH, "key column %u has %llu rows, the run offsets end at %llu", j,
                      (unsigned long long)key_cols[j]->rows, (unsigned long long)*rows);
        keys->data[j] = key_cols[j]->data;
        keys->type[j] = key_cols[j]->type;
        keys->desc[j] = descending[j] ? 1 : 0;
        keys->hint[j] = nan_direction_hint[j];
    }
    return CHGPU_OK;
}

// u32 host values into pool memory of the call (the host vector is consumed before hipMemcpyAsync returns: it is pageable)
static int merge_upload(chgpu_ctx * ctx, PairTemps & tmp, const void * host, size_t bytes, void ** dev)
{
    CHGPU_TRY(tmp.alloc(bytes, dev));
    if (bytes)
        CHGPU_HIP(hipMemcpyAsync(*dev, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    return CHGPU_OK;
}

int merge_check_flags(u32 flags)
{
    CHGPU_REQUIRE(!(flags & ~(u32)CHGPU_MERGE_CHECK_SORTED), CHGPU_ERR_BAD_ARGUMENTS, "unknown flag bits 0x%x", flags & ~(u32)CHGPU_MERGE_CHECK_SORTED);
    return CHGPU_OK;
}

// partial[n] -> out[0] = the minimum, by one workgroup: one launch, counted
static void merge_lowest(chgpu_ctx * ctx, const u64 * partial, u32 n, u64 * out)
{
    hipLaunchKernelGGL(k_merge_min, dim3(1), dim3(MRG_THREADS), 0, ctx->stream, partial, n, out);
    ctx->counters[6] += 1;
}

int merge_lowest_row(chgpu_ctx * ctx, PairTemps & tmp, u32 tiles, const std::function<void(u64 * partial)> & launch_tiles, u64 * lowest)
{
    void * partial = nullptr;
    CHGPU_TRY(tmp.alloc(((size_t)tiles + 1) * sizeof(u64), &partial));
    launch_tiles((u64 *)partial);
    ctx->counters[6] += 1;
    merge_lowest(ctx, (const u64 *)partial, tiles, (u64 *)partial + tiles);
    return chgpu_read_back(ctx, (const u64 *)partial + tiles, lowest, sizeof(u64));
}

// *first_unsorted_row: ~0, or the lowest row that orders before its predecessor inside one run.  rows >= 1.
static int merge_is_sorted(chgpu_ctx * ctx, const MergeKeys & keys, const uint64_t * run_offsets, u32 n_runs, u64 rows, u64 * first_unsorted_row)
{
    PairAllocs mem;
    mem.ctx = ctx, mem.op = "is_sorted";
    mem.begin_call();
    PairTemps tmp(mem);
    std::vector<u32> off(n_runs + 1);
    for (u32 r = 0; r <= n_runs; ++r)
        off[r] = (u32)run_offsets[r];
    void * off_dev = nullptr;
    CHGPU_TRY(merge_upload(ctx, tmp, off.data(), off.size() * sizeof(u32), &off_dev));
    const u32 tiles = merge_tiles((u32)rows);
    return merge_lowest_row(ctx, tmp, tiles, [&](u64 * partial) {
        hipLaunchKernelGGL(k_merge_is_sorted, dim3(tiles), dim3(MRG_THREADS), 0, ctx->stream, keys, (const u32 *)off_dev, n_runs, (u32)rows, partial);
    }, first_unsorted_row);
}

int merge_require_sorted(chgpu_ctx * ctx, const MergeKeys & keys, const uint64_t * run_offsets, u32 n_runs, u64 rows)
{
    u64 bad = ~0ull;
    CHGPU_TRY(merge_is_sorted(ctx, keys, run_offsets, n_runs, rows, &bad));
    CHGPU_REQUIRE(bad == ~0ull, CHGPU_ERR_BAD_ARGUMENTS, "a run is not sorted: row %llu orders before row %llu", (unsigned long long)bad,
                  (unsigned long long)(bad - 1));
    return CHGPU_OK;
}

extern "C" int chgpu_is_sorted(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const int32_t * descending, const int32_t * nan_direction_hint, uint32_t n_keys,
                               const uint64_t * run_offsets, uint32_t n_runs, uint64_t * first_unsorted_row)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    CHGPU_REQUIRE(first_unsorted_row, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    MergeKeys keys;
    u64 rows = 0;
    CHGPU_TRY(merge_validate(ctx, key_cols, descending, nan_direction_hint, n_keys, run_offsets, n_runs, &keys, &rows));
    *first_unsorted_row = ~0ull;
    if (rows < 2)
        return CHGPU_OK;
    return merge_is_sorted(ctx, keys, run_offsets, n_runs, rows, first_unsorted_row);
}

// The (word, row) pairs of n entries into `tmp`, one launch, counted.  The source rows: the runs cut by `cut_map` (cut_off[n_runs + 1]
// followed by src_off[n_runs]), else the permutation `perm`, else (both NULL) the identity.
static int merge_pairs(chgpu_ctx * ctx, PairTemps & tmp, const MergeKeys & keys, u64 n, const u32 * cut_map, u32 n_runs, const u64 * perm, void ** words, void ** rows)
{
    CHGPU_TRY(tmp.alloc(n * sizeof(u64), words));
    CHGPU_TRY(tmp.alloc(n * sizeof(u32), rows));
    const dim3 grid(chgpu_grid_for(ctx, n, 256, 8));
    if (cut_map)
        hipLaunchKernelGGL(k_merge_pairs<MergeCutRows>, grid, dim3(256), 0, ctx->stream, keys, MergeCutRows{cut_map, cut_map + n_runs + 1, n_runs}, (u32)n, (u64 *)*words,
                           (u32 *)*rows);
    else if (perm)
        hipLaunchKernelGGL(k_merge_pairs<MergePermRows>, grid, dim3(256), 0, ctx->stream, keys, MergePermRows{perm}, (u32)n, (u64 *)*words, (u32 *)*rows);
    else
        hipLaunchKernelGGL(k_merge_pairs<MergeIdentityRows>, grid, dim3(256), 0, ctx->stream, keys, MergeIdentityRows{}, (u32)n, (u64 *)*words, (u32 *)*rows);
    ctx->counters[6] += 1;
    return CHGPU_OK;
}

// merge_plan's choice for these keys
static int merge_plan_of(const MergeKeys & keys, u64 rows, u64 cut_rows, u32 n_runs)
{
    u32 key_sizes[MRG_MAX_KEYS];
    for (u32 j = 0; j < keys.n; ++j)
        key_sizes[j] = (u32)chgpu_type_size(keys.type[j]);
    return merge_plan(key_sizes, keys.n, rows, cut_rows, n_runs);
}

// *perm_out: a new UInt64 column of n_out rows, rows[0 .. n_out) widened (rows == NULL: the identity); the launch is counted
static int merge_new_perm(chgpu_ctx * ctx, const u32 * rows, u64 n_out, chgpu_col ** perm_out)
{
    chgpu_col * perm = nullptr;
    CHGPU_TRY(chgpu_col_new(ctx, CHGPU_U64, n_out, &perm));
    if (n_out)
    {
        hipLaunchKernelGGL(k_merge_perm, dim3(chgpu_grid_for(ctx, n_out, 256, 8)), dim3(256), 0, ctx->stream, rows, n_out, (u64 *)perm->data);
        ctx->counters[6] += 1;
    }
    *perm_out = perm;
    return CHGPU_OK;
}

// the merge tree over runs cut to `lens`: the last round's (word, row) arrays, in `tmp`
static int merge_tree_pairs(chgpu_ctx * ctx, PairTemps & tmp, const MergeKeys & keys, const uint64_t * run_offsets, u32 n_runs, u64 rows, const std::vector<u32> & lens,
                            u64 cut_rows, u64 limit, const u64 ** words_out, const u32 ** rows_out)
{
    const std::vector<MergeRound> rounds = merge_rounds(lens, limit);
    // one table for the whole call: the key build's run map (only when a run was cut), then every round's pairs
    std::vector<u32> map;
    if (cut_rows != rows)
    {
        map.resize(2 * (size_t)n_runs + 1);
        u32 pos = 0;
        for (u32 r = 0; r < n_runs; ++r)
        {
            map[r] = pos;
            map[n_runs + 1 + r] = (u32)run_offsets[r];
            pos += lens[r];
        }
        map[n_runs] = pos;
    }
    std::vector<MergePair> pairs;
    u32 max_splits = 0;
    for (const MergeRound & rd : rounds)
    {
        pairs.insert(pairs.end(), rd.pairs.begin(), rd.pairs.end());
        max_splits = rd.n_splits > max_splits ? rd.n_splits : max_splits;
    }
    void * map_dev = nullptr, * pairs_dev = nullptr, * splits = nullptr, * words[2] = {nullptr, nullptr}, * rws[2] = {nullptr, nullptr};
    CHGPU_TRY(merge_upload(ctx, tmp, map.data(), map.size() * sizeof(u32), &map_dev));
    CHGPU_TRY(merge_upload(ctx, tmp, pairs.data(), pairs.size() * sizeof(MergePair), &pairs_dev));
    CHGPU_TRY(tmp.alloc((size_t)max_splits * sizeof(u32), &splits));
    CHGPU_TRY(tmp.alloc(cut_rows * sizeof(u64), &words[1]));
    CHGPU_TRY(tmp.alloc(cut_rows * sizeof(u32), &rws[1]));
    CHGPU_TRY(merge_pairs(ctx, tmp, keys, cut_rows, map.empty() ? nullptr : (const u32 *)map_dev, n_runs, nullptr, &words[0], &rws[0]));
    int cur = 0;
    const MergePair * round_pairs = (const MergePair *)pairs_dev;
    for (const MergeRound & rd : rounds)
    {
        const u32 n_pairs = (u32)rd.pairs.size();
        if (rd.n_tiles)
        {
            hipLaunchKernelGGL(k_merge_split, dim3((rd.n_splits + 255) / 256), dim3(256), 0, ctx->stream, keys, round_pairs, n_pairs, rd.n_splits,
                               (const u64 *)words[cur], (const u32 *)rws[cur], (u32 *)splits);
            hipLaunchKernelGGL(k_merge_tiles, dim3(rd.n_tiles), dim3(MRG_THREADS), 0, ctx->stream, keys, round_pairs, n_pairs, (const u32 *)splits,
                               (const u64 *)words[cur], (const u32 *)rws[cur], (u64 *)words[cur ^ 1], (u32 *)rws[cur ^ 1]);
            ctx->counters[6] += 2;
        }
        round_pairs += n_pairs;
        cur ^= 1;
    }
    *words_out = (const u64 *)words[cur];
    *rows_out = (const u32 *)rws[cur];
    return CHGPU_OK;
}

// *perm_out: the first n_out row numbers of the tree's last round
static int merge_tree(chgpu_ctx * ctx, const MergeKeys & keys, const uint64_t * run_offsets, u32 n_runs, u64 rows, const std::vector<u32> & lens, u64 cut_rows,
                      u64 limit, u64 n_out, chgpu_col ** perm_out)
{
    PairAllocs mem;
    mem.ctx = ctx, mem.op = "merge_sorted";
    mem.begin_call();
    PairTemps tmp(mem);
    const u64 * words = nullptr;
    const u32 * rws = nullptr;
    CHGPU_TRY(merge_tree_pairs(ctx, tmp, keys, run_offsets, n_runs, rows, lens, cut_rows, limit, &words, &rws));
    chgpu_col * perm = nullptr;
    CHGPU_TRY(merge_new_perm(ctx, rws, n_out, &perm));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
    {
        chgpu_col_free(perm);
        return chgpu_set_error(CHGPU_ERR_DEVICE, "merge_sorted: %s", hipGetErrorString(e));
    }
    *perm_out = perm;
    return CHGPU_OK;
}

// the other plan: the stable radix sort of the concatenation, from the last key column to the first
static int merge_by_sort(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const MergeKeys & keys, u64 n_out, chgpu_col ** perm_out)
{
    chgpu_col * perm = nullptr;
    for (u32 j = keys.n; j-- > 0;)
    {
        chgpu_col * next = nullptr;
        const int rc = chgpu_sort_permutation(ctx, key_cols[j], perm, keys.desc[j], keys.hint[j], &next);
        if (perm)
            chgpu_col_free(perm);
        if (rc != CHGPU_OK)
            return rc;
        perm = next;
    }
    perm->rows = n_out; // IColumn::Permutation is simply cut (the buffer keeps its size class)
    *perm_out = perm;
    return CHGPU_OK;
}

int merge_order(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const MergeKeys & keys, const uint64_t * run_offsets, u32 n_runs, u64 rows, PairTemps & tmp,
                const u64 ** words, const u32 ** row_numbers)
{
    if (n_runs > 1 && merge_plan_of(keys, rows, rows, n_runs) == MERGE_PLAN_TREE)
        return merge_tree_pairs(ctx, tmp, keys, run_offsets, n_runs, rows, merge_initial_runs(run_offsets, n_runs, 0), rows, 0, words, row_numbers);
    // one run: M is the identity; the sort chain: M is its permutation.  The pairs are built from it.
    chgpu_col * perm = nullptr;
    if (n_runs > 1)
    {
        CHGPU_TRY(merge_by_sort(ctx, key_cols, keys, rows, &perm));
        tmp.cols.push_back(perm);
    }
    void * w = nullptr, * r = nullptr;
    CHGPU_TRY(merge_pairs(ctx, tmp, keys, rows, nullptr, 0, perm ? (const u64 *)perm->data : nullptr, &w, &r));
    *words = (const u64 *)w;
    *row_numbers = (const u32 *)r;
    return CHGPU_OK;
}

extern "C" int chgpu_merge_sorted_permutation(chgpu_ctx * ctx, const chgpu_col * const * key_cols, const int32_t * descending, const int32_t * nan_direction_hint,
                                              uint32_t n_keys, const uint64_t * run_offsets, uint32_t n_runs, uint64_t limit, uint32_t flags, chgpu_col ** perm_out_u64)
{
    ChgpuDeviceGuard _dev_guard(ctx);
    CHGPU_REQUIRE(perm_out_u64, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    MergeKeys keys;
    u64 rows = 0;
    CHGPU_TRY(merge_validate(ctx, key_cols, descending, nan_direction_hint, n_keys, run_offsets, n_runs, &keys, &rows));
    CHGPU_TRY(merge_check_flags(flags));
    if ((flags & CHGPU_MERGE_CHECK_SORTED) && rows >= 2)
        CHGPU_TRY(merge_require_sorted(ctx, keys, run_offsets, n_runs, rows));
    const u64 n_out = merge_cut(rows, limit);
    if (n_out == 0 || n_runs == 1)
        return merge_new_perm(ctx, nullptr, n_out, perm_out_u64); // nothing to merge: empty, or the identity cut to the limit
    const std::vector<u32> lens = merge_initial_runs(run_offsets, n_runs, limit);
    u64 cut_rows = 0;
    for (u32 len : lens)
        cut_rows += len;
    if (merge_plan_of(keys, rows, cut_rows, n_runs) == MERGE_PLAN_SORT)
        return merge_by_sort(ctx, key_cols, keys, n_out, perm_out_u64);
    return merge_tree(ctx, keys, run_offsets, n_runs, rows, lens, cut_rows, limit, n_out, perm_out_u64);
}
