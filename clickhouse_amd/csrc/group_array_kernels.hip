// group_array_kernels.hip — groupArray(x) / groupArray(N)(x) under GROUP BY: the (group key, value) pairs in one flat append-only store
// in HBM, IN ARRIVAL ORDER, turned into a ColumnArray (offsets + data) at the end.
//
// Reference: GroupArrayNumericImpl keeps an array per group, add() is push_back until max_elems, merge() is insert(end, rhs.begin,
// rhs.begin + min(rhs.size, max_elems - size)), insertResultInto appends the array and its end offset
// (src/AggregateFunctions/AggregateFunctionGroupArray.cpp).
//
// Design (not a translation).  Nothing is allocated per group and no table is touched, at any time:
//   store     u64 keys[cap] (keyed operators), T vals[cap]: T is the unsigned type of the value's width, the value's own bits.  Position
//             in the store IS arrival order: a filtered block is appended by survivor counts per tile -> scan -> in-wave ballot ranks
//             (k_tile_counts / k_ga_append), an unfiltered one by a widening copy of the keys and a plain copy of the values.  No
//             workgroup waits for another and no place is taken by an atomic.  While keys are written they are folded into two device
//             words, the OR and the AND of every key held (one wave reduction, one atomic pair per workgroup).
//   segments  finalize reads the two words back: or & ~and is the set of key bits that differ anywhere.  One stable 256-way pass of
//             chgpu_partition_by_key_byte over (key, value) per key byte that holds such a bit, least significant first: equal keys end up
//             adjacent, groups in ascending key order, every group's values still in arrival order.  k_tile_counts / k_ga_heads mark where
//             the key changes and write the group keys and segment starts by the same counts -> scan -> ballot ranks.
//   arrays    max_size and for_keys are one segmented copy (k_ga_seg_copy): work units of GA_UNIT OUTPUT elements that find their array
//             by binary search over the output offsets, so the division of work does not depend on array lengths.  for_keys finds a
//             key's segment by binary search over the group keys, which the passes left sorted: no table to build or keep.
// What this operator shares with others is written once elsewhere: the ranked tile (coordinate, ballots, counts kernel, head predicate,
// ranked-item loop, tile scan) is tile_rank.h, shared with limit_by_kernels.hip; the store (PairStore: reserve, merge's append, export
// of the keys), the radix passes, element load, entry checks, narrowing and plan printing are pair_store.h / pair_host.h; pool memory,
// the numbered allocations and a call's temporaries are pair_pool.h.  Its own: the append and head kernels, the value export, the row
// limit in front of the shared reserve, the two key words.
#include "chgpu_internal.h"

#include "pair_store.h"
#include "tile_rank.h"
#include "group_array_host.h"

typedef unsigned long long ull;

static constexpr u32 GA_T = TILE_T; // threads of every kernel here
static constexpr u32 GA_UNIT_R = (u32)(GA_UNIT / GA_T);

static_assert(GA_TILE == TILE_ITEMS && GA_UNIT == (u64)GA_T * GA_UNIT_R, "a tile is tile_rank.h's, a unit is whole steps of a workgroup");

// the OR and the AND of every key in the store
struct GaBits
{
    ull or_bits, and_bits;
};

__global__ void k_ga_bits_init(GaBits * b)
{
    b->or_bits = 0;
    b->and_bits = ~0ull;
}

__global__ void k_ga_bits_merge(GaBits * dst, const GaBits * src)
{
    const ull o = src->or_bits, a = src->and_bits; // (dst may be src)
    dst->or_bits |= o;
    dst->and_bits &= a;
}

// a workgroup's keys into the two words: wave reduction, then one atomic pair per workgroup.  Every thread of the workgroup calls it.
__device__ __forceinline__ void ga_fold_bits(u64 o, u64 a, GaBits * bits)
{
    __shared__ u64 s_or[GA_T / 64], s_and[GA_T / 64];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
    {
        o |= shfl_down_u64(o, d);
        a &= shfl_down_u64(a, d);
    }
    if (lane_id() == 0)
    {
        s_or[threadIdx.x >> 6] = o;
        s_and[threadIdx.x >> 6] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        for (u32 w = 1; w < GA_T / 64; ++w)
        {
            o |= s_or[w];
            a &= s_and[w];
        }
        atomicOr(&bits->or_bits, (ull)o);
        atomicAnd(&bits->and_bits, (ull)a);
    }
}

// the row's filter byte: the predicate of the filtered append (tile_rank.h)
struct GaFilterPred
{
    const u8 * f;
    u64 row_begin;
    __device__ __forceinline__ bool operator()(u64 i) const { return f[row_begin + i] != 0; }
};

// add_block with a filter: the survivors of tile t go to held + tile_off[t] + their rank in the tile.  key_size 0: without key.
template <typename T>
__global__ __launch_bounds__(GA_T) void k_ga_append(const void * __restrict__ key, u32 key_size, const T * __restrict__ val, GaFilterPred pred, u64 n, u64 n_tiles,
                                                    const u64 * __restrict__ tile_off, u64 held, u64 cap, u64 * __restrict__ out_k, T * __restrict__ out_v,
                                                    GaBits * bits)
{
    __shared__ u32 s_wave[GA_T / 64];
    u64 o = 0, a = ~0ull;
    for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
    {
        u64 m[TILE_R];
        const u64 pos = held + tile_off[tile] + tile_ballots(pred, tile, n, m, s_wave);
        tile_for_ranked(m, tile, pos, [&](u64 i, u64 at) {
            const u64 row = pred.row_begin + i;
            if (at < cap) // never past the store (the host reserved held + the survivors)
            {
                if (key_size)
                {
                    const u64 k = pair_load(key, key_size, row);
                    out_k[at] = k;
                    o |= k;
                    a &= k;
                }
                out_v[at] = val[row];
            }
        });
        __syncthreads(); // before the next tile overwrites the counts
    }
    if (key_size)
        ga_fold_bits(o, a, bits);
}

// add_block without a filter: the keys widened to the store's UInt64 (the values are a plain copy)
__global__ __launch_bounds__(GA_T) void k_ga_copy_keys(const void * __restrict__ key, u32 key_size, u64 row_begin, u64 n, u64 * __restrict__ out_k, GaBits * bits)
{
    u64 o = 0, a = ~0ull;
    for (u64 i = (u64)blockIdx.x * GA_T + threadIdx.x; i < n; i += (u64)gridDim.x * GA_T)
    {
        const u64 k = pair_load(key, key_size, row_begin + i);
        out_k[i] = k;
        o |= k;
        a &= k;
    }
    ga_fold_bits(o, a, bits);
}

// the sorted keys' run heads: group g's key and where its segment starts; src_off[groups] = n
__global__ __launch_bounds__(GA_T) void k_ga_heads(const u64 * __restrict__ sk, u64 n, u64 n_tiles, const u64 * __restrict__ tile_off, u64 groups,
                                                   u64 * __restrict__ gkeys, u64 * __restrict__ src_off)
{
    __shared__ u32 s_wave[GA_T / 64];
    const TileHeadPred<u64> pred{sk};
    if (blockIdx.x == 0 && threadIdx.x == 0)
        src_off[groups] = n;
    for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
    {
        u64 m[TILE_R];
        const u64 pos = tile_off[tile] + tile_ballots(pred, tile, n, m, s_wave);
        tile_for_ranked(m, tile, pos, [&](u64 i, u64 g) {
            if (g < groups) // (the counts were taken from these keys)
            {
                gkeys[g] = sk[i];
                src_off[g] = i;
            }
        });
        __syncthreads();
    }
}

// groupArray(N): the lengths of the arrays
__global__ __launch_bounds__(GA_T) void k_ga_lens(const u64 * __restrict__ src_off, u64 groups, u64 max_size, u32 * __restrict__ len)
{
    for (u64 g = (u64)blockIdx.x * GA_T + threadIdx.x; g < groups; g += (u64)gridDim.x * GA_T)
        len[g] = (u32)ga_trim(src_off[g + 1] - src_off[g], max_size);
}

// without key: the one segment and its array
__global__ void k_ga_nokey_offsets(u64 * src_off, u64 * out_ends, u64 held, u64 max_size)
{
    src_off[0] = 0;
    src_off[1] = held;
    out_ends[0] = ga_trim(held, max_size);
}

// for_keys: every asked key's group (GT_NONE: no group has it) and the length of its array.  The group keys are sorted: lower bound.
__global__ __launch_bounds__(GA_T) void k_ga_lookup(const u64 * __restrict__ gkeys, u64 groups, const u64 * __restrict__ ends, const void * __restrict__ keys,
                                                    u32 key_size, u64 n, u32 * __restrict__ gid, u32 * __restrict__ len)
{
    for (u64 i = (u64)blockIdx.x * GA_T + threadIdx.x; i < n; i += (u64)gridDim.x * GA_T)
    {
        const u64 k = pair_load(keys, key_size, i);
        u64 lo = 0, hi = groups;
        while (lo < hi)
        {
            const u64 mid = lo + (hi - lo) / 2;
            if (gkeys[mid] < k)
                lo = mid + 1;
            else
                hi = mid;
        }
        const bool found = lo < groups && gkeys[lo] == k;
        gid[i] = found ? (u32)lo : GT_NONE;
        len[i] = found ? (u32)(ends[lo] - (lo ? ends[lo - 1] : 0)) : 0u;
    }
}

// The segmented copy.  Output array s is [s ? ends[s - 1] : 0, ends[s]) of `out` and is the head of segment (map ? map[s] : s) of
// `src`, which starts at src_off[that segment].  A work unit is GA_UNIT consecutive OUTPUT elements (group_array_host.h ga_unit_range):
// thread 0 finds the arrays the unit touches, every element then searches only among those (none when the unit lies inside one array).
template <typename T>
__global__ __launch_bounds__(GA_T) void k_ga_seg_copy(const T * __restrict__ src, u64 src_n, const u64 * __restrict__ src_off, const u32 * __restrict__ map,
                                                      const u64 * __restrict__ ends, u64 n_segs, u64 total, T * __restrict__ out)
{
    __shared__ u64 s_range[4];
    const u64 units = ga_units(total);
    for (u64 unit = blockIdx.x; unit < units; unit += gridDim.x)
    {
        if (threadIdx.x == 0)
            ga_unit_range(ends, n_segs, total, unit, &s_range[0], &s_range[1], &s_range[2], &s_range[3]);
        __syncthreads();
        const u64 e0 = s_range[0], e1 = s_range[1], s0 = s_range[2], s1 = s_range[3];
#pragma unroll 4
        for (u32 r = 0; r < GA_UNIT_R; ++r)
        {
            const u64 e = e0 + (u64)r * GA_T + threadIdx.x;
            if (e < e1)
            {
                const u64 s = ga_seg_of(ends, s0, s1, e); // (s1 itself when no earlier array holds e)
                if (s < n_segs)
                {
                    const u64 g = map ? map[s] : s;
                    const u64 at = src_off[g] + (e - (s ? ends[s - 1] : 0));
                    if (at < src_n) // an array is never longer than its segment
                        out[e] = src[at];
                }
            }
        }
        __syncthreads(); // before the next unit overwrites the range
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
static constexpr PairNames GA_NAMES{"group_array", "operator", "an operator"};

// what finalize built from the store, kept until the store changes
struct GaFinal
{
    bool valid = false;
    u64 groups = 0, values = 0, total_out = 0;
    u32 passes = 0;
    PairMem gkeys;                   // u64[groups], ascending (keyed operators)
    PairMem src_off;                 // u64[groups + 1]: where every group's segment starts in the sorted values
    PairMem out_ends;                // u64[groups]: where every array ends (max_size != 0; else src_off + 1 is that)
    chgpu_col * sorted_v = nullptr; // the values by group (passes != 0; else the store's values are that)
};

struct chgpu_group_array : PairStore
{
    u64 max_size = 0;
    PairMem bits_mem;
    GaFinal fin;
};

static void ga_drop_final(chgpu_group_array * d)
{
    GaFinal & f = d->fin;
    if (f.sorted_v) chgpu_col_free(f.sorted_v);
    pair_free_mem(d->ctx, f.gkeys);
    pair_free_mem(d->ctx, f.src_off);
    pair_free_mem(d->ctx, f.out_ends);
    f = GaFinal{};
}

static u32 ga_grid(chgpu_ctx * ctx, u64 items) { return chgpu_grid_for(ctx, items, GA_T, 8); }
static u64 ga_tiles(u64 n) { return (n + GA_TILE - 1) / GA_TILE; }

// room for `need` values, or the row limit's answer
static int ga_reserve(chgpu_group_array * d, u64 need)
{
    CHGPU_REQUIRE(ga_capacity_for(need) != 0, CHGPU_ERR_TOO_MANY_ROWS, "group_array: %llu values, fewer than %llu fit", (unsigned long long)need,
                  (unsigned long long)GA_MAX_VALUES);
    return pair_store_reserve(GA_NAMES, *d, need);
}

extern "C" int chgpu_group_array_create(chgpu_ctx * ctx, int key_type, int value_type, uint64_t max_size, chgpu_group_array ** out)
{
    CHGPU_REQUIRE(ctx && out, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_TRY(pair_check_create(GA_NAMES, key_type, value_type));
    ChgpuDeviceGuard guard(ctx);
    chgpu_group_array * d = new chgpu_group_array();
    pair_store_init(*d, ctx, key_type, value_type, GA_NAMES.op, "test_group_array_fail_alloc");
    d->max_size = max_size;
    const int rc = chgpu_pool_alloc(ctx, 256, &d->bits_mem.p, &d->bits_mem.cls);
    if (rc != CHGPU_OK)
    {
        chgpu_group_array_free(d);
        return rc;
    }
    hipLaunchKernelGGL(k_ga_bits_init, dim3(1), dim3(1), 0, ctx->stream, (GaBits *)d->bits_mem.p);
    ctx->counters[6] += 1;
    *out = d;
    return CHGPU_OK;
}

extern "C" int chgpu_group_array_free(chgpu_group_array * d)
{
    if (!d)
        return CHGPU_OK;
    ChgpuDeviceGuard guard(d->ctx);
    ga_drop_final(d);
    pair_store_free(*d);
    pair_free_mem(d->ctx, d->bits_mem);
    chgpu_ctx * ctx = d->ctx;
    delete d;
    chgpu_ctx_release(ctx);
    return CHGPU_OK;
}

// the rows [row_begin, row_begin + n) behind the store's `held` values, in row order; *entered: how many entered.  With a filter the
// survivors are counted first and that count is read back (the one blocking read of the call), so the store grows, and answers its
// row limit, by the rows that enter and not by the rows of the range.
static int ga_append(chgpu_group_array * d, const chgpu_col * key_col, const chgpu_col * value_col, u64 row_begin, u64 n, const chgpu_col * filter_u8, u64 * entered)
{
    chgpu_ctx * ctx = d->ctx;
    const bool keyed = d->key_type >= 0;
    const u32 key_size = keyed ? (u32)chgpu_type_size(d->key_type) : 0u;
    GaBits * bits = (GaBits *)d->bits_mem.p;
    if (!filter_u8)
    {
        CHGPU_TRY(ga_reserve(d, d->held + n));
        if (keyed)
        {
            hipLaunchKernelGGL(k_ga_copy_keys, dim3(ga_grid(ctx, n)), dim3(GA_T), 0, ctx->stream, (const void *)key_col->data, key_size, row_begin, n,
                               (u64 *)d->k_mem.p + d->held, bits);
            ctx->counters[6] += 1;
        }
        CHGPU_HIP(hipMemcpyAsync((char *)d->v_mem.p + d->held * d->width, (const char *)value_col->data + row_begin * d->width, n * d->width, hipMemcpyDeviceToDevice,
                                 ctx->stream));
        CHGPU_TRY(pair_launch_ok(GA_NAMES, "append"));
        *entered = n;
        return CHGPU_OK;
    }
    PairTemps tmp(d->mem);
    const u64 n_tiles = ga_tiles(n);
    u32 * counts = nullptr;
    u64 * tile_off = nullptr; // [n_tiles], then the total
    CHGPU_TRY(tmp.alloc(n_tiles * 4, (void **)&counts));
    CHGPU_TRY(tmp.alloc((n_tiles + 1) * 8, (void **)&tile_off));
    const GaFilterPred pred{(const u8 *)filter_u8->data, row_begin};
    const dim3 grid(chgpu_grid_for(ctx, n_tiles, 1, 8)), block(GA_T);
    hipLaunchKernelGGL(k_tile_counts<GaFilterPred>, grid, block, 0, ctx->stream, pred, n, n_tiles, counts);
    ctx->counters[6] += 1;
    CHGPU_TRY(tile_scan(ctx, counts, tile_off, n_tiles, tile_off + n_tiles));
    CHGPU_TRY(pair_launch_ok(GA_NAMES, "count"));
    u64 survivors = 0;
    CHGPU_TRY(chgpu_read_back(ctx, tile_off + n_tiles, &survivors, sizeof(u64)));
    CHGPU_REQUIRE(survivors <= n, CHGPU_ERR_LOGICAL, "group_array: %llu survivors of %llu rows", (unsigned long long)survivors, (unsigned long long)n);
    if (survivors == 0)
        return CHGPU_OK;
    CHGPU_TRY(ga_reserve(d, d->held + survivors));
    dispatch_width(d->width, [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL(k_ga_append<T>, grid, block, 0, ctx->stream, keyed ? (const void *)key_col->data : nullptr, key_size, (const T *)value_col->data, pred, n, n_tiles,
                           (const u64 *)tile_off, d->held, d->cap, (u64 *)d->k_mem.p, (T *)d->v_mem.p, bits);
    });
    ctx->counters[6] += 1;
    CHGPU_TRY(pair_launch_ok(GA_NAMES, "append"));
    *entered = survivors;
    return CHGPU_OK;
}

extern "C" int chgpu_group_array_add_block(chgpu_group_array * d, const chgpu_col * key_col, const chgpu_col * value_col, uint64_t row_begin, uint64_t row_end,
                                           const chgpu_col * filter_u8)
{
    CHGPU_REQUIRE(d && value_col, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_TRY(pair_check_add_block(GA_NAMES, *d, key_col, value_col, row_begin, row_end, filter_u8));
    chgpu_ctx * ctx = d->ctx;
    ChgpuDeviceGuard guard(ctx);
    d->mem.begin_call();
    const u64 n = row_end - row_begin;
    GaAddPlan plan;
    plan.n = n;
    plan.held_before = plan.held = d->held;
    u64 entered = 0;
    const int rc = n ? ga_append(d, key_col, value_col, row_begin, n, filter_u8, &entered) : CHGPU_OK;
    if (rc == CHGPU_OK && entered) // (on an error the rows written beyond `held` are not part of the store; their bits only add passes)
    {
        ga_drop_final(d);
        d->held += entered;
        plan.entered = entered;
    }
    plan.held = d->held;
    plan.rc = rc;
    pair_print_plan(ctx, ga_format_add_plan, plan);
    return rc;
}

extern "C" int chgpu_group_array_merge(chgpu_group_array * dst, const chgpu_group_array * src)
{
    CHGPU_REQUIRE(dst && src, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_TRY(pair_check_merge(GA_NAMES, *dst, *src));
    CHGPU_REQUIRE(dst->max_size == src->max_size, CHGPU_ERR_BAD_ARGUMENTS, "group_array: merging an operator of max_size %llu into one of %llu",
                  (unsigned long long)src->max_size, (unsigned long long)dst->max_size);
    chgpu_ctx * ctx = dst->ctx;
    ChgpuDeviceGuard guard(ctx);
    dst->mem.begin_call();
    const u64 n = src->held; // (dst == src puts every array behind itself)
    GaAddPlan plan;
    plan.what = "merge";
    plan.n = n;
    plan.held_before = plan.held = dst->held;
    const int rc = pair_store_append_store(GA_NAMES, *dst, *src, [&](u64 need) { return ga_reserve(dst, need); }, [&] {
        if (dst->key_type < 0)
            return;
        hipLaunchKernelGGL(k_ga_bits_merge, dim3(1), dim3(1), 0, ctx->stream, (GaBits *)dst->bits_mem.p, (const GaBits *)src->bits_mem.p);
        ctx->counters[6] += 1;
    });
    if (rc == CHGPU_OK && n)
    {
        ga_drop_final(dst);
        plan.entered = n;
    }
    plan.held = dst->held;
    plan.rc = rc;
    pair_print_plan(ctx, ga_format_add_plan, plan);
    return rc;
}

extern "C" int chgpu_group_array_size(chgpu_group_array * d, uint64_t * values)
{
    CHGPU_REQUIRE(d && values, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    *values = d->held;
    return CHGPU_OK;
}

extern "C" int chgpu_group_array_export_pairs(chgpu_group_array * d, chgpu_col ** keys_out, chgpu_col ** values_out, uint64_t * rows)
{
    CHGPU_REQUIRE(d && values_out && rows, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    chgpu_ctx * ctx = d->ctx;
    return pair_store_export(GA_NAMES, *d, keys_out, values_out, rows, [&](chgpu_col * v) {
        ctx->counters[6] += d->key_type >= 0; // (the keys' narrowing; the values are a plain copy)
        if (hipMemcpyAsync(v->data, d->v_mem.p, d->held * d->width, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
            return chgpu_set_error(CHGPU_ERR_DEVICE, "group_array: copying the values failed");
        return (int)CHGPU_OK;
    });
}

// group keys, segment starts, array ends and the values by group of a store that holds something
static int ga_build_final(chgpu_group_array * d)
{
    chgpu_ctx * ctx = d->ctx;
    const bool keyed = d->key_type >= 0;
    GaFinal & f = d->fin;
    const u64 H = d->held;
    f.values = H;
    PairTemps tmp(d->mem);
    if (!keyed)
    {
        f.groups = 1;
        f.total_out = ga_trim(H, d->max_size);
        CHGPU_TRY(d->mem.alloc(2 * 8, &f.src_off));
        CHGPU_TRY(d->mem.alloc(8, &f.out_ends));
        hipLaunchKernelGGL(k_ga_nokey_offsets, dim3(1), dim3(1), 0, ctx->stream, (u64 *)f.src_off.p, (u64 *)f.out_ends.p, H, d->max_size);
        ctx->counters[6] += 1;
        return pair_launch_ok(GA_NAMES, "offsets");
    }
    // the one read before the passes: which key bytes vary
    GaBits bits{};
    CHGPU_TRY(chgpu_read_back(ctx, d->bits_mem.p, &bits, sizeof(bits)));
    u32 shifts[8];
    f.passes = ga_plan_passes(bits.or_bits, bits.and_bits, shifts);
    chgpu_col kview = pair_view(ctx, CHGPU_U64, d->k_mem.p, H), vview = pair_view(ctx, d->value_type, d->v_mem.p, H);
    const chgpu_col * cur[2] = {&kview, &vview};
    tmp.cols.assign(2, nullptr); // the pass's keys (freed with the call) and values (kept in the cache after the last pass)
    CHGPU_TRY(pair_run_passes(d->mem, shifts, f.passes, cur, tmp.cols.data()));
    const u64 * sk = (const u64 *)cur[0]->data;
    // run heads: counts per tile -> scan -> the group count (the second small read: the caller is told it anyway)
    const u64 n_tiles = ga_tiles(H);
    u32 * counts = nullptr;
    u64 * tile_off = nullptr;
    CHGPU_TRY(tmp.alloc(n_tiles * 4, (void **)&counts));
    CHGPU_TRY(tmp.alloc((n_tiles + 1) * 8, (void **)&tile_off));
    const dim3 tgrid(chgpu_grid_for(ctx, n_tiles, 1, 8)), block(GA_T);
    hipLaunchKernelGGL(k_tile_counts<TileHeadPred<u64>>, tgrid, block, 0, ctx->stream, TileHeadPred<u64>{sk}, H, n_tiles, counts);
    CHGPU_TRY(tile_scan(ctx, counts, tile_off, n_tiles, tile_off + n_tiles));
    ctx->counters[6] += 1;
    CHGPU_TRY(pair_launch_ok(GA_NAMES, "boundaries"));
    u64 G = 0;
    CHGPU_TRY(chgpu_read_back(ctx, tile_off + n_tiles, &G, sizeof(G)));
    CHGPU_REQUIRE(G != 0 && G <= H, CHGPU_ERR_LOGICAL, "group_array: %llu groups over %llu values", (unsigned long long)G, (unsigned long long)H);
    f.groups = G;
    CHGPU_TRY(d->mem.alloc(G * 8, &f.gkeys));
    CHGPU_TRY(d->mem.alloc((G + 1) * 8, &f.src_off));
    hipLaunchKernelGGL(k_ga_heads, tgrid, block, 0, ctx->stream, sk, H, n_tiles, (const u64 *)tile_off, G, (u64 *)f.gkeys.p, (u64 *)f.src_off.p);
    ctx->counters[6] += 1;
    CHGPU_TRY(pair_launch_ok(GA_NAMES, "heads"));
    f.total_out = H;
    if (d->max_size)
    {
        u32 * len = nullptr;
        u64 * tot = nullptr;
        CHGPU_TRY(tmp.alloc(G * 4, (void **)&len));
        CHGPU_TRY(tmp.alloc(256, (void **)&tot));
        CHGPU_TRY(d->mem.alloc(G * 8, &f.out_ends));
        hipLaunchKernelGGL(k_ga_lens, dim3(ga_grid(ctx, G)), block, 0, ctx->stream, (const u64 *)f.src_off.p, G, d->max_size, len);
        ctx->counters[6] += 1;
        CHGPU_TRY(tile_scan(ctx, len, (u64 *)f.out_ends.p, G, tot, true));
        CHGPU_TRY(chgpu_read_back(ctx, tot, &f.total_out, sizeof(u64))); // a limited operator only: how many values its arrays hold
        CHGPU_REQUIRE(f.total_out <= H, CHGPU_ERR_LOGICAL, "group_array: arrays of %llu values over %llu held", (unsigned long long)f.total_out, (unsigned long long)H);
    }
    f.sorted_v = f.passes ? tmp.cols[1] : nullptr;
    tmp.cols[1] = nullptr;
    return CHGPU_OK;
}

static int ga_ensure_final(chgpu_group_array * d, int * cached)
{
    *cached = d->fin.valid;
    if (d->fin.valid)
        return CHGPU_OK;
    ga_drop_final(d);
    const int rc = ga_build_final(d);
    if (rc != CHGPU_OK)
    {
        ga_drop_final(d);
        return rc;
    }
    d->fin.valid = true;
    return CHGPU_OK;
}

static const u64 * ga_ends(const GaFinal & f) { return f.out_ends.p ? (const u64 *)f.out_ends.p : (const u64 *)f.src_off.p + 1; }
static const void * ga_values(const chgpu_group_array * d) { return d->fin.sorted_v ? d->fin.sorted_v->data : d->v_mem.p; }

static void ga_fill_plan(const chgpu_group_array * d, int cached, GaPlan * plan)
{
    const GaFinal & f = d->fin;
    plan->groups = f.groups;
    plan->values = f.values;
    plan->passes = f.passes;
    plan->trimmed = f.values - f.total_out;
    plan->cached = cached;
}

static void ga_launch_seg_copy(chgpu_group_array * d, const u32 * map, const u64 * ends, u64 n_segs, u64 total, chgpu_col * out)
{
    chgpu_ctx * ctx = d->ctx;
    dispatch_width(d->width, [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL(k_ga_seg_copy<T>, dim3(chgpu_grid_for(ctx, ga_units(total), 1, 8)), dim3(GA_T), 0, ctx->stream, (const T *)ga_values(d), d->held,
                           (const u64 *)d->fin.src_off.p, map, ends, n_segs, total, (T *)out->data);
    });
    ctx->counters[6] += 1;
}

extern "C" int chgpu_group_array_finalize(chgpu_group_array * d, chgpu_col ** keys_out, chgpu_col ** offsets_u64, chgpu_col ** data_out, uint64_t * groups)
{
    CHGPU_REQUIRE(d && offsets_u64 && data_out && groups, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    const bool keyed = d->key_type >= 0;
    CHGPU_REQUIRE(!keyed || keys_out, CHGPU_ERR_BAD_ARGUMENTS, "NULL keys_out");
    chgpu_ctx * ctx = d->ctx;
    ChgpuDeviceGuard guard(ctx);
    d->mem.begin_call();
    chgpu_col * k = nullptr;
    chgpu_col * off = nullptr;
    chgpu_col * data = nullptr;
    GaPlan plan;
    u64 rows = 0;
    auto run = [&]() -> int {
        if (d->held == 0)
        {
            // nothing entered: no group; without key exactly one row, the empty array
            rows = keyed ? 0 : 1;
            if (keyed)
                CHGPU_TRY(d->mem.col_new(d->key_type, 0, &k));
            CHGPU_TRY(d->mem.col_new(CHGPU_U64, rows, &off));
            CHGPU_TRY(d->mem.col_new(d->value_type, 0, &data));
            if (rows)
                CHGPU_HIP(hipMemsetAsync(off->data, 0, rows * 8, ctx->stream));
            return CHGPU_OK;
        }
        int cached = 0;
        CHGPU_TRY(ga_ensure_final(d, &cached));
        const GaFinal & f = d->fin;
        ga_fill_plan(d, cached, &plan);
        rows = f.groups;
        if (keyed)
            CHGPU_TRY(d->mem.col_new(d->key_type, rows, &k));
        CHGPU_TRY(d->mem.col_new(CHGPU_U64, rows, &off));
        CHGPU_TRY(d->mem.col_new(d->value_type, f.total_out, &data));
        if (keyed)
        {
            pair_narrow(ctx, (const u64 *)f.gkeys.p, rows, k);
            ctx->counters[6] += 1;
        }
        CHGPU_HIP(hipMemcpyAsync(off->data, ga_ends(f), rows * 8, hipMemcpyDeviceToDevice, ctx->stream));
        if (f.total_out == f.values) // nothing trimmed: the values by group are the data column
            CHGPU_HIP(hipMemcpyAsync(data->data, ga_values(d), f.values * d->width, hipMemcpyDeviceToDevice, ctx->stream));
        else if (f.total_out)
            ga_launch_seg_copy(d, nullptr, ga_ends(f), f.groups, f.total_out, data);
        return pair_launch_ok(GA_NAMES, "finalize");
    };
    const int rc = run();
    if (rc != CHGPU_OK)
    {
        if (k) chgpu_col_free(k);
        if (off) chgpu_col_free(off);
        if (data) chgpu_col_free(data);
        return rc;
    }
    pair_print_plan(ctx, ga_format_plan, plan);
    if (keys_out)
        *keys_out = k;
    *offsets_u64 = off;
    *data_out = data;
    *groups = rows;
    return CHGPU_OK;
}

extern "C" int chgpu_group_array_for_keys(chgpu_group_array * d, const chgpu_col * keys, chgpu_col ** offsets_u64, chgpu_col ** data_out)
{
    CHGPU_REQUIRE(d && keys && offsets_u64 && data_out, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_TRY(pair_check_keys(GA_NAMES, *d, keys));
    CHGPU_TRY(pair_check_device(GA_NAMES, *d, keys));
    chgpu_ctx * ctx = d->ctx;
    ChgpuDeviceGuard guard(ctx);
    d->mem.begin_call();
    chgpu_col * off = nullptr;
    chgpu_col * data = nullptr;
    GaPlan plan;
    plan.what = "for_keys";
    const u64 n = keys->rows;
    auto run = [&]() -> int {
        PairTemps tmp(d->mem);
        CHGPU_TRY(d->mem.col_new(CHGPU_U64, n, &off));
        if (d->held == 0 || n == 0)
        {
            // every asked key gets the empty array; nothing is built
            if (n)
                CHGPU_HIP(hipMemsetAsync(off->data, 0, n * 8, ctx->stream));
            return d->mem.col_new(d->value_type, 0, &data);
        }
        int cached = 0;
        CHGPU_TRY(ga_ensure_final(d, &cached));
        const GaFinal & f = d->fin;
        ga_fill_plan(d, cached, &plan);
        u32 * gid = nullptr;
        u32 * len = nullptr;
        u64 * tot = nullptr;
        CHGPU_TRY(tmp.alloc(n * 4, (void **)&gid));
        CHGPU_TRY(tmp.alloc(n * 4, (void **)&len));
        CHGPU_TRY(tmp.alloc(256, (void **)&tot));
        hipLaunchKernelGGL(k_ga_lookup, dim3(ga_grid(ctx, n)), dim3(GA_T), 0, ctx->stream, (const u64 *)f.gkeys.p, f.groups, ga_ends(f), (const void *)keys->data,
                           (u32)chgpu_type_size(d->key_type), n, gid, len);
        ctx->counters[6] += 1;
        CHGPU_TRY(tile_scan(ctx, len, (u64 *)off->data, n, tot, true));
        u64 total = 0;
        CHGPU_TRY(chgpu_read_back(ctx, tot, &total, sizeof(total))); // the data column's length
        CHGPU_REQUIRE(total < (1ull << 40), CHGPU_ERR_TOO_MANY_ROWS, "group_array: the asked arrays hold %llu values", (unsigned long long)total);
        CHGPU_TRY(d->mem.col_new(d->value_type, total, &data));
        if (total)
            ga_launch_seg_copy(d, gid, (const u64 *)off->data, n, total, data);
        return pair_launch_ok(GA_NAMES, "for_keys");
    };
    const int rc = run();
    if (rc != CHGPU_OK)
    {
        if (off) chgpu_col_free(off);
        if (data) chgpu_col_free(data);
        return rc;
    }
    pair_print_plan(ctx, ga_format_plan, plan);
    *offsets_u64 = off;
    *data_out = data;
    return CHGPU_OK;
}
