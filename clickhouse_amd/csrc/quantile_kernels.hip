// quantile_kernels.hip — quantileExact / quantilesExact / medianExact (and the Low / High forms) under GROUP BY: the multiset of
// (group key, value) pairs in one flat append-only store in HBM, selected by rank at the end.
//
// Reference: QuantileExact keeps an array per group, add() is push_back (NaN skipped), get() is nth_element at
// `level < 1 ? level * size : size - 1` (src/AggregateFunctions/QuantileExact.h); Low / High differ at level 0.5 only.
//
// Design (not a translation).  Nothing is allocated per group and no table is touched while blocks arrive:
//   store    u64 keys[cap] (keyed operators), T vals[cap]: T is the unsigned type of the value's width, the value as its
//            order-preserving key (quantile_host.h qt_encode).  k_qt_append copies the rows that enter: ballot / popcount rank inside a
//            wave, one atomic per workgroup and tile of 2048 rows for the base.  The store doubles; merge appends the other store.
//   groups   finalize runs a count() chgpu_agg over the store's keys (group keys, counts), scans the counts into segment offsets,
//            builds the key -> group table (group_table.h) and scatters every value into its group's segment (k_qt_scatter: lanes of
//            a wave that hold the same group share one atomic on its cursor; k_qt_scatter_lds for few groups: a tile of rows is counted
//            per group in LDS, one atomic per group the tile met).  Kept until the store changes.
//   small    segments of at most QT_SMALL_MAX values: a workgroup takes the segments that start in one window of QT_WINDOW positions,
//            sorts them together in LDS by (segment, key) with one bitonic network and reads the ranks off (k_qt_select_small).
//   large    most-significant-byte radix select, histograms only: per value byte, work units of QT_CHUNK values count the next byte
//            of the values that match the prefix fixed so far (k_qt_hist, 256 counters per level in LDS, then added to the segment's
//            global counters); one wave per (segment, level) scans the 256 counters, fixes the byte, reduces the rank and clears them
//            (k_qt_narrow).  No host synchronisation between passes; after the last byte the prefix is the answer.
// What this operator shares with uniq_kernels.hip (element load, entry checks, the groups of the store's keys, the key -> group table)
// is pair_store.h / group_table.h; the store itself (PairStore: reserve, merge's append, export of the keys) is pair_store.h too, shared
// with group_array_kernels.hip; pool memory, the numbered allocations and a call's temporaries are pair_pool.h.  Its own: the append
// kernel, the value export, the row limit in front of the shared reserve.
#include "block_scan.h"

#include "pair_store.h"
#include "quantile_host.h"

typedef unsigned long long ull;

static constexpr u32 QT_T = 256; // threads of every kernel here

struct QtCtrl
{
    u32 held; // values in the store: the append cursor
    u32 pad;
    ull entered, nan; // of one launch
};

struct QtLevels
{
    double l[CHGPU_QUANTILE_MAX_LEVELS];
};

struct QtOut
{
    void * p[CHGPU_QUANTILE_MAX_LEVELS]; // one result column per level
};

// a large segment: where it lies in the segment array, its group, its first work unit
struct QtLarge
{
    u64 off;
    u32 n;
    u32 g;
    u64 unit0;
};

__global__ void k_qt_ctrl_reset(QtCtrl * c, u32 held)
{
    c->held = held;
    c->pad = 0;
    c->entered = c->nan = 0;
}

// add_block: the rows of [row_begin, row_begin + n) that enter, appended to the store.  key_size 0: without key.  A workgroup takes
// tiles of QT_APPEND_TILE rows: every wave counts its survivors with ballots, and ONE atomic per workgroup and tile takes the tile's
// places (a counter that every wave of the device adds to for every 64 rows is the slowest thing in the kernel).
static constexpr u32 QT_APPEND_R = 8; // rows per lane of a tile
static constexpr u64 QT_APPEND_TILE = (u64)QT_T * QT_APPEND_R;

template <typename T>
__global__ __launch_bounds__(QT_T) void k_qt_append(const void * __restrict__ key, u32 key_size, const T * __restrict__ val, const u8 * __restrict__ filter,
                                                    u64 row_begin, u64 n, int mode, u64 * __restrict__ out_k, T * __restrict__ out_v, u64 cap, QtCtrl * ctrl)
{
    __shared__ u32 s_wave[QT_T / 64];
    __shared__ u32 s_base;
    const u32 tid = threadIdx.x, wave = tid >> 6;
    u32 entered = 0, nan = 0;
    for (u64 b = (u64)blockIdx.x * QT_APPEND_TILE; b < n; b += (u64)gridDim.x * QT_APPEND_TILE)
    {
        T v[QT_APPEND_R];
        u64 m[QT_APPEND_R];
        u32 cnt = 0;
#pragma unroll
        for (u32 r = 0; r < QT_APPEND_R; ++r)
        {
            const u64 i = b + (u64)r * QT_T + tid;
            bool in = i < n;
            const u64 row = row_begin + (in ? i : 0);
            if (in && filter)
                in = filter[row] != 0;
            v[r] = in ? val[row] : (T)0;
            if (in && mode == QT_MODE_FLOAT && qt_is_nan(v[r], sizeof(T)))
            {
                in = false;
                nan += 1;
            }
            m[r] = __ballot(in);
            cnt += (u32)__popcll(m[r]);
        }
        if (lane_id() == 0)
            s_wave[wave] = cnt;
        __syncthreads();
        if (tid == 0)
        {
            u32 total = 0;
            for (u32 w = 0; w < QT_T / 64; ++w)
                total += s_wave[w];
            s_base = total ? atomicAdd(&ctrl->held, total) : 0;
        }
        __syncthreads();
        u64 off = s_base;
        for (u32 w = 0; w < wave; ++w)
            off += s_wave[w];
#pragma unroll
        for (u32 r = 0; r < QT_APPEND_R; ++r)
        {
            if ((m[r] >> lane_id()) & 1)
            {
                const u64 pos = off + mbcnt(m[r]);
                if (pos < cap) // never past the store (the host reserved held + n)
                {
                    if (key_size)
                        out_k[pos] = pair_load(key, key_size, row_begin + b + (u64)r * QT_T + tid);
                    out_v[pos] = (T)qt_encode(v[r], sizeof(T), mode);
                    entered += 1;
                }
            }
            off += (u32)__popcll(m[r]);
        }
        __syncthreads(); // before the next tile overwrites the counts
    }
    entered = wave_reduce_add_u32(entered);
    nan = wave_reduce_add_u32(nan);
    if (lane_id() == 0)
    {
        if (entered) atomicAdd(&ctrl->entered, (ull)entered);
        if (nan) atomicAdd(&ctrl->nan, (ull)nan);
    }
}

// export_pairs: values decoded (the keys go back to the key type through pair_narrow)
template <typename T>
__global__ __launch_bounds__(QT_T) void k_qt_export_values(const T * __restrict__ in, u64 n, int mode, T * __restrict__ out)
{
    for (u64 i = (u64)blockIdx.x * QT_T + threadIdx.x; i < n; i += (u64)gridDim.x * QT_T)
        out[i] = (T)qt_decode(in[i], sizeof(T), mode);
}

template <typename T>
__global__ __launch_bounds__(QT_T) void k_qt_fill(QtOut out, u32 n_levels, u64 n, T v)
{
    for (u64 i = (u64)blockIdx.x * QT_T + threadIdx.x; i < n; i += (u64)gridDim.x * QT_T)
        for (u32 l = 0; l < n_levels; ++l)
            ((T *)out.p[l])[i] = v;
}

// per group: the 32-bit count, whether the segment is large, its work units
__global__ __launch_bounds__(QT_T) void k_qt_classify(const u64 * __restrict__ counts, u64 groups, u32 * __restrict__ c32, u32 * __restrict__ flag, u32 * __restrict__ units,
                                                      ull * __restrict__ broken)
{
    for (u64 g = (u64)blockIdx.x * QT_T + threadIdx.x; g < groups; g += (u64)gridDim.x * QT_T)
    {
        const u64 n = counts[g];
        if (n == 0 || n > QT_MAX_VALUES) // a group exists through a value: the windows of k_qt_select_small rest on offsets that ascend strictly
            atomicAdd(broken, 1ull);
        c32[g] = (u32)n;
        flag[g] = !qt_is_small(n);
        units[g] = (u32)qt_units(n);
    }
}

__global__ __launch_bounds__(QT_T) void k_qt_large_list(const u32 * __restrict__ c32, const u64 * __restrict__ offsets, const u32 * __restrict__ flag,
                                                        const u64 * __restrict__ lidx, const u64 * __restrict__ uoff, u64 groups, QtLarge * __restrict__ out)
{
    for (u64 g = (u64)blockIdx.x * QT_T + threadIdx.x; g < groups; g += (u64)gridDim.x * QT_T)
        if (flag[g])
        {
            QtLarge s;
            s.off = offsets[g];
            s.n = c32[g];
            s.g = (u32)g;
            s.unit0 = uoff[g];
            out[lidx[g]] = s;
        }
}

// Every stored value to offsets[g] + cursor[g]++ of the segment array.  Lanes of a wave that hold the leader's group take their places
// with one atomic (QT_SHARE_ROUNDS leaders, which settles a wave whose rows fall into a few groups); whoever is left after that takes
// its place alone: with many groups a wave's lanes rarely meet, and their cursors are as many different addresses.
static constexpr u32 QT_SHARE_ROUNDS = 4;

// (a place past the segment array cannot come out of counts that add up to n; it is counted, never written)
template <typename T>
__device__ __forceinline__ void qt_place(T * __restrict__ seg, u64 n, u64 at, T v, u32 * __restrict__ lost)
{
    if (at < n)
        seg[at] = v;
    else
        atomicAdd(lost, 1u);
}

template <typename T>
__global__ __launch_bounds__(QT_T) void k_qt_scatter(const u64 * __restrict__ store_k, const T * __restrict__ store_v, u64 n, const u64 * __restrict__ gkeys,
                                                     const u32 * __restrict__ cells, u64 cap, const u64 * __restrict__ offsets, u32 * __restrict__ cursor,
                                                     u32 * __restrict__ lost, T * __restrict__ seg)
{
    for (u64 b = (u64)blockIdx.x * QT_T; b < n; b += (u64)gridDim.x * QT_T)
    {
        const u64 i = b + threadIdx.x;
        bool todo = i < n;
        u32 g = GT_NONE;
        T v = 0;
        if (todo)
        {
            g = gt_find(gkeys, cells, cap, store_k[i]);
            v = store_v[i];
            if (g == GT_NONE) // cannot happen: the groups were made from these keys
            {
                atomicAdd(lost, 1u);
                todo = false;
            }
        }
        for (u32 round = 0; round < QT_SHARE_ROUNDS; ++round)
        {
            const u64 left = __ballot(todo);
            if (left == 0)
                break;
            const u32 leader = (u32)__ffsll((long long)left) - 1;
            const u32 lg = __shfl(g, (int)leader, 64);
            const bool mine = todo && g == lg;
            const u64 m = __ballot(mine);
            if ((u32)__popcll(m) * 8 < (u32)__popcll(left)) // a wave of many groups: sharing would only add round trips
                break;
            u32 base = 0;
            if (lane_id() == leader)
                base = atomicAdd(&cursor[lg], (u32)__popcll(m));
            base = __shfl(base, (int)leader, 64);
            if (mine)
            {
                qt_place(seg, n, offsets[g] + base + mbcnt(m), v, lost);
                todo = false;
            }
        }
        if (todo)
            qt_place(seg, n, offsets[g] + atomicAdd(&cursor[g], 1u), v, lost);
    }
}

// The same for few groups (at most QT_SCATTER_LDS_GROUPS): rows in random order put nearly every lane of a wave into another group, and
// with few groups that is one atomic per row on a few hot cursors.  A workgroup counts a tile of rows per group in LDS (the LDS atomic
// returns the row's rank inside the tile), takes the tile's places with one atomic per group it met, and writes.
static constexpr u32 QT_SCATTER_LDS_GROUPS = 4096;
static constexpr u32 QT_SCATTER_R = 16; // rows per lane of a tile

template <typename T>
__global__ __launch_bounds__(QT_T) void k_qt_scatter_lds(const u64 * __restrict__ store_k, const T * __restrict__ store_v, u64 n, const u64 * __restrict__ gkeys,
                                                         const u32 * __restrict__ cells, u64 cap, const u64 * __restrict__ offsets, u32 * __restrict__ cursor,
                                                         u32 * __restrict__ lost, T * __restrict__ seg, u32 groups)
{
    __shared__ u32 lcnt[QT_SCATTER_LDS_GROUPS]; // the tile's rows per group, then the group's base for this tile
    const u32 tid = threadIdx.x;
    const u64 tile = (u64)QT_T * QT_SCATTER_R;
    for (u64 b = (u64)blockIdx.x * tile; b < n; b += (u64)gridDim.x * tile)
    {
        for (u32 c = tid; c < groups; c += QT_T)
            lcnt[c] = 0;
        __syncthreads();
        u32 g[QT_SCATTER_R], rk[QT_SCATTER_R];
        T v[QT_SCATTER_R];
#pragma unroll
        for (u32 r = 0; r < QT_SCATTER_R; ++r)
        {
            const u64 i = b + (u64)r * QT_T + tid;
            g[r] = GT_NONE;
            rk[r] = 0;
            v[r] = 0;
            if (i < n)
            {
                g[r] = gt_find(gkeys, cells, cap, store_k[i]);
                v[r] = store_v[i];
                if (g[r] < groups)
                    rk[r] = atomicAdd(&lcnt[g[r]], 1u);
                else // cannot happen: the groups were made from these keys
                {
                    g[r] = GT_NONE;
                    atomicAdd(lost, 1u);
                }
            }
        }
        __syncthreads();
        for (u32 c = tid; c < groups; c += QT_T)
        {
            const u32 cnt = lcnt[c];
            if (cnt)
                lcnt[c] = atomicAdd(&cursor[c], cnt);
        }
        __syncthreads();
#pragma unroll
        for (u32 r = 0; r < QT_SCATTER_R; ++r)
            if (g[r] != GT_NONE)
                qt_place(seg, n, offsets[g[r]] + lcnt[g[r]] + rk[r], v[r], lost);
        __syncthreads(); // before the next tile clears the counts
    }
}

// (segment id, key) ascending
template <typename T>
__device__ __forceinline__ bool qt_pair_greater(u16 sa, T ka, u16 sb, T kb)
{
    return sa != sb ? sa > sb : ka > kb;
}

// Small segments.  Window w owns the segments that start in [w * QT_WINDOW, (w + 1) * QT_WINDOW); a large one can only be the last of
// them, so the small ones are consecutive positions from the first segment's start, fewer than QT_TILE.  The workgroup loads them, tags
// every position with its segment, sorts by (segment, key) -- which leaves every segment in its own range, sorted -- and writes the
// requested ranks.
template <typename T>
__global__ __launch_bounds__(QT_T) void k_qt_select_small(const T * __restrict__ seg, const u64 * __restrict__ offsets, const u32 * __restrict__ counts, u64 groups,
                                                          u64 values, int kind, QtLevels lv, u32 n_levels, int mode, QtOut out)
{
    __shared__ T tile[QT_TILE];
    __shared__ u16 sid[QT_TILE];
    __shared__ u32 loff[QT_WINDOW + 1]; // the window's segments' starts, relative to the first; at most one segment per position
    __shared__ u64 s_g[2];
    __shared__ u32 s_extent;
    const u32 tid = threadIdx.x;
    const u64 windows = qt_windows(values);
    for (u64 w = blockIdx.x; w < windows; w += gridDim.x)
    {
        if (tid == 0)
        {
            u64 a, b;
            qt_window_groups(offsets, groups, w, &a, &b);
            s_g[0] = a;
            s_g[1] = b;
            s_extent = 0;
        }
        __syncthreads();
        const u64 g0 = s_g[0], g1 = s_g[1];
        const u32 ng = (u32)(g1 - g0);
        const u64 lo = ng ? offsets[g0] : 0;
        for (u32 j = tid; j < ng; j += QT_T)
        {
            const u32 n = counts[g0 + j];
            const u32 o = (u32)(offsets[g0 + j] - lo);
            loff[j] = o;
            if (qt_is_small(n))
                atomicMax(&s_extent, o + n);
        }
        __syncthreads();
        const u32 extent = s_extent; // positions up to the end of the window's last small segment; 0: it has none
        if (extent != 0 && extent <= QT_TILE && ng <= QT_WINDOW) // (the bounds hold for offsets that ascend strictly)
        {
            u32 P = 64;
            while (P < extent)
                P <<= 1;
            for (u32 p = tid; p < P; p += QT_T)
            {
                if (p < extent)
                {
                    u32 a = 0, b = ng; // the last segment that starts at or before p
                    while (b - a > 1)
                    {
                        const u32 mid = (a + b) / 2;
                        if (loff[mid] <= p)
                            a = mid;
                        else
                            b = mid;
                    }
                    sid[p] = (u16)a;
                    tile[p] = seg[lo + p];
                }
                else
                {
                    sid[p] = 0xFFFF;
                    tile[p] = 0;
                }
            }
            __syncthreads();
            for (u32 k = 2; k <= P; k <<= 1)
                for (u32 j = k >> 1; j > 0; j >>= 1)
                {
                    for (u32 t = tid; t < P / 2; t += QT_T)
                    {
                        const u32 i = (t / j) * 2 * j + (t % j), x = i + j;
                        const u16 sa = sid[i], sb = sid[x];
                        const T ka = tile[i], kb = tile[x];
                        const bool up = (i & k) == 0;
                        if (qt_pair_greater(sa, ka, sb, kb) == up)
                        {
                            sid[i] = sb;
                            sid[x] = sa;
                            tile[i] = kb;
                            tile[x] = ka;
                        }
                    }
                    __syncthreads();
                }
            for (u32 e = tid; e < ng * n_levels; e += QT_T)
            {
                const u32 j = e / n_levels, l = e % n_levels;
                const u32 n = counts[g0 + j];
                if (qt_is_small(n))
                    ((T *)out.p[l])[g0 + j] = (T)qt_decode(tile[loff[j] + (u32)qt_rank(kind, lv.l[l], n)], sizeof(T), mode);
            }
        }
        else if (extent != 0) // not reached while every group holds a value (checked where the groups are made); never silent garbage
            for (u32 e = tid; e < ng * n_levels; e += QT_T)
                if (qt_is_small(counts[g0 + e / n_levels]))
                    ((T *)out.p[e % n_levels])[g0 + e / n_levels] = (T)qt_empty_bits(sizeof(T), mode);
        __syncthreads(); // before the next window overwrites LDS
    }
}

// per (large segment, level): no byte fixed, the rank asked for
__global__ __launch_bounds__(QT_T) void k_qt_state_init(const QtLarge * __restrict__ lseg, u64 large, int kind, QtLevels lv, u32 n_levels, u64 * __restrict__ prefix,
                                                        u64 * __restrict__ rank)
{
    for (u64 e = (u64)blockIdx.x * QT_T + threadIdx.x; e < large * n_levels; e += (u64)gridDim.x * QT_T)
    {
        prefix[e] = 0;
        rank[e] = qt_rank(kind, lv.l[e % n_levels], lseg[e / n_levels].n);
    }
}

// One histogram pass over byte `byte` of the large segments' values, for the levels [l0, l0 + bl).  A work unit is QT_CHUNK values of one
// segment; a value counts for a level when its bytes above `byte` equal the level's prefix.
static constexpr u32 QT_HIST_ROUNDS = 4;

template <typename T>
__global__ __launch_bounds__(QT_T) void k_qt_hist(const T * __restrict__ seg, const QtLarge * __restrict__ lseg, u64 large, u64 units, u32 byte, u32 l0, u32 bl,
                                                  u32 n_levels, const u64 * __restrict__ prefix, u32 * __restrict__ hist, u32 rounds)
{
    __shared__ u32 h[256 * CHGPU_QUANTILE_MAX_LEVELS];
    __shared__ u64 s_pref[CHGPU_QUANTILE_MAX_LEVELS];
    __shared__ u64 s_li;
    const u32 tid = threadIdx.x;
    const bool first = byte + 1 == sizeof(T); // no byte fixed yet: every value counts
    const u32 counted = first ? 1 : bl;
    const u32 sh = 8 * byte;
    for (u64 unit = blockIdx.x; unit < units; unit += gridDim.x)
    {
        if (tid == 0)
        {
            u64 a = 0, b = large; // the last segment whose first unit is at or before this one
            while (b - a > 1)
            {
                const u64 mid = a + (b - a) / 2;
                if (lseg[mid].unit0 <= unit)
                    a = mid;
                else
                    b = mid;
            }
            s_li = a;
        }
        for (u32 c = tid; c < 256 * bl; c += QT_T)
            h[c] = 0;
        __syncthreads();
        const u64 li = s_li;
        if (tid < bl)
            s_pref[tid] = prefix[li * n_levels + l0 + tid];
        __syncthreads();
        const QtLarge s = lseg[li];
        const u64 begin = s.off + (unit - s.unit0) * QT_CHUNK;
        const u64 seg_end = s.off + s.n;
        const u64 end = begin + QT_CHUNK < seg_end ? begin + QT_CHUNK : seg_end;
        for (u64 b = begin; b < end; b += QT_T)
        {
            const u64 i = b + tid;
            const bool valid = i < end;
            const u64 v = valid ? (u64)seg[i] : 0;
            const u32 bin = (u32)(v >> sh) & 0xFF;
            for (u32 l = 0; l < counted; ++l)
            {
                const bool match = valid && (first || ((v ^ s_pref[l]) >> (sh + 8)) == 0);
                const u64 m = __ballot(match);
                // Up to QT_HIST_ROUNDS bins of the wave are added once each by a leader (equal values, the sign and exponent bytes of
                // like floats: 64 lanes on a few LDS words would take turns); a wave whose values spread over many bins adds lane by lane.
                u64 left = m;
                for (u32 round = 0; round < rounds && left; ++round)
                {
                    const u32 leader = (u32)__ffsll((long long)left) - 1;
                    const u32 b0 = __shfl(bin, (int)leader, 64);
                    const u64 same = __ballot(match && bin == b0) & left;
                    if ((u32)__popcll(same) * 8 < (u32)__popcll(left))
                        break;
                    if (lane_id() == leader)
                        atomicAdd(&h[l * 256 + b0], (u32)__popcll(same));
                    left &= ~same;
                }
                if ((left >> lane_id()) & 1)
                    atomicAdd(&h[l * 256 + bin], 1u);
            }
        }
        __syncthreads();
        // (before a byte is fixed every level of the batch has the same histogram: counted once, added to each)
        for (u32 c = tid; c < 256 * bl; c += QT_T)
        {
            const u32 x = first ? h[c % 256] : h[c];
            if (x)
                atomicAdd(&hist[(li * bl + c / 256) * 256 + c % 256], x);
        }
        __syncthreads(); // before the next unit clears LDS
    }
}

// One wave per (large segment, level of the batch): the byte whose counters hold the rank is the prefix's next byte; the rank goes on
// relative to that bin; the counters are cleared for the next pass.  After byte 0 the prefix is the answer.
template <typename T>
__global__ __launch_bounds__(QT_T) void k_qt_narrow(const QtLarge * __restrict__ lseg, u64 large, u32 byte, u32 l0, u32 bl, u32 n_levels, u64 * __restrict__ prefix,
                                                    u64 * __restrict__ rank, u32 * __restrict__ hist, int mode, QtOut out)
{
    const u64 w = ((u64)blockIdx.x * QT_T + threadIdx.x) / 64;
    if (w >= large * bl)
        return;
    const u32 lane = lane_id();
    const u64 li = w / bl;
    const u32 l = l0 + (u32)(w % bl);
    u32 * h = hist + w * 256;
    u32 c[4];
    u32 s = 0;
#pragma unroll
    for (u32 k = 0; k < 4; ++k)
    {
        c[k] = h[lane * 4 + k];
        s += c[k];
    }
    const u32 incl = wave_scan_inclusive<AddU32>(s, lane);
    const u64 e = li * n_levels + l;
    const u64 r = rank[e];
    const u64 hit = __ballot((u64)incl > r);
    const u32 owner = hit ? (u32)__ffsll((long long)hit) - 1 : 63; // (the counters hold the segment's matching values, more than r)
    if (lane == owner)
    {
        u64 rr = r - (incl - s);
        u32 k = 0;
        while (k < 3 && rr >= c[k])
        {
            rr -= c[k];
            ++k;
        }
        const u64 p = prefix[e] | ((u64)(lane * 4 + k) << (8 * byte));
        prefix[e] = p;
        rank[e] = rr;
        if (byte == 0)
            ((T *)out.p[l])[lseg[li].g] = (T)qt_decode(p, sizeof(T), mode);
    }
#pragma unroll
    for (u32 k = 0; k < 4; ++k)
        h[lane * 4 + k] = 0;
}

// for_keys: row i gets its key's group's results, the empty-state value when no group has the key
template <typename T>
__global__ __launch_bounds__(QT_T) void k_qt_gather(const u64 * __restrict__ gkeys, const u32 * __restrict__ cells, u64 cap, const void * __restrict__ keys, u32 key_size,
                                                    u64 n, QtOut res, QtOut out, u32 n_levels, T empty)
{
    for (u64 i = (u64)blockIdx.x * QT_T + threadIdx.x; i < n; i += (u64)gridDim.x * QT_T)
    {
        const u32 g = gt_find(gkeys, cells, cap, pair_load(keys, key_size, i));
        for (u32 l = 0; l < n_levels; ++l)
            ((T *)out.p[l])[i] = g == GT_NONE ? empty : ((const T *)res.p[l])[g];
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
static constexpr PairNames QT_NAMES{"quantile", "operator", "an operator"};

// what finalize computed from the store, kept until the store changes
struct QtFinal
{
    bool valid = false;
    u64 groups = 0, values = 0, small = 0, large = 0, units = 0;
    chgpu_col * gkeys = nullptr; // UInt64 group keys (keyed operators)
    PairMem counts;                // u32[groups]
    PairMem offsets;               // u64[groups + 1]
    PairMem cells;                 // key -> group table
    u64 cells_cap = 0;
    PairMem seg;                   // the segment array (keyed operators; without key the store's values are the one segment)
    PairMem lseg;                  // QtLarge[large]
};

struct chgpu_quantile : PairStore
{
    int mode = 0;
    PairMem ctrl_mem;
    QtFinal fin;
};

static void qt_drop_final(chgpu_quantile * d)
{
    QtFinal & f = d->fin;
    if (f.gkeys) chgpu_col_free(f.gkeys);
    pair_free_mem(d->ctx, f.counts);
    pair_free_mem(d->ctx, f.offsets);
    pair_free_mem(d->ctx, f.cells);
    pair_free_mem(d->ctx, f.seg);
    pair_free_mem(d->ctx, f.lseg);
    f = QtFinal{};
}

static u32 qt_grid(chgpu_ctx * ctx, u64 items) { return chgpu_grid_for(ctx, items, QT_T, 8); }

// room for `need` values, or the row limit's answer
static int qt_reserve(chgpu_quantile * d, u64 need)
{
    if (need <= d->cap)
        return CHGPU_OK;
    CHGPU_REQUIRE(need < QT_MAX_VALUES, CHGPU_ERR_TOO_MANY_ROWS, "quantile: %llu values, fewer than %llu fit", (unsigned long long)need, (unsigned long long)QT_MAX_VALUES);
    return pair_store_reserve(QT_NAMES, *d, need);
}

extern "C" int chgpu_quantile_create(chgpu_ctx * ctx, int key_type, int value_type, chgpu_quantile ** out)
{
    CHGPU_REQUIRE(ctx && out, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_TRY(pair_check_create(QT_NAMES, key_type, value_type));
    ChgpuDeviceGuard guard(ctx);
    chgpu_quantile * d = new chgpu_quantile();
    pair_store_init(*d, ctx, key_type, value_type, QT_NAMES.op, "test_quantile_fail_alloc");
    d->mode = chgpu_type_is_float(value_type) ? QT_MODE_FLOAT : chgpu_type_is_signed(value_type) ? QT_MODE_SIGNED : QT_MODE_UNSIGNED;
    const int rc = chgpu_pool_alloc(ctx, 256, &d->ctrl_mem.p, &d->ctrl_mem.cls);
    if (rc != CHGPU_OK)
    {
        chgpu_quantile_free(d);
        return rc;
    }
    *out = d;
    return CHGPU_OK;
}

extern "C" int chgpu_quantile_free(chgpu_quantile * d)
{
    if (!d)
        return CHGPU_OK;
    ChgpuDeviceGuard guard(d->ctx);
    qt_drop_final(d);
    pair_store_free(*d);
    pair_free_mem(d->ctx, d->ctrl_mem);
    chgpu_ctx * ctx = d->ctx;
    delete d;
    chgpu_ctx_release(ctx);
    return CHGPU_OK;
}

extern "C" int chgpu_quantile_add_block(chgpu_quantile * d, const chgpu_col * key_col, const chgpu_col * value_col, uint64_t row_begin, uint64_t row_end,
                                        const chgpu_col * filter_u8)
{
    CHGPU_REQUIRE(d && value_col, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_TRY(pair_check_add_block(QT_NAMES, *d, key_col, value_col, row_begin, row_end, filter_u8));
    const bool keyed = d->key_type >= 0;
    chgpu_ctx * ctx = d->ctx;
    ChgpuDeviceGuard guard(ctx);
    d->mem.begin_call();
    const u64 n = row_end - row_begin;
    QtAddPlan plan;
    plan.n = n;
    plan.held_before = plan.held = d->held;
    int rc = n ? qt_reserve(d, d->held + n) : CHGPU_OK;
    if (rc == CHGPU_OK && n)
    {
        QtCtrl * ctrl = (QtCtrl *)d->ctrl_mem.p;
        hipLaunchKernelGGL(k_qt_ctrl_reset, dim3(1), dim3(1), 0, ctx->stream, ctrl, (u32)d->held);
        const dim3 grid(qt_grid(ctx, (n + QT_APPEND_R - 1) / QT_APPEND_R)), block(QT_T);
        dispatch_width(d->width, [&](auto tag) {
            typedef decltype(tag) T;
            hipLaunchKernelGGL(k_qt_append<T>, grid, block, 0, ctx->stream, keyed ? key_col->data : nullptr, keyed ? (u32)chgpu_type_size(d->key_type) : 0u,
                               (const T *)value_col->data, filter_u8 ? (const u8 *)filter_u8->data : nullptr, row_begin, n, d->mode, (u64 *)d->k_mem.p, (T *)d->v_mem.p,
                               d->cap, ctrl);
        });
        ctx->counters[6] += 2;
        rc = pair_launch_ok(QT_NAMES, "append");
        QtCtrl c{};
        if (rc == CHGPU_OK)
            rc = chgpu_read_back(ctx, ctrl, &c, sizeof(c)); // the one blocking read of the call
        if (rc == CHGPU_OK)
        {
            plan.entered = c.entered;
            plan.nan = c.nan;
            if (c.entered)
                qt_drop_final(d);
            d->held += c.entered; // (on an error the rows written beyond `held` are not part of the store)
        }
    }
    plan.held = d->held;
    plan.rc = rc;
    pair_print_plan(ctx, qt_format_add_plan, plan);
    return rc;
}

extern "C" int chgpu_quantile_merge(chgpu_quantile * dst, const chgpu_quantile * src)
{
    CHGPU_REQUIRE(dst && src, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_TRY(pair_check_merge(QT_NAMES, *dst, *src));
    chgpu_ctx * ctx = dst->ctx;
    ChgpuDeviceGuard guard(ctx);
    dst->mem.begin_call();
    const u64 n = src->held; // (dst == src doubles every value: a multiset union with itself)
    QtAddPlan plan;
    plan.what = "merge";
    plan.n = n;
    plan.held_before = plan.held = dst->held;
    const int rc = pair_store_append_store(QT_NAMES, *dst, *src, [&](u64 need) { return qt_reserve(dst, need); }, [] {});
    if (rc == CHGPU_OK && n)
    {
        qt_drop_final(dst);
        plan.entered = n;
    }
    plan.held = dst->held;
    plan.rc = rc;
    pair_print_plan(ctx, qt_format_add_plan, plan);
    return rc;
}

extern "C" int chgpu_quantile_size(chgpu_quantile * d, uint64_t * values)
{
    CHGPU_REQUIRE(d && values, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    *values = d->held;
    return CHGPU_OK;
}

extern "C" int chgpu_quantile_export_pairs(chgpu_quantile * d, chgpu_col ** keys_out, chgpu_col ** values_out, uint64_t * rows)
{
    CHGPU_REQUIRE(d && values_out && rows, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    chgpu_ctx * ctx = d->ctx;
    return pair_store_export(QT_NAMES, *d, keys_out, values_out, rows, [&](chgpu_col * v) {
        dispatch_width(d->width, [&](auto tag) {
            typedef decltype(tag) T;
            hipLaunchKernelGGL(k_qt_export_values<T>, dim3(qt_grid(ctx, d->held)), dim3(QT_T), 0, ctx->stream, (const T *)d->v_mem.p, d->held, d->mode, (T *)v->data);
        });
        ctx->counters[6] += 2;
        return CHGPU_OK;
    });
}

// groups, segment offsets, the classes of the segments, the key table and the segment array of the store as it stands
static int qt_build_final(chgpu_quantile * d)
{
    chgpu_ctx * ctx = d->ctx;
    const bool keyed = d->key_type >= 0;
    QtFinal & f = d->fin;
    f.values = d->held;
    PairTemps tmp(d->mem);
    chgpu_col * counts = nullptr;
    if (keyed)
        CHGPU_TRY(pair_count_groups(ctx, d->k_mem.p, d->held, nullptr, &f.gkeys, &counts, &f.groups));
    else
    {
        f.groups = 1;
        CHGPU_TRY(chgpu_col_new(ctx, CHGPU_U64, 1, &counts));
        pair_set_u64(ctx, (u64 *)counts->data, d->held);
        ctx->counters[6] += 1;
    }
    struct FreeCol
    {
        chgpu_col * c;
        ~FreeCol() { if (c) chgpu_col_free(c); }
    } free_counts{counts};
    const u64 G = f.groups;
    CHGPU_REQUIRE(G != 0 && G < GT_NONE, CHGPU_ERR_LOGICAL, "quantile: %llu groups over %llu values", (unsigned long long)G, (unsigned long long)d->held);
    u32 * flag = nullptr;
    u32 * units = nullptr;
    u64 * lidx = nullptr;
    u64 * uoff = nullptr;
    u64 * tot = nullptr;
    CHGPU_TRY(d->mem.alloc(G * 4, &f.counts));
    CHGPU_TRY(d->mem.alloc((G + 1) * 8, &f.offsets));
    CHGPU_TRY(tmp.alloc(G * 4, (void **)&flag));
    CHGPU_TRY(tmp.alloc(G * 4, (void **)&units));
    CHGPU_TRY(tmp.alloc(G * 8, (void **)&lidx));
    CHGPU_TRY(tmp.alloc(G * 8, (void **)&uoff));
    CHGPU_TRY(tmp.alloc(256, (void **)&tot));
    u32 * c32 = (u32 *)f.counts.p;
    u64 * offsets = (u64 *)f.offsets.p;
    const dim3 ggrid(qt_grid(ctx, G)), block(QT_T);
    CHGPU_HIP(hipMemsetAsync(tot, 0, 3 * sizeof(u64), ctx->stream));
    hipLaunchKernelGGL(k_qt_classify, ggrid, block, 0, ctx->stream, (const u64 *)counts->data, G, c32, flag, units, (ull *)(tot + 2));
    ctx->counters[6] += 2;
    CHGPU_TRY(pair_launch_ok(QT_NAMES, "classify"));
    void * scan_tmp = nullptr;
    const size_t scan_bytes = chgpu_scan_tmp_bytes(G);
    CHGPU_TRY(chgpu_scratch(ctx, scan_bytes, &scan_tmp));
    CHGPU_TRY(chgpu_scan_exclusive_u32_u64(ctx, c32, offsets, G, offsets + G, scan_tmp, scan_bytes));
    CHGPU_TRY(chgpu_scan_exclusive_u32_u64(ctx, flag, lidx, G, tot, scan_tmp, scan_bytes));
    CHGPU_TRY(chgpu_scan_exclusive_u32_u64(ctx, units, uoff, G, tot + 1, scan_tmp, scan_bytes));
    u64 totals[3] = {0, 0, 0};
    CHGPU_TRY(chgpu_read_back(ctx, tot, totals, sizeof(totals))); // large segments, their work units, broken counts: all that crosses to the host
    CHGPU_REQUIRE(totals[2] == 0, CHGPU_ERR_LOGICAL, "quantile: %llu groups with no value or too many", (unsigned long long)totals[2]);
    f.large = totals[0];
    f.units = totals[1];
    f.small = G - f.large;
    if (f.large)
    {
        CHGPU_TRY(d->mem.alloc(f.large * sizeof(QtLarge), &f.lseg));
        hipLaunchKernelGGL(k_qt_large_list, ggrid, block, 0, ctx->stream, c32, offsets, flag, lidx, uoff, G, (QtLarge *)f.lseg.p);
        ctx->counters[6] += 1;
        CHGPU_TRY(pair_launch_ok(QT_NAMES, "large list"));
    }
    if (!keyed)
        return CHGPU_OK; // one segment: the store's values
    f.cells_cap = gt_capacity_for(G);
    CHGPU_TRY(d->mem.alloc(f.cells_cap * 4, &f.cells));
    CHGPU_TRY(d->mem.alloc(d->held * d->width, &f.seg));
    u32 * cursor = nullptr; // [G] cursors, then the count of values whose key found no group
    CHGPU_TRY(tmp.alloc((G + 1) * 4, (void **)&cursor));
    CHGPU_TRY(gt_fill(ctx, QT_NAMES.op, (const u64 *)f.gkeys->data, G, (u32 *)f.cells.p, f.cells_cap));
    CHGPU_HIP(hipMemsetAsync(cursor, 0, (G + 1) * 4, ctx->stream));
    const dim3 vgrid(qt_grid(ctx, d->held));
    dispatch_width(d->width, [&](auto tag) {
        typedef decltype(tag) T;
        if (G <= QT_SCATTER_LDS_GROUPS && chgpu_opt(ctx, "tune_quantile_no_lds_scatter", 0) == 0)
            hipLaunchKernelGGL(k_qt_scatter_lds<T>, dim3(qt_grid(ctx, (d->held + QT_SCATTER_R - 1) / QT_SCATTER_R)), block, 0, ctx->stream, (const u64 *)d->k_mem.p,
                               (const T *)d->v_mem.p, d->held, (const u64 *)f.gkeys->data, (const u32 *)f.cells.p, f.cells_cap, (const u64 *)offsets, cursor, cursor + G,
                               (T *)f.seg.p, (u32)G);
        else
            hipLaunchKernelGGL(k_qt_scatter<T>, vgrid, block, 0, ctx->stream, (const u64 *)d->k_mem.p, (const T *)d->v_mem.p, d->held, (const u64 *)f.gkeys->data,
                               (const u32 *)f.cells.p, f.cells_cap, (const u64 *)offsets, cursor, cursor + G, (T *)f.seg.p);
    });
    ctx->counters[6] += 4;
    CHGPU_TRY(pair_launch_ok(QT_NAMES, "scatter"));
    u32 lost = 0;
    CHGPU_TRY(chgpu_read_back(ctx, cursor + G, &lost, sizeof(lost)));
    CHGPU_REQUIRE(lost == 0, CHGPU_ERR_LOGICAL, "quantile: %u stored values found no place in their group's segment", lost);
    return CHGPU_OK;
}

static int qt_ensure_final(chgpu_quantile * d, int * cached)
{
    *cached = d->fin.valid;
    if (d->fin.valid)
        return CHGPU_OK;
    qt_drop_final(d);
    const int rc = qt_build_final(d);
    if (rc != CHGPU_OK)
    {
        qt_drop_final(d);
        return rc;
    }
    d->fin.valid = true;
    return CHGPU_OK;
}

// The quantiles of every group of a store that holds something: res[l] (allocated here, fin.groups rows) answers levels[l].
static int qt_select(chgpu_quantile * d, int kind, u32 n_levels, const double * levels, chgpu_col ** res, QtPlan * plan)
{
    chgpu_ctx * ctx = d->ctx;
    int cached = 0;
    CHGPU_TRY(qt_ensure_final(d, &cached));
    const QtFinal & f = d->fin;
    PairTemps tmp(d->mem);
    QtLevels lv{};
    QtOut out{};
    for (u32 l = 0; l < n_levels; ++l)
    {
        lv.l[l] = levels[l];
        CHGPU_TRY(d->mem.col_new(d->value_type, f.groups, &res[l]));
        out.p[l] = res[l]->data;
    }
    const u32 bl = qt_level_batch(f.large, n_levels, (u64)chgpu_opt(ctx, "test_quantile_hist_budget", (long long)QT_HIST_BUDGET));
    const u32 rounds = (u32)chgpu_opt(ctx, "tune_quantile_hist_rounds", QT_HIST_ROUNDS);
    u64 * prefix = nullptr;
    u64 * rank = nullptr;
    u32 * hist = nullptr;
    if (f.large)
    {
        CHGPU_TRY(tmp.alloc(f.large * n_levels * 8, (void **)&prefix));
        CHGPU_TRY(tmp.alloc(f.large * n_levels * 8, (void **)&rank));
        CHGPU_TRY(tmp.alloc(f.large * bl * 1024, (void **)&hist));
    }
    const void * seg = d->key_type >= 0 ? f.seg.p : d->v_mem.p;
    const u64 * offsets = (const u64 *)f.offsets.p;
    const u32 * counts = (const u32 *)f.counts.p;
    const QtLarge * lseg = (const QtLarge *)f.lseg.p;
    const dim3 block(QT_T);
    u32 passes = 0;
    if (f.large)
    {
        hipLaunchKernelGGL(k_qt_state_init, dim3(qt_grid(ctx, f.large * n_levels)), block, 0, ctx->stream, lseg, f.large, kind, lv, n_levels, prefix, rank);
        CHGPU_HIP(hipMemsetAsync(hist, 0, f.large * bl * 1024, ctx->stream));
        ctx->counters[6] += 2;
    }
    dispatch_width(d->width, [&](auto tag) {
        typedef decltype(tag) T;
        if (f.small)
        {
            // three workgroups' LDS fit a CU
            hipLaunchKernelGGL(k_qt_select_small<T>, dim3(chgpu_grid_for(ctx, qt_windows(f.values), 1, 3)), block, 0, ctx->stream, (const T *)seg, offsets, counts, f.groups,
                               f.values, kind, lv, n_levels, d->mode, out);
            ctx->counters[6] += 1;
        }
        if (!f.large)
            return;
        for (u32 l0 = 0; l0 < n_levels; l0 += bl)
        {
            const u32 b = n_levels - l0 < bl ? n_levels - l0 : bl;
            for (u32 byte = sizeof(T); byte-- > 0;)
            {
                hipLaunchKernelGGL(k_qt_hist<T>, dim3(chgpu_grid_for(ctx, f.units, 1, 8)), block, 0, ctx->stream, (const T *)seg, lseg, f.large, f.units, byte, l0, b,
                                   n_levels, (const u64 *)prefix, hist, rounds);
                hipLaunchKernelGGL(k_qt_narrow<T>, dim3((u32)((f.large * b * 64 + QT_T - 1) / QT_T)), block, 0, ctx->stream, lseg, f.large, byte, l0, b, n_levels, prefix,
                                   rank, hist, d->mode, out);
                ctx->counters[6] += 2;
                passes += 1;
            }
        }
    });
    CHGPU_TRY(pair_launch_ok(QT_NAMES, "select"));
    plan->groups = f.groups;
    plan->values = f.values;
    plan->small = f.small;
    plan->large = f.large;
    plan->units = f.units;
    plan->passes = passes;
    plan->levels = n_levels;
    plan->cached = cached;
    return CHGPU_OK;
}

static void qt_free_cols(chgpu_col ** cols, u32 n)
{
    for (u32 l = 0; l < n; ++l)
    {
        if (cols[l]) chgpu_col_free(cols[l]);
        cols[l] = nullptr;
    }
}

// n rows of the empty-state value in every column of `cols` (allocated here)
static int qt_empty_cols(chgpu_quantile * d, u32 n_levels, u64 n, chgpu_col ** cols)
{
    chgpu_ctx * ctx = d->ctx;
    QtOut out{};
    for (u32 l = 0; l < n_levels; ++l)
    {
        CHGPU_TRY(d->mem.col_new(d->value_type, n, &cols[l]));
        out.p[l] = cols[l]->data;
    }
    if (!n)
        return CHGPU_OK;
    const u64 empty = qt_empty_bits(d->width, d->mode);
    dispatch_width(d->width, [&](auto tag) {
        typedef decltype(tag) T;
        hipLaunchKernelGGL(k_qt_fill<T>, dim3(qt_grid(ctx, n)), dim3(QT_T), 0, ctx->stream, out, n_levels, n, (T)empty);
    });
    ctx->counters[6] += 1;
    return pair_launch_ok(QT_NAMES, "fill");
}

extern "C" int chgpu_quantile_finalize(chgpu_quantile * d, int kind, uint32_t n_levels, const double * levels, chgpu_col ** keys_out, chgpu_col ** res_cols,
                                       uint64_t * groups)
{
    CHGPU_REQUIRE(d && res_cols && groups, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    const bool keyed = d->key_type >= 0;
    CHGPU_REQUIRE(!keyed || keys_out, CHGPU_ERR_BAD_ARGUMENTS, "NULL keys_out");
    const char * msg = "";
    const int code = qt_check_levels(kind, n_levels, levels, &msg);
    CHGPU_REQUIRE(code == CHGPU_OK, code, "quantile: %s", msg);
    chgpu_ctx * ctx = d->ctx;
    ChgpuDeviceGuard guard(ctx);
    d->mem.begin_call();
    chgpu_col * res[CHGPU_QUANTILE_MAX_LEVELS] = {nullptr};
    chgpu_col * k = nullptr;
    QtPlan plan;
    plan.levels = n_levels;
    int rc = CHGPU_OK;
    u64 rows = 0;
    if (d->held == 0)
    {
        // nothing entered: no group; without key exactly one row of the empty-state value
        rows = keyed ? 0 : 1;
        rc = qt_empty_cols(d, n_levels, rows, res);
        if (rc == CHGPU_OK && keyed)
            rc = d->mem.col_new(d->key_type, 0, &k);
    }
    else
    {
        rc = qt_select(d, kind, n_levels, levels, res, &plan);
        rows = d->fin.groups;
        if (rc == CHGPU_OK && keyed)
            rc = d->mem.col_new(d->key_type, rows, &k);
        if (rc == CHGPU_OK && keyed)
        {
            pair_narrow(ctx, (const u64 *)d->fin.gkeys->data, rows, k);
            ctx->counters[6] += 1;
            rc = pair_launch_ok(QT_NAMES, "keys");
        }
    }
    if (rc != CHGPU_OK)
    {
        qt_free_cols(res, n_levels);
        if (k) chgpu_col_free(k);
        return rc;
    }
    pair_print_plan(ctx, qt_format_plan, plan);
    for (u32 l = 0; l < n_levels; ++l)
        res_cols[l] = res[l];
    if (keys_out)
        *keys_out = k;
    *groups = rows;
    return CHGPU_OK;
}

extern "C" int chgpu_quantile_for_keys(chgpu_quantile * d, int kind, uint32_t n_levels, const double * levels, const chgpu_col * keys, chgpu_col ** res_cols)
{
    CHGPU_REQUIRE(d && keys && res_cols, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_TRY(pair_check_keys(QT_NAMES, *d, keys));
    const char * msg = "";
    const int code = qt_check_levels(kind, n_levels, levels, &msg);
    CHGPU_REQUIRE(code == CHGPU_OK, code, "quantile: %s", msg);
    CHGPU_TRY(pair_check_device(QT_NAMES, *d, keys));
    chgpu_ctx * ctx = d->ctx;
    ChgpuDeviceGuard guard(ctx);
    d->mem.begin_call();
    chgpu_col * res[CHGPU_QUANTILE_MAX_LEVELS] = {nullptr};
    chgpu_col * per_group[CHGPU_QUANTILE_MAX_LEVELS] = {nullptr};
    QtPlan plan;
    plan.what = "for_keys";
    plan.levels = n_levels;
    int rc = CHGPU_OK;
    if (d->held == 0)
        rc = qt_empty_cols(d, n_levels, keys->rows, res);
    else
    {
        rc = qt_select(d, kind, n_levels, levels, per_group, &plan);
        QtOut gres{}, out{};
        for (u32 l = 0; l < n_levels && rc == CHGPU_OK; ++l)
        {
            rc = d->mem.col_new(d->value_type, keys->rows, &res[l]);
            if (rc == CHGPU_OK)
            {
                gres.p[l] = per_group[l]->data;
                out.p[l] = res[l]->data;
            }
        }
        if (rc == CHGPU_OK && keys->rows)
        {
            const QtFinal & f = d->fin;
            const u64 empty = qt_empty_bits(d->width, d->mode);
            dispatch_width(d->width, [&](auto tag) {
                typedef decltype(tag) T;
                hipLaunchKernelGGL(k_qt_gather<T>, dim3(qt_grid(ctx, keys->rows)), dim3(QT_T), 0, ctx->stream, (const u64 *)f.gkeys->data, (const u32 *)f.cells.p,
                                   f.cells_cap, (const void *)keys->data, (u32)chgpu_type_size(d->key_type), keys->rows, gres, out, n_levels, (T)empty);
            });
            ctx->counters[6] += 1;
            rc = pair_launch_ok(QT_NAMES, "for_keys");
        }
        qt_free_cols(per_group, n_levels); // (reuse of the memory is ordered behind the gather on the stream)
    }
    if (rc != CHGPU_OK)
    {
        qt_free_cols(res, n_levels);
        return rc;
    }
    pair_print_plan(ctx, qt_format_plan, plan);
    for (u32 l = 0; l < n_levels; ++l)
        res_cols[l] = res[l];
    return CHGPU_OK;
}
