// window_kernels.hip — window functions over a sorted block (chgpu_window_*): WindowTransform's partitions, peer groups and frames
// (src/Processors/Transforms/WindowTransform.cpp, src/Interpreters/WindowDescription.h) as streaming scans plus one gather per row.
//
// Every device-wide scan here is reduce-then-scan in SEPARATE launches, the shape of scan.hip: per-tile partials -> one workgroup over
// the partials -> per-tile apply.  No kernel waits for another workgroup (a CU's L1 and the per-XCD L2s are not coherent between
// workgroups of one launch), there is no decoupled look-back and no atomic: only shuffles and LDS inside a workgroup.
//
//   create     k_win_heads          keys -> one flag byte per row (bit 0 partition head, bit 1 peer head) + six partials per tile
//              k_win_scan_partials  one workgroup per kind of partial: the partials -> the carry every tile starts from, and the two totals
//   bounds     k_win_bound<MODE>    flags + carry -> ps / gs (forward max of head ? i : 0), pe / ge (backward min of the next head, or
//                                   rows), dense (forward count of peer heads); u32 per row, built on first use and kept in the handle
//   sum / avg  k_win_tile_sums, k_win_scan_tile_sums, k_win_prefix_apply: P[0 .. rows], the exclusive wrap-around prefix sum of the
//              widened argument; a frame's sum is P[fe] - P[fs], so partitions need no segmented add
//   min / max  k_win_seg_tiles, k_win_scan_seg_tiles, k_win_seg_apply<BACK>: the running extremum of agg_order_key(x) (min: its
//              complement) since the partition's first row -- or, backward, up to its last row
//   output     k_win_out_rank (row_number / rank / dense_rank / count), k_win_out_sum (sum / avg), k_win_out_extremum (min / max),
//              k_win_out_pick<W> (first_value / last_value / lagInFrame / leadInFrame): row i, its bounds, the scan array -> the result;
//              what they share around their rows is win_out_rows, and the frame itself is win_frame_of (window_host.h), the code the
//              host driver tests
//   framed     what chgpu_window_evaluate_framed alone serves (window_frames_host.h): k_win_range_bound<X> searches the ORDER BY column
//              for the bounds of a RANGE frame with offsets into a call's own fs[] / fe[], which every output kernel reads through
//              win_row_frame; k_win_ext_masks (a monotone-stack mask per row of a 64-row block), k_win_ext_level (one level of the sparse
//              table over the blocks' extrema per launch) and k_win_out_extremum_any<W> are min / max over any frame
// Both entries are win_evaluate: win_check_frame and win_plan (window_host.h) in one order of checks, then win_run, which launches what
// the plan says.  The handle's pool memory and a call's temporaries are pair_pool.h (PairMem, PairAllocs without a refusal hook, PairTemps).
#include "block_scan.h"
#include "pair_pool.h"
#include "window_frames_host.h"
#include "window_host.h"

static constexpr u32 WIN_INF = 0xFFFFFFFFu;

// ---------------------------------------------------------------------------------------------
// the scans inside a workgroup are block_scan.h's; the one Op of this file's own:
// ---------------------------------------------------------------------------------------------
// a running maximum that starts again at every element whose flag is set: (a then b) = b where b starts a segment, else the larger
struct WinSeg { u64 v; u32 f; };
struct WinSegMax
{
    typedef WinSeg T;
    static __device__ __forceinline__ T id() { return WinSeg{0, 0}; }
    static __device__ __forceinline__ T comb(T a, T b) { return WinSeg{b.f ? b.v : (a.v > b.v ? a.v : b.v), a.f | b.f}; }
};

__device__ __forceinline__ WinSeg shfl_up(WinSeg v, int d) { return WinSeg{shfl_up(v.v, d), shfl_up(v.f, d)}; }

// ---------------------------------------------------------------------------------------------
// heads
// ---------------------------------------------------------------------------------------------
struct WinKeys
{
    const void * p[2 * WIN_MAX_KEYS];
    u8 width[2 * WIN_MAX_KEYS];
    u8 is_float[2 * WIN_MAX_KEYS];
    u32 n_part, n_all; // the partition columns first, then the order columns
};

// compareAt == 0 of rows i and i - 1 of one key column: integers by value, floats with a == b or both NaN
__device__ __forceinline__ bool win_key_equal(const void * p, u32 width, bool is_float, u64 i)
{
    switch (width)
    {
        case 8:
        {
            const u64 a = ((const u64 *)p)[i], b = ((const u64 *)p)[i - 1];
            if (!is_float)
                return a == b;
            const double x = __longlong_as_double((long long)a), y = __longlong_as_double((long long)b);
            return x == y || (x != x && y != y);
        }
        case 4:
        {
            const u32 a = ((const u32 *)p)[i], b = ((const u32 *)p)[i - 1];
            if (!is_float)
                return a == b;
            const float x = __uint_as_float(a), y = __uint_as_float(b);
            return x == y || (x != x && y != y);
        }
        case 2: return ((const u16 *)p)[i] == ((const u16 *)p)[i - 1];
        default: return ((const u8 *)p)[i] == ((const u8 *)p)[i - 1];
    }
}

// the six partials of a tile, part[k * n_tiles + tile]
enum { WIN_P_LAST_P = 0, WIN_P_LAST_G, WIN_P_FIRST_P, WIN_P_FIRST_G, WIN_P_COUNT_P, WIN_P_COUNT_G, WIN_P_KINDS };

// One workgroup per tile.  flags is whole tiles long: the rows past `n` of the last tile get 0.
__global__ __launch_bounds__(WIN_THREADS) void k_win_heads(WinKeys keys, u64 n, u64 n_tiles, u8 * __restrict__ flags, u32 * __restrict__ part)
{
    __shared__ __attribute__((aligned(8))) u8 s_flags[WIN_TILE];
    __shared__ u32 red[WIN_P_KINDS][WIN_THREADS / 64];
    const u64 tile0 = (u64)blockIdx.x * WIN_TILE;
    u32 last_p = 0, last_g = 0, first_p = WIN_INF, first_g = WIN_INF, count_p = 0, count_g = 0;
#pragma unroll
    for (u32 k = 0; k < WIN_ITEMS; ++k)
    {
        const u64 i = tile0 + k * WIN_THREADS + threadIdx.x;
        u32 f = 0;
        if (i < n)
        {
            if (i == 0)
                f = 3;
            else
                // the partition columns first, stopping at the first difference: a row that starts a partition reads no order column
                // (comparing every column unconditionally was measured: no faster at few partitions, 0.43 -> 0.73 ms at 1e8 of 1e8 rows)
                for (u32 c = 0; c < keys.n_all; ++c)
                    if (!win_key_equal(keys.p[c], keys.width[c], keys.is_float[c] != 0, i))
                    {
                        f = c < keys.n_part ? 3 : 2;
                        break;
                    }
            if (f & 1)
            {
                last_p = (u32)i; // (i grows with k)
                first_p = first_p == WIN_INF ? (u32)i : first_p;
                count_p += 1;
            }
            if (f & 2)
            {
                last_g = (u32)i;
                first_g = first_g == WIN_INF ? (u32)i : first_g;
                count_g += 1;
            }
        }
        s_flags[k * WIN_THREADS + threadIdx.x] = (u8)f;
    }
    last_p = wave_reduce_all<MaxU32>(last_p);
    last_g = wave_reduce_all<MaxU32>(last_g);
    first_p = wave_reduce_all<MinU32>(first_p);
    first_g = wave_reduce_all<MinU32>(first_g);
    count_p = wave_reduce_all<AddU32>(count_p);
    count_g = wave_reduce_all<AddU32>(count_g);
    if ((threadIdx.x & 63) == 0)
    {
        const u32 wave = threadIdx.x >> 6;
        red[WIN_P_LAST_P][wave] = last_p;
        red[WIN_P_LAST_G][wave] = last_g;
        red[WIN_P_FIRST_P][wave] = first_p;
        red[WIN_P_FIRST_G][wave] = first_g;
        red[WIN_P_COUNT_P][wave] = count_p;
        red[WIN_P_COUNT_G][wave] = count_g;
    }
    __syncthreads(); // (one barrier for the flags and the six partials)
    ((u64 *)(flags + tile0))[threadIdx.x] = ((const u64 *)s_flags)[threadIdx.x];
    if (threadIdx.x < WIN_P_KINDS)
    {
        const u32 k = threadIdx.x;
        u32 r = red[k][0];
        for (u32 w = 1; w < WIN_THREADS / 64; ++w)
            r = k <= WIN_P_LAST_G ? MaxU32::comb(r, red[k][w]) : k <= WIN_P_FIRST_G ? MinU32::comb(r, red[k][w]) : r + red[k][w];
        part[k * n_tiles + blockIdx.x] = r;
    }
}

// One workgroup per kind of partial (six independent scans, no workgroup reads what another writes), in place: a tile's partial becomes
// what the tile starts from -- the last head before it (0: row 0 is one), the first head after it (or rows), the heads counted before
// it.  totals[0 / 1]: partitions, peer groups.
__global__ __launch_bounds__(WIN_PASS) void k_win_scan_partials(u32 * __restrict__ part, u64 n_tiles, u32 rows, u32 * __restrict__ totals)
{
    const u32 kind = blockIdx.x;
    u32 * a = part + kind * n_tiles;
    if (kind <= WIN_P_LAST_G)
        block_scan_array<MaxU32, false>(a, a, n_tiles, 0);
    else if (kind <= WIN_P_FIRST_G)
        block_scan_array<MinU32, true>(a, a, n_tiles, rows);
    else
    {
        const u32 total = block_scan_array<AddU32, false>(a, a, n_tiles, 0);
        if (threadIdx.x == 0)
            totals[kind - WIN_P_COUNT_P] = total;
    }
}

// ---------------------------------------------------------------------------------------------
// bounds: one workgroup per tile, a thread owns eight consecutive rows (one 8-byte load of flags, two 16-byte stores of bounds)
// ---------------------------------------------------------------------------------------------
enum { WIN_M_FWD_MAX = 0, WIN_M_BWD_MIN = 1, WIN_M_FWD_COUNT = 2 };

template <int MODE>
__global__ __launch_bounds__(WIN_THREADS) void k_win_bound(const u8 * __restrict__ flags, u32 bit, const u32 * __restrict__ carry, u32 * __restrict__ out)
{
    typedef typename std::conditional<MODE == WIN_M_FWD_MAX, MaxU32, typename std::conditional<MODE == WIN_M_BWD_MIN, MinU32, AddU32>::type>::type Op;
    __shared__ u32 lds[16];
    const u64 tile0 = (u64)blockIdx.x * WIN_TILE;
    // backward: thread 0 owns the LAST eight rows of the tile, so that the scan in thread order runs from the far end
    const u32 slot = MODE == WIN_M_BWD_MIN ? WIN_THREADS - 1 - threadIdx.x : threadIdx.x;
    const u64 r0 = tile0 + (u64)slot * WIN_ITEMS;
    const u64 f8 = *(const u64 *)(flags + r0);
    u32 v[WIN_ITEMS];
    u32 mine = Op::id();
#pragma unroll
    for (u32 k = 0; k < WIN_ITEMS; ++k)
    {
        const bool head = (f8 >> (8 * k)) & bit;
        v[k] = MODE == WIN_M_FWD_COUNT ? (head ? 1u : 0u) : head ? (u32)(r0 + k) : Op::id();
        mine = Op::comb(mine, v[k]);
    }
    u32 run = Op::comb(carry[blockIdx.x], block_scan_exclusive<Op>(mine, lds));
    u32 o[WIN_ITEMS];
    if (MODE == WIN_M_BWD_MIN)
    {
#pragma unroll
        for (int k = WIN_ITEMS - 1; k >= 0; --k)
        {
            o[k] = run; // the first head AFTER this row
            run = Op::comb(run, v[k]);
        }
    }
    else
    {
#pragma unroll
        for (u32 k = 0; k < WIN_ITEMS; ++k)
        {
            run = Op::comb(run, v[k]);
            o[k] = run;
        }
    }
    uint4 * dst = (uint4 *)(out + r0);
    dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
    dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
}

// ---------------------------------------------------------------------------------------------
// value scans
// ---------------------------------------------------------------------------------------------
// the argument widened to 64 bits: integers sign- / zero-extended, Float32 after its exact widening (as the aggregates load it)
__device__ __forceinline__ u64 win_load_bits(const void * p, int type, u64 i)
{
    switch (type)
    {
        case CHGPU_I64: case CHGPU_U64: case CHGPU_F64: return ((const u64 *)p)[i];
        case CHGPU_U32: return ((const u32 *)p)[i];
        case CHGPU_I32: return (u64)(i64)((const i32 *)p)[i];
        case CHGPU_U16: return ((const u16 *)p)[i];
        case CHGPU_I16: return (u64)(i64)((const i16 *)p)[i];
        case CHGPU_U8: return ((const u8 *)p)[i];
        case CHGPU_I8: return (u64)(i64)((const i8 *)p)[i];
        case CHGPU_F32: return (u64)__double_as_longlong((double)((const float *)p)[i]);
        default: return 0;
    }
}

__global__ __launch_bounds__(WIN_THREADS) void k_win_tile_sums(const void * __restrict__ x, int type, u64 n, u64 * __restrict__ tile_sums)
{
    __shared__ u64 lds[16];
    const u64 tile0 = (u64)blockIdx.x * WIN_TILE;
    u64 s = 0;
#pragma unroll
    for (u32 k = 0; k < WIN_ITEMS; ++k)
    {
        const u64 i = tile0 + k * WIN_THREADS + threadIdx.x;
        if (i < n)
            s += win_load_bits(x, type, i);
    }
    const u64 total = block_reduce<AddU64>(s, lds);
    if (threadIdx.x == 0)
        tile_sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(WIN_PASS) void k_win_scan_tile_sums(u64 * __restrict__ tile_sums, u64 n_tiles)
{
    block_scan_array<AddU64, false>(tile_sums, tile_sums, n_tiles, 0);
}

// P[0] = 0, P[i + 1] = x[0] + .. + x[i] (wrap-around).  The tile goes through LDS both ways, so that memory sees consecutive addresses
// and only LDS sees the thread-owns-eight-consecutive-rows pattern.
__global__ __launch_bounds__(WIN_THREADS) void k_win_prefix_apply(const void * __restrict__ x, int type, u64 n, const u64 * __restrict__ tile_off, u64 * __restrict__ P)
{
    __shared__ u64 s[WIN_TILE];
    __shared__ u64 lds[16];
    const u64 tile0 = (u64)blockIdx.x * WIN_TILE;
#pragma unroll
    for (u32 k = 0; k < WIN_ITEMS; ++k)
    {
        const u32 j = k * WIN_THREADS + threadIdx.x;
        s[j] = tile0 + j < n ? win_load_bits(x, type, tile0 + j) : 0;
    }
    __syncthreads();
    u64 v[WIN_ITEMS];
    u64 mine = 0;
#pragma unroll
    for (u32 k = 0; k < WIN_ITEMS; ++k)
    {
        v[k] = s[threadIdx.x * WIN_ITEMS + k];
        mine += v[k];
    }
    u64 run = tile_off[blockIdx.x] + block_scan_exclusive<AddU64>(mine, lds);
#pragma unroll
    for (u32 k = 0; k < WIN_ITEMS; ++k)
    {
        run += v[k];
        s[threadIdx.x * WIN_ITEMS + k] = run;
    }
    __syncthreads();
#pragma unroll
    for (u32 k = 0; k < WIN_ITEMS; ++k)
    {
        const u32 j = k * WIN_THREADS + threadIdx.x;
        if (tile0 + j < n)
            P[tile0 + j + 1] = s[j];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        P[0] = 0;
}

// The running extremum works on positions q = 0 .. n - 1 in scan order: forward q is the row, backward q is the row counted from the far
// end.  seg(q) is the position at which q's partition starts in that order: ps[row], or n - pe[row].
template <bool BACK>
__device__ __forceinline__ u64 win_row_of(u64 q, u64 n) { return BACK ? n - 1 - q : q; }
template <bool BACK>
__device__ __forceinline__ u64 win_seg_of(const u32 * __restrict__ bound, u64 q, u64 n) { return BACK ? n - bound[n - 1 - q] : bound[q]; }
__device__ __forceinline__ u64 win_ext_key(const void * x, int type, bool is_min, u64 row)
{
    const u64 k = agg_order_key(win_load_bits(x, type, row), type);
    return is_min ? ~k : k;
}

// a tile's aggregate: the extremum of its positions that lie in the partition of its last position, and whether that partition starts
// inside the tile
template <bool BACK>
__global__ __launch_bounds__(WIN_THREADS) void k_win_seg_tiles(const void * __restrict__ x, int type, int is_min, const u32 * __restrict__ bound, u64 n, WinSeg * __restrict__ agg)
{
    __shared__ u64 lds[4];
    const u64 tile0 = (u64)blockIdx.x * WIN_TILE;
    const u64 last = tile0 + WIN_TILE <= n ? tile0 + WIN_TILE - 1 : n - 1;
    const u64 start = win_seg_of<BACK>(bound, last, n);
    u64 m = 0;
#pragma unroll
    for (u32 k = 0; k < WIN_ITEMS; ++k)
    {
        const u64 q = tile0 + k * WIN_THREADS + threadIdx.x;
        if (q <= last && q >= start)
        {
            const u64 key = win_ext_key(x, type, is_min != 0, win_row_of<BACK>(q, n));
            m = key > m ? key : m;
        }
    }
    m = block_reduce<MaxU64>(m, lds);
    if (threadIdx.x == 0)
        agg[blockIdx.x] = WinSeg{m, start >= tile0 ? 1u : 0u};
}

__global__ __launch_bounds__(WIN_PASS) void k_win_scan_seg_tiles(WinSeg * __restrict__ agg, u64 n_tiles)
{
    block_scan_array<WinSegMax, false>(agg, agg, n_tiles, WinSeg{0, 0});
}

// M[row] = the extremum key over the row's partition up to and including the row, in scan order
template <bool BACK>
__global__ __launch_bounds__(WIN_THREADS) void k_win_seg_apply(const void * __restrict__ x, int type, int is_min, const u32 * __restrict__ bound, u64 n,
                                                               const WinSeg * __restrict__ carry, u64 * __restrict__ M)
{
    __shared__ u64 s[WIN_TILE];
    __shared__ u8 s_head[WIN_TILE];
    __shared__ WinSeg lds[16];
    const u64 tile0 = (u64)blockIdx.x * WIN_TILE;
#pragma unroll
    for (u32 k = 0; k < WIN_ITEMS; ++k)
    {
        const u32 j = k * WIN_THREADS + threadIdx.x;
        const u64 q = tile0 + j;
        const bool in = q < n;
        s[j] = in ? win_ext_key(x, type, is_min != 0, win_row_of<BACK>(q, n)) : 0;
        s_head[j] = in ? (win_seg_of<BACK>(bound, q, n) == q ? 1 : 0) : 1;
    }
    __syncthreads();
    WinSeg v[WIN_ITEMS];
    WinSeg mine = WinSegMax::id();
#pragma unroll
    for (u32 k = 0; k < WIN_ITEMS; ++k)
    {
        v[k] = WinSeg{s[threadIdx.x * WIN_ITEMS + k], s_head[threadIdx.x * WIN_ITEMS + k]};
        mine = WinSegMax::comb(mine, v[k]);
    }
    WinSeg run = WinSegMax::comb(WinSeg{carry[blockIdx.x].v, 0}, block_scan_exclusive<WinSegMax>(mine, lds));
#pragma unroll
    for (u32 k = 0; k < WIN_ITEMS; ++k)
    {
        run = WinSegMax::comb(run, v[k]);
        s[threadIdx.x * WIN_ITEMS + k] = run.v;
    }
    __syncthreads();
#pragma unroll
    for (u32 k = 0; k < WIN_ITEMS; ++k)
    {
        const u32 j = k * WIN_THREADS + threadIdx.x;
        if (tile0 + j < n)
            M[win_row_of<BACK>(tile0 + j, n)] = s[j];
    }
}

// ---------------------------------------------------------------------------------------------
// output: a thread owns four consecutive rows, so a u32 bound array is read 16 bytes at a time (the arrays are whole tiles long) and a
// result of four 8-byte values leaves in two 16-byte stores.  The gathers (P[fe], x[t], M[fe - 1]) are one element each.
// ---------------------------------------------------------------------------------------------
struct WinBounds
{
    const u32 * ps;
    const u32 * pe;
    const u32 * gs;
    const u32 * ge;
    const u32 * dense;
    const u32 * fs; // a call's own per-row frame begins / ends (the search behind a RANGE offset); NULL: the bound comes from win_frame_of
    const u32 * fe;
};

struct WinRow4
{
    u32 ps[4], pe[4], gs[4], ge[4], dense[4], fs[4], fe[4];
};

__device__ __forceinline__ void win_load4(const u32 * __restrict__ p, u64 i0, u32 out[4])
{
    if (!p)
    {
        out[0] = out[1] = out[2] = out[3] = 0;
        return;
    }
    const uint4 v = *(const uint4 *)(p + i0);
    out[0] = v.x, out[1] = v.y, out[2] = v.z, out[3] = v.w;
}

__device__ __forceinline__ void win_load_bounds(const WinBounds & b, u64 i0, WinRow4 * r)
{
    win_load4(b.ps, i0, r->ps);
    win_load4(b.pe, i0, r->pe);
    win_load4(b.gs, i0, r->gs);
    win_load4(b.ge, i0, r->ge);
    win_load4(b.dense, i0, r->dense); // (given to dense_rank alone)
    win_load4(b.fs, i0, r->fs);
    win_load4(b.fe, i0, r->fe);
}

// the frame of row i, the k-th of the thread's four: win_frame_of, with the bounds that were searched taken from their arrays
__device__ __forceinline__ void win_row_frame(const chgpu_window_frame & frame, const WinBounds & b, const WinRow4 & r, u32 k, u64 i, u64 * fs, u64 * fe)
{
    win_frame_of(frame, i, r.ps[k], r.pe[k], r.gs[k], r.ge[k], fs, fe);
    if (b.fs)
        *fs = r.fs[k];
    if (b.fe)
        *fe = r.fe[k];
}

// four values of W bytes to out[i0 .. i0 + 4): one access where all four rows exist, else row by row
template <typename W>
__device__ __forceinline__ void win_store4(W * __restrict__ out, u64 i0, u64 n, const u64 v[4])
{
    if (i0 + 4 <= n)
    {
        if constexpr (sizeof(W) == 8)
        {
            typedef u64 v2u64 __attribute__((ext_vector_type(2)));
            v2u64 a, b;
            a.x = v[0], a.y = v[1], b.x = v[2], b.y = v[3];
            ((v2u64 *)(out + i0))[0] = a;
            ((v2u64 *)(out + i0))[1] = b;
        }
        else if constexpr (sizeof(W) == 4)
            *(uint4 *)(out + i0) = make_uint4((u32)v[0], (u32)v[1], (u32)v[2], (u32)v[3]);
        else if constexpr (sizeof(W) == 2)
            *(uint2 *)(out + i0) = make_uint2((u32)(u16)v[0] | ((u32)(u16)v[1] << 16), (u32)(u16)v[2] | ((u32)(u16)v[3] << 16));
        else
            *(u32 *)(out + i0) = (u32)(u8)v[0] | ((u32)(u8)v[1] << 8) | ((u32)(u8)v[2] << 16) | ((u32)(u8)v[3] << 24);
        return;
    }
    for (u32 k = 0; k < 4 && i0 + k < n; ++k)
        out[i0 + k] = (W)v[k];
}

__device__ __forceinline__ u64 win_first_row() { return ((u64)blockIdx.x * WIN_THREADS + threadIdx.x) * WIN_OUT_ROWS; }

// What every output kernel does around its rows: the thread's four rows, their bounds in one load per array, body(i, k, r) -> the 64
// result bits of row i, the k-th of the four (rows past the input are skipped), and the store.  The body asks win_row_frame for the
// row's frame where it reads one.  The bodies capture by value: what they capture are kernel arguments, the same in every lane, and a
// copy leaves them in scalar registers where a reference made the compiler test `frame` again for every row.
template <typename W, typename Body>
__device__ __forceinline__ void win_out_rows(const WinBounds & b, u64 n, W * __restrict__ out, Body && body)
{
    const u64 i0 = win_first_row();
    if (i0 >= n)
        return;
    WinRow4 r;
    win_load_bounds(b, i0, &r);
    u64 v[4];
#pragma unroll
    for (u32 k = 0; k < 4; ++k)
    {
        const u64 i = i0 + k;
        v[k] = 0;
        if (i < n)
            v[k] = body(i, k, r);
    }
    win_store4(out, i0, n, v);
}

__global__ __launch_bounds__(WIN_THREADS) void k_win_out_rank(int function, chgpu_window_frame frame, WinBounds b, u64 n, u64 * __restrict__ out)
{
    win_out_rows(b, n, out, [=](u64 i, u32 k, const WinRow4 & r) -> u64 {
        if (function == CHGPU_WIN_ROW_NUMBER)
            return i - r.ps[k] + 1;
        if (function == CHGPU_WIN_RANK)
            return (u64)r.gs[k] - r.ps[k] + 1;
        if (function == CHGPU_WIN_DENSE_RANK)
            return (u64)r.dense[k] - b.dense[r.ps[k]] + 1; // (the partition's first row is a peer head itself)
        u64 fs, fe;
        win_row_frame(frame, b, r, k, i, &fs, &fe);
        return fe - fs;
    });
}

// sum: P[fe] - P[fs]; avg: that as Float64 (signed: num_signed) over Float64(fe - fs), AvgFraction::divide as k_avg_divide has it
__global__ __launch_bounds__(WIN_THREADS) void k_win_out_sum(int is_avg, int num_signed, chgpu_window_frame frame, WinBounds b, u64 n, const u64 * __restrict__ P,
                                                             u64 * __restrict__ out)
{
    win_out_rows(b, n, out, [=](u64 i, u32 k, const WinRow4 & r) -> u64 {
        u64 fs, fe;
        win_row_frame(frame, b, r, k, i, &fs, &fe);
        const u64 sum = P[fe] - P[fs];
        if (!is_avg)
            return sum;
        const double num = num_signed ? (double)(i64)sum : (double)sum;
        return (u64)__double_as_longlong(num / (double)(fe - fs));
    });
}

// an extremum's key back to the value's bits: agg_order_key's inverse (min: of the complement), Float32 narrowed from its exact widening
__device__ __forceinline__ u64 win_ext_value_bits(u64 key, int type, int is_min)
{
    const u64 bits = agg_order_key_inverse(is_min ? ~key : key, type);
    return type == CHGPU_F32 ? (u64)__float_as_uint((float)__longlong_as_double((long long)bits)) : bits;
}

// min / max: forward the answer stands at the frame's last row, backward at its first; the key goes back to the value's bits
template <typename W>
__global__ __launch_bounds__(WIN_THREADS) void k_win_out_extremum(int type, int is_min, int backward, chgpu_window_frame frame, WinBounds b, u64 n,
                                                                  const u64 * __restrict__ M, W * __restrict__ out)
{
    win_out_rows(b, n, out, [=](u64 i, u32 k, const WinRow4 & r) -> u64 {
        u64 fs, fe;
        win_row_frame(frame, b, r, k, i, &fs, &fe);
        return fs < fe ? win_ext_value_bits(M[backward ? fs : fe - 1], type, is_min) : 0;
    });
}

enum { WIN_PICK_FIRST = 0, WIN_PICK_LAST, WIN_PICK_LAG, WIN_PICK_LEAD };

// first_value / last_value / lagInFrame / leadInFrame: one element of x moved with its bits untouched
template <typename W>
__global__ __launch_bounds__(WIN_THREADS) void k_win_out_pick(int pick, chgpu_window_frame frame, WinBounds b, u64 n, const W * __restrict__ x, u64 offset, u64 default_bits,
                                                              W * __restrict__ out)
{
    win_out_rows(b, n, out, [=](u64 i, u32 k, const WinRow4 & r) -> u64 {
        u64 fs, fe, t, v;
        win_row_frame(frame, b, r, k, i, &fs, &fe);
        if (pick == WIN_PICK_FIRST || pick == WIN_PICK_LAST)
            v = fs < fe ? (u64)x[pick == WIN_PICK_FIRST ? fs : fe - 1] : 0;
        else
            v = win_shifted_row(pick == WIN_PICK_LEAD, i, offset, fs, fe, &t) ? (u64)x[t] : (u64)(W)default_bits;
        return v;
    });
}

// ---------------------------------------------------------------------------------------------
// frames of the framed entry (chgpu_window_evaluate_framed): the search behind a RANGE offset, and min / max over any frame
// ---------------------------------------------------------------------------------------------
// one searched bound: `k PRECEDING` or `k FOLLOWING` (k > 0) into out[]; out == NULL: the bound is not searched
struct WinRangeSide
{
    u32 * out;
    u64 k;
    int following;
};

// A thread per row: win_range_bound_of (window_frames_host.h) from the row's own position towards the partition edge the bound names.
// Neighbouring lanes start at neighbouring rows and gallop in step, so a wave's loads fall into the same few lines.
template <typename X>
__global__ __launch_bounds__(WIN_THREADS) void k_win_range_bound(const X * __restrict__ x, int descending, const u32 * __restrict__ ps, const u32 * __restrict__ pe, u64 n,
                                                                 WinRangeSide begin, WinRangeSide end)
{
    const u64 i = (u64)blockIdx.x * WIN_THREADS + threadIdx.x;
    if (i >= n)
        return;
    if (begin.out)
        begin.out[i] = (u32)win_range_bound_of(x, i, begin.following ? 0 : (u64)ps[i], begin.following ? (u64)pe[i] : 0, begin.following != 0, false, descending != 0, begin.k);
    if (end.out)
        end.out[i] = (u32)win_range_bound_of(x, i, end.following ? 0 : (u64)ps[i], end.following ? (u64)pe[i] : 0, end.following != 0, true, descending != 0, end.k);
}

// One wave per block of 64 rows, a lane per row.  mask[r] bit p: no row q in (p, r] of the block has key[q] >= key[p].  For every p the
// wave broadcasts key[p] and ballots key >= key[p]; the lowest such row above p ends the run of rows whose mask holds p.  Rows past the
// input hold the worst key, 0; they lie above every row of the input, so no mask of a row of the input sees them.  top[block]: the
// block's extremum key, level 0 of the table.
__global__ __launch_bounds__(WIN_THREADS) void k_win_ext_masks(const void * __restrict__ x, int type, int is_min, u64 n, u64 n_blocks, u64 * __restrict__ mask,
                                                               u64 * __restrict__ top)
{
    const u32 lane = threadIdx.x & 63;
    const u64 block = (u64)blockIdx.x * (WIN_THREADS / 64) + (threadIdx.x >> 6);
    if (block >= n_blocks) // (whole waves leave: no barrier below)
        return;
    const u64 row = block * WIN_EXT_BLOCK + lane;
    const u64 key = row < n ? win_ext_key(x, type, is_min != 0, row) : 0;
    u64 m = 0;
#pragma unroll // (all 64: p is a constant in every copy, so a copy touches one half of m and compares the lane with constants)
    for (u32 p = 0; p < 64; ++p)
    {
        const u64 kp = ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(key >> 32), (int)p) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)key, (int)p);
        const u64 ge = __ballot(key >= kp) & ~(((u64)2 << p) - 1); // the rows above p that end it (p = 63: 2 << 63 wraps to 0, none)
        const u32 held = (ge ? (u32)__builtin_ctzll(ge) : 64) - p; // the rows p .. p + held - 1 hold bit p
        if (lane - p < held)                                       // (unsigned: a lane below p wraps past every `held`)
            m |= (u64)1 << p;
    }
    mask[row] = m; // (the mask array is whole blocks long)
    const u64 best = wave_reduce_all<MaxU64>(key);
    if (lane == 0)
        top[block] = best;
}

// one level of the sparse table from the level below: cur[b] = max(prev[b], prev[b + half]), where both cells exist
__global__ __launch_bounds__(WIN_THREADS) void k_win_ext_level(const u64 * __restrict__ prev, u64 * __restrict__ cur, u64 n_blocks, u64 half)
{
    const u64 b = (u64)blockIdx.x * WIN_THREADS + threadIdx.x;
    if (b >= n_blocks)
        return;
    const u64 a = prev[b];
    cur[b] = b + half < n_blocks ? MaxU64::comb(a, prev[b + half]) : a;
}

// min / max over [fs, fe): inside one block the mask of the last row answers; over several blocks the first block's suffix (the mask of
// its last row), the last block's prefix (the mask of the frame's last row) and two cells of the table for the blocks between
template <typename W>
__global__ __launch_bounds__(WIN_THREADS) void k_win_out_extremum_any(int type, int is_min, chgpu_window_frame frame, WinBounds b, u64 n, const void * __restrict__ x,
                                                                      const u64 * __restrict__ mask, const u64 * __restrict__ table, u64 n_blocks, W * __restrict__ out)
{
    win_out_rows(b, n, out, [=](u64 i, u32 k, const WinRow4 & r) -> u64 {
        u64 fs, fe;
        win_row_frame(frame, b, r, k, i, &fs, &fe);
        if (fs >= fe)
            return 0;
        const u64 l = fs, last = fe - 1, bl = l / WIN_EXT_BLOCK, br = last / WIN_EXT_BLOCK;
        u64 key;
        if (bl == br)
            key = win_ext_key(x, type, is_min != 0, win_ext_in_block(mask[last], l));
        else
        {
            const u64 k0 = win_ext_key(x, type, is_min != 0, win_ext_in_block(mask[bl * WIN_EXT_BLOCK + WIN_EXT_BLOCK - 1], l));
            const u64 k1 = win_ext_key(x, type, is_min != 0, win_ext_in_block(mask[last], br * WIN_EXT_BLOCK));
            key = MaxU64::comb(k0, k1);
            if (br - bl > 1)
            {
                u32 level;
                u64 c0, c1;
                win_ext_cells(bl, br, &level, &c0, &c1);
                key = MaxU64::comb(key, MaxU64::comb(table[level * n_blocks + c0], table[level * n_blocks + c1]));
            }
        }
        return win_ext_value_bits(key, type, is_min);
    });
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
struct chgpu_window
{
    chgpu_ctx * ctx = nullptr;
    u64 rows = 0, n_tiles = 0;
    PairMem flags;     // u8[padded rows]
    PairMem part;      // u32[WIN_P_KINDS * n_tiles], scanned, then u32 totals[2]
    PairMem bounds[5]; // u32[padded rows] each: ps, pe, gs, ge, dense; built on first use
    WinLazy lazy;
    bool have_totals = false;
    u64 partitions = 0, peer_groups = 0;
    u32 n_order = 0;     // ORDER BY columns given to create, and the type of the first (-1: none): what a RANGE offset checks its
    int order_type = -1; // order column against
    PairAllocs mem; // (pair_pool.h; no refusal hook here)
};

static u32 * win_totals(const chgpu_window * w) { return (u32 *)w->part.p + WIN_P_KINDS * w->n_tiles; }

static int win_add_keys(chgpu_ctx * ctx, const chgpu_col * const * cols, u32 n, u64 rows, const char * what, WinKeys * keys)
{
    CHGPU_REQUIRE(n <= WIN_MAX_KEYS, CHGPU_ERR_BAD_ARGUMENTS, "window: %u %s columns, at most %u are taken", n, what, WIN_MAX_KEYS);
    CHGPU_REQUIRE(n == 0 || cols, CHGPU_ERR_BAD_ARGUMENTS, "window: NULL list of %s columns", what);
    for (u32 c = 0; c < n; ++c)
    {
        const chgpu_col * col = cols[c];
        CHGPU_REQUIRE(col, CHGPU_ERR_BAD_ARGUMENTS, "window: NULL %s column %u", what, c);
        CHGPU_REQUIRE(chgpu_type_size(col->type) != 0, CHGPU_ERR_BAD_ARGUMENTS, "window: %s column %u has an unknown type", what, c);
        CHGPU_REQUIRE(col->ctx && col->ctx->device == ctx->device, CHGPU_ERR_BAD_ARGUMENTS, "window: %s column %u lives on another device", what, c);
        CHGPU_REQUIRE(col->rows == rows, CHGPU_ERR_SIZES_MISMATCH, "window: %s column %u has %llu rows, the window %llu", what, c,
                      (unsigned long long)col->rows, (unsigned long long)rows);
        keys->p[keys->n_all] = col->data;
        keys->width[keys->n_all] = (u8)chgpu_type_size(col->type);
        keys->is_float[keys->n_all] = chgpu_type_is_float(col->type) ? 1 : 0;
        keys->n_all += 1;
    }
    return CHGPU_OK;
}

extern "C" int chgpu_window_create(chgpu_ctx * ctx, const chgpu_col * const * partition_cols, uint32_t n_partition, const chgpu_col * const * order_cols,
                                   uint32_t n_order, uint64_t rows, chgpu_window ** out)
{
    CHGPU_REQUIRE(ctx && out, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    CHGPU_REQUIRE(rows <= WIN_MAX_ROWS, CHGPU_ERR_NOT_IMPLEMENTED, "window: %llu rows, at most %llu are taken", (unsigned long long)rows,
                  (unsigned long long)WIN_MAX_ROWS);
    WinKeys keys{};
    CHGPU_TRY(win_add_keys(ctx, partition_cols, n_partition, rows, "partition", &keys));
    keys.n_part = keys.n_all;
    CHGPU_TRY(win_add_keys(ctx, order_cols, n_order, rows, "order", &keys));
    ChgpuDeviceGuard guard(ctx);
    chgpu_window * w = new chgpu_window();
    w->ctx = w->mem.ctx = ctx;
    w->rows = rows;
    w->n_tiles = win_tiles(rows);
    w->n_order = n_order;
    w->order_type = n_order ? order_cols[0]->type : -1;
    chgpu_ctx_retain(ctx);
    if (rows)
    {
        int rc = w->mem.alloc(win_padded_rows(rows), &w->flags);
        if (rc == CHGPU_OK)
            rc = w->mem.alloc((WIN_P_KINDS * w->n_tiles + 2) * sizeof(u32), &w->part);
        if (rc != CHGPU_OK)
        {
            chgpu_window_free(w);
            return rc;
        }
        hipLaunchKernelGGL(k_win_heads, dim3((u32)w->n_tiles), dim3(WIN_THREADS), 0, ctx->stream, keys, rows, w->n_tiles, (u8 *)w->flags.p, (u32 *)w->part.p);
        hipLaunchKernelGGL(k_win_scan_partials, dim3(WIN_P_KINDS), dim3(WIN_PASS), 0, ctx->stream, (u32 *)w->part.p, w->n_tiles, (u32)rows, win_totals(w));
        ctx->counters[6] += 2;
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
        {
            chgpu_window_free(w);
            return chgpu_set_error(CHGPU_ERR_DEVICE, "window: launching the head kernels failed: %s", hipGetErrorString(e));
        }
    }
    *out = w;
    return CHGPU_OK;
}

extern "C" int chgpu_window_free(chgpu_window * w)
{
    if (!w)
        return CHGPU_OK;
    ChgpuDeviceGuard guard(w->ctx);
    pair_free_mem(w->ctx, w->flags);
    pair_free_mem(w->ctx, w->part);
    for (PairMem & m : w->bounds)
        pair_free_mem(w->ctx, m);
    chgpu_ctx * ctx = w->ctx;
    delete w;
    chgpu_ctx_release(ctx);
    return CHGPU_OK;
}

extern "C" int chgpu_window_counts(chgpu_window * w, uint64_t * rows, uint64_t * partitions, uint64_t * peer_groups)
{
    CHGPU_REQUIRE(w, CHGPU_ERR_BAD_ARGUMENTS, "NULL window");
    ChgpuDeviceGuard guard(w->ctx);
    if (!w->have_totals && w->rows)
    {
        u32 t[2] = {0, 0};
        CHGPU_TRY(chgpu_read_back(w->ctx, win_totals(w), t, sizeof(t)));
        w->partitions = t[0];
        w->peer_groups = t[1];
    }
    w->have_totals = true;
    if (rows) *rows = w->rows;
    if (partitions) *partitions = w->partitions;
    if (peer_groups) *peer_groups = w->peer_groups;
    return CHGPU_OK;
}

// the arrays of `needs` the handle lacks: every allocation first, so that a failure leaves the handle as it was
static int win_ensure_bounds(chgpu_window * w, u32 needs)
{
    const u32 missing = w->lazy.missing(needs);
    if (!missing)
        return CHGPU_OK;
    chgpu_ctx * ctx = w->ctx;
    PairMem fresh[5];
    int rc = CHGPU_OK;
    for (u32 k = 0; k < 5 && rc == CHGPU_OK; ++k)
        if (missing & (1u << k))
            rc = w->mem.alloc(win_padded_rows(w->rows) * sizeof(u32), &fresh[k]);
    if (rc != CHGPU_OK)
    {
        for (PairMem & m : fresh)
            pair_free_mem(ctx, m);
        return rc;
    }
    const u8 * flags = (const u8 *)w->flags.p;
    const u32 * part = (const u32 *)w->part.p;
    const dim3 grid((u32)w->n_tiles), block(WIN_THREADS);
    for (u32 k = 0; k < 5; ++k)
    {
        if (!(missing & (1u << k)))
            continue;
        u32 * out = (u32 *)fresh[k].p;
        switch (1u << k)
        {
            case WIN_B_PS: hipLaunchKernelGGL(k_win_bound<WIN_M_FWD_MAX>, grid, block, 0, ctx->stream, flags, 1u, part + WIN_P_LAST_P * w->n_tiles, out); break;
            case WIN_B_GS: hipLaunchKernelGGL(k_win_bound<WIN_M_FWD_MAX>, grid, block, 0, ctx->stream, flags, 2u, part + WIN_P_LAST_G * w->n_tiles, out); break;
            case WIN_B_PE: hipLaunchKernelGGL(k_win_bound<WIN_M_BWD_MIN>, grid, block, 0, ctx->stream, flags, 1u, part + WIN_P_FIRST_P * w->n_tiles, out); break;
            case WIN_B_GE: hipLaunchKernelGGL(k_win_bound<WIN_M_BWD_MIN>, grid, block, 0, ctx->stream, flags, 2u, part + WIN_P_FIRST_G * w->n_tiles, out); break;
            default: hipLaunchKernelGGL(k_win_bound<WIN_M_FWD_COUNT>, grid, block, 0, ctx->stream, flags, 2u, part + WIN_P_COUNT_G * w->n_tiles, out); break;
        }
        ctx->counters[6] += 1;
        w->bounds[k] = fresh[k];
        w->lazy.mark(1u << k);
    }
    CHGPU_HIP(hipGetLastError());
    return CHGPU_OK;
}

static int win_result_type(int function, int arg_type)
{
    switch (function)
    {
        case CHGPU_WIN_ROW_NUMBER: case CHGPU_WIN_RANK: case CHGPU_WIN_DENSE_RANK: case CHGPU_WIN_COUNT: return CHGPU_U64;
        case CHGPU_WIN_SUM: return chgpu_sum_result_type(arg_type);
        case CHGPU_WIN_AVG: return CHGPU_F64;
        default: return arg_type;
    }
}

// the eight integer types an ORDER BY column of a RANGE offset has: fn(X{})
template <typename F>
static void win_dispatch_order_type(int type, F && fn)
{
    switch (type)
    {
        case CHGPU_I64: return fn(i64{});
        case CHGPU_U64: return fn(u64{});
        case CHGPU_I32: return fn(i32{});
        case CHGPU_U32: return fn(u32{});
        case CHGPU_I16: return fn(i16{});
        case CHGPU_U16: return fn(u16{});
        case CHGPU_I8: return fn(i8{});
        default: return fn(u8{});
    }
}

// One validated call: `frame` and `plan` are what win_check_frame and win_plan answered.  `order` is read only where the plan searches a
// bound.
static int win_run(chgpu_window * w, int function, const chgpu_window_frame & frame, const WinPlan & plan, const chgpu_col * order, int descending, const chgpu_col * arg,
                   uint64_t offset, uint64_t default_bits, chgpu_col ** out)
{
    chgpu_ctx * ctx = w->ctx;
    ChgpuDeviceGuard guard(ctx);
    const u64 n = w->rows;
    const u32 needs = plan.needs;
    const int arg_type = arg ? arg->type : -1;
    chgpu_col * res = nullptr;
    if (n == 0)
    {
        CHGPU_TRY(chgpu_col_new(ctx, win_result_type(function, arg_type), 0, &res));
        *out = res;
        return CHGPU_OK;
    }
    // every allocation of the call before its first launch that writes: temporaries, then the lazy bounds, then the result
    PairTemps tmp(w->mem);
    u64 * scan = nullptr;   // P[n + 1] or M[n]
    void * tiles = nullptr; // u64 / WinSeg per tile
    u64 * mask = nullptr;   // general min / max: u64 per row of the whole blocks, then the table's levels of n_blocks cells each
    u64 * table = nullptr;
    u32 * fs = nullptr;     // searched bounds, whole tiles long; a call's own, not kept in the handle
    u32 * fe = nullptr;
    const bool is_sum = function == CHGPU_WIN_SUM || function == CHGPU_WIN_AVG;
    const bool is_ext = plan.ext != WIN_EXT_NONE, general = plan.ext == WIN_EXT_GENERAL;
    const int is_min = function == CHGPU_WIN_MIN ? 1 : 0;
    const u64 n_blocks = win_ext_blocks(n);
    const u32 levels = general ? win_ext_levels(plan.width, n_blocks) : 0;
    if (general)
    {
        CHGPU_TRY(tmp.alloc(n_blocks * WIN_EXT_BLOCK * sizeof(u64), (void **)&mask));
        CHGPU_TRY(tmp.alloc(n_blocks * (levels ? levels : 1) * sizeof(u64), (void **)&table));
    }
    else if (is_sum || is_ext)
    {
        CHGPU_TRY(tmp.alloc((n + 1) * sizeof(u64), (void **)&scan));
        CHGPU_TRY(tmp.alloc(w->n_tiles * sizeof(WinSeg), &tiles));
    }
    if (plan.search_begin)
        CHGPU_TRY(tmp.alloc(win_padded_rows(n) * sizeof(u32), (void **)&fs));
    if (plan.search_end)
        CHGPU_TRY(tmp.alloc(win_padded_rows(n) * sizeof(u32), (void **)&fe));
    CHGPU_TRY(win_ensure_bounds(w, needs));
    CHGPU_TRY(chgpu_col_new(ctx, win_result_type(function, arg_type), n, &res));

    WinBounds b{};
    b.ps = needs & WIN_B_PS ? (const u32 *)w->bounds[0].p : nullptr;
    b.pe = needs & WIN_B_PE ? (const u32 *)w->bounds[1].p : nullptr;
    b.gs = needs & WIN_B_GS ? (const u32 *)w->bounds[2].p : nullptr;
    b.ge = needs & WIN_B_GE ? (const u32 *)w->bounds[3].p : nullptr;
    b.dense = needs & WIN_B_DENSE ? (const u32 *)w->bounds[4].p : nullptr;
    b.fs = fs;
    b.fe = fe;
    const dim3 tile_grid((u32)w->n_tiles), block(WIN_THREADS), out_grid((u32)win_out_blocks(n));
    hipStream_t st = ctx->stream;
    if (fs || fe)
    {
        const WinRangeSide begin{fs, frame.begin_offset, frame.begin_kind == CHGPU_BOUND_OFFSET_FOLLOWING ? 1 : 0};
        const WinRangeSide end{fe, frame.end_offset, frame.end_kind == CHGPU_BOUND_OFFSET_FOLLOWING ? 1 : 0};
        const dim3 row_grid((u32)(n / WIN_THREADS + (n % WIN_THREADS != 0)));
        win_dispatch_order_type(order->type, [&](auto tag) {
            typedef decltype(tag) X;
            hipLaunchKernelGGL(k_win_range_bound<X>, row_grid, block, 0, st, (const X *)order->data, descending ? 1 : 0, b.ps, b.pe, n, begin, end);
        });
        ctx->counters[6] += 1;
    }
    if (is_sum)
    {
        hipLaunchKernelGGL(k_win_tile_sums, tile_grid, block, 0, st, (const void *)arg->data, arg_type, n, (u64 *)tiles);
        hipLaunchKernelGGL(k_win_scan_tile_sums, dim3(1), dim3(WIN_PASS), 0, st, (u64 *)tiles, w->n_tiles);
        hipLaunchKernelGGL(k_win_prefix_apply, tile_grid, block, 0, st, (const void *)arg->data, arg_type, n, (const u64 *)tiles, scan);
        hipLaunchKernelGGL(k_win_out_sum, out_grid, block, 0, st, function == CHGPU_WIN_AVG ? 1 : 0, chgpu_type_is_signed(arg_type) ? 1 : 0, frame, b, n,
                           (const u64 *)scan, (u64 *)res->data);
        ctx->counters[6] += 4;
    }
    else if (general)
    {
        const u32 waves = WIN_THREADS / 64;
        hipLaunchKernelGGL(k_win_ext_masks, dim3((u32)(n_blocks / waves + (n_blocks % waves != 0))), block, 0, st, (const void *)arg->data, arg_type, is_min, n, n_blocks,
                           mask, table);
        const dim3 level_grid((u32)(n_blocks / WIN_THREADS + (n_blocks % WIN_THREADS != 0)));
        for (u32 j = 1; j < levels; ++j) // every level a launch of its own: it reads what the launch before wrote
            hipLaunchKernelGGL(k_win_ext_level, level_grid, block, 0, st, (const u64 *)(table + (j - 1) * n_blocks), table + j * n_blocks, n_blocks, (u64)1 << (j - 1));
        dispatch_width(chgpu_type_size(arg_type), [&](auto tag) {
            typedef decltype(tag) W;
            hipLaunchKernelGGL(k_win_out_extremum_any<W>, out_grid, block, 0, st, arg_type, is_min, frame, b, n, (const void *)arg->data, (const u64 *)mask,
                               (const u64 *)table, n_blocks, (W *)res->data);
        });
        ctx->counters[6] += 2 + (levels > 1 ? levels - 1 : 0);
    }
    else if (is_ext)
    {
        dispatch_const<0, 1>(plan.ext == WIN_EXT_BACKWARD ? 1 : 0, [&](auto back) {
            constexpr bool BACK = decltype(back)::value != 0;
            const u32 * bound = BACK ? b.pe : b.ps;
            hipLaunchKernelGGL(k_win_seg_tiles<BACK>, tile_grid, block, 0, st, (const void *)arg->data, arg_type, is_min, bound, n, (WinSeg *)tiles);
            hipLaunchKernelGGL(k_win_scan_seg_tiles, dim3(1), dim3(WIN_PASS), 0, st, (WinSeg *)tiles, w->n_tiles);
            hipLaunchKernelGGL(k_win_seg_apply<BACK>, tile_grid, block, 0, st, (const void *)arg->data, arg_type, is_min, bound, n, (const WinSeg *)tiles, scan);
            dispatch_width(chgpu_type_size(arg_type), [&](auto tag) {
                typedef decltype(tag) W;
                hipLaunchKernelGGL(k_win_out_extremum<W>, out_grid, block, 0, st, arg_type, is_min, BACK ? 1 : 0, frame, b, n, (const u64 *)scan, (W *)res->data);
            });
        });
        ctx->counters[6] += 4;
    }
    else if (win_function_takes_arg(function))
    {
        const int pick = function == CHGPU_WIN_FIRST_VALUE ? WIN_PICK_FIRST : function == CHGPU_WIN_LAST_VALUE ? WIN_PICK_LAST
            : function == CHGPU_WIN_LAG_IN_FRAME ? WIN_PICK_LAG : WIN_PICK_LEAD;
        dispatch_width(chgpu_type_size(arg_type), [&](auto tag) {
            typedef decltype(tag) W;
            hipLaunchKernelGGL(k_win_out_pick<W>, out_grid, block, 0, st, pick, frame, b, n, (const W *)arg->data, offset, default_bits, (W *)res->data);
        });
        ctx->counters[6] += 1;
    }
    else
    {
        hipLaunchKernelGGL(k_win_out_rank, out_grid, block, 0, st, function, frame, b, n, (u64 *)res->data);
        ctx->counters[6] += 1;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
    {
        chgpu_col_free(res);
        return chgpu_set_error(CHGPU_ERR_DEVICE, "window: launching the kernels failed: %s", hipGetErrorString(e));
    }
    *out = res;
    return CHGPU_OK;
}

// a column a call was given, or NULL: a known type, on the window's device
static int win_check_col(const chgpu_ctx * ctx, const chgpu_col * col, const char * what)
{
    if (col)
    {
        CHGPU_REQUIRE(chgpu_type_size(col->type) != 0, CHGPU_ERR_BAD_ARGUMENTS, "window: the %s column has an unknown type", what);
        CHGPU_REQUIRE(col->ctx && col->ctx->device == ctx->device, CHGPU_ERR_BAD_ARGUMENTS, "window: the %s column lives on another device", what);
    }
    return CHGPU_OK;
}

static int win_check_rows(const chgpu_window * w, const chgpu_col * col, const char * what)
{
    CHGPU_REQUIRE(!col || col->rows == w->rows, CHGPU_ERR_SIZES_MISMATCH, "window: the %s has %llu rows, the window %llu", what, (unsigned long long)col->rows,
                  (unsigned long long)w->rows);
    return CHGPU_OK;
}

// Both entries: the checks in the one order that decides the code of a call with two faults (NULLs; the frame; the columns' types and
// devices; win_plan: what is given, what the handle recorded, what is not implemented; the columns' rows), then win_run.  `framed`:
// chgpu_window_evaluate_framed asks; chgpu_window_evaluate has no order column to give.
static int win_evaluate(bool framed, chgpu_window * w, int function, const chgpu_window_frame * frame_in, const chgpu_col * order, int descending, const chgpu_col * arg,
                        uint64_t offset, uint64_t default_bits, chgpu_col ** out)
{
    CHGPU_REQUIRE(w && out, CHGPU_ERR_BAD_ARGUMENTS, "NULL argument");
    const char * msg = "";
    chgpu_window_frame frame = frame_in ? *frame_in : win_default_frame();
    int rc = CHGPU_OK;
    if (win_function_ignores_frame(function))
        frame = win_default_frame();
    else if ((rc = win_check_frame(frame, framed, &msg)) != CHGPU_OK)
        return chgpu_set_error(rc, "window: %s", msg);
    CHGPU_TRY(win_check_col(w->ctx, arg, "argument"));
    CHGPU_TRY(win_check_col(w->ctx, order, "order"));
    WinPlan plan;
    std::string why;
    if ((rc = win_plan(framed, function, frame, arg ? arg->type : -1, order ? order->type : -1, w->n_order, w->order_type, &plan, &why)) != CHGPU_OK)
        return chgpu_set_error(rc, "window: %s", why.c_str());
    CHGPU_TRY(win_check_rows(w, order, "order column"));
    CHGPU_TRY(win_check_rows(w, arg, "argument"));
    return win_run(w, function, win_frame_without_zero_range_offsets(frame), plan, order, descending, arg, offset, default_bits, out);
}

extern "C" int chgpu_window_evaluate(chgpu_window * w, int function, const chgpu_window_frame * frame_in, const chgpu_col * arg, uint64_t offset,
                                     uint64_t default_bits, chgpu_col ** out)
{
    return win_evaluate(false, w, function, frame_in, nullptr, 0, arg, offset, default_bits, out);
}

extern "C" int chgpu_window_evaluate_framed(chgpu_window * w, int function, const chgpu_window_frame * frame_in, const chgpu_col * order, int descending,
                                            const chgpu_col * arg, uint64_t offset, uint64_t default_bits, chgpu_col ** out)
{
    return win_evaluate(true, w, function, frame_in, order, descending, arg, offset, default_bits, out);
}
