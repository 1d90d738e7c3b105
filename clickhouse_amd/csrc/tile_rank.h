// tile_rank.h — "the items of a tile that satisfy a predicate, ranked in item order", written once for group_array_kernels.hip (the
// filtered append, the run heads of the sorted keys) and limit_by_kernels.hip (the segment heads of the rank plan).
//
// A tile is TILE_ITEMS consecutive items of one workgroup of TILE_T threads, taken wave-striped: step r of wave w covers the 64
// consecutive items from w * TILE_WAVE_ITEMS + r * 64, so the order (wave, step, lane) is item order and a rank is: the lower waves'
// counts + the wave's lower steps + the set bits below the lane.  The places are handed out by counts per tile (k_tile_counts) -> scan
// (tile_scan) -> ranks inside the tile (tile_ballots, tile_for_ranked): no workgroup waits for another, no place is taken by an atomic.
// Kernels are templates: two translation units include this file.
#pragma once

#include "chgpu_internal.h"

static constexpr u32 TILE_T = 256; // threads of a workgroup
static constexpr u32 TILE_R = 8;   // steps of 64 items a wave takes of a tile
static constexpr u32 TILE_ITEMS = TILE_T * TILE_R;
static constexpr u32 TILE_WAVE_ITEMS = TILE_R * 64;

// the first item of a run of equal key words
template <typename W>
struct TileHeadPred
{
    const W * k;
    __device__ __forceinline__ bool operator()(u64 i) const { return i == 0 || k[i] != k[i - 1]; }
};

// the item of this lane in step r
__device__ __forceinline__ u64 tile_item(u64 tile, u32 r) { return tile * TILE_ITEMS + (threadIdx.x >> 6) * TILE_WAVE_ITEMS + r * 64 + lane_id(); }

// the ballots of this wave's steps; returns the number of the tile's items that precede this wave's among those that satisfy `pred`
template <typename P>
__device__ __forceinline__ u32 tile_ballots(const P & pred, u64 tile, u64 n, u64 (&m)[TILE_R], u32 * s_wave /* [TILE_T / 64] */)
{
    u32 cnt = 0;
#pragma unroll
    for (u32 r = 0; r < TILE_R; ++r)
    {
        const u64 i = tile_item(tile, r);
        m[r] = __ballot(i < n && pred(i));
        cnt += (u32)__popcll(m[r]);
    }
    if (lane_id() == 0)
        s_wave[threadIdx.x >> 6] = cnt;
    __syncthreads();
    u32 before = 0;
    for (u32 w = 0; w < (threadIdx.x >> 6); ++w)
        before += s_wave[w];
    return before;
}

// f(item, rank) for every item of this lane that satisfies the predicate; `pos` is the rank of the wave's first such item
// (the tile's offset + what tile_ballots returned)
template <typename F>
__device__ __forceinline__ void tile_for_ranked(const u64 (&m)[TILE_R], u64 tile, u64 pos, F f)
{
#pragma unroll
    for (u32 r = 0; r < TILE_R; ++r)
    {
        if ((m[r] >> lane_id()) & 1)
            f(tile_item(tile, r), pos + mbcnt(m[r]));
        pos += (u32)__popcll(m[r]);
    }
}

template <typename P>
__global__ __launch_bounds__(TILE_T) void k_tile_counts(P pred, u64 n, u64 n_tiles, u32 * __restrict__ counts)
{
    __shared__ u32 s_wave[TILE_T / 64];
    for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
    {
        u64 m[TILE_R];
        tile_ballots(pred, tile, n, m, s_wave);
        if (threadIdx.x == 0)
        {
            u32 total = 0;
            for (u32 w = 0; w < TILE_T / 64; ++w)
                total += s_wave[w];
            counts[tile] = total;
        }
        __syncthreads(); // before the next tile overwrites the counts
    }
}

// counts[n] (already written) -> off[n], exclusive (inclusive: ColumnArray offsets), and the total in *total_dev
static int tile_scan(chgpu_ctx * ctx, const u32 * counts, u64 * off, u64 n, u64 * total_dev, bool inclusive = false)
{
    void * scan_tmp = nullptr;
    const size_t scan_bytes = chgpu_scan_tmp_bytes(n);
    CHGPU_TRY(chgpu_scratch(ctx, scan_bytes, &scan_tmp));
    return inclusive ? chgpu_scan_inclusive_u32_u64(ctx, counts, off, n, total_dev, scan_tmp, scan_bytes)
                     : chgpu_scan_exclusive_u32_u64(ctx, counts, off, n, total_dev, scan_tmp, scan_bytes);
}
