// group_table.h — key -> group index over the finalised groups of an operator that keeps (group key, value) pairs (uniqExact,
// quantileExact): an open-addressing table of u32 cells, cell = group index + 1, 0 = empty.  The group keys are distinct, so building
// takes the first empty cell; the capacity is a power of two of at least twice the groups, so a walk always meets an empty cell.
// What else the two operators share is pair_store.h.
#pragma once

#include "chgpu_internal.h"

#ifdef __HIPCC__

static constexpr u32 GT_NONE = 0xFFFFFFFFu;
static constexpr u32 GT_T = 256; // threads of the kernels the pair operators share

// cells for `groups` keys
static inline u64 gt_capacity_for(u64 groups)
{
    u64 cap = 64;
    while (cap < 2 * groups)
        cap *= 2;
    return cap;
}

// group g's key into the table
__device__ __forceinline__ void gt_insert(const u64 * __restrict__ gkeys, u64 g, u32 * __restrict__ cells, u64 cap)
{
    const u64 mask = cap - 1;
    u64 pos = dev_intHash64(gkeys[g]) & mask;
    for (u64 step = 0; step <= cap; ++step)
    {
        if (cells[pos] == 0 && atomicCAS(&cells[pos], 0u, (u32)g + 1) == 0)
            break;
        pos = (pos + 1) & mask;
    }
}

// the group of `key`, GT_NONE when no group has it (a table no kernel is writing)
__device__ __forceinline__ u32 gt_find(const u64 * __restrict__ gkeys, const u32 * __restrict__ cells, u64 cap, u64 key)
{
    const u64 mask = cap - 1;
    u64 pos = dev_intHash64(key) & mask;
    for (u64 step = 0; step <= cap; ++step)
    {
        const u32 c = cells[pos];
        if (c == 0)
            break;
        if (gkeys[c - 1] == key)
            return c - 1;
        pos = (pos + 1) & mask;
    }
    return GT_NONE;
}

static __global__ __launch_bounds__(GT_T) void k_gt_build(const u64 * __restrict__ gkeys, u64 groups, u32 * __restrict__ cells, u64 cap)
{
    for (u64 g = (u64)blockIdx.x * GT_T + threadIdx.x; g < groups; g += (u64)gridDim.x * GT_T)
        gt_insert(gkeys, g, cells, cap);
}

// The table of `groups` distinct keys in `cap` cells the caller allocated: cleared, then built (no launch for no group).  `op` names
// the operator in the message.  Counting the launches and checking them stays with the caller.
static int gt_fill(chgpu_ctx * ctx, const char * op, const u64 * gkeys, u64 groups, u32 * cells, u64 cap)
{
    if (hipMemsetAsync(cells, 0, cap * 4, ctx->stream) != hipSuccess)
        return chgpu_set_error(CHGPU_ERR_DEVICE, "%s: clearing the key table failed", op);
    if (groups)
        hipLaunchKernelGGL(k_gt_build, dim3(chgpu_grid_for(ctx, groups, GT_T, 8)), dim3(GT_T), 0, ctx->stream, gkeys, groups, cells, cap);
    return CHGPU_OK;
}

#endif // __HIPCC__
