// group_table.h — key -> group index over the finalised groups of an operator that keeps (group key, value) pairs (uniqExact,
// quantileExact): an open-addressing table of u32 cells, cell = group index + 1, 0 = empty.  The group keys are distinct, so building
// takes the first empty cell; the capacity is a power of two of at least twice the groups, so a walk always meets an empty cell.
#pragma once

#include "chgpu_internal.h"

#ifdef __HIPCC__

static constexpr u32 GT_NONE = 0xFFFFFFFFu;

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

#endif // __HIPCC__
