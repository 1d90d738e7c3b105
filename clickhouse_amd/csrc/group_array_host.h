// group_array_host.h — the parts of the groupArray operator (group_array_kernels.hip) that need no device: which radix passes the two
// key words ask for, the capacity of the doubling store, max_size, the geometry of the segmented copy's work units, and the `debug`
// option's plan lines.  Plain C++ (the functions the kernels share are __host__ __device__ under hipcc), so that
// tests/group_array_driver.cpp runs them under a sanitizer.
#pragma once

#include <cstdint>
#include <cstdio>

#include "../../include/chgpu.h"
#include "pair_host.h"

#ifdef __HIPCC__
#define GA_HD __host__ __device__ __forceinline__
#else
#define GA_HD static inline
#endif

// a store holds fewer than 2^32 - 1 values: group ids and lengths are 32-bit, 0xFFFFFFFF is "no group"
static constexpr uint64_t GA_MAX_VALUES = 0xFFFFFFFFull;
// rows of one tile of the order-preserving append and of the boundary kernels: 256 threads x 8 steps
static constexpr uint64_t GA_TILE = 2048;
// output elements of one work unit of the segmented copy: 256 threads x 16 elements
static constexpr uint64_t GA_UNIT = 4096;

// capacity of the doubling store that takes `need` values: a power of two, at least 4096.  0: `need` is beyond the row limit.
static inline uint64_t ga_capacity_for(uint64_t need)
{
    if (need >= GA_MAX_VALUES)
        return 0;
    uint64_t cap = 4096;
    while (cap < need)
        cap *= 2;
    return cap;
}

// The radix passes of finalize.  or_bits / and_bits are the OR and the AND of every key in the store (0 and ~0 for an empty one), so
// or_bits & ~and_bits is the set of key bits that differ anywhere.  One stable 256-way pass per key BYTE that holds such a bit, least
// significant first: shifts[0 .. return) are the passes' bit shifts.  A byte in which no bit varies is equal in all keys: a pass over it
// would be the identity.
static inline uint32_t ga_plan_passes(uint64_t or_bits, uint64_t and_bits, uint32_t shifts[8])
{
    const uint64_t vary = or_bits & ~and_bits;
    uint32_t n = 0;
    for (uint32_t b = 0; b < 8; ++b)
        if ((vary >> (8 * b)) & 0xFF)
            shifts[n++] = 8 * b;
    return n;
}

// groupArray(N): the first N values of a group of `count`; N = 0 is no limit
GA_HD uint64_t ga_trim(uint64_t count, uint64_t max_size) { return max_size && count > max_size ? max_size : count; }

// The segmented copy writes `total` output elements, array s being [s ? ends[s - 1] : 0, ends[s]) of them (ColumnArray offsets).  Its
// work is divided by OUTPUT ELEMENT, never by array: unit u owns elements [u * GA_UNIT, min(total, (u + 1) * GA_UNIT)) and finds the
// arrays they belong to by binary search, so that one array of 1e8 values beside a million arrays of one is the same number of equal units.
GA_HD uint64_t ga_units(uint64_t total) { return (total + GA_UNIT - 1) / GA_UNIT; }

// the array of output element e: the first s in [lo, hi) with ends[s] > e (empty arrays are stepped over); hi when there is none
GA_HD uint64_t ga_seg_of(const uint64_t * ends, uint64_t lo, uint64_t hi, uint64_t e)
{
    while (lo < hi)
    {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (ends[mid] > e)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// unit `unit` of a copy of n_segs arrays: its elements [*e0, *e1) and the arrays [*s0, *s1] they lie in (total != 0, unit < ga_units)
GA_HD void ga_unit_range(const uint64_t * ends, uint64_t n_segs, uint64_t total, uint64_t unit, uint64_t * e0, uint64_t * e1, uint64_t * s0, uint64_t * s1)
{
    *e0 = unit * GA_UNIT;
    *e1 = *e0 + GA_UNIT < total ? *e0 + GA_UNIT : total;
    *s0 = ga_seg_of(ends, 0, n_segs, *e0);
    *s1 = ga_seg_of(ends, *s0, n_segs, *e1 - 1);
}

// what one chgpu_group_array_add_block / chgpu_group_array_merge did
struct GaAddPlan
{
    const char * what = "add";
    uint64_t n = 0;       // rows of the call's range (merge: values of the source)
    uint64_t entered = 0; // rows that entered
    uint64_t held_before = 0, held = 0;
    int rc = 0;
};

static inline int ga_format_add_plan(char * buf, size_t size, const GaAddPlan & p)
{
    return snprintf(buf, size, "chgpu: group_array plan=%s n=%llu entered=%llu held=%llu->%llu rc=%d", p.what, (unsigned long long)p.n,
                    (unsigned long long)p.entered, (unsigned long long)p.held_before, (unsigned long long)p.held, p.rc);
}

// what one chgpu_group_array_finalize / chgpu_group_array_for_keys did
struct GaPlan
{
    const char * what = "finalize";
    uint64_t groups = 0, values = 0;
    uint32_t passes = 0;  // radix passes the segments were built with (one per key byte that varies)
    uint64_t trimmed = 0; // held values that max_size keeps out of the arrays
    int cached = 0;       // the segments of an earlier call were reused
};

static inline int ga_format_plan(char * buf, size_t size, const GaPlan & p)
{
    return snprintf(buf, size, "chgpu: group_array plan=%s groups=%llu values=%llu passes=%u trimmed=%llu cached=%d", p.what, (unsigned long long)p.groups,
                    (unsigned long long)p.values, p.passes, (unsigned long long)p.trimmed, p.cached);
}
