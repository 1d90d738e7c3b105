// group_array_host.h — the parts of the groupArray operator (group_array_kernels.hip) that need no device: which radix passes the two
// key words ask for and the row limit of the store (over pair_host.h's planner and capacity rule), max_size, the geometry of the
// segmented copy's work units, and the `debug` option's plan lines.  Plain C++ (the functions the kernels share are __host__ __device__ under hipcc), so that
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

// capacity of the store that takes `need` values (pair_host.h).  0: `need` is beyond the row limit.
static inline uint64_t ga_capacity_for(uint64_t need) { return need >= GA_MAX_VALUES ? 0 : pair_capacity_for(need); }

// The radix passes of finalize: or_bits / and_bits are the OR and the AND of every key in the store (0 and ~0 for an empty one); the
// planner itself is pair_plan_passes (pair_host.h), here over the eight bytes of a UInt64 key.
static inline uint32_t ga_plan_passes(uint64_t or_bits, uint64_t and_bits, uint32_t shifts[8]) { return pair_plan_passes(or_bits & ~and_bits, 8, shifts); }

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
