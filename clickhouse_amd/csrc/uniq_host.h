// uniq_host.h — the parts of the uniqExact operator (uniq_kernels.hip) that need no device: table geometry and the `debug` option's
// plan line; the row checks of chgpu_uniq_add_block are pair_host.h's.  Plain C++, so that tests/uniq_exact_driver.cpp runs them
// under a sanitizer.
#pragma once

#include <cstdint>
#include <cstdio>

#include "../../include/chgpu.h"
#include "pair_host.h"

static constexpr uint64_t UQ_CAP_MIN = 2048;            // cells of the smallest table (a power of two, like every capacity)
static constexpr uint64_t UQ_MAX_SLOTS = 1ull << 31;     // a cell holds store index + 1 in 32 bits; the 32-bit slot counter may pass the limit by a grid of lanes
static constexpr uint64_t UQ_CAP_MAX = 1ull << 32;       // limit = capacity / 2 = UQ_MAX_SLOTS: the last capacity

// growth: x4 up to 2^23 cells, then x2 (the geometry of the other tables)
static inline uint64_t uq_grow(uint64_t cap) { return cap < (1ull << 23) ? cap * 4 : cap * 2; }

// the table holds capacity / 2 pairs
static inline uint64_t uq_limit(uint64_t cap)
{
    const uint64_t l = cap / 2;
    return l < UQ_MAX_SLOTS ? l : UQ_MAX_SLOTS;
}

// smallest power of two whose limit takes `pairs`; 0 when no table does
static inline uint64_t uq_capacity_for(uint64_t pairs)
{
    if (pairs > UQ_MAX_SLOTS)
        return 0;
    uint64_t cap = UQ_CAP_MIN;
    while (uq_limit(cap) < pairs)
        cap *= 2;
    return cap;
}

// what one chgpu_uniq_add_block / chgpu_uniq_merge did
struct UqPlan
{
    const char * what = "add";
    uint64_t n = 0;                    // rows of the call's range
    uint64_t cap_before = 0, cap = 0;  // cells
    uint64_t tiles = 0;                // row tiles that went through the LDS stage
    uint32_t chunks = 0;
    uint64_t found = 0;                // rows whose pair the loop-free look-up found in its home cell (a set that held something)
    uint64_t lds = 0;                  // rows settled in LDS: their pair was already in the workgroup's set
    uint64_t sent = 0;                 // rows sent on to the global table (the tile's distinct pairs and the overflow rows)
    uint64_t ovf = 0;                  // of those, rows that found no room in the LDS set
    uint64_t deferred = 0;             // times a row met the limit and waited for the table to grow
    uint32_t grown = 0;
    uint64_t slots_before = 0, slots = 0;
    uint64_t holes_before = 0, holes = 0;
    int rc = 0;
};

static inline int uq_format_plan(char * buf, size_t size, const UqPlan & p)
{
    return snprintf(buf, size,
                    "chgpu: uniq plan=%s n=%llu cap=%llu->%llu tiles=%llu chunks=%u found=%llu lds=%llu sent=%llu ovf=%llu deferred=%llu grown=%u slots=%llu->%llu holes=%llu->%llu rc=%d",
                    p.what, (unsigned long long)p.n, (unsigned long long)p.cap_before, (unsigned long long)p.cap, (unsigned long long)p.tiles, p.chunks,
                    (unsigned long long)p.found, (unsigned long long)p.lds, (unsigned long long)p.sent, (unsigned long long)p.ovf, (unsigned long long)p.deferred, p.grown,
                    (unsigned long long)p.slots_before, (unsigned long long)p.slots, (unsigned long long)p.holes_before, (unsigned long long)p.holes, p.rc);
}
