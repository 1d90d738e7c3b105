// limit_by_host.h — the parts of the DISTINCT / LIMIT BY operator (limit_by_kernels.hip) that need no device: table geometry and
// growth, the checks of create and filter_block, which plan a block takes, which slot bytes the rank plan passes over (the planner is pair_host.h's), and the
// `debug` option's plan line.  Plain C++, so that tests/limit_by_driver.cpp runs them under a sanitizer.
#pragma once

#include <cstdint>
#include <cstdio>

#include "../../include/chgpu.h"
#include "pair_host.h"

// rows of one tile of the resolve and compaction kernels: 256 threads x 4 consecutive rows
static constexpr uint64_t LB_TILE = 1024;
static constexpr uint64_t LB_CAP_MIN = 2048;          // cells of the smallest table (a power of two, like every capacity)
static constexpr uint64_t LB_CAP_MAX = 1ull << 31;    // a slot is a cell index in 32 bits, the slot behind the last cell is the empty value's
static constexpr uint64_t LB_MAX_KEYS = 1ull << 30;   // the table is at most half full
static constexpr uint64_t LB_MAX_ROWS = 0xFFFFFFFFull; // rows of one call: a record holds its row in 32 bits, 0xFFFFFFFF is "no row"
static constexpr uint64_t LB_MAX_BOUND = 0xFFFFFFFFull; // group_offset + group_length: counters are 32-bit and saturate at that sum
static constexpr uint32_t LB_NONE = 0xFFFFFFFFu;      // slot of a row that is dead or did not enter; "no claim"
static constexpr uint32_t LB_MISSING = 0xFFFFFFFEu;   // slot of an entered row whose key the table lacks

// growth: x4 up to 2^23 cells, then x2 (the geometry of the other tables)
static inline uint64_t lb_grow(uint64_t cap) { return cap < (1ull << 23) ? cap * 4 : cap * 2; }

// the table holds capacity / 2 keys
static inline uint64_t lb_limit(uint64_t cap) { return cap / 2; }

// smallest capacity whose limit takes `keys`; 0 when no table does
static inline uint64_t lb_capacity_for(uint64_t keys)
{
    if (keys > LB_MAX_KEYS)
        return 0;
    uint64_t cap = LB_CAP_MIN;
    while (lb_limit(cap) < keys)
        cap *= 2;
    return cap;
}

// a call with this many rows of absent keys or more may grow by more than one geometry step a round
static constexpr uint64_t LB_JUMP_MIN = 1ull << 20;
static constexpr uint64_t LB_JUMP_MAX = 64; // ... but by no more than this factor: the rows may all be rows of a few keys

// The capacity after one growth of a table that met its limit with `keys` keys in it, in a call whose block has `wanted` rows of keys
// the table lacked (an upper bound of the keys to come: they may be rows of one key); 0 when there is no larger table.  One step of
// the growth rule; when the block wants LB_JUMP_MIN keys or more, the capacity that takes them, at most LB_JUMP_MAX times the present
// one (a block of 1e8 new keys that grows by one step a round walks its rows eleven times; 4.25: a block of 1e8 rows
// of a thousand new keys must not get a table for 1e8).
static inline uint64_t lb_next_capacity(uint64_t cap, uint64_t keys, uint64_t wanted)
{
    uint64_t next = lb_grow(cap);
    while (next <= LB_CAP_MAX && lb_limit(next) <= keys)
        next *= 2;
    if (next > LB_CAP_MAX)
        return 0;
    if (wanted >= LB_JUMP_MIN)
    {
        const uint64_t all = keys + wanted < LB_MAX_KEYS ? keys + wanted : LB_MAX_KEYS;
        uint64_t jump = lb_capacity_for(all);
        if (jump > cap * LB_JUMP_MAX)
            jump = cap * LB_JUMP_MAX;
        if (jump > next)
            next = jump;
    }
    return next;
}

// Whether the table grows before the next insert round.  `limit_met`: the round before raised its flag, which rows of keys that
// other rows inserted can do (their tickets are spent) and after which waves stop taking rows.  A table at its limit grows; one that
// met the flag grows when it is at least half way to the limit, or when `stalled` rounds in a row met the flag on this table without
// getting there (every such round inserts at least one key, this bounds them); otherwise the same table takes the rows again.
static inline bool lb_should_grow(uint64_t cap, uint64_t keys, bool limit_met, uint32_t stalled)
{
    if (keys >= lb_limit(cap))
        return true;
    return limit_met && (keys * 2 >= lb_limit(cap) || stalled >= 4);
}

// create's checks of the two bounds.  Returns CHGPU_OK or the error code, *msg then says why.
static inline int lb_check_bounds(uint64_t group_length, uint64_t group_offset, const char ** msg)
{
    if (group_length == 0)
    {
        *msg = "group_length is 0";
        return CHGPU_ERR_BAD_ARGUMENTS;
    }
    if (group_length > LB_MAX_BOUND || group_offset > LB_MAX_BOUND - group_length)
    {
        *msg = "group_offset + group_length beyond 2^32 - 1: 32-bit counters (CPU path)";
        return CHGPU_ERR_NOT_IMPLEMENTED;
    }
    return CHGPU_OK;
}

// filter_block's row checks: the range and the filter's length against the key column
static inline int lb_check_rows(uint64_t key_rows, int64_t filter_rows, uint64_t row_begin, uint64_t row_end, const char ** msg)
{
    const int code = pair_check_rows(-1, key_rows, filter_rows, row_begin, row_end, msg);
    if (code != CHGPU_OK)
    {
        if (code == CHGPU_ERR_SIZES_MISMATCH)
            *msg = "filter and key columns of different lengths";
        return code;
    }
    if (row_end - row_begin > LB_MAX_ROWS)
    {
        *msg = "2^32 rows or more in one call";
        return CHGPU_ERR_TOO_MANY_ROWS;
    }
    return CHGPU_OK;
}

enum LbPlanKind
{
    LB_PLAN_DEAD = 0,  // no live row: a zero filter
    LB_PLAN_CLAIM = 1, // offset + length == 1: the lowest live row of a slot passes
    LB_PLAN_RANK = 2,  // a stable split of the live records by slot, rank = position - segment head
};

static inline LbPlanKind lb_choose_plan(uint64_t live, uint64_t bound /* offset + length */)
{
    if (live == 0)
        return LB_PLAN_DEAD;
    return bound == 1 ? LB_PLAN_CLAIM : LB_PLAN_RANK;
}

static inline const char * lb_plan_name(LbPlanKind k) { return k == LB_PLAN_DEAD ? "dead" : k == LB_PLAN_CLAIM ? "claim" : "rank"; }

// The radix passes of the rank plan: or_bits / and_bits are the OR and the AND of the live records' slots (0 and ~0 for none); the
// planner itself is pair_plan_passes (pair_host.h), here over the four bytes of a slot.  No pass when one slot is live.
static inline uint32_t lb_plan_passes(uint32_t or_bits, uint32_t and_bits, uint32_t shifts[4]) { return pair_plan_passes(or_bits & ~and_bits, 4, shifts); }

// what one chgpu_limit_by_filter_block did
struct LbPlan
{
    LbPlanKind kind = LB_PLAN_DEAD;
    uint64_t n = 0;       // rows of the call's range
    uint64_t entered = 0; // rows whose filter byte was set
    uint64_t live = 0;    // of those, rows whose key's counter was below offset + length at entry
    uint32_t passes = 0;  // radix passes of the rank plan
    uint64_t passed = 0;
    uint64_t keys_before = 0, keys = 0; // keys counted at least once
    uint64_t cap_before = 0, cap = 0;   // cells
    uint32_t grown = 0;
    int rc = 0;
};

static inline int lb_format_plan(char * buf, size_t size, const LbPlan & p)
{
    return snprintf(buf, size, "chgpu: limit_by plan=%s n=%llu entered=%llu live=%llu passes=%u passed=%llu keys=%llu->%llu cap=%llu->%llu grown=%u rc=%d",
                    lb_plan_name(p.kind), (unsigned long long)p.n, (unsigned long long)p.entered, (unsigned long long)p.live, p.passes, (unsigned long long)p.passed,
                    (unsigned long long)p.keys_before, (unsigned long long)p.keys, (unsigned long long)p.cap_before, (unsigned long long)p.cap, p.grown, p.rc);
}
