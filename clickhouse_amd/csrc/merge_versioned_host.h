// merge_versioned_host.h — the VersionedCollapsing merge (merge_versioned_kernels.hip) as plain C++: the two scan states, their combines,
// the survive rule, and the two walks over a thread's positions that the kernels are made of.  Everything is __host__ __device__ under
// hipcc and reads its inputs through plain pointers, so that tests/merge_versioned_driver.cpp replays the very code the kernels run, tile
// by tile and chunk by chunk, under a sanitizer.
//
// Rule restated from src/Processors/Merges/Algorithms/VersionedCollapsingAlgorithm.cpp (include/chgpu.h has the contract).  Within a group
// -- rows equal on every sort column, the version, which is the last of them, included -- the reference keeps a queue that only ever
// holds rows of one sign (sign_in_queue): a row of that sign is pushed, a row of the other sign removes the queue's back row and both
// vanish, and the group's end emits the queue front to back.  That is a parenthesis matching, and in closed form, with
//     B_0 = 0,  B_t = B_(t-1) + s_t   over the group's rows in merged order            (the balance)
// row t of sign s survives  <=>  s * B_t >= 1  (it was pushed)  and  s * B_u >= s * B_t for every later row u of its group (never popped).
// The queue here is unbounded; the reference's max_rows_in_queue is not modelled, and the largest |B_t| is returned so that a caller can
// tell whether that bound would have been reached.
//
// Two states carry this through any split of the positions:
//   VcSum    forward: the sum of the signs since the last head, and whether a head was seen.  B_t = (prefix (+) row t).sum
//   VcAfter  backward: of a stretch of positions, the part in front of its first head (the rows that continue the group of the position
//            before the stretch): its sign sum and the least and the greatest of its prefix sums, the empty prefix (0) included, so
//            mn <= 0 <= mx.  With A = VcAfter of everything behind row t:  B_u - B_t are A's prefix sums, so
//            "never popped"  <=>  A.mn == 0 for a positive row, A.mx == 0 for a negative one.
// THE INVARIANT (merge_fold_host.h's): both combines are associative and a head cuts them, so every B_t and every A is the same however the
// positions are split into threads, tiles and passes; the output offsets are an exclusive sum of survivor counts in position order.
// Nothing depends on which workgroup runs first, and there are no atomics.  Sums are 64 bits wide in every state: a group of 2^32 - 1
// rows of one sign reaches +-(2^32 - 1).
#pragma once

#include "merge_fold_host.h"

struct VcSum
{
    int64_t sum;
    uint32_t head;  // a head is among the positions: sum counts from the last one
};
struct VcAfter
{
    int64_t sum, mn, mx;  // of the part in front of the first head
    uint32_t closed;      // a head is among the positions: nothing behind them continues the part
};

FOLD_HD VcSum vc_sum_id() { return VcSum{0, 0}; }
FOLD_HD VcAfter vc_after_id() { return VcAfter{0, 0, 0, 0}; }

// a before b in M
FOLD_HD VcSum vc_sum_combine(const VcSum & a, const VcSum & b) { return b.head ? b : VcSum{a.sum + b.sum, a.head}; }
FOLD_HD VcAfter vc_after_combine(const VcAfter & a, const VcAfter & b)
{
    if (a.closed)
        return a;
    const int64_t lo = a.sum + b.mn, hi = a.sum + b.mx;
    return VcAfter{a.sum + b.sum, lo < a.mn ? lo : a.mn, hi > a.mx ? hi : a.mx, b.closed};
}

// one position: sign is +1 or -1
FOLD_HD VcSum vc_sum_of(int sign, bool head) { return VcSum{sign, head ? 1u : 0u}; }
FOLD_HD VcAfter vc_after_of(int sign, bool head)
{
    if (head)
        return VcAfter{0, 0, 0, 1};
    return VcAfter{sign, sign < 0 ? -1 : 0, sign > 0 ? 1 : 0, 0};
}

// balance: B_t with row t counted; after: VcAfter of every position behind t
FOLD_HD bool vc_survives(int sign, int64_t balance, const VcAfter & after) { return sign > 0 ? (balance >= 1 && after.mn == 0) : (balance <= -1 && after.mx == 0); }
FOLD_HD uint64_t vc_abs(int64_t v) { return v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v; }

// ---- a thread's FOLD_ITEMS consecutive positions, as the kernels hold them in registers: byte i of `heads` is position p0 + i's head
// flag, bit i of `positive` is set where its sign is +1, `count` positions are real (fewer at the end of M) ----
struct VcItems
{
    uint64_t heads;
    uint32_t positive;
    uint32_t count;
    FOLD_HD bool head(uint32_t i) const { return ((heads >> (8 * i)) & 0xFF) != 0; }
    FOLD_HD int sign(uint32_t i) const { return ((positive >> i) & 1) ? 1 : -1; }
};
static_assert(FOLD_ITEMS == 8, "VcItems packs a thread's positions into one 64-bit word of head bytes and one byte of sign bits");

// from the columns where they lie: positions [p0, p0 + FOLD_ITEMS) cut at n
FOLD_HD VcItems vc_items_load(const uint8_t * heads, const uint32_t * rows, const int8_t * sign, uint64_t p0, uint64_t n)
{
    VcItems it{0, 0, 0};
    for (uint32_t i = 0; i < FOLD_ITEMS && p0 + i < n; ++i)
    {
        it.heads |= (uint64_t)(heads[p0 + i] ? 1 : 0) << (8 * i);
        it.positive |= (sign[rows[p0 + i]] == 1 ? 1u : 0u) << i;
        it.count = i + 1;
    }
    return it;
}

// the positions as one element of each scan
FOLD_HD void vc_aggregate(const VcItems & it, VcSum & f, VcAfter & g)
{
    f = vc_sum_id();
    g = vc_after_id();
    for (uint32_t i = 0; i < FOLD_ITEMS; ++i)  // (constant bounds: the loops unroll and the items stay in registers)
        if (i < it.count)
            f = vc_sum_combine(f, vc_sum_of(it.sign(i), it.head(i)));
    for (uint32_t i = FOLD_ITEMS; i-- > 0;)
        if (i < it.count)
            g = vc_after_combine(vc_after_of(it.sign(i), it.head(i)), g);
}

// the positions between `before` (VcSum of everything in front of them) and `after` (VcAfter of everything behind them): bit i of the
// result is set where position i survives; *max_abs is raised to the largest |B| among them
FOLD_HD uint32_t vc_decide(const VcItems & it, const VcSum & before, const VcAfter & after, uint64_t * max_abs)
{
    int64_t balance[FOLD_ITEMS];
    VcSum f = before;
    for (uint32_t i = 0; i < FOLD_ITEMS; ++i)
    {
        balance[i] = 0;
        if (i < it.count)
        {
            f = vc_sum_combine(f, vc_sum_of(it.sign(i), it.head(i)));
            balance[i] = f.sum;
            const uint64_t a = vc_abs(f.sum);
            *max_abs = a > *max_abs ? a : *max_abs;
        }
    }
    uint32_t mask = 0;
    VcAfter g = after;
    for (uint32_t i = FOLD_ITEMS; i-- > 0;)
        if (i < it.count)
        {
            if (vc_survives(it.sign(i), balance[i], g))
                mask |= 1u << i;
            g = vc_after_combine(vc_after_of(it.sign(i), it.head(i)), g);
        }
    return mask;
}
