// pair_host.h — what the store operators (uniq_host.h, quantile_host.h, group_array_host.h, limit_by_host.h) share and that needs no
// device: the row checks of an add_block, the capacity of the doubling store, and which radix passes a set of key words asks for.
// Plain C++, so that the stand-alone drivers under tests/ run it under a sanitizer.
#pragma once

#include <cstdint>

#include "../../include/chgpu.h"

// The row-range and length checks of an add_block.  key_rows < 0: no key column (without key); filter_rows < 0: no filter.
// Returns CHGPU_OK or the error code, *msg then says why.
static inline int pair_check_rows(int64_t key_rows, uint64_t value_rows, int64_t filter_rows, uint64_t row_begin, uint64_t row_end, const char ** msg)
{
    if (key_rows >= 0 && (uint64_t)key_rows != value_rows)
    {
        *msg = "key and value columns of different lengths";
        return CHGPU_ERR_SIZES_MISMATCH;
    }
    if (filter_rows >= 0 && (uint64_t)filter_rows != value_rows)
    {
        *msg = "filter and value columns of different lengths";
        return CHGPU_ERR_SIZES_MISMATCH;
    }
    if (row_begin > row_end)
    {
        *msg = "row_begin > row_end";
        return CHGPU_ERR_BAD_ARGUMENTS;
    }
    if (row_end > value_rows)
    {
        *msg = "row range past the end of the column";
        return CHGPU_ERR_BAD_ARGUMENTS;
    }
    return CHGPU_OK;
}

// capacity of the doubling (key, value) store that takes `need` values: a power of two, at least 4096
static inline uint64_t pair_capacity_for(uint64_t need)
{
    uint64_t cap = 4096;
    while (cap < need)
        cap *= 2;
    return cap;
}

// The radix passes that bring equal key words together.  `vary` is the set of bits that differ anywhere among the words (the OR of
// them all & ~ the AND of them all; 0 for none or one), `bytes` how many bytes a word has.  One stable 256-way pass per BYTE that holds
// such a bit, least significant first: shifts[0 .. return) are the passes' bit shifts.  A byte in which no bit varies is equal in all
// words: a pass over it would be the identity.
static inline uint32_t pair_plan_passes(uint64_t vary, uint32_t bytes, uint32_t * shifts /* [bytes] */)
{
    uint32_t n = 0;
    for (uint32_t b = 0; b < bytes; ++b)
        if ((vary >> (8 * b)) & 0xFF)
            shifts[n++] = 8 * b;
    return n;
}
