// pair_host.h — what the operators that keep (group key, value) pairs (uniq_host.h, quantile_host.h) share and that needs no device.
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
