// window_frames_host.h — the parts of the framed calls (chgpu_window_evaluate_framed, window_kernels.hip) that need no device, beside
// window_host.h, which checks and plans them: the search over the ORDER BY column's values behind a RANGE frame with an offset, and the
// block / level arithmetic of the general min / max (64-row masks plus a sparse table over the blocks' extrema).  Plain C++; what the
// kernels share is __host__ __device__ under hipcc, so that tests/window_frames_driver.cpp runs the very code under a sanitizer.
#pragma once

#include "window_host.h"

// ---------------------------------------------------------------------------------------------
// the search behind a RANGE offset
// ---------------------------------------------------------------------------------------------
// The distance of row i + t (forward) or i - t (backward) from row i in the direction the order runs, as the sorted column has it: never
// negative, so the difference of the 64-bit extensions is exact modulo 2^64 for all eight integer types, and `x[i] - k` below the type's
// minimum or `x[i] + k` above its maximum need no branch.  Is it within k (strict: below k)?
template <typename X>
WIN_HD bool win_range_near(const X * x, uint64_t i, X xi, uint64_t t, bool forward, bool descending, uint64_t k, bool strict)
{
    const X xj = x[forward ? i + t : i - t];
    const uint64_t d = forward != descending ? (uint64_t)xj - (uint64_t)xi : (uint64_t)xi - (uint64_t)xj;
    return strict ? d < k : d <= k;
}

// The largest t in [0, limit] whose row is near row i (k > 0, so t = 0 is), the rows being near up to some t and far beyond it.  Gallop:
// steps of 1, 2, 4 .. from the row until a far row or the limit, then a binary search of the last interval; about 2 log2(t) loads, and
// neighbouring rows read neighbouring elements.  Whatever the column holds, every index stays in [i - limit, i + limit] and the loops
// end: the step doubles, and the interval halves.
template <typename X>
WIN_HD uint64_t win_range_gallop(const X * x, uint64_t i, uint64_t limit, bool forward, bool descending, uint64_t k, bool strict)
{
    const X xi = x[i];
    uint64_t lo = 0, hi = 0, step = 1; // lo: near; hi: far
    for (;;)
    {
        if (limit - lo < step)
        {
            if (lo == limit || win_range_near(x, i, xi, limit, forward, descending, k, strict))
                return limit;
            hi = limit;
            break;
        }
        if (!win_range_near(x, i, xi, lo + step, forward, descending, k, strict))
        {
            hi = lo + step;
            break;
        }
        lo += step;
        step <<= 1;
    }
    while (hi - lo > 1)
    {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (win_range_near(x, i, xi, mid, forward, descending, k, strict))
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// One bound of the RANGE frame of row i of the partition [ps, pe): `k PRECEDING` (following = false) or `k FOLLOWING`, k > 0, as the
// frame's begin (end = false) or one past its last row.  Ascending, exact arithmetic:
//   k PRECEDING   begin: first j with x[j] >= x[i] - k          end: first j with x[j] > x[i] - k        both in [ps, i]
//   k FOLLOWING   begin: first j with x[j] >= x[i] + k, or pe   end: first j with x[j] > x[i] + k, or pe both in (i, pe]
// Descending: the same over the negated values.
template <typename X>
WIN_HD uint64_t win_range_bound_of(const X * x, uint64_t i, uint64_t ps, uint64_t pe, bool following, bool end, bool descending, uint64_t k)
{
    if (following)
        return i + win_range_gallop(x, i, pe - 1 - i, true, descending, k, !end) + 1;
    return i - win_range_gallop(x, i, i - ps, false, descending, k, end);
}

// ---------------------------------------------------------------------------------------------
// the general extremum: 64-row blocks, a mask per row, a sparse table over the blocks' extrema
// ---------------------------------------------------------------------------------------------
static constexpr uint32_t WIN_EXT_BLOCK = 64; // rows of a block: one wave

static inline uint64_t win_ext_blocks(uint64_t rows) { return rows / WIN_EXT_BLOCK + (rows % WIN_EXT_BLOCK != 0); }

WIN_HD uint32_t win_log2_floor(uint64_t v) // v > 0
{
    uint32_t l = 0;
    while (v >>= 1)
        l += 1;
    return l;
}

// Levels of the table a call builds: level j holds, for block b, the extremum of the blocks [b, b + 2^j).  A frame of at most `width`
// rows that reaches into two blocks has at most (width - 2) / 64 whole blocks between them, and there are n_blocks - 2 at the most.
static inline uint32_t win_ext_levels(uint64_t width, uint64_t n_blocks)
{
    const uint64_t by_width = width >= 2 ? (width - 2) / WIN_EXT_BLOCK : 0, by_blocks = n_blocks >= 2 ? n_blocks - 2 : 0;
    const uint64_t between = by_width < by_blocks ? by_width : by_blocks;
    return between ? win_log2_floor(between) + 1 : 0;
}

// the two cells of the table that cover the blocks strictly between the blocks bl < br - 1: level j, blocks *c0 and *c1
WIN_HD void win_ext_cells(uint64_t bl, uint64_t br, uint32_t * level, uint64_t * c0, uint64_t * c1)
{
    const uint64_t between = br - bl - 1;
    *level = win_log2_floor(between);
    *c0 = bl + 1;
    *c1 = br - ((uint64_t)1 << *level);
}

WIN_HD uint32_t win_ctz64(uint64_t v) // v != 0
{
    return (uint32_t)__builtin_ctzll(v);
}

// The mask of row r of a block: bit p is set iff no row q in (p, r] of the block has key[q] >= key[p] -- the monotone stack after row
// r.  The extremum of the rows [l, r] of ONE block then stands at the lowest set bit at or above l.
WIN_HD uint64_t win_ext_in_block(uint64_t mask_of_r, uint64_t l) { return l + win_ctz64(mask_of_r >> (l & (WIN_EXT_BLOCK - 1))); }
