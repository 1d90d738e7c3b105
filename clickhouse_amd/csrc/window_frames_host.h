// window_frames_host.h — the parts of chgpu_window_evaluate_framed (window_kernels.hip) that need no device, beside window_host.h: which
// frames and plans the framed entry serves, the search over the ORDER BY column's values behind a RANGE frame with an offset, and the
// block / level arithmetic of the general min / max (64-row masks plus a sparse table over the blocks' extrema).  Plain C++; what the
// kernels share is __host__ __device__ under hipcc, so that tests/window_frames_driver.cpp runs the very code under a sanitizer.
#pragma once

#include "window_host.h"

// ---------------------------------------------------------------------------------------------
// frames and plans
// ---------------------------------------------------------------------------------------------
static inline bool win_frame_has_range_offset(const chgpu_window_frame & f)
{
    return f.type == CHGPU_FRAME_RANGE && (win_bound_is_offset(f.begin_kind) || win_bound_is_offset(f.end_kind));
}

// win_check_frame, except that a legal RANGE frame with an offset passes
static inline int win_check_frame_framed(const chgpu_window_frame & f, const char ** msg)
{
    int rc = win_check_frame(f, msg);
    if (rc == CHGPU_ERR_NOT_IMPLEMENTED && win_frame_has_range_offset(f))
        return *msg = nullptr, CHGPU_OK;
    return rc;
}

static inline bool win_order_type_is_served(int type)
{
    switch (type)
    {
        case CHGPU_I64: case CHGPU_U64: case CHGPU_I32: case CHGPU_U32: case CHGPU_I16: case CHGPU_U16: case CHGPU_I8: case CHGPU_U8: return true;
        default: return false;
    }
}

// A RANGE offset of 0 is the peer group's edge: `0 PRECEDING` / `0 FOLLOWING` become CURRENT ROW (the search runs away from the row and
// could not find an end that lies on the row's other side).
static inline chgpu_window_frame win_frame_without_zero_range_offsets(chgpu_window_frame f)
{
    if (f.type != CHGPU_FRAME_RANGE)
        return f;
    if (win_bound_is_offset(f.begin_kind) && f.begin_offset == 0)
        f.begin_kind = CHGPU_BOUND_CURRENT_ROW;
    if (win_bound_is_offset(f.end_kind) && f.end_offset == 0)
        f.end_kind = CHGPU_BOUND_CURRENT_ROW;
    return f;
}

// how min / max run
enum
{
    WIN_EXT_NONE = 0, // not min / max
    WIN_EXT_FORWARD,  // the running extremum from the partition's first row (window_host.h's plan)
    WIN_EXT_BACKWARD, // ... up to its last row
    WIN_EXT_GENERAL   // block masks + sparse table: any frame
};

struct WinFramedPlan
{
    uint32_t needs = 0;     // the handle's bound arrays the call reads
    int ext = WIN_EXT_NONE;
    bool old_entry = false; // window_host.h's win_check_frame + win_plan serve it: the framed entry runs the old path
    bool search_begin = false, search_end = false; // fs[] / fe[] come from the search over the order column
    uint64_t width = 0;     // GENERAL: the most rows a frame can hold (~0: unknown), which bounds the levels of the table
};

// the most rows a ROWS frame whose bounds are offsets or CURRENT ROW can hold; ~0 for every other frame
static inline uint64_t win_frame_max_width(const chgpu_window_frame & f)
{
    const int b = f.begin_kind, e = f.end_kind;
    if (f.type != CHGPU_FRAME_ROWS || b == CHGPU_BOUND_UNBOUNDED_PRECEDING || e == CHGPU_BOUND_UNBOUNDED_FOLLOWING)
        return ~0ull;
    const uint64_t bo = b == CHGPU_BOUND_CURRENT_ROW ? 0 : f.begin_offset, eo = e == CHGPU_BOUND_CURRENT_ROW ? 0 : f.end_offset;
    const bool b_before = b != CHGPU_BOUND_OFFSET_FOLLOWING, e_before = e == CHGPU_BOUND_OFFSET_PRECEDING;
    if (b_before && !e_before)
        return win_sat_add(win_sat_add(bo, eo), 1); // k PRECEDING .. m FOLLOWING
    if (b_before)
        return bo - eo + 1;                         // k PRECEDING .. m PRECEDING, k >= m
    return eo - bo + 1;                             // k FOLLOWING .. m FOLLOWING, k <= m
}

// Is this (function, frame, argument type, order column) served by the framed entry, and how?  `frame` has passed win_check_frame_framed
// (it is not looked at for the three rank functions).  arg_type < 0: no argument; order_type < 0: no order column given.
static inline int win_plan_framed(int function, const chgpu_window_frame & frame_in, int arg_type, int order_type, WinFramedPlan * plan, const char ** msg)
{
    *plan = WinFramedPlan{};
    const bool searched = !win_function_ignores_frame(function) && win_frame_has_range_offset(frame_in);
    if (searched && order_type < 0)
        return *msg = "a RANGE frame with an offset needs the ORDER BY column (NULL given)", CHGPU_ERR_BAD_ARGUMENTS;
    if (!searched && order_type >= 0)
        return *msg = "an ORDER BY column is taken only with a RANGE frame that has an offset", CHGPU_ERR_BAD_ARGUMENTS;
    const chgpu_window_frame frame = searched ? win_frame_without_zero_range_offsets(frame_in) : frame_in;
    bool backward = false;
    const char * old_msg = nullptr;
    // the old plan over the frame as ROWS answers everything but the two gaps: unknown functions, arguments, float sums, the bounds read
    chgpu_window_frame as_rows = frame;
    if (searched)
        as_rows.type = CHGPU_FRAME_ROWS;
    int rc = win_plan(function, as_rows, arg_type, &plan->needs, &backward, &old_msg);
    const bool is_ext = function == CHGPU_WIN_MIN || function == CHGPU_WIN_MAX;
    const bool two_sided = is_ext && rc == CHGPU_ERR_NOT_IMPLEMENTED; // (the one thing the old plan refuses min / max for)
    if (rc != CHGPU_OK && !two_sided)
        return *msg = old_msg, rc;
    if (searched && !win_order_type_is_served(order_type))
        return *msg = "a RANGE frame with an offset over a Float32 / Float64 ORDER BY column is not implemented", CHGPU_ERR_NOT_IMPLEMENTED;
    if (!win_function_ignores_frame(function))
        plan->needs = win_frame_needs(frame);
    plan->search_begin = searched && win_bound_is_offset(frame.begin_kind);
    plan->search_end = searched && win_bound_is_offset(frame.end_kind);
    if (is_ext)
    {
        // a frame that is searched goes through the general structure even when one side is UNBOUNDED: the running extremum would do,
        // but one path less is one path less to test
        if (two_sided || searched)
            plan->ext = WIN_EXT_GENERAL, plan->width = win_frame_max_width(frame);
        else
            plan->ext = backward ? WIN_EXT_BACKWARD : WIN_EXT_FORWARD, plan->needs |= backward ? WIN_B_PE : WIN_B_PS;
    }
    plan->old_entry = !searched && !two_sided;
    return CHGPU_OK;
}

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
