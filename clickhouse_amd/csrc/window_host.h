// window_host.h — the parts of the window operator (window_kernels.hip) that need no device: the one frame check (win_check_frame) and
// the one plan (win_plan) both entries, chgpu_window_evaluate and chgpu_window_evaluate_framed, go through, the frame of a row, the
// bookkeeping of the bound arrays' lazy construction, and the tile / grid arithmetic of the scans.  Plain C++ (the functions the kernels
// share are __host__ __device__ under hipcc), so that tests/window_driver.cpp runs the very code the kernels run under a sanitizer.
#pragma once

#include <cstdint>
#include <string>

#include "../../include/chgpu.h"

#ifdef __HIPCC__
#define WIN_HD __host__ __device__ __forceinline__
#else
#define WIN_HD static inline
#endif

// bounds are 32-bit: the whole sorted input has at most 2^32 - 1 rows, so `one past the last row` still fits
static constexpr uint64_t WIN_MAX_ROWS = 0xFFFFFFFFull;
static constexpr uint32_t WIN_THREADS = 256;                   // threads of the per-tile kernels
static constexpr uint32_t WIN_ITEMS = 8;                       // consecutive rows a thread owns in a scan
static constexpr uint32_t WIN_TILE = WIN_THREADS * WIN_ITEMS;  // T: rows of one scan tile
static constexpr uint32_t WIN_PASS = 1024;                     // G: tile partials one pass of the one-workgroup kernel covers
static constexpr uint32_t WIN_OUT_ROWS = 4;                    // rows a thread of an output kernel owns (16 bytes of a u32 bound array)
static constexpr uint32_t WIN_OUT_BLOCK = WIN_THREADS * WIN_OUT_ROWS;
static constexpr uint32_t WIN_MAX_KEYS = 8;                    // columns of PARTITION BY, and of ORDER BY

WIN_HD uint64_t win_sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

static inline uint64_t win_tiles(uint64_t rows) { return rows / WIN_TILE + (rows % WIN_TILE != 0); }
static inline uint64_t win_passes(uint64_t n_tiles) { return n_tiles / WIN_PASS + (n_tiles % WIN_PASS != 0); }
static inline uint64_t win_out_blocks(uint64_t rows) { return rows / WIN_OUT_BLOCK + (rows % WIN_OUT_BLOCK != 0); }
// rows of a bound / flag array: whole tiles, so that a thread's 16-byte access at a multiple of four rows never leaves the allocation
static inline uint64_t win_padded_rows(uint64_t rows) { return win_tiles(rows) * WIN_TILE; }

// RANGE UNBOUNDED PRECEDING .. CURRENT ROW: the reference's default frame (WindowFrame's member initialisers, WindowDescription.h)
static inline chgpu_window_frame win_default_frame()
{
    chgpu_window_frame f{};
    f.type = CHGPU_FRAME_RANGE;
    f.begin_kind = CHGPU_BOUND_UNBOUNDED_PRECEDING;
    f.end_kind = CHGPU_BOUND_CURRENT_ROW;
    return f;
}

static inline bool win_bound_is_offset(int kind) { return kind == CHGPU_BOUND_OFFSET_PRECEDING || kind == CHGPU_BOUND_OFFSET_FOLLOWING; }

// a RANGE frame with an offset: its bounds come from a search over the order column's values
static inline bool win_frame_has_range_offset(const chgpu_window_frame & f)
{
    return f.type == CHGPU_FRAME_RANGE && (win_bound_is_offset(f.begin_kind) || win_bound_is_offset(f.end_kind));
}

// WindowFrame::checkValid (WindowDescription.cpp).  CHGPU_OK, or the code with *msg saying why.  A legal RANGE frame with an offset is
// NOT_IMPLEMENTED for an entry that does not serve such frames (chgpu_window_evaluate: it has no order column to search).
static inline int win_check_frame(const chgpu_window_frame & f, bool serves_range_offsets, const char ** msg)
{
    const int b = f.begin_kind, e = f.end_kind;
    if (f.type != CHGPU_FRAME_ROWS && f.type != CHGPU_FRAME_RANGE)
        return *msg = "unknown frame type", CHGPU_ERR_BAD_ARGUMENTS;
    if (b < CHGPU_BOUND_UNBOUNDED_PRECEDING || b > CHGPU_BOUND_UNBOUNDED_FOLLOWING || e < CHGPU_BOUND_UNBOUNDED_PRECEDING || e > CHGPU_BOUND_UNBOUNDED_FOLLOWING)
        return *msg = "unknown frame bound", CHGPU_ERR_BAD_ARGUMENTS;
    if (b == CHGPU_BOUND_UNBOUNDED_FOLLOWING)
        return *msg = "frame begin cannot be UNBOUNDED FOLLOWING", CHGPU_ERR_BAD_ARGUMENTS;
    if (e == CHGPU_BOUND_UNBOUNDED_PRECEDING)
        return *msg = "frame end cannot be UNBOUNDED PRECEDING", CHGPU_ERR_BAD_ARGUMENTS;
    if (b == CHGPU_BOUND_CURRENT_ROW && e == CHGPU_BOUND_OFFSET_PRECEDING)
        return *msg = "frame begins at the current row and ends before it", CHGPU_ERR_BAD_ARGUMENTS;
    if (b == CHGPU_BOUND_OFFSET_FOLLOWING && (e == CHGPU_BOUND_CURRENT_ROW || e == CHGPU_BOUND_OFFSET_PRECEDING))
        return *msg = "frame begins after the current row and ends at or before it", CHGPU_ERR_BAD_ARGUMENTS;
    if (b == CHGPU_BOUND_OFFSET_PRECEDING && e == CHGPU_BOUND_OFFSET_PRECEDING && f.begin_offset < f.end_offset)
        return *msg = "frame begin is closer to the current row than its end (both PRECEDING)", CHGPU_ERR_BAD_ARGUMENTS;
    if (b == CHGPU_BOUND_OFFSET_FOLLOWING && e == CHGPU_BOUND_OFFSET_FOLLOWING && f.begin_offset > f.end_offset)
        return *msg = "frame begin is further from the current row than its end (both FOLLOWING)", CHGPU_ERR_BAD_ARGUMENTS;
    if (!serves_range_offsets && win_frame_has_range_offset(f))
        return *msg = "RANGE frames with an offset are not implemented", CHGPU_ERR_NOT_IMPLEMENTED;
    return CHGPU_OK;
}

// The frame [*fs, *fe) of row i of a frame that passed win_check_frame.  [ps, pe) is the row's partition, [gs, ge) its peer group (read
// only by RANGE .. CURRENT ROW).  Nothing wraps for offsets up to 2^64 - 1: i, pe <= 2^32 - 1, and the one sum that can pass 2^64 saturates.
WIN_HD void win_frame_of(const chgpu_window_frame & f, uint64_t i, uint64_t ps, uint64_t pe, uint64_t gs, uint64_t ge, uint64_t * fs, uint64_t * fe)
{
    uint64_t b = ps, e = pe;
    switch (f.begin_kind)
    {
        case CHGPU_BOUND_OFFSET_PRECEDING: b = i >= f.begin_offset && i - f.begin_offset > ps ? i - f.begin_offset : ps; break;
        case CHGPU_BOUND_CURRENT_ROW: b = f.type == CHGPU_FRAME_ROWS ? i : gs; break;
        case CHGPU_BOUND_OFFSET_FOLLOWING: { const uint64_t t = win_sat_add(i, f.begin_offset); b = t < pe ? t : pe; break; }
        default: break;
    }
    switch (f.end_kind)
    {
        case CHGPU_BOUND_OFFSET_PRECEDING: e = i + 1 >= f.end_offset && i + 1 - f.end_offset > ps ? i + 1 - f.end_offset : ps; break;
        case CHGPU_BOUND_CURRENT_ROW: e = f.type == CHGPU_FRAME_ROWS ? i + 1 : ge; break;
        case CHGPU_BOUND_OFFSET_FOLLOWING: { const uint64_t t = win_sat_add(win_sat_add(i, f.end_offset), 1); e = t < pe ? t : pe; break; }
        default: break;
    }
    *fs = b;
    *fe = e;
}

// lagInFrame / leadInFrame: the row t = i -/+ offset; false when it falls outside [fs, fe) (or outside u64)
WIN_HD bool win_shifted_row(bool lead, uint64_t i, uint64_t offset, uint64_t fs, uint64_t fe, uint64_t * t)
{
    if (lead ? offset > ~0ull - i : offset > i)
        return false;
    *t = lead ? i + offset : i - offset;
    return *t >= fs && *t < fe;
}

// The per-row arrays a handle derives from its keys, each built on the first call that reads it
enum
{
    WIN_B_PS = 1,     // first row of the row's partition
    WIN_B_PE = 2,     // one past its last row
    WIN_B_GS = 4,     // the same for the peer group
    WIN_B_GE = 8,
    WIN_B_DENSE = 16, // peer heads in [0, i]
    WIN_B_ALL = 31
};

// the arrays win_frame_of reads for this frame
static inline uint32_t win_frame_needs(const chgpu_window_frame & f)
{
    uint32_t n = 0;
    if (f.begin_kind == CHGPU_BOUND_CURRENT_ROW)
        n |= f.type == CHGPU_FRAME_RANGE ? WIN_B_GS : 0;
    else if (f.begin_kind == CHGPU_BOUND_OFFSET_FOLLOWING)
        n |= WIN_B_PE;
    else
        n |= WIN_B_PS;
    if (f.end_kind == CHGPU_BOUND_CURRENT_ROW)
        n |= f.type == CHGPU_FRAME_RANGE ? WIN_B_GE : 0;
    else if (f.end_kind == CHGPU_BOUND_OFFSET_PRECEDING)
        n |= WIN_B_PS;
    else
        n |= WIN_B_PE;
    return n;
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

static inline bool win_function_takes_arg(int function) { return function >= CHGPU_WIN_SUM && function <= CHGPU_WIN_LEAD_IN_FRAME; }
static inline bool win_function_ignores_frame(int function) { return function >= CHGPU_WIN_ROW_NUMBER && function <= CHGPU_WIN_DENSE_RANK; }
static inline bool win_type_is_float(int type) { return type == CHGPU_F64 || type == CHGPU_F32; }

// how min / max run
enum
{
    WIN_EXT_NONE = 0, // not min / max
    WIN_EXT_FORWARD,  // the running extremum from the partition's first row
    WIN_EXT_BACKWARD, // ... up to its last row
    WIN_EXT_GENERAL   // block masks + sparse table: any frame
};

struct WinPlan
{
    uint32_t needs = 0; // the handle's bound arrays the call reads
    int ext = WIN_EXT_NONE;
    bool search_begin = false, search_end = false; // fs[] / fe[] come from the search over the order column
    uint64_t width = 0; // GENERAL: the most rows a frame can hold (~0: unknown), which bounds the levels of the table
};

// Is this call served, and how?  `framed`: chgpu_window_evaluate_framed asks, else chgpu_window_evaluate, which takes no order column
// and refuses min / max over a frame bounded on both sides.  `frame` has passed win_check_frame for that entry (it is not looked at for
// the three rank functions).  arg_type / order_type < 0: no such column given.  n_order and recorded_order_type are what the handle's
// create saw: how many ORDER BY columns, and the type of the first.  The order of the checks decides the code of a call with two faults.
static inline int win_plan(bool framed, int function, const chgpu_window_frame & frame_in, int arg_type, int order_type, uint32_t n_order, int recorded_order_type,
                           WinPlan * plan, std::string * msg)
{
    *plan = WinPlan{};
    const bool searched = !win_function_ignores_frame(function) && win_frame_has_range_offset(frame_in);
    if (searched && order_type < 0)
        return *msg = "a RANGE frame with an offset needs the ORDER BY column (NULL given)", CHGPU_ERR_BAD_ARGUMENTS;
    if (!searched && order_type >= 0)
        return *msg = "an ORDER BY column is taken only with a RANGE frame that has an offset", CHGPU_ERR_BAD_ARGUMENTS;
    if (function < CHGPU_WIN_ROW_NUMBER || function > CHGPU_WIN_LEAD_IN_FRAME)
        return *msg = "unknown window function", CHGPU_ERR_BAD_ARGUMENTS;
    if (win_function_takes_arg(function) != (arg_type >= 0))
        return *msg = win_function_takes_arg(function) ? "the function takes an argument column (NULL given)" : "the function takes no argument column", CHGPU_ERR_BAD_ARGUMENTS;
    if (order_type >= 0 && n_order != 1)
        return *msg = "a RANGE frame with an offset needs a window with exactly one ORDER BY column, this one has " + std::to_string(n_order), CHGPU_ERR_BAD_ARGUMENTS;
    if (order_type >= 0 && order_type != recorded_order_type)
        return *msg = "the order column's type differs from the one the window was created with", CHGPU_ERR_BAD_ARGUMENTS;
    if ((function == CHGPU_WIN_SUM || function == CHGPU_WIN_AVG) && win_type_is_float(arg_type))
        return *msg = "sum / avg over a Float32 / Float64 argument is not implemented (a parallel scan rounds differently)", CHGPU_ERR_NOT_IMPLEMENTED;
    if (searched && win_type_is_float(order_type))
        return *msg = "a RANGE frame with an offset over a Float32 / Float64 ORDER BY column is not implemented", CHGPU_ERR_NOT_IMPLEMENTED;
    const bool is_ext = function == CHGPU_WIN_MIN || function == CHGPU_WIN_MAX;
    const bool two_sided = frame_in.begin_kind != CHGPU_BOUND_UNBOUNDED_PRECEDING && frame_in.end_kind != CHGPU_BOUND_UNBOUNDED_FOLLOWING;
    if (!framed && is_ext && two_sided)
        return *msg = "min / max over a frame bounded on both sides is not implemented", CHGPU_ERR_NOT_IMPLEMENTED;
    switch (function)
    {
        case CHGPU_WIN_ROW_NUMBER: plan->needs = WIN_B_PS; return CHGPU_OK;
        case CHGPU_WIN_RANK: plan->needs = WIN_B_PS | WIN_B_GS; return CHGPU_OK;
        case CHGPU_WIN_DENSE_RANK: plan->needs = WIN_B_PS | WIN_B_DENSE; return CHGPU_OK;
        default: break;
    }
    const chgpu_window_frame frame = win_frame_without_zero_range_offsets(frame_in); // the frame the kernels get
    plan->needs = win_frame_needs(frame);
    plan->search_begin = searched && win_bound_is_offset(frame.begin_kind);
    plan->search_end = searched && win_bound_is_offset(frame.end_kind);
    if (!is_ext)
        return CHGPU_OK;
    // A frame that is searched goes through the general structure even when one side is UNBOUNDED: the running extremum would do, but
    // one path less is one path less to test.  The running extremum is segmented by partition: forward from ps it also reads ps,
    // backward from pe it reads pe.
    if (two_sided || searched)
        plan->ext = WIN_EXT_GENERAL, plan->width = win_frame_max_width(frame);
    else if (frame.begin_kind == CHGPU_BOUND_UNBOUNDED_PRECEDING)
        plan->ext = WIN_EXT_FORWARD, plan->needs |= WIN_B_PS;
    else
        plan->ext = WIN_EXT_BACKWARD, plan->needs |= WIN_B_PE;
    return CHGPU_OK;
}

// Which arrays a handle has built.  take(needs) answers the ones still to build and counts them as built from then on.
struct WinLazy
{
    uint32_t built = 0;
    uint32_t builds = 0; // arrays built so far: each at most once
    uint32_t missing(uint32_t needs) const { return needs & ~built & WIN_B_ALL; }
    void mark(uint32_t one)
    {
        if (!(built & one))
            builds += 1;
        built |= one;
    }
};
