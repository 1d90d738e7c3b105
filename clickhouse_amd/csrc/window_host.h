// window_host.h — the parts of the window operator (window_kernels.hip) that need no device: frame validation, the frame of a row, which
// bound arrays a call needs and the bookkeeping of their lazy construction, and the tile / grid arithmetic of the scans.  Plain C++ (the
// functions the kernels share are __host__ __device__ under hipcc), so that tests/window_driver.cpp runs the very code the kernels run
// under a sanitizer.
#pragma once

#include <cstdint>

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

// WindowFrame::checkValid (WindowDescription.cpp).  CHGPU_OK, or the code with *msg saying why.  A legal RANGE frame with an offset is
// NOT_IMPLEMENTED: it needs a search over the order column's values.
static inline int win_check_frame(const chgpu_window_frame & f, const char ** msg)
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
    if (f.type == CHGPU_FRAME_RANGE && (win_bound_is_offset(b) || win_bound_is_offset(e)))
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

static inline bool win_function_takes_arg(int function) { return function >= CHGPU_WIN_SUM && function <= CHGPU_WIN_LEAD_IN_FRAME; }
static inline bool win_function_ignores_frame(int function) { return function >= CHGPU_WIN_ROW_NUMBER && function <= CHGPU_WIN_DENSE_RANK; }
static inline bool win_type_is_float(int type) { return type == CHGPU_F64 || type == CHGPU_F32; }

// Is this (function, frame, argument type) served, and which arrays does it read?  `frame` has passed win_check_frame (it is not looked
// at for the three rank functions).  arg_type < 0: no argument.
static inline int win_plan(int function, const chgpu_window_frame & frame, int arg_type, uint32_t * needs, bool * backward, const char ** msg)
{
    *needs = 0;
    *backward = false;
    if (function < CHGPU_WIN_ROW_NUMBER || function > CHGPU_WIN_LEAD_IN_FRAME)
        return *msg = "unknown window function", CHGPU_ERR_BAD_ARGUMENTS;
    if (win_function_takes_arg(function) != (arg_type >= 0))
        return *msg = win_function_takes_arg(function) ? "the function takes an argument column (NULL given)" : "the function takes no argument column", CHGPU_ERR_BAD_ARGUMENTS;
    switch (function)
    {
        case CHGPU_WIN_ROW_NUMBER: *needs = WIN_B_PS; return CHGPU_OK;
        case CHGPU_WIN_RANK: *needs = WIN_B_PS | WIN_B_GS; return CHGPU_OK;
        case CHGPU_WIN_DENSE_RANK: *needs = WIN_B_PS | WIN_B_DENSE; return CHGPU_OK;
        default: break;
    }
    *needs = win_frame_needs(frame);
    if ((function == CHGPU_WIN_SUM || function == CHGPU_WIN_AVG) && win_type_is_float(arg_type))
        return *msg = "sum / avg over a Float32 / Float64 argument is not implemented (a parallel scan rounds differently)", CHGPU_ERR_NOT_IMPLEMENTED;
    if (function == CHGPU_WIN_MIN || function == CHGPU_WIN_MAX)
    {
        // the running extremum is segmented by partition: forward from ps it also reads ps, backward from pe it reads pe
        if (frame.begin_kind == CHGPU_BOUND_UNBOUNDED_PRECEDING)
            *needs |= WIN_B_PS;
        else if (frame.end_kind == CHGPU_BOUND_UNBOUNDED_FOLLOWING)
            *needs |= WIN_B_PE, *backward = true;
        else
            return *msg = "min / max over a frame bounded on both sides is not implemented", CHGPU_ERR_NOT_IMPLEMENTED;
    }
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
