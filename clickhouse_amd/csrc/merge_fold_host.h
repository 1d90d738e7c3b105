// merge_fold_host.h — the folds of the Replacing / Collapsing / Summing / Aggregating merges (merge_fold_kernels.hip) as plain C++: each
// algorithm's state, its combine operator and what a group emits at its tail, the segmented combine that stops at a group's head, and
// the three walks the kernels are made of (a thread's items, a workgroup's tiles, the apply with its tail counts), and a tile's geometry
// (a thread's positions, the padded staging slot).  Everything is
// __host__ __device__ under hipcc and reads its columns through plain pointers, so that tests/merge_fold_driver.cpp replays the very code
// the kernels run, tile by tile, under a sanitizer.
//
// Rules restated from src/Processors/Merges/Algorithms/ReplacingSortedAlgorithm.cpp, CollapsingSortedAlgorithm.cpp,
// SummingSortedAlgorithm.cpp and AggregatingSortedAlgorithm.cpp (include/chgpu.h has the contract).
//
// THE INVARIANT: a group's result is a function of its rows in merged order alone.  Every combine below is associative, a head cuts the
// scan, so the value at a tail is the same however the positions are split into threads, tiles and chunks of tiles; the output offsets
// are an exclusive sum of the tail counts in position order.  Nothing depends on which workgroup runs first, and there are no atomics.
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

#include <cstdint>

#include "merge_host.h"

#ifdef __HIPCC__
#define FOLD_HD __host__ __device__ __forceinline__
#else
#define FOLD_HD inline
#endif

static constexpr uint32_t FOLD_THREADS = MRG_THREADS;
static constexpr uint32_t FOLD_ITEMS = MRG_ITEMS;  // consecutive merged positions of a thread
static constexpr uint32_t FOLD_TILE = MRG_TILE;    // T: merged positions of a workgroup
static constexpr uint32_t FOLD_MAX_VALUES = 8;     // value columns of one folding call
static constexpr uint32_t FOLD_MAX_OUT = 2;        // outputs of one group (Collapsing: the negative and the positive row)

// flags of a scan element: it covers at least one position / a group's head is among them
enum : uint8_t { FOLD_ANY = 1, FOLD_HEAD = 2 };

// ---- the geometry of a tile, for every kernel behind the heads (the folds' and merge_versioned_kernels.hip's) and for the drivers ----
// the positions of thread `thread` of tile `tile`: [p0, p1), cut at n (empty past it).  p0 is a multiple of FOLD_ITEMS wherever the
// range is whole (p1 - p0 == FOLD_ITEMS).
FOLD_HD void fold_thread_range(uint32_t tile, uint32_t thread, uint64_t n, uint64_t & p0, uint64_t & p1)
{
    p0 = (uint64_t)tile * FOLD_TILE + (uint64_t)thread * FOLD_ITEMS;
    p1 = p0 + FOLD_ITEMS;
    p0 = p0 < n ? p0 : n;
    p1 = p1 < n ? p1 : n;
}
// Where a tile's element e waits in LDS when the states are staged (merge_fold_kernels.hip): one slot of padding per FOLD_ITEMS states,
// so that neighbouring lanes are 9 states apart, not 8, and their 16-byte reads fall on different banks.
static constexpr uint32_t FOLD_STAGE_SLOTS = FOLD_TILE + FOLD_TILE / FOLD_ITEMS;
FOLD_HD uint32_t fold_stage_slot(uint32_t e) { return e + e / FOLD_ITEMS; }

// ---- integer columns by their type tag ----
FOLD_HD bool fold_type_is_int(int type)
{
    switch (type)
    {
        case CHGPU_I64: case CHGPU_U64: case CHGPU_I32: case CHGPU_U32: case CHGPU_I16: case CHGPU_U16: case CHGPU_I8: case CHGPU_U8: return true;
        default: return false;
    }
}
FOLD_HD bool fold_type_is_signed(int type) { return type == CHGPU_I64 || type == CHGPU_I32 || type == CHGPU_I16 || type == CHGPU_I8; }
// the value sign- or zero-extended to 64 bits
FOLD_HD uint64_t fold_widen(const void * data, int type, uint64_t row)
{
    switch (type)
    {
        case CHGPU_I64: return (uint64_t)((const int64_t *)data)[row];
        case CHGPU_U64: return ((const uint64_t *)data)[row];
        case CHGPU_I32: return (uint64_t)(int64_t)((const int32_t *)data)[row];
        case CHGPU_U32: return ((const uint32_t *)data)[row];
        case CHGPU_I16: return (uint64_t)(int64_t)((const int16_t *)data)[row];
        case CHGPU_U16: return ((const uint16_t *)data)[row];
        case CHGPU_I8: return (uint64_t)(int64_t)((const int8_t *)data)[row];
        default: return ((const uint8_t *)data)[row];
    }
}
// the low bytes of `bits` as the column's element (wrap-around in the column's own type)
FOLD_HD void fold_store(void * data, int type, uint64_t row, uint64_t bits)
{
    switch (type)
    {
        case CHGPU_I64: case CHGPU_U64: ((uint64_t *)data)[row] = bits; break;
        case CHGPU_I32: case CHGPU_U32: ((uint32_t *)data)[row] = (uint32_t)bits; break;
        case CHGPU_I16: case CHGPU_U16: ((uint16_t *)data)[row] = (uint16_t)bits; break;
        default: ((uint8_t *)data)[row] = (uint8_t)bits; break;
    }
}
FOLD_HD uint64_t fold_width_mask(int type)
{
    switch (type)
    {
        case CHGPU_I64: case CHGPU_U64: return ~0ull;
        case CHGPU_I32: case CHGPU_U32: return 0xFFFFFFFFull;
        case CHGPU_I16: case CHGPU_U16: return 0xFFFFull;
        default: return 0xFFull;
    }
}
// an unsigned word that orders like the widened value does in the column's signedness, and back
FOLD_HD uint64_t fold_order_word(uint64_t widened, int type) { return fold_type_is_signed(type) ? widened ^ 0x8000000000000000ull : widened; }

// ---- Replacing: the LAST row in M among those of the greatest version (the reference compares with >= 0) ----
struct ReplacingFold
{
    const void * version = nullptr;  // NULL: the group's last row
    int32_t version_type = 0;
    const uint8_t * is_deleted = nullptr;
    int32_t cleanup = 0;
    struct State
    {
        uint64_t version_word;
        uint32_t row;
    };
    static constexpr bool PAIRED = false;
    FOLD_HD State load(uint32_t row) const
    {
        State s;
        s.version_word = version ? fold_order_word(fold_widen(version, version_type, row), version_type) : 0;
        s.row = row;
        return s;
    }
    // a comes before b in M: greater, or equal and later
    FOLD_HD State combine(const State & a, const State & b) const { return b.version_word >= a.version_word ? b : a; }
    FOLD_HD uint32_t emit(const State & s, uint32_t /*tail_row*/, uint32_t * out) const
    {
        if (is_deleted && cleanup && is_deleted[s.row] == 1)
            return 0;
        out[0] = s.row;
        return 1;
    }
    FOLD_HD void store(const State &, uint64_t) const {}
};

// ---- Collapsing ----
struct CollapsingFold
{
    const int8_t * sign = nullptr;
    struct State
    {
        uint32_t count_positive, count_negative, first_negative, last_positive;
    };
    static constexpr bool PAIRED = false;
    FOLD_HD State load(uint32_t row) const
    {
        const bool positive = sign[row] == 1;
        State s;
        s.count_positive = positive ? 1 : 0;
        s.count_negative = positive ? 0 : 1;
        s.first_negative = positive ? 0 : row;
        s.last_positive = positive ? row : 0;
        return s;
    }
    FOLD_HD State combine(const State & a, const State & b) const
    {
        State s;
        s.count_positive = a.count_positive + b.count_positive;
        s.count_negative = a.count_negative + b.count_negative;
        s.first_negative = a.count_negative ? a.first_negative : b.first_negative;
        s.last_positive = b.count_positive ? b.last_positive : a.last_positive;
        return s;
    }
    FOLD_HD uint32_t emit(const State & s, uint32_t tail_row, uint32_t * out) const
    {
        const bool last_is_positive = sign[tail_row] == 1;
        if (!(last_is_positive || s.count_positive != s.count_negative))
            return 0;
        uint32_t n = 0;
        if (s.count_positive <= s.count_negative)
            out[n++] = s.first_negative;
        if (s.count_positive >= s.count_negative)
            out[n++] = s.last_positive;
        return n;
    }
    FOLD_HD void store(const State &, uint64_t) const {}
};

// ---- Folding: Summing, and Aggregating over SimpleAggregateFunction columns ----
struct FoldValues
{
    const void * data[FOLD_MAX_VALUES];
    void * out[FOLD_MAX_VALUES];  // the result columns, indexed by output row
    int32_t type[FOLD_MAX_VALUES];
    int32_t kind[FOLD_MAX_VALUES];
    uint32_t n;
    int32_t drop_zero;
};

template <uint32_t NV>
struct FoldingFold
{
    FoldValues d;
    struct State
    {
        uint64_t v[NV ? NV : 1];  // SUM: the wrapped sum of the widened values; MIN / MAX: the extreme order word
        uint32_t first;           // the group's first row: any
    };
    static constexpr bool PAIRED = true;  // an output is the pair (first row, last row)
    FOLD_HD State load(uint32_t row) const
    {
        State s;
        s.v[0] = 0;
        for (uint32_t k = 0; k < NV; ++k)
        {
            const uint64_t w = fold_widen(d.data[k], d.type[k], row);
            s.v[k] = d.kind[k] == CHGPU_FOLD_SUM ? w : fold_order_word(w, d.type[k]);
        }
        s.first = row;
        return s;
    }
    FOLD_HD State combine(const State & a, const State & b) const
    {
        State s;
        s.v[0] = 0;
        for (uint32_t k = 0; k < NV; ++k)
            s.v[k] = d.kind[k] == CHGPU_FOLD_SUM ? a.v[k] + b.v[k] : d.kind[k] == CHGPU_FOLD_MIN ? (b.v[k] < a.v[k] ? b.v[k] : a.v[k]) : (b.v[k] > a.v[k] ? b.v[k] : a.v[k]);
        s.first = a.first;
        return s;
    }
    // the result of value k, widened (SUM: cut to the column's width, which is the wrap-around sum in its own type)
    FOLD_HD uint64_t result(const State & s, uint32_t k) const
    {
        return d.kind[k] == CHGPU_FOLD_SUM ? (s.v[k] & fold_width_mask(d.type[k])) : fold_order_word(s.v[k], d.type[k]);
    }
    FOLD_HD uint32_t emit(const State & s, uint32_t tail_row, uint32_t * out) const
    {
        if (NV && d.drop_zero)
        {
            // Summing's rule: dropped when EVERY SUM result is 0 (with no SUM column among the values that holds for every group)
            bool all_zero = true;
            for (uint32_t k = 0; k < NV; ++k)
                if (d.kind[k] == CHGPU_FOLD_SUM && result(s, k) != 0)
                    all_zero = false;
            if (all_zero)
                return 0;
        }
        out[0] = s.first;
        out[1] = tail_row;
        return 1;
    }
    FOLD_HD void store(const State & s, uint64_t out_row) const
    {
        for (uint32_t k = 0; k < NV; ++k)
            fold_store(d.out[k], d.type[k], out_row, result(s, k));
    }
};

// ---- the segmented combine: (sa, fa) := (sa, fa) (+) (sb, fb), a before b in M.  A head in b cuts off what came before it. ----
template <class A>
FOLD_HD void fold_seg_combine(const A & a, typename A::State & sa, uint8_t & fa, const typename A::State & sb, uint8_t fb)
{
    if (!(fb & FOLD_ANY))
        return;
    if ((fb & FOLD_HEAD) || !(fa & FOLD_ANY))
        sa = sb;
    else
        sa = a.combine(sa, sb);
    fa |= fb;
}

// ---- the walks.  heads[p]: position p of M starts a group; rows[p]: its concatenated row number ----
// Where a walk reads position p from: the columns where they lie.  (A kernel may put a tile's loaded states somewhere closer and answer
// state() from there; everything else is the same.)
template <class A>
struct FoldColumns
{
    const A & a;
    const uint8_t * heads;
    const uint32_t * rows;
    uint64_t n;
    FOLD_HD uint8_t head(uint64_t p) const { return heads[p]; }
    FOLD_HD uint32_t row(uint64_t p) const { return rows[p]; }
    FOLD_HD typename A::State state(uint64_t p) const { return a.load(rows[p]); }
    // the position before the next head, and n - 1
    FOLD_HD bool tail(uint64_t p) const { return p + 1 == n || heads[p + 1]; }
};

// the positions [p0, p1) as one scan element
template <class A, class Src>
FOLD_HD void fold_aggregate(const A & a, const Src & src, uint64_t p0, uint64_t p1, typename A::State & s, uint8_t & fl)
{
    fl = 0;
    for (uint64_t p = p0; p < p1; ++p)
        fold_seg_combine(a, s, fl, src.state(p), (uint8_t)(FOLD_ANY | (src.head(p) ? FOLD_HEAD : 0)));
}

// the positions [p0, p1) behind the prefix (s, fl): sink(p, state, count, out) at every tail
template <class A, class Src, class Sink>
FOLD_HD void fold_apply(const A & a, const Src & src, uint64_t p0, uint64_t p1, typename A::State s, uint8_t fl, Sink && sink)
{
    for (uint64_t p = p0; p < p1; ++p)
    {
        fold_seg_combine(a, s, fl, src.state(p), (uint8_t)(FOLD_ANY | (src.head(p) ? FOLD_HEAD : 0)));
        if (src.tail(p))
        {
            uint32_t out[FOLD_MAX_OUT] = {0, 0};
            const uint32_t count = a.emit(s, src.row(p), out);
            sink(p, s, count, out);
        }
    }
}

// The one-workgroup step over tile aggregates: thread i of FOLD_THREADS owns the tiles [fold_chunk_begin(i), fold_chunk_begin(i + 1)).
FOLD_HD uint32_t fold_chunk_begin(uint32_t thread, uint32_t n_tiles)
{
    const uint32_t per = n_tiles / FOLD_THREADS + (n_tiles % FOLD_THREADS != 0);
    const uint64_t b = (uint64_t)thread * per;
    return b < n_tiles ? (uint32_t)b : n_tiles;
}
template <class A>
FOLD_HD void fold_chunk_aggregate(const A & a, const typename A::State * agg_s, const uint8_t * agg_f, uint32_t t0, uint32_t t1, typename A::State & s, uint8_t & fl)
{
    fl = 0;
    for (uint32_t t = t0; t < t1; ++t)
        fold_seg_combine(a, s, fl, agg_s[t], agg_f[t]);
}
// carry[t]: the state of the group that is open where tile t begins (meaningful for t > 0: position 0 is a head)
template <class A>
FOLD_HD void fold_chunk_carries(const A & a, const typename A::State * agg_s, const uint8_t * agg_f, uint32_t t0, uint32_t t1, typename A::State s, uint8_t fl,
                                typename A::State * carry)
{
    for (uint32_t t = t0; t < t1; ++t)
    {
        carry[t] = s;
        fold_seg_combine(a, s, fl, agg_s[t], agg_f[t]);
    }
}
