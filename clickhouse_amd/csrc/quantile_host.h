// quantile_host.h — the parts of the quantileExact operator (quantile_kernels.hip) that need no device: the rank table, the level
// checks, the order-preserving value keys, the geometry of the small-segment windows and of the large segments' work units, and the
// `debug` option's plan lines.  Plain C++ (the functions the kernels share are __host__ __device__ under hipcc), so that
// tests/quantile_exact_driver.cpp runs them under a sanitizer.
#pragma once

#include <cstdint>
#include <cstdio>

#include "../../include/chgpu.h"
#include "pair_host.h"

#ifdef __HIPCC__
#define QT_HD __host__ __device__ __forceinline__
#else
#define QT_HD static inline
#endif

// A segment of at most QT_SMALL_MAX values is sorted in LDS; a longer one goes through the radix select.
static constexpr uint64_t QT_SMALL_MAX = 2048;
// Window w of the small-segment kernel takes the segments that START in [w * QT_WINDOW, (w + 1) * QT_WINDOW): they all lie inside
// QT_TILE = QT_WINDOW + QT_SMALL_MAX positions from the first one's start, the tile a workgroup holds in LDS.
static constexpr uint64_t QT_WINDOW = 2048;
static constexpr uint64_t QT_TILE = QT_WINDOW + QT_SMALL_MAX;
// values of a large segment that one work unit of a histogram pass streams
static constexpr uint64_t QT_CHUNK = 16384;
// a store holds fewer than 2^32 values: counts, cursors and histogram counters are 32-bit
static constexpr uint64_t QT_MAX_VALUES = 0xFFFFFFFFull;
// histogram memory of one batch of levels (large segments x levels x 1 KiB); more levels than fit run in batches (the test option
// test_quantile_hist_budget lowers it, so that a few segments already run in batches)
static constexpr uint64_t QT_HIST_BUDGET = 256ull << 20;

static_assert(QT_TILE == 4096 && (QT_TILE & (QT_TILE - 1)) == 0, "the LDS sort network wants a power of two");

// The rank table of QuantileExact / QuantileExactLow / QuantileExactHigh: the 0-based rank, in ascending order, of the element that
// answers `level` in a group of n >= 1 values.  The only place it is written.  EXACT is one IEEE double multiplication, truncated
// (0.29 * 100 = 28.999999999999996 -> 28): the reference's `level < 1 ? level * size : size - 1`.  For n beyond 2^53 the product of a
// level just below 1 can round up to n, where the reference reads past its array; the last line keeps the rank inside the group.
QT_HD uint64_t qt_rank(int kind, double level, uint64_t n)
{
    uint64_t r;
    if (level == 0.5 && kind == CHGPU_QUANTILE_EXACT_LOW)
        r = (n & 1) ? n / 2 : n / 2 - 1;
    else if (level == 0.5 && kind == CHGPU_QUANTILE_EXACT_HIGH)
        r = n / 2;
    else
        r = level < 1 ? (uint64_t)(level * (double)n) : n - 1;
    return r < n ? r : n - 1;
}

// Value -> unsigned key of the value's own width whose unsigned order is the value's order, a bijection on the bits.
// mode 0: unsigned (identity); 1: signed (sign flip); 2: IEEE float (negative: all bits flipped, else the sign bit set), so that
// -0.0 sorts directly before +0.0 and the bits that come back are an element's own.  `width` in bytes.
enum { QT_MODE_UNSIGNED = 0, QT_MODE_SIGNED = 1, QT_MODE_FLOAT = 2 };

QT_HD uint64_t qt_width_mask(uint32_t width) { return width >= 8 ? ~0ull : (1ull << (8 * width)) - 1; }

QT_HD uint64_t qt_encode(uint64_t bits, uint32_t width, int mode)
{
    const uint64_t sign = 1ull << (8 * width - 1);
    if (mode == QT_MODE_SIGNED)
        return bits ^ sign;
    if (mode == QT_MODE_FLOAT)
        return (bits & sign) ? (~bits & qt_width_mask(width)) : (bits | sign);
    return bits;
}

QT_HD uint64_t qt_decode(uint64_t key, uint32_t width, int mode)
{
    const uint64_t sign = 1ull << (8 * width - 1);
    if (mode == QT_MODE_SIGNED)
        return key ^ sign;
    if (mode == QT_MODE_FLOAT)
        return (key & sign) ? (key & ~sign) : (~key & qt_width_mask(width));
    return key;
}

// NaN by the bits (Float32 / Float64): such a row does not enter
QT_HD bool qt_is_nan(uint64_t bits, uint32_t width)
{
    return width == 4 ? (bits & 0x7FFFFFFFull) > 0x7F800000ull : (bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull;
}

// the value of an empty state, as bits: quiet NaN for floats, 0 for integers
QT_HD uint64_t qt_empty_bits(uint32_t width, int mode)
{
    if (mode != QT_MODE_FLOAT)
        return 0;
    return width == 4 ? 0x7FC00000ull : 0x7FF8000000000000ull;
}

// first index g in [0, groups] with offsets[g] >= pos (offsets ascend strictly: every group holds a value)
template <typename OFF>
QT_HD uint64_t qt_lower_bound(const OFF * offsets, uint64_t groups, uint64_t pos)
{
    uint64_t lo = 0, hi = groups;
    while (lo < hi)
    {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)offsets[mid] < pos)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// windows of the small-segment kernel over `values` stored values
QT_HD uint64_t qt_windows(uint64_t values) { return (values + QT_WINDOW - 1) / QT_WINDOW; }

// The segments window w owns: [*g0, *g1) are the ones that start in [w * QT_WINDOW, (w + 1) * QT_WINDOW).  offsets[groups] = values.
template <typename OFF>
QT_HD void qt_window_groups(const OFF * offsets, uint64_t groups, uint64_t w, uint64_t * g0, uint64_t * g1)
{
    *g0 = qt_lower_bound(offsets, groups, w * QT_WINDOW);
    *g1 = qt_lower_bound(offsets, groups, (w + 1) * QT_WINDOW);
}

QT_HD bool qt_is_small(uint64_t n) { return n <= QT_SMALL_MAX; }
// work units of a segment in one histogram pass: none for a small one
QT_HD uint64_t qt_units(uint64_t n) { return qt_is_small(n) ? 0 : (n + QT_CHUNK - 1) / QT_CHUNK; }

// levels of one batch so that large x levels x 1 KiB stays inside the budget (at least one)
static inline uint32_t qt_level_batch(uint64_t large, uint32_t n_levels, uint64_t budget = QT_HIST_BUDGET)
{
    if (large == 0)
        return n_levels;
    const uint64_t fit = budget / (large * 1024);
    return fit >= n_levels ? n_levels : fit < 1 ? 1 : (uint32_t)fit;
}

// The checks of kind and levels of chgpu_quantile_finalize / chgpu_quantile_for_keys.  Returns CHGPU_OK or the code, *msg says why.
static inline int qt_check_levels(int kind, uint32_t n_levels, const double * levels, const char ** msg)
{
    if (kind == CHGPU_QUANTILE_EXACT_INCLUSIVE || kind == CHGPU_QUANTILE_EXACT_EXCLUSIVE || kind == CHGPU_QUANTILE_EXACT_WEIGHTED)
    {
        *msg = "quantileExactInclusive / Exclusive / Weighted are not built (CPU path)";
        return CHGPU_ERR_NOT_IMPLEMENTED;
    }
    if (kind != CHGPU_QUANTILE_EXACT && kind != CHGPU_QUANTILE_EXACT_LOW && kind != CHGPU_QUANTILE_EXACT_HIGH)
    {
        *msg = "unknown kind";
        return CHGPU_ERR_BAD_ARGUMENTS;
    }
    if (n_levels == 0 || n_levels > CHGPU_QUANTILE_MAX_LEVELS)
    {
        *msg = "between 1 and CHGPU_QUANTILE_MAX_LEVELS levels";
        return CHGPU_ERR_BAD_ARGUMENTS;
    }
    if (!levels)
    {
        *msg = "NULL levels";
        return CHGPU_ERR_BAD_ARGUMENTS;
    }
    for (uint32_t i = 0; i < n_levels; ++i)
        if (!(levels[i] >= 0.0 && levels[i] <= 1.0)) // a NaN level fails both
        {
            *msg = "a level outside [0, 1]";
            return CHGPU_ERR_BAD_ARGUMENTS;
        }
    return CHGPU_OK;
}

// capacity of the store that takes `need` values (pair_host.h; qt_reserve answers the row limit in front of it)
static inline uint64_t qt_capacity_for(uint64_t need) { return pair_capacity_for(need); }

// what one chgpu_quantile_add_block / chgpu_quantile_merge did
struct QtAddPlan
{
    const char * what = "add";
    uint64_t n = 0;        // rows of the call's range
    uint64_t entered = 0;  // rows that entered
    uint64_t nan = 0;      // rows that passed the filter and were NaN
    uint64_t held_before = 0, held = 0;
    int rc = 0;
};

static inline int qt_format_add_plan(char * buf, size_t size, const QtAddPlan & p)
{
    return snprintf(buf, size, "chgpu: quantile plan=%s n=%llu entered=%llu nan=%llu held=%llu->%llu rc=%d", p.what, (unsigned long long)p.n,
                    (unsigned long long)p.entered, (unsigned long long)p.nan, (unsigned long long)p.held_before, (unsigned long long)p.held, p.rc);
}

// what one chgpu_quantile_finalize / chgpu_quantile_for_keys did
struct QtPlan
{
    const char * what = "finalize";
    uint64_t groups = 0, values = 0;
    uint64_t small = 0, large = 0; // segments sorted in LDS / selected by radix passes
    uint64_t units = 0;            // work units of one histogram pass
    uint32_t passes = 0;           // histogram passes run (value bytes x level batches; 0 without a large segment)
    uint32_t levels = 0;
    int cached = 0;                // the groups and segments of an earlier call were reused
};

static inline int qt_format_plan(char * buf, size_t size, const QtPlan & p)
{
    return snprintf(buf, size, "chgpu: quantile plan=%s groups=%llu values=%llu small=%llu large=%llu units=%llu passes=%u levels=%u cached=%d", p.what,
                    (unsigned long long)p.groups, (unsigned long long)p.values, (unsigned long long)p.small, (unsigned long long)p.large,
                    (unsigned long long)p.units, p.passes, p.levels, p.cached);
}
