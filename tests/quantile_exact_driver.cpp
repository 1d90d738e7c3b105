// The host-only parts of the quantileExact operator (clickhouse_amd/csrc/quantile_host.h): the rank table, the level checks, the value
// keys, the windows of the small-segment kernel, the work-unit arithmetic and the plan lines.  No device, no library: built with
// -fsanitize=address,undefined and run by tests/test_quantile_exact_abi.py; prints "quantile_exact_driver OK".
#include "../clickhouse_amd/csrc/quantile_host.h"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#define REQUIRE(cond)                                                        \
    do                                                                       \
    {                                                                        \
        if (!(cond))                                                         \
        {                                                                    \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

static const int E = CHGPU_QUANTILE_EXACT, LOW = CHGPU_QUANTILE_EXACT_LOW, HIGH = CHGPU_QUANTILE_EXACT_HIGH;

static void ranks()
{
    REQUIRE(qt_rank(E, 0.29, 100) == 28); // 0.29 * 100 = 28.999999999999996
    REQUIRE(qt_rank(E, 0.57, 100) == 56);
    REQUIRE(qt_rank(E, 0.07, 100) == 7);
    const uint64_t sizes[] = {1, 2, 3, 63, 64, 65, 100, 2048, 2049, 1ull << 32, (1ull << 53) - 1, 1ull << 53, (1ull << 53) + 1};
    for (uint64_t n : sizes)
    {
        REQUIRE(qt_rank(E, 1.0, n) == n - 1);
        REQUIRE(qt_rank(E, 0.0, n) == 0);
        REQUIRE(qt_rank(LOW, 0.5, n) == ((n & 1) ? n / 2 : n / 2 - 1));
        REQUIRE(qt_rank(HIGH, 0.5, n) == n / 2);
        REQUIRE(qt_rank(E, 0.5, n) == (uint64_t)(0.5 * (double)n));
        for (int kind : {LOW, HIGH})
        {
            REQUIRE(qt_rank(kind, 0.25, n) == qt_rank(E, 0.25, n));
            REQUIRE(qt_rank(kind, 1.0, n) == n - 1 && qt_rank(kind, 0.0, n) == 0);
        }
        // the l < 1 branch stays inside the group whatever the product rounds to
        const double below_one = std::nextafter(1.0, 0.0);
        for (double l : {0.0, 1e-300, 0.07, 0.29, 0.5, 0.57, 0.99, below_one})
            for (int kind : {E, LOW, HIGH})
                REQUIRE(qt_rank(kind, l, n) < n);
    }
    REQUIRE(qt_rank(E, 0.5, 1) == 0 && qt_rank(LOW, 0.5, 2) == 0 && qt_rank(HIGH, 0.5, 2) == 1 && qt_rank(LOW, 0.5, 3) == 1);
}

static void levels()
{
    const char * msg = nullptr;
    const double ok[] = {0.0, 0.5, 1.0}, low[] = {-0.1}, high[] = {0.5, 1.5}, nan[] = {std::numeric_limits<double>::quiet_NaN()};
    std::vector<double> many(CHGPU_QUANTILE_MAX_LEVELS + 1, 0.5);
    REQUIRE(qt_check_levels(E, 3, ok, &msg) == CHGPU_OK);
    REQUIRE(qt_check_levels(HIGH, CHGPU_QUANTILE_MAX_LEVELS, many.data(), &msg) == CHGPU_OK);
    REQUIRE(qt_check_levels(E, CHGPU_QUANTILE_MAX_LEVELS + 1, many.data(), &msg) == CHGPU_ERR_BAD_ARGUMENTS);
    REQUIRE(qt_check_levels(E, 0, ok, &msg) == CHGPU_ERR_BAD_ARGUMENTS);
    REQUIRE(qt_check_levels(E, 1, nullptr, &msg) == CHGPU_ERR_BAD_ARGUMENTS && std::strstr(msg, "NULL"));
    REQUIRE(qt_check_levels(E, 1, low, &msg) == CHGPU_ERR_BAD_ARGUMENTS && std::strstr(msg, "level"));
    REQUIRE(qt_check_levels(LOW, 2, high, &msg) == CHGPU_ERR_BAD_ARGUMENTS);
    REQUIRE(qt_check_levels(E, 1, nan, &msg) == CHGPU_ERR_BAD_ARGUMENTS);
    for (int kind : {CHGPU_QUANTILE_EXACT_INCLUSIVE, CHGPU_QUANTILE_EXACT_EXCLUSIVE, CHGPU_QUANTILE_EXACT_WEIGHTED})
        REQUIRE(qt_check_levels(kind, 3, ok, &msg) == CHGPU_ERR_NOT_IMPLEMENTED);
    REQUIRE(qt_check_levels(-1, 3, ok, &msg) == CHGPU_ERR_BAD_ARGUMENTS && qt_check_levels(6, 3, ok, &msg) == CHGPU_ERR_BAD_ARGUMENTS);
    REQUIRE(pair_check_rows(10, 10, 10, 0, 10, &msg) == CHGPU_OK && pair_check_rows(-1, 10, -1, 3, 3, &msg) == CHGPU_OK);
    REQUIRE(pair_check_rows(9, 10, -1, 0, 9, &msg) == CHGPU_ERR_SIZES_MISMATCH && pair_check_rows(10, 10, 11, 0, 9, &msg) == CHGPU_ERR_SIZES_MISMATCH);
    REQUIRE(pair_check_rows(10, 10, -1, 6, 5, &msg) == CHGPU_ERR_BAD_ARGUMENTS && pair_check_rows(10, 10, -1, 0, 11, &msg) == CHGPU_ERR_BAD_ARGUMENTS);
}

// the keys are a bijection on the width's bits and keep the value's order
static void value_keys()
{
    for (uint32_t width : {1u, 2u, 4u, 8u})
        for (int mode : {QT_MODE_UNSIGNED, QT_MODE_SIGNED, QT_MODE_FLOAT})
        {
            if (mode == QT_MODE_FLOAT && width < 4)
                continue;
            const uint64_t mask = qt_width_mask(width), top = 1ull << (8 * width - 1);
            for (uint64_t b : std::vector<uint64_t>{0, 1, top - 1, top, top + 1, mask - 1, mask, 0x3FF0000000000000ull & mask, 0x7FF0000000000000ull & mask})
            {
                const uint64_t k = qt_encode(b, width, mode);
                REQUIRE((k & ~mask) == 0 && qt_decode(k, width, mode) == b);
            }
        }
    REQUIRE(qt_encode(0x80, 1, QT_MODE_SIGNED) == 0 && qt_encode(0x7F, 1, QT_MODE_SIGNED) == 0xFF); // Int8 min, max
    REQUIRE(qt_encode(1ull << 63, 8, QT_MODE_UNSIGNED) == 1ull << 63);
    // doubles in ascending order, -0.0 directly before +0.0
    const double order[] = {-INFINITY, -1.5, -4.9e-324, -0.0, 0.0, 4.9e-324, 1.5, INFINITY};
    uint64_t prev = 0;
    for (size_t i = 0; i < sizeof(order) / sizeof(order[0]); ++i)
    {
        uint64_t b;
        std::memcpy(&b, &order[i], 8);
        const uint64_t k = qt_encode(b, 8, QT_MODE_FLOAT);
        REQUIRE(i == 0 || k > prev);
        prev = k;
    }
    uint64_t neg0, pos0;
    const double nz = -0.0, pz = 0.0;
    std::memcpy(&neg0, &nz, 8);
    std::memcpy(&pos0, &pz, 8);
    REQUIRE(qt_encode(neg0, 8, QT_MODE_FLOAT) + 1 == qt_encode(pos0, 8, QT_MODE_FLOAT));
    REQUIRE(qt_is_nan(0x7FF8000000000000ull, 8) && qt_is_nan(0xFFF0000000000001ull, 8) && !qt_is_nan(0x7FF0000000000000ull, 8) && !qt_is_nan(0xFFF0000000000000ull, 8));
    REQUIRE(qt_is_nan(0x7FC00000ull, 4) && qt_is_nan(0xFF800001ull, 4) && !qt_is_nan(0x7F800000ull, 4) && !qt_is_nan(0, 4));
    REQUIRE(qt_empty_bits(8, QT_MODE_FLOAT) == 0x7FF8000000000000ull && qt_empty_bits(4, QT_MODE_FLOAT) == 0x7FC00000ull && qt_empty_bits(8, QT_MODE_SIGNED) == 0);
}

// Every small segment belongs to exactly one window; a window's small segments lie inside one tile from its first segment's start; a
// large segment can only be a window's last.
static void windows_of(const std::vector<uint64_t> & counts)
{
    std::vector<uint64_t> offsets(counts.size() + 1, 0);
    for (size_t g = 0; g < counts.size(); ++g)
        offsets[g + 1] = offsets[g] + counts[g];
    const uint64_t groups = counts.size(), values = offsets.back();
    std::vector<int> owned(groups, 0);
    uint64_t next = 0;
    for (uint64_t w = 0; w < qt_windows(values); ++w)
    {
        uint64_t g0 = 0, g1 = 0;
        qt_window_groups(offsets.data(), groups, w, &g0, &g1);
        REQUIRE(g0 == next && g0 <= g1 && g1 <= groups); // consecutive runs, in order
        next = g1;
        REQUIRE(g1 - g0 <= QT_WINDOW);
        for (uint64_t g = g0; g < g1; ++g)
        {
            owned[g] += 1;
            REQUIRE(offsets[g] >= w * QT_WINDOW && offsets[g] < (w + 1) * QT_WINDOW);
            if (qt_is_small(counts[g]))
                REQUIRE(offsets[g + 1] - offsets[g0] <= QT_TILE);
            else
                REQUIRE(g + 1 == g1);
        }
    }
    REQUIRE(next == groups);
    for (int o : owned)
        REQUIRE(o == 1);
}

static void tile_packing()
{
    windows_of({});
    windows_of({1});
    windows_of(std::vector<uint64_t>(3 * QT_WINDOW + 5, 1)); // all ones
    windows_of({QT_SMALL_MAX});
    windows_of({QT_SMALL_MAX, QT_SMALL_MAX, QT_SMALL_MAX});
    std::vector<uint64_t> alternating;
    for (int i = 0; i < 40; ++i)
        alternating.push_back(i % 2 ? QT_SMALL_MAX : 1);
    windows_of(alternating);
    windows_of({QT_WINDOW - 1, QT_SMALL_MAX, 1, QT_SMALL_MAX + 1, 1, 1, 3 * QT_CHUNK + 1, 2, QT_SMALL_MAX - 1, 63, 64, 65});
    std::vector<uint64_t> threes(100000, 3);
    threes.push_back(1);
    windows_of(threes);
    const uint64_t off[] = {0, 5, 9, 9 + QT_WINDOW};
    REQUIRE(qt_lower_bound(off, 3, 0) == 0 && qt_lower_bound(off, 3, 1) == 1 && qt_lower_bound(off, 3, 9) == 2 && qt_lower_bound(off, 3, 10) == 3);
}

static void units()
{
    REQUIRE(qt_is_small(1) && qt_is_small(QT_SMALL_MAX) && !qt_is_small(QT_SMALL_MAX + 1));
    REQUIRE(qt_units(0) == 0 && qt_units(QT_SMALL_MAX) == 0 && qt_units(QT_SMALL_MAX + 1) == 1);
    REQUIRE(qt_units(QT_CHUNK - 1) == 1 && qt_units(QT_CHUNK) == 1 && qt_units(QT_CHUNK + 1) == 2 && qt_units(3 * QT_CHUNK + 1) == 4);
    REQUIRE(qt_units(QT_MAX_VALUES) == (QT_MAX_VALUES + QT_CHUNK - 1) / QT_CHUNK);
    REQUIRE(qt_windows(0) == 0 && qt_windows(1) == 1 && qt_windows(QT_WINDOW) == 1 && qt_windows(QT_WINDOW + 1) == 2);
    REQUIRE(qt_level_batch(0, 16) == 16 && qt_level_batch(1, 16) == 16 && qt_level_batch(1, 1) == 1);
    REQUIRE(qt_level_batch(QT_HIST_BUDGET / 1024 / 16, 16) == 16 && qt_level_batch(QT_HIST_BUDGET / 1024 / 16 + 1, 16) == 15);
    REQUIRE(qt_level_batch(QT_HIST_BUDGET / 1024, 16) == 1 && qt_level_batch(QT_MAX_VALUES / QT_SMALL_MAX, 16) == 1);
    // a lowered budget (the test option): 5 segments x 3 levels fit 16 KiB, the 16 levels run as 3 + 3 + ... + 1
    REQUIRE(qt_level_batch(5, 16, 16 * 1024) == 3 && qt_level_batch(5, 2, 16 * 1024) == 2 && qt_level_batch(5, 16, 1) == 1 && qt_level_batch(0, 16, 1) == 16);
    REQUIRE(qt_capacity_for(0) == 4096 && qt_capacity_for(4096) == 4096 && qt_capacity_for(4097) == 8192 && qt_capacity_for(QT_MAX_VALUES) == 1ull << 32);
}

static void plan_lines()
{
    char line[256];
    QtAddPlan a;
    a.n = 5000;
    a.entered = 4000;
    a.nan = 7;
    a.held_before = 10;
    a.held = 4010;
    int len = qt_format_add_plan(line, sizeof(line), a);
    REQUIRE(len > 0 && (size_t)len < sizeof(line));
    REQUIRE(std::string(line) == "chgpu: quantile plan=add n=5000 entered=4000 nan=7 held=10->4010 rc=0");
    QtPlan p;
    p.groups = 12;
    p.values = 99999;
    p.small = 8;
    p.large = 4;
    p.units = 9;
    p.passes = 8;
    p.levels = 3;
    p.cached = 1;
    len = qt_format_plan(line, sizeof(line), p);
    REQUIRE(len > 0 && (size_t)len < sizeof(line));
    REQUIRE(std::string(line) == "chgpu: quantile plan=finalize groups=12 values=99999 small=8 large=4 units=9 passes=8 levels=3 cached=1");
    // the widest values still fit the callers' buffers, and a short buffer is cut, terminated and never overrun
    p.what = "for_keys";
    p.groups = p.values = p.small = p.large = p.units = ~0ull;
    p.passes = p.levels = ~0u;
    REQUIRE((size_t)qt_format_plan(line, sizeof(line), p) < sizeof(line));
    a.what = "merge";
    a.n = a.entered = a.nan = a.held_before = a.held = ~0ull;
    a.rc = -7;
    REQUIRE((size_t)qt_format_add_plan(line, sizeof(line), a) < sizeof(line));
    std::vector<char> small(16, 'x');
    const int full = qt_format_plan(small.data(), small.size(), p);
    REQUIRE((size_t)full > small.size() && small[15] == '\0' && std::strlen(small.data()) == 15);
}

int main()
{
    ranks();
    levels();
    value_keys();
    tile_packing();
    units();
    plan_lines();
    std::printf("quantile_exact_driver OK\n");
    return 0;
}
