// window_frames_driver.cpp — the host-only parts of chgpu_window_evaluate_framed (clickhouse_amd/csrc/window_frames_host.h) as a
// stand-alone program, built with -fsanitize=address,undefined by tests/test_window_frames_abi.py: the search behind a RANGE offset against
// a linear scan in 128-bit arithmetic (all eight types, both directions, values at the types' limits, unsorted data), a host restatement
// of the block masks plus the query arithmetic of the general min / max against brute force, the level count, and which frames and plans
// the framed entry accepts: the one frame check and the one plan of window_host.h, asked as the framed entry and as the old one, with
// the order of their refusals.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../clickhouse_amd/csrc/window_frames_host.h"

#define CHECK(cond)                                                         \
    do                                                                      \
    {                                                                       \
        if (!(cond))                                                        \
        {                                                                   \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

typedef __int128 wide;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static chgpu_window_frame frame_of(int type, int b, uint64_t bo, int e, uint64_t eo)
{
    chgpu_window_frame f{};
    f.type = type;
    f.begin_kind = b;
    f.end_kind = e;
    f.begin_offset = bo;
    f.end_offset = eo;
    return f;
}

// ---------------------------------------------------------------------------------------------
// the search
// ---------------------------------------------------------------------------------------------
// the contract's table by a linear scan: first j in [ps, pe) with y[j] >= t (end: > t), else pe; y = x, negated when descending
template <typename X>
static uint64_t bound_by_scan(const std::vector<X> & x, uint64_t i, uint64_t ps, uint64_t pe, bool following, bool end, bool descending, uint64_t k)
{
    const wide sign = descending ? -1 : 1;
    const wide t = sign * (wide)x[i] + (following ? (wide)k : -(wide)k);
    for (uint64_t j = ps; j < pe; ++j)
    {
        const wide y = sign * (wide)x[j];
        if (end ? y > t : y >= t)
            return j;
    }
    return pe;
}

template <typename X>
static void check_partition(const std::vector<X> & x, uint64_t ps, uint64_t pe, bool descending, bool sorted, uint64_t * checked)
{
    const uint64_t offsets[] = {1, 2, 3, 100, 1ull << 63, ~0ull};
    std::vector<uint64_t> rows_checked; // every row of a short partition; of a long one a few, its first and last among them
    for (uint64_t i = ps; i < pe; i += pe - ps > 200 ? 211 : 1)
        rows_checked.push_back(i);
    rows_checked.push_back(pe - 1);
    for (uint64_t k : offsets)
        for (int following = 0; following < 2; ++following)
            for (int end = 0; end < 2; ++end)
                for (uint64_t i : rows_checked)
                {
                    const uint64_t got = win_range_bound_of(x.data(), i, ps, pe, following != 0, end != 0, descending, k);
                    CHECK(got >= ps && got <= pe);                       // whatever the data
                    CHECK(following ? got > i : got <= i);
                    if (sorted)
                        CHECK(got == bound_by_scan(x, i, ps, pe, following != 0, end != 0, descending, k));
                    *checked += 1;
                }
}

template <typename X>
static void test_search_of_type()
{
    const X lo = std::numeric_limits<X>::min(), hi = std::numeric_limits<X>::max();
    const uint64_t lengths[] = {1, 2, 63, 64, 65, 5000};
    uint64_t checked = 0;
    for (int descending = 0; descending < 2; ++descending)
        for (uint64_t len : lengths)
            for (int shape = 0; shape < 4; ++shape)
            {
                // the partition sits inside a longer column, with rows of other partitions (far values) on both sides
                const uint64_t ps = 3, pe = ps + len;
                std::vector<X> x(pe + 2, shape % 2 ? lo : hi);
                // shape 0: from the minimum in small steps with duplicates; 1: up to the maximum; 2: the minimum, then the maximum;
                // 3: unit steps around the middle
                std::vector<wide> v(len);
                wide cur = 0;
                for (uint64_t j = 0; j < len; ++j)
                {
                    cur += shape == 3 ? 1 : (wide)(rnd() % 4 == 0 ? rnd() % 9 : rnd() % 2);
                    v[j] = cur;
                }
                const wide span = (wide)hi - (wide)lo;
                for (uint64_t j = 0; j < len; ++j)
                {
                    wide val;
                    if (shape == 0)
                        val = (wide)lo + (v[j] > span ? span : v[j]);
                    else if (shape == 1)
                        val = (wide)hi - (v[len - 1] - v[j] > span ? span : v[len - 1] - v[j]);
                    else if (shape == 2)
                        val = j < len / 2 ? (wide)lo : (wide)hi;
                    else
                        val = (wide)lo + span / 2 + (v[j] > span / 2 ? span / 2 : v[j]);
                    x[ps + (descending ? len - 1 - j : j)] = (X)val;
                }
                check_partition(x, ps, pe, descending != 0, true, &checked);
                // unsorted: the answers mean nothing, but the search ends and stays inside the partition
                for (uint64_t j = ps; j < pe; ++j)
                    x[j] = (X)rnd();
                check_partition(x, ps, pe, descending != 0, false, &checked);
            }
    CHECK(checked > 10000);
}

static void test_search()
{
    test_search_of_type<int64_t>();
    test_search_of_type<uint64_t>();
    test_search_of_type<int32_t>();
    test_search_of_type<uint32_t>();
    test_search_of_type<int16_t>();
    test_search_of_type<uint16_t>();
    test_search_of_type<int8_t>();
    test_search_of_type<uint8_t>();
    // offset 0 never reaches the search: it becomes CURRENT ROW, whose bounds are the peer group's
    const int OP = CHGPU_BOUND_OFFSET_PRECEDING, OF = CHGPU_BOUND_OFFSET_FOLLOWING, CR = CHGPU_BOUND_CURRENT_ROW;
    chgpu_window_frame f = win_frame_without_zero_range_offsets(frame_of(CHGPU_FRAME_RANGE, OP, 0, OF, 0));
    CHECK(f.begin_kind == CR && f.end_kind == CR && f.type == CHGPU_FRAME_RANGE);
    f = win_frame_without_zero_range_offsets(frame_of(CHGPU_FRAME_RANGE, OP, 5, OP, 0));
    CHECK(f.begin_kind == OP && f.begin_offset == 5 && f.end_kind == CR);
    f = win_frame_without_zero_range_offsets(frame_of(CHGPU_FRAME_RANGE, OF, 0, OF, 1ull << 63));
    CHECK(f.begin_kind == CR && f.end_kind == OF && f.end_offset == 1ull << 63);
    f = win_frame_without_zero_range_offsets(frame_of(CHGPU_FRAME_ROWS, OP, 0, OF, 0)); // ROWS: untouched
    CHECK(f.begin_kind == OP && f.end_kind == OF);
    // and a hand-made case at the limits: Int8 -128, -1, 0, 127 with 200 and 255 PRECEDING / FOLLOWING
    const std::vector<int8_t> x = {-128, -1, 0, 127};
    CHECK(win_range_bound_of(x.data(), 3, 0, 4, false, false, false, 200) == 1);  // 127 - 200 = -73: -1 is the first row >= it
    CHECK(win_range_bound_of(x.data(), 3, 0, 4, false, false, false, 255) == 0);  // -128 itself
    CHECK(win_range_bound_of(x.data(), 0, 0, 4, false, false, false, ~0ull) == 0);
    CHECK(win_range_bound_of(x.data(), 0, 0, 4, true, true, false, 200) == 3);    // -128 + 200 = 72: 127 is the first row above it
    CHECK(win_range_bound_of(x.data(), 1, 0, 4, true, true, false, 200) == 4);    // -1 + 200 leaves Int8: no row is above it
    CHECK(win_range_bound_of(x.data(), 0, 0, 4, true, false, false, 255) == 3);   // first row >= 127
}

// ---------------------------------------------------------------------------------------------
// the general extremum
// ---------------------------------------------------------------------------------------------
// the kernels' structure restated on the host: masks by the definition, level 0 per block, the levels above by the doubling rule
struct ExtStructure
{
    uint64_t n = 0, n_blocks = 0;
    uint32_t levels = 0;
    std::vector<uint64_t> key, mask, table;
};

static ExtStructure ext_build(const std::vector<uint64_t> & keys, uint64_t width)
{
    ExtStructure s;
    s.n = keys.size();
    s.n_blocks = win_ext_blocks(s.n);
    s.levels = win_ext_levels(width, s.n_blocks);
    s.key = keys;
    s.key.resize(s.n_blocks * WIN_EXT_BLOCK, 0); // rows past the input: the worst key
    s.mask.assign(s.n_blocks * WIN_EXT_BLOCK, 0);
    s.table.assign(s.n_blocks * (s.levels ? s.levels : 1), 0);
    for (uint64_t b = 0; b < s.n_blocks; ++b)
    {
        uint64_t top = 0;
        uint64_t m = 0;
        for (uint64_t r = 0; r < WIN_EXT_BLOCK; ++r)
        {
            // bit p stays while no row q in (p, r] has key[q] >= key[p]: row r ends every p <= its key, and stands itself
            for (uint64_t p = 0; p < r; ++p)
                if (s.key[b * WIN_EXT_BLOCK + r] >= s.key[b * WIN_EXT_BLOCK + p])
                    m &= ~((uint64_t)1 << p);
            m |= (uint64_t)1 << r;
            s.mask[b * WIN_EXT_BLOCK + r] = m;
            top = s.key[b * WIN_EXT_BLOCK + r] > top ? s.key[b * WIN_EXT_BLOCK + r] : top;
        }
        s.table[b] = top;
    }
    for (uint32_t j = 1; j < s.levels; ++j)
        for (uint64_t b = 0; b < s.n_blocks; ++b)
        {
            const uint64_t half = (uint64_t)1 << (j - 1), a = s.table[(j - 1) * s.n_blocks + b];
            s.table[j * s.n_blocks + b] = b + half < s.n_blocks && s.table[(j - 1) * s.n_blocks + b + half] > a ? s.table[(j - 1) * s.n_blocks + b + half] : a;
        }
    return s;
}

// the output kernel's query, with every index checked
static uint64_t ext_query(const ExtStructure & s, uint64_t l, uint64_t last)
{
    CHECK(l <= last && last < s.n);
    const uint64_t bl = l / WIN_EXT_BLOCK, br = last / WIN_EXT_BLOCK;
    if (bl == br)
    {
        const uint64_t at = win_ext_in_block(s.mask[last], l);
        CHECK(at >= l && at <= last);
        return s.key[at];
    }
    const uint64_t a0 = win_ext_in_block(s.mask[bl * WIN_EXT_BLOCK + WIN_EXT_BLOCK - 1], l), a1 = win_ext_in_block(s.mask[last], br * WIN_EXT_BLOCK);
    CHECK(a0 >= l && a0 < (bl + 1) * WIN_EXT_BLOCK && a1 >= br * WIN_EXT_BLOCK && a1 <= last);
    uint64_t best = s.key[a0] > s.key[a1] ? s.key[a0] : s.key[a1];
    if (br - bl > 1)
    {
        uint32_t level = 0;
        uint64_t c0 = 0, c1 = 0;
        win_ext_cells(bl, br, &level, &c0, &c1);
        CHECK(level < s.levels);
        CHECK(c0 == bl + 1 && c1 >= c0 && c1 + ((uint64_t)1 << level) == br && c0 + ((uint64_t)1 << level) >= c1);
        CHECK(level * s.n_blocks + c1 < s.table.size());
        for (uint64_t c : {c0, c1})
            best = s.table[level * s.n_blocks + c] > best ? s.table[level * s.n_blocks + c] : best;
    }
    return best;
}

static void test_extremum_structure()
{
    const uint64_t sizes[] = {1, 63, 64, 65, 129, 4161};
    uint64_t checked = 0;
    for (uint64_t n : sizes)
        for (int shape = 0; shape < 4; ++shape)
        {
            std::vector<uint64_t> keys(n);
            for (uint64_t i = 0; i < n; ++i)
                keys[i] = shape == 0 ? rnd() % 3 : shape == 1 ? i + 1 : shape == 2 ? n - i : rnd(); // {0, 1, 2}; rising; falling; random
            const ExtStructure s = ext_build(keys, ~0ull);
            // rising: a stack of one row; falling: of every row so far
            if (shape == 1)
                CHECK(s.mask[n - 1] == (uint64_t)1 << ((n - 1) % WIN_EXT_BLOCK));
            if (shape == 2)
                CHECK(s.mask[n - 1] == (((n - 1) % WIN_EXT_BLOCK) == 63 ? ~0ull : ((uint64_t)2 << ((n - 1) % WIN_EXT_BLOCK)) - 1));
            const uint64_t l_stride = n > 200 ? 61 : 1;
            for (uint64_t l = 0; l < n; l += l_stride)
            {
                uint64_t want = 0;
                for (uint64_t last = l; last < n; ++last)
                {
                    want = keys[last] > want ? keys[last] : want;
                    if (n > 200 && (last - l) % 7 != 0 && last - l > 130 && last != n - 1)
                        continue;
                    CHECK(ext_query(s, l, last) == want);
                    checked += 1;
                }
            }
            // a structure built for narrow frames answers them with fewer levels
            for (uint64_t width : {(uint64_t)1, (uint64_t)64, (uint64_t)65, (uint64_t)130, (uint64_t)1000})
            {
                const ExtStructure narrow = ext_build(keys, width);
                CHECK(narrow.levels <= s.levels);
                for (uint64_t l = 0; l < n; l += 13)
                {
                    const uint64_t last = l + width - 1 < n ? l + width - 1 : n - 1;
                    uint64_t want = 0;
                    for (uint64_t j = l; j <= last; ++j)
                        want = keys[j] > want ? keys[j] : want;
                    CHECK(ext_query(narrow, l, last) == want);
                    checked += 1;
                }
            }
        }
    CHECK(checked > 100000);
    // levels: a frame of `width` rows has at most (width - 2) / 64 whole blocks between its first and its last block
    const uint64_t many = 1ull << 26;
    CHECK(win_ext_levels(1, many) == 0 && win_ext_levels(64, many) == 0 && win_ext_levels(65, many) == 0);
    CHECK(win_ext_levels(66, many) == 1 && win_ext_levels(128, many) == 1 && win_ext_levels(129, many) == 1 && win_ext_levels(130, many) == 2);
    CHECK(win_ext_levels(1ull << 32, many) == 26);                      // 2^26 - 1 blocks between: levels 0 .. 25
    CHECK(win_ext_levels(~0ull, many) == 26 && win_ext_levels(~0ull, 1) == 0 && win_ext_levels(~0ull, 2) == 0 && win_ext_levels(~0ull, 3) == 1);
    CHECK(win_ext_levels(~0ull, 4) == 2 && win_ext_levels(~0ull, 2049) == 11 && win_ext_levels(1000, 3) == 1);
    CHECK(win_ext_blocks(0) == 0 && win_ext_blocks(1) == 1 && win_ext_blocks(64) == 1 && win_ext_blocks(65) == 2 && win_ext_blocks(WIN_MAX_ROWS) == 1ull << 26);
    // the table stays within 8 B * blocks * ceil(log2(blocks))
    for (uint64_t nb = 2; nb < 5000; ++nb)
    {
        uint32_t ceil_log = 0;
        while (((uint64_t)1 << ceil_log) < nb)
            ceil_log += 1;
        CHECK(win_ext_levels(~0ull, nb) <= ceil_log);
    }
    CHECK(win_log2_floor(1) == 0 && win_log2_floor(2) == 1 && win_log2_floor(3) == 1 && win_log2_floor(1ull << 63) == 63 && win_ctz64(1ull << 63) == 63);
}

// ---------------------------------------------------------------------------------------------
// frames and plans
// ---------------------------------------------------------------------------------------------
static void test_frames_and_plans()
{
    const int UP = CHGPU_BOUND_UNBOUNDED_PRECEDING, OP = CHGPU_BOUND_OFFSET_PRECEDING, CR = CHGPU_BOUND_CURRENT_ROW, OF = CHGPU_BOUND_OFFSET_FOLLOWING,
              UF = CHGPU_BOUND_UNBOUNDED_FOLLOWING;
    // every pair of bounds: the one check answers the same for both entries, except that a legal RANGE offset passes where the entry serves it
    for (int type = 0; type < 2; ++type)
        for (int b = UP; b <= UF; ++b)
            for (int e = UP; e <= UF; ++e)
            {
                const char * msg = nullptr, * old_msg = nullptr;
                const chgpu_window_frame f = frame_of(type, b, 3, e, 3);
                const int rc = win_check_frame(f, true, &msg), old = win_check_frame(f, false, &old_msg);
                CHECK(rc == (old == CHGPU_ERR_NOT_IMPLEMENTED ? CHGPU_OK : old));
                CHECK((old == CHGPU_ERR_NOT_IMPLEMENTED) == (rc == CHGPU_OK && win_frame_has_range_offset(f)));
                CHECK((rc == CHGPU_OK) == (msg == nullptr) && (old == CHGPU_OK) == (old_msg == nullptr));
            }
    const char * msg = nullptr;
    CHECK(win_check_frame(frame_of(CHGPU_FRAME_RANGE, OP, 1, OP, 2), true, &msg) == CHGPU_ERR_BAD_ARGUMENTS);
    CHECK(win_check_frame(frame_of(CHGPU_FRAME_RANGE, OF, 2, OF, 1), true, &msg) == CHGPU_ERR_BAD_ARGUMENTS);
    CHECK(win_check_frame(frame_of(CHGPU_FRAME_RANGE, OP, 2, OP, 1), true, &msg) == CHGPU_OK);
    CHECK(win_check_frame(frame_of(2, OP, 2, OP, 1), true, &msg) == CHGPU_ERR_BAD_ARGUMENTS);

    const chgpu_window_frame dflt = win_default_frame();
    const chgpu_window_frame whole = frame_of(CHGPU_FRAME_ROWS, UP, 0, UF, 0);
    const chgpu_window_frame ahead = frame_of(CHGPU_FRAME_ROWS, CR, 0, UF, 0);
    const chgpu_window_frame around = frame_of(CHGPU_FRAME_ROWS, OP, 1000, OF, 1000);
    const chgpu_window_frame before = frame_of(CHGPU_FRAME_ROWS, OP, 5, OP, 2);
    const chgpu_window_frame peers = frame_of(CHGPU_FRAME_RANGE, CR, 0, CR, 0);
    const chgpu_window_frame week = frame_of(CHGPU_FRAME_RANGE, OP, 604800, CR, 0);
    const chgpu_window_frame band = frame_of(CHGPU_FRAME_RANGE, OP, 10, OF, 0);
    const chgpu_window_frame tail = frame_of(CHGPU_FRAME_RANGE, OF, 3, UF, 0);
    WinPlan plan;
    std::string why;
    // the framed entry on a handle that recorded the very order column given (or any handle, where none is given)
    const auto framed = [&](int function, const chgpu_window_frame & frame, int arg_type, int order_type) {
        return win_plan(true, function, frame, arg_type, order_type, 1, order_type, &plan, &why);
    };
    // `plan` is, field for field, what chgpu_window_evaluate plans for the call
    const auto same_as_unframed = [&](int function, const chgpu_window_frame & frame, int arg_type) {
        WinPlan old;
        std::string old_why;
        return win_plan(false, function, frame, arg_type, -1, 1, -1, &old, &old_why) == CHGPU_OK && old.needs == plan.needs && old.ext == plan.ext
            && old.search_begin == plan.search_begin && old.search_end == plan.search_end && old.width == plan.width;
    };
    const auto unframed_refuses = [&](int function, const chgpu_window_frame & frame, int arg_type) {
        WinPlan old;
        std::string old_why;
        const char * m = nullptr;
        return win_check_frame(frame, false, &m) == CHGPU_ERR_NOT_IMPLEMENTED || win_plan(false, function, frame, arg_type, -1, 1, -1, &old, &old_why) == CHGPU_ERR_NOT_IMPLEMENTED;
    };
    // what the old entry serves gets the old entry's plan
    CHECK(framed(CHGPU_WIN_RANK, dflt, -1, -1) == CHGPU_OK && same_as_unframed(CHGPU_WIN_RANK, dflt, -1) && plan.needs == (WIN_B_PS | WIN_B_GS));
    CHECK(framed(CHGPU_WIN_SUM, around, CHGPU_I32, -1) == CHGPU_OK && same_as_unframed(CHGPU_WIN_SUM, around, CHGPU_I32) && plan.needs == (WIN_B_PS | WIN_B_PE));
    CHECK(framed(CHGPU_WIN_MAX, whole, CHGPU_F64, -1) == CHGPU_OK && same_as_unframed(CHGPU_WIN_MAX, whole, CHGPU_F64) && plan.ext == WIN_EXT_FORWARD);
    CHECK(framed(CHGPU_WIN_MIN, ahead, CHGPU_F32, -1) == CHGPU_OK && same_as_unframed(CHGPU_WIN_MIN, ahead, CHGPU_F32) && plan.ext == WIN_EXT_BACKWARD && plan.needs == WIN_B_PE);
    // (a) min / max over a frame bounded on both sides
    CHECK(framed(CHGPU_WIN_MAX, around, CHGPU_I64, -1) == CHGPU_OK && unframed_refuses(CHGPU_WIN_MAX, around, CHGPU_I64) && plan.ext == WIN_EXT_GENERAL);
    CHECK(plan.width == 2001 && plan.needs == (WIN_B_PS | WIN_B_PE) && !plan.search_begin && !plan.search_end);
    CHECK(framed(CHGPU_WIN_MIN, before, CHGPU_F32, -1) == CHGPU_OK && plan.ext == WIN_EXT_GENERAL && plan.width == 4 && plan.needs == WIN_B_PS);
    CHECK(framed(CHGPU_WIN_MIN, peers, CHGPU_U8, -1) == CHGPU_OK && plan.ext == WIN_EXT_GENERAL && plan.width == ~0ull);
    CHECK(plan.needs == (WIN_B_GS | WIN_B_GE));
    CHECK(win_frame_max_width(frame_of(CHGPU_FRAME_ROWS, OP, ~0ull, OF, ~0ull)) == ~0ull && win_frame_max_width(frame_of(CHGPU_FRAME_ROWS, CR, 0, CR, 0)) == 1);
    CHECK(win_frame_max_width(frame_of(CHGPU_FRAME_ROWS, OF, 2, OF, 9)) == 8 && win_frame_max_width(frame_of(CHGPU_FRAME_ROWS, OP, 3, CR, 0)) == 4);
    // (b) RANGE offsets: every function that reads a frame, all eight order types
    const int order_types[] = {CHGPU_I64, CHGPU_U64, CHGPU_I32, CHGPU_U32, CHGPU_I16, CHGPU_U16, CHGPU_I8, CHGPU_U8};
    for (int ot : order_types)
        for (int fn = CHGPU_WIN_COUNT; fn <= CHGPU_WIN_LEAD_IN_FRAME; ++fn)
        {
            CHECK(framed(fn, week, fn == CHGPU_WIN_COUNT ? -1 : CHGPU_I64, ot) == CHGPU_OK);
            CHECK(unframed_refuses(fn, week, fn == CHGPU_WIN_COUNT ? -1 : CHGPU_I64) && plan.search_begin && !plan.search_end && plan.needs == (WIN_B_PS | WIN_B_GE));
            CHECK(plan.ext == (fn == CHGPU_WIN_MIN || fn == CHGPU_WIN_MAX ? WIN_EXT_GENERAL : WIN_EXT_NONE));
        }
    CHECK(framed(CHGPU_WIN_SUM, band, CHGPU_U16, CHGPU_I64) == CHGPU_OK && plan.search_begin && !plan.search_end); // 0 FOLLOWING: ge
    CHECK(plan.needs == (WIN_B_PS | WIN_B_GE));
    CHECK(framed(CHGPU_WIN_MAX, tail, CHGPU_F64, CHGPU_U8) == CHGPU_OK && plan.ext == WIN_EXT_GENERAL && plan.search_begin && plan.needs == WIN_B_PE);
    CHECK(plan.width == ~0ull);
    // the refusals and their codes
    CHECK(framed(CHGPU_WIN_SUM, week, CHGPU_I64, -1) == CHGPU_ERR_BAD_ARGUMENTS);          // no order column
    CHECK(framed(CHGPU_WIN_SUM, around, CHGPU_I64, CHGPU_I64) == CHGPU_ERR_BAD_ARGUMENTS); // a surplus one
    CHECK(framed(CHGPU_WIN_RANK, week, -1, CHGPU_I64) == CHGPU_ERR_BAD_ARGUMENTS);         // rank ignores the frame
    CHECK(framed(CHGPU_WIN_RANK, week, -1, -1) == CHGPU_OK && same_as_unframed(CHGPU_WIN_RANK, week, -1));
    CHECK(framed(CHGPU_WIN_SUM, week, CHGPU_I64, CHGPU_F64) == CHGPU_ERR_NOT_IMPLEMENTED);
    CHECK(framed(CHGPU_WIN_COUNT, week, -1, CHGPU_F32) == CHGPU_ERR_NOT_IMPLEMENTED);
    CHECK(framed(CHGPU_WIN_SUM, week, CHGPU_F64, CHGPU_I64) == CHGPU_ERR_NOT_IMPLEMENTED); // float sums stay out
    CHECK(framed(CHGPU_WIN_AVG, around, CHGPU_F32, -1) == CHGPU_ERR_NOT_IMPLEMENTED);
    CHECK(framed(CHGPU_WIN_SUM, week, -1, CHGPU_I64) == CHGPU_ERR_BAD_ARGUMENTS);          // no argument
    CHECK(framed(CHGPU_WIN_COUNT, week, CHGPU_I64, CHGPU_I64) == CHGPU_ERR_BAD_ARGUMENTS); // a surplus one
    CHECK(framed(CHGPU_WIN_MAX, around, -1, -1) == CHGPU_ERR_BAD_ARGUMENTS);
    CHECK(framed(12, around, CHGPU_I64, -1) == CHGPU_ERR_BAD_ARGUMENTS);
    CHECK(framed(-1, week, CHGPU_I64, CHGPU_I64) == CHGPU_ERR_BAD_ARGUMENTS);

    // what the handle recorded at create comes before what is not implemented: (ORDER BY columns, type of the first) of three handles
    // that cannot take an Int64 order column, and of the three that cannot take a Float64 one
    const auto on_handle = [&](int function, int arg_type, int order_type, uint32_t n_order, int recorded) {
        return win_plan(true, function, week, arg_type, order_type, n_order, recorded, &plan, &why);
    };
    struct Handle { uint32_t n_order; int recorded; };
    for (const Handle & h : {Handle{0, -1}, Handle{2, CHGPU_I64}, Handle{1, CHGPU_I32}})
    {
        CHECK(on_handle(CHGPU_WIN_SUM, CHGPU_I64, CHGPU_I64, h.n_order, h.recorded) == CHGPU_ERR_BAD_ARGUMENTS);
        CHECK(on_handle(CHGPU_WIN_SUM, CHGPU_F64, CHGPU_I64, h.n_order, h.recorded) == CHGPU_ERR_BAD_ARGUMENTS); // a float sum as well
        CHECK(on_handle(CHGPU_WIN_SUM, -1, CHGPU_I64, h.n_order, h.recorded) == CHGPU_ERR_BAD_ARGUMENTS);        // the missing argument is found first
        CHECK(why.find("takes an argument column") != std::string::npos);
    }
    for (const Handle & h : {Handle{0, -1}, Handle{2, CHGPU_F64}, Handle{1, CHGPU_I64}})
        CHECK(on_handle(CHGPU_WIN_SUM, CHGPU_I64, CHGPU_F64, h.n_order, h.recorded) == CHGPU_ERR_BAD_ARGUMENTS);
    CHECK(on_handle(CHGPU_WIN_SUM, CHGPU_I64, CHGPU_F64, 1, CHGPU_F64) == CHGPU_ERR_NOT_IMPLEMENTED); // the handle matches: a float order column
    CHECK(on_handle(CHGPU_WIN_SUM, CHGPU_F64, CHGPU_I64, 1, CHGPU_I64) == CHGPU_ERR_NOT_IMPLEMENTED); // ... a float sum
    CHECK(on_handle(CHGPU_WIN_SUM, CHGPU_I64, CHGPU_I64, 2, CHGPU_I64) == CHGPU_ERR_BAD_ARGUMENTS && why.find("this one has 2") != std::string::npos);
    // an unknown function with a legal RANGE offset: the old entry stops at the frame, the framed one at the function
    CHECK(win_check_frame(week, false, &msg) == CHGPU_ERR_NOT_IMPLEMENTED);
    CHECK(win_check_frame(week, true, &msg) == CHGPU_OK && framed(12, week, CHGPU_I64, CHGPU_I64) == CHGPU_ERR_BAD_ARGUMENTS && why == "unknown window function");
}

int main()
{
    test_search();
    test_extremum_structure();
    test_frames_and_plans();
    printf("window_frames_driver OK\n");
    return 0;
}
