// The host-only parts of the groupArray operator (clickhouse_amd/csrc/group_array_host.h): the pass planning from the two key words,
// the capacity of the doubling store up to the row limit, max_size, the work-unit arithmetic of the segmented copy and the plan lines.
// No device, no library: built with -fsanitize=address,undefined and run by tests/test_group_array_abi.py; prints
// "group_array_driver OK".
#include "../clickhouse_amd/csrc/group_array_host.h"

#include <cstdlib>
#include <cstring>
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

// the two words of a key list, as the device folds them
static void fold(const std::vector<uint64_t> & keys, uint64_t * o, uint64_t * a)
{
    *o = 0;
    *a = ~0ull;
    for (uint64_t k : keys)
    {
        *o |= k;
        *a &= k;
    }
}

static std::vector<uint32_t> passes_of(const std::vector<uint64_t> & keys)
{
    uint64_t o, a;
    fold(keys, &o, &a);
    uint32_t shifts[8];
    const uint32_t n = ga_plan_passes(o, a, shifts);
    REQUIRE(n <= 8);
    return std::vector<uint32_t>(shifts, shifts + n);
}

static void pass_planning()
{
    typedef std::vector<uint32_t> S;
    REQUIRE(passes_of({}) == S{});                                            // the empty store: or = 0, and = ~0
    REQUIRE(passes_of({42}) == S{});                                          // one key
    REQUIRE(passes_of({0xDEADBEEFCAFEF00Dull, 0xDEADBEEFCAFEF00Dull}) == S{}); // no varying bit
    REQUIRE(passes_of({0, 0}) == S{} && passes_of({~0ull, ~0ull}) == S{});
    REQUIRE(passes_of({0x0000050000000011ull, 0x0000070000000011ull, 0x0000FF0000000011ull}) == S{40}); // only byte 5
    REQUIRE(passes_of({0x0100000000000001ull, 0x0200000000000002ull}) == (S{0, 56}));                    // bytes 0 and 7
    REQUIRE(passes_of({0, ~0ull}) == (S{0, 8, 16, 24, 32, 40, 48, 56}));                                  // all eight
    REQUIRE(passes_of({0x0101010101010101ull, 0x0202020202020202ull}).size() == 8);
    REQUIRE(passes_of({0x1FF, 0x100}) == S{0});   // byte 1 is equal in both
    REQUIRE(passes_of({1, 2, 3, 0xFFFFF}) == (S{0, 8, 16})); // dictionary ids below 2^20: three passes, not eight
    // a byte is passed over exactly when all keys agree in it: sorting by the planned bytes sorts the keys
    const std::vector<uint64_t> keys{0xAA00000000BB0001ull, 0xAA00000000BB0300ull, 0xAA00000000BB0002ull, 0xAA00000000CC0001ull};
    const S sh = passes_of(keys);
    REQUIRE(sh == (S{0, 8, 16}));
    for (size_t i = 0; i < keys.size(); ++i)
        for (size_t j = 0; j < keys.size(); ++j)
        {
            uint64_t mi = 0, mj = 0; // the keys as the planned bytes only
            for (size_t p = 0; p < sh.size(); ++p)
            {
                mi |= ((keys[i] >> sh[p]) & 0xFF) << (8 * p);
                mj |= ((keys[j] >> sh[p]) & 0xFF) << (8 * p);
            }
            REQUIRE((keys[i] < keys[j]) == (mi < mj));
        }
}

static void capacity()
{
    REQUIRE(ga_capacity_for(0) == 4096 && ga_capacity_for(1) == 4096 && ga_capacity_for(4096) == 4096 && ga_capacity_for(4097) == 8192);
    uint64_t prev = 0;
    for (uint64_t need = 1; need < GA_MAX_VALUES; need = need * 2 + 1)
    {
        const uint64_t cap = ga_capacity_for(need);
        REQUIRE(cap >= need && (cap & (cap - 1)) == 0 && cap >= prev && (cap == 4096 || cap / 2 < need));
        prev = cap;
    }
    REQUIRE(ga_capacity_for(GA_MAX_VALUES - 1) == (1ull << 32));
    REQUIRE(ga_capacity_for(GA_MAX_VALUES) == 0 && ga_capacity_for(GA_MAX_VALUES + 1) == 0 && ga_capacity_for(~0ull) == 0); // the row limit
    REQUIRE(ga_trim(5, 0) == 5 && ga_trim(5, 3) == 3 && ga_trim(3, 3) == 3 && ga_trim(2, 3) == 2 && ga_trim(0, 1) == 0);
}

// every output element of a copy of arrays of `counts` elements is reached exactly once, through the unit that owns it, and lands in
// the right array at the right place
static void cover(const std::vector<uint64_t> & counts)
{
    std::vector<uint64_t> ends;
    uint64_t total = 0;
    for (uint64_t c : counts)
        ends.push_back(total += c);
    const uint64_t n_segs = counts.size();
    std::vector<std::vector<uint8_t>> seen(n_segs);
    for (uint64_t s = 0; s < n_segs; ++s)
        seen[s].assign(counts[s], 0);
    const uint64_t units = ga_units(total);
    REQUIRE(units == (total + GA_UNIT - 1) / GA_UNIT);
    uint64_t next = 0;
    for (uint64_t u = 0; u < units; ++u)
    {
        uint64_t e0, e1, s0, s1;
        ga_unit_range(ends.data(), n_segs, total, u, &e0, &e1, &s0, &s1);
        REQUIRE(e0 == next && e1 > e0 && e1 - e0 <= GA_UNIT && e1 <= total && s0 <= s1 && s1 < n_segs);
        next = e1;
        for (uint64_t e = e0; e < e1; ++e)
        {
            const uint64_t s = ga_seg_of(ends.data(), s0, s1, e); // as k_ga_seg_copy searches: among the unit's arrays only
            REQUIRE(s >= s0 && s <= s1 && s == ga_seg_of(ends.data(), 0, n_segs, e));
            const uint64_t start = s ? ends[s - 1] : 0;
            REQUIRE(e >= start && e < ends[s]);
            REQUIRE(seen[s][e - start] == 0);
            seen[s][e - start] = 1;
        }
    }
    REQUIRE(next == total);
    for (uint64_t s = 0; s < n_segs; ++s)
        for (uint8_t b : seen[s])
            REQUIRE(b == 1);
}

static void unit_arithmetic()
{
    REQUIRE(ga_units(0) == 0 && ga_units(1) == 1 && ga_units(GA_UNIT) == 1 && ga_units(GA_UNIT + 1) == 2);
    cover({});
    cover({0, 0, 0});
    cover({1});
    cover({GA_UNIT});
    cover({GA_UNIT - 1, 1, 1});
    cover({GA_UNIT + 1});
    cover({0, 0, 5, 0, 0, 0, 7, 0});                        // zeros before, between and behind
    cover({3 * GA_UNIT + 17});                              // one giant array: every unit lies inside it
    cover({0, 10 * GA_UNIT + 1, 0, 1, 0});
    std::vector<uint64_t> ones(3 * GA_UNIT + 5, 1);         // a run of ones: a unit touches GA_UNIT arrays
    cover(ones);
    std::vector<uint64_t> mixed(2000, 1);                   // ones, a giant, zeros, ones
    mixed.push_back(5 * GA_UNIT - 3);
    mixed.insert(mixed.end(), 300, 0);
    mixed.insert(mixed.end(), 5000, 1);
    mixed.push_back(0);
    cover(mixed);
    std::vector<uint64_t> ragged;
    uint64_t x = 88172645463325252ull;                       // xorshift: lengths 0 .. 40 with a long one now and then
    for (int i = 0; i < 3000; ++i)
    {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        ragged.push_back(x % 97 == 0 ? GA_UNIT + x % 1000 : x % 41);
    }
    cover(ragged);
    const uint64_t ends[] = {0, 0, 4, 4, 9}; // empty arrays are stepped over; past the last end there is no array
    REQUIRE(ga_seg_of(ends, 0, 5, 0) == 2 && ga_seg_of(ends, 0, 5, 3) == 2 && ga_seg_of(ends, 0, 5, 4) == 4 && ga_seg_of(ends, 0, 5, 9) == 5);
}

static void plan_lines()
{
    char buf[512];
    GaAddPlan a;
    a.n = 100;
    a.entered = 40;
    a.held_before = 7;
    a.held = 47;
    ga_format_add_plan(buf, sizeof(buf), a);
    REQUIRE(std::string(buf) == "chgpu: group_array plan=add n=100 entered=40 held=7->47 rc=0");
    a.what = "merge";
    a.rc = CHGPU_ERR_OOM;
    a.entered = 0;
    a.held = 7;
    ga_format_add_plan(buf, sizeof(buf), a);
    REQUIRE(std::string(buf) == "chgpu: group_array plan=merge n=100 entered=0 held=7->7 rc=" + std::to_string(CHGPU_ERR_OOM));
    GaPlan p;
    p.groups = 3;
    p.values = 1ull << 33;
    p.passes = 2;
    p.trimmed = 5;
    p.cached = 1;
    ga_format_plan(buf, sizeof(buf), p);
    REQUIRE(std::string(buf) == "chgpu: group_array plan=finalize groups=3 values=8589934592 passes=2 trimmed=5 cached=1");
    p.what = "for_keys";
    char tiny[16];
    const int need = ga_format_plan(tiny, sizeof(tiny), p); // truncated, terminated, never past the buffer
    REQUIRE(need > (int)sizeof(tiny) && std::strlen(tiny) == sizeof(tiny) - 1);
    REQUIRE(GaPlan().cached == 0 && GaPlan().passes == 0 && std::string(GaPlan().what) == "finalize" && std::string(GaAddPlan().what) == "add");
}

static void row_checks() // the shared checks this operator's add_block answers with
{
    const char * msg = "";
    REQUIRE(pair_check_rows(10, 10, -1, 0, 10, &msg) == CHGPU_OK);
    REQUIRE(pair_check_rows(9, 10, -1, 0, 10, &msg) == CHGPU_ERR_SIZES_MISMATCH);
    REQUIRE(pair_check_rows(-1, 10, 9, 0, 10, &msg) == CHGPU_ERR_SIZES_MISMATCH);
    REQUIRE(pair_check_rows(-1, 10, -1, 6, 5, &msg) == CHGPU_ERR_BAD_ARGUMENTS);
    REQUIRE(pair_check_rows(-1, 10, -1, 0, 11, &msg) == CHGPU_ERR_BAD_ARGUMENTS);
}

int main()
{
    pass_planning();
    capacity();
    unit_arithmetic();
    plan_lines();
    row_checks();
    std::printf("group_array_driver OK\n");
    return 0;
}
