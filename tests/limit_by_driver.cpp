// The host-only parts of the DISTINCT / LIMIT BY operator (clickhouse_amd/csrc/limit_by_host.h): table capacity and growth, the
// checks of create and filter_block, the plan choice, which slot bytes the rank plan passes over and the plan line.
// No device, no library: built with -fsanitize=address,undefined and run by tests/test_limit_by_abi.py; prints "limit_by_driver OK".
#include "../clickhouse_amd/csrc/limit_by_host.h"

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

static void capacity_and_growth()
{
    REQUIRE(LB_TILE == 1024 && (LB_CAP_MIN & (LB_CAP_MIN - 1)) == 0 && (LB_CAP_MAX & (LB_CAP_MAX - 1)) == 0);
    REQUIRE(lb_limit(LB_CAP_MAX) == LB_MAX_KEYS);
    REQUIRE(LB_CAP_MAX < LB_MISSING && LB_MISSING < LB_NONE); // every slot, the empty value's (= capacity) included, is below the marks
    REQUIRE(lb_capacity_for(0) == LB_CAP_MIN && lb_capacity_for(1) == LB_CAP_MIN && lb_capacity_for(LB_CAP_MIN / 2) == LB_CAP_MIN);
    REQUIRE(lb_capacity_for(LB_CAP_MIN / 2 + 1) == 2 * LB_CAP_MIN);
    REQUIRE(lb_capacity_for(LB_MAX_KEYS) == LB_CAP_MAX && lb_capacity_for(LB_MAX_KEYS + 1) == 0);
    for (uint64_t keys : {0ull, 1ull, 1000ull, 1024ull, 1025ull, 20000ull, 1ull << 20, (1ull << 27) + 3})
    {
        const uint64_t cap = lb_capacity_for(keys);
        REQUIRE(cap != 0 && (cap & (cap - 1)) == 0 && lb_limit(cap) >= keys && (cap == LB_CAP_MIN || lb_limit(cap / 2) < keys));
    }
    // the growth rule: x4 below 2^23 cells, x2 from there; always past the keys held; nothing beyond the last capacity
    REQUIRE(lb_grow(2048) == 8192 && lb_grow(1ull << 22) == (1ull << 24) && lb_grow(1ull << 23) == (1ull << 24));
    REQUIRE(lb_next_capacity(2048, 1024, 20000) == 8192);
    REQUIRE(lb_next_capacity(8192, 4096, 20000) == 32768 && lb_next_capacity(32768, 16384, 20000) == 131072);
    REQUIRE(lb_next_capacity(1ull << 23, 1ull << 22, 5) == (1ull << 24));
    REQUIRE(lb_next_capacity(2048, 1ull << 13, 0) == (1ull << 15)); // a table far past its limit: doubled until the keys fit below it
    REQUIRE(lb_next_capacity(LB_CAP_MAX, LB_MAX_KEYS, 1) == 0 && lb_next_capacity(LB_CAP_MAX / 2, LB_MAX_KEYS / 2, 1) == LB_CAP_MAX);
    // a block with a million rows of absent keys or more: sized for them at once, but by no more than x64 a growth
    REQUIRE(lb_next_capacity(2048, 1024, LB_JUMP_MIN - 1) == 8192);
    REQUIRE(lb_next_capacity(2048, 1024, LB_JUMP_MIN) == 2048 * LB_JUMP_MAX && lb_next_capacity(2048, 1024, 100000000ull) == 2048 * LB_JUMP_MAX);
    REQUIRE(lb_next_capacity(1ull << 17, 1ull << 16, LB_JUMP_MIN) == lb_capacity_for((1ull << 16) + LB_JUMP_MIN));
    REQUIRE(lb_next_capacity(1ull << 23, 1ull << 22, 100000000ull) == (1ull << 28));
    REQUIRE(lb_next_capacity(2048, 1024, ~0ull >> 1) == 2048 * LB_JUMP_MAX && lb_next_capacity(1ull << 29, 1ull << 28, ~0ull >> 1) == LB_CAP_MAX);
    // every chain of growths ends at the last capacity
    uint64_t cap = LB_CAP_MIN, steps = 0;
    while (uint64_t next = lb_next_capacity(cap, lb_limit(cap), 1))
    {
        REQUIRE(next > cap && steps++ < 64);
        cap = next;
    }
    REQUIRE(cap == LB_CAP_MAX);
    // growth between insert rounds: at the limit always; after a round that met its flag only from half way to the limit, or after four
    // such rounds on one table
    REQUIRE(lb_should_grow(2048, 1024, false, 0) && lb_should_grow(2048, 1024, true, 0) && lb_should_grow(2048, 5000, false, 0));
    REQUIRE(!lb_should_grow(2048, 0, false, 0) && !lb_should_grow(2048, 1023, false, 9));
    REQUIRE(!lb_should_grow(2048, 209, true, 0) && !lb_should_grow(2048, 511, true, 3) && lb_should_grow(2048, 512, true, 0) && lb_should_grow(2048, 1, true, 4));
}

static void bounds_and_rows()
{
    const char * msg = nullptr;
    REQUIRE(lb_check_bounds(1, 0, &msg) == CHGPU_OK);
    REQUIRE(lb_check_bounds(0, 0, &msg) == CHGPU_ERR_BAD_ARGUMENTS && std::strstr(msg, "group_length"));
    REQUIRE(lb_check_bounds(0, 5, &msg) == CHGPU_ERR_BAD_ARGUMENTS);
    // offset + length at 2^32 - 2, 2^32 - 1 and 2^32, however the sum is split
    const uint64_t top = 0xFFFFFFFFull;
    REQUIRE(lb_check_bounds(top - 1, 0, &msg) == CHGPU_OK && lb_check_bounds(1, top - 2, &msg) == CHGPU_OK && lb_check_bounds(1000, top - 1001, &msg) == CHGPU_OK);
    REQUIRE(lb_check_bounds(top, 0, &msg) == CHGPU_OK && lb_check_bounds(1, top - 1, &msg) == CHGPU_OK && lb_check_bounds(top - 1, 1, &msg) == CHGPU_OK);
    REQUIRE(lb_check_bounds(top + 1, 0, &msg) == CHGPU_ERR_NOT_IMPLEMENTED && std::strstr(msg, "2^32"));
    REQUIRE(lb_check_bounds(1, top, &msg) == CHGPU_ERR_NOT_IMPLEMENTED && lb_check_bounds(top, 1, &msg) == CHGPU_ERR_NOT_IMPLEMENTED);
    REQUIRE(lb_check_bounds(~0ull, ~0ull, &msg) == CHGPU_ERR_NOT_IMPLEMENTED && lb_check_bounds(1, ~0ull, &msg) == CHGPU_ERR_NOT_IMPLEMENTED); // no wrap-around

    REQUIRE(lb_check_rows(10, -1, 0, 10, &msg) == CHGPU_OK && lb_check_rows(10, 10, 3, 3, &msg) == CHGPU_OK && lb_check_rows(0, -1, 0, 0, &msg) == CHGPU_OK);
    REQUIRE(lb_check_rows(10, -1, 4, 3, &msg) == CHGPU_ERR_BAD_ARGUMENTS && std::strstr(msg, "row_begin"));
    REQUIRE(lb_check_rows(10, -1, 0, 11, &msg) == CHGPU_ERR_BAD_ARGUMENTS && std::strstr(msg, "past"));
    REQUIRE(lb_check_rows(10, 9, 0, 10, &msg) == CHGPU_ERR_SIZES_MISMATCH && std::strstr(msg, "filter"));
    REQUIRE(lb_check_rows(10, 0, 0, 0, &msg) == CHGPU_ERR_SIZES_MISMATCH);
    REQUIRE(lb_check_rows(1ull << 33, -1, 5, 5 + LB_MAX_ROWS, &msg) == CHGPU_OK);
    REQUIRE(lb_check_rows(1ull << 33, -1, 5, 5 + LB_MAX_ROWS + 1, &msg) == CHGPU_ERR_TOO_MANY_ROWS && std::strstr(msg, "2^32"));
}

static void plan_choice()
{
    REQUIRE(lb_choose_plan(0, 1) == LB_PLAN_DEAD && lb_choose_plan(0, 7) == LB_PLAN_DEAD);
    REQUIRE(lb_choose_plan(1, 1) == LB_PLAN_CLAIM && lb_choose_plan(1ull << 31, 1) == LB_PLAN_CLAIM);
    REQUIRE(lb_choose_plan(1, 2) == LB_PLAN_RANK && lb_choose_plan(5, 0xFFFFFFFFull) == LB_PLAN_RANK);
    REQUIRE(!std::strcmp(lb_plan_name(LB_PLAN_DEAD), "dead") && !std::strcmp(lb_plan_name(LB_PLAN_CLAIM), "claim") && !std::strcmp(lb_plan_name(LB_PLAN_RANK), "rank"));
}

// the two words of a slot list, as the device folds them
static std::vector<uint32_t> passes_of(const std::vector<uint32_t> & slots)
{
    uint32_t o = 0, a = ~0u;
    for (uint32_t s : slots)
    {
        o |= s;
        a &= s;
    }
    uint32_t shifts[4];
    const uint32_t n = lb_plan_passes(o, a, shifts);
    REQUIRE(n <= 4);
    return std::vector<uint32_t>(shifts, shifts + n);
}

static void slot_bytes()
{
    typedef std::vector<uint32_t> S;
    REQUIRE(passes_of({}) == S{});                     // no live record: or = 0, and = ~0
    REQUIRE(passes_of({77}) == S{} && passes_of({0x12345678u, 0x12345678u}) == S{} && passes_of({0, 0}) == S{}); // one live slot: no pass
    REQUIRE(passes_of({0x00050011u, 0x00070011u, 0x00FF0011u}) == S{16});  // only byte 2
    REQUIRE(passes_of({0x1FF, 0x100}) == S{0});       // byte 1 is equal in both
    REQUIRE(passes_of({1, 0x101}) == S{8});
    REQUIRE(passes_of({0x01000001u, 0x02000002u}) == (S{0, 24}));
    REQUIRE(passes_of({0, 0x7FFFFFFFu}) == (S{0, 8, 16, 24}) && passes_of({0x01010101u, 0x02020202u}) == (S{0, 8, 16, 24})); // all four
    REQUIRE(passes_of({3, 2048}) == (S{0, 8}));       // a cell and the empty value's slot of the smallest table
    // sorting by the planned bytes, least significant first and stably, sorts the slots
    std::vector<uint32_t> slots{0xAB000301u, 0xAB000002u, 0xAB010001u, 0xAB000301u, 0xAB000001u};
    const S sh = passes_of(slots);
    REQUIRE(sh == (S{0, 8, 16}));
    for (uint32_t shift : sh)
    {
        std::vector<uint32_t> next;
        for (uint32_t b = 0; b < 256; ++b)
            for (uint32_t s : slots)
                if (((s >> shift) & 0xFF) == b)
                    next.push_back(s);
        slots = next;
    }
    for (size_t i = 1; i < slots.size(); ++i)
        REQUIRE(slots[i - 1] <= slots[i]);
}

static void plan_line()
{
    LbPlan p;
    p.kind = LB_PLAN_RANK;
    p.n = 5121;
    p.entered = 5000;
    p.live = 4000;
    p.passes = 2;
    p.passed = 17;
    p.keys_before = 3;
    p.keys = 20;
    p.cap_before = 2048;
    p.cap = 8192;
    p.grown = 1;
    p.rc = CHGPU_ERR_OOM;
    char line[512];
    const int len = lb_format_plan(line, sizeof(line), p);
    REQUIRE(len > 0 && (size_t)len < sizeof(line));
    REQUIRE(std::string(line) == "chgpu: limit_by plan=rank n=5121 entered=5000 live=4000 passes=2 passed=17 keys=3->20 cap=2048->8192 grown=1 rc=-3");
    LbPlan dead;
    lb_format_plan(line, sizeof(line), dead);
    REQUIRE(std::string(line) == "chgpu: limit_by plan=dead n=0 entered=0 live=0 passes=0 passed=0 keys=0->0 cap=0->0 grown=0 rc=0");
    LbPlan big;
    big.kind = LB_PLAN_CLAIM;
    big.n = big.entered = big.live = big.passed = LB_MAX_ROWS;
    big.keys_before = big.keys = LB_MAX_KEYS;
    big.cap_before = big.cap = LB_CAP_MAX;
    big.grown = ~0u;
    char small[32];
    const int want = lb_format_plan(small, sizeof(small), big); // a short buffer is cut, never overrun
    REQUIRE(want > (int)sizeof(small) && std::strlen(small) == sizeof(small) - 1);
}

int main()
{
    capacity_and_growth();
    bounds_and_rows();
    plan_choice();
    slot_bytes();
    plan_line();
    std::printf("limit_by_driver OK\n");
    return 0;
}
