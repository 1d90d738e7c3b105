// The host-only parts of the uniqExact operator (clickhouse_amd/csrc/uniq_host.h): table geometry, the row checks of
// chgpu_uniq_add_block and the plan line.  No device, no library: built with -fsanitize=address,undefined and run by
// tests/test_uniq_exact_abi.py; prints "uniq_exact_driver OK".
#include "../clickhouse_amd/csrc/uniq_host.h"

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

static void geometry()
{
    REQUIRE(uq_grow(2048) == 8192);
    REQUIRE(uq_grow(1ull << 21) == 1ull << 23);
    REQUIRE(uq_grow(1ull << 23) == 1ull << 24);
    REQUIRE(uq_limit(2048) == 1024);
    REQUIRE(uq_limit(UQ_CAP_MAX) == UQ_MAX_SLOTS);
    REQUIRE(uq_limit(UQ_CAP_MAX * 2) == UQ_MAX_SLOTS);
    REQUIRE(uq_capacity_for(0) == UQ_CAP_MIN);
    REQUIRE(uq_capacity_for(1024) == 2048);
    REQUIRE(uq_capacity_for(1025) == 4096);
    REQUIRE(uq_capacity_for(UQ_MAX_SLOTS) == UQ_CAP_MAX);
    REQUIRE(uq_capacity_for(UQ_MAX_SLOTS + 1) == 0);
    REQUIRE(uq_capacity_for(~0ull) == 0);
    // every capacity growth reaches is a power of two, and the chain ends exactly at the largest
    uint64_t cap = UQ_CAP_MIN;
    int steps = 0;
    while (cap < UQ_CAP_MAX)
    {
        cap = uq_grow(cap);
        REQUIRE((cap & (cap - 1)) == 0);
        ++steps;
    }
    REQUIRE(cap == UQ_CAP_MAX && steps == 6 + 9);
}

static void row_checks()
{
    const char * msg = nullptr;
    REQUIRE(pair_check_rows(10, 10, 10, 0, 10, &msg) == CHGPU_OK);
    REQUIRE(pair_check_rows(-1, 10, -1, 3, 3, &msg) == CHGPU_OK);  // an empty range is not an error
    REQUIRE(pair_check_rows(0, 0, 0, 0, 0, &msg) == CHGPU_OK);     // nor is a column of no rows
    REQUIRE(pair_check_rows(9, 10, -1, 0, 9, &msg) == CHGPU_ERR_SIZES_MISMATCH && std::strstr(msg, "key"));
    REQUIRE(pair_check_rows(10, 10, 11, 0, 9, &msg) == CHGPU_ERR_SIZES_MISMATCH && std::strstr(msg, "filter"));
    REQUIRE(pair_check_rows(10, 10, -1, 6, 5, &msg) == CHGPU_ERR_BAD_ARGUMENTS && std::strstr(msg, "row_begin"));
    REQUIRE(pair_check_rows(10, 10, -1, 0, 11, &msg) == CHGPU_ERR_BAD_ARGUMENTS && std::strstr(msg, "past"));
    REQUIRE(pair_check_rows(-1, ~0ull, -1, ~0ull, ~0ull, &msg) == CHGPU_OK);
    REQUIRE(pair_check_rows(-1, 5, -1, ~0ull, 0, &msg) == CHGPU_ERR_BAD_ARGUMENTS);
}

static void plan_line()
{
    UqPlan p;
    p.what = "add";
    p.n = 5000;
    p.cap_before = 2048;
    p.cap = 8192;
    p.tiles = 3;
    p.chunks = 1;
    p.found = 9;
    p.lds = 4000;
    p.sent = 1000;
    p.ovf = 7;
    p.deferred = 12;
    p.grown = 1;
    p.slots_before = 0;
    p.slots = 1001;
    p.holes_before = 0;
    p.holes = 1;
    p.rc = 0;
    char line[512];
    const int len = uq_format_plan(line, sizeof(line), p);
    REQUIRE(len > 0 && (size_t)len < sizeof(line));
    REQUIRE(std::string(line) ==
            "chgpu: uniq plan=add n=5000 cap=2048->8192 tiles=3 chunks=1 found=9 lds=4000 sent=1000 ovf=7 deferred=12 grown=1 slots=0->1001 holes=0->1 rc=0");
    // the widest values still fit the caller's buffer, and a short buffer is cut, terminated and never overrun
    p.n = p.cap_before = p.cap = p.tiles = p.found = p.lds = p.sent = p.ovf = p.deferred = p.slots_before = p.slots = p.holes_before = p.holes = ~0ull;
    p.chunks = p.grown = ~0u;
    p.rc = -7;
    p.what = "merge";
    REQUIRE((size_t)uq_format_plan(line, sizeof(line), p) < sizeof(line));
    std::vector<char> small(16, 'x');
    const int full = uq_format_plan(small.data(), small.size(), p);
    REQUIRE((size_t)full > small.size() && small[15] == '\0' && std::strlen(small.data()) == 15);
}

int main()
{
    geometry();
    row_checks();
    plan_line();
    std::printf("uniq_exact_driver OK\n");
    return 0;
}
