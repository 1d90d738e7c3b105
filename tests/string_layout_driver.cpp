// The buffer layouts of the ColumnString operators (clickhouse_amd/csrc/string_host.h): for every layout and row count, the sub-buffers
// lie in declaration order, start on 256-byte boundaries, are large enough, do not overlap and end exactly at the size the sizing run
// asked of the pool; the sizing run and the carving run agree.  No device, no library, nothing is dereferenced: built with
// -fsanitize=address,undefined and run by tests/test_string_layout_abi.py; prints "string_layout_driver OK".
#include "../clickhouse_amd/csrc/string_host.h"

#include <cstdio>
#include <cstdlib>
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

struct Part
{
    const void * p;
    uint64_t bytes; // what the kernels use of it
};

static const uintptr_t BASE = 0x7f0000000000ull; // an address as the pool gives it: 256-aligned, never dereferenced

// as scan.hip's chgpu_scan_tmp_bytes: one u64 per tile of 2048 elements and two more (any size must carve alike)
static size_t scan_tmp_bytes(uint64_t n) { return (size_t)((n + 2047) / 2048 + 2) * 8; }

// as chgpu_string_dictionary_encode derives its table: a power of two, at least two cells per row
static uint64_t str_dict_capacity(uint64_t n)
{
    uint64_t cap = 1024;
    while (cap < 2 * n)
        cap <<= 1;
    return cap;
}

static void check(const char * what, uint64_t n, size_t sized, size_t carved, const std::vector<Part> & sizing, const std::vector<Part> & parts)
{
    REQUIRE(sized == carved);
    REQUIRE(sized % 256 == 0 && sized > 0);
    for (const Part & s : sizing)
        REQUIRE(s.p == nullptr); // the sizing run hands out no pointer
    uintptr_t at = BASE;
    for (const Part & part : parts)
    {
        const uintptr_t p = (uintptr_t)part.p;
        REQUIRE(p == at);         // declaration order, nothing between two sub-buffers but the rounding
        REQUIRE(p % 256 == 0);
        at = p + (uintptr_t)((part.bytes + 255) / 256 * 256);
        REQUIRE(at >= p + part.bytes && at - (p + part.bytes) < 256); // disjoint from the next one, by less than one rounding
    }
    REQUIRE(at == BASE + sized);  // the last one ends where the allocation ends
    std::printf("%s n=%llu bytes=%zu\n", what, (unsigned long long)n, sized);
}

static std::vector<Part> parts_of(const StrDictLayout & l, uint64_t n, uint64_t cap, size_t tmp)
{
    return {{l.hash, n * 8}, {l.rep_row, n * 8}, {l.is_first, n * 4}, {l.prefix, n * 8}, {l.tags, cap * 8}, {l.first_row, cap * 8},
            {l.fail, 4}, {l.total, 8}, {l.scan_tmp, tmp}};
}

static std::vector<Part> parts_of(const StrValuesLayout & l, uint64_t n, bool kept, size_t tmp)
{
    std::vector<Part> v;
    if (kept)
        v = {{l.flag, n * 4}, {l.row_pos, n * 8}};
    for (const Part & part : std::vector<Part>{{l.sizes, n * 4}, {l.pos, n * 8}, {l.words, sizeof(StrLayoutWords)}, {l.scan_tmp, tmp}})
        v.push_back(part);
    return v;
}

static std::vector<Part> parts_of(const SsSegs & t, uint64_t cap)
{
    return {{t.start, cap * 8}, {t.first, cap * 8}, {t.depth, cap * 8}, {t.adv, cap * 8}, {t.head, cap * 8}};
}

static std::vector<Part> parts_of(const SsRoundLayout & l, uint64_t m, size_t tmp)
{
    return {{l.new_head, m * 4}, {l.active, m * 4}, {l.seg_no, m * 8}, {l.slot, m * 8}, {l.totals, 16}, {l.scan_tmp, tmp}};
}

int main()
{
    REQUIRE(sizeof(StrLayoutWords) == 32 && sizeof(void *) == 8);
    REQUIRE(str_dict_capacity(1) == 1024 && str_dict_capacity(512) == 1024 && str_dict_capacity(513) == 2048);
    for (uint64_t n : {1ull, 63ull, 64ull, 65ull, 2048ull, (1ull << 32) - 1})
    {
        const size_t tmp = scan_tmp_bytes(n);
        {
            const uint64_t cap = str_dict_capacity(n);
            REQUIRE((cap & (cap - 1)) == 0 && cap >= 2 * n && (cap == 1024 || cap / 2 < 2 * n));
            StrDictLayout a, b;
            const size_t sized = str_dict_lay(0, n, cap, tmp, &a), carved = str_dict_lay(BASE, n, cap, tmp, &b);
            check("dictionary_encode", n, sized, carved, parts_of(a, n, cap, tmp), parts_of(b, n, cap, tmp));
        }
        for (bool kept : {true, false}) // filter, index
        {
            StrValuesLayout a, b;
            const size_t sized = str_values_lay(0, n, kept, tmp, &a), carved = str_values_lay(BASE, n, kept, tmp, &b);
            REQUIRE(kept || (b.flag == nullptr && b.row_pos == nullptr));
            check(kept ? "filter" : "index", n, sized, carved, parts_of(a, n, kept, tmp), parts_of(b, n, kept, tmp));
        }
        {
            SsRoundLayout a, b;
            const size_t sized = ss_round_lay(0, n, tmp, &a), carved = ss_round_lay(BASE, n, tmp, &b);
            check("sort round", n, sized, carved, parts_of(a, n, tmp), parts_of(b, n, tmp));
        }
        for (uint64_t cap : {(uint64_t)1, n / 2 + 1}) // the first round's one segment; a round over n rows leaves at most n / 2 segments
        {
            SsSegs a, b;
            const size_t sized = ss_segs_lay(0, cap, &a), carved = ss_segs_lay(BASE, cap, &b);
            check("sort segments", cap, sized, carved, parts_of(a, cap), parts_of(b, cap));
        }
    }
    // what the entry points ask of the pool for one row, term by term
    {
        StrDictLayout d;
        StrValuesLayout f, s;
        SsRoundLayout r;
        SsSegs t;
        REQUIRE(str_dict_lay(0, 1, 1024, 24, &d) == 4 * 256 + 2 * 8192 + 3 * 256);
        REQUIRE(str_values_lay(0, 1, true, 24, &f) == 6 * 256 && str_values_lay(0, 1, false, 24, &s) == 4 * 256);
        REQUIRE(ss_round_lay(0, 1, 24, &r) == 6 * 256 && ss_segs_lay(0, 1, &t) == 5 * 256);
    }
    std::printf("string_layout_driver OK\n");
    return 0;
}
