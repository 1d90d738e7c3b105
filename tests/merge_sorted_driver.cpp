// merge_sorted_driver.cpp — the host-only parts of the merge of sorted runs (clickhouse_amd/csrc/merge_host.h) as a stand-alone program,
// built with -fsanitize=address,undefined by tests/test_merge_sorted_abi.py: the validation of the run offsets, the run list of every
// round for K = 0 to 9 and K = 257 with empty runs and with limits, the tile-to-pair table, the merge-path search against a brute-force
// merge (all-equal arrays included), the whole tree replayed on the host tile by tile with the kernels' own arithmetic against
// std::stable_sort, and merge_plan on the shapes tests/test_gpu_merge_sorted.py uses to reach each plan.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "../clickhouse_amd/csrc/merge_host.h"

#define CHECK(cond)                                                         \
    do                                                                      \
    {                                                                       \
        if (!(cond))                                                        \
        {                                                                   \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static void test_offsets()
{
    const char * msg = nullptr;
    uint64_t rows = 7;
    const uint64_t none[1] = {0};
    CHECK(merge_check_offsets(none, 0, &rows, &msg) == CHGPU_OK && rows == 0);
    const uint64_t good[5] = {0, 3, 3, 10, 10};
    CHECK(merge_check_offsets(good, 4, &rows, &msg) == CHGPU_OK && rows == 10);
    msg = nullptr;
    CHECK(merge_check_offsets(nullptr, 2, &rows, &msg) == CHGPU_ERR_BAD_ARGUMENTS && msg);
    const uint64_t late[3] = {1, 3, 4};
    msg = nullptr;
    CHECK(merge_check_offsets(late, 2, &rows, &msg) == CHGPU_ERR_BAD_ARGUMENTS && msg);
    const uint64_t down[4] = {0, 5, 4, 9};
    msg = nullptr;
    CHECK(merge_check_offsets(down, 3, &rows, &msg) == CHGPU_ERR_BAD_ARGUMENTS && msg);
    const uint64_t most[2] = {0, MRG_MAX_ROWS};
    CHECK(merge_check_offsets(most, 1, &rows, &msg) == CHGPU_OK && rows == MRG_MAX_ROWS);
    const uint64_t wide[3] = {0, 1, MRG_MAX_ROWS + 1};
    msg = nullptr;
    CHECK(merge_check_offsets(wide, 2, &rows, &msg) == CHGPU_ERR_NOT_IMPLEMENTED && msg);
    CHECK(MRG_TILE == MRG_THREADS * MRG_ITEMS);
}

// every round of `lens` under `limit`: pairs tile the input and the output back to back, the odd run passes through, outputs are cut
static void check_rounds(const std::vector<uint32_t> & lens0, uint64_t limit)
{
    std::vector<uint32_t> lens = lens0;
    for (uint32_t & l : lens)
        l = (uint32_t)merge_cut(l, limit);
    const std::vector<MergeRound> rounds = merge_rounds(lens, limit);
    CHECK(rounds.size() == merge_round_count((uint32_t)lens0.size()));
    for (const MergeRound & rd : rounds)
    {
        CHECK(rd.pairs.size() == (lens.size() + 1) / 2);
        uint32_t in_pos = 0, out_pos = 0, tiles = 0;
        std::vector<uint32_t> next;
        for (size_t j = 0; j < rd.pairs.size(); ++j)
        {
            const MergePair & p = rd.pairs[j];
            CHECK(p.a_begin == in_pos && p.a_len == lens[2 * j] && p.b_begin == in_pos + p.a_len);
            CHECK(p.b_len == (2 * j + 1 < lens.size() ? lens[2 * j + 1] : 0));
            in_pos += p.a_len + p.b_len;
            CHECK(p.out_begin == out_pos);
            CHECK(p.out_len == (limit && p.a_len + p.b_len > limit ? limit : p.a_len + p.b_len));
            out_pos += p.out_len;
            CHECK(p.tile_begin == tiles && p.split_begin == tiles + j);
            tiles += (p.out_len + MRG_TILE - 1) / MRG_TILE;
            next.push_back(p.out_len);
        }
        CHECK(in_pos == std::accumulate(lens.begin(), lens.end(), 0u));
        CHECK(rd.n_tiles == tiles && rd.n_splits == tiles + rd.pairs.size() && rd.out_rows == out_pos);
        // the tile-to-pair table: every tile and every tile edge finds its pair
        for (size_t j = 0; j < rd.pairs.size(); ++j)
        {
            const MergePair & p = rd.pairs[j];
            const uint32_t n = (p.out_len + MRG_TILE - 1) / MRG_TILE;
            for (uint32_t k = 0; k < n; ++k)
                CHECK(merge_pair_of<&MergePair::tile_begin>(rd.pairs.data(), (uint32_t)rd.pairs.size(), p.tile_begin + k) == j);
            for (uint32_t k = 0; k <= n; ++k)
                CHECK(merge_pair_of<&MergePair::split_begin>(rd.pairs.data(), (uint32_t)rd.pairs.size(), p.split_begin + k) == j);
        }
        lens.swap(next);
    }
    CHECK(lens.size() <= 1 || lens0.size() <= 1);
    if (lens0.size() > 1)
    {
        const uint64_t total = std::accumulate(lens0.begin(), lens0.end(), (uint64_t)0);
        CHECK(lens.size() == 1 && lens[0] == merge_cut(total, limit));
    }
}

static void test_rounds()
{
    CHECK(merge_round_count(0) == 0 && merge_round_count(1) == 0 && merge_round_count(2) == 1 && merge_round_count(3) == 2);
    CHECK(merge_round_count(8) == 3 && merge_round_count(9) == 4 && merge_round_count(257) == 9 && merge_round_count(1024) == 10);
    const uint64_t limits[] = {0, 1, 5, MRG_TILE, MRG_TILE + 1, 1000000};
    for (uint32_t K = 0; K <= 9; ++K)
        for (uint64_t limit : limits)
            for (int shape = 0; shape < 4; ++shape)
            {
                std::vector<uint32_t> lens(K);
                for (uint32_t r = 0; r < K; ++r)
                    lens[r] = shape == 0 ? 0 : shape == 1 ? (r % 3 == 1 ? 0 : r + 1) : shape == 2 ? MRG_TILE * (r % 3) + (r % 2) : (uint32_t)(rnd() % (3 * MRG_TILE));
                check_rounds(lens, limit);
            }
    for (uint64_t limit : limits)
    {
        std::vector<uint32_t> lens(257);
        for (uint32_t r = 0; r < 257; ++r)
            lens[r] = r % 5 == 2 ? 0 : (uint32_t)(rnd() % 40);
        lens[100] = 3 * MRG_TILE + 1;
        check_rounds(lens, limit);
    }
}

static std::vector<uint32_t> brute_merge_a_counts(const std::vector<uint32_t> & a, const std::vector<uint32_t> & b)
{
    // counts[d] = how many of the first d outputs of the stable merge (A first on ties) come from A
    std::vector<uint32_t> counts(a.size() + b.size() + 1, 0);
    size_t i = 0, j = 0;
    for (size_t d = 0; d < a.size() + b.size(); ++d)
    {
        const bool take_b = j < b.size() && (i >= a.size() || b[j] < a[i]);
        take_b ? ++j : ++i;
        counts[d + 1] = (uint32_t)i;
    }
    return counts;
}

static void test_merge_path()
{
    for (int round = 0; round < 400; ++round)
    {
        const uint32_t na = (uint32_t)(rnd() % 20), nb = (uint32_t)(rnd() % 20);
        const uint32_t range = round % 4 == 0 ? 1 : (uint32_t)(rnd() % 6 + 1); // range 1: all-equal arrays
        std::vector<uint32_t> a(na), b(nb);
        for (uint32_t & x : a)
            x = (uint32_t)(rnd() % range);
        for (uint32_t & x : b)
            x = (uint32_t)(rnd() % range);
        std::sort(a.begin(), a.end());
        std::sort(b.begin(), b.end());
        const std::vector<uint32_t> want = brute_merge_a_counts(a, b);
        for (uint32_t d = 0; d <= na + nb; ++d)
        {
            const uint32_t got = merge_path(d, na, nb, [&](uint32_t bi, uint32_t ai) {
                CHECK(bi < nb && ai < na); // the search never reads outside either run
                return b[bi] < a[ai];
            });
            CHECK(got == want[d]);
        }
        if (range == 1)
            for (uint32_t d = 0; d <= na + nb; ++d)
                CHECK(want[d] == (d < na ? d : na)); // all equal: the whole left run first
    }
}

// The tree as the kernels run it: (word, row) arrays ping-pong, every round's splits by merge_path over the whole runs, every tile staged,
// each of its threads finding its diagonal and merging MRG_ITEMS outputs.  Against std::stable_sort of the concatenation.
static void replay_tree(const std::vector<uint32_t> & lens0, uint32_t range, uint64_t limit)
{
    struct Rec { uint64_t word; uint32_t row; };
    std::vector<Rec> all;
    std::vector<Rec> cur;
    std::vector<uint32_t> lens;
    uint32_t row = 0;
    for (uint32_t len : lens0)
    {
        std::vector<Rec> run(len);
        for (Rec & r : run)
            r.word = rnd() % range;
        std::sort(run.begin(), run.end(), [](const Rec & x, const Rec & y) { return x.word < y.word; });
        for (Rec & r : run)
            r.row = row++;
        all.insert(all.end(), run.begin(), run.end());
        const uint32_t keep = (uint32_t)merge_cut(len, limit);
        cur.insert(cur.end(), run.begin(), run.begin() + keep);
        lens.push_back(keep);
    }
    std::stable_sort(all.begin(), all.end(), [](const Rec & x, const Rec & y) { return x.word < y.word; });
    for (const MergeRound & rd : merge_rounds(lens, limit))
    {
        std::vector<Rec> out(rd.out_rows);
        std::vector<uint32_t> splits(rd.n_splits);
        const uint32_t n_pairs = (uint32_t)rd.pairs.size();
        for (uint32_t s = 0; s < rd.n_splits; ++s)
        {
            const MergePair & p = rd.pairs[merge_pair_of<&MergePair::split_begin>(rd.pairs.data(), n_pairs, s)];
            const uint64_t edge = (uint64_t)(s - p.split_begin) * MRG_TILE;
            const uint32_t diag = edge < p.out_len ? (uint32_t)edge : p.out_len;
            splits[s] = merge_path(diag, p.a_len, p.b_len, [&](uint32_t bi, uint32_t ai) { return cur[p.b_begin + bi].word < cur[p.a_begin + ai].word; });
        }
        for (uint32_t g = 0; g < rd.n_tiles; ++g)
        {
            const MergePair & p = rd.pairs[merge_pair_of<&MergePair::tile_begin>(rd.pairs.data(), n_pairs, g)];
            const uint32_t k = g - p.tile_begin, d0 = k * MRG_TILE;
            CHECK(d0 < p.out_len);
            const uint32_t n = p.out_len - d0 < MRG_TILE ? p.out_len - d0 : MRG_TILE;
            const uint32_t a0 = splits[p.split_begin + k], a1 = splits[p.split_begin + k + 1];
            CHECK(a0 <= a1 && a1 - a0 <= n && a1 <= p.a_len);
            const uint32_t b0 = d0 - a0, na = a1 - a0, nb = n - na;
            CHECK(b0 + nb <= p.b_len);
            std::vector<Rec> lds(n);
            for (uint32_t e = 0; e < n; ++e)
                lds[e] = cur[e < na ? p.a_begin + a0 + e : p.b_begin + b0 + (e - na)];
            for (uint32_t tid = 0; tid < MRG_THREADS; ++tid)
            {
                const uint32_t d = tid * MRG_ITEMS < n ? tid * MRG_ITEMS : n;
                const uint32_t count = n - d < MRG_ITEMS ? n - d : MRG_ITEMS;
                uint32_t ai = merge_path(d, na, nb, [&](uint32_t bi, uint32_t ai_) { return lds[na + bi].word < lds[ai_].word; });
                uint32_t bi = d - ai;
                for (uint32_t i = 0; i < count; ++i)
                {
                    const bool take_b = bi < nb && (ai >= na || lds[na + bi].word < lds[ai].word);
                    out[p.out_begin + d0 + d + i] = take_b ? lds[na + bi] : lds[ai];
                    take_b ? ++bi : ++ai;
                }
            }
        }
        cur.swap(out);
    }
    if (lens0.size() > 1)
    {
        const size_t n_out = (size_t)merge_cut(all.size(), limit);
        CHECK(cur.size() == n_out);
        for (size_t i = 0; i < n_out; ++i)
            CHECK(cur[i].row == all[i].row && cur[i].word == all[i].word);
    }
}

static void test_tree()
{
    const uint32_t T = MRG_TILE;
    const uint64_t limits[] = {0, 1, T, T + 1, 5000};
    for (uint64_t limit : limits)
    {
        for (uint32_t range : {1u, 3u, 1000000u})
        {
            replay_tree({T - 1, T + 1}, range, limit);
            replay_tree({1, 3 * T}, range, limit);
            replay_tree({3 * T, 0}, range, limit);
            replay_tree({0, 65}, range, limit);
            replay_tree({63, 64, T, 0, 2, 1, 65, T + 1, 2 * T + 7}, range, limit);
            replay_tree({100, 200, 300, 400, 500}, range, limit);
        }
        std::vector<uint32_t> many(257);
        for (uint32_t r = 0; r < 257; ++r)
            many[r] = r % 5 == 2 ? 0 : (uint32_t)(rnd() % 40);
        replay_tree(many, 5, limit);
    }
}

static void test_plan()
{
    // the shapes of tests/test_gpu_merge_sorted.py::test_both_plans
    const uint32_t u8[1] = {1}, i64[1] = {8};
    CHECK(merge_plan(u8, 1, 64 * 300, 64 * 300, 64) == MERGE_PLAN_SORT);  // many runs over a narrow key: cheaper to sort again
    CHECK(merge_plan(i64, 1, 3 * 5000, 3 * 5000, 3) == MERGE_PLAN_TREE);
    // the byte model at the measured shapes: 64 runs of UInt8 re-sort (two runs merge), 2 to 1024 runs of Int64 merge
    CHECK(merge_plan(u8, 1, 100000000, 100000000, 2) == MERGE_PLAN_TREE && merge_plan(u8, 1, 100000000, 100000000, 3) == MERGE_PLAN_SORT);
    CHECK(merge_plan(i64, 1, 100000000, 100000000, 1024) == MERGE_PLAN_TREE);
    CHECK(merge_plan(u8, 1, 100000000, 100000000, 64) == MERGE_PLAN_SORT);
    CHECK(merge_plan(i64, 1, 100000000, 100000000, 2) == MERGE_PLAN_TREE);
    CHECK(merge_plan(i64, 1, 100000000, 100000000, 8) == MERGE_PLAN_TREE);
    // a limit leaves the tree almost nothing to move: the top 10 of 8 runs is 80 rows
    CHECK(merge_plan(u8, 1, 100000000, 80, 8) == MERGE_PLAN_TREE);
    const uint32_t two[2] = {4, 8};
    CHECK(merge_plan(two, 2, 100000000, 100000000, 8) == MERGE_PLAN_TREE);
    CHECK(merge_tree_bytes(8, 10, 2) == 10 * (8 + 12 + 24 + 12) && merge_sort_bytes(i64, 1, 10) == 10 * 9 * 2 * 16);
}

int main()
{
    test_offsets();
    test_rounds();
    test_merge_path();
    test_tree();
    test_plan();
    printf("merge_sorted_driver OK\n");
    return 0;
}
