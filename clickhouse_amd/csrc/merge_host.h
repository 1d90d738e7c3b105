// merge_host.h — the parts of the merge of sorted runs (merge_kernels.hip) that need no device: the validation of the run offsets, the
// run list of every round of the pairwise merge tree (with the pass-through run and the limit cut), the table that maps an output tile
// to its pair, the merge-path search and the choice between the merge tree and a re-sort.  Plain C++ (the functions the kernels share
// are __host__ __device__ under hipcc), so that tests/merge_sorted_driver.cpp runs the very code the kernels run under a sanitizer.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/chgpu.h"

#ifdef __HIPCC__
#define MRG_HD __host__ __device__ __forceinline__
#else
#define MRG_HD static inline
#endif

// row numbers travel as UInt32 next to the key word
static constexpr uint64_t MRG_MAX_ROWS = 0xFFFFFFFFull;
static constexpr uint32_t MRG_THREADS = 256;                   // threads of a tile kernel
static constexpr uint32_t MRG_ITEMS = 8;                       // consecutive outputs a thread merges
static constexpr uint32_t MRG_TILE = MRG_THREADS * MRG_ITEMS;  // T: outputs of one merge tile
static constexpr uint32_t MRG_MAX_KEYS = 8;

enum { MERGE_PLAN_TREE = 0, MERGE_PLAN_SORT = 1 };

// run_offsets: n_runs + 1 cumulative entries that start at 0 and never decrease.  CHGPU_OK and *rows = run_offsets[n_runs] (0 without
// runs), or the code with *msg saying why.
static inline int merge_check_offsets(const uint64_t * run_offsets, uint32_t n_runs, uint64_t * rows, const char ** msg)
{
    *rows = 0;
    if (!run_offsets)
        return *msg = "NULL run offsets", CHGPU_ERR_BAD_ARGUMENTS;
    if (run_offsets[0] != 0)
        return *msg = "run offsets do not start at 0", CHGPU_ERR_BAD_ARGUMENTS;
    for (uint32_t r = 0; r < n_runs; ++r)
        if (run_offsets[r + 1] < run_offsets[r])
            return *msg = "run offsets decrease", CHGPU_ERR_BAD_ARGUMENTS;
    *rows = run_offsets[n_runs];
    if (*rows > MRG_MAX_ROWS)
        return *msg = "2^32 rows or more are not implemented (row numbers travel as UInt32)", CHGPU_ERR_NOT_IMPLEMENTED;
    return CHGPU_OK;
}

// One pairwise merge of a round: the left run [a_begin, a_begin + a_len) and the right run [b_begin, ..) of the round's input arrays
// give the first out_len entries of their merge at [out_begin, ..) of its output arrays, in the tiles [tile_begin, next pair's).
// The kernels read this struct from a device table as it stands.
struct MergePair
{
    uint32_t a_begin, a_len, b_begin, b_len, out_begin, out_len, tile_begin, split_begin;
};

struct MergeRound
{
    std::vector<MergePair> pairs;
    uint32_t n_tiles = 0;   // all pairs' tiles: ONE tile launch
    uint32_t n_splits = 0;  // n_tiles + pairs (a pair of k tiles has k + 1 tile edges): ONE split launch
    uint32_t out_rows = 0;
};

static inline uint32_t merge_tiles(uint32_t rows) { return rows / MRG_TILE + (rows % MRG_TILE != 0); }
static inline uint64_t merge_cut(uint64_t len, uint64_t limit) { return limit && len > limit ? limit : len; }

// The run lengths the tree starts from: every run cut to its first `limit` rows (only they can reach the first `limit` outputs)
static inline std::vector<uint32_t> merge_initial_runs(const uint64_t * run_offsets, uint32_t n_runs, uint64_t limit)
{
    std::vector<uint32_t> lens(n_runs);
    for (uint32_t r = 0; r < n_runs; ++r)
        lens[r] = (uint32_t)merge_cut(run_offsets[r + 1] - run_offsets[r], limit);
    return lens;
}

// One round over the run lengths `lens` (runs lie back to back in the input arrays, and so do the outputs): runs 2j and 2j + 1 merge,
// an odd last run passes through as a pair with an empty right side; every output run is cut to `limit`.  *out_lens: the next round's.
static inline MergeRound merge_round(const std::vector<uint32_t> & lens, uint64_t limit, std::vector<uint32_t> * out_lens)
{
    MergeRound rd;
    out_lens->clear();
    uint32_t in_pos = 0, out_pos = 0;
    for (size_t j = 0; j < lens.size(); j += 2)
    {
        MergePair p{};
        p.a_begin = in_pos;
        p.a_len = lens[j];
        p.b_begin = in_pos + p.a_len;
        p.b_len = j + 1 < lens.size() ? lens[j + 1] : 0;
        in_pos = p.b_begin + p.b_len;
        p.out_begin = out_pos;
        p.out_len = (uint32_t)merge_cut((uint64_t)p.a_len + p.b_len, limit);
        out_pos += p.out_len;
        p.tile_begin = rd.n_tiles;
        p.split_begin = rd.n_tiles + (uint32_t)rd.pairs.size();
        rd.n_tiles += merge_tiles(p.out_len);
        rd.pairs.push_back(p);
        out_lens->push_back(p.out_len);
    }
    rd.n_splits = rd.n_tiles + (uint32_t)rd.pairs.size();
    rd.out_rows = out_pos;
    return rd;
}

// every round until one run is left (none for 0 or 1 runs)
static inline std::vector<MergeRound> merge_rounds(std::vector<uint32_t> lens, uint64_t limit)
{
    std::vector<MergeRound> rounds;
    while (lens.size() > 1)
    {
        std::vector<uint32_t> next;
        rounds.push_back(merge_round(lens, limit, &next));
        lens.swap(next);
    }
    return rounds;
}

static inline uint32_t merge_round_count(uint32_t n_runs)
{
    uint32_t t = 0;
    for (uint64_t k = 1; k < n_runs; k *= 2)
        t += 1;
    return t;
}

// The pair of tile `tile` (FIELD = tile_begin) or of tile edge `split` (FIELD = split_begin): the last pair that begins at or before
// it.  Pairs without tiles share their begin with the next pair and are never the answer for a tile; a tile edge always has one.
template <uint32_t MergePair::*FIELD>
MRG_HD uint32_t merge_pair_of(const MergePair * pairs, uint32_t n_pairs, uint32_t x)
{
    uint32_t lo = 0, hi = n_pairs; // pairs[lo].*FIELD <= x < pairs[hi].*FIELD (hi == n_pairs: +inf)
    while (hi - lo > 1)
    {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pairs[mid].*FIELD <= x)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// Merge path: how many of the first `diag` outputs of the stable merge of A (na elements) and B (nb) come from A.
// b_before_a(bi, ai) says whether B[bi] orders STRICTLY before A[ai].
// INVARIANT (the stability of the whole tree rests on it): where the two are equal on every column the element of the LEFT run goes
// first.  Every row of a left run has a lower concatenated row number than any row of its right run -- runs are merged with their
// neighbours only, in order -- so "left first" IS "lower row number first", SortCursor's tie on `order`.
template <typename BeforeFn>
MRG_HD uint32_t merge_path(uint32_t diag, uint32_t na, uint32_t nb, BeforeFn b_before_a)
{
    uint32_t lo = diag > nb ? diag - nb : 0, hi = diag < na ? diag : na;
    while (lo < hi)
    {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (!b_before_a(diag - 1 - mid, mid))
            lo = mid + 1; // A[mid] goes before B[diag - 1 - mid]: it is among the first diag outputs
        else
            hi = mid;
    }
    return lo;
}

// The byte model.  A merge round reads and writes a (u64 word, u32 row) pair per row, the key build reads the first column and writes
// the pair, the last step writes the u64 permutation; a radix sort of the concatenation reads and writes (key + u64 row) once per key
// byte of every column, after a key pass of the same size.  Only the rows that survive the limit cut enter the tree; the sort takes
// them all.  Gathers of the later columns on first-word ties are not in the model (measured: DESIGN 4.26).
static inline uint64_t merge_tree_bytes(uint32_t first_key_size, uint64_t cut_rows, uint32_t n_runs)
{
    return cut_rows * (first_key_size + 12ull + 24ull * merge_round_count(n_runs) + 12ull);
}
static inline uint64_t merge_sort_bytes(const uint32_t * key_sizes, uint32_t n_keys, uint64_t rows)
{
    uint64_t per_row = 0;
    for (uint32_t j = 0; j < n_keys; ++j)
        per_row += (uint64_t)(key_sizes[j] + 1) * 2 * (key_sizes[j] + 8);
    return rows * per_row;
}
// Measured (DESIGN 4.26, 10^8 rows): the tree moves its model bytes at the rate of a column copy, the radix sort's partition passes move
// theirs at half of it, so a byte of the sort's model costs two of the tree's.
static constexpr uint64_t MRG_SORT_BYTE_COST = 2;
// ONE place decides: MERGE_PLAN_TREE or MERGE_PLAN_SORT (chgpu_sort_permutation from the last key column to the first).  Both give
// the same permutation.
static inline int merge_plan(const uint32_t * key_sizes, uint32_t n_keys, uint64_t rows, uint64_t cut_rows, uint32_t n_runs)
{
    return merge_tree_bytes(key_sizes[0], cut_rows, n_runs) <= MRG_SORT_BYTE_COST * merge_sort_bytes(key_sizes, n_keys, rows) ? MERGE_PLAN_TREE : MERGE_PLAN_SORT;
}
