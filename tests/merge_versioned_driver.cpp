// merge_versioned_driver.cpp — TEST INFRASTRUCTURE ONLY.  A stand-alone program (its own main, built with -fsanitize=address,undefined and
// run as a plain executable) that replays clickhouse_amd/csrc/merge_versioned_host.h the way merge_versioned_kernels.hip runs it -- a
// thread's items, the workgroup's forward and backward scans, the tile elements, the one-workgroup carry step in passes with a carry
// between them, the decision between the two carries with its masks, counts and largest balance, the exclusive offsets and the compacted
// stores -- tile by tile on the host, against a queue written here, over crafted and random groups.  Every scan is done with several
// splits (a sequential fold, the doubling steps of a wave scan, carry passes of 1, 3, 7 and FOLD_THREADS tiles) and all must agree.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../clickhouse_amd/csrc/merge_versioned_host.h"

typedef uint64_t u64;
typedef uint32_t u32;
typedef uint8_t u8;

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u64 rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

#define REQUIRE(cond)                                                      \
    do                                                                     \
    {                                                                      \
        if (!(cond))                                                       \
        {                                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

static bool same(const VcSum & a, const VcSum & b) { return a.sum == b.sum && a.head == b.head; }
static bool same(const VcAfter & a, const VcAfter & b) { return a.sum == b.sum && a.mn == b.mn && a.mx == b.mx && a.closed == b.closed; }

struct Forward
{
    typedef VcSum T;
    static T id() { return vc_sum_id(); }
    static T comb(const T & a, const T & b) { return vc_sum_combine(a, b); }
};
// over an array turned round: what the scan met earlier lies later in M
struct Backward
{
    typedef VcAfter T;
    static T id() { return vc_after_id(); }
    static T comb(const T & a, const T & b) { return vc_after_combine(b, a); }
};

// the exclusive scan of v in passes of `pass` elements with a carry between them; inside a pass the doubling steps of the device's scan
template <class Op>
static std::vector<typename Op::T> scan_exclusive(const std::vector<typename Op::T> & v, size_t pass, typename Op::T * total)
{
    typedef typename Op::T T;
    std::vector<T> out(v.size());
    T carry = Op::id();
    for (size_t base = 0; base < v.size(); base += pass)
    {
        const size_t m = v.size() - base < pass ? v.size() - base : pass;
        std::vector<T> inc(v.begin() + base, v.begin() + base + m);
        for (size_t d = 1; d < m; d <<= 1)
        {
            std::vector<T> next = inc;
            for (size_t i = d; i < m; ++i)
                next[i] = Op::comb(inc[i - d], inc[i]);
            inc.swap(next);
        }
        for (size_t i = 0; i < m; ++i)
            out[base + i] = i ? Op::comb(carry, inc[i - 1]) : carry;
        carry = Op::comb(carry, inc[m - 1]);
    }
    // the same by a plain fold
    T run = Op::id();
    for (size_t i = 0; i < v.size(); ++i)
    {
        REQUIRE(same(out[i], run));
        run = Op::comb(run, v[i]);
    }
    REQUIRE(same(run, carry));
    *total = carry;
    return out;
}

template <class T>
static std::vector<T> turned(std::vector<T> v)
{
    for (size_t i = 0, j = v.size(); i + 1 < j; ++i, --j)
        std::swap(v[i], v[j - 1]);
    return v;
}

struct Input
{
    std::vector<u8> heads;
    std::vector<u32> rows;      // a permutation: the merged order
    std::vector<int8_t> sign;   // by row
};

// groups of the given lengths; signs[p] is the sign at merged position p
static Input input_of(const std::vector<u32> & group_lens, const std::vector<int8_t> & signs)
{
    Input in;
    for (u32 len : group_lens)
        for (u32 i = 0; i < len; ++i)
            in.heads.push_back(i == 0);
    const u32 n = (u32)in.heads.size();
    REQUIRE(signs.size() == n);
    in.rows.resize(n);
    for (u32 i = 0; i < n; ++i)
        in.rows[i] = i;
    for (u32 i = n; i > 1; --i)
        std::swap(in.rows[i - 1], in.rows[rnd() % i]);
    in.sign.assign(n + 1, 0);
    for (u32 p = 0; p < n; ++p)
        in.sign[in.rows[p]] = signs[p];
    return in;
}

struct Result
{
    std::vector<u64> rows;
    u64 max_balance = 0;
};

// the reference's loop with an unbounded queue
static Result queue_of(const Input & in)
{
    Result r;
    std::vector<u32> queue;
    int sign_in_queue = 0;
    for (size_t p = 0; p < in.heads.size(); ++p)
    {
        if (in.heads[p])
        {
            r.rows.insert(r.rows.end(), queue.begin(), queue.end());
            queue.clear();
        }
        const u32 row = in.rows[p];
        if (queue.empty())
        {
            sign_in_queue = in.sign[row];
            queue.push_back(row);
        }
        else if (in.sign[row] == sign_in_queue)
            queue.push_back(row);
        else
            queue.pop_back();
        r.max_balance = queue.size() > r.max_balance ? queue.size() : r.max_balance;
    }
    r.rows.insert(r.rows.end(), queue.begin(), queue.end());
    return r;
}

// the kernels' sequence; carry_pass: the tiles one pass of the one-workgroup step takes
static Result replay(const Input & in, size_t carry_pass)
{
    const u64 n = in.heads.size();
    const u32 tiles = merge_tiles((u32)n);
    Result r;
    if (!n)
        return r;
    std::vector<VcItems> items((size_t)tiles * FOLD_THREADS);
    std::vector<VcSum> agg_f(tiles), before((size_t)tiles * FOLD_THREADS);
    std::vector<VcAfter> agg_g(tiles), after((size_t)tiles * FOLD_THREADS);
    for (u32 tile = 0; tile < tiles; ++tile)  // k_vc_tile (and the scans k_vc_decide does again)
    {
        std::vector<VcSum> f(FOLD_THREADS);
        std::vector<VcAfter> g(FOLD_THREADS);
        for (u32 t = 0; t < FOLD_THREADS; ++t)
        {
            const size_t slot = (size_t)tile * FOLD_THREADS + t;
            u64 p0, p1;
            fold_thread_range(tile, t, n, p0, p1);
            items[slot] = vc_items_load(in.heads.data(), in.rows.data(), in.sign.data(), p0, n);
            vc_aggregate(items[slot], f[t], g[t]);
        }
        const std::vector<VcSum> bf = scan_exclusive<Forward>(f, 64, &agg_f[tile]);
        const std::vector<VcAfter> ag = turned(scan_exclusive<Backward>(turned(g), 64, &agg_g[tile]));
        for (u32 t = 0; t < FOLD_THREADS; ++t)
        {
            before[(size_t)tile * FOLD_THREADS + t] = bf[t];
            after[(size_t)tile * FOLD_THREADS + t] = ag[t];
        }
    }
    VcSum all_f;
    VcAfter all_g;
    const std::vector<VcSum> carry_f = scan_exclusive<Forward>(agg_f, carry_pass, &all_f);  // k_vc_carry
    const std::vector<VcAfter> carry_g = turned(scan_exclusive<Backward>(turned(agg_g), carry_pass, &all_g));
    std::vector<u8> masks((size_t)tiles * FOLD_THREADS);
    std::vector<u64> off(tiles + 1, 0);
    for (u32 tile = 0; tile < tiles; ++tile)  // k_vc_decide, k_vc_offsets
    {
        u32 count = 0;
        for (u32 t = 0; t < FOLD_THREADS; ++t)
        {
            const size_t slot = (size_t)tile * FOLD_THREADS + t;
            const u32 mask = vc_decide(items[slot], vc_sum_combine(carry_f[tile], before[slot]), vc_after_combine(after[slot], carry_g[tile]), &r.max_balance);
            REQUIRE(mask < (1u << items[slot].count));
            masks[slot] = (u8)mask;
            count += (u32)__builtin_popcount(mask);
        }
        REQUIRE(count <= FOLD_TILE);
        off[tile + 1] = off[tile] + count;
    }
    r.rows.assign(off[tiles], ~0ull);
    for (u32 tile = 0; tile < tiles; ++tile)  // k_vc_emit
    {
        u64 at = off[tile];
        for (u32 t = 0; t < FOLD_THREADS; ++t)
        {
            u64 p0, p1;
            fold_thread_range(tile, t, n, p0, p1);
            for (u32 i = 0; i < FOLD_ITEMS; ++i)
                if ((masks[(size_t)tile * FOLD_THREADS + t] >> i) & 1)
                    r.rows[at++] = in.rows[p0 + i];
        }
        REQUIRE(at == off[tile + 1]);
    }
    return r;
}

// pattern 0 .. 7 for a group of `len` rows
static void pattern(std::vector<int8_t> & out, u32 len, int kind)
{
    for (u32 i = 0; i < len; ++i)
    {
        int s = 1;
        switch (kind)
        {
            case 0: s = 1; break;
            case 1: s = -1; break;
            case 2: s = i % 2 ? -1 : 1; break;
            case 3: s = i % 2 ? 1 : -1; break;
            case 4: s = i < len / 2 ? 1 : -1; break;                         // + ^ k  - ^ k
            case 5: s = i < (len > 3 ? (len - 3) / 2 : 0) ? -1 : 1; break;   // - ^ k  + ^ (k + 3)
            case 6: s = rnd() % 2 ? 1 : -1; break;
            default: s = rnd() % 10 ? 1 : -1; break;
        }
        out.push_back((int8_t)s);
    }
}

static u32 check(const std::vector<u32> & lens, int kind, bool every_pass)
{
    std::vector<int8_t> signs;
    for (u32 len : lens)
        pattern(signs, len, kind < 0 ? (int)(rnd() % 8) : kind);
    const Input in = input_of(lens, signs);
    const Result want = queue_of(in);
    u32 cases = 0;
    for (size_t pass : {(size_t)FOLD_THREADS, (size_t)1, (size_t)3, (size_t)7})
    {
        const Result got = replay(in, pass);
        REQUIRE(got.rows == want.rows);
        REQUIRE(got.max_balance == want.max_balance);
        cases += 1;
        if (!every_pass)
            break;
    }
    return cases;
}

int main()
{
    const u32 T = FOLD_TILE;
    // 64 bits in every state: a group of 2^32 - 1 rows of one sign
    static_assert(sizeof(VcSum::sum) == 8 && sizeof(VcAfter::sum) == 8 && sizeof(VcAfter::mn) == 8 && sizeof(VcAfter::mx) == 8, "balances are 64 bits wide");
    {
        const int64_t big = 0xFFFFFFFFll - 1;
        REQUIRE(vc_sum_combine(VcSum{big, 1}, VcSum{1, 0}).sum == 0xFFFFFFFFll);
        REQUIRE(vc_sum_combine(VcSum{-big, 0}, VcSum{-1, 0}).sum == -0xFFFFFFFFll);
        const VcAfter a = vc_after_combine(VcAfter{-big, -big, 0, 0}, VcAfter{-1, -1, 0, 1});
        REQUIRE(a.sum == -0xFFFFFFFFll && a.mn == -0xFFFFFFFFll && a.mx == 0 && a.closed == 1);
        REQUIRE(vc_abs(-0xFFFFFFFFll) == 0xFFFFFFFFull && vc_abs(INT64_MIN) == 0x8000000000000000ull);
        REQUIRE(vc_survives(1, 0xFFFFFFFFll, vc_after_id()) && !vc_survives(1, 0, vc_after_id()) && vc_survives(-1, -1, vc_after_id()));
        REQUIRE(!vc_survives(1, 5, VcAfter{0, -1, 0, 0}) && vc_survives(-1, -5, VcAfter{-2, -2, 0, 0}) && !vc_survives(-1, -5, VcAfter{0, 0, 1, 0}));
    }
    u32 cases = 0;
    const std::vector<std::vector<u32>> layouts = {
        {}, {1}, {2}, {1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3, 1, 2}, {T, T}, {T - 1, 1, T, 1}, {T + 1, T - 1, 3}, {3, 3 * T, 3 * T - 3, 9},
        std::vector<u32>(T + 3, 1), std::vector<u32>(2 * T, 2), {5 * T + 7}};
    for (const std::vector<u32> & lens : layouts)
        for (int kind = -1; kind < 8; ++kind)
            cases += check(lens, kind, true);
    // hand-written groups, each also behind a stretch that moves it across a tile edge
    for (const char * text : {"+", "-", "+-", "-+", "++-", "+--+", "--+++", "+++--", "+-++-+"})
        for (u32 lead : {0u, T - 1, T - 2, 2 * T - 3})
        {
            std::vector<u32> lens;
            std::vector<int8_t> signs(lead, 1);
            if (lead)
                lens.push_back(lead);
            u32 len = 0;
            for (const char * c = text; *c; ++c, ++len)
                signs.push_back(*c == '+' ? 1 : -1);
            lens.push_back(len);
            const Input in = input_of(lens, signs);
            const Result want = queue_of(in), got = replay(in, FOLD_THREADS);
            REQUIRE(got.rows == want.rows && got.max_balance == want.max_balance);
            cases += 1;
        }
    // a + whose - is the first row of the next tile; one whose - is three tiles later with a balanced stretch between
    {
        std::vector<int8_t> signs(T - 1, -1);
        signs.push_back(1), signs.push_back(-1);
        std::vector<u32> lens = {T - 1, 2};
        Input in = input_of(lens, signs);
        REQUIRE(replay(in, 3).rows == queue_of(in).rows && queue_of(in).rows.size() == T - 1);
        signs.assign(1, 1);
        for (u32 i = 0; i < 3 * T / 2; ++i)
            signs.push_back(1), signs.push_back(-1);
        signs.push_back(-1), signs.push_back(1);
        lens = {3 * T + 3};
        in = input_of(lens, signs);
        const Result got = replay(in, 1);
        REQUIRE(got.rows == queue_of(in).rows && got.rows.size() == 1 && got.rows[0] == in.rows[3 * T + 2] && got.max_balance == 2);
        cases += 2;
    }
    // random groups of geometric length, and more tiles than one pass of the carry step takes
    for (int round = 0; round < 6; ++round)
    {
        std::vector<u32> lens;
        for (u32 rows = 0; rows < 6 * T + 100;)
        {
            u32 len = 1;
            while (rnd() % 40)
                ++len;
            lens.push_back(len);
            rows += len;
        }
        cases += check(lens, -1, true);
    }
    cases += check({(FOLD_THREADS + 40) * T + 11, 5, 3 * T}, 6, false);
    cases += check({(FOLD_THREADS + 2) * T + 5}, 7, false);
    std::printf("merge_versioned_driver OK (%u cases)\n", cases);
    return 0;
}
