// merge_fold_driver.cpp — TEST INFRASTRUCTURE ONLY.  A stand-alone program (its own main, built with -fsanitize=address,undefined and run
// as a plain executable) that replays the fold of clickhouse_amd/csrc/merge_fold_host.h the way merge_fold_kernels.hip runs it -- thread
// elements, the workgroup's segmented scan, tile aggregates, the one-workgroup carry step over chunks of tiles, the apply behind the
// carries with its tail counts, the exclusive offsets and the compacted stores -- tile by tile on the host, against a sequential loop
// over the merged positions, for Replacing, Collapsing and Folding on the group extents the GPU tests use.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../clickhouse_amd/csrc/merge_fold_host.h"

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

struct Layout
{
    std::vector<u8> heads;
    std::vector<u32> rows;  // a permutation: the merged order
};

static Layout layout_of(const std::vector<u32> & group_lens)
{
    Layout l;
    for (u32 len : group_lens)
        for (u32 i = 0; i < len; ++i)
            l.heads.push_back(i == 0);
    const u32 n = (u32)l.heads.size();
    l.rows.resize(n);
    for (u32 i = 0; i < n; ++i)
        l.rows[i] = i;
    for (u32 i = n; i > 1; --i)
    {
        const u32 j = (u32)(rnd() % i);
        std::swap(l.rows[i - 1], l.rows[j]);
    }
    return l;
}

// the workgroup's inclusive scan, step by step as fold_block_scan does it
template <class A>
static void block_scan(const A & a, std::vector<typename A::State> & s, std::vector<u8> & f)
{
    for (u32 d = 1; d < FOLD_THREADS; d <<= 1)
    {
        std::vector<typename A::State> ns = s;
        std::vector<u8> nf = f;
        for (u32 t = d; t < FOLD_THREADS; ++t)
        {
            typename A::State ps = s[t - d];
            u8 pf = f[t - d];
            fold_seg_combine(a, ps, pf, s[t], f[t]);
            ns[t] = ps;
            nf[t] = pf;
        }
        s.swap(ns);
        f.swap(nf);
    }
}

template <class A>
static void tile_scan(const A & a, const Layout & l, u32 tile, std::vector<typename A::State> & s, std::vector<u8> & f)
{
    const u64 n = l.heads.size();
    s.assign(FOLD_THREADS, typename A::State{});
    f.assign(FOLD_THREADS, 0);
    for (u32 t = 0; t < FOLD_THREADS; ++t)
    {
        u64 p0, p1;
        fold_thread_range(tile, t, n, p0, p1);
        fold_aggregate(a, FoldColumns<A>{a, l.heads.data(), l.rows.data(), n}, p0, p1, s[t], f[t]);
    }
    block_scan(a, s, f);
}

struct Emitted
{
    std::vector<u64> out0, out1;
};

// the kernels' sequence; make_a(outputs) gives the algorithm with its result columns sized for `outputs` rows
template <class A, class MakeA>
static Emitted replay(const Layout & l, MakeA make_a)
{
    typedef typename A::State State;
    const u64 n = l.heads.size();
    const u32 tiles = merge_tiles((u32)n);
    Emitted e;
    A a = make_a(0);
    if (!n)
        return e;
    std::vector<State> agg_s(tiles), carry(tiles), s;
    std::vector<u8> agg_f(tiles), f;
    for (u32 tile = 0; tile < tiles; ++tile)  // k_fold_tile
    {
        tile_scan(a, l, tile, s, f);
        agg_s[tile] = s[FOLD_THREADS - 1];
        agg_f[tile] = f[FOLD_THREADS - 1];
    }
    {  // k_fold_carry
        std::vector<State> cs(FOLD_THREADS, State{});
        std::vector<u8> cf(FOLD_THREADS, 0);
        for (u32 t = 0; t < FOLD_THREADS; ++t)
            fold_chunk_aggregate(a, agg_s.data(), agg_f.data(), fold_chunk_begin(t, tiles), fold_chunk_begin(t + 1, tiles), cs[t], cf[t]);
        REQUIRE(fold_chunk_begin(FOLD_THREADS, tiles) == tiles);
        block_scan(a, cs, cf);
        for (u32 t = 0; t < FOLD_THREADS; ++t)
            fold_chunk_carries(a, agg_s.data(), agg_f.data(), fold_chunk_begin(t, tiles), fold_chunk_begin(t + 1, tiles), t ? cs[t - 1] : State{}, t ? cf[t - 1] : (u8)0,
                               carry.data());
    }
    std::vector<u32> counts(tiles, 0);
    std::vector<u64> off(tiles + 1, 0);
    for (int pass = 0; pass < 2; ++pass)  // k_fold_apply<false>, k_fold_offsets, k_fold_apply<true>
    {
        for (u32 tile = 0; tile < tiles; ++tile)
        {
            tile_scan(a, l, tile, s, f);
            u32 at = 0;
            for (u32 t = 0; t < FOLD_THREADS; ++t)
            {
                State ps{};
                u8 pf = 0;
                if (tile)
                {
                    ps = carry[tile];
                    pf = FOLD_ANY;
                }
                if (t)
                    fold_seg_combine(a, ps, pf, s[t - 1], f[t - 1]);
                u64 p0, p1;
                fold_thread_range(tile, t, n, p0, p1);
                fold_apply(a, FoldColumns<A>{a, l.heads.data(), l.rows.data(), n}, p0, p1, ps, pf, [&](u64, const State & st, u32 c, const u32 * o) {
                    REQUIRE(c <= FOLD_MAX_OUT);
                    if (pass && c)
                    {
                        if (A::PAIRED)
                        {
                            e.out0[off[tile] + at] = o[0];
                            e.out1[off[tile] + at] = o[1];
                            a.store(st, off[tile] + at);
                        }
                        else
                            for (u32 j = 0; j < c; ++j)
                                e.out0[off[tile] + at + j] = o[j];
                    }
                    at += c;
                });
            }
            if (!pass)
                counts[tile] = at;
            else
                REQUIRE(at == counts[tile]);
        }
        if (!pass)
        {
            for (u32 tile = 0; tile < tiles; ++tile)
                off[tile + 1] = off[tile] + counts[tile];
            e.out0.assign(off[tiles], ~0ull);
            if (A::PAIRED)
                e.out1.assign(off[tiles], ~0ull);
            a = make_a(off[tiles]);
        }
    }
    return e;
}

static std::vector<std::vector<u32>> layouts()
{
    const u32 T = FOLD_TILE;
    std::vector<std::vector<u32>> ls = {
        {}, {1}, {1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5, 1, 2}, {5 * T + 7}, {T, T}, {T - 1, 1, T, 1}, {T + 1, T - 1, 3}, {3, 3 * T, 3 * T - 3, 9},
        std::vector<u32>(T + 3, 1), std::vector<u32>(2 * T, 2)};
    std::vector<u32> mixed;
    for (u32 i = 0; i < 3000; ++i)
        mixed.push_back(1 + (u32)(rnd() % 9));
    ls.push_back(mixed);
    // more tiles than threads of the carry step: chunks of two tiles
    ls.push_back({(FOLD_THREADS + 40) * T + 11, 5, 3 * T});
    return ls;
}

static void check_replacing(const Layout & l, int variant)
{
    const u32 n = (u32)l.heads.size();
    std::vector<int64_t> ver(n + 1);
    std::vector<u8> del(n + 1);
    for (u32 i = 0; i < n; ++i)
    {
        const u64 r = rnd() % 7;
        ver[i] = r == 0 ? INT64_MIN : r == 1 ? INT64_MAX : (int64_t)(rnd() % 3) - 1;
        del[i] = (u8)(rnd() % 2);
    }
    ReplacingFold a;
    a.version = variant ? ver.data() : nullptr;
    a.version_type = CHGPU_I64;
    a.is_deleted = variant == 2 ? del.data() : nullptr;
    a.cleanup = variant == 2;
    const Emitted e = replay<ReplacingFold>(l, [&](u64) { return a; });
    std::vector<u64> want;
    for (u32 p = 0; p < n;)
    {
        u32 q = p, sel = l.rows[p];
        for (; q < n && (q == p || !l.heads[q]); ++q)
            if (!variant || ver[l.rows[q]] >= ver[sel])
                sel = l.rows[q];
        if (!(variant == 2 && del[sel] == 1))
            want.push_back(sel);
        p = q;
    }
    REQUIRE(e.out0 == want);
}

static void check_collapsing(const Layout & l, int variant)
{
    const u32 n = (u32)l.heads.size();
    std::vector<int8_t> sign(n + 1);
    for (u32 i = 0; i < n; ++i)
        sign[i] = variant == 0 ? (rnd() % 2 ? 1 : -1) : variant == 1 ? (i % 2 ? 1 : -1) : (rnd() % 16 ? 1 : -1);
    CollapsingFold a;
    a.sign = sign.data();
    const Emitted e = replay<CollapsingFold>(l, [&](u64) { return a; });
    std::vector<u64> want;
    for (u32 p = 0; p < n;)
    {
        u32 q = p, cp = 0, cn = 0, first_negative = 0, last_positive = 0;
        bool last_is_positive = false;
        for (; q < n && (q == p || !l.heads[q]); ++q)
        {
            const u32 row = l.rows[q];
            if (sign[row] == 1)
                ++cp, last_positive = row, last_is_positive = true;
            else
            {
                if (!cn)
                    first_negative = row;
                ++cn, last_is_positive = false;
            }
        }
        if (last_is_positive || cp != cn)
        {
            if (cp <= cn)
                want.push_back(first_negative);
            if (cp >= cn)
                want.push_back(last_positive);
        }
        p = q;
    }
    REQUIRE(e.out0 == want);
}

template <u32 NV>
static void check_folding(const Layout & l, bool drop_zero)
{
    const u32 n = (u32)l.heads.size();
    std::vector<int8_t> v0(n + 1);
    std::vector<u64> v1(n + 1);
    std::vector<int32_t> v2(n + 1);
    for (u32 i = 0; i < n; ++i)
    {
        v0[i] = (int8_t)(rnd() % 5 == 0 ? 127 : (int)(rnd() % 3) - 1);
        v1[i] = rnd() % 4 == 0 ? ~0ull : rnd() % 3;
        v2[i] = rnd() % 9 == 0 ? INT32_MIN : (int32_t)rnd();
    }
    const void * data[3] = {v0.data(), v1.data(), v2.data()};
    const int type[3] = {CHGPU_I8, CHGPU_U64, CHGPU_I32};
    const int kind[3] = {CHGPU_FOLD_SUM, NV == 2 ? CHGPU_FOLD_SUM : CHGPU_FOLD_MAX, CHGPU_FOLD_MIN};
    std::vector<int8_t> r0;
    std::vector<u64> r1;
    std::vector<int32_t> r2;
    const Emitted e = replay<FoldingFold<NV>>(l, [&](u64 outputs) {
        r0.assign(outputs + 1, 0), r1.assign(outputs + 1, 0), r2.assign(outputs + 1, 0);
        FoldingFold<NV> a;
        a.d = FoldValues{};
        a.d.n = NV;
        a.d.drop_zero = drop_zero;
        void * out[3] = {r0.data(), r1.data(), r2.data()};
        for (u32 k = 0; k < NV; ++k)
            a.d.data[k] = data[k], a.d.out[k] = out[k], a.d.type[k] = type[k], a.d.kind[k] = kind[k];
        return a;
    });
    std::vector<u64> first, last, w1;
    std::vector<int8_t> w0;
    std::vector<int32_t> w2;
    for (u32 p = 0; p < n;)
    {
        u32 q = p;
        uint8_t s0 = 0;
        u64 s1 = 0;  // the sum's and the unsigned maximum's start
        int32_t s2 = INT32_MAX;
        for (; q < n && (q == p || !l.heads[q]); ++q)
        {
            const u32 row = l.rows[q];
            s0 = (uint8_t)(s0 + (uint8_t)v0[row]);
            s1 = kind[1] == CHGPU_FOLD_SUM ? s1 + v1[row] : (v1[row] > s1 ? v1[row] : s1);
            s2 = v2[row] < s2 ? v2[row] : s2;
        }
        bool zero = NV > 0 && s0 == 0;
        if (NV >= 2 && kind[1] == CHGPU_FOLD_SUM && s1 != 0)
            zero = false;
        if (!(drop_zero && zero))
        {
            first.push_back(l.rows[p]), last.push_back(l.rows[q - 1]);
            w0.push_back((int8_t)s0), w1.push_back(s1), w2.push_back(s2);
        }
        p = q;
    }
    REQUIRE(e.out0 == first && e.out1 == last);
    r0.resize(first.size()), r1.resize(first.size()), r2.resize(first.size());
    if (NV >= 1)
        REQUIRE(r0 == w0);
    if (NV >= 2)
        REQUIRE(r1 == w1);
    if (NV >= 3)
        REQUIRE(r2 == w2);
}

int main()
{
    // the order word of a version and the wrap of a narrow sum
    REQUIRE(fold_order_word((u64)INT64_MIN, CHGPU_I64) == 0 && fold_order_word(~0ull, CHGPU_U64) == ~0ull);
    REQUIRE(fold_order_word(fold_order_word((u64)-5, CHGPU_I8), CHGPU_I8) == (u64)-5);
    REQUIRE(fold_chunk_begin(0, 0) == 0 && fold_chunk_begin(1, 1) == 1 && fold_chunk_begin(256, 257) == 257 && fold_chunk_begin(1, 257) == 2);
    u32 cases = 0;
    for (const std::vector<u32> & lens : layouts())
    {
        const Layout l = layout_of(lens);
        for (int variant = 0; variant < 3; ++variant)
        {
            check_replacing(l, variant);
            check_collapsing(l, variant);
            cases += 2;
        }
        check_folding<0>(l, true);
        check_folding<1>(l, true);
        check_folding<2>(l, true);
        check_folding<3>(l, true);
        check_folding<3>(l, false);
        cases += 5;
    }
    std::printf("merge_fold_driver OK (%u cases)\n", cases);
    return 0;
}
