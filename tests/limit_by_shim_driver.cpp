// GpuDistinctTransform / GpuLimitByTransform (clickhouse_amd/host/chgpu_shim.hpp) driven as a chain over host chunks and checked
// against plain host loops: one key column, two packed key columns, three wide ones through the dictionary, the drop of an empty chunk,
// the pass-through of a full one and DISTINCT's limit_hint.  Built and run by tests/test_gpu_limit_by.py; prints "limit_by_shim_driver OK".
#include "../clickhouse_amd/host/chgpu_shim.hpp"

#include <array>
#include <cstdio>
#include <cstdlib>
#include <map>

using namespace chgpu;

#define REQUIRE(cond)                                                        \
    do                                                                       \
    {                                                                        \
        if (!(cond))                                                         \
        {                                                                    \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

struct HostChunk
{
    std::vector<uint64_t> a, b;
    std::vector<uint32_t> c;
    std::vector<int64_t> payload;
};

static uint64_t next_random(uint64_t & s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 33;
}

static std::vector<HostChunk> make_chunks(size_t n_chunks, size_t rows, uint64_t domain, uint64_t seed)
{
    std::vector<HostChunk> out(n_chunks);
    int64_t serial = 0;
    for (HostChunk & h : out)
        for (size_t i = 0; i < rows; ++i)
        {
            h.a.push_back(next_random(seed) % domain);
            h.b.push_back((next_random(seed) % 3) << 40);
            h.c.push_back(static_cast<uint32_t>(next_random(seed) % 2));
            h.payload.push_back(serial++);
        }
    return out;
}

static Chunk upload(const ContextPtr & ctx, const HostChunk & h)
{
    Chunk c;
    c.columns = {ColumnVector::fromHost(ctx, h.a.data(), h.a.size()), ColumnVector::fromHost(ctx, h.b.data(), h.b.size()),
                 ColumnVector::fromHost(ctx, h.c.data(), h.c.size()), ColumnVector::fromHost(ctx, h.payload.data(), h.payload.size())};
    c.num_rows = h.a.size();
    return c;
}

// the payloads (row serial numbers) the reference lets through, chunk by chunk; n_keys: how many of the columns a, b, c are the key
static std::vector<std::vector<int64_t>> expect(const std::vector<HostChunk> & chunks, size_t n_keys, uint64_t length, uint64_t offset)
{
    std::map<std::array<uint64_t, 3>, uint64_t> count;
    std::vector<std::vector<int64_t>> out;
    for (const HostChunk & h : chunks)
    {
        std::vector<int64_t> pass;
        for (size_t i = 0; i < h.a.size(); ++i)
        {
            const std::array<uint64_t, 3> key{h.a[i], n_keys > 1 ? h.b[i] : 0, n_keys > 2 ? h.c[i] : 0};
            uint64_t & c = count[key];
            if (c < offset + length)
            {
                if (c >= offset)
                    pass.push_back(h.payload[i]);
                c += 1;
            }
        }
        out.push_back(pass);
    }
    return out;
}

static std::vector<std::vector<int64_t>> run(ISimpleTransform & t, const ContextPtr & ctx, const std::vector<HostChunk> & chunks, size_t * taken,
                                             std::vector<const void *> * passed_through = nullptr)
{
    std::vector<std::vector<int64_t>> out;
    size_t next = 0;
    std::vector<const void *> sent;
    executeChain(
        [&](Chunk & c) {
            if (next == chunks.size())
                return false;
            c = upload(ctx, chunks[next++]);
            sent.push_back(c.columns.at(3).get());
            return true;
        },
        {&t},
        [&](Chunk c) {
            REQUIRE(c.num_rows != 0 && c.columns.size() == 4 && c.columns.at(0)->size() == c.num_rows);
            out.push_back(c.columns.at(3)->getData<int64_t>());
            if (passed_through)
                for (const void * p : sent)
                    if (p == c.columns.at(3).get())
                        passed_through->push_back(p);
        });
    *taken = next;
    return out;
}

static std::vector<std::vector<int64_t>> non_empty(const std::vector<std::vector<int64_t>> & v)
{
    std::vector<std::vector<int64_t>> out;
    for (const auto & x : v)
        if (!x.empty())
            out.push_back(x);
    return out;
}

int main()
{
    ContextPtr ctx = std::make_shared<Context>(0);
    size_t taken = 0;
    {
        // DISTINCT a over 6 chunks of 5000 rows and 300 values: the later chunks bring nothing new and are dropped
        const auto chunks = make_chunks(6, 5000, 300, 1);
        GpuDistinctTransform t(ctx, {0});
        const auto got = run(t, ctx, chunks, &taken);
        const auto want = expect(chunks, 1, 1, 0);
        REQUIRE(got == non_empty(want) && got.size() < chunks.size() && taken == chunks.size());
        REQUIRE(t.keys() == 300 && t.passed_rows == 300);
    }
    {
        // DISTINCT a, b, c: 8 + 8 + 4 key bytes go through the dictionary; a first chunk of all-distinct rows passes through untouched
        auto chunks = make_chunks(3, 2000, 50, 2);
        for (size_t i = 0; i < chunks[0].a.size(); ++i)
            chunks[0].a[i] = 1000 + i;
        GpuDistinctTransform t(ctx, {0, 1, 2});
        std::vector<const void *> through;
        const auto got = run(t, ctx, chunks, &taken, &through);
        REQUIRE(got == non_empty(expect(chunks, 3, 1, 0)));
        REQUIRE(through.size() == 1 && got.at(0).size() == 2000);
    }
    {
        // LIMIT 2 OFFSET 1 BY a, c: 8 + 4 key bytes ... do not pack; LIMIT 3 BY c (4 bytes, one column) and BY (c, c) (packed) do
        const auto chunks = make_chunks(4, 3000, 40, 3);
        GpuLimitByTransform wide(ctx, {0, 2}, 2, 1);
        std::map<std::pair<uint64_t, uint32_t>, uint64_t> count;
        std::vector<std::vector<int64_t>> want;
        for (const HostChunk & h : chunks)
        {
            std::vector<int64_t> pass;
            for (size_t i = 0; i < h.a.size(); ++i)
            {
                uint64_t & c = count[{h.a[i], h.c[i]}];
                if (c < 3)
                {
                    if (c >= 1)
                        pass.push_back(h.payload[i]);
                    c += 1;
                }
            }
            want.push_back(pass);
        }
        REQUIRE(run(wide, ctx, chunks, &taken) == non_empty(want));
        GpuLimitByTransform one(ctx, {2}, 3, 0), packed(ctx, {2, 2}, 3, 0);
        const auto got_one = run(one, ctx, chunks, &taken), got_packed = run(packed, ctx, chunks, &taken);
        REQUIRE(got_one == got_packed && got_one.size() == 1 && got_one.at(0).size() == 6 && one.keys() == 2);
    }
    {
        // DISTINCT a LIMIT 450: 300 new values a chunk; the second chunk crosses the hint, goes out whole, and no further chunk is taken
        auto chunks = make_chunks(5, 300, 1, 4);
        for (size_t k = 0; k < chunks.size(); ++k)
            for (size_t i = 0; i < 300; ++i)
                chunks[k].a[i] = k * 300 + i;
        GpuDistinctTransform t(ctx, {0}, 450);
        const auto got = run(t, ctx, chunks, &taken);
        REQUIRE(got.size() == 2 && got.at(1).size() == 300 && taken == 2 && t.passed_rows == 600);
    }
    std::printf("limit_by_shim_driver OK\n");
    return 0;
}
