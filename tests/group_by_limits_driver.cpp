// GROUP BY limits through the C++ host shim (clickhouse_amd/host/chgpu_shim.hpp), checked against plain host loops:
//   break: group_by_overflow_mode BREAK makes a GpuAggregatingTransform finish its input (isConsumeFinished) on the block that crosses
//          max_rows_to_group_by; the driver stops feeding it and the result holds exactly the blocks consumed;
//   any:   ANY with an overflow row over two streams sharing ManyAggregatedData: each stream turns find-only on its own, the last one
//          merges the variants largest first (chgpu_agg_merge_limited), and generate() yields the is_overflows chunk first.
// Built by tests/test_gpu_group_by_limits.py against libchgpu.so; prints "group_by_limits_driver OK".
#include "../clickhouse_amd/host/chgpu_shim.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

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

static Chunk block(const ContextPtr & ctx, const std::vector<uint32_t> & k, const std::vector<int64_t> & v)
{
    Chunk c;
    c.columns.push_back(ColumnVector::fromHost<uint32_t>(ctx, k.data(), k.size()));
    c.columns.push_back(ColumnVector::fromHost<int64_t>(ctx, v.data(), v.size()));
    c.num_rows = k.size();
    return c;
}

// block b of stream s: 100 rows, keys s*1000 + b*7 + (0 .. 19), value = key + 1
static void make_block(int s, int b, std::vector<uint32_t> & k, std::vector<int64_t> & v)
{
    k.clear(), v.clear();
    for (int r = 0; r < 100; ++r)
    {
        const uint32_t key = static_cast<uint32_t>(s * 1000 + b * 7 + r % 20);
        k.push_back(key);
        v.push_back(static_cast<int64_t>(key) + 1);
    }
}

static std::map<uint32_t, std::pair<int64_t, uint64_t>> keyed(const Chunk & c)
{
    std::map<uint32_t, std::pair<int64_t, uint64_t>> out;
    auto k = c.columns.at(0)->getData<uint32_t>();
    auto s = c.columns.at(1)->getData<int64_t>();
    auto n = c.columns.at(2)->getData<uint64_t>();
    for (size_t i = 0; i < c.num_rows; ++i)
        out[k[i]] = {s[i], n[i]};
    return out;
}

int main()
{
    auto ctx = std::make_shared<Context>(0);
    const std::vector<AggregateDescription> aggs = {{CHGPU_AGG_SUM, CHGPU_I64, 1}, {CHGPU_AGG_COUNT, CHGPU_U64, 0}};
    std::vector<uint32_t> k;
    std::vector<int64_t> v;
    {
        // ---- BREAK: 20 keys per block, 7 new ones per later block; M = 40 -> blocks 0..3 give 20, 27, 34, 41 groups: block 3 crosses
        GroupByLimits lim;
        lim.max_rows_to_group_by = 40;
        lim.group_by_overflow_mode = CHGPU_OVERFLOW_BREAK;
        auto agg = std::make_shared<GpuAggregator>(ctx, CHGPU_U32, aggs, 0, lim);
        GpuAggregatingTransform tr(agg, std::optional<size_t>(0));
        std::map<uint32_t, std::pair<int64_t, uint64_t>> want;
        int fed = 0;
        for (int b = 0; b < 10 && !tr.isConsumeFinished(); ++b, ++fed)
        {
            make_block(0, b, k, v);
            tr.consume(block(ctx, k, v));
            for (size_t i = 0; i < k.size(); ++i)
                want[k[i]].first += v[i], want[k[i]].second += 1;
        }
        REQUIRE(tr.isConsumeFinished());
        REQUIRE(fed == 4);
        tr.work();
        Chunk first = tr.generate();
        REQUIRE(!first.is_overflows);
        REQUIRE(keyed(first) == want);
    }
    {
        // ---- ANY + overflow row, two streams: M = 30; stream s sees blocks 0..5 of keys s*1000 + ...
        GroupByLimits lim;
        lim.max_rows_to_group_by = 30;
        lim.group_by_overflow_mode = CHGPU_OVERFLOW_ANY;
        lim.overflow_row = true;
        auto many = std::make_shared<ManyAggregatedData>(std::vector<std::shared_ptr<GpuAggregator>>{
            std::make_shared<GpuAggregator>(ctx, CHGPU_U32, aggs, 0, lim), std::make_shared<GpuAggregator>(ctx, CHGPU_U32, aggs, 0, lim)});
        GpuAggregatingTransform t0(many, 0, std::optional<size_t>(0)), t1(many, 1, std::optional<size_t>(0));
        // host model: per stream, a block is added in full while the stream's no_more_keys is off; then rows of absent keys overflow
        std::map<uint32_t, std::pair<int64_t, uint64_t>> part[2];
        int64_t ovf_sum = 0;
        uint64_t ovf_cnt = 0;
        for (int s = 0; s < 2; ++s)
        {
            bool nmk = false;
            for (int b = 0; b < (s == 0 ? 6 : 2); ++b)
            {
                make_block(s, b, k, v);
                (s == 0 ? t0 : t1).consume(block(ctx, k, v));
                for (size_t i = 0; i < k.size(); ++i)
                {
                    if (nmk && !part[s].count(k[i]))
                    {
                        ovf_sum += v[i], ovf_cnt += 1;
                        continue;
                    }
                    part[s][k[i]].first += v[i], part[s][k[i]].second += 1;
                }
                if (!nmk && part[s].size() > 30)
                    nmk = true;
            }
        }
        REQUIRE(!t0.isConsumeFinished() && !t1.isConsumeFinished());
        // merge (largest first: stream 0 holds 34 groups, stream 1 27): dst has 34 > 30 -> the merge is find-only from the start, the
        // source's keys are all absent (disjoint streams) -> every state of stream 1 goes to the overflow row
        std::map<uint32_t, std::pair<int64_t, uint64_t>> want = part[0];
        for (auto & kv : part[1])
            ovf_sum += kv.second.first, ovf_cnt += kv.second.second;
        t0.work();
        t1.work();
        REQUIRE(t1.isGenerating() && !t0.isGenerating());
        Chunk o = t1.generate();
        REQUIRE(o.is_overflows && o.num_rows == 1);
        REQUIRE(o.columns.at(0)->getData<uint32_t>()[0] == 0);
        REQUIRE(o.columns.at(1)->getData<int64_t>()[0] == ovf_sum);
        REQUIRE(o.columns.at(2)->getData<uint64_t>()[0] == ovf_cnt);
        Chunk r = t1.generate();
        REQUIRE(!r.is_overflows);
        REQUIRE(keyed(r) == want);
    }
    std::printf("group_by_limits_driver OK\n");
    return 0;
}
