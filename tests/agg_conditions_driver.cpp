// The -If combinator and a Nullable argument through the C++ host shim (clickhouse_amd/host/chgpu_shim.hpp), checked against a plain
// host loop: SELECT k, sumIf(v, c), min(v over Nullable), count(v over Nullable), count() GROUP BY k over two blocks.
//   * key 0 is present; key 7's rows all fail the condition and are all NULL; key 9's rows all pass and none is NULL;
//   * GpuAggregator::convertToBlock appends one UInt8 null-map column per function with a Nullable result (here: the min);
//   * AggregateDescription::stateWords counts the `seen` word of the NULL-mode min.
// Built by tests/test_gpu_agg_conditions.py against libchgpu.so; prints "agg_conditions_driver OK".
#include "../clickhouse_amd/host/chgpu_shim.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
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

struct Want
{
    int64_t sum_if = 0;
    bool has_min = false;
    int64_t min = 0;
    uint64_t not_null = 0, rows = 0;
};

int main()
{
    auto ctx = std::make_shared<Context>(0);
    // chunk layout: 0 key, 1 value, 2 condition, 3 null map
    AggregateDescription sum_if{CHGPU_AGG_SUM, CHGPU_I64, 1};
    sum_if.condition_mode = CHGPU_AGG_COND_IF;
    sum_if.condition = 2;
    AggregateDescription min_null{CHGPU_AGG_MIN, CHGPU_I64, 1};
    min_null.condition_mode = CHGPU_AGG_COND_NULL;
    min_null.condition = 3;
    AggregateDescription count_null{CHGPU_AGG_COUNT, CHGPU_U64, 0};
    count_null.condition_mode = CHGPU_AGG_COND_NULL;
    count_null.condition = 3;
    AggregateDescription count_all{CHGPU_AGG_COUNT, CHGPU_U64, 0};
    REQUIRE(sum_if.stateWords() == 1 && min_null.stateWords() == 2 && count_null.stateWords() == 1);
    REQUIRE(min_null.nullableResult() && !count_null.nullableResult() && !sum_if.nullableResult());
    GpuAggregator agg(ctx, CHGPU_U32, {sum_if, min_null, count_null, count_all}, 0);
    REQUIRE(agg.stateWords() == 5);

    std::map<uint32_t, Want> want;
    for (int b = 0; b < 2; ++b)
    {
        std::vector<uint32_t> k;
        std::vector<int64_t> v;
        std::vector<uint8_t> c, nm;
        for (int r = 0; r < 1000; ++r)
        {
            const uint32_t key = static_cast<uint32_t>((r * 7 + b) % 10);
            const int64_t val = key == 3 ? INT64_MIN + r : static_cast<int64_t>(r) * 1000 - 400000 + b;
            uint8_t cond = static_cast<uint8_t>(r % 3 == 0 ? 0 : r % 3 == 1 ? 1 : 255);
            uint8_t null = static_cast<uint8_t>(r % 4 == 0 ? 1 : 0);
            if (key == 7)
                cond = 0, null = 1;
            if (key == 9)
                cond = 2, null = 0;
            k.push_back(key), v.push_back(val), c.push_back(cond), nm.push_back(null);
            Want & w = want[key];
            w.rows += 1;
            if (cond)
                w.sum_if += val;
            if (!null)
            {
                w.not_null += 1;
                if (!w.has_min || val < w.min)
                    w.min = val;
                w.has_min = true;
            }
        }
        Chunk chunk;
        chunk.columns.push_back(ColumnVector::fromHost<uint32_t>(ctx, k.data(), k.size()));
        chunk.columns.push_back(ColumnVector::fromHost<int64_t>(ctx, v.data(), v.size()));
        chunk.columns.push_back(ColumnVector::fromHost<uint8_t>(ctx, c.data(), c.size()));
        chunk.columns.push_back(ColumnVector::fromHost<uint8_t>(ctx, nm.data(), nm.size()));
        chunk.num_rows = k.size();
        REQUIRE(agg.executeOnBlock(chunk.columns, 0, chunk.num_rows, std::optional<size_t>(0)));
    }
    REQUIRE(want.count(0) && want.at(7).sum_if == 0 && !want.at(7).has_min && want.at(9).not_null == want.at(9).rows);

    Chunk out = agg.convertToBlock();
    REQUIRE(out.num_rows == want.size());
    REQUIRE(out.columns.size() == 1 + 4 + 1); // key, four results, the min's null map
    auto k = out.columns.at(0)->getData<uint32_t>();
    auto s = out.columns.at(1)->getData<int64_t>();
    auto m = out.columns.at(2)->getData<int64_t>();
    auto nn = out.columns.at(3)->getData<uint64_t>();
    auto n = out.columns.at(4)->getData<uint64_t>();
    auto m_null = out.columns.at(5)->getData<uint8_t>();
    for (size_t i = 0; i < out.num_rows; ++i)
    {
        const Want & w = want.at(k[i]);
        REQUIRE(s[i] == w.sum_if);
        REQUIRE(m_null[i] == (w.has_min ? 0 : 1));
        REQUIRE(m[i] == (w.has_min ? w.min : 0)); // NULL: the nested value is the type's default
        REQUIRE(nn[i] == w.not_null);
        REQUIRE(n[i] == w.rows);
    }
    std::printf("agg_conditions_driver OK\n");
    return 0;
}
