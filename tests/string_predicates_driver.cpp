// String predicates through the C++ host shim (clickhouse_amd/host/chgpu_shim.hpp): the five members of chgpu::ColumnString that turn a
// ColumnString and a constant into a UInt8 filter column, and that column in front of a GpuFilterTransform.
// Compiled syntax-only by tests/test_string_predicates_abi.py (no GPU, no library).
#include "../clickhouse_amd/host/chgpu_shim.hpp"

#include <string_view>

using namespace chgpu;

Chunk drive(const ColumnString & url, ColumnPtr hits)
{
    using namespace std::string_view_literals;
    ColumnPtr between = url.compare(CHGPU_GE, "MFGR#2221");
    ColumnPtr upper = url.compare(CHGPU_LE, std::string_view("MFGR#2228"));
    ColumnPtr binary = url.compare(CHGPU_EQ, "a\0b"sv); // constants are binary-safe
    ColumnPtr google = url.like("%google%");
    ColumnPtr not_like = url.like("a_c%", true);
    ColumnPtr has = url.contains("http");
    ColumnPtr no_scheme = url.startsWith("https://", true);
    ColumnPtr html = url.endsWith(".html");
    (void)between, (void)upper, (void)binary, (void)not_like, (void)has, (void)no_scheme, (void)html;

    Chunk chunk;
    chunk.columns = {hits, google};
    chunk.num_rows = hits->size();
    GpuFilterTransform where(1, true); // the predicate's result is the filter column, removed after use
    where.setInput(std::move(chunk));
    where.work();
    return where.pullOutput();
}
