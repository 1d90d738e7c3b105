// The String functions through the C++ host shim (clickhouse_amd/host/chgpu_shim.hpp): length, lengthUTF8, empty, notEmpty, lower,
// upper, substring, position, compareColumn and the static concat of chgpu::ColumnString over a small column, against std::string loops.
// Compiled syntax-only by tests/test_string_functions_abi.py; built and run by tests/test_gpu_string_functions.py; prints
// "string_functions_shim_driver OK".
#include "../clickhouse_amd/host/chgpu_shim.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <string_view>

using namespace chgpu;
using namespace std::string_view_literals;

#define REQUIRE(cond)                                                        \
    do                                                                       \
    {                                                                        \
        if (!(cond))                                                         \
        {                                                                    \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

static ColumnString upload(const ContextPtr & ctx, const std::vector<std::string> & values)
{
    std::vector<uint64_t> offsets;
    std::vector<uint8_t> chars;
    for (const std::string & v : values)
    {
        chars.insert(chars.end(), v.begin(), v.end());
        chars.push_back(0);
        offsets.push_back(chars.size());
    }
    return ColumnString{ColumnVector::fromHost(ctx, offsets.data(), offsets.size()), ColumnVector::fromHost(ctx, chars.data(), chars.size())};
}

static std::vector<std::string> download(const ColumnString & col)
{
    const std::vector<uint64_t> offsets = col.offsets->getData<uint64_t>();
    const std::vector<uint8_t> chars = col.chars->getData<uint8_t>();
    REQUIRE(chars.size() == (offsets.empty() ? 0 : offsets.back()));
    std::vector<std::string> out;
    uint64_t begin = 0;
    for (uint64_t end : offsets)
    {
        REQUIRE(end > begin && chars[end - 1] == 0);
        out.emplace_back(reinterpret_cast<const char *>(chars.data()) + begin, end - 1 - begin);
        begin = end;
    }
    return out;
}

template <class T, class F>
static void expect_numbers(const ColumnPtr & got, const std::vector<std::string> & values, F && f)
{
    const std::vector<T> g = got->getData<T>();
    REQUIRE(g.size() == values.size());
    for (size_t i = 0; i < values.size(); ++i)
        REQUIRE(g[i] == static_cast<T>(f(i)));
}

template <class F>
static void expect_strings(const ColumnString & got, const std::vector<std::string> & values, F && f)
{
    const std::vector<std::string> g = download(got);
    REQUIRE(g.size() == values.size());
    for (size_t i = 0; i < values.size(); ++i)
        REQUIRE(g[i] == f(i));
}

static std::string ascii_case(std::string s, bool upper)
{
    for (char & ch : s)
        if (upper ? (ch >= 'a' && ch <= 'z') : (ch >= 'A' && ch <= 'Z'))
            ch ^= 0x20;
    return s;
}

int main()
{
    ContextPtr ctx = std::make_shared<Context>(0);
    std::vector<std::string> a_values, b_values;
    const std::string pieces[] = {"", "a", "Hello, World", std::string("zero\0inside", 11), "\xD0\xB6\xE2\x82\xAC", "https://example.com/Path/To/Page.html",
                                  "ABCDEFGHIJKLMNOPQRSTUVWXYZ@[`{az", "needle in a haystack with a needle"};
    for (size_t i = 0; i < 300; ++i)
    {
        a_values.push_back(pieces[i % 8] + (i % 3 ? std::to_string(i) : ""));
        b_values.push_back(pieces[(i * 5 + 1) % 8] + (i % 2 ? std::to_string(i) : ""));
    }
    const ColumnString a = upload(ctx, a_values), b = upload(ctx, b_values);

    expect_numbers<uint64_t>(a.length(), a_values, [&](size_t i) { return a_values[i].size(); });
    expect_numbers<uint64_t>(a.lengthUTF8(), a_values, [&](size_t i) {
        return std::count_if(a_values[i].begin(), a_values[i].end(), [](char ch) { return (static_cast<unsigned char>(ch) & 0xC0) != 0x80; });
    });
    expect_numbers<uint8_t>(a.empty(), a_values, [&](size_t i) { return a_values[i].empty(); });
    expect_numbers<uint8_t>(a.notEmpty(), a_values, [&](size_t i) { return !a_values[i].empty(); });
    expect_strings(a.lower(), a_values, [&](size_t i) { return ascii_case(a_values[i], false); });
    expect_strings(a.upper(), a_values, [&](size_t i) { return ascii_case(a_values[i], true); });
    expect_strings(a.substring(3), a_values, [&](size_t i) { return a_values[i].size() > 2 ? a_values[i].substr(2) : std::string(); });
    expect_strings(a.substring(2, 5), a_values, [&](size_t i) { return a_values[i].size() > 1 ? a_values[i].substr(1, 5) : std::string(); });
    expect_strings(a.substring(-4, 2), a_values, [&](size_t i) {
        const std::string & v = a_values[i]; // the window starts 4 bytes before the end, possibly in front of the value
        const long start = static_cast<long>(v.size()) - 4, lo = std::max(start, 0l), hi = std::min<long>(start + 2, v.size());
        return hi > lo ? v.substr(lo, hi - lo) : std::string();
    });
    expect_numbers<uint64_t>(a.position("needle"), a_values, [&](size_t i) {
        const size_t at = a_values[i].find("needle");
        return at == std::string::npos ? 0 : at + 1;
    });
    expect_numbers<uint64_t>(a.position("\0in"sv), a_values, [&](size_t i) {
        const size_t at = a_values[i].find("\0in"sv);
        return at == std::string::npos ? 0 : at + 1;
    });
    expect_numbers<uint8_t>(a.compareColumn(CHGPU_LT, b), a_values, [&](size_t i) { return a_values[i] < b_values[i]; }); // std::string orders by unsigned bytes, then length
    expect_numbers<uint8_t>(a.compareColumn(CHGPU_EQ, a), a_values, [&](size_t) { return 1; });
    expect_strings(ColumnString::concat({a, "/"sv, b}), a_values, [&](size_t i) { return a_values[i] + "/" + b_values[i]; });
    expect_strings(ColumnString::concat({"<\0"sv, a, a, ">"}), a_values, [&](size_t i) { return std::string("<\0", 2) + a_values[i] + a_values[i] + ">"; });

    bool refused = false;
    try
    {
        a.substring(0);
    }
    catch (const Exception & e)
    {
        refused = e.isNotImplemented();
    }
    REQUIRE(refused);
    std::printf("string_functions_shim_driver OK\n");
    return 0;
}
