// window_driver.cpp — the host-only parts of the window operator (clickhouse_amd/csrc/window_host.h) as a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_window_abi.py: frame validation over every pair of bounds, the frame of a row against a
// brute-force membership test in 128-bit arithmetic, lagInFrame / leadInFrame's shifted row, which bound arrays a call asks for and the
// bookkeeping of their lazy construction, and the tile / grid arithmetic at its edges.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../clickhouse_amd/csrc/window_host.h"

#define CHECK(cond)                                                         \
    do                                                                      \
    {                                                                       \
        if (!(cond))                                                        \
        {                                                                   \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

typedef __int128 wide;

static chgpu_window_frame frame_of(int type, int b, uint64_t bo, int e, uint64_t eo)
{
    chgpu_window_frame f{};
    f.type = type;
    f.begin_kind = b;
    f.end_kind = e;
    f.begin_offset = bo;
    f.end_offset = eo;
    return f;
}

static void test_frame_validation()
{
    const int UP = CHGPU_BOUND_UNBOUNDED_PRECEDING, OP = CHGPU_BOUND_OFFSET_PRECEDING, CR = CHGPU_BOUND_CURRENT_ROW, OF = CHGPU_BOUND_OFFSET_FOLLOWING,
              UF = CHGPU_BOUND_UNBOUNDED_FOLLOWING;
    // legal[begin][end] with equal offsets, written out: rows UP, OP, CR, OF, UF; columns likewise
    const bool legal[5][5] = {{false, true, true, true, true},
                              {false, true, true, true, true},
                              {false, false, true, true, true},
                              {false, false, false, true, true},
                              {false, false, false, false, false}};
    int seen = 0;
    for (int type = 0; type < 2; ++type)
        for (int b = UP; b <= UF; ++b)
            for (int e = UP; e <= UF; ++e)
            {
                // an entry that serves no RANGE offsets refuses the legal ones; for every other frame the flag changes nothing
                const bool offset = b == OP || b == OF || e == OP || e == OF;
                for (int serves = 0; serves < 2; ++serves)
                {
                    const char * msg = nullptr;
                    const int rc = win_check_frame(frame_of(type, b, 3, e, 3), serves != 0, &msg);
                    const int want = !legal[b][e] ? CHGPU_ERR_BAD_ARGUMENTS : (type == CHGPU_FRAME_RANGE && offset && !serves) ? CHGPU_ERR_NOT_IMPLEMENTED : CHGPU_OK;
                    CHECK(rc == want);
                    CHECK((rc == CHGPU_OK) == (msg == nullptr));
                }
                seen += 1;
            }
    CHECK(seen == 50);
    const char * msg = nullptr;
    CHECK(win_check_frame(frame_of(CHGPU_FRAME_ROWS, OP, 1, OP, 2), false, &msg) == CHGPU_ERR_BAD_ARGUMENTS);
    CHECK(win_check_frame(frame_of(CHGPU_FRAME_ROWS, OP, 2, OP, 1), false, &msg) == CHGPU_OK);
    CHECK(win_check_frame(frame_of(CHGPU_FRAME_ROWS, OF, 2, OF, 1), false, &msg) == CHGPU_ERR_BAD_ARGUMENTS);
    CHECK(win_check_frame(frame_of(CHGPU_FRAME_ROWS, OF, 1, OF, 2), false, &msg) == CHGPU_OK);
    CHECK(win_check_frame(frame_of(CHGPU_FRAME_RANGE, OP, 1, OP, 2), false, &msg) == CHGPU_ERR_BAD_ARGUMENTS); // illegal before unimplemented
    CHECK(win_check_frame(frame_of(2, UP, 0, CR, 0), false, &msg) == CHGPU_ERR_BAD_ARGUMENTS);
    CHECK(win_check_frame(frame_of(CHGPU_FRAME_ROWS, -1, 0, CR, 0), false, &msg) == CHGPU_ERR_BAD_ARGUMENTS);
    CHECK(win_check_frame(frame_of(CHGPU_FRAME_ROWS, UP, 0, 5, 0), false, &msg) == CHGPU_ERR_BAD_ARGUMENTS);
    const chgpu_window_frame d = win_default_frame();
    CHECK(d.type == CHGPU_FRAME_RANGE && d.begin_kind == UP && d.end_kind == CR && win_check_frame(d, false, &msg) == CHGPU_OK);
}

// is row j of the partition inside the frame of row i?  Straight from the definition, in arithmetic that cannot wrap.
static bool in_frame(const chgpu_window_frame & f, uint64_t i, uint64_t j, uint64_t gs, uint64_t ge)
{
    bool after_begin = true, before_end = true;
    switch (f.begin_kind)
    {
        case CHGPU_BOUND_OFFSET_PRECEDING: after_begin = (wide)j >= (wide)i - (wide)f.begin_offset; break;
        case CHGPU_BOUND_CURRENT_ROW: after_begin = f.type == CHGPU_FRAME_ROWS ? j >= i : j >= gs; break;
        case CHGPU_BOUND_OFFSET_FOLLOWING: after_begin = (wide)j >= (wide)i + (wide)f.begin_offset; break;
        default: break;
    }
    switch (f.end_kind)
    {
        case CHGPU_BOUND_OFFSET_PRECEDING: before_end = (wide)j <= (wide)i - (wide)f.end_offset; break;
        case CHGPU_BOUND_CURRENT_ROW: before_end = f.type == CHGPU_FRAME_ROWS ? j <= i : j < ge; break;
        case CHGPU_BOUND_OFFSET_FOLLOWING: before_end = (wide)j <= (wide)i + (wide)f.end_offset; break;
        default: break;
    }
    return after_begin && before_end;
}

static void test_frames_against_brute_force()
{
    const uint64_t offsets[] = {0, 1, 2, 3, 7, 1ull << 32, ~0ull - 1, ~0ull};
    // partitions as (first row, length) with peer groups of the given length inside; the last one ends at the row limit
    struct Layout { uint64_t ps, len, peer; };
    const Layout layouts[] = {{0, 1, 1}, {0, 6, 2}, {5, 9, 3}, {100, 4, 4}, {WIN_MAX_ROWS - 7, 7, 2}};
    uint64_t checked = 0;
    for (const Layout & L : layouts)
        for (int type = 0; type < 2; ++type)
            for (int b = 0; b < 5; ++b)
                for (int e = 0; e < 5; ++e)
                    for (uint64_t bo : offsets)
                        for (uint64_t eo : offsets)
                        {
                            const chgpu_window_frame f = frame_of(type, b, bo, e, eo);
                            const char * msg = nullptr;
                            if (win_check_frame(f, false, &msg) != CHGPU_OK)
                                continue;
                            const uint64_t ps = L.ps, pe = L.ps + L.len;
                            for (uint64_t i = ps; i < pe; ++i)
                            {
                                const uint64_t gs = ps + (i - ps) / L.peer * L.peer, ge = gs + L.peer < pe ? gs + L.peer : pe;
                                uint64_t fs = 0, fe = 0;
                                win_frame_of(f, i, ps, pe, gs, ge, &fs, &fe);
                                CHECK(ps <= fs && fs <= fe && fe <= pe);
                                uint64_t members = 0, first = pe;
                                for (uint64_t j = ps; j < pe; ++j)
                                    if (in_frame(f, i, j, gs, ge))
                                    {
                                        first = members ? first : j;
                                        members += 1;
                                        CHECK(j >= fs && j < fe);
                                    }
                                CHECK(members == fe - fs);
                                CHECK(members == 0 || first == fs);
                                checked += 1;
                            }
                        }
    CHECK(checked > 10000);
    // the arrays a frame reads are the ones win_frame_needs names: garbage in the others changes nothing
    for (int type = 0; type < 2; ++type)
        for (int b = 0; b < 5; ++b)
            for (int e = 0; e < 5; ++e)
            {
                const chgpu_window_frame f = frame_of(type, b, 2, e, 2);
                const char * msg = nullptr;
                if (win_check_frame(f, false, &msg) != CHGPU_OK)
                    continue;
                const uint32_t needs = win_frame_needs(f);
                uint64_t fs = 0, fe = 0, gs2 = 0, ge2 = 0;
                win_frame_of(f, 12, 10, 20, 11, 14, &fs, &fe);
                win_frame_of(f, 12, needs & WIN_B_PS ? 10 : 999, needs & WIN_B_PE ? 20 : 999, needs & WIN_B_GS ? 11 : 999, needs & WIN_B_GE ? 14 : 999, &gs2, &ge2);
                CHECK(fs == gs2 && fe == ge2);
            }
}

static void test_shifted_row()
{
    const uint64_t offsets[] = {0, 1, 2, 5, 1ull << 33, ~0ull - 3, ~0ull};
    for (uint64_t i : {0ull, 3ull, 9ull, (unsigned long long)WIN_MAX_ROWS - 1})
        for (uint64_t off : offsets)
            for (int lead = 0; lead < 2; ++lead)
            {
                const uint64_t fs = i >= 3 ? i - 3 : 0, fe = i + 3 < WIN_MAX_ROWS ? i + 3 : WIN_MAX_ROWS;
                const wide t = lead ? (wide)i + (wide)off : (wide)i - (wide)off;
                const bool want = t >= (wide)fs && t < (wide)fe;
                uint64_t got_t = 0;
                const bool got = win_shifted_row(lead != 0, i, off, fs, fe, &got_t);
                CHECK(got == want);
                CHECK(!got || (wide)got_t == t);
            }
}

static void test_plans_and_lazy_bounds()
{
    const chgpu_window_frame dflt = win_default_frame();
    const chgpu_window_frame rows_running = frame_of(CHGPU_FRAME_ROWS, CHGPU_BOUND_UNBOUNDED_PRECEDING, 0, CHGPU_BOUND_CURRENT_ROW, 0);
    const chgpu_window_frame whole = frame_of(CHGPU_FRAME_ROWS, CHGPU_BOUND_UNBOUNDED_PRECEDING, 0, CHGPU_BOUND_UNBOUNDED_FOLLOWING, 0);
    const chgpu_window_frame sliding = frame_of(CHGPU_FRAME_ROWS, CHGPU_BOUND_OFFSET_PRECEDING, 9, CHGPU_BOUND_CURRENT_ROW, 0);
    const chgpu_window_frame ahead = frame_of(CHGPU_FRAME_ROWS, CHGPU_BOUND_CURRENT_ROW, 0, CHGPU_BOUND_UNBOUNDED_FOLLOWING, 0);
    const chgpu_window_frame self = frame_of(CHGPU_FRAME_ROWS, CHGPU_BOUND_CURRENT_ROW, 0, CHGPU_BOUND_CURRENT_ROW, 0);
    const chgpu_window_frame two_sided = frame_of(CHGPU_FRAME_ROWS, CHGPU_BOUND_OFFSET_PRECEDING, 1, CHGPU_BOUND_OFFSET_FOLLOWING, 1);
    // chgpu_window_evaluate's plans: no order column, and a handle whose facts do not enter without one
    WinPlan plan;
    std::string msg;
    const auto plan_of = [&](int function, const chgpu_window_frame & frame, int arg_type) { return win_plan(false, function, frame, arg_type, -1, 0, -1, &plan, &msg); };
    CHECK(plan_of(CHGPU_WIN_ROW_NUMBER, dflt, -1) == CHGPU_OK && plan.needs == WIN_B_PS);
    CHECK(plan_of(CHGPU_WIN_RANK, dflt, -1) == CHGPU_OK && plan.needs == (WIN_B_PS | WIN_B_GS)); // rank() never builds pe
    CHECK(plan_of(CHGPU_WIN_DENSE_RANK, dflt, -1) == CHGPU_OK && plan.needs == (WIN_B_PS | WIN_B_DENSE));
    CHECK(plan_of(CHGPU_WIN_COUNT, dflt, -1) == CHGPU_OK && plan.needs == (WIN_B_PS | WIN_B_GE));
    CHECK(plan_of(CHGPU_WIN_COUNT, self, -1) == CHGPU_OK && plan.needs == 0);
    CHECK(plan_of(CHGPU_WIN_SUM, rows_running, CHGPU_I64) == CHGPU_OK && plan.needs == WIN_B_PS);
    CHECK(plan_of(CHGPU_WIN_SUM, sliding, CHGPU_U8) == CHGPU_OK && plan.needs == WIN_B_PS);
    CHECK(plan_of(CHGPU_WIN_AVG, two_sided, CHGPU_I16) == CHGPU_OK && plan.needs == (WIN_B_PS | WIN_B_PE));
    CHECK(plan_of(CHGPU_WIN_MAX, whole, CHGPU_F64) == CHGPU_OK && plan.needs == (WIN_B_PS | WIN_B_PE) && plan.ext == WIN_EXT_FORWARD);
    CHECK(plan_of(CHGPU_WIN_MIN, ahead, CHGPU_F32) == CHGPU_OK && plan.needs == WIN_B_PE && plan.ext == WIN_EXT_BACKWARD);
    CHECK(plan_of(CHGPU_WIN_MIN, two_sided, CHGPU_I64) == CHGPU_ERR_NOT_IMPLEMENTED);
    CHECK(plan_of(CHGPU_WIN_SUM, whole, CHGPU_F64) == CHGPU_ERR_NOT_IMPLEMENTED);
    CHECK(plan_of(CHGPU_WIN_AVG, whole, CHGPU_F32) == CHGPU_ERR_NOT_IMPLEMENTED);
    CHECK(plan_of(CHGPU_WIN_LAG_IN_FRAME, whole, CHGPU_F32) == CHGPU_OK && plan.needs == (WIN_B_PS | WIN_B_PE));
    CHECK(plan_of(CHGPU_WIN_SUM, whole, -1) == CHGPU_ERR_BAD_ARGUMENTS);  // no argument
    CHECK(plan_of(CHGPU_WIN_RANK, whole, CHGPU_I64) == CHGPU_ERR_BAD_ARGUMENTS); // a surplus one
    CHECK(plan_of(-1, whole, -1) == CHGPU_ERR_BAD_ARGUMENTS);
    CHECK(plan_of(CHGPU_WIN_LEAD_IN_FRAME + 1, whole, CHGPU_I64) == CHGPU_ERR_BAD_ARGUMENTS);

    WinLazy lazy;
    CHECK(lazy.missing(WIN_B_PS | WIN_B_GS) == (WIN_B_PS | WIN_B_GS));
    lazy.mark(WIN_B_PS);
    lazy.mark(WIN_B_GS);
    CHECK(lazy.builds == 2 && lazy.missing(WIN_B_PS | WIN_B_GS) == 0 && lazy.missing(WIN_B_PS | WIN_B_PE) == WIN_B_PE);
    lazy.mark(WIN_B_PS); // an array is built at most once
    CHECK(lazy.builds == 2);
    lazy.mark(WIN_B_PE);
    lazy.mark(WIN_B_GE);
    lazy.mark(WIN_B_DENSE);
    CHECK(lazy.builds == 5 && lazy.missing(WIN_B_ALL) == 0 && lazy.missing(~0u) == 0);
}

static void test_tile_and_grid_arithmetic()
{
    const uint64_t T = WIN_TILE;
    CHECK(T == 2048 && WIN_PASS == 1024 && WIN_OUT_BLOCK == 1024 && WIN_THREADS * WIN_ITEMS == WIN_TILE);
    CHECK(win_tiles(0) == 0 && win_tiles(1) == 1 && win_tiles(T - 1) == 1 && win_tiles(T) == 1 && win_tiles(T + 1) == 2);
    CHECK(win_tiles(WIN_MAX_ROWS) == (1ull << 21));                    // 2^32 - 1 rows: the grid of the per-tile kernels
    CHECK(win_padded_rows(0) == 0 && win_padded_rows(1) == T && win_padded_rows(T) == T && win_padded_rows(T + 1) == 2 * T);
    CHECK(win_padded_rows(WIN_MAX_ROWS) == (1ull << 32));              // past u32: indices into the padded arrays are 64-bit
    CHECK(win_passes(0) == 0 && win_passes(1) == 1 && win_passes(WIN_PASS) == 1 && win_passes(WIN_PASS + 1) == 2);
    CHECK(win_passes(win_tiles(T * WIN_PASS + T + 5)) == 2);
    CHECK(win_passes(win_tiles(WIN_MAX_ROWS)) == 2048);
    CHECK(win_out_blocks(0) == 0 && win_out_blocks(1) == 1 && win_out_blocks(WIN_OUT_BLOCK) == 1 && win_out_blocks(WIN_OUT_BLOCK + 1) == 2);
    CHECK(win_out_blocks(WIN_MAX_ROWS) == (1ull << 22));               // fits a 32-bit grid
    // every thread's four rows start at a multiple of four inside the padded arrays
    CHECK(win_out_blocks(WIN_MAX_ROWS) * WIN_OUT_BLOCK <= win_padded_rows(WIN_MAX_ROWS));
    CHECK(win_out_blocks(T + 1) * WIN_OUT_BLOCK <= win_padded_rows(T + 1));
    CHECK(win_sat_add(~0ull, 1) == ~0ull && win_sat_add(~0ull - 1, 1) == ~0ull && win_sat_add(5, 6) == 11 && win_sat_add(~0ull, ~0ull) == ~0ull);
}

int main()
{
    test_frame_validation();
    test_frames_against_brute_force();
    test_shifted_row();
    test_plans_and_lazy_bounds();
    test_tile_and_grid_arithmetic();
    printf("window_driver OK\n");
    return 0;
}
