"""The C ABI of the window operator without a GPU: the four entry points are declared, bound and exported, the enums and the frame struct
are in the header, NULL handles and outputs answer BAD_ARGUMENTS with a message, the Python classes reject bad dtypes and illegal frames
before they touch the library, the shim's GpuWindowTransform compiles, and the host-only parts run under a sanitizer as a stand-alone
program (the checks that need a context are in test_gpu_window.py)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SYMBOLS = ("chgpu_window_create", "chgpu_window_counts", "chgpu_window_evaluate", "chgpu_window_free")


@pytest.fixture(scope="module")
def K():
    from clickhouse_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    _capi.lib()
    return _capi


def _expect_bad(K, rc):
    assert rc == K.ERR_BAD_ARGUMENTS
    with pytest.raises(K.ChgpuError) as e:
        K.check(rc)
    assert e.value.code == K.ERR_BAD_ARGUMENTS and "NULL" in str(e.value)


def test_entry_points_are_declared_bound_and_exported(K):
    for name in SYMBOLS:
        assert name in K.declared_symbols() and name in K.SIGNATURES
        assert getattr(K.lib(), name)
    assert K.lib().chgpu_abi_version() == 1


def test_enums_and_frame_struct_are_in_the_header(K):
    header = open(K.HEADER_PATH).read()
    assert "typedef struct chgpu_window chgpu_window;" in header
    assert "typedef struct { int32_t type, begin_kind, end_kind, reserved; uint64_t begin_offset, end_offset; } chgpu_window_frame;" in header
    functions = re.search(r"enum \{ (CHGPU_WIN_ROW_NUMBER = 0[^}]*)\}", header).group(1)
    names = [n.strip().split(" ")[0] for n in functions.split(",")]
    assert names == ["CHGPU_WIN_ROW_NUMBER", "CHGPU_WIN_RANK", "CHGPU_WIN_DENSE_RANK", "CHGPU_WIN_COUNT", "CHGPU_WIN_SUM", "CHGPU_WIN_AVG", "CHGPU_WIN_MIN",
                     "CHGPU_WIN_MAX", "CHGPU_WIN_FIRST_VALUE", "CHGPU_WIN_LAST_VALUE", "CHGPU_WIN_LAG_IN_FRAME", "CHGPU_WIN_LEAD_IN_FRAME"]
    assert [getattr(K, n[len("CHGPU_"):]) for n in names] == list(range(12))
    assert "enum { CHGPU_FRAME_ROWS = 0, CHGPU_FRAME_RANGE = 1 };" in header and (K.FRAME_ROWS, K.FRAME_RANGE) == (0, 1)
    bounds = re.search(r"enum \{ (CHGPU_BOUND_UNBOUNDED_PRECEDING = 0[^}]*)\}", header).group(1)
    names = [n.strip().split(" ")[0] for n in bounds.split(",")]
    assert [getattr(K, n[len("CHGPU_"):]) for n in names] == list(range(5)) and names[2] == "CHGPU_BOUND_CURRENT_ROW"
    assert C.sizeof(K.WindowFrame) == 32 and K.WindowFrame.begin_offset.offset == 16
    assert "WindowTransform.cpp" in header and "WindowDescription.h" in header


def test_python_mirrors_the_scan_geometry():
    from clickhouse_amd import window
    host = open(os.path.join(REPO, "clickhouse_amd", "csrc", "window_host.h")).read()
    threads = int(re.search(r"WIN_THREADS = (\d+);", host).group(1))
    items = int(re.search(r"WIN_ITEMS = (\d+);", host).group(1))
    assert "WIN_TILE = WIN_THREADS * WIN_ITEMS;" in host and window.TILE == threads * items
    assert window.PASS_TILES == int(re.search(r"WIN_PASS = (\d+);", host).group(1))
    assert window.MAX_KEYS == int(re.search(r"WIN_MAX_KEYS = (\d+);", host).group(1))


def test_null_handles_and_outputs_are_bad_arguments(K):
    h, out = C.c_void_p(), C.c_void_p()
    n = C.c_uint64(0)
    _expect_bad(K, K.lib().chgpu_window_create(None, None, 0, None, 0, 0, C.byref(h)))
    _expect_bad(K, K.lib().chgpu_window_create(None, None, 0, None, 0, 10, None))
    _expect_bad(K, K.lib().chgpu_window_counts(None, C.byref(n), C.byref(n), C.byref(n)))
    _expect_bad(K, K.lib().chgpu_window_evaluate(None, K.WIN_ROW_NUMBER, None, None, 0, 0, C.byref(out)))
    frame = K.WindowFrame(K.FRAME_ROWS, K.BOUND_UNBOUNDED_PRECEDING, K.BOUND_CURRENT_ROW, 0, 0, 0)
    _expect_bad(K, K.lib().chgpu_window_evaluate(None, K.WIN_COUNT, C.byref(frame), None, 0, 0, None))


def test_free_takes_null(K):
    assert K.lib().chgpu_window_free(None) == K.OK


def test_python_rejects_bad_dtypes_before_the_library(K):
    import clickhouse_amd
    from clickhouse_amd.window import Window
    assert clickhouse_amd.Window is Window
    ok = np.zeros(4, dtype=np.uint32)
    with pytest.raises(ValueError):
        Window([np.zeros(4, dtype=np.float16)], [ok], ctx=object())
    with pytest.raises(ValueError):
        Window([ok], [np.zeros(4, dtype=np.complex64)], ctx=object())
    with pytest.raises(ValueError):
        Window([ok], [np.array(["a", "b", "c", "d"])], ctx=object())
    with pytest.raises(ValueError):
        Window([ok] * 9, [], ctx=object())
    with pytest.raises(ValueError):
        Window([ok], [np.zeros(5, dtype=np.int64)], ctx=object())
    with pytest.raises(ValueError):
        Window([], [], ctx=object())
    # the methods: a handle-less object stands for a window of four rows; nothing below may reach the library
    w = Window.__new__(Window)
    w.rows, w.ctx, w._h = 4, object(), None
    with pytest.raises(ValueError):
        w.sum(np.zeros(4, dtype=np.float16))
    with pytest.raises(ValueError):
        w.lag_in_frame(np.zeros(4, dtype="U3"))
    with pytest.raises(ValueError):
        w.max(np.zeros(3, dtype=np.int64))
    with pytest.raises(ValueError):
        w.first_value(None)
    with pytest.raises(ValueError):
        w.lead_in_frame(np.zeros(4, dtype=np.int64), offset=-1)
    with pytest.raises(ValueError):
        w.count(frame=(0, 0, 0, 2, 0))


def test_python_rejects_illegal_frames_before_the_library(K):
    from clickhouse_amd import CURRENT_ROW, UNBOUNDED, Frame, following, preceding
    for begin, end in [(CURRENT_ROW, preceding(1)), (following(1), CURRENT_ROW), (following(1), preceding(1)), (preceding(1), preceding(2)),
                       (following(2), following(1))]:
        for make in (Frame.rows, Frame.range):
            with pytest.raises(ValueError):
                make(begin, end)
    with pytest.raises(ValueError):
        Frame.rows(3, CURRENT_ROW)
    with pytest.raises(ValueError):
        Frame(2, UNBOUNDED, UNBOUNDED)
    with pytest.raises(ValueError):
        preceding(-1)
    with pytest.raises(ValueError):
        following(2**64)
    f = Frame.rows(preceding(2**64 - 1), following(0))
    c = f._c()
    assert (c.type, c.begin_kind, c.end_kind, c.begin_offset, c.end_offset) == (K.FRAME_ROWS, K.BOUND_OFFSET_PRECEDING, K.BOUND_OFFSET_FOLLOWING, 2**64 - 1, 0)
    whole = Frame.range(UNBOUNDED, UNBOUNDED)
    assert (whole.begin_kind, whole.end_kind) == (K.BOUND_UNBOUNDED_PRECEDING, K.BOUND_UNBOUNDED_FOLLOWING)
    Frame.rows(preceding(2), preceding(2))
    Frame.rows(following(1), following(1))
    Frame.range(preceding(1), CURRENT_ROW)   # legal; the library answers NOT_IMPLEMENTED


def test_shim_transform_compiles_behind_a_sort(tmp_path):
    # syntax-only: GpuWindowTransform as a driver uses it (no GPU, no library)
    src = tmp_path / "snippet.cpp"
    src.write_text('#include "' + os.path.join(REPO, "clickhouse_amd", "host", "chgpu_shim.hpp") + '"\n' + r'''
using namespace chgpu;
Chunk drive(ContextPtr ctx, std::vector<Chunk> sorted_chunks)
{
    // SELECT k, t, x, row_number() OVER w, rank() OVER w, sum(x) OVER (w ROWS BETWEEN 9 PRECEDING AND CURRENT ROW),
    //        max(x) OVER (w ROWS BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED FOLLOWING), lagInFrame(x, 1, -1) OVER (w ROWS ...)
    // WINDOW w AS (PARTITION BY k ORDER BY t): columns k, t, x
    WindowFrame whole = WindowFrame::rows(CHGPU_BOUND_UNBOUNDED_PRECEDING, 0, CHGPU_BOUND_UNBOUNDED_FOLLOWING, 0);
    std::vector<WindowFunctionDescription> functions;
    functions.push_back(WindowFunctionDescription{CHGPU_WIN_ROW_NUMBER, std::nullopt, WindowFrame{}, 0, 0});
    functions.push_back(WindowFunctionDescription{CHGPU_WIN_RANK, std::nullopt, WindowFrame{}, 0, 0});
    functions.push_back(WindowFunctionDescription{CHGPU_WIN_SUM, 2, WindowFrame::rows(CHGPU_BOUND_OFFSET_PRECEDING, 9, CHGPU_BOUND_CURRENT_ROW, 0), 0, 0});
    functions.push_back(WindowFunctionDescription{CHGPU_WIN_MAX, 2, whole, 0, 0});
    functions.push_back(WindowFunctionDescription{CHGPU_WIN_LAG_IN_FRAME, 2, whole, 1, ~0ull});
    functions.push_back(WindowFunctionDescription{CHGPU_WIN_COUNT, std::nullopt, WindowFrame::range(CHGPU_BOUND_CURRENT_ROW, CHGPU_BOUND_CURRENT_ROW), 0, 0});
    GpuWindowTransform window(ctx, {0}, {1}, functions);
    for (auto & chunk : sorted_chunks)
    {
        sortBlock(chunk, SortDescription{{0, 1, 1}, {1, 1, 1}});
        window.consume(std::move(chunk));
    }
    Chunk out = window.finish();
    uint64_t n = window.numPartitions() + window.numPeerGroups();
    (void)n;
    chgpu_window_frame c = whole.toC();
    (void)c;
    return out;
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_host_only_parts_under_address_and_undefined_sanitizers(tmp_path):
    # frame validation, the frame of a row, the lazy-bounds bookkeeping and the tile arithmetic need no device: a stand-alone program
    # with its own main, run as a plain executable
    exe = tmp_path / "window_driver"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(REPO, "tests", "window_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "window_driver OK" in r.stdout, r.stdout + r.stderr
