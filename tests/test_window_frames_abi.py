"""chgpu_window_evaluate_framed without a GPU: the entry point is declared, bound and exported, its contract is in the header, NULL handles
and outputs answer BAD_ARGUMENTS, FramedWindow rejects a RANGE offset without its order column, a float order column and wrong lengths
before it touches the library, the shim compiles a framed RANGE-offset max over a descending order, and the host-only parts (the search,
the mask and table arithmetic, the plans) run under a sanitizer as a stand-alone program.  What needs a context is in
test_gpu_window_frames.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SYMBOL = "chgpu_window_evaluate_framed"


@pytest.fixture(scope="module")
def K():
    from clickhouse_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    _capi.lib()
    return _capi


def test_entry_point_is_declared_bound_and_exported(K):
    assert SYMBOL in K.declared_symbols() and SYMBOL in K.SIGNATURES
    assert getattr(K.lib(), SYMBOL)
    restype, argtypes = K.SIGNATURES[SYMBOL]
    assert len(argtypes) == 9 and len(K.SIGNATURES["chgpu_window_evaluate"][1]) == 7   # + order, descending
    assert K.lib().chgpu_abi_version() == 1


def test_contract_is_in_the_header(K):
    header = " ".join(open(K.HEADER_PATH).read().split())
    assert "int chgpu_window_evaluate_framed(chgpu_window * window, int function, const chgpu_window_frame * frame /* NULL = default */," in header
    for phrase in ("MIN / MAX over every legal frame", "x[j] >= x[i] - k", "x[j] > x[i] + k", "An offset of 0 gives gs / ge", "as if in unbounded integers",
                   "compareValuesWithOffset", "exactly one ORDER BY column", "every index a kernel forms stays inside [ps, pe] and every loop ends",
                   "A failed call allocates nothing"):
        assert phrase in header, phrase


def test_null_window_and_null_out_are_bad_arguments(K):
    out = C.c_void_p()
    frame = K.WindowFrame(K.FRAME_RANGE, K.BOUND_OFFSET_PRECEDING, K.BOUND_CURRENT_ROW, 0, 5, 0)
    for rc in (K.lib().chgpu_window_evaluate_framed(None, K.WIN_COUNT, C.byref(frame), None, 0, None, 0, 0, C.byref(out)),
               K.lib().chgpu_window_evaluate_framed(None, K.WIN_ROW_NUMBER, None, None, 1, None, 0, 0, None)):
        assert rc == K.ERR_BAD_ARGUMENTS
        with pytest.raises(K.ChgpuError) as e:
            K.check(rc)
        assert e.value.code == K.ERR_BAD_ARGUMENTS and "NULL" in str(e.value)
    assert not out.value


def test_framed_window_rejects_before_the_library(K):
    import clickhouse_amd
    from clickhouse_amd import CURRENT_ROW, UNBOUNDED, Frame, following, preceding
    from clickhouse_amd.window import FramedWindow, Window
    assert clickhouse_amd.FramedWindow is FramedWindow
    # a handle-less object stands for a window of four rows; nothing below may reach the library
    w = Window.__new__(Window)
    w.rows, w.ctx, w._h = 4, object(), None
    week = Frame.range(preceding(7), CURRENT_ROW)
    with pytest.raises(ValueError):
        w.over(week)                                                   # a RANGE offset without its order column
    with pytest.raises(ValueError):
        w.over(Frame.range(UNBOUNDED, following(0)))                   # an offset of 0 is still an offset bound
    with pytest.raises(ValueError):
        w.over(week, order=np.zeros(4, dtype=np.float64))
    with pytest.raises(ValueError):
        w.over(week, order=np.zeros(4, dtype=np.float32), descending=True)
    with pytest.raises(ValueError):
        w.over(week, order=np.zeros(3, dtype=np.int64))
    with pytest.raises(ValueError):
        w.over(week, order=np.zeros(4, dtype=np.float16))
    with pytest.raises(ValueError):
        w.over(Frame.rows(preceding(7), CURRENT_ROW), order=np.zeros(4, dtype=np.int64))   # an order column nothing reads
    with pytest.raises(ValueError):
        w.over(None, order=np.zeros(4, dtype=np.int64))
    with pytest.raises(ValueError):
        w.over((1, 1, 7, 2, 0))
    fw = w.over(Frame.rows(preceding(50), following(50)))
    assert isinstance(fw, FramedWindow) and fw.order is None and fw.descending is False
    with pytest.raises(ValueError):
        fw.max(np.zeros(3, dtype=np.int64))
    with pytest.raises(ValueError):
        fw.min(np.zeros(4, dtype=np.float16))
    with pytest.raises(ValueError):
        fw.sum(None)
    with pytest.raises(ValueError):
        fw.evaluate_column(K.WIN_COUNT, np.zeros(4, dtype=np.int64))
    with pytest.raises(ValueError):
        fw.lag_in_frame(np.zeros(4, dtype=np.int64), offset=-1)


def test_shim_compiles_a_framed_range_offset_max_over_a_descending_order(tmp_path):
    src = tmp_path / "snippet.cpp"
    src.write_text('#include "' + os.path.join(REPO, "clickhouse_amd", "host", "chgpu_shim.hpp") + '"\n' + r'''
using namespace chgpu;
Chunk drive(ContextPtr ctx, Chunk sorted)
{
    // SELECT k, t, x, max(x) OVER (PARTITION BY k ORDER BY t DESC RANGE BETWEEN 604800 PRECEDING AND CURRENT ROW),
    //        min(x) OVER (PARTITION BY k ORDER BY t DESC ROWS BETWEEN 50 PRECEDING AND 50 FOLLOWING), rank() OVER (...): columns k, t, x
    std::vector<WindowFunctionDescription> functions;
    functions.push_back(WindowFunctionDescription{CHGPU_WIN_MAX, 2, WindowFrame::range(CHGPU_BOUND_OFFSET_PRECEDING, 604800, CHGPU_BOUND_CURRENT_ROW, 0), 0, 0, true});
    functions.push_back(WindowFunctionDescription{CHGPU_WIN_MIN, 2, WindowFrame::rows(CHGPU_BOUND_OFFSET_PRECEDING, 50, CHGPU_BOUND_OFFSET_FOLLOWING, 50), 0, 0, true});
    functions.push_back(WindowFunctionDescription{CHGPU_WIN_RANK, std::nullopt, WindowFrame{}, 0, 0});   // the five-value form still stands
    GpuWindowTransform window(ctx, {0}, {1}, functions, /*order_descending=*/true);
    window.consume(std::move(sorted));
    return window.finish();
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_host_only_parts_under_address_and_undefined_sanitizers(tmp_path):
    exe = tmp_path / "window_frames_driver"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(REPO, "tests", "window_frames_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "window_frames_driver OK" in r.stdout, r.stdout + r.stderr
