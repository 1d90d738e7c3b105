"""The ColumnString operators without a GPU: the refusal option is known to the library, and the buffer layouts of string_host.h run
under a sanitizer as a stand-alone program (the checks that need a context are in test_gpu_string_alloc.py)."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


@pytest.fixture(scope="module")
def K():
    from clickhouse_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    _capi.lib()
    return _capi


def test_the_test_option_is_known(K):
    # (process-wide default: no context, no device)
    assert K.lib().chgpu_ctx_set_option(None, b"test_string_fail_alloc", 0) == K.OK


def test_layouts_under_address_and_undefined_sanitizers(tmp_path):
    # every layout is one list run twice, for the size and for the pointers: a stand-alone program with its own main, no device, no library
    exe = tmp_path / "string_layout_driver"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(REPO, "tests", "string_layout_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "string_layout_driver OK" in r.stdout, r.stdout + r.stderr
