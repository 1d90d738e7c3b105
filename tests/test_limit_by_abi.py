"""The C ABI of DISTINCT / LIMIT BY without a GPU: every entry point is declared, bound and exported, answers a NULL handle with
BAD_ARGUMENTS and a message, the Python classes reject an unknown dtype before they touch the library, the shim's transforms compile, and
the host-only parts run under a sanitizer as a stand-alone program (the checks that need a context are in test_gpu_limit_by.py)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SYMBOLS = ("chgpu_limit_by_create", "chgpu_limit_by_filter_block", "chgpu_limit_by_keys", "chgpu_limit_by_free")


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
    header = open(K.HEADER_PATH).read()
    assert "typedef struct chgpu_limit_by chgpu_limit_by;" in header
    assert "uint64_t group_length, uint64_t group_offset, uint64_t size_hint, chgpu_limit_by ** out" in header


def test_create_rejects_null(K):
    h = C.c_void_p()
    _expect_bad(K, K.lib().chgpu_limit_by_create(None, K.U64, 1, 0, 0, C.byref(h)))
    _expect_bad(K, K.lib().chgpu_limit_by_create(None, K.U64, 5, 2, 100, None))


def test_filter_block_and_keys_reject_null(K):
    out, n = C.c_void_p(), C.c_uint64(0)
    _expect_bad(K, K.lib().chgpu_limit_by_filter_block(None, None, 0, 0, None, C.byref(out), C.byref(n)))
    _expect_bad(K, K.lib().chgpu_limit_by_filter_block(None, None, 0, 0, None, None, None))
    _expect_bad(K, K.lib().chgpu_limit_by_keys(None, C.byref(n)))
    _expect_bad(K, K.lib().chgpu_limit_by_keys(None, None))


def test_free_takes_null(K):
    assert K.lib().chgpu_limit_by_free(None) == K.OK


def test_the_test_options_are_known(K):
    # (process-wide defaults: no context, no device)
    for name in (b"test_limit_by_fail_alloc", b"test_limit_by_grid"):
        assert K.lib().chgpu_ctx_set_option(None, name, 0) == K.OK


def test_python_classes_reject_an_unknown_dtype_before_the_library(K):
    from clickhouse_amd.limit_by import BlockKeys, Distinct, LimitBy, distinct_block, limit_by_block
    with pytest.raises(ValueError):
        LimitBy("complex64", 1, ctx=object())
    with pytest.raises(ValueError):
        LimitBy("U3", 2, 1, ctx=object())
    with pytest.raises(ValueError):
        Distinct("float16", ctx=object())
    with pytest.raises(ValueError):
        LimitBy("uint64", -1, ctx=object())
    with pytest.raises(ValueError):
        LimitBy("uint64", 1, offset=-1, ctx=object())
    import clickhouse_amd
    assert clickhouse_amd.LimitBy is LimitBy and clickhouse_amd.Distinct is Distinct and clickhouse_amd.BlockKeys is BlockKeys
    assert clickhouse_amd.distinct_block is distinct_block and clickhouse_amd.limit_by_block is limit_by_block


def test_shim_transforms_compile_in_a_chain(tmp_path):
    # syntax-only: GpuDistinctTransform / GpuLimitByTransform as a driver uses them (no GPU, no library)
    src = tmp_path / "snippet.cpp"
    src.write_text('#include "' + os.path.join(REPO, "clickhouse_amd", "host", "chgpu_shim.hpp") + '"\n' + r'''
using namespace chgpu;
size_t drive(ContextPtr ctx, std::vector<Chunk> chunks)
{
    // SELECT DISTINCT a, b ... LIMIT 100, then LIMIT 2 OFFSET 1 BY a over what is left
    GpuDistinctTransform distinct(ctx, {0, 1}, 100);
    GpuLimitByTransform limit_by(ctx, {0}, 2, 1, 1000);
    size_t next = 0, rows = 0;
    executeChain([&](Chunk & c) { if (next == chunks.size()) return false; c = std::move(chunks[next++]); return true; },
                 {&distinct, &limit_by}, [&](Chunk c) { rows += c.num_rows; });
    return rows + distinct.passed_rows + limit_by.passed_rows + distinct.keys() + limit_by.keys() + distinct.getName().size();
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_host_only_parts_under_address_and_undefined_sanitizers(tmp_path):
    # table geometry and growth, the argument checks, the plan choice, the slot bytes the rank plan passes over and the plan line
    # need no device: a stand-alone program with its own main, run as a plain executable
    exe = tmp_path / "limit_by_driver"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(REPO, "tests", "limit_by_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "limit_by_driver OK" in r.stdout, r.stdout + r.stderr
