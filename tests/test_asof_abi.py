"""The C ABI of the ASOF join without a GPU: the five entry points are declared, bound and exported, answer a NULL handle and NULL
out-pointers with BAD_ARGUMENTS and a message, chgpu_asof_free takes NULL, and AsofJoin rejects an unknown dtype before it touches the
library (the checks that need a context are in test_gpu_asof_edges.py)."""
import ctypes as C
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SYMBOLS = ("chgpu_asof_create", "chgpu_asof_add_block", "chgpu_asof_total_rows", "chgpu_asof_probe", "chgpu_asof_free")


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
    assert sorted(n for n in K.declared_symbols() if n.startswith("chgpu_asof_")) == sorted(SYMBOLS)
    header = open(K.HEADER_PATH).read()
    assert "typedef struct chgpu_asof chgpu_asof;" in header
    assert "int chgpu_asof_create(chgpu_ctx * ctx, int key_type, int asof_type, int kind, int inequality, chgpu_asof ** out);" in header
    assert "enum { CHGPU_ASOF_LESS = 1, CHGPU_ASOF_GREATER = 2, CHGPU_ASOF_LESS_OR_EQUALS = 3, CHGPU_ASOF_GREATER_OR_EQUALS = 4 };" in header
    assert (K.ASOF_LESS, K.ASOF_GREATER, K.ASOF_LESS_OR_EQUALS, K.ASOF_GREATER_OR_EQUALS) == (1, 2, 3, 4)


def test_create_rejects_null(K):
    h = C.c_void_p()
    _expect_bad(K, K.lib().chgpu_asof_create(None, K.U64, K.U32, K.JOIN_LEFT, K.ASOF_GREATER_OR_EQUALS, C.byref(h)))
    assert not h.value
    _expect_bad(K, K.lib().chgpu_asof_create(None, K.U64, K.U32, K.JOIN_INNER, K.ASOF_LESS, None))


def test_add_block_total_rows_and_probe_reject_null(K):
    bi, n = C.c_uint64(7), C.c_uint64(7)
    fh, rh = C.c_void_p(), C.c_void_p()
    _expect_bad(K, K.lib().chgpu_asof_add_block(None, None, None, None, None, C.byref(bi)))
    _expect_bad(K, K.lib().chgpu_asof_add_block(None, None, None, None, None, None))
    _expect_bad(K, K.lib().chgpu_asof_total_rows(None, C.byref(n)))
    _expect_bad(K, K.lib().chgpu_asof_total_rows(None, None))
    _expect_bad(K, K.lib().chgpu_asof_probe(None, None, None, None, C.byref(fh), C.byref(rh), C.byref(n)))
    _expect_bad(K, K.lib().chgpu_asof_probe(None, None, None, None, None, None, None))
    assert (bi.value, n.value, fh.value, rh.value) == (7, 7, None, None)   # nothing was written


def test_free_takes_null(K):
    assert K.lib().chgpu_asof_free(None) == K.OK


def test_asof_join_rejects_an_unknown_dtype_before_the_library(K):
    import clickhouse_amd
    from clickhouse_amd.hashjoin import AsofJoin
    assert clickhouse_amd.AsofJoin is AsofJoin
    # (ctx=object(): any use of the context or of a handle would raise something else)
    for bad in ("complex64", "float16", "U3", "bool"):
        with pytest.raises(ValueError, match="key dtype"):
            AsofJoin(K.JOIN_LEFT, key_dtype=bad, ctx=object())
        with pytest.raises(ValueError, match="asof dtype"):
            AsofJoin(K.JOIN_INNER, K.ASOF_LESS, asof_dtype=bad, ctx=object())
