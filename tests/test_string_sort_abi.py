"""The String sort's drop-in boundary without a GPU: include/chgpu.h declares chgpu_string_sort_permutation and chgpu_string_index,
libchgpu.so exports them, the ctypes table carries them, and NULL arguments are answered with BAD_ARGUMENTS and a message."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("chgpu_string_sort_permutation", "chgpu_string_index")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    so = os.path.join(REPO, "clickhouse_amd", "libchgpu.so")
    if not os.path.exists(so):
        g.build()
    return so


def test_header_declares_both_calls():
    with open(os.path.join(REPO, "include", "chgpu.h")) as f:
        header = f.read()
    sort = re.search(r"int chgpu_string_sort_permutation\(([^;]*)\);", header)
    index = re.search(r"int chgpu_string_index\(([^;]*)\);", header)
    assert sort and index
    sort_args = [a.strip() for a in " ".join(sort.group(1).split()).split(",")]
    index_args = [a.strip() for a in " ".join(index.group(1).split()).split(",")]
    assert sort_args == ["chgpu_ctx * ctx", "const chgpu_col * offsets_u64", "const chgpu_col * chars_u8", "const chgpu_col * perm_in_u64",
                         "int descending", "uint64_t limit", "chgpu_col ** perm_out_u64"]
    assert index_args == ["chgpu_ctx * ctx", "const chgpu_col * offsets_u64", "const chgpu_col * chars_u8", "const chgpu_col * indexes_u64",
                          "uint64_t limit", "chgpu_col ** out_offsets_u64", "chgpu_col ** out_chars_u8"]


def test_library_exports_and_ctypes_table(built):
    from clickhouse_amd import _capi
    L = ctypes.CDLL(built)
    for name in CALLS:
        assert hasattr(L, name), name
        assert name in _capi.declared_symbols()
        assert name in _capi.SIGNATURES
        restype, argtypes = _capi.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == 7


def test_null_arguments_are_bad_arguments_with_a_message(built):
    from clickhouse_amd import _capi
    L = _capi.lib()
    out = ctypes.c_void_p()
    out2 = ctypes.c_void_p()
    assert L.chgpu_string_sort_permutation(None, None, None, None, 0, 0, ctypes.byref(out)) == _capi.ERR_BAD_ARGUMENTS
    assert b"NULL" in L.chgpu_last_error()
    assert L.chgpu_string_sort_permutation(None, None, None, None, 1, 5, None) == _capi.ERR_BAD_ARGUMENTS
    assert b"NULL" in L.chgpu_last_error()
    assert L.chgpu_string_index(None, None, None, None, 0, ctypes.byref(out), ctypes.byref(out2)) == _capi.ERR_BAD_ARGUMENTS
    assert b"NULL" in L.chgpu_last_error()
    assert L.chgpu_string_index(None, None, None, None, 3, None, None) == _capi.ERR_BAD_ARGUMENTS
    assert b"NULL" in L.chgpu_last_error()
    assert not out.value and not out2.value


def test_python_mirror_has_the_methods():
    import clickhouse_amd as ch
    assert callable(ch.ColumnString.get_permutation) and callable(ch.ColumnString.index)
