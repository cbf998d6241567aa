"""ccm_map_table_attach and ccm_map_table_handles (include/ccm_hot.h "map-point table", table views) without a GPU: the symbols, their
prototypes, the Python mirror, the NULL-argument answers and the ABI version, which a new pair of functions does not move."""
import ctypes as C
import os
import re

from motioncheck_ccm_slam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "ccm_hot.h")).read(), flags=re.S)


def test_symbols_are_exported_prototyped_and_listed():
    lib = _lib.load()
    txt = _header()
    assert re.search(r"\bint\s+ccm_map_table_attach\(ccm_ctx\* c, ccm_map_table\* table, ccm_map_table\*\* view\);", txt)
    assert re.search(r"\bint\s+ccm_map_table_handles\(const ccm_map_table\*\);", txt)
    for name, n_args in (("ccm_map_table_attach", 3), ("ccm_map_table_handles", 1)):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == n_args, name


def test_the_abi_version_stays_3():
    assert "#define CCM_ABI_VERSION 3" in _header()
    assert _lib.load().ccm_abi_version() == 3 == _lib.ABI_VERSION


def test_null_arguments_are_argument_errors_and_clear_the_view():
    lib = _lib.load()
    assert lib.ccm_map_table_handles(None) == E_ARG
    assert lib.ccm_map_table_attach(None, None, None) == E_ARG
    fake = C.c_void_p(0x1000)                                     # never dereferenced: a NULL among the three is found first
    for ctx, table in ((None, None), (fake, None), (None, fake)):
        view = C.c_void_p(0xdead)
        assert lib.ccm_map_table_attach(ctx, table, C.byref(view)) == E_ARG
        assert view.value is None
    assert lib.ccm_map_table_attach(fake, fake, None) == E_ARG


def test_python_mirror_and_documents_name_the_calls():
    from motioncheck_ccm_slam_amd.tracking import MapPointTable
    assert callable(MapPointTable.attach) and callable(MapPointTable.handles)
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "ccm_map_table_attach" in open(os.path.join(ROOT, doc)).read(), doc
