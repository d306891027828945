"""Imagers (gridhip_imager_*), the checks that need no GPU: the header declares them, the library exports them, the ctypes
table and the Haskell import block carry them, Context has `imager`, and every entry point refuses a NULL imager or a
NULL context with GRIDHIP_EINVAL before it touches a device."""
import ctypes as C
import os
import re

from conftest import ROOT

NAMES = ["gridhip_imager_create_dev", "gridhip_imager_create_aw_dev", "gridhip_imager_psf_dev",
         "gridhip_imager_cycle_dev", "gridhip_imager_predict_dev", "gridhip_imager_destroy"]


def test_header_library_and_tables_carry_the_imager():
    from gridhip import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gridhip.h")).read(), flags=re.S)
    assert "typedef struct gridhip_imager gridhip_imager;" in src
    lib = _lib.load()
    for name in NAMES:
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.gridhip_version() >= 150
    assert int(re.search(r"#define GRIDHIP_VERSION (\d+)", src).group(1)) >= 150


def test_python_and_haskell_bindings_carry_the_imager():
    import gridhip
    assert callable(getattr(gridhip.Context, "imager"))
    for attr in ("psf", "pmax", "cycle", "predict", "close"):
        assert hasattr(gridhip.Imager, attr), attr
    hs = open(os.path.join(ROOT, "bindings", "haskell", "GridHip.hs")).read()
    block = hs[hs.index("-- BEGIN GENERATED IMPORTS"):hs.index("-- END GENERATED IMPORTS")]
    for name in NAMES:
        assert f'foreign import ccall unsafe "{name}"' in block, name
    assert "Ptr (Ptr Imager)" in block and "\ndata Imager\n" in hs
    head = hs[hs.index("module GridHip"):hs.index(") where")]
    for wrapper in ("withImager", "imagerCycleIO"):
        assert wrapper in head and re.search(rf"^{wrapper} ::", hs, flags=re.M), wrapper


def test_null_imager_and_null_context_are_refused():
    from gridhip import _lib
    lib = _lib.load()
    x = (C.c_double * 8)()
    p = C.cast(x, C.c_void_p)
    pm = C.c_double(7.0)
    assert lib.gridhip_imager_cycle_dev(None, p, p, p, p) == _lib.EINVAL
    assert lib.gridhip_imager_predict_dev(None, p, None, p) == _lib.EINVAL
    assert lib.gridhip_imager_psf_dev(None, p, C.byref(pm)) == _lib.EINVAL and pm.value == 7.0
    assert lib.gridhip_imager_destroy(None) == _lib.OK
    h = C.c_void_p(0x1234)  # a refused creation hands back NULL, not what was there
    assert lib.gridhip_imager_create_dev(None, 0, 0, 0, 0, 0, 0, None, 0.1, 640, 1, p, p, p, 1, C.byref(h)) == _lib.EINVAL
    assert not h.value
    h = C.c_void_p(0x1234)
    assert lib.gridhip_imager_create_aw_dev(None, 0.1, 640, 1, 1, 5, 1, p, p, p, 1, p, p, p, 1, p, p,
                                            C.byref(h)) == _lib.EINVAL
    assert not h.value
    assert all(v == 0.0 for v in x)
