"""CPU checks of the C-ABI boundary: the library is built, loads, and exports exactly what
include/gridhip.h declares; without a GPU every compute path refuses loudly (no fallback)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "bindings", "haskell"))
import gen_imports  # noqa: E402  (the header parser the Haskell binding is generated with)

HEADER = os.path.join(ROOT, "include", "gridhip.h")


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gridhip_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_path():
    syms = declared_symbols()
    for need in ("gridhip_grid", "gridhip_convgrid", "gridhip_convgrid2", "gridhip_degrid2",
                 "gridhip_convgrid2_dev", "gridhip_create", "gridhip_last_error"):
        assert need in syms


def test_library_exports_every_declared_symbol():
    from gridhip import _lib
    assert os.path.exists(_lib.LIB_PATH), "libgridhip.so missing: run __graft_entry__.build()"
    lib = C.CDLL(_lib.LIB_PATH)
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, f"declared in gridhip.h but not exported: {missing}"
    # and the Python prototypes cover the header too
    assert sorted(_lib.SIGNATURES) == declared_symbols()


SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double, "const char *": C.c_char_p}


def agrees(ctype, py):
    """one parameter or return type of the header against its ctypes entry: int, int64_t, double and const char * exactly,
    everything else a pointer on both sides - and where the table names the pointee, the header's base type"""
    ctype = " ".join(ctype.replace("*", " * ").split())
    if ctype in SCALARS:
        return py is SCALARS[ctype]
    if "*" not in ctype or py in SCALARS.values():
        return False
    if py is C.c_void_p:
        return True
    if not issubclass(py, C._Pointer):
        return False
    base = ctype.replace("const", "").replace("*", "").strip()
    if ctype.count("*") > 1:  # (a pointer to pointers: gridhip_ctx **, double *const *)
        return py._type_ is C.c_void_p
    return base in SCALARS and py._type_ is SCALARS[base]


def test_agrees_knows_a_wrong_entry():
    assert agrees("int64_t", C.c_int64) and not agrees("int64_t", C.c_int) and not agrees("int", C.c_int64)
    assert agrees("double", C.c_double) and not agrees("double", C.c_void_p) and not agrees("const double *", C.c_double)
    assert agrees("const double *", C.c_void_p) and agrees("double *", C.POINTER(C.c_double))
    assert not agrees("int64_t *", C.POINTER(C.c_int)) and agrees("gridhip_ctx **", C.POINTER(C.c_void_p))
    assert agrees("const char *", C.c_char_p) and not agrees("const char *", C.c_void_p)
    assert not agrees("int64_t", C.c_void_p) and not agrees("void *", C.c_int64)


def test_python_prototypes_match_the_header():
    """_lib.SIGNATURES is written by hand: every entry against the header's prototype - arity, each parameter's type
    and the return type (a c_int where the header says int64_t would pass every other CPU test)."""
    from gridhip import _lib
    protos = gen_imports.prototypes()
    assert sorted(name for _, name, _ in protos) == sorted(_lib.SIGNATURES)
    wrong = []
    for ret, name, params in protos:
        res, args = _lib.SIGNATURES[name]
        if len(args) != len(params):
            wrong.append(f"{name}: {len(args)} argtypes for {len(params)} parameters")
            continue
        if not agrees(ret, res):
            wrong.append(f"{name}: returns {ret}, restype {res.__name__}")
        wrong += [f"{name}: parameter {i} `{t} {pname}` is {py.__name__}"
                  for i, ((t, pname), py) in enumerate(zip(params, args)) if not agrees(t, py)]
    assert not wrong, "\n".join(wrong)


def test_library_is_gfx950_code_object():
    from gridhip import _lib
    out = subprocess.run(["strings", "-a", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out


def test_version_and_strerror():
    from gridhip import _lib
    lib = _lib.load()
    assert lib.gridhip_version() >= 100
    assert lib.gridhip_strerror(0) == b"ok"
    assert b"argument" in lib.gridhip_strerror(-1)


def test_no_gpu_means_loud_failure_not_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present; covered by the gpu tests")
    import gridhip
    with pytest.raises(gridhip.GridHipError) as ei:
        gridhip.Context(0)
    assert ei.value.code == gridhip._lib.ENODEV


def test_null_context_is_rejected():
    from gridhip import _lib
    lib = _lib.load()
    assert lib.gridhip_synchronize(None) == _lib.EINVAL
    assert lib.gridhip_set_option(None, b"tile", 64) == _lib.EINVAL
    assert lib.gridhip_last_error(None) == b"null context"


def test_module_level_degrid2_passes_out_through(monkeypatch):
    import numpy as np
    import gridhip

    class Stub:
        def degrid2(self, gcf, a, p, wbin, out=None):
            return out
    monkeypatch.setitem(gridhip._default, 0, Stub())
    a, out = np.zeros((2, 2), dtype=np.complex128), np.zeros(3, dtype=np.complex128)
    assert gridhip.degrid2(None, a, None, None, out=out) is out and gridhip.degrid2(None, a, None, None, out) is out
    assert gridhip.degrid2(None, a, None, None) is None
