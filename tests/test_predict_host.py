"""CPU checks of prediction (a model image -> visibilities): the library, the header and the ctypes table carry the four
entry points, the version says so, the Python binding has Context.predict, NULL-context and bad-argument calls are
refused without a device, and host/predict_check.cpp (gridding.hpp's predict / predict_aw) compiles and links against
include/gridhip.h and libgridhip.so.  The GPU half runs predict_check."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "host")
LIBDIR = os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd", "lib")
HEADER = os.path.join(ROOT, "include", "gridhip.h")
NEW = ("gridhip_predict", "gridhip_predict_dev", "gridhip_predict_aw", "gridhip_predict_aw_dev")


def build(tmp_path):
    exe = str(tmp_path / "predict_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(HOST, "predict_check.cpp"),
                           "-L" + LIBDIR, "-lgridhip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_new_symbols_are_declared_exported_and_bound():
    from gridhip import _lib
    lib = _lib.load()
    src = open(HEADER).read()
    for name in NEW:
        assert f"int {name}(" in src, name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_version():
    from gridhip import _lib
    assert _lib.load().gridhip_version() >= 140


def test_python_binding_has_predict():
    import gridhip
    assert callable(getattr(gridhip.Context, "predict"))


def test_null_context_and_bad_arguments_are_refused_without_a_device():
    import ctypes as C
    from gridhip import _lib
    lib = _lib.load()
    model = np.zeros((10, 10))
    u = np.zeros(4)
    out = np.full(4, 7 + 7j)
    p = lambda a: C.c_void_p(a.ctypes.data)
    for dev in (False, True):
        fn = lib.gridhip_predict_dev if dev else lib.gridhip_predict
        # a well-formed call, a bad kind, a NULL model, a NULL vis_out: no context, so EINVAL before anything
        assert fn(None, 0, 0, 0, 0, 0, 0, None, 0.1, 100, p(model), 4, p(u), p(u), p(u), 1, None, p(out)) == _lib.EINVAL
        assert fn(None, 9, 0, 0, 0, 0, 0, None, 0.1, 100, p(model), 4, p(u), p(u), p(u), 1, None, p(out)) == _lib.EINVAL
        assert fn(None, 0, 0, 0, 0, 0, 0, None, 0.1, 100, None, 4, p(u), p(u), p(u), 1, None, p(out)) == _lib.EINVAL
        assert fn(None, 0, 0, 0, 0, 0, 0, None, 0.1, 100, p(model), 4, p(u), p(u), p(u), 1, None, None) == _lib.EINVAL
        fa = lib.gridhip_predict_aw_dev if dev else lib.gridhip_predict_aw
        assert fa(None, 0.1, 100, 1, 1, 5, 1, None, None, None, p(model), 4, p(u), p(u), p(u), 1, None, None, None,
                  p(out)) == _lib.EINVAL
    assert np.all(out == 7 + 7j)  # (never touched)


def test_python_predict_without_a_device_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present; covered by tests/test_gpu_predict.py")
    import gridhip
    with pytest.raises(gridhip.GridHipError):
        gridhip.Context(0)


def test_cpp_predict_check_compiles_and_links(tmp_path):
    assert os.path.exists(build(tmp_path))


@pytest.mark.gpu
def test_cpp_predict_check_runs(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = dict((l.split()[0], l.split()[1:]) for l in out.stdout.strip().splitlines())
    assert float(lines["adjoint_simple"][0]) < 1e-10
    assert float(lines["adjoint_aw"][0]) < 1e-10
    assert lines["residual"] == ["1"]
    assert lines["error"] == ["-1"]
