"""The byte-range rules of the argument checks (csrc/argrules.h: overlap, span_bytes, the range tables), as a stand-alone
host program under the address and undefined-behaviour sanitizers.  The header is plain C++, so nothing of HIP, of the
library or of Python is involved: the program (host/argrules_check.cpp) includes the header alone and has its own main."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd")


def test_argument_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "argrules_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(PKG, "host", "argrules_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.strip() == "argrules ok", (out.stdout, out.stderr)


def test_the_header_includes_nothing_of_hip():
    with open(os.path.join(PKG, "csrc", "argrules.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert sorted(includes) == ["<cstddef>", "<cstdint>", "<initializer_list>"]
