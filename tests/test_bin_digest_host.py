"""The digest the binning pre-pass keeps of its pre-records (csrc/bin_digest.h), through the host build: the header is
plain C++ that the kernels share, so a stand-alone host program (host/bin_digest_check.cpp, its own main) calls the very
functions the sweeps call, under the address and undefined-behaviour sanitizers.  Checked there: flipping any single bit
of a pre-record changes the element's contribution; two distinct pre-records that swap places change their group's
digest (both groups' when they lie in two); elements past n contribute nothing; the salt is linear in the index."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "ska-sdp-accelerate-gridding_amd")


def test_digest_mix_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bin_digest_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(PKG, "host", "bin_digest_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.strip() == "bin_digest ok", (out.stdout, out.stderr)


def test_the_header_includes_nothing_of_hip():
    with open(os.path.join(PKG, "csrc", "bin_digest.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes == ["<stdint.h>"]
