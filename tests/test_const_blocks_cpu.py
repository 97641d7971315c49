"""Constant blocks -- full blocks of one symbol, which the host coder passes over in the header phase of a step -- through every
entry point of the range coder: tests/native/const_blocks.cpp, a stand-alone program, built plain and under ASan + UBSan.
Its expected bytes and decoder results come from a per-symbol block coder on the rngcod13 primitives of wr_compat.cpp."""
import os
import shutil
import subprocess
import tempfile

import pytest

from util import ROOT

CSRC = os.path.join(ROOT, "waverange_amd", "csrc")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _builds(flags):
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write("int main(){return 0;}\n")
        return subprocess.run(["g++", "-std=c++17"] + flags + [src, "-o", os.path.join(d, "t")], capture_output=True).returncode == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "asan_ubsan"])
def test_constant_blocks_native(flags):
    if flags is SAN and not _builds(SAN):
        pytest.skip("g++ with ASan/UBSan not available")
    cxx = ["g++", "-std=c++17"] + flags
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "const_blocks")
        vec_o = os.path.join(d, "vec.o")
        subprocess.check_call(cxx + ["-mavx512f", "-mavx512bw", "-mavx512dq", "-mavx512vl", "-c", os.path.join(CSRC, "wr_rangecoder_avx512.cpp"), "-o", vec_o])
        subprocess.check_call(cxx + ["-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "const_blocks.cpp"),
                                     os.path.join(CSRC, "wr_rangecoder.cpp"), os.path.join(CSRC, "wr_compat.cpp"), vec_o, "-o", exe, "-lpthread"])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
        assert "constant blocks run OK" in r.stdout
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
