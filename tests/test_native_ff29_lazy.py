"""Host build of the lazy memory image the NTT passes keep between them (csrc/ff29.h pack_lazy /
unpack_lazy) under UBSan + ASan: tests/native/ff29_lazy.cpp, a program of its own, run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_ff29_lazy_image_host(tmp_path):
    """Round trip limb for limb and the image as a signed 256-bit integer against big-integer
    arithmetic: zero, +-1, limbs all 2^29 - 1, the ends of wred's output range, wred of +-24 r and
    of +-(2^7 r - 1) with limbs at +-(2^31 - 1); canonical 0, 1, r - 1 read as unpack29 reads them.
    Signed overflow or a shift out of range ends the sanitized program, so it is an error here."""
    exe = str(tmp_path / "ff29_lazy")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=undefined,address",
                           "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "gnark_crypto_primitives_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "ff29_lazy.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "ff29 lazy image tests ok" in out.stdout
