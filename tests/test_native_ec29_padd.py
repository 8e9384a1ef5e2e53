"""Host build of csrc/ec29.h's sums of two accumulators (padd29) and of the packed partials that the
MSM accumulate kernels hand to the chunk reduction, against csrc/ec.h (tests/native/
test_ec29_padd.cpp): a program of its own under UBSan + ASan, run directly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_ec29_padd_host_sanitized(tmp_path):
    """G1 and G2: sums of 1-40 mixed additions on both sides, P + P, P + (-P), infinity on either
    side and on both, and chains of 64 sums on packed intermediates, each compared with ec.h's
    padd after to_affine.  Signed overflow inside the documented bounds ends the program."""
    exe = str(tmp_path / "test_ec29_padd")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=undefined,address",
                           "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "gnark_crypto_primitives_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "test_ec29_padd.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "g1: ok" in out.stdout and "g2: ok" in out.stdout
    assert "ec29 padd tests ok" in out.stdout
