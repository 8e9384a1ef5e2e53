"""The digit pass's 32 x 32 bit transpose and sign-pattern digit (csrc/bit_transpose.h) on the host.
tests/native/bit_transpose_check.cpp compares, for every group size k = 1 .. 21, the window words
(the signed kernel's top row at bit 31 included) and the signed and unsigned digits with a
bit-by-bit extraction and with the sign rule restated there, over all-zero, all-ones, one-hot-row,
one-hot-bit and seeded random scalars; complemented and skipped bits come from comb_sign.h.  Built
plain and with -fsanitize=address,undefined; both must pass and print the same."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_bit_transpose_native(tmp_path):
    outs = []
    for name, flags in (("plain", ["-O2"]),
                        ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined",
                                       "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("bit_transpose_check_" + name))
        subprocess.check_call(["g++", "-std=c++17", *flags, "-I",
                               os.path.join(ROOT, "gnark_crypto_primitives_amd", "csrc"),
                               os.path.join(ROOT, "tests", "native", "bit_transpose_check.cpp"),
                               "-o", exe])
        run = subprocess.run([exe], text=True, capture_output=True)
        assert run.returncode == 0, run.stdout + run.stderr
        outs.append(run.stdout)
    assert outs[0] == outs[1], "the plain and the sanitized build disagree"
    lines = outs[0].splitlines()
    assert lines[0] == "ok full"
    assert lines[1].startswith("ok groups k=1..21: ")
    # 8 words x 32 bits unsigned + the 254 fed windows signed, per group; a few thousand random groups
    assert int(lines[1].split()[3]) > 21 * 150 * (256 + 254)
