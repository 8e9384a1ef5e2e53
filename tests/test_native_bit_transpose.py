"""The digit pass's 32 x 32 bit transpose and sign-pattern digit (csrc/bit_transpose.h) on the host.
tests/native/bit_transpose_check.cpp compares, for every group size k = 1 .. 21, the window words
(the signed kernel's top row at bit 31 included) and the signed and unsigned digits with a
bit-by-bit extraction and with the sign rule restated there, over all-zero, all-ones, one-hot-row,
one-hot-bit and seeded random scalars; complemented and skipped bits come from comb_sign.h.  Built
plain and with -fsanitize=address,undefined; both must pass and print the same."""
from tests import native_build


@native_build.needs_gxx
def test_bit_transpose_native(tmp_path):
    _, out, _ = native_build.run_both(native_build.build("bit_transpose_check.cpp", tmp_path))
    lines = out.splitlines()
    assert lines[0] == "ok full"
    assert lines[1].startswith("ok groups k=1..21: ")
    # 8 words x 32 bits unsigned + the 254 fed windows signed, per group; a few thousand random groups
    assert int(lines[1].split()[3]) > 21 * 150 * (256 + 254)
