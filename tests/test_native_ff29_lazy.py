"""Host build of the lazy memory image the NTT passes keep between them (csrc/ff29.h pack_lazy /
unpack_lazy) under UBSan + ASan: tests/native/ff29_lazy.cpp, a program of its own, run directly."""
from tests import native_build


@native_build.needs_gxx
def test_ff29_lazy_image_host(tmp_path):
    """Round trip limb for limb and the image as a signed 256-bit integer against big-integer
    arithmetic: zero, +-1, limbs all 2^29 - 1, the ends of wred's output range, wred of +-24 r and
    of +-(2^7 r - 1) with limbs at +-(2^31 - 1); canonical 0, 1, r - 1 read as unpack29 reads them.
    Signed overflow or a shift out of range ends the sanitized program, so it is an error here."""
    exes = native_build.build("ff29_lazy.cpp", tmp_path, kinds=("sanitized",))
    assert "ff29 lazy image tests ok" in native_build.run_both(exes, timeout=300)[1]
