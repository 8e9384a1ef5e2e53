"""Host build of csrc/ec29.h's sums of two accumulators (padd29) and of the packed partials that the
MSM accumulate kernels hand to the chunk reduction, against csrc/ec.h (tests/native/
test_ec29_padd.cpp): a program of its own under UBSan + ASan, run directly."""
from tests import native_build


@native_build.needs_gxx
def test_ec29_padd_host_sanitized(tmp_path):
    """G1 and G2: sums of 1-40 mixed additions on both sides, P + P, P + (-P), infinity on either
    side and on both, and chains of 64 sums on packed intermediates, each compared with ec.h's
    padd after to_affine.  Signed overflow inside the documented bounds ends the program."""
    exes = native_build.build("test_ec29_padd.cpp", tmp_path, kinds=("sanitized",))
    out = native_build.run_both(exes, timeout=300)[1]
    assert "g1: ok" in out and "g2: ok" in out
    assert "ec29 padd tests ok" in out
