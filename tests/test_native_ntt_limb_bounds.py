"""The limb form the 29-bit transform chains keep between their passes (csrc/ntt.hip): the schedule
run on the host build of csrc/ff29.h by tests/native/ntt_limb_bounds_check.cpp, a program of its
own, built plain and with -fsanitize=address,undefined.  No GPU."""
import subprocess

import pytest

from tests import native_build

pytestmark = native_build.needs_gxx


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    # the sanitized build at -O2 too, for its run time alone: the schedule takes a third longer at -O1
    plain, sanitized = native_build.build("ntt_limb_bounds_check.cpp", tmp_path_factory.mktemp("ntt_limb_bounds"),
                                          sanitized_opt="-O2")
    return {"plain": plain, "sanitized": sanitized}


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_limb_form_schedule_host(exes, build):
    """First pass with the unit products skipped, ntt_mid29<1, 2, 3>, middle passes, both fused
    passes, forward passes and the a_c * b_c product at log n = 8..12, inputs 0, r - 1, alternating
    and random, as computed and with the worst representative of every product: every limb fits an
    int32, every column sum an int64, |a b| < 64 r^2, every stored value is below the
    (24 + 1.5 (s - 4)) r that ntt.hip states and equals 256-bit integer arithmetic mod r.  A signed
    overflow or a shift out of range ends the sanitized program, so it is an error here."""
    out = subprocess.run([exes[build]], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "ntt limb bounds ok" in out.stdout
    assert out.stdout.count(": ok") == 21 and "FAIL" not in out.stdout
