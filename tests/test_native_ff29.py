"""Host build of the GPU field/curve headers: the 9 x 29-bit lazy representation used by the MSM
kernels (csrc/ff29.h, ec29.h) against the reference representation (csrc/ff.h, ec.h)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import native_build

ROOT = native_build.ROOT


@native_build.needs_gxx
def test_ff29_host_unit_tests(tmp_path):
    exes = native_build.build("test_ff29.cpp", tmp_path, kinds=("plain",))
    assert "ff29 tests ok" in native_build.run_both(exes, timeout=300)[1]


@pytest.fixture(scope="module")
def ff29_host_results(tmp_path_factory):
    """tests/native/ff29_ops.cpp under UBSan + ASan (a program of its own, run directly) on the
    operand sets of tests/ff29_ref.py: [(field, op, class, expected, got)]"""
    from tests import ff29_ref
    tmp = tmp_path_factory.mktemp("ff29_ops")
    operands = str(tmp / "operands.bin")
    exes = native_build.build("ff29_ops.cpp", tmp, kinds=("sanitized",))
    recs = ff29_ref.write_operand_file(operands)
    out = native_build.run_both(exes, [operands], timeout=300)[1]
    got = np.array(out.split(), dtype=np.int64).reshape(-1, 9)
    assert len(got) == sum(len(exp) for _, _, _, exp in recs)
    got = got.astype(np.uint32).view(np.int32)
    res, at = [], 0
    for field, op, name, exp in recs:
        res.append((field, op, name, exp, got[at:at + len(exp)]))
        at += len(exp)
    return res


@native_build.needs_gxx
@pytest.mark.parametrize("field", [0, 1], ids=["fr", "fq"])
def test_ff29_host_forms_match_bigint(ff29_host_results, field):
    """The C++ forms (mul, mul_ilp, sqr, mul_add2, wred, pack_canonical) on the host, limb for limb
    against the big-integer reference, on exactly the operand sets the GPU test uses: contract
    edges of limbs and values, values in [2^252, p), products = 0 mod p.  Signed overflow inside
    the contract ends the sanitized program, so it is an error here."""
    from tests import ff29_ref
    seen = set()
    for f, op, name, exp, got in ff29_host_results:
        if f != field:
            continue
        seen.add(op)
        bad = np.nonzero((exp != got).any(axis=1))[0]
        assert not len(bad), (f"{ff29_ref.FIELDS[f]} {ff29_ref.OPS[op]} class {name}: "
                              f"{len(bad)} of {len(exp)} differ, first at element {bad[0]}: "
                              f"got {got[bad[0]].tolist()} want {exp[bad[0]].tolist()}")
    assert seen == set(range(len(ff29_ref.OPS)))


def test_ff29_asm_header_is_what_the_generator_emits(tmp_path):
    """csrc/ff29_asm.h is never edited by hand: tools/gen_ff29_asm.py reproduces it byte for byte."""
    out = tmp_path / "ff29_asm.h"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_ff29_asm.py"), str(out)])
    committed = os.path.join(ROOT, "gnark_crypto_primitives_amd", "csrc", "ff29_asm.h")
    assert out.read_bytes() == open(committed, "rb").read()
