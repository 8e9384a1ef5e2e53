"""The emulated-product hint in the C ABI (the method of tests/test_abi_r1cs_solver.py): a C compiler
sees ZKMI_HINT_EMULMUL = 7 and ZKMI_HINTS_EMULATED = 3 in include/zkmi.h, lib.py carries the same
number, and zkmi_r1cs_solver_desc is as large as it was."""
import ctypes as C
import os
import subprocess

import pytest

from gnark_crypto_primitives_amd import groth16, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_lib_agree_on_kind_7_and_set_3(tmp_path):
    prog = ['#include <stdio.h>', '#include "zkmi.h"', 'int main(void) {',
            'printf("%d %d %d %d %zu\\n", ZKMI_HINT_EMULMUL, ZKMI_HINTS_EMULATED, ZKMI_HINTS_BASIC, '
            'ZKMI_HINTS_STD, sizeof(zkmi_r1cs_solver_desc));', 'return 0; }']
    src = tmp_path / "emul.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "emul"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    kind, emulated, basic, std, size = (int(x) for x in subprocess.check_output([str(exe)], text=True).split())
    assert (kind, emulated, basic, std) == (7, 3, 0, 1)
    assert (lib.HINTS_BASIC, lib.HINTS_STD, lib.HINTS_EMULATED) == (0, 1, 3)
    # the set is read as bits: 1 = the std kinds, 2 = the emulated product
    assert lib.HINTS_EMULATED == lib.HINTS_STD | 2
    # eleven 4- and 8-byte fields as before: 4 counts, 7 pointers, lanes_per_proof and hint_set
    cls = lib.R1csSolverDesc
    assert size == C.sizeof(cls) == 4 * 4 + 7 * C.sizeof(C.c_void_p) + 2 * 4


def test_load_r1cs_solver_knows_the_three_sets_by_name():
    class Stop(Exception):
        pass

    class P:
        r1cs_solver_h = None

        @property
        def cc(self):
            raise Stop          # reached only once the name has been accepted
    for name in ("basic", "std", "emulated"):
        with pytest.raises(Stop):
            groth16.Prover.load_r1cs_solver(P(), 0, hints=name)
    with pytest.raises(ValueError, match='hints must be "basic", "std" or "emulated"'):
        groth16.Prover.load_r1cs_solver(P(), 0, hints="all")
