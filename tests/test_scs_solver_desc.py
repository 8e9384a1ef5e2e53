"""ScsCircuit.solver_description / solve_description (frontend/scs.py): the gnark-shaped export of
a sparse system's solve -- instruction order, InvZero and NBits hints, where the inputs land -- and
its plain-Python interpreter, against the frontend program's own solve.  No GPU."""
import random

import numpy as np
import pytest

from gnark_crypto_primitives_amd import circuits
from gnark_crypto_primitives_amd.ecc import babyjub_native as bjj
from gnark_crypto_primitives_amd.frontend import Public, Secret
from gnark_crypto_primitives_amd.frontend.scs import compile_scs
from gnark_crypto_primitives_amd.hash import poseidon_native
from gnark_crypto_primitives_amd.tree import smt_witness
from tests import helpers as H

R = H.R


class Tiny:                      # as in tests/test_gpu_plonk_witness.py
    X = Secret()
    Y = Public()

    def define(self, api):
        x2 = api.Mul(self.X, self.X)
        x3 = api.Mul(x2, self.X)
        w = api.Sub(api.Mul(api.Add(api.Add(x3, self.X), 5), 3), x2)
        api.AssertIsEqual(w, self.Y)


class Nine:                      # as in tests/test_gpu_plonk_witness.py
    P = Public(9)
    S = Secret()

    def define(self, api):
        acc = self.S
        for i in range(8):
            acc = api.Add(api.Mul(acc, self.P[i]), i + 1)
        api.AssertIsEqual(acc, self.P[8])


def _tiny(rng):
    x = rng.randrange(R)
    return {"X": x, "Y": (3 * (x * x * x + x + 5) - x * x) % R}


def _nine(rng):
    p = [rng.randrange(R) for _ in range(8)]
    s = acc = rng.randrange(R)
    for i in range(8):
        acc = (acc * p[i] + i + 1) % R
    return {"P": p + [acc], "S": s}


def _mixed(rng):
    from tests.test_frontend import _mixed_expected
    x = rng.randrange(1 << 16)
    y = x if rng.randrange(3) == 0 else rng.randrange(R)
    return {"X": x, "Y": y, "Z": _mixed_expected(x, y)}


def _poseidon(rng):
    d = rng.randrange(R)
    return {"Data": d, "Hash": poseidon_native.hash([d])}


def _smt(rng):
    return smt_witness.synthetic_inclusion(rng, 8, 1 + rng.randrange(7))


def _eddsa(rng):
    from gnark_crypto_primitives_amd.ecc import eddsa
    sk, nonce, msg = rng.randrange(bjj.ORDER), rng.randrange(bjj.ORDER), rng.randrange(R)
    a, r8, S = eddsa.sign_native(sk, nonce, msg, poseidon_native.hash)
    return {"A": list(a), "R": list(r8), "S": S, "Msg": msg}


def _mixed_circuit():
    from tests.test_frontend import Mixed
    return Mixed()


CASES = {"tiny": (Tiny, _tiny, 3), "nine": (Nine, _nine, 3), "mixed": (_mixed_circuit, _mixed, 6),
         "poseidon": (circuits.PoseidonCircuit, _poseidon, 2),
         "smt8": (lambda: circuits.smt_inclusion_circuit(8), _smt, 2),
         "eddsa": (circuits.EdDSACircuit, _eddsa, 1)}


@pytest.mark.parametrize("name", list(CASES))
def test_description_solves_what_the_program_solves(name):
    make, assign, count = CASES[name]
    sc = compile_scs(make())
    desc = sc.solver_description()
    xa, xb, xc, n_wires = sc.wiring()
    assert desc["n_wires"] >= n_wires and len(desc["input_wire"]) == sc.n_inputs
    # every gate once, in an order of its own
    gates = [idx for kind, idx in desc["instr"].tolist() if kind == 0]
    assert sorted(gates) == list(range(sc.n_gates))
    # hints: InvZero and NBits alone (no exported hint is a division), one single-term input each
    assert set(desc["hint_kind"].tolist()) <= {1, 2}
    assert np.array_equal(np.diff(desc["hint_in_ptr"]), np.ones(len(desc["hint_kind"]), np.uint32))
    hints = [idx for kind, idx in desc["instr"].tolist() if kind == 1]
    assert hints == list(range(len(desc["hint_kind"])))
    # the public inputs land on the wires of the public gates
    n_pub = sc.n_public - 1
    assert desc["input_wire"][:n_pub].tolist() == xa[:n_pub].tolist()
    rng = random.Random(len(name))
    for _ in range(count):
        inp = sc.assignment_vector(assign(rng))
        want = sc.wire_vectors(*[[col] for col in sc.run_vprogram(inp)[1:]])[0]
        assert sc.last_status == 0
        got, status = sc.solve_description(desc, inp)
        assert status == 0
        assert got[:n_wires] == want


def test_interpreter_flags_a_zero_divisor_and_a_wrong_output():
    sc = compile_scs(_mixed_circuit())
    desc = sc.solver_description()
    ok = _mixed(random.Random(1))
    assert sc.solve_description(desc, sc.assignment_vector(ok))[1] == 0
    wrong = dict(ok, Z=(ok["Z"] + 1) % R)
    assert sc.solve_description(desc, sc.assignment_vector(wrong))[1] == -5
    zero = {"X": 5, "Y": R - 2, "Z": 0}                  # 1 / (Y + 2): the divisor is 0
    assert sc.solve_description(desc, sc.assignment_vector(zero))[1] == -5


def test_other_hints_are_refused_by_name():
    from tests.test_commitment import RangeCircuit
    sc = compile_scs(RangeCircuit())
    with pytest.raises(ValueError, match=r"solver_description: the circuit holds OP_\w+ .*\(\w"):
        sc.solver_description()
