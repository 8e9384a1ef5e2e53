"""The gnark-shaped solver on the GPU (zkmi_r1cs_solver_load / zkmi_r1cs_solve_batch /
zkmi_prove_r1cs_submit): every template instance of r1cs_solve_kernel<S>, S = lanes per proof in
{1, 2, 4, 8, 16, 32, 64} and the automatic choice, against the oracle's constraint-by-constraint
solver and against the frontend program's solve (wires, a, b, c, status); proofs of two pipelined
batches against the oracle's prover and against Prover.prove; the refusals of the C ABI.  Modelled on
tests/test_gpu_parity_holes.py::test_solver_every_lane_count_vs_oracle: 70 proofs are two ragged
wavefronts at S = 1 and more than one wavefront at every S."""
import random

import numpy as np
import pytest

from gnark_crypto_primitives_amd import circuits, groth16, lib
from gnark_crypto_primitives_amd.ecc import babyjub_native as bjj
from gnark_crypto_primitives_amd.frontend import compile_circuit
from gnark_crypto_primitives_amd.frontend.api import HINT_LIMBS
from gnark_crypto_primitives_amd.frontend.compile import to_mont_array
from gnark_crypto_primitives_amd.tree import smt_witness
from tests import helpers as H

pytestmark = pytest.mark.gpu

B = 70


def _assignments(name, rng):
    """(circuit, 70 assignments, the planted unsatisfied lanes)"""
    from tests.test_frontend import Mixed, _mixed_expected
    if name == "mixed":
        asg = []
        for i in range(B):
            x = rng.randrange(1 << 16)
            y = x if i % 5 == 0 else rng.randrange(H.R)
            asg.append({"X": x, "Y": y, "Z": _mixed_expected(x, y)})
        asg[3]["Z"] = (asg[3]["Z"] + 1) % H.R                    # a wrong Z
        asg[64] = {"X": 5, "Y": H.R - 2, "Z": 0}                 # 1 / (Y + 2): the divisor is 0
        return Mixed(), asg, {3, 64}
    if name == "smt8":
        asg = [smt_witness.synthetic_inclusion(rng, 8, 1 + i % 7) for i in range(B)]
        asg[69] = dict(asg[69], Root=(asg[69]["Root"] + 1) % H.R)   # a wrong Root
        return circuits.smt_inclusion_circuit(8), asg, {69}
    from gnark_crypto_primitives_amd.ecc import eddsa
    from gnark_crypto_primitives_amd.hash import poseidon_native
    sigs = []
    for _ in range(5):
        sk, nonce, msg = rng.randrange(bjj.ORDER), rng.randrange(bjj.ORDER), rng.randrange(H.R)
        a, r8, S = eddsa.sign_native(sk, nonce, msg, poseidon_native.hash)
        sigs.append({"A": list(a), "R": list(r8), "S": S, "Msg": msg})
    asg = [sigs[i % 5] for i in range(B)]
    asg[1] = dict(asg[1], Msg=(asg[1]["Msg"] + 1) % H.R)
    asg[65] = dict(asg[65], S=(asg[65]["S"] + 1) % bjj.ORDER)
    return circuits.EdDSACircuit(), asg, {1, 65}


class Case:
    """One circuit: its prover, 70 inputs, and the two references computed once -- the oracle's
    solve of every lane and the frontend program's solve on the GPU."""

    def __init__(self, ctx, name):
        from oracle import cref
        rng = random.Random(sum(map(ord, name)))
        circuit, asg, self.bad = _assignments(name, rng)
        self.cc = cc = compile_circuit(circuit)
        self.pk, _, _ = groth16.setup(cc, 7, groth16.gpu_mul(ctx))
        self.prover = groth16.Prover(ctx, cc, self.pk, 7, 5)
        self.inp = np.stack([to_mont_array(cc.assignment_vector(a)) for a in asg])
        self.rs = np.stack([to_mont_array([rng.randrange(H.R), rng.randrange(H.R)]) for _ in asg])
        self.rh = cref.R1csHandle(cc)
        self.oracle = [cref.r1cs_solve(self.rh, x) for x in self.inp]
        # at most 3 of the 70 lanes leave the value comparison, and they are the planted ones
        assert {i for i, o in enumerate(self.oracle) if o[0] != 0} == self.bad and len(self.bad) <= 3
        self.program = self.prover.solve(self.inp, want_wires=True, want_abc=True)
        assert set(np.nonzero(self.program[0])[0]) == self.bad

    def close(self):
        self.prover.close()


@pytest.fixture(scope="module")
def cases(zk_ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(zk_ctx, name)
        return made[name]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("lanes", [1, 2, 4, 8, 16, 32, 64, 0])
@pytest.mark.parametrize("name", ["mixed", "smt8", "eddsa"])
def test_solve_every_lane_count_vs_oracle(zk_ctx, cases, name, lanes):
    case = cases(name)
    cc = case.cc
    info = zk_ctx.r1cs_solver_info(case.prover.load_r1cs_solver(lanes))
    assert info["lanes_per_proof"] == lanes or (lanes == 0 and info["lanes_per_proof"] in (1, 2, 4, 8, 16))
    assert (info["n_instr"], info["n_wires"], info["n_constraints"], info["n_inputs"]) == \
        (cc.instr.shape[0], cc.n_wires, cc.n_constraints, cc.n_inputs)
    if name == "eddsa":       # 1 524 inversions in L-solves, rows of up to 261 terms
        assert info["n_inversions"] >= 1524 and info["longest"] >= 261
    status, wires, abc = case.prover.solve_r1cs(case.inp, want_wires=True, want_abc=True)
    assert set(np.nonzero(status)[0]) == case.bad and set(status.tolist()) <= {0, -5}
    pstatus, pwires, pabc = case.program
    for i, (rc, w, a, b, c) in enumerate(case.oracle):
        if i in case.bad:
            continue
        assert np.array_equal(wires[i], w), (name, lanes, i)
        assert np.array_equal(abc[0][i], a) and np.array_equal(abc[1][i], b) \
            and np.array_equal(abc[2][i], c), (name, lanes, i)
    ok = status == 0
    assert np.array_equal(wires[ok], pwires[ok]) and np.array_equal(abc[:, ok], pabc[:, ok])


@pytest.mark.parametrize("name", ["mixed", "smt8"])
def test_pipelined_proofs_vs_oracle_and_program(zk_ctx, cases, name):
    from oracle import cref
    case = cases(name)
    prover = case.prover
    prover.load_r1cs_solver(0)
    want, wstatus, _ = cref.groth16_prove_batch(case.rh, cref.PkHandle(case.pk), case.inp, case.rs)
    assert set(np.nonzero(wstatus)[0]) == case.bad
    batches = [(case.inp, case.rs), (np.ascontiguousarray(case.inp[:65]), np.ascontiguousarray(case.rs[:65]))]
    for inp, rs in batches:                      # both submitted before the first collect
        prover.submit_r1cs(inp, rs)
    got = [prover.collect() for _ in batches]
    for (inp, rs), (proofs, status) in zip(batches, got):
        n = inp.shape[0]
        assert set(np.nonzero(status)[0]) == {i for i in case.bad if i < n}
        ok = status == 0
        assert np.array_equal(proofs[ok], want[:n][ok])
        pproofs, pstatus = prover.prove(inp, rs)
        assert np.array_equal(status, pstatus) and np.array_equal(proofs[ok], pproofs[ok])


def _solver_desc(cc, keep, **edit):
    kinds, in_ptr, lc_ptr, hcol, hcid, out_ptr, outs = (x.copy() for x in cc.hint_arrays)
    for h, kind in edit.get("hint_kind", {}).items():
        kinds[h] = kind
    arrs = [np.ascontiguousarray(x, dtype=np.uint32) for x in
            (cc.instr, kinds, in_ptr, lc_ptr, np.stack([hcid, hcol], axis=1), out_ptr, outs)]
    keep += arrs
    return lib.R1csSolverDesc(cc.n_public, cc.n_secret, cc.instr.shape[0], len(kinds),
                              *[a.ctypes.data for a in arrs], 0)


def test_refusals_leave_the_context_usable(zk_ctx, cases):
    from tests.test_commitment import RangeCircuit
    case = cases("mixed")
    prover, cc = case.prover, case.cc
    solver = prover.load_r1cs_solver(0)
    prover.submit_r1cs(case.inp, case.rs)
    proofs, status = prover.collect()
    # a description that holds a limbs hint
    keep = []
    with pytest.raises(lib.ZkmiError, match=r"instruction \d+ \(hint 0\): hints limbs \(kind 3\) are "
                                            "not supported on this entry"):
        zk_ctx.r1cs_solver_load(prover.load_r1cs(), _solver_desc(cc, keep, hint_kind={0: HINT_LIMBS}))
    prover.submit_r1cs(case.inp, case.rs)
    again, status2 = prover.collect()
    assert np.array_equal(again, proofs) and np.array_equal(status2, status)
    # a key with commitments, before anything is queued
    rcc = compile_circuit(RangeCircuit())
    assert rcc.commitments
    rpk, _, _ = groth16.setup(rcc, 5, groth16.gpu_mul(zk_ctx))
    rprover = groth16.Prover(zk_ctx, rcc, rpk, 7, 5)
    try:
        with pytest.raises(lib.ZkmiError, match="this key has commitments"):
            zk_ctx.prove_r1cs_submit(rprover.pk_h, solver, case.inp, B, case.rs)
        with pytest.raises(lib.ZkmiError, match=r"hints .* are not supported on this entry"):
            rprover.load_r1cs_solver()
        with pytest.raises(lib.ZkmiError, match="nothing submitted"):      # nothing was queued
            zk_ctx.prove_collect(np.zeros((B, 32), np.uint64), np.zeros(B, np.int32))
    finally:
        rprover.close()
    prover.submit_r1cs(case.inp, case.rs)
    again, status2 = prover.collect()
    assert np.array_equal(again, proofs) and np.array_equal(status2, status)
    assert set(np.nonzero(status)[0]) == case.bad
