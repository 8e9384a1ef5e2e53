"""The gnark-shaped solver with the emulated-product hint on the GPU (kind 7, ZKMI_HINTS_EMULATED,
r1cs_solve_kernel<S, 2>): direct hint calls on every lane count against the oracle's gnark-style
solver (its own bit-by-bit division) and the frontend program's solve; circuits over an emulated
field proved from inputs, two batches in flight, against the oracle's prover and Prover.submit; the
refusals of the C ABI.  70 proofs are two ragged wavefronts at S = 1 and more than one wavefront at
every S."""
import random

import numpy as np
import pytest

from gnark_crypto_primitives_amd import groth16, lib, verify
from gnark_crypto_primitives_amd.frontend import compile_circuit
from gnark_crypto_primitives_amd.frontend.compile import to_mont_array
from gnark_crypto_primitives_amd.std import emulated as em
from tests import helpers as H
from tests.r1cs_plan_harness import NO_KEYS, EmulDirect, emul_direct_assignments
from tests.test_emulated import ArithCircuit, FormatCircuit, format_assignment

pytestmark = pytest.mark.gpu

B = 70
NAME = r"emulated product \(kind 7\)"


# ---------------------------------------------------------------------------------------------
# direct hint calls, no commitment: every shape and modulus of tests/test_native_r1cs_emul.py
class DirectCase:
    def __init__(self, ctx):
        from oracle import cref
        self.cc = cc = compile_circuit(EmulDirect())
        self.bad = {0, 63, 64}
        asg = emul_direct_assignments(B, random.Random(44), bad=self.bad)
        self.pk, _, _ = groth16.setup(cc, 7, groth16.gpu_mul(ctx))
        self.prover = groth16.Prover(ctx, cc, self.pk, 7, 5)
        self.inp = np.stack([to_mont_array(cc.assignment_vector(a)) for a in asg])
        rh, ch = cref.R1csHandle(cc), cref.CommitKeysHandle(NO_KEYS)
        self.oracle = [cref.r1cs_solve_ex(rh, ch, x)[:5] for x in self.inp]
        assert {i for i, o in enumerate(self.oracle) if o[0] != 0} == self.bad
        self.program = self.prover.solve(self.inp, want_wires=True, want_abc=True)
        assert set(np.nonzero(self.program[0])[0]) == self.bad


@pytest.fixture(scope="module")
def direct(zk_ctx):
    case = DirectCase(zk_ctx)
    yield case
    case.prover.close()


@pytest.mark.parametrize("lanes", [1, 2, 4, 8, 16, 32, 64])
def test_emul_direct_every_lane_count_vs_oracle_and_program(zk_ctx, direct, lanes):
    cc = direct.cc
    info = zk_ctx.r1cs_solver_info(direct.prover.load_r1cs_solver(lanes, hints="emulated"))
    assert info["lanes_per_proof"] == lanes
    assert (info["n_instr"], info["n_wires"], info["n_constraints"]) == (21, cc.n_wires, cc.n_constraints)
    status, wires, abc = direct.prover.solve_r1cs(direct.inp, want_wires=True, want_abc=True)
    assert set(np.nonzero(status)[0]) == direct.bad and set(status.tolist()) <= {0, -5}
    for i, (rc, w, a, b, c) in enumerate(direct.oracle):
        # the planted lanes too: a wrong public value changes no solved wire
        assert np.array_equal(wires[i], w), (lanes, i)
        if i in direct.bad:     # the oracle leaves the row of a failing assertion unwritten
            continue
        assert np.array_equal(abc[0][i], a) and np.array_equal(abc[1][i], b) \
            and np.array_equal(abc[2][i], c), (lanes, i)
    pstatus, pwires, pabc = direct.program
    ok = status == 0
    assert np.array_equal(status, pstatus) and np.array_equal(wires, pwires)
    assert np.array_equal(abc[:, ok], pabc[:, ok])


# ---------------------------------------------------------------------------------------------
# circuits over an emulated field: range checks, lookups and a commitment around the products
def _arith_assignments(circ, seed):
    """the 70 assignments and bad lanes of tests/test_gpu_emulated.py::test_emulated_arithmetic"""
    p = circ.params.modulus
    rng = random.Random(seed)
    asg = [circ.assignment(rng.randrange(p), rng.randrange(p)) for _ in range(B)]
    asg[1] = circ.assignment(p - 1, 1)
    asg[2] = circ.assignment(0, 0)
    x = rng.randrange(p)
    asg[3] = circ.assignment(x, x)
    asg[4] = circ.assignment(p - 1, p - 1)
    asg[9] = circ.assignment(x, 5, z=7)
    asg[63] = circ.assignment(x, 6, flag=1)
    asg[64] = circ.assignment(x, 7, s=x)
    limbs = list(asg[69]["X"])
    limbs[2] += 1 << 64
    asg[69] = dict(asg[69], X=limbs)
    return asg, [9, 63, 64, 69]


class CommitCase:
    """One circuit with a commitment: prover, inputs, and the two references computed once -- the
    oracle's proofs and those of the frontend program's path (Prover.submit)."""

    def __init__(self, ctx, cc, asg, bad, seed):
        from oracle import cref
        self.cc, self.bad = cc, set(bad)
        self.pk, self.vk, _ = groth16.setup(cc, seed, groth16.gpu_mul(ctx))
        self.prover = groth16.Prover(ctx, cc, self.pk, 7, 5)
        rng = random.Random(seed)
        self.inp = np.stack([to_mont_array(cc.assignment_vector(a)) for a in asg])
        self.rs = np.stack([to_mont_array([rng.randrange(H.R), rng.randrange(H.R)]) for _ in asg])
        rh, ph, ch = cref.R1csHandle(cc), cref.PkHandle(self.pk), cref.CommitKeysHandle(self.pk)
        self.want = cref.groth16_prove_batch_ex(rh, ph, ch, self.inp, self.rs, 16)[:4]
        # at most 4 lanes leave the value comparison, and they are the planted ones
        assert set(np.nonzero(self.want[3])[0]) == self.bad and len(self.bad) <= 4
        self.prover.submit(self.inp, self.rs)
        self.program = self.prover.collect()
        assert set(np.nonzero(self.program[1])[0]) == self.bad

    def check(self, proofs, status, coms, n):
        want, wcoms, wpoks, wstatus = (x[:n] for x in self.want)
        assert set(np.nonzero(status)[0]) == set(np.nonzero(wstatus)[0]) == {i for i in self.bad if i < n}
        ok = status == 0
        assert np.array_equal(proofs[ok], want[ok])
        assert np.array_equal(coms[ok][:, :-1], wcoms[ok]) and np.array_equal(coms[ok][:, -1], wpoks[ok])
        pproofs, pstatus, pcoms = (x[:n] for x in self.program)
        assert np.array_equal(status, pstatus)
        assert np.array_equal(proofs[ok], pproofs[ok]) and np.array_equal(coms[ok], pcoms[ok])


def _pipelined(zk_ctx, case, lanes):
    prover = case.prover
    info = zk_ctx.r1cs_solver_info(prover.load_r1cs_solver(lanes, hints="emulated"))
    assert info["n_instr"] == case.cc.instr.shape[0]
    assert info["lanes_per_proof"] == lanes or (lanes == 0 and info["lanes_per_proof"] in (1, 2, 4, 8, 16))
    n = len(case.inp)
    short = n - 5 if n > 5 else n - 1
    batches = [(case.inp, case.rs), (np.ascontiguousarray(case.inp[:short]), np.ascontiguousarray(case.rs[:short]))]
    for inp, rs in batches:                      # both submitted before the first collect
        prover.submit_r1cs(inp, rs)
    got = [prover.collect() for _ in batches]
    for (inp, rs), (proofs, status, coms) in zip(batches, got):
        case.check(proofs, status, coms, inp.shape[0])
    return got[0]


@pytest.mark.parametrize("params,lanes,seed", [(em.BN254Fr, 1, 1), (em.Secp256k1Fp, 64, 64), (em.BN254Fp, 0, 8)],
                         ids=lambda v: getattr(v, "name", str(v)))
def test_emulated_arithmetic_from_inputs_pipelined(zk_ctx, params, lanes, seed):
    circ = ArithCircuit(params)
    asg, bad = _arith_assignments(circ, seed)
    case = CommitCase(zk_ctx, compile_circuit(circ), asg, bad, 70 + seed)
    try:
        proofs, status, coms = _pipelined(zk_ctx, case, lanes)
        i = 0
        pub = list(asg[i]["Z"]) + [asg[i]["Flag"]]
        assert status[i] == 0 and verify.verify(case.vk, pub, proofs[i], coms[i, :-1], coms[i, -1])
        assert not verify.verify(case.vk, [pub[0] + 1] + pub[1:], proofs[i], coms[i, :-1], coms[i, -1])
    finally:
        case.prover.close()


@pytest.fixture(scope="module")
def format_case(zk_ctx):
    """ecc/format's TE -> RTE conversion, the reference's own emulated gadget: 8 proofs, one bad"""
    rng = random.Random(5)
    asg = [format_assignment(False)] + \
        [format_assignment(False, rng.randrange(H.R), rng.randrange(H.R)) for _ in range(7)]
    asg[6] = format_assignment(False, 3, 4, bad=True)
    case = CommitCase(zk_ctx, compile_circuit(FormatCircuit(False)), asg, [6], 90)
    yield case
    case.prover.close()


def test_format_te_to_rte_from_inputs(zk_ctx, format_case):
    _pipelined(zk_ctx, format_case, 0)


# ---------------------------------------------------------------------------------------------
def test_refusals_through_the_abi_leave_the_context_usable(zk_ctx, direct, format_case):
    first = _pipelined(zk_ctx, format_case, 0)
    # the emulated product stays outside ZKMI_HINTS_STD, by name
    with pytest.raises(lib.ZkmiError, match=r"instruction 0 \(hint 0\): hints " + NAME +
                                            " are not supported on this entry"):
        direct.prover.load_r1cs_solver(0, hints="std")
    with pytest.raises(lib.ZkmiError, match="hints " + NAME + " are not supported on this entry"):
        format_case.prover.load_r1cs_solver(0, hints="std")
    # a modulus below 2^224: the top limb's expression of hint 0 loses its only term
    cc = direct.cc
    kinds, in_ptr, lc_ptr, hcol, hcid, out_ptr, outs = (np.array(x) for x in cc.hint_arrays)
    e = int(in_ptr[1]) - 1                              # the last expression of hint 0
    assert lc_ptr[e + 1] - lc_ptr[e] == 1
    t = int(lc_ptr[e])
    hcol, hcid = np.delete(hcol, t), np.delete(hcid, t)
    lc_ptr = lc_ptr.copy()
    lc_ptr[e + 1:] -= 1
    arrs = [np.ascontiguousarray(x, dtype=np.uint32) for x in
            (cc.instr, kinds, in_ptr, lc_ptr, np.stack([hcid, hcol], axis=1), out_ptr, outs)]
    sd = lib.R1csSolverDesc(cc.n_public, cc.n_secret, cc.instr.shape[0], len(kinds),
                            *[a.ctypes.data for a in arrs], 0, lib.HINTS_EMULATED)
    with pytest.raises(lib.ZkmiError, match=r"instruction 0 \(hint 0\): the modulus of " + NAME +
                                            r" is below 2\^224"):
        zk_ctx.r1cs_solver_load(direct.prover.load_r1cs(), sd)
    sd.hint_set = 2
    with pytest.raises(lib.ZkmiError, match=r"hint_set must be ZKMI_HINTS_BASIC \(0\) or ZKMI_HINTS_STD \(1\)"):
        zk_ctx.r1cs_solver_load(direct.prover.load_r1cs(), sd)
    # a solve alone cannot supply the commitment of an emulated circuit
    format_case.prover.load_r1cs_solver(0, hints="emulated")
    with pytest.raises(lib.ZkmiError, match="needs? a proving key.*zkmi_prove_r1cs_submit"):
        format_case.prover.solve_r1cs(format_case.inp)
    # a good batch on the same context afterwards equals the earlier result
    format_case.prover.submit_r1cs(format_case.inp, format_case.rs)
    again = format_case.prover.collect()
    assert all(np.array_equal(x, y) for x, y in zip(again, first))
