"""The gnark-shaped solver with the hints of ZKMI_HINTS_STD on the GPU (r1cs_solve_kernel<S, true>:
limbs, lookup multiplicities, byte operations; zkmi_prove_r1cs_submit stopping at the commitment
hints): every lane count against the oracle's gnark-style solver and the frontend program's solve;
a lookup hint over a 65 536-entry table; proofs, commitments and proofs of knowledge of pipelined
batches against the oracle's prover and against Prover.submit; the address circuit with its
commitment-backed range checks; the refusals of the C ABI.  70 proofs are two ragged wavefronts at
S = 1 and more than one wavefront at every S."""
import random

import numpy as np
import pytest

from gnark_crypto_primitives_amd import groth16, lib, verify
from gnark_crypto_primitives_amd.frontend import compile_circuit
from gnark_crypto_primitives_amd.frontend.compile import Public, Secret, to_mont_array
from tests import helpers as H
from tests.r1cs_plan_harness import HintsPlain, hints_plain_assignments, limbs_of
from tests.test_commitment import RangeCircuit, TwoCommitments

pytestmark = pytest.mark.gpu

B = 70


# ---------------------------------------------------------------------------------------------
# limbs, lookup multiplicities and byte operations, no commitment
class PlainCase:
    def __init__(self, ctx):
        from oracle import cref
        rng = random.Random(3)
        self.cc = cc = compile_circuit(HintsPlain())
        asg = hints_plain_assignments(B, rng)          # lane 0: Z = r - 1, lane 7: a wrong X
        self.bad = {7}
        self.pk, _, _ = groth16.setup(cc, 7, groth16.gpu_mul(ctx))
        self.prover = groth16.Prover(ctx, cc, self.pk, 7, 5)
        self.inp = np.stack([to_mont_array(cc.assignment_vector(a)) for a in asg])
        rh = cref.R1csHandle(cc)
        self.oracle = [cref.r1cs_solve(rh, x) for x in self.inp]
        # at most 3 of the 70 lanes leave the value comparison, and they are the planted ones
        assert {i for i, o in enumerate(self.oracle) if o[0] != 0} == self.bad
        self.program = self.prover.solve(self.inp, want_wires=True, want_abc=True)
        assert set(np.nonzero(self.program[0])[0]) == self.bad


@pytest.fixture(scope="module")
def plain(zk_ctx):
    case = PlainCase(zk_ctx)
    yield case
    case.prover.close()


@pytest.mark.parametrize("lanes", [1, 2, 4, 8, 16, 32, 64, 0])
def test_hints_plain_every_lane_count_vs_oracle_and_program(zk_ctx, plain, lanes):
    cc = plain.cc
    info = zk_ctx.r1cs_solver_info(plain.prover.load_r1cs_solver(lanes, hints="std"))
    assert info["lanes_per_proof"] == lanes or (lanes == 0 and info["lanes_per_proof"] in (1, 2, 4, 8, 16))
    assert (info["n_instr"], info["n_wires"], info["n_constraints"]) == (7, 105, cc.n_constraints)
    status, wires, abc = plain.prover.solve_r1cs(plain.inp, want_wires=True, want_abc=True)
    assert set(np.nonzero(status)[0]) == plain.bad and set(status.tolist()) <= {0, -5}
    for i, (rc, w, a, b, c) in enumerate(plain.oracle):
        if i in plain.bad:
            continue
        assert np.array_equal(wires[i], w), (lanes, i)
        assert np.array_equal(abc[0][i], a) and np.array_equal(abc[1][i], b) \
            and np.array_equal(abc[2][i], c), (lanes, i)
    pstatus, pwires, pabc = plain.program
    ok = status == 0
    assert np.array_equal(wires[ok], pwires[ok]) and np.array_equal(abc[:, ok], pabc[:, ok])


def test_the_default_solver_stays_basic(zk_ctx, plain):
    with pytest.raises(lib.ZkmiError, match=r"instruction 0 \(hint 0\): hints limbs \(kind 3\) are not "
                                            "supported on this entry"):
        plain.prover.load_r1cs_solver(0)
    with pytest.raises(ValueError):
        plain.prover.load_r1cs_solver(0, hints="all")


# ---------------------------------------------------------------------------------------------
# a lookup hint over the table 0 .. 65 535: the zero / convert loops and the counter addressing of
# the real byte tables, without a commitment
TABLE = 1 << 16
WATCHED = (0, 1, 2, 12345, 65534, 65535)       # the counters the circuit weighs


class BigTable:
    X = Public()
    Y = Secret()

    def define(self, api):
        l = api.NewHintLimbs(self.Y, 16, 16)
        q = list(l) + [api.Add(v, 1) for v in l] + [api.Add(l[i], l[(i + 1) % 16]) for i in range(16)] + \
            [api.Add(api.Mul(l[i], 2), l[(i + 5) % 16], 1) for i in range(16)] + \
            [api.Sub(l[i], l[(i + 3) % 16]) for i in range(16)] + [api.Mul(l[i], 65535) for i in range(16)]
        c = api.NewHintCount(q, TABLE)
        api.AssertIsEqual(api.Sum([api.Mul(c[j], 1 + 7 * n) for n, j in enumerate(WATCHED)]), self.X)


def big_table_x(y):
    l = limbs_of(y, 16, 16)
    q = l + [v + 1 for v in l] + [l[i] + l[(i + 1) % 16] for i in range(16)] + \
        [2 * l[i] + l[(i + 5) % 16] + 1 for i in range(16)] + \
        [(l[i] - l[(i + 3) % 16]) % H.R for i in range(16)] + [l[i] * 65535 for i in range(16)]
    assert len(q) == 96
    return sum((1 + 7 * n) * sum(1 for v in q if v == j) for n, j in enumerate(WATCHED)), q


@pytest.fixture(scope="module")
def big_table(zk_ctx):
    """(circuit, loaded system, inputs, the oracle's solve of each, planted lanes)"""
    from oracle import cref
    rng = random.Random(16)
    cc = compile_circuit(BigTable())
    assert cc.n_wires > TABLE and cc.n_constraints <= 4
    asg = []
    for i in range(B):
        # limbs from the watched values and their neighbours, and random ones
        l = [rng.choice(WATCHED + (3, 12344, 32767)) if rng.random() < 0.7 else rng.randrange(TABLE)
             for _ in range(16)]
        l[15] = rng.randrange(0x3000)                   # Y stays below r
        if i == 0:
            l[0], l[1] = 65535, 0                       # queries 65 535 and 65 536 (= l[0] + 1)
        y = sum(v << (16 * j) for j, v in enumerate(l))
        x, q = big_table_x(y)
        if i == 0:
            assert 65535 in q and 65536 in q
        asg.append({"X": x, "Y": y})
    asg[66]["X"] += 1
    inp = np.stack([to_mont_array(cc.assignment_vector(a)) for a in asg])
    rh = cref.R1csHandle(cc)
    oracle = [cref.r1cs_solve(rh, x) for x in inp]
    assert {i for i, o in enumerate(oracle) if o[0] != 0} == {66}
    coeffs = to_mont_array(cc.consts)
    keep, fields = [coeffs], []
    for ptr, col, cid in (cc.L, cc.Rm, cc.O):
        terms = np.ascontiguousarray(np.stack([cid, col], axis=1).astype(np.uint32))
        ptr = np.ascontiguousarray(ptr, dtype=np.uint32)
        keep += [ptr, terms]
        fields += [ptr.ctypes.data, terms.ctypes.data]
    r1cs_h = zk_ctx.r1cs_load(lib.R1csDesc(cc.n_wires, cc.n_constraints, len(cc.consts),
                                           coeffs.ctypes.data, *fields))
    yield cc, r1cs_h, inp, oracle, {66}
    zk_ctx.r1cs_free(r1cs_h)


@pytest.mark.parametrize("lanes", [1, 16, 0])
def test_count_hint_over_a_65536_entry_table(zk_ctx, big_table, lanes):
    cc, r1cs_h, inp, oracle, bad = big_table
    kinds, in_ptr, lc_ptr, hcol, hcid, out_ptr, outs = cc.hint_arrays
    arrs = [np.ascontiguousarray(x, dtype=np.uint32) for x in
            (cc.instr, kinds, in_ptr, lc_ptr, np.stack([hcid, hcol], axis=1), out_ptr, outs)]
    sd = lib.R1csSolverDesc(cc.n_public, cc.n_secret, cc.instr.shape[0], len(kinds),
                            *[a.ctypes.data for a in arrs], lanes, lib.HINTS_STD)
    solver = zk_ctx.r1cs_solver_load(r1cs_h, sd)
    try:
        wires = np.zeros((B, cc.n_wires, 4), np.uint64)
        abc = np.zeros((3, B, cc.n_constraints, 4), np.uint64)
        status = zk_ctx.r1cs_solve_batch(solver, inp, B, wires, abc)
    finally:
        zk_ctx.r1cs_solver_free(solver)
    assert set(np.nonzero(status)[0]) == bad and set(status.tolist()) <= {0, -5}
    for i, (rc, w, a, b, c) in enumerate(oracle):
        if i in bad:
            continue
        assert np.array_equal(wires[i], w), (lanes, i)
        assert np.array_equal(abc[0][i], a) and np.array_equal(abc[1][i], b) \
            and np.array_equal(abc[2][i], c), (lanes, i)


# ---------------------------------------------------------------------------------------------
# commitments: the solve stops at the commitment hints
class CommitCase:
    """One circuit with commitments: prover, inputs, and the two references computed once -- the
    oracle's proofs and those of the frontend program's path (Prover.submit)."""

    def __init__(self, ctx, cc, asg, bad, seed, wbits=(7, 5), **plan):
        from oracle import cref
        self.cc, self.bad = cc, set(bad)
        self.pk, self.vk, _ = groth16.setup(cc, seed, groth16.gpu_mul(ctx))
        self.prover = groth16.Prover(ctx, cc, self.pk, *wbits, **plan)
        rng = random.Random(seed)
        self.inp = np.stack([to_mont_array(cc.assignment_vector(a)) for a in asg])
        self.rs = np.stack([to_mont_array([rng.randrange(H.R), rng.randrange(H.R)]) for _ in asg])
        rh, ph, ch = cref.R1csHandle(cc), cref.PkHandle(self.pk), cref.CommitKeysHandle(self.pk)
        self.want = cref.groth16_prove_batch_ex(rh, ph, ch, self.inp, self.rs, 16)[:4]
        # at most 3 lanes leave the value comparison, and they are the planted ones
        assert set(np.nonzero(self.want[3])[0]) == self.bad and len(self.bad) <= 3
        self.prover.submit(self.inp, self.rs)
        self.program = self.prover.collect()
        assert set(np.nonzero(self.program[1])[0]) == self.bad

    def check(self, proofs, status, coms, n=None):
        n = len(self.inp) if n is None else n
        want, wcoms, wpoks, wstatus = (x[:n] for x in self.want)
        assert set(np.nonzero(status)[0]) == set(np.nonzero(wstatus)[0]) == {i for i in self.bad if i < n}
        ok = status == 0
        assert np.array_equal(proofs[ok], want[ok])
        assert np.array_equal(coms[ok][:, :-1], wcoms[ok]) and np.array_equal(coms[ok][:, -1], wpoks[ok])
        pproofs, pstatus, pcoms = (x[:n] for x in self.program)
        assert np.array_equal(status, pstatus)
        assert np.array_equal(proofs[ok], pproofs[ok]) and np.array_equal(coms[ok], pcoms[ok])


def _range_assignments():
    rng = random.Random(1)
    asg = []
    for i in range(B):
        a, b = rng.randrange(1, 90), rng.randrange(1, 90)
        asg.append({"X": a * b, "Y": a | b << 8 | rng.getrandbits(48) << 16})
    asg[5]["Y"] += 1 << 64          # a ninth byte: recomposition fails
    asg[64] = {"X": 8190, "Y": 0x2ac3}     # X + 3 >= 2^13
    asg[69]["X"] += 1
    return asg, [5, 64, 69]


@pytest.fixture(scope="module")
def commit_cases(zk_ctx):
    made = {}

    def get(name):
        if name not in made:
            if name == "range":
                asg, bad = _range_assignments()
                made[name] = CommitCase(zk_ctx, compile_circuit(RangeCircuit()), asg, bad, 32)
            else:
                asg = [{"X": y * y % H.R, "Y": y} for y in range(3, 3 + B)]
                asg[10]["X"] += 1
                made[name] = CommitCase(zk_ctx, compile_circuit(TwoCommitments()), asg, [10], 41)
        return made[name]
    yield get
    for c in made.values():
        c.prover.close()


@pytest.mark.parametrize("lanes", [1, 16, 64, 0])
@pytest.mark.parametrize("name", ["range", "two"])
def test_commitment_circuits_pipelined_vs_oracle_and_program(zk_ctx, commit_cases, name, lanes):
    case = commit_cases(name)
    prover = case.prover
    info = zk_ctx.r1cs_solver_info(prover.load_r1cs_solver(lanes, hints="std"))
    assert info["n_instr"] == case.cc.instr.shape[0]
    batches = [(case.inp, case.rs), (np.ascontiguousarray(case.inp[:65]), np.ascontiguousarray(case.rs[:65]))]
    for inp, rs in batches:                      # both submitted before the first collect
        prover.submit_r1cs(inp, rs)
    got = [prover.collect() for _ in batches]
    for (inp, rs), (proofs, status, coms) in zip(batches, got):
        case.check(proofs, status, coms, inp.shape[0])


def test_config5_address_with_commitment_through_the_std_solver(zk_ctx):
    """The address circuit with its 64 input bytes range-checked as gnark's uints.New does it (lookup +
    commitment, 144 committed wires), 2^18 domain: the assignments of
    tests/test_gpu_commitment.py::test_config5_address_with_commitment_range_checks."""
    from gnark_crypto_primitives_amd.std.emulated import limbs_of as emulated_limbs
    from oracle import cref, pyref
    cc = H.compiled("address-commit")
    assert cc.domain_log2() == 18 and len(cc.commitments) == 1
    assert len(cc.commitments[0]["private"]) == 144
    rng = random.Random(56)
    asg = []
    for priv in (1, 2, rng.randrange(1, pyref.SECP_N), rng.randrange(1, pyref.SECP_N),
                 rng.randrange(1, pyref.SECP_N)):
        pub = pyref.secp256k1_mul(priv)
        asg.append({"Address": pyref.eth_address(pub), "X": emulated_limbs(pub[0]),
                    "Y": emulated_limbs(pub[1])})
    asg[3] = dict(asg[3], Address=asg[2]["Address"])          # wrong address
    x = list(asg[4]["X"])
    x[1] += 1 << 64                                            # a limb byte out of range
    asg[4] = dict(asg[4], X=x)
    bad = {3, 4}
    pk, vk, _ = groth16.setup(cc, 57, groth16.gpu_mul(zk_ctx))
    prover = groth16.Prover(zk_ctx, cc, pk, 0, 0, max_batch=64)
    try:
        rng = random.Random(57)
        inp = np.stack([to_mont_array(cc.assignment_vector(a)) for a in asg])
        rs = np.stack([to_mont_array([rng.randrange(H.R), rng.randrange(H.R)]) for _ in asg])
        rh, ph, ch = cref.R1csHandle(cc), cref.PkHandle(pk), cref.CommitKeysHandle(pk)
        want, wcoms, wpoks, wstatus, _ = cref.groth16_prove_batch_ex(rh, ph, ch, inp, rs, 16)
        assert set(np.nonzero(wstatus)[0]) == bad
        prover.load_r1cs_solver(0, hints="std")
        prover.submit_r1cs(inp, rs)
        proofs, status, coms = prover.collect()
        assert set(np.nonzero(status)[0]) == bad
        ok = status == 0
        assert np.array_equal(proofs[ok], want[ok])
        assert np.array_equal(coms[ok][:, :-1], wcoms[ok]) and np.array_equal(coms[ok][:, -1], wpoks[ok])
        for i in np.nonzero(ok)[0]:
            pub = [asg[i]["Address"]]
            assert verify.verify(vk, pub, proofs[i], coms[i, :-1], coms[i, -1])
            assert not verify.verify(vk, [pub[0] + 1], proofs[i], coms[i, :-1], coms[i, -1])
    finally:
        prover.close()


def test_refusals_through_the_abi_leave_the_context_usable(zk_ctx, commit_cases, plain):
    rcase, tcase = commit_cases("range"), commit_cases("two")
    solver = rcase.prover.load_r1cs_solver(0, hints="std")
    rcase.prover.submit_r1cs(rcase.inp, rcase.rs)
    first = rcase.prover.collect()
    rcase.check(*first)
    # a solve alone cannot supply a commitment
    with pytest.raises(lib.ZkmiError, match="needs? a proving key.*zkmi_prove_r1cs_submit"):
        rcase.prover.solve_r1cs(rcase.inp)
    # the solver of one circuit with the key of another: refused with nothing queued
    with pytest.raises(lib.ZkmiError, match="the solver holds 1 commitment hints, the proving key 2"):
        zk_ctx.prove_r1cs_submit(tcase.prover.pk_h, solver, rcase.inp, B, rcase.rs)
    # a solver with commitment hints and a key without commitments
    with pytest.raises(lib.ZkmiError, match="the solver holds 1 commitment hints, the proving key 0"):
        zk_ctx.prove_r1cs_submit(plain.prover.pk_h, solver, rcase.inp, B, rcase.rs)
    # a key with commitments and a solver without commitment hints: the message of the basic entry
    with pytest.raises(lib.ZkmiError, match="this key has commitments"):
        zk_ctx.prove_r1cs_submit(rcase.prover.pk_h, plain.prover.load_r1cs_solver(0, hints="std"),
                                 rcase.inp, B, rcase.rs)
    with pytest.raises(lib.ZkmiError, match="nothing submitted"):
        zk_ctx.prove_collect(np.zeros((B, 32), np.uint64), np.zeros(B, np.int32),
                             np.zeros((B, 2, 8), np.uint64))
    # a good batch on the same context afterwards equals the earlier result
    rcase.prover.submit_r1cs(rcase.inp, rcase.rs)
    again = rcase.prover.collect()
    assert all(np.array_equal(x, y) for x, y in zip(again, first))
