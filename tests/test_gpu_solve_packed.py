"""solve_vliw_kernel packed W wavefronts to a workgroup (zkmi_set_solve_waves_per_block): wires,
a / b / c and status equal the C oracle's constraint-by-constraint solver and are byte-identical
across W = 1, 2, 4, 8 -- with fewer waves than W (Bp S / 64 = 1, 2 against W = 8), wave counts W does
not divide (3 against W = 2, 4, 8), an unsatisfied witness in the second wave, the OP_EMUL instance,
and a pipelined run at the default W (batches of 1, 64 and 65 proofs, two in flight)."""
import random

import numpy as np
import pytest

from gnark_crypto_primitives_amd import circuits, groth16
from gnark_crypto_primitives_amd.frontend import compile_circuit
from gnark_crypto_primitives_amd.frontend.compile import to_mont_array
from tests import helpers as H

pytestmark = pytest.mark.gpu

WAVES = (1, 2, 4, 8)


@pytest.fixture
def waves(zk_ctx):
    """setter of the knob on the shared context; the default is back when the test ends"""
    try:
        yield zk_ctx.set_solve_waves_per_block
    finally:
        zk_ctx.set_solve_waves_per_block(0)


def _mixed_assignments(n):
    from tests.test_frontend import _mixed_expected
    rng = random.Random(77)
    asg = []
    for i in range(n):
        x = rng.randrange(1 << 16)
        y = x if i % 5 == 0 else rng.randrange(H.R)
        asg.append({"X": x, "Y": y, "Z": _mixed_expected(x, y)})
    return asg


def _poseidon_assignments(n):
    from gnark_crypto_primitives_amd.hash import poseidon_native
    rng = random.Random(78)
    datas = [rng.randrange(H.R) for _ in range(n)]
    return [{"Data": d, "Hash": poseidon_native.hash([d])} for d in datas]


def _circuit(name):
    if name == "mixed":
        from tests.test_frontend import Mixed
        return Mixed(), _mixed_assignments
    return circuits.PoseidonCircuit(), _poseidon_assignments


def _spoil(name, a):
    key = "Z" if name == "mixed" else "Hash"
    return dict(a, **{key: (a[key] + 1) % H.R})


@pytest.mark.parametrize("lanes", [1, 8, 64])
@pytest.mark.parametrize("name", ["mixed", "poseidon"])
def test_packed_solve_matches_oracle_and_one_wave_blocks(zk_ctx, waves, name, lanes):
    from oracle import cref
    circuit, make = _circuit(name)
    cc = compile_circuit(circuit, lanes)
    assert cc.lanes_per_proof == lanes
    # batches 1, 64, 65: 1 / 1 / 2 wavefronts at S = 1, 8 / 8 / 16 at S = 8, 64 / 64 / 128 at S = 64;
    # 130 proofs at S = 1 are three wavefronts, which none of 2, 4, 8 divides
    batches = (1, 64, 65) + ((130,) if lanes == 1 else ())
    n = max(batches)
    asg = make(n)
    asg[3] = _spoil(name, asg[3])          # first wave of the launch
    if n > 64:
        asg[64] = _spoil(name, asg[64])    # S = 1: lane 0 of the second wave; S = 64: wave 64
    inp = np.stack([to_mont_array(cc.assignment_vector(a)) for a in asg])
    rh = cref.R1csHandle(cc)
    want = [cref.r1cs_solve(rh, inp[i]) for i in range(n)]
    assert [i for i in range(n) if want[i][0] != 0] == [i for i in (3, 64) if i < n]
    pk, _, _ = groth16.setup(cc, 7, groth16.gpu_mul(zk_ctx))
    prover = groth16.Prover(zk_ctx, cc, pk, 7, 5)
    try:
        for batch in batches:
            got = {}
            for w in WAVES:
                waves(w)
                got[w] = prover.solve(np.ascontiguousarray(inp[:batch]), want_wires=True,
                                      want_abc=True)
            status, wires, abc = got[1]
            assert [i for i in range(batch) if status[i] != 0] == [i for i in (3, 64) if i < batch]
            for i in range(batch):
                st, w_, a, b, c = want[i]
                if st != 0:
                    continue
                assert np.array_equal(wires[i], w_), (batch, i)
                assert np.array_equal(abc[0][i], a) and np.array_equal(abc[1][i], b) \
                    and np.array_equal(abc[2][i], c), (batch, i)
            ok = status == 0
            for w in WAVES[1:]:
                s2, w2, abc2 = got[w]
                assert np.array_equal(s2, status), (batch, w)
                assert w2[ok].tobytes() == wires[ok].tobytes(), (batch, w)
                assert abc2[:, ok].tobytes() == abc[:, ok].tobytes(), (batch, w)
    finally:
        prover.close()


@pytest.mark.parametrize("lanes", [1, 8])
def test_packed_solve_with_emulated_products(zk_ctx, waves, lanes):
    """solve_vliw_kernel<S, true> eight waves to a workgroup: proofs, commitments and status of an
    emulated-field circuit against the oracle, one witness unsatisfied in the second wave."""
    from gnark_crypto_primitives_amd.std import emulated as em
    from oracle import cref
    from tests.test_emulated import ArithCircuit
    circ = ArithCircuit(em.BN254Fr)
    cc = compile_circuit(circ, lanes)
    p = em.BN254Fr.modulus
    rng = random.Random(lanes)
    asg = [circ.assignment(rng.randrange(p), rng.randrange(p)) for _ in range(70)]
    asg[1] = circ.assignment(p - 1, 1)
    asg[66] = circ.assignment(rng.randrange(p), 5, z=7)      # wrong product
    pk, _, _ = groth16.setup(cc, 70 + lanes, groth16.gpu_mul(zk_ctx))
    inp = np.stack([to_mont_array(cc.assignment_vector(a)) for a in asg])
    rs = np.stack([to_mont_array([rng.randrange(H.R), rng.randrange(H.R)]) for _ in asg])
    rh, ph, ch = cref.R1csHandle(cc), cref.PkHandle(pk), cref.CommitKeysHandle(pk)
    want, wcoms, wpoks, wstatus, _ = cref.groth16_prove_batch_ex(rh, ph, ch, inp, rs, 16)
    assert list(np.nonzero(wstatus)[0]) == [66]
    prover = groth16.Prover(zk_ctx, cc, pk, 7, 5)
    try:
        waves(8)
        prover.submit(inp, rs)
        proofs, status, coms = prover.collect()
        assert list(np.nonzero(status)[0]) == [66]
        ok = status == 0
        assert np.array_equal(proofs[ok], want[ok])
        assert np.array_equal(coms[ok][:, :-1], wcoms[ok])
        assert np.array_equal(coms[ok][:, -1], wpoks[ok])
    finally:
        prover.close()


def test_pipelined_batches_at_the_default(zk_ctx):
    """Three batches (1, 64, 65 proofs) two deep on the Poseidon key, default W: the solve of a
    batch runs beside the other's MSMs and assembly.  Proofs and status against the oracle."""
    from oracle import cref
    cc = compile_circuit(circuits.PoseidonCircuit())
    pk, _, _ = groth16.setup(cc, 1, groth16.gpu_mul(zk_ctx))
    rng = random.Random(5)
    batches = []
    for bsz in (1, 64, 65):
        asg = _poseidon_assignments(bsz)
        inp = np.stack([to_mont_array(cc.assignment_vector(a)) for a in asg])
        rs = np.stack([to_mont_array([rng.randrange(H.R), rng.randrange(H.R)])
                       for _ in range(bsz)])
        batches.append((inp, rs))
    batches[2][0][64, 0, 0] ^= 1
    rh, ph = cref.R1csHandle(cc), cref.PkHandle(pk)
    zk_ctx.set_solve_waves_per_block(0)
    prover = groth16.Prover(zk_ctx, cc, pk, 7, 5)
    try:
        got = list(prover.prove_stream(batches))
    finally:
        prover.close()
    for k, ((inp, rs), (proofs, status)) in enumerate(zip(batches, got)):
        want, wstatus, _ = cref.groth16_prove_batch(rh, ph, inp, rs)
        assert np.array_equal(status != 0, wstatus != 0), k
        assert list(np.nonzero(status)[0]) == ([64] if k == 2 else []), k
        ok = status == 0
        assert np.array_equal(proofs[ok], want[ok]), k


def test_unsupported_block_sizes_are_refused(zk_ctx):
    from gnark_crypto_primitives_amd import lib
    for w in (3, 16):
        with pytest.raises(lib.ZkmiError):
            zk_ctx.set_solve_waves_per_block(w)
    zk_ctx.set_solve_waves_per_block(0)
