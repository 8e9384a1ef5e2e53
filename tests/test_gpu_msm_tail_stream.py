"""The tails of the proving-key MSMs on a stream of their own (zkmi_ctx::stream4): common sums of the
uniform groups and the sums over the chunk partials run beside the next MSM's kernels, out of
buffers that alternate between consecutive MSMs and consecutive batches (msm_part_layout.h).

What could go wrong is a tail that reads what a later MSM or a later batch has already overwritten
(lane 0's digits, the list of uniform groups, the counts), or a Horner step that starts before its
window sums are complete.  So: six consecutive batches, two in flight, on the small Poseidon key
with a forced comb plan per MSM; every batch has other witnesses, another split into uniform and
varying groups and another size than its neighbours, and every proof is the C oracle's byte for
byte.  The same through the blocking entry point, and on a second prover of the same context.
"""
import random

import numpy as np
import pytest

from gnark_crypto_primitives_amd import circuits, groth16
from gnark_crypto_primitives_amd.frontend import compile_circuit
from gnark_crypto_primitives_amd.frontend.compile import to_mont_array
from tests import helpers as H

pytestmark = pytest.mark.gpu

R = H.R
# A, B1, K, Z, B2 (tests/test_gpu_msm_mixed_plan.py): five widths; table kinds mixed
PLANS = {"five_widths": (305, 306, 307, 308, 304), "mixed_kinds": (205, 306, 207, 308, 204)}
SIZES = (65, 1, 65, 65, 1, 65)     # padding lanes and chunk counts change between neighbours
# 1: one witness in every lane (no group of a wire MSM varies: everything through the common sums)
# 2: a witness of its own per lane (no group is uniform); 3: half and half
PATTERNS = (1, 2, 3, 2, 3, 1)
BAD = (2, 5)                       # batch 2, lane 5: unsatisfied

_MEMO = {}


def _key(zk_ctx):
    if "key" not in _MEMO:
        cc = compile_circuit(circuits.PoseidonCircuit())
        pk, _, _ = groth16.setup(cc, 131, groth16.gpu_mul(zk_ctx))
        assert cc.n_constraints == 214
        _MEMO["key"] = (cc, pk)
    return _MEMO["key"]


def _batches(zk_ctx):
    """[(inputs, rs, want proofs, want status)] of the six batches: the reference is computed once
    and shared by every case"""
    if "batches" not in _MEMO:
        from oracle import cref, pyref
        cc, pk = _key(zk_ctx)
        r1cs, pkh = cref.R1csHandle(cc), cref.PkHandle(pk)
        out = []
        for i, (B, pattern) in enumerate(zip(SIZES, PATTERNS)):
            rng = random.Random(1400 + i)
            own = [rng.randrange(R) for _ in range(B)]
            if pattern == 1:
                datas = [own[0]] * B
            elif pattern == 2:
                datas = own
            else:
                datas = [own[0] if p < (B + 1) // 2 else own[p] for p in range(B)]
            inp = np.stack([to_mont_array(cc.assignment_vector(
                {"Data": d, "Hash": pyref.poseidon_hash([d])})) for d in datas])
            if i == BAD[0]:
                inp[BAD[1]] = to_mont_array(cc.assignment_vector({"Data": 5, "Hash": 7}))
            rs = np.stack([to_mont_array([rng.randrange(R), rng.randrange(R)]) for _ in range(B)])
            want, wstatus, _ = cref.groth16_prove_batch(r1cs, pkh, inp, rs)
            assert list(wstatus != 0) == [(i, p) == BAD for p in range(B)]
            out.append((inp, rs, want, wstatus))
        _MEMO["batches"] = out
    return _MEMO["batches"]


def _same(i, proofs, status, want, wstatus):
    assert list(status != 0) == list(wstatus != 0), f"batch {i}: status"
    ok = wstatus == 0
    assert np.array_equal(proofs[ok], want[ok]), f"batch {i}: proofs differ from the C oracle's"


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("plan", sorted(PLANS))
def test_six_batches_two_deep_vs_oracle(zk_ctx, plan, fold):
    cc, pk = _key(zk_ctx)
    batches = _batches(zk_ctx)
    wbs = PLANS[plan]
    prover = groth16.Prover(zk_ctx, cc, pk, fold_quotient=fold, msm_window_bits=wbs)
    try:
        assert prover.folded == fold
        info = zk_ctx.pk_info(prover.pk_h)
        assert list(info["msm_comb_k"].values()) == [w % 100 for w in wbs], info
        # two deep, as bench.py runs: submit(k + 1) before collect(k)
        got = []
        prover.submit(batches[0][0], batches[0][1])
        for i in range(len(batches)):
            if i + 1 < len(batches):
                prover.submit(batches[i + 1][0], batches[i + 1][1])
            got.append(prover.collect())
        for i, ((proofs, status), (_, _, want, wstatus)) in enumerate(zip(got, batches)):
            _same(i, proofs, status, want, wstatus)
        # one batch in flight: the same bytes, unsatisfied lane included
        for i, (inp, rs, want, wstatus) in enumerate(batches):
            proofs, status = prover.prove(inp, rs)
            _same(i, proofs, status, want, wstatus)
            ok = wstatus == 0     # (the record of an unsatisfied lane is unspecified)
            assert np.array_equal(proofs[ok], got[i][0][ok]) and np.array_equal(status, got[i][1])
    finally:
        prover.close()
    # a second prover on the same context starts from the first one's events and buffer turn
    prover = groth16.Prover(zk_ctx, cc, pk, fold_quotient=fold, msm_window_bits=wbs)
    try:
        inp, rs, want, wstatus = batches[0]
        prover.submit(inp, rs)
        proofs, status = prover.collect()
        _same(0, proofs, status, want, wstatus)
    finally:
        prover.close()
