"""Comb MSMs whose groups share their scalars across the batch (csrc/msm.hip, comb_common_sums).

A comb group whose k scalars are the same in every real lane of a batch is summed once per window
and added to every lane by the last chunk reduction; only the varying groups go through the
per-lane accumulate kernel.  These tests build batches in which chosen groups are uniform, differ
in one lane only, are all zero, or gather identity table entries, and compare every real lane with
the C oracle; at prover level, batches with uniform wires run pipelined behind batches without.
"""
import random

import numpy as np
import pytest

from gnark_crypto_primitives_amd import groth16
from gnark_crypto_primitives_amd.frontend.compile import to_mont_array
from gnark_crypto_primitives_amd.tree import smt_witness
from tests import helpers as H
from tests.test_gpu_fullsize import _rand_fr_array

pytestmark = pytest.mark.gpu

K = 6
N = 238          # 40 groups of 6, the last one ragged (4 bases)
CANCEL = 2       # group whose top base is minus the sum of the others


def _neg_point(group, pt):
    ncoord = 4 if group == 1 else 8
    out = pt.copy()
    y = pt.reshape(-1, 4)[ncoord // 4:]
    for j in range(y.shape[0]):
        v = int.from_bytes(y[j].tobytes(), "little")
        out.reshape(-1, 4)[ncoord // 4 + j] = H.ints_to_array([(H.P - v) % H.P])[0]
    return out


_BASES = {}


def _bases(zk_ctx, group):
    """N random multiples of the generator; in group CANCEL, P_5 = -(P_0 + ... + P_4), so the
    table entry of the all-ones subset (unsigned) / all-plus pattern (signed) is the identity"""
    if group not in _BASES:
        from oracle import cref
        rng = np.random.default_rng(70 + group)
        gen = H.g1_gen_mont() if group == 1 else H.g2_gen_mont()
        ks = _rand_fr_array(rng, (N,))
        bases = np.zeros((N, 8 if group == 1 else 16), dtype=np.uint64)
        zk_ctx.fixed_base_mul(group, gen, ks, N, bases)
        g0 = CANCEL * K
        acc = bases[g0].copy()
        for i in range(1, K - 1):
            acc = cref.point_add(group, acc, bases[g0 + i])
        bases[g0 + K - 1] = _neg_point(group, acc)
        _BASES[group] = bases
    return _BASES[group]


def _grp(g):
    return slice(g * K, min((g + 1) * K, N))


def _scalars(rng, batch, scenario):
    sc = np.broadcast_to(_rand_fr_array(rng, (N,)), (batch, N, 4)).copy()
    # group CANCEL: the same integer for all of its bases, so every window gathers the identity
    # entry or nothing (unsigned) / the identity entry (signed)
    sc[:, _grp(CANCEL)] = H.to_mont_array([random.Random(batch).randrange(1, H.R)])[0]
    if scenario == "none_uniform":
        sc = _rand_fr_array(rng, (batch, N))
        sc[:, _grp(CANCEL)] = H.to_mont_array([5])[0]   # ... and one lane differs in it
        sc[batch - 1, CANCEL * K] = H.to_mont_array([6])[0]
    elif scenario == "chosen":
        for g in (1, 4, 5, 39):                          # per-lane random (39: the ragged group)
            w = len(range(N)[_grp(g)])
            sc[:, _grp(g)] = _rand_fr_array(rng, (batch, w))
        sc[:, _grp(3)] = 0                               # uniform all-zero group
        # groups that differ in one lane only: the last real lane, lane 0 (the reference lane),
        # and a lane at a wavefront edge
        sc[batch - 1, 7 * K + 2] = _rand_fr_array(rng, (1,))[0]
        sc[0, 9 * K] = _rand_fr_array(rng, (1,))[0]
        sc[min(63, batch - 1), 11 * K + 5] = 0
    else:
        assert scenario == "all_uniform"
    return sc


@pytest.mark.parametrize("scenario", ["chosen", "all_uniform", "none_uniform"])
@pytest.mark.parametrize("batch", [2, 64, 65, 130])
@pytest.mark.parametrize("wb", [200 + K, 300 + K])
@pytest.mark.parametrize("group", [1, 2])
def test_msm_comb_uniform_groups_vs_oracle(zk_ctx, group, wb, batch, scenario):
    from oracle import cref
    bases = _bases(zk_ctx, group)
    rng = np.random.default_rng(1000 * group + 10 * batch + wb)
    sc = _scalars(rng, batch, scenario)
    h = zk_ctx.msm_bases_load(group, bases, N, wb)
    res = np.zeros((batch, bases.shape[1]), dtype=np.uint64)
    try:
        zk_ctx.msm_batch(h, sc, batch, res)
    finally:
        zk_ctx.msm_bases_free(h)
    want = {}
    for p in range(batch):
        key = sc[p].tobytes()
        if key not in want:
            want[key] = cref.msm(group, bases, sc[p])
        assert np.array_equal(res[p], want[key]), (scenario, p)


def _witness(cc, rng, populated):
    return to_mont_array(cc.assignment_vector(smt_witness.synthetic_inclusion(rng, 160, populated)))


def test_arbo160_uniform_batches_pipelined_vs_oracle(zk_ctx):
    """Auto plan on the Arbo-160 key, 96-proof batches (one padded wavefront) streamed two deep:
    nothing uniform (populated 159), then 10 distinct populated-10 witnesses with one populated-40
    lane, again nothing uniform, then one witness repeated in every lane (even the quotient's Z MSM
    is uniform).  A sample of every batch against the C oracle's prover."""
    from oracle import cref
    B = 96
    cc = H.compiled("arbo160")
    pk, _, _ = groth16.setup(cc, 2, groth16.gpu_mul(zk_ctx))
    prover = groth16.Prover(zk_ctx, cc, pk, 0, 0)
    info = zk_ctx.pk_info(prover.pk_h)
    assert info["g1_comb_k"] > 0 and info["g2_comb_k"] > 0, info
    rng = random.Random(4040)

    def rs():
        return np.stack([to_mont_array([rng.randrange(H.R), rng.randrange(H.R)]) for _ in range(B)])

    def varied():
        return np.stack([_witness(cc, rng, 159) for _ in range(B)])

    ws10 = [_witness(cc, rng, 10) for _ in range(10)]
    mixed = np.stack([ws10[rng.randrange(10)] for _ in range(B)])
    odd = 77
    mixed[odd] = _witness(cc, rng, 40)
    same = np.stack([_witness(cc, rng, 10)] * B)
    batches = [(varied(), rs()), (mixed, rs()), (varied(), rs()), (same, rs())]
    rh, ph = cref.R1csHandle(cc), cref.PkHandle(pk)
    try:
        got = list(prover.prove_stream(batches))
        for k, ((inp, r), (proofs, status)) in enumerate(zip(batches, got)):
            assert not status.any(), k
            sample = sorted({0, 1, 63, 64, odd - 1, odd, odd + 1, B - 1})
            want, wstatus, _ = cref.groth16_prove_batch(rh, ph, inp[sample], r[sample], 16)
            assert not wstatus.any()
            assert np.array_equal(proofs[sample], want), k
        # one witness in every lane: the proofs still differ through (r, s)
        assert len({got[3][0][p].tobytes() for p in range(B)}) == B
    finally:
        prover.close()
