"""A comb group size per MSM of a proving key (csrc/comb_plan.h, zkmi_pk_load_planned).

Base sets at explicit comb widths around each other (k = 5, 6, 7, sign patterns and subset sums)
against big-integer sums of oracle/pyref.py: every base is a known multiple of the generator, so the
MSM of a lane is one multiplication of the generator by sum_i s_i k_i.  Then one small key whose
five MSMs are forced to five different tables: proofs byte for byte the C oracle's, also with the
table kinds mixed (the Horner step of the four G1 MSMs is then not fused), with B1 and B2 at the
same width, and with batches in which no wire or every wire varies.
"""
import random

import numpy as np
import pytest

from gnark_crypto_primitives_amd import circuits, groth16
from gnark_crypto_primitives_amd.frontend import compile_circuit
from gnark_crypto_primitives_amd.frontend.compile import to_mont_array
from tests import helpers as H

pytestmark = pytest.mark.gpu

R, P = H.R, H.P
N = 70                      # 14 / 12 (ragged) / 10 groups at k = 5 / 6 / 7
INF = (4, 17, 41, 65, 66, 67, 68, 69)   # bases at infinity: single ones, and the tail of every plan
BATCHES = (1, 64, 65)


def _image(ints, image):
    return H.ints_to_array([x * (1 << (261 if image else 256)) % R for x in ints])


def _point_array(group, pt):
    """pyref affine point (None = infinity) -> gnark's Montgomery words"""
    if pt is None:
        return np.zeros(8 if group == 1 else 16, dtype=np.uint64)
    if group == 1:
        return H.fq_mont([pt[0], pt[1]]).reshape(-1)
    return H.fq_mont([pt[0][0], pt[0][1], pt[1][0], pt[1][1]]).reshape(-1)


_MEMO = {}


def _bases(cref, group):
    """(multiples k_i, points k_i * G); k_i = 0 and a zero point for the bases at infinity"""
    if ("bases", group) not in _MEMO:
        rng = random.Random(1300 + group)
        ks = [0 if i in INF else rng.randrange(1, R) for i in range(N)]
        gen = H.g1_gen_mont() if group == 1 else H.g2_gen_mont()
        pts = cref.batch_mul(group, gen, H.to_mont_array([k if k else 1 for k in ks]))
        for i in INF:
            pts[i] = 0
        _MEMO[("bases", group)] = (ks, pts)
    return _MEMO[("bases", group)]


def _scalars(batch):
    """(plain scalars [batch][N + 2], row_idx [N], a permutation with two rows left out): the
    scalars of the bases with i % 10 < 4 and of bases 20 .. 34 are the same in every lane (edge
    values among them), the others random per lane.  So at k = 5, 6 and 7 alike some groups are
    uniform as a whole (inside 20 .. 34), most hold uniform and varying rows, some only varying."""
    if ("scalars", batch) not in _MEMO:
        rng = random.Random(1400 + batch)
        n_rows = N + 2
        row_idx = list(range(n_rows))
        rng.shuffle(row_idx)
        row_idx = row_idx[:N]
        edge = [0, 1, R - 1, 2, 1 << 253, (1 << 253) - 1, R - 2, (1 << 128) | 1]
        sc = [[rng.randrange(R) for _ in range(n_rows)] for _ in range(batch)]
        for i in range(N):
            if i % 10 < 4 or 20 <= i < 35:
                v = edge[i % len(edge)] if i % 3 == 0 else rng.randrange(R)
                for p in range(batch):
                    sc[p][row_idx[i]] = v
        _MEMO[("scalars", batch)] = (sc, np.array(row_idx, dtype=np.uint32))
    return _MEMO[("scalars", batch)]


def _want(cref, group, batch):
    """big-integer reference, computed once per (group, batch) and shared by every width"""
    if ("want", group, batch) not in _MEMO:
        from oracle import pyref
        ks, _ = _bases(cref, group)
        sc, row_idx = _scalars(batch)
        gen, mul = (H.G1_GEN, pyref.g1_mul) if group == 1 else (H.G2_GEN, pyref.g2_mul)
        out, memo = [], {}
        for p in range(batch):
            e = sum(sc[p][row_idx[i]] * ks[i] for i in range(N)) % R
            if e not in memo:
                memo[e] = _point_array(group, mul(gen, e) if e else None)
            out.append(memo[e])
        _MEMO[("want", group, batch)] = np.stack(out)
    return _MEMO[("want", group, batch)]


@pytest.fixture(scope="module")
def cref():
    from oracle import cref
    return cref


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("group", [1, 2])
def test_comb_widths_5_6_7_vs_bigint(zk_ctx, cref, group, batch):
    _, pts = _bases(cref, group)
    sc, row_idx = _scalars(batch)
    want = _want(cref, group, batch)
    scal = np.stack([_image(row, 1) for row in sc])
    for wb in (305, 306, 307, 205, 206, 207):
        h = zk_ctx.msm_bases_load_image(group, pts, N, wb, 1)
        try:
            for uniform in (0, 1):
                out = np.zeros_like(want)
                zk_ctx.msm_batch_rows(h, scal, N + 2, row_idx, batch, 1, uniform, out)
                assert np.array_equal(out, want), (wb, uniform)
        finally:
            zk_ctx.msm_bases_free(h)


_KEY = {}


def _poseidon_key(zk_ctx):
    if not _KEY:
        cc = compile_circuit(circuits.PoseidonCircuit())
        pk, _, _ = groth16.setup(cc, 131, groth16.gpu_mul(zk_ctx))
        _KEY["k"] = (cc, pk)
    return _KEY["k"]


def _inputs(cc, datas):
    from oracle import pyref
    return np.stack([to_mont_array(cc.assignment_vector(
        {"Data": d, "Hash": pyref.poseidon_hash([d])})) for d in datas])


def _prove_and_compare(zk_ctx, cref, wbs, inp, rs, fold, bad=()):
    cc, pk = _poseidon_key(zk_ctx)
    want, wstatus, _ = cref.groth16_prove_batch(cref.R1csHandle(cc), cref.PkHandle(pk), inp, rs)
    prover = groth16.Prover(zk_ctx, cc, pk, fold_quotient=fold, msm_window_bits=wbs)
    try:
        info = zk_ctx.pk_info(prover.pk_h)
        assert prover.folded == fold
        assert list(info["msm_comb_k"].values()) == [w % 100 for w in wbs], info
        assert list(info["msm_comb_signed"].values()) == [int(w >= 300) for w in wbs], info
        assert info["g1_comb_k"] == wbs[3] % 100 and info["g2_comb_k"] == wbs[4] % 100
        prover.submit(inp, rs)
        proofs, status = prover.collect()
    finally:
        prover.close()
    assert list(status != 0) == list(wstatus != 0) == [i in bad for i in range(len(inp))]
    ok = status == 0
    assert np.array_equal(proofs[ok], want[ok])


# A, B1, K, Z, B2: five widths; kinds mixed (no fused Horner step, scalar conversion passes);
# B1 and B2 alike (the same digits for both)
PLANS = {"five_widths": (305, 306, 307, 308, 304), "mixed_kinds": (205, 306, 207, 308, 204),
         "b_alike": (305, 306, 304, 307, 306), "b_alike_unsigned": (305, 206, 304, 307, 206)}


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("plan", sorted(PLANS))
def test_poseidon_proofs_on_a_plan_per_msm(zk_ctx, cref, plan, fold):
    """70 lanes (one padded wavefront and a second one), lane 5 unsatisfied"""
    cc, _ = _poseidon_key(zk_ctx)
    rng = random.Random(132)
    B = 70
    inp = _inputs(cc, [0, 1, R - 1] + [rng.randrange(R) for _ in range(B - 3)])
    inp[5] = to_mont_array(cc.assignment_vector({"Data": 5, "Hash": 7}))
    rs = np.stack([to_mont_array([rng.randrange(R), rng.randrange(R)]) for _ in range(B)])
    _prove_and_compare(zk_ctx, cref, PLANS[plan], inp, rs, fold, bad=(5,))


@pytest.mark.parametrize("batch", [1, 64, 65])
@pytest.mark.parametrize("varying", [False, True])
def test_equal_b_widths_uniform_and_varying_batches(zk_ctx, cref, varying, batch):
    """one witness in every lane (no group of a wire MSM varies: the lists of varying groups are
    empty) and a witness of its own per lane, B1 and B2 at one width beside three others"""
    cc, _ = _poseidon_key(zk_ctx)
    rng = random.Random(133 + batch)
    datas = [rng.randrange(R) for _ in range(batch)] if varying else [rng.randrange(R)] * batch
    rs = np.stack([to_mont_array([rng.randrange(R), rng.randrange(R)]) for _ in range(batch)])
    _prove_and_compare(zk_ctx, cref, PLANS["b_alike"], _inputs(cc, datas), rs, True)


def test_plan_per_msm_is_checked(zk_ctx):
    from gnark_crypto_primitives_amd.lib import ZkmiError
    cc, pk = _poseidon_key(zk_ctx)
    for wbs in ((305, 306, 307, 0, 304), (305, 306, 307, 322, 304), (8, 306, 307, 308, 304)):
        with pytest.raises(ZkmiError):
            groth16.Prover(zk_ctx, cc, pk, msm_window_bits=wbs)
