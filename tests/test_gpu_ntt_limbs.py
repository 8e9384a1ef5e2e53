"""The limb form between the passes of the 29-bit transform chains (csrc/ntt.hip: nine int32 limbs as
the butterflies leave them, limb 8 in a plane beside the buffer, norm at the load) through every
entry that runs on those kernels: ntt_batch for every log n mod 4 (every ntt_mid29), h_batch and
ab_coset_batch against Python integers, and proofs of a folded and an unfolded key, whose planes
come from the set's c buffer and from the context."""
import random

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu
R = H.R


@pytest.fixture(scope="module")
def cref():
    from oracle import cref
    return cref


_ROWS = {}


def _rows(log_n):
    """65 proofs as integers, read-only: row 0 random, row 1 all zero, row 2 all r - 1, 62 random"""
    if log_n not in _ROWS:
        n = 1 << log_n
        r = H.rng(8200 + log_n)
        rows = [H.rand_fr(r, n)[0], [0] * n, [R - 1] * n] + [H.rand_fr(r, n)[0] for _ in range(62)]
        data = np.stack([H.to_mont_array(row) for row in rows])
        data.setflags(write=False)
        _ROWS[log_n] = (rows, data)
    return _ROWS[log_n]


@pytest.mark.parametrize("log_n", [8, 9, 10, 11, 12])
@pytest.mark.parametrize("inverse,coset", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_ntt_batches(zk_ctx, cref, log_n, inverse, coset):
    """ntt_batch == the C oracle's transform for batches of 1 (random, zero, r - 1), 64 and 65"""
    _, data = _rows(log_n)
    want = np.stack([cref.ntt(row, log_n, inverse, coset) for row in data])
    for lo, hi in ((0, 1), (1, 2), (2, 3), (1, 65), (0, 65)):
        got = data[lo:hi].copy()
        zk_ctx.ntt_batch(got, log_n, hi - lo, inverse, coset)
        assert np.array_equal(got, want[lo:hi]), (lo, hi)


def _ntt_int(v, w):
    """natural-order evaluations of the polynomial with coefficients v at the powers of w"""
    n = len(v)
    if n == 1:
        return v
    w2 = w * w % R
    e, o = _ntt_int(v[0::2], w2), _ntt_int(v[1::2], w2)
    out, x, h = [0] * n, 1, n // 2
    for i in range(h):
        t = x * o[i] % R
        out[i], out[i + h] = (e[i] + t) % R, (e[i] - t) % R
        x = x * w % R
    return out


def _to_coset_int(evals, log_n):
    """evaluations on the domain -> evaluations on the coset 5 * domain"""
    n = 1 << log_n
    w = pow(5, (R - 1) >> log_n, R)
    n_inv = pow(n, R - 2, R)
    coef = [x * n_inv % R for x in _ntt_int(evals, pow(w, R - 2, R))]
    return _ntt_int([c * pow(5, i, R) % R for i, c in enumerate(coef)], w)


@pytest.fixture(scope="module", params=[8, 9])
def coset_case(request):
    """(log n, data, coset evaluations of every row as integers)"""
    log_n = request.param
    rows, data = _rows(log_n)
    return log_n, data, [_to_coset_int(row, log_n) for row in rows]


def test_ab_coset_batch_against_integers(zk_ctx, coset_case):
    """batch 65; b is a rotated by one proof, so zero and r - 1 meet random rows in the product.
    The result is in gnark's image, as include/zkmi.h documents it."""
    log_n, a, ac = coset_case
    b = np.roll(a, 1, axis=0)
    want = np.stack([H.to_mont_array([x * y % R for x, y in zip(ac[i], ac[i - 1])])
                     for i in range(len(a))])
    out = np.zeros_like(a)
    zk_ctx.ab_coset_batch(a.copy(), b.copy(), out, log_n, len(a))
    assert np.array_equal(out, want)


def test_h_batch_against_integers(zk_ctx, coset_case):
    """batch 65; h = cosetiNTT((a_c b_c - c_c) / (g^n - 1)) with b and c rotations of a"""
    log_n, a, ac = coset_case
    n = 1 << log_n
    b, c = np.roll(a, 1, axis=0), np.roll(a, 5, axis=0)
    w_inv = pow(pow(5, (R - 1) >> log_n, R), R - 2, R)
    den = pow(pow(5, n, R) - 1, R - 2, R) * pow(n, R - 2, R) % R
    g_inv = pow(5, R - 2, R)
    want = []
    for i in range(len(a)):
        q = [(x * y - z) * den % R for x, y, z in zip(ac[i], ac[i - 1], ac[i - 5])]
        want.append(H.to_mont_array([x * pow(g_inv, k, R) % R
                                     for k, x in enumerate(_ntt_int(q, w_inv))]))
    out = np.zeros_like(a)
    zk_ctx.h_batch(a.copy(), b.copy(), c.copy(), out, log_n, len(a))
    assert np.array_equal(out, np.stack(want))


@pytest.fixture(scope="module")
def poseidon_case(zk_ctx, cref):
    """single Poseidon (214 constraints of 2^8), batch 65, lane 5 unsatisfied, and the oracle's
    proofs and status"""
    from gnark_crypto_primitives_amd import circuits, groth16
    from gnark_crypto_primitives_amd.frontend import compile_circuit
    from oracle import pyref
    cc = compile_circuit(circuits.PoseidonCircuit())
    pk, _, _ = groth16.setup(cc, 83, groth16.gpu_mul(zk_ctx))
    assert pk.log_n == 8
    rng = random.Random(83)
    datas = [0, 1, R - 1] + [rng.randrange(R) for _ in range(62)]
    inp = np.stack([H.to_mont_array(cc.assignment_vector(
        {"Data": d, "Hash": pyref.poseidon_hash([d])})) for d in datas])
    inp[5] = H.to_mont_array(cc.assignment_vector({"Data": 5, "Hash": 7}))
    rs = np.stack([H.to_mont_array([rng.randrange(R), rng.randrange(R)]) for _ in range(65)])
    want, wstatus, _ = cref.groth16_prove_batch(cref.R1csHandle(cc), cref.PkHandle(pk), inp, rs)
    assert list(wstatus != 0) == [i == 5 for i in range(65)]
    return cc, pk, inp, rs, want, wstatus


@pytest.mark.parametrize("fold", [True, False])
def test_poseidon_proofs(zk_ctx, poseidon_case, fold):
    """folded: the planes are the set's c buffer; unfolded: the context's, and c is transformed"""
    from gnark_crypto_primitives_amd import groth16
    cc, pk, inp, rs, want, wstatus = poseidon_case
    prover = groth16.Prover(zk_ctx, cc, pk, window_bits_g1=8, window_bits_g2=6, fold_quotient=fold)
    assert prover.folded == fold
    proofs, status = prover.prove(inp, rs)
    prover.close()
    assert np.array_equal(status != 0, wstatus != 0)
    ok = status == 0
    assert np.array_equal(proofs[ok], want[ok])
