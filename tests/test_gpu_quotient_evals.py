"""The quotient in evaluation form on the GPU (csrc/quotient_fold.hip, compute_ab_coset_bi in
csrc/ntt.hip): the bases E and L that a folded key builds from pk.G1.Z against their closed forms,
the four-transform schedule against the C oracle's transforms, and proofs of folded keys against
the oracle and against the same key loaded unfolded."""
import random

import numpy as np
import pytest

from gnark_crypto_primitives_amd import circuits, groth16
from gnark_crypto_primitives_amd.frontend import Public, Secret, compile_circuit
from gnark_crypto_primitives_amd.frontend.compile import from_mont_array, to_mont_array
from tests import helpers as H

pytestmark = pytest.mark.gpu
R = H.R


@pytest.fixture(scope="module")
def cref():
    from oracle import cref
    return cref


# ---- base transform ------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [8, 9])
def test_quotient_bases_closed_form(zk_ctx, log_n):
    """Z_k = tau^k z G: E_i and L_i are s G with s = den/n sum_k g^-k w^-ik tau^k z and
    1/n sum_k w^-ik tau^k z over k < n - 1.  Points past n - 1 are ignored."""
    n = 1 << log_n
    tau, z = groth16.sample_trapdoor(400 + log_n)[:2]
    mul = groth16.gpu_mul(zk_ctx)
    zs = [pow(tau, k, R) * z % R for k in range(n + 3)]
    pts = mul(1, to_mont_array(zs))
    w_inv = pow(pow(5, (R - 1) >> log_n, R), R - 2, R)
    g_inv, n_inv = pow(5, R - 2, R), pow(n, R - 2, R)
    den = pow(pow(5, n, R) - 1, R - 2, R)
    gz = [zs[k] * pow(g_inv, k, R) % R for k in range(n - 1)]
    e_s, l_s = [], []
    for i in range(n):
        wi, x, se, sl = pow(w_inv, i, R), 1, 0, 0
        for k in range(n - 1):
            se += gz[k] * x
            sl += zs[k] * x
            x = x * wi % R
        e_s.append(se % R * den % R * n_inv % R)
        l_s.append(sl % R * n_inv % R)
    want = mul(1, to_mont_array(e_s + l_s))
    for n_z in (n - 1, n + 3):
        e, l = zk_ctx.quotient_bases(np.ascontiguousarray(pts[:n_z]), log_n)
        assert np.array_equal(e, want[:n]), (log_n, n_z)
        assert np.array_equal(l, want[n:]), (log_n, n_z)


# ---- schedule ------------------------------------------------------------------------------------
_BATCH_CACHE = {}


def _edge_batch(log_n):
    """The 113-proof edge batch of tests/test_gpu_quotient_lazy.py: the constant vectors r-1 and 1,
    +-1 at the 16 rows k n/16 and at rows 1 and n-1, alternating 0 / r-1, w^(k i) for k in
    {0, 1, n/2, n-1}, 70 random proofs.  Montgomery images [113][n][4], read-only."""
    if log_n not in _BATCH_CACHE:
        n = 1 << log_n
        w = pow(5, (R - 1) >> log_n, R)
        rows = [[R - 1] * n, [1] * n]
        for at in [k * n // 16 for k in range(16)] + [1, n - 1]:
            for v in (1, R - 1):
                rows.append([v if i == at else 0 for i in range(n)])
        rows.append([(R - 1) * (i & 1) for i in range(n)])
        for k in (0, 1, n // 2, n - 1):
            wk, x, row = pow(w, k, R), 1, []
            for _ in range(n):
                row.append(x)
                x = x * wk % R
            rows.append(row)
        r = H.rng(7100 + log_n)
        rows += [H.rand_fr(r, n)[0] for _ in range(70)]
        assert len(rows) == 113
        data = np.stack([H.to_mont_array(row) for row in rows])
        data.setflags(write=False)
        _BATCH_CACHE[log_n] = data
    return _BATCH_CACHE[log_n]


@pytest.mark.parametrize("log_n", [8, 9, 10, 11, 12])
def test_ab_coset_schedule(zk_ctx, cref, log_n):
    """ab_coset_batch == the product of the oracle's coset transforms of a and b, bit for bit, for
    log n mod 4 = 0 .. 3, the empty middle forward range (2^8) and a middle LDS pass (2^12); b is a
    rotated against itself, so constant vectors, impulses and random proofs meet in the product."""
    a = _edge_batch(log_n)
    b = np.roll(a, 1, axis=0)
    coset = [cref.ntt(cref.ntt(row, log_n, True, False), log_n, False, True) for row in a]
    ints = [from_mont_array(x) for x in coset]
    want = np.stack([to_mont_array([x * y % R for x, y in zip(ints[i], ints[i - 1])])
                     for i in range(len(a))])
    out = np.zeros_like(a)
    zk_ctx.ab_coset_batch(a.copy(), b.copy(), out, log_n, len(a))
    assert np.array_equal(out, want)


# ---- proofs --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def poseidon_case(zk_ctx, cref):
    """(cc, pk, batches, [(want proofs, want status)]): single Poseidon, 214 constraints of 2^8, two
    batches of 67 and 64, one unsatisfied lane"""
    from oracle import pyref
    cc = compile_circuit(circuits.PoseidonCircuit())
    assert cc.n_constraints == 214
    pk, _, _ = groth16.setup(cc, 61, groth16.gpu_mul(zk_ctx))
    assert pk.log_n == 8
    rng = random.Random(61)
    batches = []
    for bsz in (67, 64):
        datas = [0, 1, R - 1] + [rng.randrange(R) for _ in range(bsz - 3)]
        inp = np.stack([to_mont_array(cc.assignment_vector(
            {"Data": d, "Hash": pyref.poseidon_hash([d])})) for d in datas])
        rs = np.stack([to_mont_array([rng.randrange(R), rng.randrange(R)]) for _ in range(bsz)])
        batches.append((inp, rs))
    batches[0][0][5] = to_mont_array(cc.assignment_vector({"Data": 5, "Hash": 7}))
    rh, ph = cref.R1csHandle(cc), cref.PkHandle(pk)
    want = [cref.groth16_prove_batch(rh, ph, inp, rs)[:2] for inp, rs in batches]
    return cc, pk, batches, want


@pytest.mark.parametrize("gnark_key_layout", [False, True])
def test_folded_poseidon_streams(zk_ctx, poseidon_case, gnark_key_layout):
    cc, pk, batches, want = poseidon_case
    got = {}
    for fold in (True, False):
        prover = groth16.Prover(zk_ctx, cc, pk, window_bits_g1=8, window_bits_g2=6,
                                gnark_key_layout=gnark_key_layout, fold_quotient=fold)
        assert prover.folded == fold
        got[fold] = list(prover.prove_stream(batches))
        prover.close()
    for k, (wproofs, wstatus) in enumerate(want):
        proofs, status = got[True][k]
        assert list(status != 0) == list(wstatus != 0) == [k == 0 and i == 5
                                                            for i in range(len(status))]
        assert np.array_equal(status, got[False][k][1])
        ok = status == 0
        assert np.array_equal(proofs[ok], wproofs[ok])
        assert np.array_equal(proofs[ok], got[False][k][0][ok])


class FoldEdges:
    """O with terms on the ONE wire (the 7) and on the public wires Z and V, which pk.G1.K does not
    hold; a chain of squarings pads the system past 128 constraints (domain 2^8)."""
    X = Secret()
    Y = Secret()
    Z = Public()
    V = Public()

    def define(self, api):
        api.AssertIsEqual(api.Mul(self.X, self.Y), api.Add(self.Z, 7))
        t = self.X
        for _ in range(130):
            t = api.Mul(t, t)
        api.AssertIsEqual(api.Mul(t, self.Y), api.Sub(self.V, self.Z))


@pytest.fixture(scope="module")
def edges_case(zk_ctx, cref):
    cc = compile_circuit(FoldEdges())
    assert cc.n_constraints > 128 and cc.domain_log2() == 8
    # asserted on the matrix itself: the appended K bases are exercised
    o_wires = set(cc.O[1].tolist())
    assert 0 in o_wires and any(1 <= w < cc.n_public for w in o_wires)
    pk, _, _ = groth16.setup(cc, 67, groth16.gpu_mul(zk_ctx))
    assert not set(np.asarray(pk.k_wire).tolist()) & set(range(cc.n_public))
    rng = random.Random(67)
    asg = []
    for _ in range(64):
        x, y = rng.randrange(R), rng.randrange(R)
        z = (x * y - 7) % R
        asg.append({"X": x, "Y": y, "Z": z, "V": (pow(x, 1 << 130, R) * y + z) % R})
    inp = np.stack([to_mont_array(cc.assignment_vector(a)) for a in asg])
    rs = np.stack([to_mont_array([rng.randrange(R), rng.randrange(R)]) for _ in range(64)])
    rh = cref.R1csHandle(cc)
    want, wstatus, _ = cref.groth16_prove_batch(rh, cref.PkHandle(pk), inp, rs)
    assert not wstatus.any()
    prover = groth16.Prover(zk_ctx, cc, pk, window_bits_g1=8, window_bits_g2=6)
    assert prover.folded
    yield cc, prover, inp, rs, want, rh
    prover.close()


def test_folded_key_with_appended_bases(edges_case):
    cc, prover, inp, rs, want, _ = edges_case
    proofs, status = prover.prove(inp, rs)
    assert not status.any()
    assert np.array_equal(proofs, want)


def test_folded_key_from_solved_witnesses(edges_case, cref):
    """the same key through zkmi_prove_witness_submit: with the R1CS resident, and with a, b, c from
    the caller's solver"""
    cc, prover, inp, rs, want, rh = edges_case
    sol = [cref.r1cs_solve(rh, x) for x in inp]
    assert all(s[0] == 0 for s in sol)
    W, A, B, Cc = (np.stack([s[k] for s in sol]) for k in (1, 2, 3, 4))
    prover.submit_witness(W, rs)
    prover.submit_witness(W, rs, A, B, Cc)
    for _ in range(2):
        proofs, status = prover.collect()
        assert not status.any()
        assert np.array_equal(proofs, want)


class OneCommitment:
    X = Public()
    Y = Secret()

    def define(self, api):
        y2 = api.Mul(self.Y, self.Y)
        c1 = api.Commit(self.Y, y2)
        api.AssertIsEqual(api.Mul(c1, 0), 0)
        api.AssertIsEqual(api.Add(y2, 0), self.X)


def test_key_with_commitment_loads_unfolded(zk_ctx, cref):
    cc = compile_circuit(OneCommitment())
    pk, _, _ = groth16.setup(cc, 71, groth16.gpu_mul(zk_ctx))
    assert len(pk.commitment_keys) == 1
    prover = groth16.Prover(zk_ctx, cc, pk, 7, 5, fold_quotient=True)
    assert not prover.folded
    rng = random.Random(71)
    inp = np.stack([to_mont_array(cc.assignment_vector({"X": y * y % R, "Y": y}))
                    for y in range(3, 67)])
    rs = np.stack([to_mont_array([rng.randrange(R), rng.randrange(R)]) for _ in range(64)])
    want, wcoms, wpoks, wstatus, _ = cref.groth16_prove_batch_ex(
        cref.R1csHandle(cc), cref.PkHandle(pk), cref.CommitKeysHandle(pk), inp, rs, 16)
    assert not wstatus.any()
    try:
        proofs, status, coms = prover.prove(inp, rs)
    finally:
        prover.close()
    assert not status.any()
    assert np.array_equal(proofs, want)
    assert np.array_equal(coms[:, :-1], wcoms) and np.array_equal(coms[:, -1], wpoks)
