"""Sign-pattern comb tables native to a scalar image (csrc/msm_impl.h, csrc/comb_sign.h).

A table loaded for image 0 (x * 2^256) or 1 (x * 2^261) reads scalars of that image as they are and
converts the other image in one pass; the groups whose scalars the batch shares are found inside
the MSM, from one pass over all scalar rows before it, or not looked for.  Every combination must
give the C oracle's naive sum: small explicit plans (300 + k), group sizes around k, bases at
infinity, edge scalars, row maps with repeated and permuted rows, batches around the 64-lane
padding.  One prove test through zkmi_prove_submit on sign-pattern plans, folded key and not.
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
K = 5
EDGE = [0, 1, 2, R - 1, R - 2, 1 << 253, (1 << 253) - 1, (1 << 253) | 1, (1 << 32) - 1, 1 << 32,
        (1 << 64) - 1, 1 << 64, (1 << 128) | (1 << 127), (1 << 224) - 1, 1 << 224, 3]


@pytest.fixture(scope="module")
def cref():
    from oracle import cref
    return cref


def _image(ints, image):
    """canonical image of plain integers: x * 2^256 (0) or x * 2^261 (1) mod r, 4 x u64"""
    return H.ints_to_array([x * (1 << (261 if image else 256)) % R for x in ints])


_BASES = {}


def _bases(cref, group, n):
    """n random multiples of the generator; from n = K on, the top base of group 0 is the point at
    infinity; at n = 3K + 2 also a middle base of group 1 and the whole of the ragged group 3"""
    if (group, n) not in _BASES:
        rng = random.Random(500 + 10 * n + group)
        gen = H.g1_gen_mont() if group == 1 else H.g2_gen_mont()
        bases = cref.batch_mul(group, gen, H.to_mont_array([rng.randrange(1, R) for _ in range(n)]))
        if n >= K:
            bases[K - 1] = 0
        if n >= 3 * K + 2:
            bases[K + 2] = 0
            bases[3 * K:] = 0
        _BASES[(group, n)] = bases
    return _BASES[(group, n)]


def _case(n, batch):
    """(plain scalars [batch][n_rows], row_idx [n]): n + 3 rows, read through a map with one row
    repeated and the rest permuted.  By group of K bases: 0 the same in every lane (edge values),
    1 random per lane, 2 the same but for the last lane, 3 edge values per lane; the rows no base
    reads are random, so a pass over all rows sees varying rows that no group owns.  (The padding
    lanes of the device matrix hold zeros, which differ from every uniform row.)"""
    rng = random.Random(7000 + 131 * n + batch)
    n_rows = n + 3
    row_idx = list(range(n_rows))
    rng.shuffle(row_idx)
    row_idx = row_idx[:n]
    if n >= 2:
        row_idx[1] = row_idx[0]
    sc = [[rng.randrange(R) for _ in range(n_rows)] for _ in range(batch)]
    for i in range(n):
        g, row = i // K, row_idx[i]
        if i == 1 and n >= 2:
            continue
        if g % 4 == 0:
            v = EDGE[(i * 3 + n) % len(EDGE)]
            for p in range(batch):
                sc[p][row] = v
        elif g % 4 == 2:
            v = rng.randrange(R)
            for p in range(batch):
                sc[p][row] = v
            if i % K == K - 1:
                sc[batch - 1][row] = EDGE[i % len(EDGE)]
        elif g % 4 == 3:
            for p in range(batch):
                sc[p][row] = EDGE[(p + i) % len(EDGE)]
    return sc, np.array(row_idx, dtype=np.uint32)


@pytest.mark.parametrize("batch", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("n", [1, K - 1, K, K + 1, 3 * K + 2])
@pytest.mark.parametrize("group", [1, 2])
def test_images_and_uniform_modes_vs_oracle(zk_ctx, cref, group, n, batch):
    bases = _bases(cref, group, n)
    sc, row_idx = _case(n, batch)
    std = np.stack([_image(row, 0) for row in sc])
    scal = {0: std, 1: np.stack([_image(row, 1) for row in sc])}
    want, memo = [], {}
    for p in range(batch):
        picked = np.ascontiguousarray(std[p][row_idx])
        key = picked.tobytes()
        if key not in memo:
            memo[key] = cref.msm(group, bases, picked, naive=True)
        want.append(memo[key])
    want = np.stack(want)
    for table_image in (0, 1):
        h = zk_ctx.msm_bases_load_image(group, bases, n, 300 + K, table_image)
        try:
            for scalar_image in (0, 1):
                for uniform in (0, 1, 2):
                    out = np.zeros_like(want)
                    zk_ctx.msm_batch_rows(h, scal[scalar_image], n + 3, row_idx, batch,
                                          scalar_image, uniform, out)
                    assert np.array_equal(out, want), (table_image, scalar_image, uniform)
        finally:
            zk_ctx.msm_bases_free(h)


@pytest.mark.parametrize("wb", [8, 106, 200 + K])
def test_other_plans_take_both_images(zk_ctx, cref, wb):
    """per-window, shared and subset-sum tables ignore the image of the load and still convert"""
    n, batch = 3 * K + 2, 65
    bases = _bases(cref, 1, n)
    sc, row_idx = _case(n, batch)
    std = np.stack([_image(row, 0) for row in sc])
    want = np.stack([cref.msm(1, bases, np.ascontiguousarray(std[p][row_idx]), naive=True)
                     for p in range(batch)])
    h = zk_ctx.msm_bases_load_image(1, bases, n, wb, 1)
    try:
        for image in (0, 1):
            out = np.zeros_like(want)
            zk_ctx.msm_batch_rows(h, np.stack([_image(row, image) for row in sc]), n + 3, row_idx,
                                  batch, image, 0, out)
            assert np.array_equal(out, want), image
    finally:
        zk_ctx.msm_bases_free(h)


def test_row_map_is_range_checked(zk_ctx, cref):
    from gnark_crypto_primitives_amd.lib import ZkmiError
    bases = _bases(cref, 1, K)
    h = zk_ctx.msm_bases_load_image(1, bases, K, 300 + K, 1)
    try:
        with pytest.raises(ZkmiError):
            zk_ctx.msm_batch_rows(h, np.zeros((2, K, 4), np.uint64), K,
                                  np.array([0, 1, 2, 3, K], dtype=np.uint32), 2, 0, 0,
                                  np.zeros((2, 8), np.uint64))
    finally:
        zk_ctx.msm_bases_free(h)


@pytest.mark.parametrize("fold", [True, False])
def test_poseidon_proofs_on_sign_pattern_plans(zk_ctx, cref, fold):
    """single Poseidon, 70 lanes, lane 5 unsatisfied, sign-pattern plans for both groups: wire MSMs
    on F-native tables, the quotient MSM on a std-native one, flags once per batch"""
    from oracle import pyref
    cc = compile_circuit(circuits.PoseidonCircuit())
    pk, _, _ = groth16.setup(cc, 71, groth16.gpu_mul(zk_ctx))
    rng = random.Random(71)
    B = 70
    datas = [0, 1, R - 1] + [rng.randrange(R) for _ in range(B - 3)]
    inp = np.stack([to_mont_array(cc.assignment_vector(
        {"Data": d, "Hash": pyref.poseidon_hash([d])})) for d in datas])
    inp[5] = to_mont_array(cc.assignment_vector({"Data": 5, "Hash": 7}))
    rs = np.stack([to_mont_array([rng.randrange(R), rng.randrange(R)]) for _ in range(B)])
    want, wstatus, _ = cref.groth16_prove_batch(cref.R1csHandle(cc), cref.PkHandle(pk), inp, rs)
    prover = groth16.Prover(zk_ctx, cc, pk, window_bits_g1=300 + K, window_bits_g2=300 + K - 1,
                            fold_quotient=fold)
    try:
        assert prover.folded == fold
        prover.submit(inp, rs)
        proofs, status = prover.collect()
    finally:
        prover.close()
    assert list(status != 0) == list(wstatus != 0) == [i == 5 for i in range(B)]
    ok = status == 0
    assert np.array_equal(proofs[ok], want[ok])
