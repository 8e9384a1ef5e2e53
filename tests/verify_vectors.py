"""Groth16 verifying keys and proofs without a circuit, for the verifier tests.

With chosen scalars alpha, beta, gamma, delta and k_0 .. k_n the key is (alpha G1, beta G2, gamma G2,
delta G2, K_j = k_j G1).  For public inputs pub, x = k_0 + sum pub_j k_j, and any a, b with
c = (a b - alpha beta - x gamma) / delta give a valid proof (a G1, c G1, b G2).  Two edges no prover
produces are reachable this way: Krs at infinity on a valid proof (c = 0, solve for a) and vk_x at
infinity (pub_1 = -(k_0 + sum_{j>1} pub_j k_j) / k_1).

``mul(group, scalars_mont[n, 4]) -> points`` multiplies the generator (cpu_mul here; groth16.gpu_mul
has the same shape)."""
import random

import numpy as np

from gnark_crypto_primitives_amd import groth16
from gnark_crypto_primitives_amd import verify as V
from gnark_crypto_primitives_amd.frontend.compile import ints_to_array, to_mont_array

R, P = V.R, V.P
MONT = (1 << 256) % P

# the cases every verifier must decide like verify.verify, and which of them it accepts
CASES = ["valid", "wrong_public", "krs_swapped", "ar_bitflip", "ar_noncanonical", "ar_inf",
         "bs_inf", "bs_not_in_subgroup", "krs_inf_valid", "vkx_inf_valid"]
ACCEPTED = {"valid", "krs_inf_valid", "vkx_inf_valid"}
NEEDS_PUBLIC = {"wrong_public", "vkx_inf_valid"}


def cpu_mul(group, scalars):
    from oracle import cref
    from tests import helpers
    base = helpers.g1_gen_mont() if group == 1 else helpers.g2_gen_mont()
    return cref.batch_mul(group, base, np.ascontiguousarray(scalars))


def _mul_ints(mul, group, scalars):
    """generator multiples of integer scalars; the multiple by 0 is the all-zero image"""
    pts = np.array(mul(group, to_mont_array([s % R for s in scalars])), dtype=np.uint64)
    for i, s in enumerate(scalars):
        if s % R == 0:
            pts[i] = 0
    return pts


# ---- Fq2 for the point outside the subgroup --------------------------------------------------------
def _mul2(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def _pow2(a, e):
    out = (1, 0)
    while e:
        if e & 1:
            out = _mul2(out, a)
        a = _mul2(a, a)
        e >>= 1
    return out


def fq2_sqrt(a):
    """square root in Fq2 by exponentiation (p = 3 mod 4), or None"""
    a1 = _pow2(a, (P - 3) // 4)
    alpha = _mul2(_mul2(a1, a1), a)
    a0 = _mul2((alpha[0], (-alpha[1]) % P), alpha)
    if a0 == (P - 1, 0):
        return None
    x0 = _mul2(a1, a)
    if alpha == (P - 1, 0):
        x = _mul2((0, 1), x0)
    else:
        x = _mul2(_pow2(((1 + alpha[0]) % P, alpha[1]), (P - 1) // 2), x0)
    return x if _mul2(x, x) == (a[0] % P, a[1] % P) else None


def twist_point_outside_subgroup(x=1):
    """(x + 0 u, sqrt(x^3 + 3 / (9 + u))): on the twist, not of order r; integer coordinates"""
    d = pow(82, P - 2, P)
    b2 = (27 * d % P, (-3 * d) % P)
    y = fq2_sqrt(((x ** 3 + b2[0]) % P, b2[1]))
    assert y is not None
    return ((x % P, 0), y)


def g2_image(q):
    return ints_to_array([c * MONT % P for c in (q[0][0], q[0][1], q[1][0], q[1][1])]).reshape(-1)


# ---- keys and proofs -------------------------------------------------------------------------------
class SynthKey:
    def __init__(self, n_inputs, seed, mul):
        rng = random.Random(seed)
        self.n_inputs = n_inputs
        self.alpha, self.beta, self.gamma, self.delta = (rng.randrange(1, R) for _ in range(4))
        self.k = [rng.randrange(1, R) for _ in range(n_inputs + 1)]
        g1 = _mul_ints(mul, 1, self.k + [self.alpha])
        g2 = _mul_ints(mul, 2, [self.beta, self.gamma, self.delta])
        vk = self.vk = groth16.VerifyingKey()
        vk.g1_k = np.ascontiguousarray(g1[:n_inputs + 1])
        vk.g1_alpha = g1[n_inputs + 1].copy()
        vk.g2_beta, vk.g2_gamma, vk.g2_delta = g2[0].copy(), g2[1].copy(), g2[2].copy()

    def x(self, pub):
        return (self.k[0] + sum(p * k for p, k in zip(pub, self.k[1:]))) % R

    def scalars(self, pub, rng, krs_inf=False):
        """(a, c, b) of a valid proof for these public inputs"""
        ab = (self.alpha * self.beta + self.x(pub) * self.gamma) % R
        b = rng.randrange(1, R)
        if krs_inf:
            return ab * pow(b, R - 2, R) % R, 0, b
        a = rng.randrange(1, R)
        return a, (a * b - ab) * pow(self.delta, R - 2, R) % R, b

    def pub_vkx_inf(self, rng):
        pub = [rng.randrange(R) for _ in range(self.n_inputs)]
        rest = (self.k[0] + sum(p * k for p, k in zip(pub[1:], self.k[2:]))) % R
        pub[0] = (-rest) * pow(self.k[1], R - 2, R) % R
        return pub


def make_batch(key, batch, cases, seed, mul):
    """-> (pubs: batch lists of ints, proofs uint64[batch, 32], expected bool[batch]).  ``cases``:
    {lane: name from CASES}; every other lane holds a plain valid proof."""
    rng = random.Random(seed)
    kinds = [cases.get(i, "valid") for i in range(batch)]
    pubs = [key.pub_vkx_inf(rng) if kd == "vkx_inf_valid" else
            [rng.randrange(R) for _ in range(key.n_inputs)] for kd in kinds]
    sc = [key.scalars(pub, rng, kd == "krs_inf_valid") for pub, kd in zip(pubs, kinds)]
    sc.append(key.scalars(pubs[0], rng))              # donor of a foreign Krs
    g1 = _mul_ints(mul, 1, [s[0] for s in sc] + [s[1] for s in sc])
    g2 = _mul_ints(mul, 2, [s[2] for s in sc])
    n = batch + 1
    proofs = np.zeros((batch, 32), dtype=np.uint64)
    proofs[:, 0:8], proofs[:, 8:16], proofs[:, 16:32] = g1[:batch], g1[n:n + batch], g2[:batch]
    for i, kd in enumerate(kinds):
        if kd == "wrong_public":
            pubs[i][0] = (pubs[i][0] + 1) % R
        elif kd == "krs_swapped":
            proofs[i, 8:16] = g1[n + batch]
        elif kd == "ar_bitflip":
            proofs[i, 0] ^= np.uint64(1)
        elif kd == "ar_noncanonical":                  # x + p fits 256 bits, is not canonical
            x = sum(int(w) << (64 * j) for j, w in enumerate(proofs[i, 0:4])) + P
            proofs[i, 0:4] = ints_to_array([x]).reshape(-1)
        elif kd == "ar_inf":
            proofs[i, 0:8] = 0
        elif kd == "bs_inf":
            proofs[i, 16:32] = 0
        elif kd == "bs_not_in_subgroup":
            proofs[i, 16:32] = g2_image(twist_point_outside_subgroup(1))
    return pubs, proofs, np.array([kd in ACCEPTED for kd in kinds])


def pubs_mont(pubs, n_inputs):
    """uint64[batch, n_inputs, 4] Montgomery image of integer public inputs"""
    flat = [p for row in pubs for p in row]
    arr = to_mont_array(flat) if flat else np.zeros((0, 4), np.uint64)
    return np.ascontiguousarray(arr, dtype=np.uint64).reshape(len(pubs), n_inputs, 4)
