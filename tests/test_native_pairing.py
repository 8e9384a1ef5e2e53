"""Host build of csrc/pairing.h (tests/native/test_pairing.cpp): the BN254 pairing and the per-proof
Groth16 decision (decode and point checks, shared-squaring Miller loop, final exponentiation),
against verify.py's Python integers.  The driver is built twice, plain -O2 and under UBSan + ASan (a
program of its own, run directly), and both builds must print the same."""
import random

import numpy as np
import pytest

from gnark_crypto_primitives_amd import verify as V
from tests import helpers, native_build, verify_vectors as vv

P, R = V.P, V.R
PAIRS = [(5, 7), (0x1234567890abcdef1234567890abcdef, R - 3), (R - 1, 2 ** 200 + 9)]
N_INPUTS = 3

pytestmark = native_build.needs_gxx


def _hex(a):
    return np.ascontiguousarray(a, dtype=np.uint64).tobytes().hex()


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """the driver's answers to one command script, from both builds: {label: output lines}"""
    tmp = tmp_path_factory.mktemp("pairing")
    rng = random.Random(2024)
    key = vv.SynthKey(N_INPUTS, 11, vv.cpu_mul)
    cases = dict(enumerate(vv.CASES))
    pubs, proofs, expected = vv.make_batch(key, len(vv.CASES), cases, 12, vv.cpu_mul)
    # pairing operands: aP, -abP, -P in G1; bQ, Q in G2
    g1s, g2s = [], []
    for a, b in PAIRS:
        g1s += [a, (-a * b) % R, R - 1]
        g2s += [b, 1]
    g1 = vv._mul_ints(vv.cpu_mul, 1, g1s)
    g2 = vv._mul_ints(vv.cpu_mul, 2, g2s + [rng.randrange(1, R)])
    outside = vv.g2_image(vv.twist_point_outside_subgroup(1))
    script, labels = ["consts"], ["consts"]
    for i in range(len(PAIRS)):
        aP, nabP, nP, bQ, Q = g1[3 * i], g1[3 * i + 1], g1[3 * i + 2], g2[2 * i], g2[2 * i + 1]
        script += [f"pair {_hex(aP)} {_hex(bQ)}",
                   f"prod2 {_hex(aP)} {_hex(bQ)} {_hex(nabP)} {_hex(Q)}",
                   f"prod2 {_hex(aP)} {_hex(bQ)} {_hex(nP)} {_hex(Q)}"]
        labels += [f"pair{i}", f"bilinear{i}", f"nondegenerate{i}"]
    script += [f"g2 {_hex(g2[1])}", f"g2 {_hex(g2[-1])}", f"g2 {_hex(outside)}"]
    labels += ["g2_generator", "g2_multiple", "g2_outside"]
    vk = key.vk
    script.append(" ".join(["vk", str(N_INPUTS + 1)] + [_hex(k) for k in vk.g1_k] +
                           [_hex(vk.g1_alpha), _hex(vk.g2_beta), _hex(vk.g2_gamma), _hex(vk.g2_delta)]))
    labels.append("vk")
    pm = vv.pubs_mont(pubs, N_INPUTS)
    for i, name in enumerate(vv.CASES):
        script.append(f"verify {_hex(proofs[i])} {_hex(pm[i])}")
        labels.append("verify_" + name)
    # key loading refuses: gamma outside the subgroup, alpha off the curve, no ONE wire
    bad_alpha = vk.g1_alpha.copy()
    bad_alpha[0] ^= np.uint64(1)
    ks = [_hex(k) for k in vk.g1_k]
    script += [" ".join(["vk", str(N_INPUTS + 1)] + ks + [_hex(vk.g1_alpha), _hex(vk.g2_beta),
                                                         _hex(outside), _hex(vk.g2_delta)]),
               " ".join(["vk", str(N_INPUTS + 1)] + ks + [_hex(bad_alpha), _hex(vk.g2_beta),
                                                         _hex(vk.g2_gamma), _hex(vk.g2_delta)]),
               " ".join(["vk", "0", _hex(vk.g1_alpha), _hex(vk.g2_beta), _hex(vk.g2_gamma),
                         _hex(vk.g2_delta)])]
    labels += ["vk_gamma_outside", "vk_alpha_off_curve", "vk_no_wires"]
    _, out, _ = native_build.run_both(native_build.build("test_pairing.cpp", tmp),
                                      stdin="\n".join(script) + "\n")
    lines = out.strip().split("\n")
    assert lines.pop() == "pairing driver ok"
    res = {"consts": lines[:7]}
    assert len(lines) == 7 + len(labels) - 1
    for lab, ln in zip(labels[1:], lines[7:]):
        res[lab] = ln
    res["_key"], res["_pubs"], res["_proofs"], res["_expected"] = key, pubs, proofs, expected
    res["_g1"], res["_g2"] = g1, g2
    return res


def _ints(line):
    return [int(t, 16) for t in line.split()]


def _xi_pow(e):
    return vv._pow2((9, 1), e)


def test_parameters_and_tower_constants(run):
    c = run["consts"]
    u, ate_lo, ate_bits, n_lines = (int(t) for t in c[0].split())
    assert P == 36 * u ** 4 + 36 * u ** 3 + 24 * u ** 2 + 6 * u + 1
    assert R == 36 * u ** 4 + 36 * u ** 3 + 18 * u ** 2 + 6 * u + 1
    assert (1 << 64) + ate_lo == 6 * u + 2 == V.ATE_LOOP and ate_bits == V.ATE_LOOP.bit_length()
    assert n_lines == 64 + bin(V.ATE_LOOP).count("1") - 1 + 2
    # the hard part: digits of (p^4 - p^2 + 1) / r in base p as polynomials in u (multiple c = 1)
    d = [int(t) for t in c[1].split()]
    l0 = -sum(k * u ** i for i, k in enumerate(d[0:4]))
    l1 = 1 - sum(k * u ** i for i, k in enumerate(d[4:8]))
    l2 = sum(k * u ** i for i, k in enumerate(d[8:12]))
    assert (P ** 4 - P * P + 1) % R == 0
    assert l0 + l1 * P + l2 * P * P + P ** 3 == (P ** 4 - P * P + 1) // R
    for k in range(3):
        got = _ints(c[2 + k])
        for i in range(6):
            assert (got[2 * i], got[2 * i + 1]) == _xi_pow(i * (P ** (k + 1) - 1) // 6), (k, i)
    inv82 = pow(82, P - 2, P)
    assert _ints(c[5]) == [27 * inv82 % P, (-3 * inv82) % P]
    g = helpers.G2_GEN
    assert _ints(c[6]) == [1, 2, g[0][0], g[0][1], g[1][0], g[1][1]]


def _tower_to_single(vals):
    """12 Fq in tower order (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2; each a0, a1) -> coefficients
    of verify.py's basis 1, w, .., w^11 (v = w^2, u = w^6 - 9)"""
    out = [0] * 12
    for idx, i in enumerate([0, 2, 4, 1, 3, 5]):
        a0, a1 = vals[2 * idx], vals[2 * idx + 1]
        out[i] = (out[i] + a0 - 9 * a1) % P
        out[i + 6] = (out[i + 6] + a1) % P
    return out


@pytest.mark.parametrize("i", range(len(PAIRS)))
def test_gt_value_matches_python(run, i):
    p = V.g1_from_image(run["_g1"][3 * i])
    q = V.g2_from_image(run["_g2"][2 * i])
    want = V.final_exponentiation(V.miller_loop(q, p))
    assert _tower_to_single(_ints(run[f"pair{i}"])) == want


def test_bilinear_and_non_degenerate(run):
    for i in range(len(PAIRS)):
        assert run[f"bilinear{i}"] == "1"          # e(aP, bQ) e(-abP, Q) = 1
        assert run[f"nondegenerate{i}"] == "0"     # e(aP, bQ) e(-P, Q) != 1


def test_g2_subgroup_check(run):
    assert run["g2_generator"] == "1 1"
    assert run["g2_multiple"] == "1 1"
    assert run["g2_outside"] == "1 0"
    q = vv.twist_point_outside_subgroup(1)
    assert V._on_g2(q) and not V._in_g2_subgroup(q)


def test_key_loading(run):
    assert run["vk"] == "1"
    assert run["vk_gamma_outside"] == "0"
    assert run["vk_alpha_off_curve"] == "0"
    assert run["vk_no_wires"] == "0"


@pytest.mark.parametrize("case", vv.CASES)
def test_decision_equals_verify_py(run, case):
    i = vv.CASES.index(case)
    want = V.verify(run["_key"].vk, run["_pubs"][i], run["_proofs"][i])
    assert want == bool(run["_expected"][i]), "the vector is not what it was built to be"
    assert run["verify_" + case] == ("1" if want else "0")
