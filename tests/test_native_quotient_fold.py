"""Host side of the quotient in evaluation form.  tests/native/quotient_fold_check.cpp builds the
fold plan of csrc/quotient_fold.h (what zkmi_pk_load makes of zkmi_pk_desc.fold_r1cs) for a hand-made
O and checks it against a dense matrix, 256-bit reference scalars and every refusal; it is built
plain and with -fsanitize=address,undefined, and the two builds must print the same.  The identity
the fold rests on is checked here in Python integers, the bases taken as scalars."""
import random

import pytest

from tests import helpers as H
from tests import native_build

R = H.R


@native_build.needs_gxx
def test_fold_plan_native(tmp_path):
    _, out, _ = native_build.run_both(native_build.build("quotient_fold_check.cpp", tmp_path))
    assert out.splitlines() == ["ok den", "ok plan terms=23 columns=6", "ok merge bases=9", "ok refusals"]


def _intt(x, w_inv, n, shift_inv=1):
    """inverse transform on the domain (shift_inv = 1) or on the coset g <w> (shift_inv = 1 / g)"""
    n_inv = pow(n, R - 2, R)
    return [sum(x[i] * pow(w_inv, i * k, R) for i in range(n)) % R * n_inv % R * pow(shift_inv, k, R) % R
            for k in range(n)]


@pytest.mark.parametrize("log_n", [3, 4])
def test_identity_in_integers(log_n):
    """sum_k h_k Z_k with h = cosetiNTT(a_c b_c den) - den iNTT(c), as the prover computes it, equals
    sum_i (a_c b_c)_i E_i + sum_w wire_w D_w, with Z_k = tau^k z as scalars, Z_(n-1) = 0,
    n_constraints = n - 3 and random a_c b_c: both are linear in (a_c b_c, wires), so no witness
    has to satisfy anything."""
    n = 1 << log_n
    rng = random.Random(90 + log_n)
    w = pow(5, (R - 1) >> log_n, R)
    w_inv, g_inv, n_inv = pow(w, R - 2, R), pow(5, R - 2, R), pow(n, R - 2, R)
    den = pow(pow(5, n, R) - 1, R - 2, R)
    tau, z = rng.randrange(1, R), rng.randrange(1, R)
    Z = [pow(tau, k, R) * z % R for k in range(n - 1)] + [0]
    n_c, n_w = n - 3, 6
    O = [[rng.choice((0, 0, 1, R - 1, rng.randrange(R))) for _ in range(n_w)] for _ in range(n_c)]
    wires = [1] + [rng.randrange(R) for _ in range(n_w - 1)]
    ab = [rng.randrange(R) for _ in range(n)]
    c = [sum(O[i][j] * wires[j] for j in range(n_w)) % R for i in range(n_c)] + [0] * (n - n_c)
    # the prover's side
    h1 = _intt([x * den % R for x in ab], w_inv, n, g_inv)
    h2 = _intt(c, w_inv, n)
    lhs = sum((h1[k] - den * h2[k]) * Z[k] for k in range(n)) % R
    # the folded key's side
    E = [den * n_inv % R * sum(pow(g_inv, k, R) * pow(w_inv, i * k, R) * Z[k] for k in range(n)) % R
         for i in range(n)]
    L = [n_inv * sum(pow(w_inv, i * k, R) * Z[k] for k in range(n)) % R for i in range(n)]
    D = [(R - den) * sum(O[i][j] * L[i] for i in range(n_c)) % R for j in range(n_w)]
    rhs = (sum(ab[i] * E[i] for i in range(n)) + sum(wires[j] * D[j] for j in range(n_w))) % R
    assert lhs == rhs
