"""ScsCircuit.wiring() / wire_vectors(): the wire form of a sparse constraint system, what
zkmi_scs_desc and zkmi_plonk_prove_witness take.  Gathering the wire vector through the wiring
gives the solved columns back, the wires are numbered densely with ONE and the public inputs in
front, and the cycles of sigma are the classes of equal wires."""
import random

import numpy as np
import pytest

from gnark_crypto_primitives_amd import circuits
from gnark_crypto_primitives_amd.frontend.compile import from_mont_array, to_mont_array
from gnark_crypto_primitives_amd.frontend.scs import compile_scs
from gnark_crypto_primitives_amd.hash import poseidon_native
from tests.test_frontend import Mixed, _mixed_expected

R = poseidon_native.R


def _poseidon():
    sc = compile_scs(circuits.PoseidonCircuit())
    rng = random.Random(3)
    datas = [rng.randrange(R) for _ in range(3)]
    return sc, [sc.assignment_vector({"Data": d, "Hash": poseidon_native.hash([d])}) for d in datas]


def _mixed():
    sc = compile_scs(Mixed())
    asg = [(7 + i, 1000 + 3 * i) for i in range(3)] + [(40000, 40000)]
    return sc, [sc.assignment_vector({"X": x, "Y": y, "Z": _mixed_expected(x, y)}) for x, y in asg]


@pytest.mark.parametrize("make", [_poseidon, _mixed])
def test_wire_vector_gathers_back_to_the_columns(make):
    sc, inps = make()
    xa, xb, xc, n_wires = sc.wiring()
    n_pub = sc.n_public - 1
    assert all(x.dtype == np.uint32 and x.shape == (sc.n_gates,) for x in (xa, xb, xc))
    # dense: every wire below n_wires is read somewhere; ONE and the public inputs keep their places
    assert sorted(set(xa.tolist()) | set(xb.tolist()) | set(xc.tolist())) == list(range(n_wires))
    assert xa[:n_pub + 1].tolist() == list(range(1, n_pub + 1)) + [0]
    cols = [sc.run_vprogram(inp)[1:] for inp in inps]
    a, b, c = ([col[k] for col in cols] for k in range(3))
    wires = sc.wire_vectors(a, b, c)
    for w, inp, ai, bi, ci in zip(wires, inps, a, b, c):
        assert len(w) == n_wires and w[0] == 1 and w[1:n_pub + 1] == list(inp[:n_pub])
        ga, gb, gc = ([w[i] for i in x.tolist()] for x in (xa, xb, xc))
        assert (ga, gb, gc) == (list(ai), list(bi), list(ci))
        assert sc.is_satisfied(ga, gb, gc, inp[:n_pub]) == (True, -1)
    # the array form (Montgomery images, what the C entry takes) agrees with the integer form
    arr = sc.wire_vectors(*(np.stack([to_mont_array(col) for col in x]) for x in (a, b, c)))
    assert arr.shape == (len(inps), n_wires, 4) and arr.dtype == np.uint64
    assert [from_mont_array(v) for v in arr] == wires


@pytest.mark.parametrize("make", [_poseidon, _mixed])
def test_sigma_cycles_are_the_classes_of_equal_wires(make):
    sc, _ = make()
    xa, xb, xc, _ = sc.wiring()
    n = 1 << sc.log_n
    x = (xa, xb, xc)
    for p in range(3 * n):
        q = int(sc.sigma[p])
        if p % n >= sc.n_gates:
            assert q == p
        else:
            assert q % n < sc.n_gates and x[q // n][q % n] == x[p // n][p % n]
    # a changed wire shows as an unsatisfied gate, never as a broken copy constraint
    _, inps = make()
    _, a, b, c = sc.run_vprogram(inps[0])
    w = sc.wire_vectors([a], [b], [c])[0]
    w[int(xc[sc.n_gates - 1])] = (w[int(xc[sc.n_gates - 1])] + 1) % R
    ga, gb, gc = ([w[i] for i in col.tolist()] for col in x)
    ok, where = sc.is_satisfied(ga, gb, gc, inps[0][:sc.n_public - 1])
    assert not ok and where >= 0
