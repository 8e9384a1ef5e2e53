"""The comb plan of a proving key: one group size k per MSM (csrc/comb_plan.h).
tests/native/comb_plan_check.cpp prints the equal-k plan and the searched plan of one input through
the functions zkmi_pk_load calls; built plain and with -fsanitize=address,undefined, the two builds
must print the same.  Bytes and costs are recomputed here in Python."""
import pytest

from tests import native_build

pytestmark = native_build.needs_gxx
ARBO = (40196, 27059, 40522, 65536, 27059)      # A, B1, K, Z (folded key), B2 of the Arbo-160 key
GUARD = 0.02


def _bytes(n, k, sg):
    return sum(-(-ni // ki) * (1 << (ki - si)) * (128 if i == 4 else 64)
               for i, (ni, ki, si) in enumerate(zip(n, k, sg)))


def _cost(n, k, sg, phi):
    per = lambda i, s: ((255 * 178.5 if s else 254 * 171.6) if i == 4 else
                        (255 * 62.8 if s else 254 * 61.1))
    return sum((1.0 if i == 3 else phi) * per(i, si) * -(-ni // ki)
               for i, (ni, ki, si) in enumerate(zip(n, k, sg)))


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    return native_build.build("comb_plan_check.cpp", tmp_path_factory.mktemp("comb_plan"))


def _plan(exes, n, budget, allow_signed=1, phi=0.5, guard=GUARD):
    args = [*map(str, n), repr(float(budget)), str(allow_signed), repr(phi), repr(guard)]
    _, out, _ = native_build.run_both(exes, args)
    res = {}
    for line in out.splitlines():
        name, *f = line.split()
        k, sg = [int(x) for x in f[:5]], [int(x) for x in f[5:10]]
        res[name] = {"k": k, "sg": sg, "fits": int(f[10]), "bytes": float(f[11]),
                     "worst": float(f[12])}
        # what the header computes is what this file computes
        assert res[name]["bytes"] == _bytes(n, k, sg)
        assert abs(res[name]["worst"] - _cost(n, k, sg, 1.0)) <= 1e-6 * res[name]["worst"]
        for ki, si in zip(k, sg):
            assert 8 <= ki <= (21 if si else 20)
            assert allow_signed or not si
    return res["equal"], res["search"]


def test_phi_one_is_the_equal_k_plan(exes):
    eq, p = _plan(exes, ARBO, 244e9, phi=1.0)
    assert eq["k"] == [19, 19, 19, 19, 20] and eq["sg"] == [1] * 5 and eq["fits"]
    assert p["k"] == eq["k"] and p["sg"] == eq["sg"] and p["fits"]
    assert p["bytes"] <= 244e9


def test_headline_plan_widens_the_quotient_table(exes):
    eq, p = _plan(exes, ARBO, 244e9, phi=0.5)
    assert p["fits"] and p["bytes"] <= eq["bytes"] <= 244e9
    assert p["k"][3] >= 20
    # a machine with more free HBM than the equal-k plan takes: the same plan, not a larger one
    assert _plan(exes, ARBO, 270e9, phi=0.5)[1] == p
    assert p["worst"] <= (1 + GUARD) * eq["worst"]
    assert _cost(ARBO, p["k"], p["sg"], 0.5) < _cost(ARBO, eq["k"], eq["sg"], 0.5)


@pytest.mark.parametrize("gb", [32, 64, 128, 244])
@pytest.mark.parametrize("allow_signed", [0, 1])
@pytest.mark.parametrize("phi", [0.5, 1.0])
def test_plans_fit_their_budget_and_the_guard(exes, gb, allow_signed, phi):
    eq, p = _plan(exes, ARBO, gb * 1e9, allow_signed, phi)
    assert eq["fits"] and p["fits"]
    assert p["bytes"] <= gb * 1e9 and p["bytes"] <= eq["bytes"]
    assert p["worst"] <= (1 + GUARD) * eq["worst"]
    # never worse than the equal-k plan under the weights it was searched with
    assert _cost(ARBO, p["k"], p["sg"], phi) <= _cost(ARBO, eq["k"], eq["sg"], phi)


def test_tight_guard_keeps_the_worst_case(exes):
    eq, p = _plan(exes, ARBO, 244e9, phi=0.5, guard=0.0)
    assert p["worst"] <= eq["worst"]


def test_budget_too_small_for_any_comb_plan(exes):
    eq, p = _plan(exes, ARBO, 1e6)
    assert not eq["fits"] and not p["fits"]
    assert p["k"] == [8] * 5 == eq["k"]


def test_msms_without_bases_and_small_keys(exes):
    # a key planned for G1 only (explicit G2 plan): B2 brings no bases and no bytes
    n = (ARBO[0], ARBO[1], ARBO[2], ARBO[3], 0)
    eq, p = _plan(exes, n, 100e9)
    assert p["fits"] and p["bytes"] <= 100e9 and p["k"][4] == eq["k"][4]
    # few bases: every table fits at the widest k, which is then the plan
    eq, p = _plan(exes, (40, 30, 41, 64, 30), 244e9)
    assert p["fits"] and p["bytes"] <= 244e9
    assert p["worst"] <= eq["worst"]
