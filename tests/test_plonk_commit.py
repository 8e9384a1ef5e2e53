"""PLONK lowering of circuits that call api.Commit (frontend/scs.py), without a GPU: the committed
and commitment rows, the Qcp columns, host evaluation against ``is_satisfied`` with pi2 / H computed
here, and a circuit without commitments lowering as before.  What gnark's scs builder emits is
recalled, not pinned [UPSTREAM-RECALL]: parity unpinned."""
import hashlib

import pytest

from gnark_crypto_primitives_amd import hash_to_field
from gnark_crypto_primitives_amd.frontend import Public, Secret, compile_circuit
from gnark_crypto_primitives_amd.frontend.api import (OP_ABC, OP_ADD, OP_ADDC, OP_MUL, OP_MULABC,
                                                      OP_MULC)
from gnark_crypto_primitives_amd.frontend.scs import compile_scs
from tests.test_commitment import RangeCircuit, TwoCommitments

R = hash_to_field.R
CASES = [(0x11 * 0x22, 0x1122334455662211, True), (0x11 * 0x22 + 1, 0x2211, False),
         (0x11 * 0x22, 0x2211 + (1 << 64), False), (8184, 0x21f8, True), (8190, 0x2ac3, False)]


def stand_in(idx, vals):
    """a commitment hash for the host evaluation: any function of the committed values will do"""
    h = hashlib.sha256(b"test %d" % idx)
    for v in vals:
        h.update(int(v).to_bytes(32, "big"))
    return int.from_bytes(h.digest(), "big") % R


def rows_have_the_stated_shape(sc):
    n_pub = sc.n_public - 1
    seen = set()
    for i, c in enumerate(sc.commitments):
        assert c["rows"] == sorted(set(c["rows"])) and len(c["rows"]) >= 1
        assert c["row"] not in c["rows"] and min(c["rows"]) > n_pub
        for g in c["rows"] + [c["row"]]:
            wa, wb, wc, qL, qR, qO, qM, qC = sc.gates[g]
            assert wa == wb == wc and (qL, qR, qO, qM, qC) == (R - 1, 0, 0, 0, 0)
        assert sc.gates[c["row"]][0] == c["val"]
        assert [int(v) for v in sc.qcp[i]] == [1 if g in c["rows"] else 0
                                               for g in range(1 << sc.log_n)]
        assert not seen & set(c["rows"])
        seen |= set(c["rows"])
        xa, xb, xc, n_wires = sc.wiring()
        assert xa[c["row"]] == xb[c["row"]] == xc[c["row"]] == c["wire"] < n_wires
        # the program's check flag is off on these rows: they hold by construction
        for w0, d, x, y in (q for row in sc.vprogram.tolist() for q in row[1:]):
            if w0 & 0x1f == OP_ABC and (w0 >> 9) in c["rows"] + [c["row"]]:
                assert not w0 & 0x20
    assert len(sc.qcp) == len(sc.commitments)


@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_range_circuit_lowers_and_evaluates(lanes):
    cc = compile_circuit(RangeCircuit(), lanes)
    assert cc.n_constraints == 51 and len(cc.commitments) == 1
    sc = compile_scs(RangeCircuit(), lanes)
    assert len(sc.commitments) == 1 and len(sc.commitments[0]["rows"]) == 37
    rows_have_the_stated_shape(sc)
    sc.commit_fn = stand_in
    for x, y, ok in CASES:
        _, a, b, c = sc.run_vprogram(sc.assignment_vector({"X": x, "Y": y}))
        assert (sc.last_status == 0) == ok
        cm = sc.commitments[0]
        pi2 = [{g: a[g] for g in cm["rows"]}]
        H = [stand_in(0, [a[g] for g in cm["rows"]])]
        assert sc.is_satisfied(a, b, c, [x], pi2=pi2, H=H)[0] == ok, (x, y)
        assert sc.is_satisfied(a, b, c, [x])[0] == ok
        if ok:
            assert a[cm["row"]] == H[0]
            assert not sc.is_satisfied(a, b, c, [x], pi2=pi2, H=[(H[0] + 1) % R])[0]
            g = cm["rows"][5]
            bad = [dict(pi2[0])]
            bad[0][g] = (bad[0][g] + 1) % R
            assert sc.is_satisfied(a, b, c, [x], pi2=bad, H=H) == (False, g)
            assert not sc.is_satisfied(a, b, c, [(x + 1) % R], pi2=pi2, H=H)[0]


def test_two_commitments_second_one_commits_public_and_first():
    cc = compile_circuit(TwoCommitments())
    assert cc.n_constraints == 4 and len(cc.commitments) == 2
    sc = compile_scs(TwoCommitments())
    rows_have_the_stated_shape(sc)
    c1, c2 = sc.commitments
    assert len(c1["rows"]) == 2 and len(c2["rows"]) == 4 and c1["row"] < c2["rows"][0]
    # X, t, c1 and y2 + 1, in operand order: the public wire and the first commitment's wire included
    vals = [sc.gates[g][0] for g in c2["rows"]]
    assert vals[0] == 1 and vals[2] == c1["val"] and len(set(vals)) == 4
    sc.commit_fn = stand_in
    _, a, b, c = sc.run_vprogram(sc.assignment_vector({"X": 49, "Y": 7}))
    assert sc.last_status == 0
    assert [a[g] for g in c1["rows"]] == [7, 49]
    h1 = stand_in(0, [7, 49])
    assert [a[g] for g in c2["rows"]] == [49, h1 * 7 % R, h1, 50]
    H = [h1, stand_in(1, [49, h1 * 7 % R, h1, 50])]
    pi2 = [[a[g] if g in cm["rows"] else 0 for g in range(sc.n_gates)] for cm in sc.commitments]
    assert sc.is_satisfied(a, b, c, [49], pi2=pi2, H=H) == (True, -1)
    assert not sc.is_satisfied(a, b, c, [49], pi2=pi2, H=H[::-1])[0]
    assert not sc.is_satisfied(a, b, c, [49], pi2=pi2[::-1], H=H)[0]
    sc.run_vprogram(sc.assignment_vector({"X": 50, "Y": 7}))
    assert sc.last_status != 0


class Plain:
    X = Public()
    Y = Secret()

    def define(self, api):
        t = api.Mul(self.Y, self.Y)
        u = api.Add(api.Add(t, self.Y), 5)
        api.AssertIsEqual(api.Mul(u, 3), self.X)


def test_circuit_without_commitments_lowers_as_before():
    """one gate per operation, as the module's table states them (written out here)"""
    sc = compile_scs(Plain())
    assert sc.commitments == [] and sc.qcp == []
    m1 = R - 1
    cc = sc.cc
    want = [(1, 1, 1, 1, 0, 0, 0, 0), (0, 0, 0, 1, 0, 0, 0, m1)]
    prog = [(OP_ABC, 1, 1, 1), (OP_ABC, 0, 0, 0)]
    k_row = 0
    for op, d, a, b in cc._ops:
        if op == OP_ABC:
            want.append((d, a, b, 0, 0, m1, 1, 0))
            prog.append((OP_ABC, d, a, b))
            k_row += 1
            continue
        gate = {OP_MUL: (a, b, d, 0, 0, m1, 1, 0), OP_MULABC: (a, b, d, 0, 0, m1, 1, 0),
                OP_ADD: (a, b, d, 1, 1, m1, 0, 0)}.get(op)
        if op == OP_ADDC:
            gate = (a, a, d, 1, 0, m1, 0, cc.consts[b])
        elif gate is None:
            assert op == OP_MULC
            gate = (a, a, d, cc.consts[b], 0, m1, 0, 0)
        want.append(gate)
        prog += [(OP_MUL if op == OP_MULABC else op, d, a, b), (OP_ABC, gate[0], gate[1], gate[2])]
    assert sc.gates == want and sc.n_gates == len(want)
    # sigma: the positions holding one value form one cycle, in column-major order
    n = 1 << sc.log_n
    where = {}
    for col in range(3):
        for r, g in enumerate(want):
            where.setdefault(g[col], []).append(col * n + r)
    for pos in where.values():
        for i, p in enumerate(pos):
            assert sc.sigma[p] == pos[(i + 1) % len(pos)]
    assert all(sc.sigma[c * n + r] == c * n + r for c in range(3) for r in range(len(want), n))
    # the program: the same operations with an OP_ABC row per gate, evaluated on the host
    x = 3 * (11 * 11 + 11 + 5)
    _, a, b, c = sc.run_vprogram(sc.assignment_vector({"X": x, "Y": 11}))
    assert sc.last_status == 0 and sc.is_satisfied(a, b, c, [x]) == (True, -1)
    ops = [q[0] & 0x1f for row in sc.vprogram.tolist() for q in row[1:] if q[0] & 0x1f]
    assert sorted(ops) == sorted(p[0] for p in prog)
    assert a[:2] == [x, 1] and a[2:5] == [11, 121, 132]
