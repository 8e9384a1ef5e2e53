"""Host build of csrc/r1cs_plan.h, the solve plan of a gnark-shaped R1CS (what zkmi_r1cs_solver_load
builds and r1cs_solve_kernel runs): tests/native/r1cs_plan_check.cpp builds the plan of a system
dumped from compile_circuit for every number of sub-lanes 0 (auto), 1 .. 64 and interprets it on the
host.  Checked here: wires, a, b, c against the oracle's solver; the unknown the builder finds
against the frontend's solve_wire; the layout and the padding of the term rows; every refusal.  The
program is built plain and with -fsanitize=undefined,address; the two builds must agree byte for
byte."""
import functools
import random

import numpy as np
import pytest

from gnark_crypto_primitives_amd import circuits
from gnark_crypto_primitives_amd.ecc import babyjub_native as bjj
from gnark_crypto_primitives_amd.frontend import compile_circuit
from gnark_crypto_primitives_amd.frontend.compile import to_mont_array
from gnark_crypto_primitives_amd.tree import smt_witness
from oracle import cref
from tests import helpers as H
from tests.native_build import needs_gxx
from tests.r1cs_plan_harness import (BASIC, LANES_MSG, POW2, RK_ASSERT, RK_INVZERO, RK_NBITS, RK_SOLVE_L,
                                     RK_SOLVE_O, RK_SOLVE_R, parse, run)
from tests.r1cs_plan_harness import builds  # noqa: F401 (a fixture)
from tests.r1cs_plan_harness import description as std_description
from tests.test_frontend import Mixed, _mixed_expected

pytestmark = needs_gxx
# every system here is dumped under ZKMI_HINTS_BASIC, without commitment values
description = functools.partial(std_description, hint_set=BASIC)


@functools.lru_cache(maxsize=None)
def walk(cc):
    """The solve order as this test works it out from the description alone: per instruction the
    known terms {(tag, wire, coefficient index)} and the unknown wire (or None)."""
    kinds, in_ptr, lc_ptr, hcol, hcid, out_ptr, outs = cc.hint_arrays
    solved = np.zeros(cc.n_wires, dtype=bool)
    solved[:cc.n_public + cc.n_secret] = True
    res = []
    for kind, idx in cc.instr.tolist():
        known, unknown = [], None
        if kind == 1:
            lc = int(in_ptr[idx])
            known = [(0, int(hcol[t]), int(hcid[t])) for t in range(lc_ptr[lc], lc_ptr[lc + 1])]
            for x in outs[out_ptr[idx]:out_ptr[idx + 1]]:
                solved[x] = True
        else:
            for tag, (ptr, col, cid) in enumerate((cc.L, cc.Rm, cc.O)):
                for t in range(ptr[idx], ptr[idx + 1]):
                    if solved[col[t]]:
                        known.append((tag, int(col[t]), int(cid[t])))
                    else:
                        unknown = int(col[t])
            if unknown is not None:
                solved[unknown] = True
        res.append((known, unknown))
    assert solved.all()
    return res


def check_plan(cc, S, recs, terms, outs, n_coeffs):
    """the layout rules of r1cs_plan.h"""
    n_instr = cc.instr.shape[0]
    kinds = cc.hint_arrays[0]
    out_ptr, houts = cc.hint_arrays[5], cc.hint_arrays[6]
    unit_of = {i: 1 if v % H.R == 1 else 2 if v % H.R == H.R - 1 else 0 for i, v in enumerate(cc.consts)}
    assert recs.shape[0] == n_instr + 1
    tag, wire = terms[:, 0] >> 30, terms[:, 0] & 0x3fffffff
    unit, cid = terms[:, 1] >> 30, terms[:, 1] & 0x3fffffff
    pad = tag == 3
    assert (terms[pad] == [3 << 30, 0]).all()
    at, n_solves, longest, total = 0, 0, 0, 0
    for i, ((known, unknown), (ik, idx)) in enumerate(zip(walk(cc), cc.instr.tolist())):
        kind, target, coef, coef_inv, first, mul_rows, unit_rows, k = (int(x) for x in recs[i])
        assert first == at, i                                   # rows follow each other without gaps
        n_mul = sum(1 for t in known if unit_of[t[2]] == 0)
        n_unit = len(known) - n_mul
        assert mul_rows == -(-n_mul // S) and unit_rows == -(-n_unit // S), (i, S)
        m0, m1, u1 = first, first + mul_rows * S, first + (mul_rows + unit_rows) * S
        # every group: its terms first, padding only behind them, up to a whole row
        assert not pad[m0:m0 + n_mul].any() and pad[m0 + n_mul:m1].all(), i
        assert not pad[m1:m1 + n_unit].any() and pad[m1 + n_unit:u1].all(), i
        assert (unit[m0:m0 + n_mul] == 0).all() and (unit[m1:m1 + n_unit] != 0).all(), i
        got = sorted(zip(tag[m0:u1][~pad[m0:u1]].tolist(), wire[m0:u1][~pad[m0:u1]].tolist(),
                         cid[m0:u1][~pad[m0:u1]].tolist()))
        assert got == sorted(known), i
        assert all(unit_of[c] == u for c, u in zip(cid[m0:u1][~pad[m0:u1]].tolist(),
                                                   unit[m0:u1][~pad[m0:u1]].tolist())), i
        if ik == 1:
            assert kind == (RK_INVZERO if kinds[idx] == 1 else RK_NBITS)
            ows = houts[out_ptr[idx]:out_ptr[idx + 1]].tolist()
            if kind == RK_INVZERO:
                assert [target] == ows
            else:
                assert k == len(ows) and outs[target:target + k].tolist() == ows
        else:
            # the unknown the builder finds is the wire the frontend solves the constraint for
            sw = int(cc.solve_wire[idx])
            assert k == idx and (unknown if unknown is not None else -1) == sw, i
            if sw < 0:
                assert kind == RK_ASSERT
            else:
                assert kind in (RK_SOLVE_O, RK_SOLVE_L, RK_SOLVE_R) and target == sw
                side = (cc.O, cc.L, cc.Rm)[kind - RK_SOLVE_O]
                row = slice(side[0][idx], side[0][idx + 1])
                (c_unknown,) = side[2][row][side[1][row] == sw].tolist()
                assert coef & 0x3fffffff == c_unknown and coef >> 30 == unit_of[c_unknown]
                assert coef_inv == len(cc.consts) + n_solves     # inverses follow the system's table
                n_solves += 1
        at = u1
        longest, total = max(longest, len(known)), total + len(known)
    kind, _, _, _, first, mul_rows, unit_rows, _ = (int(x) for x in recs[n_instr])
    assert (kind, first, mul_rows, unit_rows) == (RK_ASSERT, at, 0, 0)
    assert terms.shape[0] == at + 3 * S and pad[at:].all()      # three rows are fetched ahead
    assert n_coeffs == len(cc.consts) + n_solves
    return total, longest


def auto_lanes(total, n_instr):
    mean = total / n_instr
    return min((1, 2, 4, 8, 16), key=lambda s: (abs(mean - s), s))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(compiled circuit, inputs [batch, n_inputs, 4] Montgomery: satisfied ones and one that is not)"""
    rng = random.Random(11)
    if name == "mixed":
        cc = compile_circuit(Mixed())
        asg = []
        for i in range(6):
            x = rng.randrange(1 << 16)
            y = x if i == 2 else rng.randrange(H.R)
            asg.append({"X": x, "Y": y, "Z": _mixed_expected(x, y)})
        asg.append(dict(asg[0], Z=(asg[0]["Z"] + 1) % H.R))      # the final assertion fails
        asg.append({"X": 5, "Y": H.R - 2, "Z": 0})               # 1 / (Y + 2): the divisor is 0
    elif name == "elgamal-add":
        cc = compile_circuit(circuits.ElGamalAddCircuit())
        pub = bjj.mul(bjj.BASE, rng.randrange(bjj.ORDER))

        def enc(m):
            k = rng.randrange(bjj.ORDER)
            return bjj.mul(bjj.BASE, k) + bjj.add(bjj.mul(bjj.BASE, m), bjj.mul(pub, k))
        asg = []
        for m in (3, 4, 5):
            a, b = enc(m), enc(m + 1)
            asg.append({"A": list(a), "B": list(b),
                        "Sum": list(bjj.add(a[:2], b[:2]) + bjj.add(a[2:], b[2:]))})
        asg.append(dict(asg[0], Sum=asg[0]["A"]))
    else:
        cc = compile_circuit(circuits.smt_inclusion_circuit(8))
        asg = [smt_witness.synthetic_inclusion(rng, 8, 1 + i % 7) for i in range(3)]
        asg.append(dict(asg[0], Root=(asg[0]["Root"] + 1) % H.R))
    return cc, np.stack([to_mont_array(cc.assignment_vector(a)) for a in asg])


@pytest.mark.parametrize("name,n_constraints", [("mixed", 31), ("elgamal-add", 16), ("smt8", 2513)])
def test_plans_solve_like_the_oracle(builds, name, n_constraints):
    cc, inputs = _case(name)
    assert cc.n_constraints == n_constraints
    lines, blob = run(builds, description(cc, inputs), 0, 64, name)
    plans = parse(blob, cc.n_wires, cc.n_constraints)
    assert [p[0] for p in plans] == [plans[0][0], *POW2]          # auto first, then 1 .. 64
    rh = cref.R1csHandle(cc)
    want = [cref.r1cs_solve(rh, x) for x in inputs]
    assert [rc != 0 for rc, *_ in want] == [False] * (len(want) - 1 - (name == "mixed")) + \
        [True] * (1 + (name == "mixed"))
    kinds_seen = set()
    for n, (S, ext, recs, terms, outs, commits, n_coeffs, sol) in enumerate(plans):
        assert ext == 0 and not commits
        total, longest = check_plan(cc, S, recs, terms, outs, n_coeffs)
        kinds_seen |= set(recs[:-1, 0].tolist())
        if n == 0:
            assert S == auto_lanes(total, cc.instr.shape[0])
        inversions = int(np.isin(recs[:-1, 0], (RK_SOLVE_L, RK_SOLVE_R, RK_INVZERO)).sum())
        assert lines[S if n else 0].startswith(
            "ok lanes=%d emul=0 instr=%d terms=%d longest=%d inversions=%d plan_terms=%d coeffs=%d "
            % (S, cc.instr.shape[0], total, longest, inversions, terms.shape[0], n_coeffs))
        for (st, w, a, b, c), (rc, w0, a0, b0, c0) in zip(sol, want):
            assert (st != 0) == (rc != 0) and st in (0, -5)
            if rc == 0:
                assert np.array_equal(w, w0) and np.array_equal(a, a0) and np.array_equal(b, b0) \
                    and np.array_equal(c, c0), (name, S)
    for S in range(1, 65):
        if S not in POW2:
            assert lines[S] == "refused: " + LANES_MSG
    if name == "mixed":     # both hint kinds, unknowns in O and in L
        assert {RK_ASSERT, RK_SOLVE_O, RK_SOLVE_L, RK_INVZERO, RK_NBITS} <= kinds_seen
    if name == "elgamal-add":
        assert RK_SOLVE_L in kinds_seen
    if name == "smt8":
        assert max(int(r[5] + r[6]) * p[0] for p in plans[:1] for r in p[2]) >= 123


def _insert_term(d, m, row, cid, wire):
    """one more term in row `row` of matrix m ('l', 'r', 'o')"""
    ptr, terms = d[m + "_ptr"], d[m + "_terms"].reshape(-1, 2)
    at = int(ptr[row + 1])
    d[m + "_terms"] = np.concatenate([terms[:at], [[cid, wire]], terms[at:]]).reshape(-1)
    ptr[row + 1:] += 1


def test_every_refusal_for_every_lane_count(builds):
    cc, inputs = _case("mixed")
    order = cc.instr.tolist()
    sw = cc.solve_wire
    cases = []

    def case(what, message, edit):
        d = description(cc, inputs[:1])
        edit(d)
        cases.append((what, message, d))

    # a constraint moved in front of the one that solves a wire it reads
    def solver_of(wire):
        return next(j for j, (k, idx) in enumerate(order) if k == 0 and sw[idx] == wire)
    i, dep, used = next(
        (i, solver_of(w), w) for i, (k, idx) in enumerate(order) if k == 0 and sw[idx] >= 0
        for w in cc.L[1][cc.L[0][idx]:cc.L[0][idx + 1]].tolist()
        if w != sw[idx] and w >= cc.n_public + cc.n_secret and (sw == w).any())
    moved = order[:dep] + [order[i]] + order[dep:i] + order[i + 1:]
    case("two unknowns", "r1cs solver: instruction %d (constraint %d): two unknown wires"
         % (dep, order[i][1]), lambda d: d.update(instr=np.array(moved, dtype=np.uint32).reshape(-1)))
    # the unknown of an O-solve once more in O, and in L
    j, k = next((j, idx) for j, (kk, idx) in enumerate(order) if kk == 0 and sw[idx] >= 0
                and sw[idx] in cc.O[1][cc.O[0][idx]:cc.O[0][idx + 1]])
    case("unknown twice in O", "r1cs solver: instruction %d (constraint %d): the unknown wire %d occurs "
         "twice in one expression" % (j, k, sw[k]), lambda d: _insert_term(d, "o", k, 0, sw[k]))
    case("unknown in L and O", "r1cs solver: instruction %d (constraint %d): the unknown wire %d occurs "
         "in more than one of L, R, O" % (j, k, sw[k]), lambda d: _insert_term(d, "l", k, 0, sw[k]))
    # a hint whose expression reads the last wire
    h = next(j for j, (kk, idx) in enumerate(order) if kk == 1)
    hi = order[h][1]
    t0 = int(cc.hint_arrays[2][cc.hint_arrays[1][hi]])

    def reads_last(d):
        d["hint_terms"][2 * t0 + 1] = cc.n_wires - 1
    case("hint reads an unsolved wire", "r1cs solver: instruction %d (hint %d): reads wire %d, which is "
         "not solved yet" % (h, hi, cc.n_wires - 1), reads_last)
    # indices out of range
    case("constraint index", "r1cs solver: instruction %d: constraint index %d out of range"
         % (j, cc.n_constraints), lambda d: d["instr"].__setitem__(2 * j + 1, cc.n_constraints))
    case("hint index", "r1cs solver: instruction %d: hint index %d out of range" % (h, len(cc.hints)),
         lambda d: d["instr"].__setitem__(2 * h + 1, len(cc.hints)))
    case("instruction kind", "r1cs solver: instruction %d: kind 2 is neither a constraint (0) nor a "
         "hint (1)" % j, lambda d: d["instr"].__setitem__(2 * j, 2))
    o0 = int(cc.hint_arrays[5][hi])
    case("hint output wire", "r1cs solver: instruction %d (hint %d): output wire %d out of range"
         % (h, hi, cc.n_wires), lambda d: d["hint_out"].__setitem__(o0, cc.n_wires))
    case("hint coefficient", "r1cs solver: instruction %d (hint %d): a term's coefficient or wire index "
         "is out of range" % (h, hi), lambda d: d["hint_terms"].__setitem__(2 * t0, len(cc.consts)))
    case("matrix wire", "r1cs solver: malformed matrix R (offsets not monotone from 0, or a term's "
         "coefficient / wire index out of range)", lambda d: d["r_terms"].__setitem__(1, cc.n_wires))
    case("hint offsets", "r1cs solver: hint table: offsets are not monotone from 0, or a null array",
         lambda d: d["hint_out_ptr"].__setitem__(1, int(d["hint_out_ptr"][-1]) + 1))
    # a wire nobody solves, a constraint twice and never
    case("unsolved wire", "r1cs solver: wire %d is still unsolved after the last instruction" % cc.n_wires,
         lambda d: d["header"].__setitem__(0, cc.n_wires + 1))
    last = len(order) - 1
    assert order[last][0] == 0 and sw[order[last][1]] < 0          # the final assertion
    case("constraint twice", "r1cs solver: instruction %d (constraint %d): the constraint occurs twice"
         % (last + 1, order[last][1]),
         lambda d: d.update(instr=np.concatenate([d["instr"], d["instr"][-2:]])))
    case("constraint never", "r1cs solver: constraint %d occurs in no instruction" % order[last][1],
         lambda d: d.update(instr=d["instr"][:-2]))
    # hint kinds out of scope, by name
    for kind, word in ((3, "limbs (kind 3)"), (4, "lookup multiplicities (kind 4)"),
                       (5, "commitment (kind 5)"), (6, "byte operation (kind 6)"),
                       (7, "emulated product (kind 7)"), (9, "of an unknown kind")):
        case("hint kind %d" % kind, "r1cs solver: instruction %d (hint %d): hints %s are not supported "
             "on this entry" % (h, hi, word), lambda d, kind=kind: d["hint_kind"].__setitem__(hi, kind))
    assert len(cases) == 20
    for n, (what, message, d) in enumerate(cases):
        lines, blob = run(builds, d, 1, 64, "refusal%d" % n)
        assert blob == b"", what
        for S in range(1, 65):
            # (the two unknowns are named behind the message)
            assert lines[S].startswith("refused: " + (message if S in POW2 else LANES_MSG)), (what, S)
