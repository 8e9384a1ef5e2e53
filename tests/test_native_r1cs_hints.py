"""Host build of csrc/r1cs_plan.h for the hints of ZKMI_HINTS_STD (limbs, lookup multiplicities, byte
operations, commitments): tests/native/r1cs_plan_check.cpp plans a system dumped from compile_circuit
for every number of sub-lanes 0 (auto), 1 .. 64 and interprets the plan on the host, sub-lane by
sub-lane as r1cs_solve_kernel<S, true> does.  Checked here: wires, a, b, c against the oracle's
gnark-style solver (cref.r1cs_solve, cref.r1cs_solve_ex -- at a commitment the interpreter is handed
the oracle's value of the commitment wire, nothing is hashed); the commitment list against the
frontend's; hand-edited descriptions the frontend cannot emit against Python integers; every refusal.
The program is built plain and with -fsanitize=undefined,address; the two builds must agree byte for
byte."""
import functools
import random

import numpy as np
import pytest

from gnark_crypto_primitives_amd import groth16
from gnark_crypto_primitives_amd.frontend import compile_circuit
from gnark_crypto_primitives_amd.frontend.compile import from_mont_array, to_mont_array
from oracle import cref
from tests import helpers as H
from tests.native_build import needs_gxx
from tests.r1cs_plan_harness import (BASIC, K_BYTEOP, K_COMMIT, K_COUNT, K_LIMBS, LANES_MSG, POW2, RK_COMMIT,
                                     RK_COUNT_BEGIN, RK_COUNT_END, RK_COUNT_Q, RK_LIMBS, STD, HintsPlain,
                                     coefficient, description, hint_list, hints_plain_assignments, limbs_of,
                                     parse, run)
from tests.r1cs_plan_harness import builds  # noqa: F401 (a fixture)
from tests.test_commitment import RangeCircuit, TwoCommitments, _mul

pytestmark = needs_gxx


@functools.lru_cache(maxsize=None)
def _case(name):
    """(compiled circuit, inputs [batch, n_inputs, 4], the oracle's solve of each: rc, wires, a, b, c)"""
    rng = random.Random(23)
    if name == "plain":
        cc = compile_circuit(HintsPlain())
        asg = hints_plain_assignments(9, rng)
    elif name == "range":
        cc = compile_circuit(RangeCircuit())
        asg = [{"X": 0x11 * 0x22, "Y": 0x1122334455662211}, {"X": 0x11 * 0x22 + 1, "Y": 0x2211},
               {"X": 0x11 * 0x22, "Y": 0x2211 + (1 << 64)}, {"X": 8184, "Y": 0x21f8},
               {"X": 8190, "Y": 0x2ac3}]
    else:
        cc = compile_circuit(TwoCommitments())
        asg = [{"X": y * y, "Y": y} for y in (7, 1 << 100, H.R - 3)] + [{"X": 50, "Y": 7}]
        asg[1]["X"] %= H.R
        asg[2]["X"] %= H.R
    inputs = np.stack([to_mont_array(cc.assignment_vector(a)) for a in asg])
    if cc.commitments:
        pk, _, _ = groth16.setup(cc, 9, _mul)
        rh, ch = cref.R1csHandle(cc), cref.CommitKeysHandle(pk)
        want = [cref.r1cs_solve_ex(rh, ch, x)[:5] for x in inputs]
    else:
        rh = cref.R1csHandle(cc)
        want = [cref.r1cs_solve(rh, x) for x in inputs]
    return cc, inputs, want


@pytest.mark.parametrize("name,shape,n_bad", [("plain", (105, 7), 1), ("range", (87, 63), 3),
                                              ("two", None, 1)])
def test_std_plans_solve_like_the_oracle(builds, name, shape, n_bad):
    cc, inputs, want = _case(name)
    hints = hint_list(cc)
    if shape:
        assert (cc.n_wires, cc.instr.shape[0]) == shape
    if name == "plain":
        assert sorted(h[0] for h in hints) == [K_LIMBS, K_LIMBS, K_COUNT, K_BYTEOP, K_BYTEOP]
        assert [len(e) for e in hints[2][1][1:]] == [1] * 51 + [2, 2]
    if name == "range":     # one commitment over 37 wires at instruction 24
        assert cc.instr[24].tolist() == [1, next(i for i, h in enumerate(hints) if h[0] == K_COMMIT)]
        assert len(cc.commitments) == 1 and len(cc.commitments[0]["private"]) == 37
    if name == "two":       # the second commitment hashes the first one's wire
        assert cc.commitments[0]["wire"] in cc.commitments[1]["hashed"]
    assert sum(1 for rc, *_ in want if rc != 0) == n_bad
    cwires = [c["wire"] for c in cc.commitments]
    cvals = [[w[x] for x in cwires] for rc, w, *_ in want]
    lines, blob = run(builds, description(cc, inputs, commit_values=cvals), 0, 64, name)
    plans = parse(blob, cc.n_wires, cc.n_constraints)
    assert [p[0] for p in plans[1:]] == list(POW2) and plans[0][0] in (1, 2, 4, 8, 16)
    n_queries = [len(h[1]) - 1 for h in hints if h[0] == K_COUNT]
    for S, ext, recs, terms, outs, commits, n_coeffs, sol in plans:
        assert ext == 1
        kinds = recs[:-1, 0]
        assert int((kinds == RK_COUNT_Q).sum()) == sum(-(-n // S) for n in n_queries)
        assert int((kinds == RK_COUNT_BEGIN).sum()) == int((kinds == RK_COUNT_END).sum()) == len(n_queries)
        assert recs.shape[0] - 1 == cc.instr.shape[0] + int((kinds == RK_COUNT_Q).sum()) + len(n_queries)
        assert terms.shape[0] == int(recs[-1, 4]) + 3 * S
        # hints emit no a / b / c row; a commitment is a record without terms, at the place the plan says
        assert [(i, w, h, p) for i, _, w, h, p in commits] == \
            [(int(np.nonzero((cc.instr[:, 0] == 1) & (np.array([hints[j][0] if k == 1 else 0 for k, j in
                                                                 cc.instr.tolist()]) == K_COMMIT))[0][n]),
              c["wire"], list(c["hashed"]), list(c["private"])) for n, c in enumerate(cc.commitments)]
        for n, (_, rec, wire, _, _) in enumerate(commits):
            assert recs[rec].tolist()[:2] == [RK_COMMIT, wire] and recs[rec, 5] == recs[rec, 6] == 0
            assert recs[rec, 7] == n
        for i, ((st, w, a, b, c), (rc, w0, a0, b0, c0)) in enumerate(zip(sol, want)):
            assert (st != 0) == (rc != 0) and st in (0, -5), (name, S, i)
            if rc == 0:
                assert np.array_equal(w, w0), (name, S, i)
                assert np.array_equal(a, a0) and np.array_equal(b, b0) and np.array_equal(c, c0), (name, S, i)
    for S in range(1, 65):
        if S not in POW2:
            assert lines[S] == "refused: " + LANES_MSG


def test_a_plan_without_the_new_kinds_is_not_ext(builds):
    from tests.test_frontend import Mixed
    cc = compile_circuit(Mixed())
    inputs = np.zeros((0, cc.n_inputs, 4), np.uint64)
    blobs = [run(builds, description(cc, inputs, hint_set=hs), 0, 4, "mixed%d" % hs)[1] for hs in (BASIC, STD)]
    assert blobs[0] == blobs[1]
    assert [p[1] for p in parse(blobs[0], cc.n_wires, cc.n_constraints)] == [0] * 4


@pytest.mark.parametrize("width", [64, 37])
def test_wide_limbs_past_bit_256_against_python_integers(builds, width):
    """16 limbs of 64 (37) bits of Z: more than 256 bits, limbs that straddle three 32-bit words --
    widths the frontend does not emit"""
    cc, inputs, _ = _case("plain")
    hints = hint_list(cc)
    d0 = description(cc, inputs)
    cid = coefficient(d0, width)
    h = next(i for i, x in enumerate(hints) if x[0] == K_LIMBS and len(x[2]) == 16)
    assert hints[h][1][0] == [(hints[h][1][0][0][0], 0)] and cc.consts[hints[h][1][0][0][0]] == 16
    hints[h][1][0] = [(cid, 0)]
    d = description(cc, inputs, hints=hints)
    d["coeffs"] = d0["coeffs"]
    lines, blob = run(builds, d, 0, 64, "wide%d" % width)
    zs = [from_mont_array(x[None, cc.n_public - 1 + 1])[0] for x in inputs]      # Z: the second secret
    assert zs[0] == H.R - 1
    for S, ext, recs, terms, outs, commits, n_coeffs, sol in parse(blob, cc.n_wires, cc.n_constraints):
        rec = next(r for r in recs if r[0] == RK_LIMBS and r[7] == 16)
        assert rec[2] == width
        for z, (st, w, *_rest) in zip(zs, sol):
            got = from_mont_array(w[outs[rec[1]:rec[1] + 16]])
            assert got == limbs_of(z, width, 16), (S, width)
            assert got[256 // width + 1:] == [0] * (15 - 256 // width)


def test_count_steps_with_unequal_queries_against_python_integers(builds):
    """query j of the lookup hint gets j % 3 more terms: at every S > 1 the queries of a step differ
    in length (rows padded per sub-lane), and at S = 1 the steps do"""
    cc, inputs, _ = _case("plain")
    hints = hint_list(cc)
    h = next(i for i, x in enumerate(hints) if x[0] == K_COUNT)
    lw = next(x for x in hints if x[0] == K_LIMBS and len(x[2]) == 51)[2]        # the wires of l
    d0 = description(cc, inputs)
    one, three = coefficient(d0, 1), coefficient(d0, H.R - 3)
    queries = []
    for j in range(53):
        # l[j % 51] + l[j + 1] - 3 l[j + 2], the last j % 3 of the three terms dropped from the end
        full = [(one, lw[j % 51]), (one, lw[(j + 1) % 51]), (three, lw[(j + 2) % 51])]
        queries.append(full[:1 + j % 3])
    hints[h][1] = hints[h][1][:1] + queries
    d = description(cc, inputs, hints=hints)
    d["coeffs"] = d0["coeffs"]
    lines, blob = run(builds, d, 0, 64, "ragged")
    ys = [from_mont_array(x[None, cc.n_public - 1])[0] for x in inputs]
    for S, ext, recs, terms, outs, commits, n_coeffs, sol in parse(blob, cc.n_wires, cc.n_constraints):
        steps = [r for r in recs if r[0] == RK_COUNT_Q]
        assert [int(r[7]) for r in steps] == [min(S, 53 - q) for q in range(0, 53, S)]
        assert [int(r[5]) for r in steps] == [max(1 + j % 3 for j in range(q, min(q + S, 53)))
                                              for q in range(0, 53, S)]
        if S > 1:       # both padded and full columns in a step
            first = terms[steps[0][4]:steps[0][4] + steps[0][5] * S, 0].reshape(-1, S) >> 30
            assert (first[-1] == 3).any() and (first[-1] != 3).any()
        begin = next(r for r in recs if r[0] == RK_COUNT_BEGIN)
        for y, (st, w, *_rest) in zip(ys, sol):
            l = limbs_of(y, 5, 51)
            q = [(l[j % 51] + (l[(j + 1) % 51] if j % 3 else 0) - (3 * l[(j + 2) % 51] if j % 3 == 2 else 0))
                 % H.R for j in range(53)]
            assert any(v >= 32 for v in q)
            want = [sum(1 for v in q if v == t) for t in range(32)]
            assert from_mont_array(w[outs[begin[1]:begin[1] + 32]]) == want, S


def test_every_refusal_for_every_lane_count(builds):
    cc, inputs, _ = _case("plain")
    rcc, rinputs, _ = _case("range")
    order = cc.instr.tolist()
    base = hint_list(cc)
    at = {}         # hint kind -> (instruction, hint index) of its first occurrence
    for i, (k, idx) in enumerate(order):
        if k == 1:
            at.setdefault(base[idx][0], (i, idx))
    rbase = hint_list(rcc)
    rat = next((i, idx) for i, (k, idx) in enumerate(rcc.instr.tolist()) if k == 1 and rbase[idx][0] == K_COMMIT)
    cases = []

    def case(what, kind, message, edit, hint_set=STD, range_circuit=False):
        c, inp, hs = (rcc, rinputs, rbase) if range_circuit else (cc, inputs, base)
        hints = [[k, [list(e) for e in ex], list(o)] for k, ex, o in hs]
        i, idx = rat if range_circuit else at[kind]
        d0 = description(c, inp[:1], hint_set)
        edit(hints[idx], d0)
        d = description(c, inp[:1], hint_set, hints=hints, commit_values=[[[0] * 4]] * len(c.commitments))
        d["coeffs"] = d0["coeffs"]
        cases.append((what, "r1cs solver: instruction %d (hint %d): %s" % (i, idx, message), d))

    def param(value):
        return lambda h, d: h[1].__setitem__(0, [(coefficient(d, value), 0)])
    limbs, count, byteop, commit = ("limbs (kind 3)", "lookup multiplicities (kind 4)",
                                    "byte operation (kind 6)", "commitment (kind 5)")
    # operand and output counts
    case("limbs: two values", K_LIMBS, limbs + " takes a width and one input and has outputs",
         lambda h, d: h[1].append(h[1][1]))
    case("limbs: no output", K_LIMBS, limbs + " takes a width and one input and has outputs",
         lambda h, d: h[2].clear())
    case("count: no query", K_COUNT, count + " takes a table size and queries and has outputs",
         lambda h, d: h[1].__delitem__(slice(1, None)))
    case("byteop: one value", K_BYTEOP, byteop + " takes an operation and two inputs and has one output",
         lambda h, d: h[1].pop())
    case("byteop: two outputs", K_BYTEOP, byteop + " takes an operation and two inputs and has one output",
         lambda h, d: h[2].append(cc.n_wires - 1))
    case("commit: two outputs", K_COMMIT, commit + " takes the number of hashed operands and the operands "
         "and has one output", lambda h, d: h[2].append(rcc.n_wires - 1), range_circuit=True)
    # parameters
    case("width 0", K_LIMBS, "limb width 0 is outside 1 .. 64", param(0))
    case("width 65", K_LIMBS, "limb width 65 is outside 1 .. 64", param(65))
    case("table size 31", K_COUNT, "table size 31 is not the number of outputs, 32", param(31))
    case("table size 0", K_COUNT, "table size 0 is not the number of outputs, 32", param(0))
    case("byte operation 3", K_BYTEOP, "byte operation 3 is neither 1 (XOR) nor 2 (AND)", param(3))
    case("hashed operands", K_COMMIT, "38 hashed operands among 37", param(38), range_circuit=True)
    for kind, name in ((K_LIMBS, limbs), (K_COUNT, count), (K_BYTEOP, byteop)):
        case("parameter on a wire", kind, "the parameter of %s is not a constant (it reads wire 1)" % name,
             lambda h, d: h[1][0].append((0, 1)))
    case("parameter on a wire", K_COMMIT, "the parameter of %s is not a constant (it reads wire 1)" % commit,
         lambda h, d: h[1][0].append((0, 1)), range_circuit=True)
    # commitment operands are wires
    case("commit: an expression", K_COMMIT, "commitment operand 3 is not a single wire with coefficient 1",
         lambda h, d: h[1][4].append((0, 0)), range_circuit=True)
    case("commit: coefficient 2", K_COMMIT, "commitment operand 0 is not a single wire with coefficient 1",
         lambda h, d: h[1].__setitem__(1, [(coefficient(d, 2), h[1][1][0][1])]), range_circuit=True)
    # the checks every hint gets
    case("limbs read an unsolved wire", K_LIMBS, "reads wire %d, which is not solved yet" % (cc.n_wires - 1),
         lambda h, d: h[1][1].append((0, cc.n_wires - 1)))
    case("count output solved", K_COUNT, "output wire 1 is already solved", lambda h, d: h[2].__setitem__(3, 1))
    case("byteop output range", K_BYTEOP, "output wire %d out of range" % cc.n_wires,
         lambda h, d: h[2].__setitem__(0, cc.n_wires))
    case("commit reads an unsolved wire", K_COMMIT, "reads wire %d, which is not solved yet" % (rcc.n_wires - 1),
         lambda h, d: h[1].__setitem__(1, [(h[1][1][0][0], rcc.n_wires - 1)]), range_circuit=True)
    # kinds out of scope, by name: 7 and unknown ones under STD, 3 .. 6 under BASIC with today's wording
    # (the first hint of the system takes the kind: nothing in front of it is refused under BASIC)
    assert at[K_LIMBS][0] == 0
    for kind, word, hs in ((7, "emulated product (kind 7)", STD), (9, "of an unknown kind", STD),
                           (K_LIMBS, limbs, BASIC), (K_COUNT, count, BASIC), (K_COMMIT, commit, BASIC),
                           (K_BYTEOP, byteop, BASIC)):
        case("kind %d, set %d" % (kind, hs), K_LIMBS, "hints %s are not supported on this entry" % word,
             lambda h, d, kind=kind: h.__setitem__(0, kind), hint_set=hs)
    d = description(cc, inputs[:1], 2)
    cases.append(("hint set 2", "r1cs solver: hint_set must be ZKMI_HINTS_BASIC (0) or ZKMI_HINTS_STD (1)", d))
    assert len(cases) == 29
    for n, (what, message, d) in enumerate(cases):
        lines, blob = run(builds, d, 0, 64, "refusal%d" % n)
        assert blob == b"", what
        for S in range(0, 65):
            assert lines[S] == "refused: " + (message if S in (0,) + POW2 else LANES_MSG), (what, S)
