"""Host build of csrc/scs_plan.h, the solve plan of a gnark-shaped sparse system (what
zkmi_scs_solver_load builds and scs_solve_kernel runs): tests/native/scs_plan_check.cpp builds the
plan of a system for every number of sub-lanes 0 (auto), 1 .. 64, asserts the plan's two guarantees
on every step (no record reads a wire its own step writes; every wire read was written earlier or is
an input) and interprets it with ff.h.  Checked here: the wires against the Python reference
(ScsCircuit.solve_description), a hand-built system that exercises every position of the unknown,
every refusal.  The program is built plain and with -fsanitize=address,undefined; the two builds must
print the same."""
import os
import random
import shutil
import subprocess
import types

import numpy as np
import pytest

from gnark_crypto_primitives_amd import circuits
from gnark_crypto_primitives_amd.frontend.compile import to_mont_array
from gnark_crypto_primitives_amd.frontend.scs import ScsCircuit, compile_scs
from gnark_crypto_primitives_amd.tree import smt_witness
from tests import helpers as H
from tests.test_frontend import Mixed, _mixed_expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
R = H.R
NONE = 0xFFFFFFFF
POW2 = (1, 2, 4, 8, 16, 32, 64)
LANES_MSG = "scs solver: lanes_per_proof must be 0 (auto) or a power of two, 1 .. 64"


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    d = tmp_path_factory.mktemp("scs_plan")
    out = []
    for name, flags in (("plain", ["-O2"]),
                        ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined",
                                       "-fno-sanitize-recover=all"])):
        exe = str(d / ("scs_plan_check_" + name))
        subprocess.check_call(["g++", "-std=c++17", *flags, "-I",
                               os.path.join(ROOT, "gnark_crypto_primitives_amd", "csrc"),
                               os.path.join(ROOT, "tests", "native", "scs_plan_check.cpp"),
                               "-o", exe])
        out.append(exe)
    return d, out


def words(ints):
    return to_mont_array([int(v) % R for v in ints]).view(np.uint32).reshape(-1) if len(ints) else \
        np.zeros(0, np.uint32)


def dump_of(system, desc, inputs):
    """the arrays of the dump, by name, as the test may edit them"""
    xa, xb, xc, _ = system.wiring()
    ng = len(xa)
    sel = np.concatenate([words([int(v) for v in col[:ng]])
                          for col in (system.qL, system.qR, system.qO, system.qM, system.qC)])
    return {"header": np.array([desc["n_wires"], ng, system.n_public - 1, len(desc["input_wire"]),
                                len(desc["hint_kind"]), 0]),
            "xa": xa.copy(), "xb": xb.copy(), "xc": xc.copy(), "sel": sel,
            "input_wire": desc["input_wire"].copy(), "instr": desc["instr"].reshape(-1).copy(),
            "hint_kind": desc["hint_kind"].copy(), "hint_in_ptr": desc["hint_in_ptr"].copy(),
            "hint_in_wire": desc["hint_in_wire"].copy(), "hint_in_coef": words(desc["hint_in_coef"]),
            "hint_out_ptr": desc["hint_out_ptr"].copy(), "hint_out": desc["hint_out"].copy(),
            "inputs": np.concatenate([words(x) for x in inputs]) if inputs else np.zeros(0, np.uint32)}


ORDER = ("header", "xa", "xb", "xc", "sel", "input_wire", "instr", "hint_kind", "hint_in_ptr",
         "hint_in_wire", "hint_in_coef", "hint_out_ptr", "hint_out", "inputs")


def run(builds, dump, s_first, s_last, tag="case"):
    """(stdout by S, [(S, [(status, wires [n_wires, 4])])]) -- the same from both builds"""
    d, exes = builds
    src = str(d / (tag + ".in"))
    with open(src, "wb") as f:
        for name in ORDER:
            a = np.ascontiguousarray(dump[name], dtype=np.uint32)
            f.write(np.uint32(a.size).tobytes())
            f.write(a.tobytes())
    got = []
    for exe in exes:
        dst = str(d / (tag + ".out"))
        p = subprocess.run([exe, src, dst, str(s_first), str(s_last)], text=True, capture_output=True)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        got.append((p.stdout, open(dst, "rb").read()))
    assert got[0] == got[1], "the plain and the sanitized build disagree"
    lines = {}
    for line in got[0][0].splitlines():
        head, rest = line.split(" ", 1)
        lines[int(head[2:])] = rest
    assert sorted(lines) == list(range(s_first, s_last + 1))
    w = np.frombuffer(got[0][1], dtype=np.uint32)
    n_wires, plans, o = int(dump["header"][0]), [], 0
    while o < w.size:
        S, batch = int(w[o]), int(w[o + 1])
        o += 2
        sol = []
        for _ in range(batch):
            sol.append((int(w[o:o + 1].view(np.int32)[0]),
                        w[o + 1:o + 1 + 8 * n_wires].view(np.uint64).reshape(n_wires, 4)))
            o += 1 + 8 * n_wires
        plans.append((S, sol))
    return lines, plans


def every_lane_count(builds, system, desc, inputs, want_status, tag):
    """plans for lanes 0 .. 64: refused unless a power of two; every accepted plan solves every
    proof to the reference's wires and status"""
    dump = dump_of(system, desc, inputs)
    lines, plans = run(builds, dump, 0, 64, tag)
    ref = [system.solve_description(desc, x) for x in inputs]
    assert [st for _, st in ref] == want_status
    want = [to_mont_array(w) for w, _ in ref]
    assert len(plans) == 8
    for s in range(65):
        if s and s not in POW2:
            assert lines[s] == "error: " + LANES_MSG
            continue
        ok, lanes, records, steps, levels, inversions = lines[s].split()
        assert ok == "ok" and (int(lanes) == s or (s == 0 and int(lanes) in (1, 2, 4, 8, 16)))
        assert int(steps) >= int(levels) >= 1 and int(steps) * int(lanes) >= int(records)
    for S, sol in plans:
        for i, (status, wires) in enumerate(sol):
            assert status == want_status[i], (S, i)
            if want_status[i] == 0:
                assert np.array_equal(wires, want[i]), (S, i)
    return lines


def test_mixed_every_lane_count(builds):
    rng = random.Random(11)
    sc = compile_scs(Mixed())
    asg = []
    for i in range(4):
        x = rng.randrange(1 << 16)
        y = x if i == 0 else rng.randrange(R)
        asg.append({"X": x, "Y": y, "Z": _mixed_expected(x, y)})
    asg.append({"X": 5, "Y": R - 2, "Z": 0})             # 1 / (Y + 2): the divisor is 0
    inputs = [sc.assignment_vector(a) for a in asg]
    every_lane_count(builds, sc, sc.solver_description(), inputs, [0, 0, 0, 0, -5], "mixed")


def test_smt8_every_lane_count(builds):
    rng = random.Random(12)
    sc = compile_scs(circuits.smt_inclusion_circuit(8))
    inputs = [sc.assignment_vector(smt_witness.synthetic_inclusion(rng, 8, 3))]
    every_lane_count(builds, sc, sc.solver_description(), inputs, [0], "smt8")


class Hand:
    """A hand-built system: the unknown in column a alone, b alone, c alone and in all three; a DIV
    with the unknown in b and one in a without a linear part; marked (+1 / -1) and unmarked selectors
    on the unknown; a constant hint input; InvZero of zero; NBits over two records; an assertion."""
    n_public = 2          # counting ONE, as ScsCircuit does: one public input
    #        a   b   c   qL  qR  qO  qM  qC
    gates = [(0, 0, 0, 1, 0, 0, 0, 0),            # public input p = wire 0
             (2, 2, 2, 1, 0, 0, 0, -1),           # w2 = 1: all three positions, k = 1 (marked)
             (3, 1, 0, 5, 1, -1, 0, 7),           # a alone, unmarked 5 on the unknown
             (1, 4, 3, 1, -1, 2, 0, 0),           # b alone, marked -1 on the unknown
             (3, 4, 5, 0, 0, -1, 3, 0),           # c alone, behind an unmarked product
             (5, 6, 4, 2, 3, -1, 1, 0),           # DIV, unknown in b: -(2 w5 - w4) / (3 + w5)
             (7, 5, 1, 0, 0, -1, 1, 0),           # DIV, unknown in a, k = 0: w1 / w5
             (29, 7, 2, 0, 0, -1, 1, 0),          # an assertion: w29 w7 = 1
             (30, 30, 30, 1, 0, 0, 0, 0),         # w30 = 0
             (32, 32, 7, 2, 3, 1, 0, 0)]          # a and b together, qM = 0: 5 x + w7 = 0
    n_gates = len(gates)
    n_wires = 33

    def __init__(self):
        col = lambda j: np.array([g[j] % R for g in self.gates], dtype=object)
        self.qL, self.qR, self.qO, self.qM, self.qC = (col(j) for j in (3, 4, 5, 6, 7))

    def wiring(self):
        x = [np.array([g[j] for g in self.gates], dtype=np.uint32) for j in range(3)]
        return x[0], x[1], x[2], self.n_wires

    solve_description = ScsCircuit.solve_description

    def description(self):
        u32 = lambda x: np.array(x, dtype=np.uint32)
        instr = [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (1, 0), (1, 1), (1, 2), (0, 7),
                 (0, 8), (1, 3), (0, 9)]
        return {"n_wires": self.n_wires, "input_wire": u32([0, 1, NONE]), "instr": u32(instr),
                "hint_kind": u32([2, 1, 1, 1]), "hint_in_ptr": u32([0, 1, 2, 3, 4]),
                "hint_in_wire": u32([1, NONE, 7, 30]), "hint_in_coef": [3, 9, 1, 1],
                "hint_out_ptr": u32([0, 20, 21, 22, 23]),
                "hint_out": u32(list(range(8, 28)) + [28, 29, 31])}


def hand_inputs(rng):
    return [rng.randrange(R), rng.randrange(1 << 18), rng.randrange(R)]


def test_hand_built_system_every_lane_count(builds):
    rng = random.Random(13)
    hand = Hand()
    desc = hand.description()
    inputs = [hand_inputs(rng) for _ in range(3)]
    # the reference itself: spot values worked out by hand
    w, st = hand.solve_description(desc, inputs[0])
    p, s = inputs[0][0], inputs[0][1]
    inv = lambda x: pow(x, R - 2, R)
    w3 = (p - s - 7) * inv(5) % R
    w4 = (s + 2 * w3) % R
    w5 = 3 * w3 * w4 % R
    assert st == 0 and w[2] == 1 and w[3] == w3 and w[4] == w4 and w[5] == w5
    assert w[6] == (w4 - 2 * w5) * inv(3 + w5) % R and w[7] == s * inv(w5) % R
    assert w[8:28] == [(3 * s >> j) & 1 for j in range(20)] and w[28] == inv(9)
    assert w[29] == inv(w[7]) and w[30] == 0 and w[31] == 0 and w[32] == -w[7] * inv(5) % R
    every_lane_count(builds, hand, desc, inputs, [0, 0, 0], "hand")


def refusal(builds, dump, tag, lanes=4):
    lines, plans = run(builds, dump, lanes, lanes, tag)
    assert not plans
    assert lines[lanes].startswith("error: scs solver: "), lines[lanes]
    return lines[lanes][len("error: scs solver: "):]


def test_refusals(builds):
    hand = Hand()
    base = hand.description()
    inputs = [hand_inputs(random.Random(14))]

    def edited(**edit):
        d = dump_of(hand, base, inputs)
        for k, v in edit.items():
            d[k] = np.array(v, dtype=np.uint32)
        return d

    def gate_edit(g, **cols):
        """the dump with gate g's wires or selectors replaced"""
        d = dump_of(hand, base, inputs)
        for k, v in cols.items():
            if k in ("xa", "xb", "xc"):
                d[k][g] = v
            else:
                q = "LROMC".index(k[1])
                d["sel"][8 * (q * hand.n_gates + g):8 * (q * hand.n_gates + g) + 8] = words([v])
        return d

    instr = base["instr"].reshape(-1).copy()
    swap = lambda i, kind, idx: np.concatenate([instr[:2 * i], [kind, idx], instr[2 * i + 2:]])
    # two unknown wires in a gate: gate 3 (1, 4, 3) in front of gate 2, which solves wire 3
    order = instr.copy()
    order[4:8] = [0, 3, 0, 2]
    assert refusal(builds, edited(instr=order), "two") == \
        "instruction 2 (gate 3): two unknown wires (4, 3)"
    # the unknown in both a and b with qM != 0
    assert refusal(builds, gate_edit(9, qM=1), "both") == \
        "instruction 13 (gate 9): the unknown wire 32 is both factors of the product (qM != 0)"
    # k = 0
    assert refusal(builds, gate_edit(9, qL=2, qR=R - 2), "kzero") == \
        "instruction 13 (gate 9): the unknown wire 32 has coefficient 0"
    # a hint that reads an unsolved wire / writes a solved one
    assert refusal(builds, edited(hint_in_wire=[1, NONE, 32, 30]), "unsolved") == \
        "instruction 9 (hint 2): reads wire 32, which is not solved yet"
    assert refusal(builds, edited(hint_out=list(range(8, 28)) + [28, 3, 31]), "solved") == \
        "instruction 9 (hint 2): output wire 3 is already solved"
    # wrong operand or output counts for kinds 1 and 2
    assert refusal(builds, edited(hint_out_ptr=[0, 19, 21, 22, 23]), "counts1") == \
        "instruction 8 (hint 1): InvZero takes one input and has one output"
    assert refusal(builds, edited(hint_in_ptr=[0, 2, 2, 3, 4]), "counts2") == \
        "instruction 7 (hint 0): NBits takes one input and has outputs"
    # kinds 3 .. 7 by name, and an unknown kind
    names = {3: "limbs (kind 3)", 4: "lookup multiplicities (kind 4)", 5: "commitment (kind 5)",
             6: "byte operation (kind 6)", 7: "emulated product (kind 7)"}
    for kind, name in names.items():
        assert refusal(builds, edited(hint_kind=[2, kind, 1, 1]), "kind%d" % kind) == \
            "instruction 8 (hint 1): hints %s are not supported on this entry" % name
    assert refusal(builds, edited(hint_kind=[2, 9, 1, 1]), "kind9") == \
        "instruction 8 (hint 1): hints of an unknown kind (9) are not supported on this entry"
    # indices out of range
    assert refusal(builds, edited(instr=swap(13, 0, 10)), "gate_range") == \
        "instruction 13: gate index 10 out of range"
    assert refusal(builds, edited(instr=swap(12, 1, 4)), "hint_range") == \
        "instruction 12: hint index 4 out of range"
    assert refusal(builds, edited(instr=swap(12, 2, 0)), "instr_kind") == \
        "instruction 12: kind 2 is neither a gate (0) nor a hint (1)"
    assert refusal(builds, edited(hint_in_wire=[1, NONE, 33, 30]), "in_range") == \
        "instruction 9 (hint 2): input wire 33 out of range"
    assert refusal(builds, edited(hint_out=list(range(8, 28)) + [28, 29, 33]), "out_range") == \
        "instruction 12 (hint 3): output wire 33 out of range"
    assert refusal(builds, gate_edit(4, xb=33), "wire_range") == \
        "xb[4] = 33 is not a wire (n_wires = 33)"
    assert refusal(builds, edited(input_wire=[0, 40, NONE]), "input_range") == \
        "input_wire[1] = 40 is not a wire"
    # a gate that occurs twice or never
    assert refusal(builds, edited(instr=swap(10, 0, 6)), "twice") == \
        "instruction 10 (gate 6): the gate occurs twice"
    assert refusal(builds, edited(instr=instr[:20].tolist() + instr[22:].tolist()), "never") == \
        "gate 7 occurs in no instruction"
    # a wire still unsolved at the end
    assert refusal(builds, edited(header=[34, hand.n_gates, 1, 3, 4, 0]), "left") == \
        "wire 33 is still unsolved after the last instruction"
    # lanes_per_proof, hint_set
    assert "scs solver: " + refusal(builds, edited(), "lanes", lanes=3) == LANES_MSG
    assert refusal(builds, edited(header=[33, hand.n_gates, 1, 3, 4, 1]), "hint_set") == \
        "hint_set must be ZKMI_HINTS_BASIC (0): this entry solves InvZero and NBits hints only"
    # input_wire entries that repeat; n_inputs inconsistent with n_public
    assert refusal(builds, edited(input_wire=[0, 1, 1]), "repeat") == \
        "input_wire[2] = 1 repeats an earlier entry"
    assert refusal(builds, edited(header=[33, hand.n_gates, 4, 3, 4, 0]), "n_public") == \
        "n_inputs = 3 is inconsistent with the system's n_public = 4 (the public inputs come first)"
    assert refusal(builds, edited(input_wire=[1, 0, NONE]), "public_wire") == \
        "input_wire[0] = 1 is not the wire of public gate 0, 0"
    # the unedited description is accepted
    lines, plans = run(builds, edited(), 4, 4, "accepted")
    assert lines[4].startswith("ok 4 ") and len(plans) == 1
