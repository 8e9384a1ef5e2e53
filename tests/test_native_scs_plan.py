"""Host build of csrc/scs_plan.h, the solve plan of a gnark-shaped sparse system (what
zkmi_scs_solver_load builds and scs_solve_kernel runs): tests/native/scs_plan_check.cpp builds the
plan of a system for every number of sub-lanes 0 (auto), 1 .. 64, asserts the plan's two guarantees
on every step (no record reads a wire its own step writes; every wire read was written earlier or is
an input) and interprets it with ff.h.  Checked here: the wires against the Python reference
(ScsCircuit.solve_description), a hand-built system that exercises every position of the unknown,
every refusal.  The program is built plain and with -fsanitize=address,undefined; the two builds must
print the same."""
import random

import numpy as np

from gnark_crypto_primitives_amd import circuits
from gnark_crypto_primitives_amd.frontend.compile import to_mont_array
from gnark_crypto_primitives_amd.frontend.scs import compile_scs
from gnark_crypto_primitives_amd.tree import smt_witness
from tests.native_build import needs_gxx
from tests.scs_plan_harness import LANES_MSG, NONE, POW2, R, Hand, dump_of, hand_inputs, refusal, run, words
from tests.scs_plan_harness import builds  # noqa: F401 (a fixture)
from tests.test_frontend import Mixed, _mixed_expected

pytestmark = needs_gxx


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
        ok, lanes, records, steps, levels, inversions, std, _ = lines[s].split()
        assert ok == "ok" and std == "0" and (int(lanes) == s or (s == 0 and int(lanes) in (1, 2, 4, 8, 16)))
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
