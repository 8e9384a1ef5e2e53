"""What the tests of the gnark-shaped sparse-system solve share (a plain module, no test in it): the
dump that tests/native/scs_plan_check.cpp reads and the OUT it writes, the program's two builds, and
the hand-written systems that the host tests and the GPU tests both solve."""
import numpy as np
import pytest

from gnark_crypto_primitives_amd.frontend.compile import to_mont_array
from gnark_crypto_primitives_amd.frontend.scs import ScsCircuit
from tests import helpers as H
from tests import native_build
from tests.r1cs_plan_harness import lines_by_s, write_sections

R = H.R
NONE = 0xFFFFFFFF
BASIC, STD = 0, 1
POW2 = (1, 2, 4, 8, 16, 32, 64)
LANES_MSG = "scs solver: lanes_per_proof must be 0 (auto) or a power of two, 1 .. 64"


# ---- the check program: its builds, its dump, its answer ------------------------------------------

@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    """(directory for the dumps, [plain, sanitized]): built once, whichever modules ask"""
    return native_build.build_once("scs_plan_check.cpp", tmp_path_factory)


def words(ints):
    return to_mont_array([int(v) % R for v in ints]).view(np.uint32).reshape(-1) if len(ints) else \
        np.zeros(0, np.uint32)


def dump_of(system, desc, inputs, hint_set=BASIC, max_set=BASIC):
    """the arrays of the dump, by name, as the test may edit them; max_set, the highest hint set the
    builder may accept, goes to the program's command line"""
    xa, xb, xc, _ = system.wiring()
    ng = len(xa)
    sel = np.concatenate([words([int(v) for v in col[:ng]])
                          for col in (system.qL, system.qR, system.qO, system.qM, system.qC)])
    return {"header": np.array([desc["n_wires"], ng, system.n_public - 1, len(desc["input_wire"]),
                                len(desc["hint_kind"]), hint_set]),
            "xa": xa.copy(), "xb": xb.copy(), "xc": xc.copy(), "sel": sel,
            "input_wire": desc["input_wire"].copy(), "instr": desc["instr"].reshape(-1).copy(),
            "hint_kind": desc["hint_kind"].copy(), "hint_in_ptr": desc["hint_in_ptr"].copy(),
            "hint_in_wire": desc["hint_in_wire"].copy(), "hint_in_coef": words(desc["hint_in_coef"]),
            "hint_out_ptr": desc["hint_out_ptr"].copy(), "hint_out": desc["hint_out"].copy(),
            "inputs": np.concatenate([words(x) for x in inputs]) if inputs else np.zeros(0, np.uint32),
            "skip_rows": np.array(system.skip_rows() if hasattr(system, "skip_rows") else [], dtype=np.uint32),
            "max_set": max_set}


ORDER = ("header", "xa", "xb", "xc", "sel", "input_wire", "instr", "hint_kind", "hint_in_ptr",
         "hint_in_wire", "hint_in_coef", "hint_out_ptr", "hint_out", "inputs", "skip_rows")


def run(builds, dump, s_first, s_last, tag="case"):
    """(stdout by S, [(S, [(status, wires [n_wires, 4])])]) -- the same from both builds"""
    d, exes = builds
    src, dst = str(d / (tag + ".in")), str(d / (tag + ".out"))
    write_sections(src, dump, ORDER)
    _, text, blob = native_build.run_both(
        exes, [src, dst, str(s_first), str(s_last), str(dump["max_set"])], out_file=dst)
    w = np.frombuffer(blob, dtype=np.uint32)
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
    return lines_by_s(text, s_first, s_last), plans


def refusal(builds, dump, tag, lanes=4):
    lines, plans = run(builds, dump, lanes, lanes, tag)
    assert not plans
    assert lines[lanes].startswith("error: scs solver: "), lines[lanes]
    return lines[lanes][len("error: scs solver: "):]


# ---- Hand: the basic hints -------------------------------------------------------------------------

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


# ---- HandStd: the hints of ZKMI_HINTS_STD ----------------------------------------------------------

class HandStd:
    """A hand-written system for the hints of ZKMI_HINTS_STD.  Inputs: the public p (wire 0), s
    (wire 1), t (wire 2) and one that no gate reads.
      limbs      width 8 of s, 5 outputs; width 64 of 3 t, 5 outputs (the last one lies past bit 256)
      counts     a table of 17 (one chunk of 16 and 1) with 7 queries -- limbs (mostly >= 17: they
                 count nowhere), the constant 5, 2 * ONE, ONE --; a table of 5 on the same levels
                 with a query >= its size; a table of 2 with no query
      byte ops   XOR of s and 5 t (field elements: bits above 32 set), AND of a 64-bit limb and a
                 48-bit constant
      commitments (``commits=True``): 0 over inputs only (its first range of steps is empty), 1 over
                 the first one's wire and a wire deep in the solve, 2 over the last wire solved
                 (nothing depends on it: the last range is empty)"""
    n_public = 2          # counting ONE
    BASE = [(0, 0, 0, 1, 0, 0, 0, 0),               # public input p = wire 0
            (3, 3, 3, 1, 0, 0, 0, -1),              # ONE = wire 3
            (38, 39, 40, 1, 1, -1, 0, 0),           # w40 = xor + and
            (40, 14, 41, 0, 0, -1, 1, 0)]           # w41 = w40 * (count of 0 in the table of 17)
    COMMIT = [(1, 1, 1, -1, 0, 0, 0, 0), (2, 2, 2, -1, 0, 0, 0, 0),      # rows 4, 5: C_0
              (42, 42, 42, -1, 0, 0, 0, 0),                              # row 6: r_0, wire 42
              (42, 42, 42, -1, 0, 0, 0, 0), (41, 41, 41, -1, 0, 0, 0, 0),  # rows 7, 8: C_1
              (43, 43, 43, -1, 0, 0, 0, 0),                              # row 9: r_1, wire 43
              (43, 42, 44, 1, 1, -1, 0, 0),                              # row 10: w44 = w43 + w42
              (44, 44, 44, -1, 0, 0, 0, 0),                              # row 11: C_2
              (45, 45, 45, -1, 0, 0, 0, 0)]                              # row 12: r_2, wire 45

    def __init__(self, commits=True):
        self.with_commits = commits
        self.gates = self.BASE + (self.COMMIT if commits else [])
        self.n_gates = len(self.gates)
        self.n_wires = 46 if commits else 42
        self.commitments = [{"rows": [4, 5], "row": 6}, {"rows": [7, 8], "row": 9},
                            {"rows": [11], "row": 12}] if commits else []
        col = lambda j: np.array([g[j] % R for g in self.gates], dtype=object)
        self.qL, self.qR, self.qO, self.qM, self.qC = (col(j) for j in (3, 4, 5, 6, 7))
        # (kind, [(wire | NONE, coefficient)], outputs)
        self.hints = [
            (3, [(NONE, 8), (1, 1)], list(range(4, 9))),
            (3, [(NONE, 64), (2, 3)], list(range(9, 14))),
            (4, [(NONE, 17), (4, 1), (5, 1), (6, 1), (NONE, 5), (3, 2), (3, 1), (8, 1)], list(range(14, 31))),
            (4, [(NONE, 5), (3, 1), (3, 1), (NONE, 7), (3, 4)], list(range(31, 36))),
            (4, [(NONE, 2)], [36, 37]),
            (6, [(NONE, 1), (1, 1), (2, 5)], [38]),
            (6, [(NONE, 2), (9, 1), (NONE, 0xFFFF0000FFFF)], [39])]
        self.instr = [(0, 0), (0, 1)] + [(1, h) for h in range(7)] + [(0, 2), (0, 3)]
        if commits:
            self.hints += [(5, [(NONE, 0), (1, 1), (2, 1)], [42]), (5, [(NONE, 1), (42, 1), (41, 1)], [43]),
                           (5, [(NONE, 2), (44, 1)], [45])]
            self.instr += [(0, 4), (0, 5), (1, 7), (0, 6), (0, 7), (0, 8), (1, 8), (0, 9), (0, 10), (0, 11),
                           (1, 9), (0, 12)]

    def wiring(self):
        x = [np.array([g[j] for g in self.gates], dtype=np.uint32) for j in range(3)]
        return x[0], x[1], x[2], self.n_wires

    solve_description = ScsCircuit.solve_description

    def description(self, hints=None, instr=None, n_wires=None):
        hints = self.hints if hints is None else hints
        u32 = lambda x: np.array(x, dtype=np.uint32)
        in_ptr, out_ptr = [0], [0]
        for _, ins, outs in hints:
            in_ptr.append(in_ptr[-1] + len(ins))
            out_ptr.append(out_ptr[-1] + len(outs))
        return {"hint_set": 1, "n_wires": self.n_wires if n_wires is None else n_wires,
                "input_wire": u32([0, 1, 2, NONE]),
                "instr": u32(self.instr if instr is None else instr).reshape(-1, 2),
                "hint_kind": u32([k for k, _, _ in hints]), "hint_in_ptr": u32(in_ptr),
                "hint_in_wire": u32([w for _, ins, _ in hints for w, _ in ins]),
                "hint_in_coef": [c for _, ins, _ in hints for _, c in ins],
                "hint_out_ptr": u32(out_ptr), "hint_out": u32([o for _, _, outs in hints for o in outs])}

    def skip_rows(self):
        return [r for c in self.commitments for r in c["rows"] + [c["row"]]]


def stand_in(i, vals):
    """the challenge scs_plan_check.cpp gives commitment i"""
    return (1 + i + sum((j + 1) * v for j, v in enumerate(vals))) % R


def std_inputs(rng):
    return [rng.randrange(R), rng.randrange(R), rng.randrange(R), rng.randrange(R)]
