"""PLONK arithmetisation ("sparse constraint system") of a compiled circuit.

gnark compiles a circuit for PLONK with ``frontend.Compile(field, scs.NewBuilder, circuit)``
(third-party module, go.mod:8) [UPSTREAM-RECALL]: every constraint is one gate
    qL.a + qR.b + qO.c + qM.a.b + qC (+ PI) = 0
over three wire columns, plus copy constraints tying equal wires together.  BASELINE config 5 names
that backend; the reference's own test of the circuit uses Groth16 over R1CS
(ecc/secp256k1/ecdsa/address_test.go:40,57), so nothing in the reference pins a PLONK result:
parity unpinned.

This module lowers the SSA witness program the R1CS frontend records (frontend/api.py: one field
operation per API call, dead code eliminated) to gates, one per operation, the SSA values being the
PLONK wires:

    d = a + b      ->  (a, b, d)  qL = 1, qR = 1, qO = -1        d = a * b   ->  qM = 1, qO = -1
    d = a - b      ->  qL = 1, qR = -1, qO = -1                 d = k a     ->  (a, a, d) qL = k, qO = -1
    d = a + k      ->  (a, a, d) qL = 1, qC = k, qO = -1         d = -a      ->  qL = 1, qO = 1
    d = a xor b    ->  qL = 1, qR = 1, qM = -2, qO = -1          d = k       ->  (d, d, d) qO = -1, qC = k
    R1CS row (L, R, O) kept as a row (assertions, hint-defining rows): (vL, vR, vO) qM = 1, qO = -1
    public input x_j: (v_j, v_j, v_j) qL = 1, PI_j = -x_j;  ONE wire: qL = 1, qC = -1

Hints (inverse-or-zero, bit decomposition, unchecked division, the batched inversion) get no gate:
as in the R1CS, the rows that use their outputs constrain them.  The witness program of the system
is the same program with an OP_ABC row per gate, so the GPU solver (csrc/solve.hip) emits the
three wire columns a, b, c directly.

api.Commit (gnark's scs builder, BSB22 [UPSTREAM-RECALL]; parity unpinned) is carried by one more
selector column per commitment, Qcp_i, and the gate equation becomes
    qL a + qR b + qO c + qM a b + qC + PI' + sum_i Qcp_i pi2_i = 0,   PI'_(r_i) = +H_i.
Every operand w of commitment i (private, public or an earlier commitment wire, in operand order)
gets a committed row (w, w, w) with qL = -1 and Qcp_i = 1, so pi2_i = a there; the commitment wire
h_i gets the commitment row r_i: (h_i, h_i, h_i) with qL = -1, where the prover's
H_i = hash_to_field([pi2_i]) enters as a public-input term.  The OP_COMMIT unit stays in the witness
program as it is for the R1CS (the solver stops there and the prover supplies the challenge); the
lookup multiplicities (OP_HIST), the emulated products (OP_EMUL) and the byte hints lower as hints.
"""
from __future__ import annotations

import numpy as np

import hashlib

from .api import (OP_ABC, OP_ADD, OP_ADDC, OP_BAND, OP_BATCHINV, OP_BITS, OP_BXOR, OP_COMMIT, OP_COPY,
                  OP_DIV, OP_EMUL, OP_HIST, OP_HQ, OP_INV, OP_MUL, OP_MULABC, OP_MULC, OP_NEG, OP_PAIR,
                  OP_SETC, OP_SUB, OP_XOR, OP_XORABC, R)
from .compile import CompiledCircuit, build_vprogram

COSET_SHIFT = 5          # fr.MultiplicativeGen: the columns' identity permutation is X, 5X, 25X


class ScsCircuit:
    """Selectors, wiring and witness program of one circuit (gnark: constraint.SparseR1CS)."""

    def __init__(self, cc: CompiledCircuit, lanes_per_proof: int = 0):
        self.cc = cc
        self.layout = cc.layout
        self.n_public = cc.n_public            # including ONE, as in the R1CS
        self.n_secret = cc.n_secret
        self.n_inputs = cc.n_inputs
        self.n_wires = cc.n_wires              # value slots below n_wires stay wire-backed
        self.consts = list(cc.consts)
        ops, val_wire = cc._ops, cc._val_wire
        n_pub = cc.n_public - 1
        gates = []                             # (a, b, c, qL, qR, qO, qM, qC) on SSA value ids
        one = 0                                # SSA value of the ONE wire (api.val_one)
        for j in range(1, n_pub + 1):          # public inputs first (their values are vals 1..)
            gates.append((j, j, j, 1, 0, 0, 0, 0))
        gates.append((one, one, one, 1, 0, 0, 0, R - 1))
        prog, row_of, chk = [], {}, {}
        self.commitments = []                  # {"rows": committed rows, "row": r_i, "wire", "val"}
        commit_vals = []                       # per commitment: SSA values of its operands

        def gate(g, check=0):
            row_of[len(prog)] = len(gates)
            chk[len(prog)] = check
            prog.append((OP_ABC, g[0], g[1], g[2]))
            gates.append(g)

        C = self.consts
        k_row = 0
        pending = None                         # the OP_COMMIT unit whose operand rows are being read
        for op, d, a, b in ops:
            if pending is not None and op != OP_HQ:
                raise AssertionError("OP_COMMIT unit cut short")
            if op == OP_COMMIT:
                pending = [d, a, b, []]
                if a == 0:
                    raise AssertionError("OP_COMMIT without operands")
                continue
            if op == OP_HQ and pending is not None:
                pending[3].append(a)
                if len(pending[3]) == pending[1]:
                    h, _, idx, reads = pending
                    pending = None
                    if idx != len(self.commitments):
                        raise AssertionError("commitments out of order")
                    rows = []
                    for v in reads:            # committed rows, operand order
                        rows.append(len(gates))
                        gate((v, v, v, R - 1, 0, 0, 0, 0))
                    prog.append((OP_COMMIT, h, len(reads), idx))
                    prog.extend((OP_HQ, 0, v, 0) for v in reads)
                    self.commitments.append({"rows": rows, "row": len(gates), "val": h})
                    commit_vals.append(list(reads))
                    gate((h, h, h, R - 1, 0, 0, 0, 0))
                continue
            if op == OP_ABC:
                gate((d, a, b, 0, 0, R - 1, 1, 0), 1 if cc._row_check[k_row] else 0)
                k_row += 1
                continue
            if op == OP_MULABC:
                k_row += 1
                prog.append((OP_MUL, d, a, b))
                gate((a, b, d, 0, 0, R - 1, 1, 0))
            elif op == OP_XORABC:
                k_row += 1
                prog.append((OP_XOR, d, a, b))
                gate((a, b, d, 1, 1, R - 1, R - 2, 0))
            elif op == OP_MUL:
                prog.append((op, d, a, b))
                gate((a, b, d, 0, 0, R - 1, 1, 0))
            elif op == OP_ADD:
                prog.append((op, d, a, b))
                gate((a, b, d, 1, 1, R - 1, 0, 0))
            elif op == OP_SUB:
                prog.append((op, d, a, b))
                gate((a, b, d, 1, R - 1, R - 1, 0, 0))
            elif op == OP_MULC:
                prog.append((op, d, a, b))
                gate((a, a, d, C[b], 0, R - 1, 0, 0))
            elif op == OP_ADDC:
                prog.append((op, d, a, b))
                gate((a, a, d, 1, 0, R - 1, 0, C[b]))
            elif op == OP_NEG:
                prog.append((op, d, a, b))
                gate((a, a, d, 1, 0, 1, 0, 0))
            elif op == OP_COPY:
                prog.append((op, d, a, b))
                gate((a, a, d, 1, 0, R - 1, 0, 0))
            elif op == OP_SETC:
                prog.append((op, d, a, b))
                gate((d, d, d, 0, 0, R - 1, 0, C[b]))
            elif op in (OP_INV, OP_DIV, OP_BITS, OP_BATCHINV, OP_PAIR, OP_HIST, OP_HQ, OP_EMUL,
                        OP_BXOR, OP_BAND):
                prog.append((op, d, a, b))     # hints: constrained by the rows that use them
            else:
                raise AssertionError(op)
        # rows of the public-input / ONE gates come first: prepend their OP_ABC rows
        head = [(OP_ABC, g[0], g[1], g[2]) for g in gates[:n_pub + 1]]
        shift = len(head)
        row_of = {i + shift: r for i, r in row_of.items()}
        chk = {i + shift: c for i, c in chk.items()}
        for i in range(shift):
            row_of[i] = i
        prog = head + prog
        self._prog, self._row_of = prog, row_of    # program order before scheduling (solver_description)
        self.n_gates = len(gates)
        self.n_constraints = self.n_gates      # rows the solver emits
        self.log_n = max(2, (self.n_gates - 1).bit_length())
        self.gates = gates
        (self.vprogram, self.v_n_rows, self.v_n_steps, self.v_n_slots, self.lanes_per_proof,
         self.schedule_cost) = build_vprogram(prog, val_wire, row_of, chk, cc.n_wires,
                                              lanes_per_proof)
        self._build_tables()
        # commitments: the wire numbers a shim sees (wiring()), the operands' value slots for the CPU
        # evaluation of the program, and the Qcp columns on the domain
        xa = self.wiring()[0]
        n = 1 << self.log_n
        self.qcp = []
        for c, vals in zip(self.commitments, commit_vals):
            c["wire"] = int(xa[c["row"]])
            c["slots"] = [val_wire[v] for v in vals]
            col = np.zeros(n, dtype=object)
            col[c["rows"]] = 1
            self.qcp.append(col)
        self.commit_fn = None      # run_vprogram: (index, committed values in operand order) -> int

    def _commit_value(self, idx, s):
        """challenge of commitment ``idx`` from the value file: ``commit_fn(idx, committed values)``
        (plonk side: hash of [pi2_idx]); without one, a SHA-256 stand-in, as for the R1CS."""
        vals = [s[w] for w in self.commitments[idx]["slots"]]
        if self.commit_fn is not None:
            return int(self.commit_fn(idx, vals)) % R
        h = hashlib.sha256(b"stand-in plonk commitment %d" % idx)
        for v in vals:
            h.update(int(v).to_bytes(32, "big"))
        return int.from_bytes(h.digest(), "big") % R

    # the CPU evaluation of the scheduled program is the R1CS one (same machinery)
    run_vprogram = CompiledCircuit.run_vprogram

    def assignment_vector(self, assignment):
        return self.cc.assignment_vector(assignment)

    def _build_tables(self):
        n = 1 << self.log_n
        g = self.gates
        col = lambda j: np.array([x[j] for x in g] + [0] * (n - len(g)), dtype=object)
        self.qL, self.qR, self.qO, self.qM, self.qC = (col(j) for j in (3, 4, 5, 6, 7))
        # copy constraints: positions (column, row) holding the same SSA value form one cycle
        wires = [[x[j] for x in g] for j in (0, 1, 2)]
        sigma = np.arange(3 * n, dtype=np.int64)          # identity on padding rows
        where = {}
        for c in range(3):
            for r, v in enumerate(wires[c]):
                where.setdefault(v, []).append(c * n + r)
        for pos in where.values():
            for i, p in enumerate(pos):
                sigma[p] = pos[(i + 1) % len(pos)]
        self.sigma = sigma
        self.wires = wires
        # Rows of each column whose value is known to be a bit (a wire the builder knows boolean,
        # the ONE wire, padding rows): the Lagrange-basis commitment of a column (plonk.py) orders
        # its bases with the other rows first, so that whole groups of its subset-sum tables see
        # one-bit scalars.  Only speed depends on this classification, never a result.
        val_wire = self.cc._val_wire
        bw = self.cc.boolean_wires
        bitv = {0} | {v for v, w in val_wire.items() if w in bw}
        C = self.consts
        for op, d, a, b in self.cc._ops:          # bits stay bits under and / xor / not / copy
            if op in (OP_MUL, OP_MULABC, OP_XOR, OP_XORABC):
                if a in bitv and b in bitv:
                    bitv.add(d)
            elif op == OP_SUB:
                if a == 0 and b in bitv:          # 1 - b
                    bitv.add(d)
            elif op == OP_COPY:
                if a in bitv:
                    bitv.add(d)
            elif op == OP_SETC:
                if C[b] in (0, 1):
                    bitv.add(d)
        is_bit = lambda v: v in bitv
        self.lag_order = []
        for c in range(3):
            head = [r for r, v in enumerate(wires[c]) if not is_bit(v)]
            hs = set(head)
            self.lag_order.append(np.array(head + [r for r in range(n) if r not in hs],
                                           dtype=np.uint32))
            self.n_nonbit_rows = max(getattr(self, "n_nonbit_rows", 0), len(head))

    def wiring(self):
        """(xa, xb, xc, n_wires): the wire every gate reads in columns a, b, c (uint32 [n_gates]
        each), what zkmi_scs_desc takes and what a shim reads off gnark's SparseR1CS.  The wires are
        the SSA values the gates touch, renumbered densely: ONE stays 0, the public inputs stay
        1 .. n_public - 1, the rest follow in the order of their SSA ids."""
        if getattr(self, "_wiring", None) is None:
            n_pub = self.n_public - 1
            rest = sorted({v for col in self.wires for v in col if v > n_pub})
            wire_of = {v: v for v in range(n_pub + 1)}
            wire_of.update({v: n_pub + 1 + i for i, v in enumerate(rest)})
            cols = [np.array([wire_of[v] for v in col], dtype=np.uint32) for col in self.wires]
            self._wiring = (cols[0], cols[1], cols[2], n_pub + 1 + len(rest))
        return self._wiring

    def solver_description(self, hints="basic"):
        """The gnark-shaped description of the solve (zkmi_scs_solver_desc), in the numbering of
        ``wiring()``: a dict with ``n_wires``, ``input_wire`` [n_inputs] (0xFFFFFFFF: nothing reads
        the input), ``instr`` [n_instr, 2] ((0, gate) | (1, hint), the program order before
        scheduling), and the hint table ``hint_kind``, ``hint_in_ptr``, ``hint_in_wire``,
        ``hint_in_coef`` (integers), ``hint_out_ptr``, ``hint_out``.  OP_INV becomes InvZero (kind
        1), OP_BITS of width 0 / 1 NBits (kind 2); the divisions (OP_DIV, OP_BATCHINV + OP_PAIR) are
        not exported: the kept rows that define their results are gates the solver divides in.  The
        one exception is an OP_PAIR value without such a row (IsZero's batched inverse-or-zero, whose
        first gate has a second unknown): it is the InvZero hint it stands for, placed in front of
        that gate.  Any other hint raises.  A hint operand or output no gate touches gets a wire behind those of
        ``wiring()``, so ``n_wires`` here may exceed wiring()'s.

        ``hints="std"`` (ZKMI_HINTS_STD; the dict's ``hint_set`` is then 1, else 0) exports four more
        kinds, each with the constant parameter p0 as its first input: OP_BITS with a limb width as
        limbs (kind 3, p0 = width), OP_HIST with its OP_HQ queries as lookup multiplicities (kind 4,
        p0 = table size), OP_BXOR / OP_BAND as byte operations (kind 6, p0 = 1 / 2) and the OP_COMMIT
        unit as a commitment hint (kind 5, p0 = index, then the committed wires in the order of the
        commitment's rows), which stands in front of its commitment row's gate.  OP_EMUL raises under
        both."""
        if hints not in ("basic", "std"):
            raise ValueError("hints: 'basic' or 'std'")
        std = hints == "std"
        cache = self.__dict__.setdefault("_solver_descs", {})
        if hints in cache:
            return cache[hints]
        names = {OP_HIST: "OP_HIST (lookup multiplicities)", OP_HQ: "OP_HQ (a lookup query)",
                 OP_COMMIT: "OP_COMMIT (api.Commit)", OP_EMUL: "OP_EMUL (the emulated product)",
                 OP_BXOR: "OP_BXOR (byte xor)", OP_BAND: "OP_BAND (byte and)",
                 OP_BITS: "OP_BITS with a limb width (limbs)"}
        n_pub = self.n_public - 1
        xa, _, _, n_wires = self.wiring()
        rest = sorted({v for col in self.wires for v in col if v > n_pub})
        wire_of = {v: v for v in range(n_pub + 1)}
        wire_of.update({v: n_pub + 1 + i for i, v in enumerate(rest)})

        def wire(v):                                   # a value no gate touches: a wire of its own
            nonlocal n_wires
            if v not in wire_of:
                wire_of[v] = n_wires
                n_wires += 1
            return wire_of[v]

        instr, kinds, in_ptr, in_wire, in_coef, out_ptr, outs = [], [], [0], [], [], [0], []

        def hint(kind, a, out_vals, p0=None):
            """a: the operand value, or the list of them; p0: the constant parameter in front"""
            instr.append((1, len(kinds)))
            kinds.append(kind)
            if p0 is not None:
                in_wire.append(0xFFFFFFFF)
                in_coef.append(p0)
            for v in (a if isinstance(a, list) else [a]):
                in_wire.append(wire(v))
                in_coef.append(1)
            in_ptr.append(len(in_wire))
            outs.extend(wire(v) for v in out_vals)
            out_ptr.append(len(outs))

        known = set(range(n_pub + 1)) | {v for v, w in self.cc._val_wire.items()
                                         if 1 <= w <= self.n_inputs}
        pairs = {}                                     # value of a pending OP_PAIR -> its operand
        unit = None                                    # std: [kind, p0, out values, rows to come, operands]
        for i, (op, d, a, b) in enumerate(self._prog):
            if std and unit is not None and op == OP_HQ:
                unit[4].append(a)
                unit[3] -= 1
            elif std and op in (OP_HIST, OP_COMMIT):
                unit = [4, b, list(range(d, d + b)), a, []] if op == OP_HIST else [5, b, [d], a, []]
            elif std and op == OP_BITS and (b >> 16) > 1:
                out_vals = [d + j for j in range(b & 0xffff)]
                hint(3, a, out_vals, p0=b >> 16)
                known.update(out_vals)
            elif std and op in (OP_BXOR, OP_BAND):
                hint(6, [a, b], [d], p0=1 if op == OP_BXOR else 2)
                known.add(d)
            if std and unit is not None:
                if unit[3] == 0:
                    hint(unit[0], unit[4], unit[2], p0=unit[1])
                    known.update(unit[2])
                    unit = None
                continue
            if std and (op in (OP_BXOR, OP_BAND) or (op == OP_BITS and (b >> 16) > 1)):
                continue
            if op == OP_ABC:
                unknown = {v for v in (d, a, b) if v not in known}
                if len(unknown) > 1:
                    for v in sorted(unknown & pairs.keys()):
                        hint(1, pairs.pop(v), [v])
                instr.append((0, self._row_of[i]))
                known.update((d, a, b))
            elif op == OP_INV or (op == OP_BITS and (b >> 16) <= 1):
                out_vals = [d + j for j in range(1 if op == OP_INV else b & 0xffff)]
                hint(1 if op == OP_INV else 2, a, out_vals)
                known.update(out_vals)
            elif op == OP_PAIR:
                pairs[d] = a
            elif op in names:
                raise ValueError(f"solver_description: the circuit holds {names[op]}, which the "
                                 + ("std hint set (limbs, lookup multiplicities, commitment, byte "
                                    "operations) does not cover" if std else
                                    "basic hint set (InvZero, NBits) does not cover"))
            # every other op is a gate (its OP_ABC row follows) or a division a gate defines
        val_of = {}
        for v, w in self.cc._val_wire.items():
            if 1 <= w <= self.n_inputs and (w not in val_of or v < val_of[w]):
                val_of[w] = v
        input_wire = [wire_of.get(val_of.get(1 + i), 0xFFFFFFFF) for i in range(self.n_inputs)]
        u32 = lambda x, shape=(-1,): np.array(x, dtype=np.uint32).reshape(shape)
        cache[hints] = {
            "hint_set": 1 if std else 0,
            "n_wires": n_wires, "input_wire": u32(input_wire), "instr": u32(instr, (-1, 2)),
            "hint_kind": u32(kinds), "hint_in_ptr": u32(in_ptr), "hint_in_wire": u32(in_wire),
            "hint_in_coef": list(in_coef), "hint_out_ptr": u32(out_ptr), "hint_out": u32(outs)}
        return cache[hints]

    def solve_description(self, desc, inputs, commit_fn=None):
        """Plain-Python interpreter of a solver description: the statement of what
        zkmi_scs_solve_batch computes and the CPU reference of its tests.  One walk over ``instr``
        with a solved-wire bitmap that starts with the inputs' wires (ONE is not special: its gate
        solves it).  A gate whose wires are all known is an assertion; otherwise its one unknown u is
        solved: where u takes no part in the product (qM = 0, or u in neither a nor b),
        x = -rest / k with k the sum of the linear selectors on u's positions; where u is exactly one
        of a, b and qM != 0, x = -rest / (k + qM other), a zero divisor flagging the proof.  Hints:
        InvZero (1 / v, 0 for v = 0) and NBits (output i = bit i of v), v = coef * wire or coef.
        The kinds of ZKMI_HINTS_STD, with the constant p0 as their first input: limbs (3: output j =
        bits [j p0, (j + 1) p0) of v), lookup multiplicities (4: output j = the number of queries
        equal to j, a query >= p0 counting nowhere), commitment (5: ``commit_fn(index, committed
        values)``, or the SHA-256 stand-in of ``_commit_value``) and byte operations (6: p0 = 1 XOR, 2
        AND on the low 32 bits).  The rows of the commitments (``self.commitments``) hold by
        construction and take no part in the gate check.
        inputs: n_inputs integers, public first.  Returns (wires, status): desc["n_wires"] integers
        and 0 or -5 (a zero divisor, or a gate that does not hold)."""
        xs = [x.tolist() for x in self.wiring()[:3]]
        n_wires, n_pub = desc["n_wires"], self.n_public - 1
        w, solved = [0] * n_wires, [False] * n_wires
        if len(inputs) != len(desc["input_wire"]):
            raise ValueError(f"expected {len(desc['input_wire'])} inputs, got {len(inputs)}")
        for v, iw in zip(inputs, desc["input_wire"].tolist()):
            if iw != 0xFFFFFFFF:
                w[iw], solved[iw] = int(v) % R, True
        status, seen = 0, set()
        kinds, ip, op_ = desc["hint_kind"].tolist(), desc["hint_in_ptr"].tolist(), desc["hint_out_ptr"].tolist()
        hw, hc, ho = desc["hint_in_wire"].tolist(), desc["hint_in_coef"], desc["hint_out"].tolist()
        for ii, (kind, idx) in enumerate(desc["instr"].tolist()):
            if kind == 1 and kinds[idx] in (3, 4, 5, 6):
                ts = list(range(ip[idx], ip[idx + 1]))
                o = ho[op_[idx]:op_[idx + 1]]
                if not ts or hw[ts[0]] != 0xFFFFFFFF:
                    raise ValueError(f"instruction {ii}: the parameter p0 must be a constant")
                for t in ts[1:]:
                    if hw[t] != 0xFFFFFFFF and not solved[hw[t]]:
                        raise ValueError(f"instruction {ii}: reads wire {hw[t]}, which is not solved yet")
                if any(solved[x] for x in o):
                    raise ValueError(f"instruction {ii}: an output wire is already solved")
                p0 = hc[ts[0]] % R
                vals = [hc[t] * (w[hw[t]] if hw[t] != 0xFFFFFFFF else 1) % R for t in ts[1:]]
                hk = kinds[idx]
                if hk == 3:
                    if len(vals) != 1 or not 1 <= p0 <= 64:
                        raise ValueError(f"instruction {ii}: limbs take a width in 1 .. 64 and one value")
                    for j, x in enumerate(o):
                        w[x] = (vals[0] >> (j * p0)) & ((1 << p0) - 1)
                elif hk == 4:
                    if p0 != len(o):
                        raise ValueError(f"instruction {ii}: the table size is not the number of outputs")
                    for j, x in enumerate(o):
                        w[x] = sum(1 for v in vals if v == j)
                elif hk == 6:
                    if len(vals) != 2 or len(o) != 1 or p0 not in (1, 2):
                        raise ValueError(f"instruction {ii}: a byte operation takes 1 | 2 and two values")
                    u, v = vals[0] & 0xffffffff, vals[1] & 0xffffffff
                    w[o[0]] = u ^ v if p0 == 1 else u & v
                else:
                    if len(o) != 1 or not vals:
                        raise ValueError(f"instruction {ii}: a commitment has operands and one output")
                    if commit_fn is not None:
                        w[o[0]] = int(commit_fn(p0, vals)) % R
                    else:
                        h = hashlib.sha256(b"stand-in plonk commitment %d" % p0)
                        for v in vals:
                            h.update(int(v).to_bytes(32, "big"))
                        w[o[0]] = int.from_bytes(h.digest(), "big") % R
                for x in o:
                    solved[x] = True
                continue
            if kind == 1:
                if kinds[idx] not in (1, 2) or ip[idx + 1] - ip[idx] != 1:
                    raise ValueError(f"instruction {ii}: not an InvZero or NBits hint with one input")
                t = ip[idx]
                if hw[t] != 0xFFFFFFFF and not solved[hw[t]]:
                    raise ValueError(f"instruction {ii}: reads wire {hw[t]}, which is not solved yet")
                v = hc[t] * (w[hw[t]] if hw[t] != 0xFFFFFFFF else 1) % R
                o = ho[op_[idx]:op_[idx + 1]]
                if any(solved[x] for x in o):
                    raise ValueError(f"instruction {ii}: an output wire is already solved")
                if kinds[idx] == 1:
                    w[o[0]] = pow(v, R - 2, R)
                else:
                    for j, x in enumerate(o):
                        w[x] = (v >> j) & 1
                for x in o:
                    solved[x] = True
                continue
            g = idx
            if g in seen:
                raise ValueError(f"instruction {ii}: gate {g} occurs twice")
            seen.add(g)
            pos = [xs[0][g], xs[1][g], xs[2][g]]
            _, _, _, qL, qR, qO, qM, qC = self.gates[g]
            unknown = {x for x in pos if not solved[x]}
            if not unknown:
                continue
            if len(unknown) > 1:
                raise ValueError(f"instruction {ii}: gate {g} has two unknown wires")
            u = unknown.pop()
            in_a, in_b = pos[0] == u, pos[1] == u
            k = sum(q for q, x in zip((qL, qR, qO), pos) if x == u) % R
            rest = (sum(q * w[x] for q, x in zip((qL, qR, qO), pos) if x != u) + qC) % R
            if g < n_pub:
                raise ValueError(f"instruction {ii}: public gate {g} has an unknown wire")
            if qM % R and (in_a or in_b):
                if in_a and in_b:
                    raise ValueError(f"instruction {ii}: gate {g} is quadratic in its unknown")
                den = (k + qM * w[pos[1] if in_a else pos[0]]) % R
                if den == 0:
                    status = -5
                w[u] = -rest * pow(den, R - 2, R) % R
            else:
                if k == 0:
                    raise ValueError(f"instruction {ii}: the unknown of gate {g} has coefficient 0")
                rest = (rest + qM * w[pos[0]] * w[pos[1]]) % R
                w[u] = -rest * pow(k, R - 2, R) % R
            solved[u] = True
        if len(seen) != self.n_gates:
            raise ValueError("a gate occurs in no instruction")
        if not all(solved):
            raise ValueError(f"wire {solved.index(False)} is still unsolved")
        held = {r for c in getattr(self, "commitments", []) for r in list(c["rows"]) + [c["row"]]}
        for g, (_, _, _, qL, qR, qO, qM, qC) in enumerate(self.gates):
            a, b, c = w[xs[0][g]], w[xs[1][g]], w[xs[2][g]]
            if g in held:
                continue
            if (qL * a + qR * b + qO * c + qM * a * b + qC - (a if g < n_pub else 0)) % R:
                status = -5
        return w, status

    def wire_vectors(self, a, b, c):
        """Solved columns -> the wire vectors zkmi_plonk_prove_witness takes (scs != NULL form): wire
        w gets the value of a position that reads it.  a, b, c: [batch, n_gates, 4] uint64 arrays
        (Montgomery image) -> [batch, n_wires, 4]; or, per proof, lists of n_gates integers -> lists
        of n_wires integers."""
        xa, xb, xc, n_wires = self.wiring()
        if isinstance(a, np.ndarray) and a.ndim == 3:
            out = np.zeros((a.shape[0], n_wires, 4), dtype=np.uint64)
            for x, col in ((xa, a), (xb, b), (xc, c)):
                out[:, x] = col[:, :self.n_gates]
            return out
        out = [[0] * n_wires for _ in a]
        for x, col in ((xa, a), (xb, b), (xc, c)):
            for w, vals in zip(out, col):
                for g, xw in enumerate(x.tolist()):
                    w[xw] = vals[g]
        return out

    def is_satisfied(self, a, b, c, public, pi2=None, H=None):
        """gate equations + copy constraints on full columns (lists of ints, length n_gates).
        pi2: per commitment, its Lagrange values (a sequence over the gate rows, or {row: value});
        H: per commitment, the value hashed from [pi2_i].  Left out, they are what the columns
        imply (pi2_i = a on the committed rows, H_i = a at the commitment row)."""
        g = self.gates
        n_pub = self.n_public - 1
        extra = {}                             # row -> PI' + sum_i Qcp_i pi2_i beyond the public rows
        for i, cm in enumerate(self.commitments):
            r = cm["row"]
            extra[r] = (extra.get(r, 0) + (a[r] if H is None else H[i])) % R
            for row in cm["rows"]:
                v = a[row] if pi2 is None else pi2[i][row]
                extra[row] = (extra.get(row, 0) + v) % R
        for i, (wa, wb, wc, qL, qR, qO, qM, qC) in enumerate(g):
            pi = ((-public[i]) % R if i < n_pub else 0) + extra.get(i, 0)
            if (qL * a[i] + qR * b[i] + qO * c[i] + qM * a[i] * b[i] + qC + pi) % R:
                return False, i
        n = 1 << self.log_n
        cols = (a, b, c)
        val = lambda p: cols[p // n][p % n] if p % n < len(g) else 0
        for p in range(3 * n):
            if self.sigma[p] != p and val(p) != val(int(self.sigma[p])):
                return False, -p
        return True, -1


def compile_scs(circuit, lanes_per_proof: int = 0) -> ScsCircuit:
    """``frontend.Compile(field, scs.NewBuilder, circuit)`` look-alike."""
    from .compile import compile_circuit
    cc = circuit if isinstance(circuit, CompiledCircuit) else compile_circuit(circuit)
    return ScsCircuit(cc, lanes_per_proof)
