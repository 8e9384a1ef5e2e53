"""The gnark-shaped PLONK solver under ZKMI_HINTS_STD on the GPU (scs_solve_kernel<S, 1>,
zkmi_plonk_prove_scs_ex): the hand description of tests/test_native_scs_std_plan.py through
zkmi_scs_solve_batch at every lane count against the Python reference; circuits with range checks,
lookups and api.Commit proved from inputs alone, byte for byte against the prover that runs the
frontend's witness program and against the wire form, on both key loaders; the refusals of the C ABI.
70 proofs are two ragged wavefronts at S = 1 and more than one wavefront at every S."""
import copy
import ctypes as C
import random

import numpy as np
import pytest

from gnark_crypto_primitives_amd import lib, plonk
from gnark_crypto_primitives_amd.frontend import Public, Secret
from gnark_crypto_primitives_amd.frontend.compile import to_mont_array
from gnark_crypto_primitives_amd.frontend.scs import compile_scs
from tests.scs_plan_harness import HandStd, std_inputs
from tests.test_gpu_plonk_commit import RANGE_BAD, RANGE_GOOD, SEED, UNSAT, key, mont

pytestmark = pytest.mark.gpu
R = plonk.R
NONE = 0xFFFFFFFF


# ---- 1. the hand description, no key -----------------------------------------------------------------
class HandSolve:
    """HandStd without its commitment hints on the device: the system, 70 inputs of 6 distinct
    kinds, the reference of each (computed once)"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.hand = hand = HandStd(commits=False)
        self.desc = hand.description()
        rng = random.Random(70)
        kinds = [std_inputs(rng) for _ in range(5)] + [[1, 0, 0, 0]]
        self.rows = [kinds[i % 6] if i != 64 else kinds[0] for i in range(70)]
        self.ref = {tuple(v): hand.solve_description(self.desc, v) for v in kinds}
        assert all(st == 0 for _, st in self.ref.values())
        self.inp = np.stack([to_mont_array(v) for v in self.rows])
        xa, xb, xc, n_wires = hand.wiring()
        sel = np.stack([to_mont_array([int(v) % R for v in col])
                        for col in (hand.qL, hand.qR, hand.qO, hand.qM, hand.qC)])
        self._keep = [np.ascontiguousarray(x, dtype=np.uint32) for x in (xa, xb, xc)] + [np.ascontiguousarray(sel)]
        self.scs_h = ctx.scs_load(lib.ScsDesc(n_wires, hand.n_gates, hand.n_public - 1,
                                              *[x.ctypes.data for x in self._keep]))

    def load(self, lanes, desc=None):
        d = self.desc if desc is None else desc
        u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32)
        arrs = [u32(d[k]) for k in ("input_wire", "instr", "hint_kind", "hint_in_ptr", "hint_in_wire")]
        arrs += [np.ascontiguousarray(to_mont_array([int(c) % R for c in d["hint_in_coef"]])),
                 u32(d["hint_out_ptr"]), u32(d["hint_out"])]
        sd = lib.ScsSolverDesc(len(arrs[0]), arrs[0].ctypes.data, arrs[1].size // 2, len(arrs[2]),
                               *[a.ctypes.data for a in arrs[1:]], lanes, d["hint_set"])
        return self.ctx.scs_solver_load(self.scs_h, sd)

    def solve(self, h, batch):
        wires = np.zeros((batch, self.hand.n_wires, 4), dtype=np.uint64)
        status = self.ctx.scs_solve_batch(h, np.ascontiguousarray(self.inp[:batch]), batch, wires)
        return status, wires

    def check(self, lanes, batch):
        h = self.load(lanes)
        try:
            info = self.ctx.scs_solver_info(h)
            assert info["lanes_per_proof"] == lanes or (lanes == 0 and info["lanes_per_proof"] in (1, 2, 4, 8, 16))
            assert info["n_records"] == 26 and info["n_steps"] * info["lanes_per_proof"] >= 26
            status, wires = self.solve(h, batch)
        finally:
            self.ctx.scs_solver_free(h)
        assert not status.any()
        for i in range(batch):
            assert np.array_equal(wires[i], to_mont_array(self.ref[tuple(self.rows[i])][0])), (lanes, batch, i)

    def close(self):
        self.ctx.scs_free(self.scs_h)


@pytest.fixture(scope="module")
def hand_solve(zk_ctx):
    s = HandSolve(zk_ctx)
    yield s
    s.close()


@pytest.mark.parametrize("lanes", [1, 2, 4, 8, 16, 32, 64, 0])
def test_hand_description_every_lane_count(hand_solve, lanes):
    hand_solve.check(lanes, 70)


@pytest.mark.parametrize("batch", [1, 63, 64, 65])
def test_hand_description_ragged_batches(hand_solve, batch):
    hand_solve.check(4, batch)


# ---- 2. proofs from inputs alone ---------------------------------------------------------------------
def assignment(name, kind):
    if name.startswith("range"):
        x, y = RANGE_BAD[kind - 2] if kind >= 2 else RANGE_GOOD[kind]
    else:
        y = 3 + kind
        x = y * y
    return {"X": x, "Y": y}


class Case:
    """One circuit with commitments: its key, the prover from inputs (zkmi_plonk_pk_load), the
    witness prover on the trace-loaded key with the std solver loaded.  A batch has two kinds of
    proofs (assignment and commitment blinding), so the host solve of the wire form is two runs."""

    def __init__(self, ctx, name):
        self.ctx, self.name = ctx, name
        self.sc, self.pk, self.prover = key(ctx, name)
        self.wp = plonk.WitnessProver(ctx, self.sc, self.pk, max_batch=128)
        self.wp.load_solver(hints="std")
        n_c = len(self.sc.commitments)
        rng = random.Random(len(name))
        self.bc_kinds = [[rng.randrange(R) for _ in range(2 * n_c)] for _ in range(2)]
        self.wires_of = {}

    def batch(self, batch, bad_at=()):
        rng = random.Random(batch)
        kinds = [2 + i % 3 if i in bad_at else i % 2 for i in range(batch)]
        inps = [self.sc.assignment_vector(assignment(self.name, k)) for k in kinds]
        blinds = [[rng.randrange(R) for _ in range(9)] for _ in range(batch)]
        bc = [self.bc_kinds[i % 2] for i in range(batch)]
        return kinds, inps, mont(inps), mont(blinds), mont(bc)

    def wires(self, kinds):
        """the solved wires of proofs of kinds 0 / 1, by the frontend's program with H_i from tau"""
        sc = self.sc
        for k in (0, 1):
            if k not in self.wires_of:
                sc.commit_fn = plonk.seeded_commit_fn(sc, SEED, self.bc_kinds[k])
                try:
                    cols = sc.run_vprogram(sc.assignment_vector(assignment(self.name, k)))[1:]
                finally:
                    sc.commit_fn = None
                assert sc.last_status == 0
                self.wires_of[k] = sc.wire_vectors(*[[c] for c in cols])[0]
        return mont([self.wires_of[k] for k in kinds])

    def prove_ex(self, pk_h, inp, blind, bc, solver_h=None, commit=True):
        batch = inp.shape[0]
        n_c = len(self.sc.commitments)
        rec = np.zeros((batch, 96), dtype=np.uint64)
        cm = np.zeros((batch, n_c, 12), dtype=np.uint64)
        st = np.ones(batch, dtype=np.int32)
        vkd = (C.c_uint8 * 32).from_buffer_copy(self.pk.vk_digest)
        rc = self.ctx.lib.zkmi_plonk_prove_scs_ex(
            self.ctx.h, pk_h, self.wp.solver_h if solver_h is None else solver_h, inp.ctypes.data, batch,
            blind.ctypes.data, bc.ctypes.data if commit else None, vkd, rec.ctypes.data,
            cm.ctypes.data if commit else None, st.ctypes.data)
        return rc, rec, st, cm

    def close(self):
        self.wp.close()


@pytest.fixture(scope="module")
def cases(zk_ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(zk_ctx, name)
        return made[name]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("batch", [1, 64, 65])
@pytest.mark.parametrize("name", ["range1", "range4", "range16", "two"])
def test_proofs_from_inputs_equal_the_other_entries(zk_ctx, cases, name, batch):
    c = cases(name)
    kinds, inps, inp, blind, bc = c.batch(batch)
    want, wstatus, wcm = c.prover.prove_raw(inp, blind, bc)
    assert not wstatus.any()
    rec, status, cm = c.wp.prove_raw(blind, inputs=inp, blind_commit=bc)
    assert not status.any() and rec.tobytes() == want.tobytes() and cm.tobytes() == wcm.tobytes()
    wrec, wst, wcm2 = c.wp.prove_raw(blind, wires=c.wires(kinds), blind_commit=bc)
    assert not wst.any() and wrec.tobytes() == want.tobytes() and wcm2.tobytes() == wcm.tobytes()
    # the key plonk.setup expanded on the host, through the C entry
    rc, rec2, st2, cm2 = c.prove_ex(c.prover.pk_h, inp, blind, bc)
    zk_ctx._check(rc, "zkmi_plonk_prove_scs_ex")
    assert not st2.any() and rec2.tobytes() == want.tobytes() and cm2.tobytes() == wcm.tobytes()
    proofs = plonk.Prover.proofs_of(rec, cm)
    for i in sorted({0, batch - 1}):
        assert len(proofs[i].bsb) == len(c.sc.commitments)
        assert plonk.verify(c.pk, [assignment(name, kinds[i])["X"]], proofs[i]), i


def test_a_key_without_commitments_returns_what_the_plain_entry_returns(zk_ctx):
    from tests.test_gpu_plonk_witness import case, mont as wmont, witnesses
    sc, pk, _ = case(zk_ctx, "tiny")
    inps, blinds, _, _ = witnesses("tiny", 5)
    inp, blind = wmont(inps), wmont(blinds)
    wp = plonk.WitnessProver(zk_ctx, sc, pk, max_batch=64, lagrange=False)
    try:
        for hints in ("basic", "std"):
            wp.load_solver(hints=hints)
            want, wstatus = wp.prove_raw(blind, inputs=inp)
            rec = np.zeros((5, 96), dtype=np.uint64)
            st = np.ones(5, dtype=np.int32)
            vkd = (C.c_uint8 * 32).from_buffer_copy(pk.vk_digest)
            zk_ctx._check(zk_ctx.lib.zkmi_plonk_prove_scs_ex(
                zk_ctx.h, wp.pk_h, wp.solver_h, inp.ctypes.data, 5, blind.ctypes.data, None, vkd,
                rec.ctypes.data, None, st.ctypes.data), "zkmi_plonk_prove_scs_ex")
            assert not st.any() and not wstatus.any() and rec.tobytes() == want.tobytes()
    finally:
        wp.close()


# ---- 3. a broken range check ---------------------------------------------------------------------------
def test_an_input_that_breaks_a_range_check_is_flagged(cases):
    """lanes 3 and 64 of 65 hold inputs outside their ranges (or a wrong product): exactly those are
    flagged, as from the witness program; every other record is the same"""
    c = cases("range4")
    kinds, inps, inp, blind, bc = c.batch(65, bad_at={3, 64})
    want, wstatus, wcm = c.prover.prove_raw(inp, blind, bc)
    rec, status, cm = c.wp.prove_raw(blind, inputs=inp, blind_commit=bc)
    assert [int(s) for s in status] == [UNSAT if i in (3, 64) else 0 for i in range(65)]
    assert np.array_equal(status, wstatus)
    ok = status == 0
    assert rec[ok].tobytes() == want[ok].tobytes() and cm[ok].tobytes() == wcm[ok].tobytes()


# ---- 4. refusals ---------------------------------------------------------------------------------------
class TwoIndependent:
    """two commitments that do not depend on each other: a plan may take them in either order"""
    X = Public()
    Y = Secret()

    def define(self, api):
        y2 = api.Mul(self.Y, self.Y)
        c1 = api.Commit(self.Y)
        c2 = api.Commit(y2)
        api.AssertIsEqual(api.Mul(api.Add(c1, c2), 0), 0)
        t = y2
        for _ in range(8):                       # enough gates for a domain of 2^4
            t = api.Mul(t, self.Y)
        api.AssertIsEqual(t, self.X)


def swapped_order(sc, desc):
    """the description with the block of commitment 1 (its committed rows' gates, its hint, its
    commitment row's gate) in front of commitment 0's, the indices renumbered"""
    instr = [tuple(x) for x in desc["instr"].tolist()]
    hk = desc["hint_kind"].tolist()
    h0, h1 = [h for h, k in enumerate(hk) if k == 5]
    blocks = []
    for h, c in ((h0, sc.commitments[0]), (h1, sc.commitments[1])):
        blocks.append([(0, r) for r in c["rows"]] + [(1, h), (0, c["row"])])
    rest = [x for x in instr if x not in blocks[0] and x not in blocks[1]]
    at = min(instr.index(x) for x in blocks[0])
    coef = list(desc["hint_in_coef"])
    ip = desc["hint_in_ptr"].tolist()
    coef[ip[h0]], coef[ip[h1]] = 1, 0
    return dict(desc, instr=np.array(rest[:at] + blocks[1] + blocks[0] + rest[at:], dtype=np.uint32),
                hint_in_coef=coef)


def test_refusals_leave_the_context_usable(zk_ctx, cases):
    from tests.test_gpu_plonk_witness import case, mont as wmont, witnesses
    c = cases("two")
    sc = c.sc
    kinds, inps, inp, blind, bc = c.batch(5)
    want, wstatus, wcm = c.wp.prove_raw(blind, inputs=inp, blind_commit=bc)
    assert not wstatus.any()
    std = sc.solver_description("std")
    plain_pk = copy.copy(c.pk)
    plain_pk.commitments = []
    plain = plonk.WitnessProver(zk_ctx, sc, plain_pk, max_batch=64)
    tsc, tpk, _ = case(zk_ctx, "tiny")
    tiny = plonk.WitnessProver(zk_ctx, tsc, tpk, max_batch=64, lagrange=False)
    isc = compile_scs(TwoIndependent())
    ipk = plonk.setup(zk_ctx, isc, SEED)
    ind = plonk.WitnessProver(zk_ctx, isc, ipk, max_batch=64)
    try:
        # a std solver with commitment hints on a key without commitments
        rc, rec, st, _ = c.prove_ex(plain.pk_h, inp, blind, bc, commit=False)
        with pytest.raises(lib.ZkmiError, match="the key carries 0 commitments, the solver's plan holds 2 "
                                                "commitment hints"):
            zk_ctx._check(rc, "zkmi_plonk_prove_scs_ex")
        assert not rec.any()
        # ... and through the entries without commitments, and the solve alone
        plain.load_solver(hints="std")
        with pytest.raises(lib.ZkmiError, match="the plan holds commitment hints: their values need a proving key"):
            plain.prove_raw(blind, inputs=inp)
        with pytest.raises(lib.ZkmiError, match="the plan holds commitment hints: their values need a proving key"):
            c.wp.solve(inp)
        # the plain solver entry on the key with commitments: today's message
        vkd = (C.c_uint8 * 32).from_buffer_copy(c.pk.vk_digest)
        with pytest.raises(lib.ZkmiError, match="this key carries commitments: the solver entries"):
            zk_ctx._check(zk_ctx.lib.zkmi_plonk_prove_scs(
                zk_ctx.h, c.wp.pk_h, c.wp.solver_h, inp.ctypes.data, 5, blind.ctypes.data, vkd,
                rec.ctypes.data, st.ctypes.data), "zkmi_plonk_prove_scs")
        # a basic solver on a key with commitments (one public input and a domain of 2^4, as Tiny has)
        tiny.load_solver()
        tinps, tblinds, _, _ = witnesses("tiny", 5)
        _, _, oprover = key(zk_ctx, "one")
        one_bc = mont([[1, 2]] * 5)
        cm1 = np.zeros((5, 1, 12), dtype=np.uint64)
        rc = zk_ctx.lib.zkmi_plonk_prove_scs_ex(
            zk_ctx.h, oprover.pk_h, tiny.solver_h, wmont(tinps).ctypes.data, 5, wmont(tblinds).ctypes.data,
            one_bc.ctypes.data, vkd, rec.ctypes.data, cm1.ctypes.data, st.ctypes.data)
        with pytest.raises(lib.ZkmiError, match="the key carries 1 commitments, the solver's plan holds 0 "
                                                "commitment hints"):
            zk_ctx._check(rc, "zkmi_plonk_prove_scs_ex")
        # the extras are needed, as for the other _ex entries
        rc, _, _, _ = c.prove_ex(c.wp.pk_h, inp, blind, bc, commit=False)
        with pytest.raises(lib.ZkmiError, match="needs blind_commit"):
            zk_ctx._check(rc, "zkmi_plonk_prove_scs_ex")
        # a committed-wire list that differs from the key's rows: the first two operands exchanged
        hk, ip = std["hint_kind"].tolist(), std["hint_in_ptr"].tolist()
        h0 = hk.index(5)
        hw = std["hint_in_wire"].copy()
        hw[ip[h0] + 1], hw[ip[h0] + 2] = hw[ip[h0] + 2], hw[ip[h0] + 1]
        other = c.wp.solver_h
        c.wp.solver_h = None
        try:
            c.wp.load_solver(desc=dict(std, hint_in_wire=hw))
            with pytest.raises(lib.ZkmiError, match="commitment hint 0 of the plan is not commitment 0 of the key"):
                c.wp.prove_raw(blind, inputs=inp, blind_commit=bc)
        finally:
            zk_ctx.scs_solver_free(c.wp.solver_h)
            c.wp.solver_h = other
        # a swapped commitment order
        ind.load_solver(hints="std")
        iinp = mont([isc.assignment_vector({"X": 3 ** 10, "Y": 3})] * 2)
        ibc = mont([[1, 2, 3, 4]] * 2)
        irec, ist, icm = ind.prove_raw(blind[:2], inputs=iinp, blind_commit=ibc)
        assert not ist.any()
        ind.load_solver(desc=swapped_order(isc, isc.solver_description("std")))
        with pytest.raises(lib.ZkmiError, match="commitment hint 0 of the plan is not commitment 0 of the key"):
            ind.prove_raw(blind[:2], inputs=iinp, blind_commit=ibc)
        ind.load_solver(hints="std")
        again = ind.prove_raw(blind[:2], inputs=iinp, blind_commit=ibc)
        assert again[0].tobytes() == irec.tobytes() and again[2].tobytes() == icm.tobytes()
        # kind 7 is refused by name under the std set, and the hint sets this entry lacks
        seven = dict(std, hint_kind=np.where(std["hint_kind"] == 5, 7, std["hint_kind"]).astype(np.uint32))
        with pytest.raises(lib.ZkmiError, match=r"hints emulated product \(kind 7\) are not supported on this entry"):
            c.wp.load_solver(desc=seven)
        with pytest.raises(lib.ZkmiError, match=r"hint_set must be ZKMI_HINTS_BASIC \(0\) or ZKMI_HINTS_STD \(1\)"):
            c.wp.load_solver(desc=dict(std, hint_set=3))
        with pytest.raises(lib.ZkmiError, match=r"hints commitment \(kind 5\) are not supported on this entry"):
            c.wp.load_solver(desc=dict(std, hint_set=0))
        # the context proves correctly afterwards, with the solver that stayed in place
        rec2, st2, cm2 = c.wp.prove_raw(blind, inputs=inp, blind_commit=bc)
        assert not st2.any() and rec2.tobytes() == want.tobytes() and cm2.tobytes() == wcm.tobytes()
    finally:
        plain.close()
        tiny.close()
        ind.close()
