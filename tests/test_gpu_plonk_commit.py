"""PLONK for circuits that call api.Commit (Qcp columns, BSB22) on the GPU: the commitment step
against integers, proofs from inputs and from solved wires against plonk.verify and its mutations,
the pieces of one proof against values recomputed in Python, and the plain entries unchanged.  Keys
come from plonk.setup with a seeded tau, so every Lagrange value L_g(tau) is a known integer and a
commitment is ONE Python scalar multiplication.  Parity with gnark is unpinned, as for the rest of
the PLONK prover.

Every good proof of batch 1 goes through plonk.verify; of the batches of 64 and 65 a fixed sample
does (first and last lane of the first wavefront, the lane in the second one): a verification is a
pairing in Python, and the lanes of a batch run the same instructions."""
import copy
import ctypes as C
import random

import numpy as np
import pytest

from gnark_crypto_primitives_amd import circuits, hash_to_field, lib, plonk, verify
from gnark_crypto_primitives_amd.frontend import Public, Secret
from gnark_crypto_primitives_amd.frontend.compile import array_to_ints, to_mont_array
from gnark_crypto_primitives_amd.frontend.scs import compile_scs
from gnark_crypto_primitives_amd.hash import poseidon_native
from tests.test_commitment import RangeCircuit, TwoCommitments

pytestmark = pytest.mark.gpu
R = plonk.R
RINV = pow(1 << 256, R - 2, R)
UNSAT = -5
SEED = 31


class OneRow:
    """a commitment over a single wire: |C_0| = 1"""
    X = Public()
    Y = Secret()

    def define(self, api):
        api.Commit(self.Y)
        t = self.Y
        for _ in range(8):                       # enough gates for the smallest domain, 2^4
            t = api.Mul(t, self.Y)
        api.AssertIsEqual(t, self.X)


MAKE = {"range1": lambda: compile_scs(RangeCircuit(), 1), "range4": lambda: compile_scs(RangeCircuit(), 4),
        "range16": lambda: compile_scs(RangeCircuit(), 16), "two": lambda: compile_scs(TwoCommitments()),
        "one": lambda: compile_scs(OneRow())}
_keys = {}


def key(zk_ctx, name):
    """(system, key, prover from inputs), once per circuit"""
    if name not in _keys:
        sc = MAKE[name]()
        pk = plonk.setup(zk_ctx, sc, SEED)
        _keys[name] = (sc, pk, plonk.Prover(zk_ctx, sc, pk, max_batch=128))
    return _keys[name]


def lagrange_at(log_n, x, rows):
    """L_g(x) on the domain of 2^log_n rows, as integers"""
    n, w = 1 << log_n, plonk.root_of_unity(log_n)
    zn = (pow(x, n, R) - 1) * pow(n, -1, R) % R
    return {g: pow(w, g, R) * zn % R * pow((x - pow(w, g, R)) % R, -1, R) % R for g in rows}


def tau():
    return random.Random(SEED).randrange(2, R)


def commitment_point(sc, i, values, b0, b1):
    """[pi2_i] as one scalar multiplication of the generator"""
    c, n = sc.commitments[i], 1 << sc.log_n
    L = lagrange_at(sc.log_n, tau(), set(c["rows"]) | {c["row"], n - 1})
    s = sum(v * L[g] for v, g in zip(values, c["rows"]))
    s += b1 * L[n - 1] + (0 if c["row"] == n - 1 else b0 * L[c["row"]])
    return verify._g1_mul((1, 2), s % R)


def mont(rows):
    return np.stack([to_mont_array(list(v)) for v in rows])


def ints(arr):
    return [v * RINV % R for v in array_to_ints(np.ascontiguousarray(arr))]


def last_error(ctx):
    return ctx.lib.zkmi_last_error(ctx.h).decode()


# ---- 1. the commitment step against integers --------------------------------------------------------
def hint(ctx, prover, index, values, blinds):
    batch = len(values)
    v, b = mont(values), mont(blinds)
    pts = np.zeros((batch, 8), dtype=np.uint64)
    hs = np.zeros((batch, 4), dtype=np.uint64)
    ctx._check(ctx.lib.zkmi_plonk_commit_hint(ctx.h, prover.pk_h, index, v.ctypes.data, b.ctypes.data,
                                              batch, pts.ctypes.data, hs.ctypes.data),
               "zkmi_plonk_commit_hint")
    return [verify.g1_from_image(p) for p in pts], ints(hs)


@pytest.mark.parametrize("batch", [1, 64, 65])
def test_commitment_step_against_integers(zk_ctx, batch):
    sc, pk, prover = key(zk_ctx, "range1")
    n_rows = len(sc.commitments[0]["rows"])
    assert n_rows == 37
    rng = random.Random(batch)
    values = [[rng.randrange(256) if j % 3 else rng.randrange(R) for j in range(n_rows)]
              for _ in range(batch)]
    blinds = [[rng.randrange(R), rng.randrange(R)] for _ in range(batch)]
    values[0], blinds[0] = [0] * n_rows, [0, 0]                       # the point at infinity
    if batch > 1:
        values[batch - 1] = [R - 1 - j for j in range(n_rows)]      # 254 bits
        blinds[batch - 1] = [R - 1, R - 2]
    pts, hs = hint(zk_ctx, prover, 0, values, blinds)
    assert pts[0] is None
    for p in range(batch):
        assert pts[p] == commitment_point(sc, 0, values[p], *blinds[p]), p
        assert hs[p] == hash_to_field.hash_fr(hash_to_field.g1_marshal(pts[p]),
                                              hash_to_field.PLONK_DST)[0], p


def test_commitment_step_single_row_and_254_bits(zk_ctx):
    sc, pk, prover = key(zk_ctx, "one")
    assert [len(c["rows"]) for c in sc.commitments] == [1]
    values, blinds = [[R - 1], [5], [0]], [[R - 1, R - 1], [0, 0], [1, 0]]
    pts, hs = hint(zk_ctx, prover, 0, values, blinds)
    for p in range(3):
        assert pts[p] == commitment_point(sc, 0, values[p], *blinds[p])
        assert hs[p] == plonk.commitment_hash(pts[p])
    sc2, _, prover2 = key(zk_ctx, "two")                             # the second commitment of a key
    values = [[3, 4, 5, 6]]
    pts, hs = hint(zk_ctx, prover2, 1, values, [[7, 8]])
    assert pts[0] == commitment_point(sc2, 1, values[0], 7, 8)


# ---- 2. end to end from inputs -------------------------------------------------------------------------
RANGE_GOOD = [(0x11 * 0x22, 0x1122334455662211), (8184, 0x21f8)]
RANGE_BAD = [(0x11 * 0x22 + 1, 0x2211), (0x11 * 0x22, 0x2211 + (1 << 64)), (8190, 0x2ac3)]


def assignments(name, batch, bad_at):
    out = []
    for i in range(batch):
        if name.startswith("range"):
            x, y = (RANGE_BAD[i % 3] if i in bad_at else RANGE_GOOD[i % 2])
        else:
            y = 3 + i
            x = y * y + (1 if i in bad_at else 0)
        out.append({"X": x, "Y": y})
    return out


def prove_inputs(zk_ctx, name, batch, bad_at, seed=9):
    sc, pk, prover = key(zk_ctx, name)
    rng = random.Random(seed)
    asg = assignments(name, batch, bad_at)
    inps = [sc.assignment_vector(a) for a in asg]
    blinds = [[rng.randrange(R) for _ in range(9)] for _ in range(batch)]
    bc = [[rng.randrange(R) for _ in range(2 * len(sc.commitments))] for _ in range(batch)]
    rec, status, cm = prover.prove_raw(mont(inps), mont(blinds), mont(bc))
    return sc, pk, asg, inps, blinds, bc, rec, status, cm


@pytest.mark.parametrize("batch", [1, 64, 65])
@pytest.mark.parametrize("name", ["range1", "range4", "range16", "two"])
def test_proofs_from_inputs_verify(zk_ctx, name, batch):
    bad_at = {3} if batch > 1 else set()
    sc, pk, asg, inps, blinds, bc, rec, status, cm = prove_inputs(zk_ctx, name, batch, bad_at)
    assert [int(s) for s in status] == [UNSAT if i in bad_at else 0 for i in range(batch)]
    proofs = plonk.Prover.proofs_of(rec, cm)
    sample = sorted({0, min(63, batch - 1), batch - 1})
    for i in sample:
        assert len(proofs[i].bsb) == len(sc.commitments)
        assert plonk.verify(pk, [asg[i]["X"]], proofs[i]), i
    for i in bad_at:
        assert not plonk.verify(pk, [asg[i]["X"]], proofs[i])
    if batch == 1:                                       # the out-of-range witness alone
        *_, status1, _ = prove_inputs(zk_ctx, name, 1, {0})
        assert int(status1[0]) == UNSAT


@pytest.mark.parametrize("name", ["range4", "two"])
def test_mutated_proofs_fail(zk_ctx, name):
    sc, pk, asg, inps, blinds, bc, rec, status, cm = prove_inputs(zk_ctx, name, 2, set(), seed=4)
    p0, p1 = plonk.Prover.proofs_of(rec, cm)
    pub = [asg[0]["X"]]
    assert plonk.verify(pk, pub, p0) and plonk.verify(pk, [asg[1]["X"]], p1)
    assert not plonk.verify(pk, [(pub[0] + 1) % R], p0)
    m = copy.deepcopy(p0)
    m.bsb = list(p1.bsb)                                 # [pi2_i] of another proof
    assert p0.bsb != p1.bsb and not plonk.verify(pk, pub, m)
    m = copy.deepcopy(p0)
    m.ev_qcp = ((p0.ev_qcp[0] + 1) % R,) + tuple(p0.ev_qcp[1:])
    assert not plonk.verify(pk, pub, m)
    if len(sc.commitments) == 2:
        m = copy.deepcopy(p0)
        m.bsb = p0.bsb[::-1]
        assert not plonk.verify(pk, pub, m)
    plain = copy.copy(pk)                                # a key whose digest omits the commitments
    plain.vk_digest = plonk.challenge("vk", pk.log_n, pk.n_public,
                                      *[pk.com[k] for k in plonk._NAMES]).to_bytes(32, "big")
    assert plain.vk_digest != pk.vk_digest and not plonk.verify(plain, pub, p0)


def test_first_commitment_at_infinity(zk_ctx):
    sc, pk, prover = key(zk_ctx, "two")
    inp = mont([sc.assignment_vector({"X": 0, "Y": 0})])
    rng = random.Random(2)
    blind = mont([[rng.randrange(R) for _ in range(9)]])
    rec, status, cm = prover.prove_raw(inp, blind, np.zeros((1, 4, 4), dtype=np.uint64))
    proof = plonk.Prover.proofs_of(rec, cm)[0]
    assert int(status[0]) == 0 and proof.bsb[0] is None and proof.bsb[1] is not None
    assert plonk.verify(pk, [0], proof)


# ---- 3. the pieces of one proof against integers -----------------------------------------------------
def real_commit_fn(sc, bc):
    """ScsCircuit.commit_fn with the prover's blinding: H_i from one scalar multiplication"""
    return lambda i, vals: plonk.commitment_hash(commitment_point(sc, i, vals, bc[2 * i], bc[2 * i + 1]))


@pytest.mark.parametrize("name", ["range4", "two"])
def test_pieces_of_one_proof(zk_ctx, name):
    sc, pk, asg, inps, blinds, bc, rec, status, cm = prove_inputs(zk_ctx, name, 1, set(), seed=6)
    proof = plonk.Prover.proofs_of(rec, cm)[0]
    sc.commit_fn = real_commit_fn(sc, bc[0])
    try:
        _, a, b, c = sc.run_vprogram(inps[0])
    finally:
        sc.commit_fn = None
    assert sc.last_status == 0
    n = 1 << sc.log_n
    for i, cmt in enumerate(sc.commitments):
        want = commitment_point(sc, i, [a[g] for g in cmt["rows"]], bc[0][2 * i], bc[0][2 * i + 1])
        assert proof.bsb[i] == want
        assert a[cmt["row"]] == plonk.commitment_hash(proof.bsb[i])      # the commitment wire is H_i
    H = [plonk.commitment_hash(pt) for pt in proof.bsb]
    assert sc.is_satisfied(a, b, c, [asg[0]["X"]], H=H)[0]
    pub = [asg[0]["X"]]
    gamma = plonk.challenge("gamma", pk.vk_digest, *pub, proof.a, proof.b, proof.c)
    beta = plonk.challenge("beta", gamma)
    alpha = plonk.challenge("alpha", beta, *proof.bsb, proof.z)
    zeta = plonk.challenge("zeta", alpha, proof.tlo, proof.tmid, proof.thi)
    L = lagrange_at(sc.log_n, zeta, range(n))
    zh = (pow(zeta, n, R) - 1) % R
    for k, col in enumerate((a, b, c)):
        want = (sum(v * L[g] for g, v in enumerate(col)) +
                (blinds[0][2 * k] * zeta + blinds[0][2 * k + 1]) * zh) % R
        assert proof.ev[k] == want, k
    for i, cmt in enumerate(sc.commitments):
        assert proof.ev_qcp[i] == sum(L[g] for g in cmt["rows"]) % R


# ---- 4. the entries agree --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["range4", "two"])
def test_witness_entries_equal_the_prover_from_inputs(zk_ctx, name):
    batch = 3
    sc, pk, asg, inps, blinds, bc, rec, status, cm = prove_inputs(zk_ctx, name, batch, set(), seed=8)
    prover = key(zk_ctx, name)[2]
    cols = []
    for p in range(batch):
        sc.commit_fn = real_commit_fn(sc, bc[p])
        try:
            cols.append(sc.run_vprogram(inps[p])[1:])
        finally:
            sc.commit_fn = None
    a, b, c = ([col[k] for col in cols] for k in range(3))
    wires = mont(sc.wire_vectors(a, b, c))
    columns = tuple(mont(x) for x in (a, b, c))
    bl, bcm = mont(blinds), mont(bc)
    wp = plonk.WitnessProver(zk_ctx, sc, pk, max_batch=64)           # the trace-loaded key
    try:
        for kw in ({"wires": wires}, {"columns": columns}):
            r2, s2, c2 = wp.prove_raw(bl, blind_commit=bcm, **kw)
            assert not s2.any() and np.array_equal(r2, rec) and np.array_equal(c2, cm), list(kw)
        # the expanded key, column form
        r3 = np.zeros_like(rec)
        c3 = np.zeros_like(cm)
        s3 = np.zeros(batch, dtype=np.int32)
        vkd = (C.c_uint8 * 32).from_buffer_copy(pk.vk_digest)
        zk_ctx._check(zk_ctx.lib.zkmi_plonk_prove_witness_ex(
            zk_ctx.h, prover.pk_h, None, None, *[x.ctypes.data for x in columns], sc.n_gates, batch,
            bl.ctypes.data, bcm.ctypes.data, vkd, r3.ctypes.data, c3.ctypes.data, s3.ctypes.data),
            "zkmi_plonk_prove_witness_ex")
        assert not s3.any() and np.array_equal(r3, rec) and np.array_equal(c3, cm)
        # a commitment wire off by one: that proof alone is flagged
        w = sc.commitments[-1]["wire"]
        off = sc.wire_vectors(a, b, c)
        off[1][w] = (off[1][w] + 1) % R
        _, s4, _ = wp.prove_raw(bl, wires=mont(off), blind_commit=bcm)
        assert [int(s) for s in s4] == [0, UNSAT, 0]
    finally:
        wp.close()


# ---- 5. nothing else moved -----------------------------------------------------------------------------
def test_ex_entries_without_commitments_return_the_plain_bytes(zk_ctx):
    sc = compile_scs(circuits.PoseidonCircuit())
    pk = plonk.setup(zk_ctx, sc, 7)
    assert pk.commitments == [] and pk.vk_digest == plonk.challenge(
        "vk", pk.log_n, pk.n_public, *[pk.com[k] for k in plonk._NAMES]).to_bytes(32, "big")
    prover = plonk.Prover(zk_ctx, sc, pk, max_batch=64)
    try:
        rng = random.Random(1)
        datas = [rng.randrange(R) for _ in range(5)]
        inp = mont([sc.assignment_vector({"Data": d, "Hash": poseidon_native.hash([d])}) for d in datas])
        blind = mont([[rng.randrange(R) for _ in range(9)] for _ in range(5)])
        rec, status = prover.prove_raw(inp, blind)
        r2, s2 = np.zeros_like(rec), np.zeros_like(status)
        vkd = (C.c_uint8 * 32).from_buffer_copy(pk.vk_digest)
        L = zk_ctx.lib
        zk_ctx._check(L.zkmi_plonk_prove_ex(zk_ctx.h, prover.pk_h, prover.cs_h, inp.ctypes.data, 5,
                                            blind.ctypes.data, None, vkd, r2.ctypes.data, None,
                                            s2.ctypes.data), "zkmi_plonk_prove_ex")
        assert np.array_equal(r2, rec) and np.array_equal(s2, status) and not status.any()
        cols = [sc.run_vprogram(array_to_ints_row(inp[i]))[1:] for i in range(5)]
        columns = tuple(mont([col[k] for col in cols]) for k in range(3))
        r3, s3 = np.zeros_like(rec), np.zeros_like(status)
        zk_ctx._check(L.zkmi_plonk_prove_witness_ex(
            zk_ctx.h, prover.pk_h, None, None, *[x.ctypes.data for x in columns], sc.n_gates, 5,
            blind.ctypes.data, None, vkd, r3.ctypes.data, None, s3.ctypes.data),
            "zkmi_plonk_prove_witness_ex")
        r4, s4 = np.zeros_like(rec), np.zeros_like(status)
        zk_ctx._check(L.zkmi_plonk_prove_witness(
            zk_ctx.h, prover.pk_h, None, None, *[x.ctypes.data for x in columns], sc.n_gates, 5,
            blind.ctypes.data, vkd, r4.ctypes.data, s4.ctypes.data), "zkmi_plonk_prove_witness")
        assert np.array_equal(r3, r4) and np.array_equal(r3, rec)
        # extras for a key without commitments are refused
        cm = np.zeros((5, 1, 12), dtype=np.uint64)
        assert L.zkmi_plonk_prove_ex(zk_ctx.h, prover.pk_h, prover.cs_h, inp.ctypes.data, 5,
                                     blind.ctypes.data, blind.ctypes.data, vkd, r2.ctypes.data,
                                     cm.ctypes.data, s2.ctypes.data) == -1
        assert "without commitments" in last_error(zk_ctx)
    finally:
        prover.close()


def array_to_ints_row(row):
    return ints(row)


def test_plain_entries_refuse_a_key_with_commitments(zk_ctx):
    sc, pk, prover = key(zk_ctx, "two")
    L = zk_ctx.lib
    inp = mont([sc.assignment_vector({"X": 9, "Y": 3})])
    blind = mont([[1] * 9])
    rec = np.zeros((1, 96), dtype=np.uint64)
    st = np.zeros(1, dtype=np.int32)
    abc = np.zeros((1, 3, 8), dtype=np.uint64)
    vkd = (C.c_uint8 * 32).from_buffer_copy(pk.vk_digest)
    assert L.zkmi_plonk_prove(zk_ctx.h, prover.pk_h, prover.cs_h, inp.ctypes.data, 1, blind.ctypes.data,
                              vkd, rec.ctypes.data, st.ctypes.data) == -1
    assert "carries commitments" in last_error(zk_ctx)
    assert L.zkmi_plonk_round1(zk_ctx.h, prover.pk_h, prover.cs_h, inp.ctypes.data, 1,
                               blind.ctypes.data, abc.ctypes.data, st.ctypes.data) == -1
    assert "carries commitments" in last_error(zk_ctx)
    col = mont([[0] * sc.n_gates])
    assert L.zkmi_plonk_prove_witness(zk_ctx.h, prover.pk_h, None, None, col.ctypes.data, col.ctypes.data,
                                      col.ctypes.data, sc.n_gates, 1, blind.ctypes.data, vkd,
                                      rec.ctypes.data, st.ctypes.data) == -1
    assert "carries commitments" in last_error(zk_ctx)
    assert L.zkmi_plonk_round1_witness(zk_ctx.h, prover.pk_h, None, None, col.ctypes.data,
                                       col.ctypes.data, col.ctypes.data, sc.n_gates, 1,
                                       blind.ctypes.data, abc.ctypes.data, st.ctypes.data) == -1
    assert not rec.any()
    with pytest.raises(ValueError):
        prover.prove(inp, blind)
    # the extras are needed
    assert L.zkmi_plonk_prove_ex(zk_ctx.h, prover.pk_h, prover.cs_h, inp.ctypes.data, 1,
                                 blind.ctypes.data, None, vkd, rec.ctypes.data, None,
                                 st.ctypes.data) == -1
    assert "needs blind_commit" in last_error(zk_ctx)
    # a second set_commitments, and one after a prove, are refused and leave the key as it is
    with pytest.raises(lib.ZkmiError, match="already carries"):
        plonk.set_commitments(zk_ctx, pk, prover.pk_h, [])
    bc = mont([[1, 2, 3, 4]])
    r1, s1, c1 = prover.prove_raw(inp, blind, bc)
    assert int(s1[0]) == 0 and plonk.verify(pk, [9], plonk.Prover.proofs_of(r1, c1)[0])


def test_set_commitments_refusals_on_a_fresh_key(zk_ctx):
    sc, pk, _ = key(zk_ctx, "two")
    bare = copy.copy(pk)
    bare.commitments = []                                # load the key without attaching anything
    prover = plonk.Prover(zk_ctx, sc, bare, max_batch=64)
    try:
        broken = copy.copy(pk)
        broken.commitments = [dict(c) for c in pk.commitments]
        broken.commitments[1]["rows"] = broken.commitments[1]["rows"][::-1]
        with pytest.raises(lib.ZkmiError, match="ascending"):
            plonk.set_commitments(zk_ctx, broken, prover.pk_h, [])
        broken.commitments = [dict(pk.commitments[0]) for _ in range(9)]
        with pytest.raises(lib.ZkmiError, match="at most 8"):
            plonk.set_commitments(zk_ctx, broken, prover.pk_h, [])
        plonk.set_commitments(zk_ctx, pk, prover.pk_h, prover._keep)      # nothing was half-attached
        inp = mont([sc.assignment_vector({"X": 16, "Y": 4})])
        rec, status, cm = plonk.Prover.prove_raw(_with_key(prover, pk), inp, mont([[2] * 9]),
                                                 mont([[5, 6, 7, 8]]))
        assert int(status[0]) == 0
        assert plonk.verify(pk, [16], plonk.Prover.proofs_of(rec, cm)[0])
    finally:
        prover.close()


def _with_key(prover, pk):
    prover.pk = pk
    return prover
