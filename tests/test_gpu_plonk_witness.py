"""The gnark drop-in entry of the PLONK prover on the GPU: a key loaded from its trace form
(zkmi_plonk_pk_load_trace) against the expanded key of plonk.setup, and plonk.Prove from solved wires
or columns (zkmi_scs_load, zkmi_plonk_round1_witness, zkmi_plonk_prove_witness) against the prover
that solves from inputs and against the CPU restatement (oracle/plonk_ref.py).  Every comparison is
bit for bit.  Parity with gnark is unpinned, as for the rest of the PLONK prover."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from gnark_crypto_primitives_amd import circuits, lib, plonk
from gnark_crypto_primitives_amd.frontend import Public, Secret
from gnark_crypto_primitives_amd.frontend.compile import to_mont_array
from gnark_crypto_primitives_amd.frontend.scs import compile_scs
from gnark_crypto_primitives_amd.hash import poseidon_native

pytestmark = pytest.mark.gpu
R = plonk.R


class Tiny:
    """nine gates: the domain is 2^4, the quotient's 2^6 (the transforms' small-domain passes)"""
    X = Secret()
    Y = Public()

    def define(self, api):
        x2 = api.Mul(self.X, self.X)
        x3 = api.Mul(x2, self.X)
        w = api.Sub(api.Mul(api.Add(api.Add(x3, self.X), 5), 3), x2)
        api.AssertIsEqual(w, self.Y)


class Nine:
    """nine public inputs: PI(X) goes through the transforms in round 3"""
    P = Public(9)
    S = Secret()

    def define(self, api):
        acc = self.S
        for i in range(8):
            acc = api.Add(api.Mul(acc, self.P[i]), i + 1)
        api.AssertIsEqual(acc, self.P[8])


def _tiny_assignment(rng):
    x = rng.randrange(R)
    return {"X": x, "Y": (3 * (x * x * x + x + 5) - x * x) % R}


def _nine_assignment(rng):
    p = [rng.randrange(R) for _ in range(8)]
    s = acc = rng.randrange(R)
    for i in range(8):
        acc = (acc * p[i] + i + 1) % R
    return {"P": p + [acc], "S": s}


def _poseidon_assignment(rng):
    d = rng.randrange(R)
    return {"Data": d, "Hash": poseidon_native.hash([d])}


CASES = {"tiny": (Tiny, _tiny_assignment, 4, 21), "poseidon": (circuits.PoseidonCircuit,
                                                               _poseidon_assignment, 10, 7),
         "nine": (Nine, _nine_assignment, 5, 23)}
_cache = {}


def case(zk_ctx, name):
    """(system, GPU key of plonk.setup, oracle key), once per circuit"""
    from oracle import plonk_ref as P
    if name not in _cache:
        make, _, log_n, seed = CASES[name]
        sc = compile_scs(make())
        assert sc.log_n == log_n
        pk = plonk.setup(zk_ctx, sc, seed)
        key = P.setup(sc, seed)
        assert pk.com == key["com"]
        _cache[name] = (sc, pk, key)
    return _cache[name]


@functools.lru_cache(maxsize=None)
def witnesses(name, batch, seed=5):
    """inputs, blinding, solved columns and wire vectors of a batch (CPU solver), once"""
    sc = compile_scs(CASES[name][0]()) if name not in _cache else _cache[name][0]
    rng = random.Random(seed)
    inps = [sc.assignment_vector(CASES[name][1](rng)) for _ in range(batch)]
    blinds = [[rng.randrange(R) for _ in range(9)] for _ in range(batch)]
    if batch > 1:
        blinds[1] = [0] * 9
    cols = [sc.run_vprogram(inp)[1:] for inp in inps]
    a, b, c = ([col[k] for col in cols] for k in range(3))
    return inps, blinds, (a, b, c), sc.wire_vectors(a, b, c)


def mont(rows):
    return np.stack([to_mont_array(v) for v in rows])


def same(gp, op):
    return all(getattr(gp, f) == op[f] for f in plonk.Proof.FIELDS) and gp.ev == op["ev"]


@functools.lru_cache(maxsize=None)
def oracle_proofs(name, batch):
    """the CPU restatement's proofs of a whole batch of `witnesses`, once (its loops are in C and
    leave the interpreter free: eight at a time)"""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import plonk_ref as P
    sc, _, key = _cache[name]
    inps, blinds, cols, _ = witnesses(name, batch)
    n_pub = sc.n_public - 1
    one = lambda i: P.prove_fast(key, cols[0][i], cols[1][i], cols[2][i], inps[i][:n_pub], blinds[i])
    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(one, range(batch)))


def oracle_records_match(name, batch, rec, lanes):
    want = oracle_proofs(name, batch)
    proofs = plonk.Prover.proofs_of(rec)
    for i in lanes:
        assert same(proofs[i], want[i]), i


@pytest.mark.parametrize("name", ["tiny", "poseidon", "nine"])
def test_trace_key_equals_expanded_key(zk_ctx, name):
    """the same inputs and blinding through zkmi_plonk_prove on the key plonk.setup expanded on the
    host and on the key the GPU expanded from selectors and permutation: identical records, and the
    oracle's; for nine public inputs the wire form too, verified"""
    sc, pk, key = case(zk_ctx, name)
    batch = 5
    inps, blinds, cols, wires = witnesses(name, batch)
    inp, blind = mont(inps), mont(blinds)
    prover = plonk.Prover(zk_ctx, sc, pk, max_batch=64, lagrange=False)
    wp = plonk.WitnessProver(zk_ctx, sc, pk, max_batch=64, lagrange=False)
    want, wstatus = prover.prove_raw(inp, blind)
    rec = np.zeros((batch, 96), dtype=np.uint64)
    status = np.ones(batch, dtype=np.int32)
    vkd = (C.c_uint8 * 32).from_buffer_copy(pk.vk_digest)
    zk_ctx._check(zk_ctx.lib.zkmi_plonk_prove(zk_ctx.h, wp.pk_h, prover.cs_h, inp.ctypes.data, batch,
                                              blind.ctypes.data, vkd, rec.ctypes.data,
                                              status.ctypes.data), "zkmi_plonk_prove")
    wrec, wst = wp.prove_raw(blind, wires=mont(wires))
    prover.close()
    wp.close()
    assert not wstatus.any() and not status.any() and not wst.any()
    assert rec.tobytes() == want.tobytes()
    assert wrec.tobytes() == want.tobytes()
    oracle_records_match(name, batch, rec, range(batch))
    n_pub = sc.n_public - 1
    proofs = plonk.Prover.proofs_of(wrec)
    for i in range(batch if name == "nine" else 1):      # the host pairing takes a second a proof
        assert plonk.verify(pk, inps[i][:n_pub], proofs[i]), i


def test_wire_form_from_pageable_pinned_and_device_memory(zk_ctx):
    import torch
    sc, pk, key = case(zk_ctx, "poseidon")
    batch = 67                                                   # ragged second wavefront
    inps, blinds, cols, wires = witnesses("poseidon", batch)
    inp, blind, w = mont(inps), mont(blinds), mont(wires)
    prover = plonk.Prover(zk_ctx, sc, pk, max_batch=128, lagrange=False)
    want, wstatus = prover.prove_raw(inp, blind)
    prover.close()
    assert not wstatus.any()
    wp = plonk.WitnessProver(zk_ctx, sc, pk, max_batch=128, lagrange=False)
    pinned = zk_ctx.host_alloc(w.shape)
    pinned[...] = w
    dev = torch.from_numpy(w.view(np.int64)).to("cuda:0")
    for source in (w, pinned, dev):
        rec, status = wp.prove_raw(blind, wires=source)
        assert not status.any()
        assert rec.tobytes() == want.tobytes()
    zk_ctx.host_free(pinned)
    proofs, status = wp.prove(blind, wires=w)                    # the round-by-round twin
    assert not status.any() and proofs == plonk.Prover.proofs_of(want)
    for nb in (1, 64):
        rec, status = wp.prove_raw(blind[:nb], wires=np.ascontiguousarray(w[:nb]))
        assert not status.any() and rec.tobytes() == want[:nb].tobytes()
    # the column form: the same columns, taken as they are
    columns = tuple(mont(col) for col in cols)
    rec, status = wp.prove_raw(blind, columns=columns)
    assert (status == 0).all() and rec.tobytes() == want.tobytes()
    proofs, status = wp.prove(blind, columns=columns)
    wp.close()
    assert (status == 0).all() and proofs == plonk.Prover.proofs_of(want)
    oracle_records_match("poseidon", batch, want, (0, 1, 63, 64, 66))


def test_unsatisfied_lanes_are_flagged(zk_ctx):
    """lanes 0, 63, 64, 66 of 67 each carry one wrong wire; exactly those are flagged, the CPU check
    of the gathered columns fails on exactly those, every other lane's record is the oracle's"""
    sc, pk, key = case(zk_ctx, "poseidon")
    batch = 67
    inps, blinds, cols, wires = witnesses("poseidon", batch)
    xa, xb, xc, _ = sc.wiring()
    n_pub = sc.n_public - 1
    sel = lambda g: tuple(int(v) % R for v in sc.gates[g][3:])
    first = lambda want: next(g for g in range(n_pub + 1, sc.n_gates) if want(*sel(g)))
    g_mul = first(lambda qL, qR, qO, qM, qC: (qL, qR, qO, qM, qC) == (0, 0, R - 1, 1, 0))
    g_const = first(lambda qL, qR, qO, qM, qC: qC != 0 and qM == 0 and qR == 0)
    g_add = first(lambda qL, qR, qO, qM, qC: (qL, qR, qO, qM, qC) == (1, 1, R - 1, 0, 0))
    faults = {0: int(xc[g_mul]),         # a wrong product wire
              63: 1,                     # a changed public wire
              64: int(xc[g_const]),      # the output wire of a constant gate (c = a + k)
              66: int(xc[g_add])}        # a wrong c of an addition
    bad = [list(w) for w in wires]
    for lane, wire in faults.items():
        bad[lane][wire] = (bad[lane][wire] + 1 + lane) % R
    cpu_fails = []
    for i, w in enumerate(bad):
        ga, gb, gc = ([w[j] for j in x.tolist()] for x in (xa, xb, xc))
        if not sc.is_satisfied(ga, gb, gc, ga[:n_pub])[0]:
            cpu_fails.append(i)
    assert cpu_fails == sorted(faults)
    wp = plonk.WitnessProver(zk_ctx, sc, pk, max_batch=128, lagrange=False)
    rec, status = wp.prove_raw(mont(blinds), wires=mont(bad))
    wp.close()
    assert [i for i in range(batch) if status[i] != 0] == sorted(faults)
    assert all(status[i] == lib.ZKMI_ERR_UNSATISFIED for i in faults)
    good = [i for i in range(batch) if i not in faults]
    oracle_records_match("poseidon", batch, rec, good)


def test_lagrange_basis_from_wires(zk_ctx):
    sc, pk, key = case(zk_ctx, "poseidon")
    batch = 67
    inps, blinds, cols, wires = witnesses("poseidon", batch)
    blind, w = mont(blinds), mont(wires)
    out = {}
    for mode in (True, False):
        wp = plonk.WitnessProver(zk_ctx, sc, pk, max_batch=128, lagrange=mode)
        assert wp.lagrange == mode
        out[mode], status = wp.prove_raw(blind, wires=w)
        wp.close()
        assert not status.any()
    assert out[True].tobytes() == out[False].tobytes()
    oracle_records_match("poseidon", batch, out[True], (0, 1, 63, 64, 66))


def _refused(zk_ctx, rc, text):
    assert rc == -1, rc                                          # ZKMI_ERR_ARG
    msg = zk_ctx.lib.zkmi_last_error(zk_ctx.h).decode()
    assert text in msg, msg


def test_refusals_leave_the_context_usable(zk_ctx):
    sc, pk, key = case(zk_ctx, "tiny")
    inps, blinds, cols, wires = witnesses("tiny", 9)
    blind, w = mont(blinds), mont(wires)
    a, b, c = (mont(col) for col in cols)
    n, ng, nw = 1 << sc.log_n, sc.n_gates, sc.wiring()[3]
    wp = plonk.WitnessProver(zk_ctx, sc, pk, max_batch=8, lagrange=False)
    L = zk_ctx.lib
    vkd = (C.c_uint8 * 32).from_buffer_copy(pk.vk_digest)
    rec = np.zeros((9, 96), dtype=np.uint64)
    st = np.zeros(9, dtype=np.int32)
    p = lambda x: x.ctypes.data

    def prove(scs_h, wires_p, a_p, b_p, c_p, n_gates, batch):
        return L.zkmi_plonk_prove_witness(zk_ctx.h, wp.pk_h, scs_h, wires_p, a_p, b_p, c_p, n_gates,
                                          batch, p(blind), vkd, p(rec), p(st))
    # round 2 before either round 1
    bg = mont([[1, 2]] * 4)
    cz = np.zeros((4, 8), dtype=np.uint64)
    _refused(zk_ctx, L.zkmi_plonk_round2(zk_ctx.h, wp.pk_h, p(bg), p(cz)), "round 2 out of order")
    _refused(zk_ctx, prove(wp.scs_h, p(w), p(a), p(b), p(c), 0, 4), "either")       # both forms
    _refused(zk_ctx, prove(None, None, None, None, None, 0, 4), "either")           # neither
    _refused(zk_ctx, prove(wp.scs_h, p(w), None, None, None, 0, 9), "max_batch")    # batch 9 > 8
    # the columns of a system larger than the domain
    big = np.zeros((4, n + 1, 4), dtype=np.uint64)
    _refused(zk_ctx, prove(None, None, p(big), p(big), p(big), n + 1, 4), "n_gates")
    xa, xb, xc, _ = sc.wiring()
    gsel = np.ascontiguousarray(np.stack([to_mont_array([int(v) % R for v in col[:ng]]) for col in
                                          (sc.qL, sc.qR, sc.qO, sc.qM, sc.qC)]))
    # a system with another number of public inputs
    other = zk_ctx.scs_load(lib.ScsDesc(nw, ng, pk.n_public + 1, p(xa), p(xb), p(xc), p(gsel)))
    _refused(zk_ctx, prove(other, p(w), None, None, None, 0, 4), "public inputs")
    zk_ctx.scs_free(other)
    # a wiring that contradicts the key's permutation: one gate reads another wire in column b
    xb2 = xb.copy()
    xb2[ng - 2] = (xb2[ng - 2] + 1) % nw
    other = zk_ctx.scs_load(lib.ScsDesc(nw, ng, pk.n_public, p(xa), p(xb2), p(xc), p(gsel)))
    _refused(zk_ctx, prove(other, p(w), None, None, None, 0, 4), "contradicts the key's permutation")
    zk_ctx.scs_free(other)
    # the loaders' own refusals
    with pytest.raises(lib.ZkmiError, match="not a wire"):
        xa2 = xa.copy()
        xa2[3] = nw
        zk_ctx.scs_load(lib.ScsDesc(nw, ng, pk.n_public, p(xa2), p(xb), p(xc), p(gsel)))
    perm = np.ascontiguousarray(sc.sigma, dtype=np.uint32)
    perm[5] = perm[6]
    sel = np.ascontiguousarray(np.stack([to_mont_array([int(v) % R for v in col]) for col in
                                         (sc.qL, sc.qR, sc.qO, sc.qM, sc.qC)]))
    srs = np.ascontiguousarray(pk.srs_g1)
    none3 = (C.c_void_p * 3)()
    with pytest.raises(lib.ZkmiError, match="not a bijection"):
        zk_ctx.plonk_pk_load_trace(lib.PlonkTraceDesc(pk.log_n, pk.n_public, p(sel), p(perm), p(srs),
                                                      0, 8, none3, none3, 0))
    perm[5] = 3 * n
    with pytest.raises(lib.ZkmiError, match="not a position"):
        zk_ctx.plonk_pk_load_trace(lib.PlonkTraceDesc(pk.log_n, pk.n_public, p(sel), p(perm), p(srs),
                                                      0, 8, none3, none3, 0))
    # and a good batch proves on the same context, same key, same system
    got, status = wp.prove_raw(blind[:8], wires=np.ascontiguousarray(w[:8]))
    wp.close()
    assert not status.any()
    oracle_records_match("tiny", 9, got, range(8))
