#!/usr/bin/env python3
"""Times the gnark drop-in entry of the PLONK prover next to the entries it stands beside, on the
address circuit (BASELINE config 5: 231 270 gates, domain 2^18), batch 512.  Prints one JSON line.

    python tools/plonk_witness_time.py [--batch 512] [--workload address|address-commit] [--out FILE]
                                       [--entry scs]

--entry scs: a third leg behind the two, on the trace-loaded key: the gnark-shaped solver
(zkmi_scs_solver_load) for every lane count 1 .. 64 and the automatic one -- the plan's records,
steps and inversions, and the solve alone (zkmi_scs_solve_batch without the wires copied out) -- then
one batch through zkmi_plonk_prove_scs with the automatic lane count; the records of the three
entries must be identical.  With --workload address-commit the solver is loaded with the std hint
set (limbs, lookup multiplicities, commitment) at the automatic lane count alone and the batch goes
through zkmi_plonk_prove_scs_ex beside zkmi_plonk_prove_ex and zkmi_plonk_prove_witness_ex; the
solve alone is not timed there (zkmi_scs_solve_batch refuses a plan with commitment hints), so the
leg gives the plan's figures, the whole prove and its difference to the wire-form entry.

--workload address-commit: the same circuit with its bytes range-checked through api.Commit
(circuits.AddressCircuitCommit), proved through zkmi_plonk_prove_ex / zkmi_plonk_prove_witness_ex;
its wire vectors come from the host evaluation of the program, the commitment hashes from tau
(plonk.seeded_commit_fn), since the commitment wire depends on the blinding scalars.

Two pairs of numbers, all host clock around calls that end in a stream synchronise:
  key_load   seconds to a resident key: through the trace loader (selectors and permutation to
             zkmi_plonk_pk_load_trace + zkmi_scs_load; the GPU expands the key), and through
             plonk.setup (the host expands the key; this figure also holds the seeded SRS, which the
             trace path takes ready-made, so `setup_srs_s`, measured alone, is given beside it) plus
             the expanded loader (zkmi_plonk_pk_load)
  prove      milliseconds of one batch: zkmi_plonk_prove_witness with the wire vectors in page-locked
             host memory (the transfer and the gather are inside), and zkmi_plonk_prove from inputs
             (the witness solve is inside); one warm-up call, then the median of three.  The wire
             vectors are those of four distinct witnesses solved on the GPU (zkmi_solve_batch),
             repeated over the batch, as the inputs are.

One key is resident at a time (the second of two would leave the batch's buffers no room beside
its SRS tables).  One GPU process, under a time limit of its own; nothing runs on the GPU after it.
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIMIT_S = 540
DISTINCT = 4


def measure(batch, workload="address", entry=None):
    import numpy as np
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    from gnark_crypto_primitives_amd import circuits, lib, plonk, workloads
    from gnark_crypto_primitives_amd.frontend import compile_circuit
    from gnark_crypto_primitives_amd.frontend.compile import to_mont_array
    from gnark_crypto_primitives_amd.frontend.scs import compile_scs
    from gnark_crypto_primitives_amd.groth16 import g1_gen_mont
    t0 = time.perf_counter()
    circuit, gen, _ = workloads.build(workload)
    sc = compile_scs(compile_circuit(circuit, 16))
    n_c = len(sc.commitments)
    out = {"circuit": type(circuit).__name__, "gates": sc.n_gates, "domain_log2": sc.log_n,
           "batch": batch, "n_wires": sc.wiring()[3], "commitments": n_c,
           "committed_rows": [len(c["rows"]) for c in sc.commitments],
           "compile_s": time.perf_counter() - t0}
    ctx = lib.Context(0)

    def timed(fn):
        t = time.perf_counter()
        r = fn()
        ctx.sync()
        return r, time.perf_counter() - t
    # ---- key load
    pk, setup_s = timed(lambda: plonk.setup(ctx, sc, 3))
    n = 1 << sc.log_n
    pw = to_mont_array([pow(3, i, plonk.R) for i in range(n + 6)])
    srs = np.zeros((n + 6, 8), dtype=np.uint64)
    _, srs_s = timed(lambda: ctx.fixed_base_mul(1, g1_gen_mont(), pw, n + 6, srs))

    def median_ms(fn):
        fn()
        ms = []
        for _ in range(3):
            t = time.perf_counter()
            res = fn()
            ms.append((time.perf_counter() - t) * 1e3)
        return res, {"median_ms": statistics.median(ms), "min_ms": min(ms), "runs": 3}
    # One key at a time: the SRS tables of a key are planned into the HBM that is free when it
    # loads, so the second of two resident keys would leave the batch's buffers no room.
    # ---- the expanded loader, and one batch from inputs
    prover, expanded_s = timed(lambda: plonk.Prover(ctx, sc, pk, max_batch=batch))
    rng = random.Random(77)
    ws = [to_mont_array(sc.assignment_vector(gen(rng))) for _ in range(DISTINCT)]
    inp = np.stack([ws[i % DISTINCT] for i in range(batch)])
    blind = np.stack([to_mont_array([rng.randrange(plonk.R) for _ in range(9)]) for _ in range(batch)])
    extra = {}
    if n_c:
        # the commitment wires depend on the blinding scalars: one pair per distinct witness, the
        # columns from the host evaluation of the program
        bcs = [[rng.randrange(plonk.R) for _ in range(2 * n_c)] for _ in range(DISTINCT)]
        extra = {"blind_commit": np.stack([to_mont_array(bcs[i % DISTINCT]) for i in range(batch)])}
        rows = []
        for w, bc in zip(ws, bcs):
            sc.commit_fn = plonk.seeded_commit_fn(sc, 3, bc)
            vec = [v * pow(1 << 256, -1, plonk.R) % plonk.R
                   for v in __import__("gnark_crypto_primitives_amd.frontend.compile",
                                       fromlist=["array_to_ints"]).array_to_ints(w)]
            _, a, b, c = sc.run_vprogram(vec)
            assert sc.last_status == 0
            rows.append(to_mont_array(sc.wire_vectors([a], [b], [c])[0]))
        sc.commit_fn = None
        distinct = np.stack(rows)
    else:
        abc = np.zeros((3, DISTINCT, sc.n_gates, 4), dtype=np.uint64)
        status = ctx.solve_batch(prover.cs_h, np.stack(ws), DISTINCT, None, abc)
        assert not status.any()
        distinct = sc.wire_vectors(abc[0], abc[1], abc[2])
    (rec_i, st_i, *cm_i), t_i = median_ms(lambda: prover.prove_raw(inp, blind, *extra.values()))
    lagrange = prover.lagrange
    prover.close()
    # ---- the trace loader, and the same batch from wire vectors in page-locked memory
    calls = {}
    for name in ("plonk_pk_load_trace", "scs_load"):
        def wrapped(desc, fn=getattr(ctx, name), name=name):
            t = time.perf_counter()
            h = fn(desc)
            ctx.sync()
            calls[name] = time.perf_counter() - t
            return h
        setattr(ctx, name, wrapped)
    wp, trace_s = timed(lambda: plonk.WitnessProver(ctx, sc, pk, max_batch=batch))
    assert wp.lagrange == lagrange
    out["key_load"] = {"trace_loader_s": trace_s, "trace_loader_call_s": calls["plonk_pk_load_trace"],
                       "scs_load_call_s": calls["scs_load"], "setup_s": setup_s,
                       "setup_srs_s": srs_s, "expanded_loader_s": expanded_s,
                       "setup_plus_expanded_loader_s": setup_s + expanded_s,
                       "lagrange_basis": bool(lagrange)}
    wires = ctx.host_alloc((batch, wp.n_wires, 4))
    for i in range(batch):
        wires[i] = distinct[i % DISTINCT]
    out["wire_bytes_per_batch"] = int(wires.nbytes)
    (rec_w, st_w, *cm_w), t_w = median_ms(lambda: wp.prove_raw(blind, wires=wires, **extra))
    assert not st_w.any() and not st_i.any()
    out["prove"] = {"witness_pinned": t_w, "inputs": t_i,
                    "ratio_witness_to_inputs": t_w["median_ms"] / t_i["median_ms"],
                    "records_identical": rec_w.tobytes() == rec_i.tobytes() and
                    all(x.tobytes() == y.tobytes() for x, y in zip(cm_w, cm_i))}
    ctx.host_free(wires)
    if entry == "scs":
        hints = "std" if n_c else "basic"
        t = time.perf_counter()
        desc = sc.solver_description(hints)
        leg = {"description_s": time.perf_counter() - t, "n_wires": int(desc["n_wires"]), "hint_set": hints,
               "n_hints": int(len(desc["hint_kind"])), "lanes": {}}
        for lanes in ((0,) if n_c else (1, 2, 4, 8, 16, 32, 64, 0)):
            t = time.perf_counter()
            h = wp.load_solver(lanes, hints=hints)
            load_s = time.perf_counter() - t
            info = dict(ctx.scs_solver_info(h), load_s=load_s)
            if not n_c:
                st_s, info["solve"] = median_ms(lambda: ctx.scs_solve_batch(h, inp, batch))
                assert not st_s.any()
            leg["lanes"]["auto" if lanes == 0 else str(lanes)] = info
        (rec_s, st_s, *cm_s), t_p = median_ms(lambda: wp.prove_raw(blind, inputs=inp, **extra))
        assert not st_s.any()
        assert rec_s.tobytes() == rec_i.tobytes() == rec_w.tobytes(), "the three entries disagree"
        assert all(x.tobytes() == y.tobytes() for x, y in zip(cm_s, cm_i)), "the commit records disagree"
        if n_c:   # solve, boundary synchronisations and commitment step, less the wire transfer
            leg["prove_minus_witness_ms"] = t_p["median_ms"] - t_w["median_ms"]
        leg["prove"] = t_p
        leg["records_identical"] = True
        out["scs"] = leg
    wp.close()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--workload", default="address", choices=("address", "address-commit"))
    ap.add_argument("--entry", default=None, choices=("scs",), help="also time the solver entry")
    ap.add_argument("--child", action="store_true", help="run the measurement in this process")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(measure(args.batch, args.workload, args.entry)), flush=True)
        return 0
    # a fresh child, killed at its limit; nothing more runs on the GPU after a failure
    limit = LIMIT_S + (300 if args.entry else 0)     # the third leg: eight plans, 36 more batches
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--batch",
                            str(args.batch), "--workload", args.workload] +
                           (["--entry", args.entry] if args.entry else []), capture_output=True,
                           text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": f"time limit of {limit} s"}))
        return 1
    lines = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        print(json.dumps({"error": f"exit status {p.returncode}", "stderr": p.stderr[-2000:]}))
        return 1
    line = lines[-1][7:]
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
