#!/usr/bin/env python3
"""Times the gnark-shaped solver (zkmi_r1cs_solve_batch / zkmi_prove_r1cs_submit) next to the
frontend program's solver (zkmi_solve_batch / zkmi_prove_submit) as the yardstick.  Prints one JSON
line.  Workloads:
  arbo160         the benched circuit, smt_inclusion_circuit(160) x 1024 proofs with 10 populated
                  siblings, through the basic solver
  address-commit  the address circuit with its commitment-backed range checks (2^18 domain, 144
                  committed wires) x 64 proofs, through the solver loaded with hints="std"
  emulated-poseidon  EmulatedPoseidonCircuit (2^17 domain, about 8 * 10^2 emulated products per
                  proof) x 64 proofs -- the batch size of its GPU test, filled with that test's
                  satisfied assignments -- through the solver loaded with hints="emulated"

    python tools/r1cs_solver_time.py [--workload arbo160|address-commit|emulated-poseidon] [--out FILE]

Three GPU steps, each a child process of its own under its own time limit; the first step that fails
ends the run (nothing more is started on the GPU):
  solve        idle-chip milliseconds of one solve of the batch, inputs resident in HBM, no outputs
               copied back: the gnark-shaped solver at the automatic lane count and at 8, 16, 32
               lanes per proof, then the frontend program.  Host clock around calls that end in a
               stream synchronise; one warm-up call, then the median and the least of five.
               address-commit, emulated-poseidon: a solve alone cannot supply the commitment, so the figure is the
               stage-1 device time (zkmi_last_timings [0]: solve launches, commitment MSM and hash)
               of submit_r1cs + collect, and of submit + collect, one batch at a time.
  pipe-program pipelined proofs/s of submit + collect over --steps batches (two in flight)
  pipe-r1cs    the same through submit_r1cs
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

LEVELS, POPULATED, BATCH, DISTINCT = 160, 10, 1024, 64
ADDRESS_BATCH = 64
WORKLOAD = "arbo160"
STEP_LIMIT_S = {"solve": 240, "pipe-program": 240, "pipe-r1cs": 300}
# the workloads with a commitment: the hint set their solver is loaded with
COMMITTED = {"address-commit": "std", "emulated-poseidon": "emulated"}


def _setup_address(need_key):
    import numpy as np
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    from gnark_crypto_primitives_amd import circuits, groth16, lib
    from gnark_crypto_primitives_amd.frontend import compile_circuit
    from gnark_crypto_primitives_amd.frontend.compile import to_mont_array
    from gnark_crypto_primitives_amd.std.emulated import limbs_of
    from oracle import pyref
    ctx = lib.Context(0)
    if WORKLOAD == "emulated-poseidon":
        cc = compile_circuit(circuits.EmulatedPoseidonCircuit(), 16)
        rng = random.Random(8)
        mk = circuits.EmulatedPoseidonCircuit.assignment
        distinct = [to_mont_array(cc.assignment_vector(a)) for a in
                    (mk((1, 2, 3)), mk((0, 0, 0)), mk((groth16.R - 1, groth16.R - 2, 1)),
                     mk([rng.randrange(groth16.R) for _ in range(3)]))]
    else:
        cc = compile_circuit(circuits.AddressCircuitCommit(), 16)
        rng = random.Random(56)
        distinct = []
        for _ in range(4):
            pub = pyref.secp256k1_mul(rng.randrange(1, pyref.SECP_N))
            distinct.append(to_mont_array(cc.assignment_vector(
                {"Address": pyref.eth_address(pub), "X": limbs_of(pub[0]), "Y": limbs_of(pub[1])})))
    inp = np.stack([distinct[i % len(distinct)] for i in range(ADDRESS_BATCH)])
    rs = np.stack([to_mont_array([rng.randrange(groth16.R), rng.randrange(groth16.R)])
                   for _ in range(ADDRESS_BATCH)])
    pk, _, _ = groth16.setup(cc, 1, groth16.gpu_mul(ctx))
    prover = groth16.Prover(ctx, cc, pk, 0, 0, max_batch=ADDRESS_BATCH)
    dev = torch.device("cuda:0")
    inp_d = torch.from_numpy(inp.view(np.int64)).to(dev)
    rs_d = torch.from_numpy(rs.view(np.int64)).to(dev)
    torch.cuda.synchronize()
    return ctx, cc, prover, inp_d, rs_d


def _setup(need_key):
    if WORKLOAD in COMMITTED:
        return _setup_address(need_key)
    import numpy as np
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    from gnark_crypto_primitives_amd import circuits, groth16, lib
    from gnark_crypto_primitives_amd.frontend import compile_circuit
    from gnark_crypto_primitives_amd.frontend.compile import to_mont_array
    from gnark_crypto_primitives_amd.tree import smt_witness
    ctx = lib.Context(0)
    cc = compile_circuit(circuits.smt_inclusion_circuit(LEVELS))
    rng = random.Random(160)
    distinct = [to_mont_array(cc.assignment_vector(
        smt_witness.synthetic_inclusion(rng, LEVELS, POPULATED))) for _ in range(DISTINCT)]
    inp = np.stack([distinct[i % DISTINCT] for i in range(BATCH)])
    rs = np.stack([to_mont_array([rng.randrange(groth16.R), rng.randrange(groth16.R)])
                   for _ in range(BATCH)])
    # the solve step needs no proving key worth its tables: the narrowest windows load fastest
    pk, _, _ = groth16.setup(cc, 1, groth16.gpu_mul(ctx))
    prover = groth16.Prover(ctx, cc, pk, *((0, 0) if need_key else (4, 4)), max_batch=BATCH)
    dev = torch.device("cuda:0")
    inp_d = torch.from_numpy(inp.view(np.int64)).to(dev)
    rs_d = torch.from_numpy(rs.view(np.int64)).to(dev)
    torch.cuda.synchronize()
    return ctx, cc, prover, inp_d, rs_d


def _time_ms(fn, repeats=5):
    fn()                                    # warm-up: code objects, scratch buffers
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "runs": repeats}


def step_solve_address():
    ctx, cc, prover, inp_d, rs_d = _setup(True)
    out = {}
    for which in ("r1cs", "program"):
        submit = prover.submit if which == "program" else prover.submit_r1cs
        if which == "r1cs":
            info = ctx.r1cs_solver_info(prover.load_r1cs_solver(0, hints=COMMITTED[WORKLOAD]))
            out["instr"] = {k: info[k] for k in ("n_instr", "n_terms", "longest", "n_inversions")}
        ms = []
        for n in range(4):                      # one warm-up, then three
            submit(inp_d, rs_d)
            _, st, _ = prover.collect()
            assert not st.any()
            if n:
                ms.append(ctx.last_timings()[0])
        out[which] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "runs": len(ms),
                      "lanes_per_proof": info["lanes_per_proof"] if which == "r1cs" else cc.lanes_per_proof}
    out["ratio_r1cs_to_program"] = out["r1cs"]["median_ms"] / out["program"]["median_ms"]
    prover.close()
    return out


def step_solve():
    if WORKLOAD in COMMITTED:
        return step_solve_address()
    import numpy as np
    ctx, cc, prover, inp_d, _ = _setup(False)
    status = np.zeros(BATCH, np.int32)
    out = {"instr": None, "r1cs": {}}
    for lanes in (0, 8, 16, 32):
        h = prover.load_r1cs_solver(lanes)
        info = ctx.r1cs_solver_info(h)
        out["instr"] = {k: info[k] for k in ("n_instr", "n_terms", "longest", "n_inversions")}
        t = _time_ms(lambda: ctx.r1cs_solve_batch(h, inp_d, BATCH, None, None, status))
        assert not status.any()
        out["r1cs"]["auto" if lanes == 0 else str(lanes)] = dict(t, lanes_per_proof=info["lanes_per_proof"])
    t = _time_ms(lambda: ctx.solve_batch(prover.cs_h, inp_d, BATCH, None, None, status))
    assert not status.any()
    out["program"] = dict(t, lanes_per_proof=cc.lanes_per_proof)
    out["ratio_auto_to_program"] = out["r1cs"]["auto"]["median_ms"] / t["median_ms"]
    prover.close()
    return out


def step_pipe(which, steps):
    ctx, cc, prover, inp_d, rs_d = _setup(True)
    submit = prover.submit if which == "program" else prover.submit_r1cs
    if which == "r1cs":
        prover.load_r1cs_solver(0, hints=COMMITTED.get(WORKLOAD, "basic"))
    batch = inp_d.shape[0]

    def run(n):
        submit(inp_d, rs_d)
        for _ in range(n - 1):
            submit(inp_d, rs_d)
            assert not prover.collect()[1].any()
        assert not prover.collect()[1].any()
        return ctx.last_timings()
    run(3)
    t0 = time.perf_counter()
    timings = run(steps)
    dt = time.perf_counter() - t0
    prover.close()
    return {"proofs_per_s": steps * batch / dt, "ms_per_step": dt / steps * 1e3, "steps": steps,
            "solve_stage_ms_last_batch": timings[0]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=tuple(STEP_LIMIT_S), help="run one step in this process")
    ap.add_argument("--steps", type=int, default=12, help="batches of a pipelined step (at least 10)")
    ap.add_argument("--workload", choices=("arbo160", "address-commit", "emulated-poseidon"), default="arbo160")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.steps < 10:
        ap.error("--steps must be at least 10")
    global WORKLOAD
    WORKLOAD = args.workload
    if args.step:
        res = step_solve() if args.step == "solve" else step_pipe(args.step[5:], args.steps)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    result = {"circuit": f"smt_inclusion_circuit({LEVELS})", "batch": BATCH, "populated": POPULATED}
    if WORKLOAD == "address-commit":
        result = {"circuit": "AddressCircuitCommit", "batch": ADDRESS_BATCH}
    if WORKLOAD == "emulated-poseidon":
        result = {"circuit": "EmulatedPoseidonCircuit", "batch": ADDRESS_BATCH}
    rc = 0
    for step, limit in STEP_LIMIT_S.items():
        # a fresh child per step; killed at its limit; after a failure nothing more runs on the GPU
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step,
                                "--steps", str(args.steps), "--workload", WORKLOAD], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            result[step] = {"error": f"time limit of {limit} s"}
            rc = 1
            break
        lines = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            result[step] = {"error": f"exit status {p.returncode}", "stderr": p.stderr[-2000:]}
            rc = 1
            break
        result[step] = json.loads(lines[-1][7:])
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
