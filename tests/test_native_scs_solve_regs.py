"""Build-time guard for csrc/scs_solve.hip, in the manner of tests/test_native_r1cs_solve_regs.py:
the code-object remarks of scs_solve_kernel<S, EXT> must show all fourteen instances (seven lane
counts, without and with the std classes), no instance may spill a vector register, and none may use
LDS: the design states none (records and wires come straight from global memory, the field code is
inline, bits and limbs under a per-lane index are chains of selects, never an indexed register
array).  The occupancy the solve's speed rests on is asserted: four waves per SIMD for the EXT = 0
instances up to 32 lanes per proof -- the std arms must not cost the plain plans a wave --, three for
the rest.  Registers and scratch per lane are printed and recorded in DESIGN.md §3.6.2, not
asserted.  The file is compiled once for both tests."""
import functools
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
LANES = (1, 2, 4, 8, 16, 32, 64)
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC) and not shutil.which("hipcc"), reason="hipcc missing")


@functools.lru_cache(maxsize=None)
def instances():
    """(S, EXT) -> the remarks of scs_solve_kernel<S, EXT>; exactly the fourteen instances"""
    src = os.path.join(ROOT, "gnark_crypto_primitives_amd", "csrc", "scs_solve.hip")
    err = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17",
                          "--offload-arch=gfx950", "--offload-device-only", "-mllvm",
                          "-pragma-unroll-threshold=1000000",
                          "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                         capture_output=True, text=True, timeout=900).stderr
    seen, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"remark:.*\s(VGPRs|AGPRs|VGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]"
                      r"|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur and "scs_solve_kernel" in cur:
            seen.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    inst = {}
    for name, r in seen.items():
        m = re.search(r"scs_solve_kernelILi(\d+)ELb([01])EE", name)
        assert m, name
        inst[int(m.group(1)), int(m.group(2))] = r
    assert sorted(inst) == [(S, ext) for S in LANES for ext in (0, 1)], sorted(inst)
    return inst


def check(ext):
    inst = instances()
    for S in LANES:
        key, r = (S, ext), inst[S, ext]
        print(key, r)
        assert r["VGPRs Spill"] == 0, (key, r)
        assert r["VGPRs"] + r["AGPRs"] <= 512, (key, r)        # __launch_bounds__(64)
        assert r["LDS Size [bytes/block]"] == 0, (key, r)
        assert r["Occupancy [waves/SIMD]"] >= (4 if ext == 0 and S <= 32 else 3), (key, r)


@needs_hipcc
def test_scs_solver_instances_are_all_there_and_spill_nothing():
    check(0)


@needs_hipcc
def test_scs_std_instances_are_all_there_and_spill_nothing():
    check(1)
