"""Build-time guard for csrc/r1cs_solve.hip, in the manner of tests/test_native_solve_regs.py: the
code-object remarks of r1cs_solve_kernel<S, EXT> must show all seven lane counts times the three
variants (0 = basic, 1 = the kinds of ZKMI_HINTS_STD, 2 = also the emulated product), and no instance
may spill a vector register.  The emulated arm keeps the images of up to eight operand limbs live
across records and twelve more inside the closing record: select chains over compile-time indices
hold them in registers (csrc/r1cs_plan.h: r1cs_pick / r1cs_put); a switch over the entries had put
them into scratch memory.  The scratch size must be the same in all three variants: whatever the
basic instance takes, none of it is the emulated arm's."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC) and not shutil.which("hipcc"), reason="hipcc missing")
def test_r1cs_solver_instances_are_all_there_and_spill_nothing():
    src = os.path.join(ROOT, "gnark_crypto_primitives_amd", "csrc", "r1cs_solve.hip")
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
        m = re.search(r"remark:.*\s(VGPRs|AGPRs|VGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)",
                      line)
        if m and cur and "r1cs_solve_kernel" in cur:
            seen.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    inst = {}
    for name, r in seen.items():
        m = re.search(r"r1cs_solve_kernelILi(\d+)ELi(\d)E", name)
        assert m, name
        inst[(int(m.group(1)), int(m.group(2)))] = r
    assert sorted(inst) == [(s, e) for s in (1, 2, 4, 8, 16, 32, 64) for e in (0, 1, 2)], sorted(inst)
    for key, r in sorted(inst.items()):
        print(key, r)
        assert r["VGPRs Spill"] == 0, (key, r)
        assert r["VGPRs"] + r["AGPRs"] <= 512, (key, r)        # __launch_bounds__(64)
        assert r["LDS Size [bytes/block]"] == 0, (key, r)       # no register array demoted to LDS
    # the emulated arm adds no scratch memory of its own
    for s in (1, 2, 4, 8, 16, 32, 64):
        assert inst[(s, 2)]["ScratchSize [bytes/lane]"] == inst[(s, 1)]["ScratchSize [bytes/lane]"], s
