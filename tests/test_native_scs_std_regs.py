"""Build-time guard for csrc/scs_solve_std.hip, in the manner of tests/test_native_scs_solve_regs.py:
the code-object remarks of scs_std_kernel<S> must show all seven lane counts, no instance may spill a
vector register, and none may use LDS: bits and limbs under a per-lane index are chains of selects,
never an indexed register array.  Registers and scratch per lane are printed and recorded in
DESIGN.md §3.6.2, not asserted."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC) and not shutil.which("hipcc"), reason="hipcc missing")
def test_scs_std_instances_are_all_there_and_spill_nothing():
    src = os.path.join(ROOT, "gnark_crypto_primitives_amd", "csrc", "scs_solve_std.hip")
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
        if m and cur and "scs_std_kernel" in cur:
            seen.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    inst = {}
    for name, r in seen.items():
        m = re.search(r"scs_std_kernelILi(\d+)EE", name)
        assert m, name
        inst[int(m.group(1))] = r
    assert sorted(inst) == [1, 2, 4, 8, 16, 32, 64], sorted(inst)
    for key, r in sorted(inst.items()):
        print(key, r)
        assert r["VGPRs Spill"] == 0, (key, r)
        assert r["VGPRs"] + r["AGPRs"] <= 512, (key, r)        # __launch_bounds__(64)
        assert r["LDS Size [bytes/block]"] == 0, (key, r)
