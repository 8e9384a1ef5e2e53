"""Build-time guard for the packed instances of csrc/solve.hip, beside
tests/test_native_solve_regs.py, read from the remarks and from the generated assembly.

solve_vliw_packed_kernel<S, EMUL, 4> (two or four waves per workgroup, one per SIMD) issues its row
stores from the fixed accumulation registers a0..a31 in inline asm, untracked by the compiler, as the
one-wave kernel does: AGPRs = 32 exactly, and no instruction outside the asm blocks names an
accumulation register at all (an asm clobber reserves a register only at the asm statement, so the
count alone does not show whether the allocator put a value of its own into a0..a31).  The same
scan runs over the one-wave kernel.

solve_vliw_packed_kernel<S, EMUL, 8> (two waves per SIMD, 256 registers each) stores from VGPRs with
ordinary stores and must not touch accumulation registers anywhere: AGPRs = 0, nothing in the
assembly, inside asm blocks or outside.

Every packed instance: no VGPR spill, and exactly the scratch of the one-wave kernel at the same S
and EMUL (no new scratch)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
AGPR = re.compile(r"\ba\d+\b|\ba\[\d+:\d+\]|accvgpr")


def agpr_lines(asm_text):
    """{kernel symbol: (lines inside asm blocks that name an AGPR, such lines outside)}"""
    out, cur, inasm = {}, None, False
    for line in asm_text.splitlines():
        m = re.match(r"^(_ZN2zk\d+solve_vliw\w+):", line)
        if m:
            cur, inasm = m.group(1), False
            out[cur] = ([], [])
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
        if cur is None:
            continue
        if ";;#ASMSTART" in line:
            inasm = True
        elif ";;#ASMEND" in line:
            inasm = False
        else:
            code = line.split(";")[0]
            if AGPR.search(code):
                out[cur][0 if inasm else 1].append(code.strip())
    return out


def test_the_scan_sees_a_compiler_write_to_an_accumulation_register():
    text = "\n".join(["_ZN2zk24solve_vliw_packed_kernelILi16ELb0ELi8EEEvPKx:", "\ts_nop 0",
                      "\tv_accvgpr_write_b32 a6, v98", "\t;;#ASMSTART",
                      "\tglobal_store_dwordx4 v[2:3], a[0:3], off", "\t;;#ASMEND",
                      "\tv_add_u32_e32 v1, v2, v3 ; a0 in a comment", ".Lfunc_end0:",
                      "\tv_accvgpr_read_b32 v0, a1"])
    (inside, outside), = agpr_lines(text).values()
    assert inside == ["global_store_dwordx4 v[2:3], a[0:3], off"]
    assert outside == ["v_accvgpr_write_b32 a6, v98"]


@pytest.mark.skipif(not os.path.exists(HIPCC) and not shutil.which("hipcc"), reason="hipcc missing")
def test_packed_solver_kernels_registers_and_scratch(tmp_path):
    src = os.path.join(ROOT, "gnark_crypto_primitives_amd", "csrc", "solve.hip")
    asm = tmp_path / "solve.s"
    err = subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "-O3", "-std=c++17",
                          "--offload-arch=gfx950", "--offload-device-only", "-mllvm",
                          "-pragma-unroll-threshold=1000000",
                          "-Rpass-analysis=kernel-resource-usage", "-S", src, "-o", str(asm)],
                         capture_output=True, text=True, timeout=1500).stderr
    one, packed, cur = {}, {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|VGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if not (m and cur):
            continue
        k = re.search(r"solve_vliw_packed_kernelILi(\d+)ELb(\d)ELi(\d+)E", cur)
        if k:
            packed.setdefault(tuple(int(x) for x in k.groups()), {})[m.group(1)] = int(m.group(2))
        k = re.search(r"solve_vliw_kernelILi(\d+)ELb(\d)EE", cur)
        if k:
            one.setdefault(tuple(int(x) for x in k.groups()), {})[m.group(1)] = int(m.group(2))
    lanes = [(s, e) for s in (1, 2, 4, 8, 16, 32, 64) for e in (0, 1)]
    assert sorted(one) == lanes
    assert sorted(packed) == [(s, e, w) for s, e in lanes for w in (4, 8)]
    for (s, e, w), r in packed.items():
        assert r["VGPRs Spill"] == 0, (s, e, w, r)
        assert r["ScratchSize [bytes/lane]"] == one[(s, e)]["ScratchSize [bytes/lane]"], (s, e, w, r)
        assert r["AGPRs"] == (32 if w == 4 else 0), (s, e, w, r)
        assert r["VGPRs"] + r["AGPRs"] <= 512 // (w // 4), (s, e, w, r)   # resident: W / 4 waves per SIMD
    scan = agpr_lines(asm.read_text())
    assert len(scan) == len(one) + len(packed)
    for name, (inside, outside) in scan.items():
        assert not outside, (name, outside[:5])
        if re.search(r"packed_kernelILi\d+ELb\dELi8E", name):
            assert not inside, (name, inside[:5])
        else:
            assert inside, name     # the staged stores are there
