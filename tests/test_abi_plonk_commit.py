"""The PLONK commitment entries at the C boundary, without a GPU: zkmi_plonk_commit_desc as a C
compiler lays out include/zkmi.h against its ctypes mirror, the new symbols exported and bound with
the argument counts of the header (the method of tests/test_abi_plonk_witness.py), and the entries
refusing when there is no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from gnark_crypto_primitives_amd import hash_to_field, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"zkmi_plonk_pk_set_commitments": 4, "zkmi_plonk_commit_hint": 8, "zkmi_plonk_prove_ex": 11,
       "zkmi_plonk_prove_witness_ex": 15}


def test_descriptor_layout_matches_header(tmp_path):
    st, cls = "zkmi_plonk_commit_desc", lib.PlonkCommitDesc
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "zkmi.h"', 'int main(void) {',
            f'printf("{st} %zu\\n", sizeof({st}));']
    prog += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f, _ in cls._fields_]
    prog += [f'printf("rows %zu\\n", sizeof(*(({st}*)0)->rows));',
             'printf("max %d\\n", ZKMI_PLONK_MAX_COMMITMENTS);', 'return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out[st]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(out[f"{st}.{f}"]) == getattr(cls, f).offset, f
    assert out["rows"] == "4" and int(out["max"]) == lib.PLONK_MAX_COMMITMENTS == 8
    # the constant of the host-compilable checks is the header's
    chk = open(os.path.join(ROOT, "gnark_crypto_primitives_amd", "csrc", "plonk_commit_check.h")).read()
    assert re.search(r"PLONK_MAX_COMMITMENTS\s*=\s*8\b", chk)
    assert hash_to_field.PLONK_DST == b"BSB22-Plonk"


def test_symbols_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "zkmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    handle = lib.load()
    bound = {n: args for n, _, args in lib.SYMBOLS}
    for name, n_args in NEW.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert decl, f"{name} is not declared in zkmi.h"
        assert len(decl.group(1).split(",")) == n_args, name
        assert hasattr(handle, name), f"{name} missing from libzkmi.so"
        assert len(bound[name]) == n_args, name


def test_entries_refuse_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        return
    handle = lib.load()
    h = C.c_void_p()
    assert handle.zkmi_init(0, C.byref(h)) == -3 and not h.value
    rec = np.zeros((1, 96), dtype=np.uint64)
    cm = np.zeros((1, 1, 12), dtype=np.uint64)
    st = np.zeros(1, dtype=np.int32)
    assert handle.zkmi_plonk_prove_ex(None, None, None, None, 1, None, None, None, rec.ctypes.data,
                                      cm.ctypes.data, st.ctypes.data) == -1
    assert handle.zkmi_plonk_prove_witness_ex(None, None, None, None, None, None, None, 0, 1, None,
                                              None, None, rec.ctypes.data, cm.ctypes.data,
                                              st.ctypes.data) == -1
    assert handle.zkmi_plonk_pk_set_commitments(None, None, None, 0) == -1
    assert handle.zkmi_plonk_commit_hint(None, None, 0, None, None, 1, None, None) == -1
    assert not rec.any() and not cm.any()
