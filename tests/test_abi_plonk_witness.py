"""The PLONK witness entry at the C boundary, without a GPU: zkmi_plonk_trace_desc and zkmi_scs_desc
as a C compiler lays out include/zkmi.h against their ctypes mirrors (the method of
tests/test_abi.py::test_struct_layouts_match_header), the new symbols exported and bound with the
argument counts of the header, and the entries refusing when there is no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from gnark_crypto_primitives_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"zkmi_plonk_pk_load_trace": 3, "zkmi_scs_load": 3, "zkmi_scs_free": 2,
       "zkmi_plonk_round1_witness": 12, "zkmi_plonk_prove_witness": 13}


def test_descriptor_layouts_match_header(tmp_path):
    structs = {"zkmi_plonk_trace_desc": lib.PlonkTraceDesc, "zkmi_scs_desc": lib.ScsDesc}
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "zkmi.h"', 'int main(void) {']
    for st, cls in structs.items():
        prog.append(f'printf("{st} %zu\\n", sizeof({st}));')
        prog += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f, _ in cls._fields_]
    prog += ['printf("perm %zu\\n", sizeof(*((zkmi_plonk_trace_desc*)0)->perm));', 'return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for st, cls in structs.items():
        assert int(out[st]) == C.sizeof(cls), st
        for f, _ in cls._fields_:
            assert int(out[f"{st}.{f}"]) == getattr(cls, f).offset, (st, f)
    assert out["perm"] == "4"                       # the one integer width of the permutation
    # the fields the trace form shares with the expanded descriptor carry the same names and types
    from gnark_crypto_primitives_amd import plonk
    old = dict(plonk.PlonkDesc._fields_)
    for f, t in lib.PlonkTraceDesc._fields_:
        if f not in ("selectors", "perm"):
            assert old[f] is t, f


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
    """No device, no context: nothing to load a key or a system into, and no CPU path behind the
    entries (the convention of tests/test_abi.py::test_no_cpu_fallback_without_gpu)."""
    import torch
    if torch.cuda.is_available():
        return
    handle = lib.load()
    h = C.c_void_p()
    assert handle.zkmi_init(0, C.byref(h)) == -3 and not h.value
    rec = np.zeros((1, 96), dtype=np.uint64)
    st = np.zeros(1, dtype=np.int32)
    assert handle.zkmi_plonk_prove_witness(None, None, None, None, None, None, None, 0, 1, None,
                                           None, rec.ctypes.data, st.ctypes.data) == -1
    assert not rec.any()
    handle.zkmi_scs_free(None, None)                # freeing nothing is allowed, as for the others
