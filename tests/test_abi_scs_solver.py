"""The PLONK solver entry at the C boundary, without a GPU: zkmi_scs_solver_desc as a C compiler lays
out include/zkmi.h against its ctypes mirror (the method of tests/test_abi_plonk_witness.py), the new
symbols exported and bound with the argument counts of the header, and the entries refusing when
there is no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from gnark_crypto_primitives_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"zkmi_scs_solver_load": 4, "zkmi_scs_solver_free": 2, "zkmi_scs_solver_info": 2,
       "zkmi_scs_solve_batch": 6, "zkmi_plonk_round1_scs": 8, "zkmi_plonk_prove_scs": 9}


def test_descriptor_layout_matches_header(tmp_path):
    st, cls = "zkmi_scs_solver_desc", lib.ScsSolverDesc
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "zkmi.h"', 'int main(void) {',
            f'printf("{st} %zu\\n", sizeof({st}));']
    prog += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f, _ in cls._fields_]
    prog += [f'printf("{f} %zu\\n", sizeof(*(({st}*)0)->{f}));'
             for f in ("input_wire", "instr", "hint_kind", "hint_in_ptr", "hint_in_wire",
                       "hint_out_ptr", "hint_out")]
    prog += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out[st]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(out[f"{st}.{f}"]) == getattr(cls, f).offset, f
    for f in ("input_wire", "instr", "hint_kind", "hint_in_ptr", "hint_in_wire", "hint_out_ptr",
              "hint_out"):
        assert out[f] == "4", f                      # the one integer width of every index array
    # hint_set is the last field: a later hint set extends its values, not the layout
    assert cls._fields_[-1][0] == "hint_set" and cls._fields_[-2][0] == "lanes_per_proof"
    # the fields the two solver descriptors share carry the same names and types
    old = dict(lib.R1csSolverDesc._fields_)
    for f, t in cls._fields_:
        if f in old:
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
    """No device, no context: nothing to load a solver into, and no CPU path behind the entries."""
    import torch
    if torch.cuda.is_available():
        return
    handle = lib.load()
    h = C.c_void_p()
    assert handle.zkmi_init(0, C.byref(h)) == -3 and not h.value
    rec = np.zeros((1, 96), dtype=np.uint64)
    st = np.zeros(1, dtype=np.int32)
    s = C.c_void_p()
    assert handle.zkmi_scs_solver_load(None, None, None, C.byref(s)) == -1 and not s.value
    assert handle.zkmi_plonk_prove_scs(None, None, None, None, 1, None, None, rec.ctypes.data,
                                       st.ctypes.data) == -1
    assert handle.zkmi_plonk_round1_scs(None, None, None, None, 1, None, rec.ctypes.data,
                                        st.ctypes.data) == -1
    assert handle.zkmi_scs_solve_batch(None, None, None, 1, None, st.ctypes.data) == -1
    assert not rec.any()
    handle.zkmi_scs_solver_free(None, None)          # freeing nothing is allowed, as for the others
    info = (C.c_uint64 * 8)()
    assert handle.zkmi_scs_solver_info(None, info) == -1
