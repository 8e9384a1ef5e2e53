"""zkmi_plonk_prove_scs_ex in the C ABI (no GPU needed): the library exports it, lib.py binds it with
as many arguments as include/zkmi.h declares, and without a context it refuses instead of running."""
import ctypes as C
import os
import re

from gnark_crypto_primitives_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "zkmi_plonk_prove_scs_ex"


def _declared_arguments(name):
    src = open(os.path.join(ROOT, "include", "zkmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name + " is not declared in zkmi.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_symbol_is_exported_and_bound_with_the_headers_arguments():
    args = _declared_arguments(NAME)
    assert len(args) == 11 and args[6].endswith("blind_commit") and args[9].endswith("commit_out")
    handle = lib.load()
    assert hasattr(handle, NAME)
    bound = {n: (res, a) for n, res, a in lib.SYMBOLS}
    assert NAME in bound
    res, a = bound[NAME]
    assert res is C.c_int and len(a) == len(args)
    # the twin without commitments has the same arguments but the two commitment pointers
    assert len(bound["zkmi_plonk_prove_scs"][1]) == len(a) - 2
    assert a[4] is C.c_size_t                                   # batch


def test_it_refuses_without_a_context():
    """no GPU, so no context: ZKMI_ERR_ARG, and nothing is written"""
    handle = lib.load()
    rec = (C.c_uint64 * 96)()
    status = (C.c_int32 * 1)(7)
    rc = getattr(handle, NAME)(None, None, None, None, 1, None, None, None, rec, None, status)
    assert rc == -1
    assert not any(rec) and status[0] == 7


def test_the_hint_set_travels_in_the_description():
    """ScsSolverDesc's last field is the hint set (enum zkmi_hint_set)"""
    assert lib.ScsSolverDesc._fields_[-1][0] == "hint_set"
