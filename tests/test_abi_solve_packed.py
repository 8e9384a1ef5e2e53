"""zkmi_set_solve_waves_per_block at the C boundary, without a GPU (the method of
tests/test_abi_scs_solver.py): declared in include/zkmi.h, exported by libzkmi.so and bound in lib.py
with the header's argument count; 3 and 16 wavefronts per workgroup are refused on the host with
ZKMI_ERR_ARG (16 waves of the solve kernel cannot be resident on a compute unit), 0 restores the
default."""
import ctypes as C
import os
import re

import pytest

from gnark_crypto_primitives_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "zkmi_set_solve_waves_per_block"


def test_symbol_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "zkmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, src)
    assert decl, f"{NAME} is not declared in zkmi.h"
    assert len(decl.group(1).split(",")) == 2
    handle = lib.load()
    assert hasattr(handle, NAME), f"{NAME} missing from libzkmi.so"
    bound = {n: (res, args) for n, res, args in lib.SYMBOLS}
    assert bound[NAME] == (C.c_int, [C.c_void_p, C.c_int])
    assert callable(getattr(lib.Context, "set_solve_waves_per_block"))


def test_values_accepted_and_refused():
    """The setter reads nothing of the context and writes one int of it, so a block of zeros stands
    in for a context on a machine that has no device to make one on.  This assumes that zkmi_ctx
    (csrc/zkmi_internal.h: a few kilobytes of pointers, events and two pipeline sets) stays far
    below the 1 MiB of the block, and that the setter keeps to that one member: a setter that read or
    wrote anything else of the context would have to be tested on a real one (the GPU test
    tests/test_gpu_solve_packed.py::test_unsupported_block_sizes_are_refused is)."""
    handle = lib.load()
    fake = C.create_string_buffer(1 << 20)
    ctx = C.cast(fake, C.c_void_p)
    f = getattr(handle, NAME)
    for w in (1, 2, 4, 8):
        assert f(ctx, w) == 0, w
    for w in (3, 16, -1, 5, 6, 7, 9, 32, 64):
        assert f(ctx, w) == -1, w            # ZKMI_ERR_ARG
    # a refusal leaves the last accepted value in place: 8 is the only non-zero word of the block
    words = memoryview(fake.raw).cast("i")
    assert [v for v in words if v] == [8]
    assert f(ctx, 0) == 0                    # back to the default
    assert not any(memoryview(fake.raw).cast("i"))
    assert f(None, 1) == -1 and f(None, 0) == -1


def test_wrapper_raises_on_a_refused_value():
    class Ctx:
        h = None
        lib = lib.load()
    with pytest.raises(lib.ZkmiError, match=r"\(16\) refused \(-1\)"):
        lib.Context.set_solve_waves_per_block(Ctx(), 16)
