"""ctypes binding of libzkmi.so (include/zkmi.h).  Loading fails loudly: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZKMI_LIB", os.path.join(_HERE, "libzkmi.so"))

ZKMI_OK = 0
ZKMI_ERR_UNSATISFIED = -5


class ZkmiError(RuntimeError):
    pass


class PkDesc(C.Structure):
    _fields_ = [("log_n", C.c_uint32), ("n_wires", C.c_uint32), ("n_a", C.c_uint32),
                ("n_b", C.c_uint32), ("n_k", C.c_uint32), ("n_z", C.c_uint32),
                ("a_wire", C.c_void_p), ("b_wire", C.c_void_p), ("k_wire", C.c_void_p),
                ("g1_a", C.c_void_p), ("g1_b", C.c_void_p), ("g1_k", C.c_void_p),
                ("g1_z", C.c_void_p), ("g2_b", C.c_void_p), ("g1_alpha", C.c_void_p),
                ("g1_beta", C.c_void_p), ("g1_delta", C.c_void_p), ("g2_beta", C.c_void_p),
                ("g2_delta", C.c_void_p), ("window_bits_g1", C.c_uint32),
                ("window_bits_g2", C.c_uint32),
                ("infinity_a", C.c_void_p), ("infinity_b", C.c_void_p), ("n_public", C.c_uint32),
                ("max_batch", C.c_uint32), ("table_budget_bytes", C.c_uint64),
                ("n_slots_hint", C.c_uint32), ("msm_chunk_factor", C.c_uint32),
                ("sparse_witness", C.c_uint32), ("n_commitments", C.c_uint32),
                ("commitments", C.c_void_p), ("fold_r1cs", C.c_void_p)]


class CommitmentDesc(C.Structure):
    _fields_ = [("n_private", C.c_uint32), ("n_hashed", C.c_uint32),
                ("commitment_wire", C.c_uint32), ("reserved", C.c_uint32),
                ("private_wires", C.c_void_p), ("hashed_wires", C.c_void_p),
                ("basis", C.c_void_p), ("basis_exp_sigma", C.c_void_p)]


class CsDesc(C.Structure):
    _fields_ = [("n_wires", C.c_uint32), ("n_public", C.c_uint32), ("n_secret", C.c_uint32),
                ("n_constraints", C.c_uint32), ("n_slots", C.c_uint32), ("n_rows", C.c_uint32),
                ("n_consts", C.c_uint32), ("lanes_per_proof", C.c_uint32), ("program", C.c_void_p),
                ("consts", C.c_void_p)]


class R1csDesc(C.Structure):
    _fields_ = [("n_wires", C.c_uint32), ("n_constraints", C.c_uint32), ("n_coeffs", C.c_uint32),
                ("coeffs", C.c_void_p), ("l_ptr", C.c_void_p), ("l_terms", C.c_void_p),
                ("r_ptr", C.c_void_p), ("r_terms", C.c_void_p), ("o_ptr", C.c_void_p),
                ("o_terms", C.c_void_p)]


class R1csSolverDesc(C.Structure):
    _fields_ = [("n_public", C.c_uint32), ("n_secret", C.c_uint32), ("n_instr", C.c_uint32),
                ("n_hints", C.c_uint32), ("instr", C.c_void_p), ("hint_kind", C.c_void_p),
                ("hint_in_ptr", C.c_void_p), ("hint_lc_ptr", C.c_void_p), ("hint_terms", C.c_void_p),
                ("hint_out_ptr", C.c_void_p), ("hint_out", C.c_void_p),
                ("lanes_per_proof", C.c_uint32), ("hint_set", C.c_uint32)]


class PlonkTraceDesc(C.Structure):
    _fields_ = [("log_n", C.c_uint32), ("n_public", C.c_uint32), ("selectors", C.c_void_p),
                ("perm", C.c_void_p), ("srs_g1", C.c_void_p), ("window_bits", C.c_uint32),
                ("max_batch", C.c_uint32), ("lag_g1", C.c_void_p * 3), ("lag_rows", C.c_void_p * 3),
                ("lag_k", C.c_uint32)]


class ScsDesc(C.Structure):
    _fields_ = [("n_wires", C.c_uint32), ("n_gates", C.c_uint32), ("n_public", C.c_uint32),
                ("xa", C.c_void_p), ("xb", C.c_void_p), ("xc", C.c_void_p),
                ("selectors", C.c_void_p)]


class ScsSolverDesc(C.Structure):
    _fields_ = [("n_inputs", C.c_uint32), ("input_wire", C.c_void_p), ("n_instr", C.c_uint32),
                ("n_hints", C.c_uint32), ("instr", C.c_void_p), ("hint_kind", C.c_void_p),
                ("hint_in_ptr", C.c_void_p), ("hint_in_wire", C.c_void_p),
                ("hint_in_coef", C.c_void_p), ("hint_out_ptr", C.c_void_p), ("hint_out", C.c_void_p),
                ("lanes_per_proof", C.c_uint32), ("hint_set", C.c_uint32)]


class PlonkCommitDesc(C.Structure):
    _fields_ = [("n_rows", C.c_uint32), ("row", C.c_uint32), ("rows", C.c_void_p),
                ("slots", C.c_void_p), ("lag_g1", C.c_void_p), ("lag_k", C.c_uint32)]


PLONK_MAX_COMMITMENTS = 8                               # ZKMI_PLONK_MAX_COMMITMENTS
HINTS_BASIC, HINTS_STD, HINTS_EMULATED = 0, 1, 3      # enum zkmi_hint_set (2 alone is not a set)


# every symbol include/zkmi.h declares: (name, restype, argtypes)
_P, _SZ, _I = C.c_void_p, C.c_size_t, C.c_int
SYMBOLS = [
    ("zkmi_init", _I, [_I, C.POINTER(_P)]),
    ("zkmi_destroy", None, [_P]),
    ("zkmi_last_error", C.c_char_p, [_P]),
    ("zkmi_sync", _I, [_P]),
    ("zkmi_stream", _P, [_P]),
    ("zkmi_field_mul", _I, [_P, _I, _P, _P, _P, _SZ]),
    ("zkmi_ff29_op", _I, [_P, _I, _I, _P, _P, _SZ]),
    ("zkmi_field_mul_bench", _I, [_P, _I, _SZ, _I, C.POINTER(C.c_double)]),
    ("zkmi_ntt_batch", _I, [_P, _P, _I, _SZ, _I, _I]),
    ("zkmi_h_batch", _I, [_P, _P, _P, _P, _P, _I, _SZ]),
    ("zkmi_ab_coset_batch", _I, [_P, _P, _P, _P, _I, _SZ]),
    ("zkmi_quotient_bases", _I, [_P, _P, _SZ, _I, _P, _P]),
    ("zkmi_msm_bases_load", _I, [_P, _I, _P, _SZ, _I, C.POINTER(_P)]),
    ("zkmi_msm_bases_free", None, [_P, _P]),
    ("zkmi_msm_batch", _I, [_P, _P, _P, _SZ, _P]),
    ("zkmi_msm_bases_load_image", _I, [_P, _I, _P, _SZ, _I, _I, C.POINTER(_P)]),
    ("zkmi_msm_batch_rows", _I, [_P, _P, _P, _SZ, _P, _SZ, _I, _I, _P]),
    ("zkmi_comb_min_groups_per_chunk", C.c_uint32, []),
    ("zkmi_fixed_base_mul", _I, [_P, _I, _P, _P, _SZ, _P]),
    ("zkmi_pk_load", _I, [_P, C.POINTER(PkDesc), C.POINTER(_P)]),
    ("zkmi_pk_free", None, [_P, _P]),
    ("zkmi_pk_load_planned", _I, [_P, C.POINTER(PkDesc), C.POINTER(C.c_uint32), C.POINTER(_P)]),
    ("zkmi_pk_info", _I, [_P, C.POINTER(C.c_uint64)]),
    ("zkmi_pk_msm_plan", _I, [_P, C.POINTER(C.c_uint32)]),
    ("zkmi_pk_folded", _I, [_P]),
    ("zkmi_cs_load", _I, [_P, C.POINTER(CsDesc), C.POINTER(_P)]),
    ("zkmi_cs_free", None, [_P, _P]),
    ("zkmi_solve_batch", _I, [_P, _P, _P, _SZ, _P, _P, _P]),
    ("zkmi_prove_batch", _I, [_P, _P, _P, _P, _SZ, _P, _P, _P]),
    ("zkmi_prove_submit", _I, [_P, _P, _P, _P, _SZ, _P]),
    ("zkmi_prove_collect", _I, [_P, _P, _P]),
    ("zkmi_prove_collect_ex", _I, [_P, _P, _P, _P]),
    ("zkmi_prove_witness_batch", _I, [_P, _P, _P, _P, _P, _P, _SZ, _SZ, _P, _P]),
    ("zkmi_host_alloc", _P, [_P, _SZ]),
    ("zkmi_host_free", None, [_P, _P]),
    ("zkmi_set_copy_threads", _I, [_P, _I]),
    ("zkmi_set_solve_waves_per_block", _I, [_P, _I]),
    ("zkmi_r1cs_load", _I, [_P, C.POINTER(R1csDesc), C.POINTER(_P)]),
    ("zkmi_r1cs_free", None, [_P, _P]),
    ("zkmi_prove_witness_submit", _I, [_P, _P, _P, _P, _P, _P, _P, _SZ, _SZ, _P]),
    ("zkmi_r1cs_solver_load", _I, [_P, _P, C.POINTER(R1csSolverDesc), C.POINTER(_P)]),
    ("zkmi_r1cs_solver_free", None, [_P, _P]),
    ("zkmi_r1cs_solver_info", _I, [_P, C.POINTER(C.c_uint64)]),
    ("zkmi_r1cs_solve_batch", _I, [_P, _P, _P, _SZ, _P, _P, _P]),
    ("zkmi_prove_r1cs_submit", _I, [_P, _P, _P, _P, _SZ, _P]),
    ("zkmi_last_timings", _I, [_P, C.POINTER(C.c_double)]),
    ("zkmi_plonk_pk_load", _I, [_P, _P, C.POINTER(_P)]),
    ("zkmi_plonk_pk_free", None, [_P, _P]),
    ("zkmi_plonk_round1", _I, [_P, _P, _P, _P, _SZ, _P, _P, _P]),
    ("zkmi_plonk_round2", _I, [_P, _P, _P, _P]),
    ("zkmi_plonk_round3", _I, [_P, _P, _P, _P]),
    ("zkmi_plonk_round4", _I, [_P, _P, _P, _P]),
    ("zkmi_plonk_round5", _I, [_P, _P, _P, _P]),
    ("zkmi_plonk_prove", _I, [_P, _P, _P, _P, _SZ, _P, _P, _P, _P]),
    ("zkmi_plonk_pk_load_trace", _I, [_P, C.POINTER(PlonkTraceDesc), C.POINTER(_P)]),
    ("zkmi_scs_load", _I, [_P, C.POINTER(ScsDesc), C.POINTER(_P)]),
    ("zkmi_scs_free", None, [_P, _P]),
    ("zkmi_plonk_round1_witness", _I, [_P, _P, _P, _P, _P, _P, _P, _SZ, _SZ, _P, _P, _P]),
    ("zkmi_plonk_prove_witness", _I, [_P, _P, _P, _P, _P, _P, _P, _SZ, _SZ, _P, _P, _P, _P]),
    ("zkmi_plonk_pk_set_commitments", _I, [_P, _P, C.POINTER(PlonkCommitDesc), C.c_uint32]),
    ("zkmi_plonk_commit_hint", _I, [_P, _P, C.c_uint32, _P, _P, _SZ, _P, _P]),
    ("zkmi_plonk_prove_ex", _I, [_P, _P, _P, _P, _SZ, _P, _P, _P, _P, _P, _P]),
    ("zkmi_plonk_prove_witness_ex", _I, [_P, _P, _P, _P, _P, _P, _P, _SZ, _SZ, _P, _P, _P, _P, _P,
                                         _P]),
    ("zkmi_scs_solver_load", _I, [_P, _P, C.POINTER(ScsSolverDesc), C.POINTER(_P)]),
    ("zkmi_scs_solver_free", None, [_P, _P]),
    ("zkmi_scs_solver_info", _I, [_P, C.POINTER(C.c_uint64)]),
    ("zkmi_scs_solve_batch", _I, [_P, _P, _P, _SZ, _P, _P]),
    ("zkmi_plonk_round1_scs", _I, [_P, _P, _P, _P, _SZ, _P, _P, _P]),
    ("zkmi_plonk_prove_scs", _I, [_P, _P, _P, _P, _SZ, _P, _P, _P, _P]),
    ("zkmi_plonk_prove_scs_ex", _I, [_P, _P, _P, _P, _SZ, _P, _P, _P, _P, _P, _P]),
]

_lib = None


def load():
    """dlopen libzkmi.so and bind every declared symbol; raises if the library is missing.
    A process that also uses torch on the GPU must import torch BEFORE this call: torch ships its
    own libamdhip64.so.7, and the HIP runtime loaded first serves every later library."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ZkmiError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as "
                        "g; g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)       # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(x):
    """numpy array / torch tensor / int -> raw address (host or device)."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        if not x.flags["C_CONTIGUOUS"]:
            raise ValueError("array must be C-contiguous")
        return x.ctypes.data
    if hasattr(x, "data_ptr"):
        if not x.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return x.data_ptr()
    return int(x)


class Context:
    """One per GPU (zkmi_init / zkmi_destroy)."""

    def __init__(self, device: int = 0):
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.zkmi_init(device, C.byref(h))
        if rc != 0:
            raise ZkmiError(f"zkmi_init(device={device}) failed with {rc} "
                            "(-3 = no HIP device: this library only runs on a GPU)")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.zkmi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.zkmi_last_error(self.h)
            raise ZkmiError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def sync(self):
        self._check(self.lib.zkmi_sync(self.h), "zkmi_sync")

    def stream(self) -> int:
        return self.lib.zkmi_stream(self.h) or 0

    # ---- primitives
    def field_mul(self, which, a, b, out=None):
        n = a.shape[0]
        out = np.empty_like(a) if out is None else out
        self._check(self.lib.zkmi_field_mul(self.h, which, _ptr(a), _ptr(b), _ptr(out), n),
                    "zkmi_field_mul")
        return out

    def ff29_op(self, field, op, operands, out=None):
        """operands: int32 [n][arity][9] raw limbs -> int32 [n][9] (zkmi_ff29_op)"""
        n = operands.shape[0]
        out = np.empty((n, 9), dtype=np.int32) if out is None else out
        self._check(self.lib.zkmi_ff29_op(self.h, field, op, _ptr(operands), _ptr(out), n),
                    "zkmi_ff29_op")
        return out

    def field_mul_bench(self, which=1, n_threads=1 << 20, iters=256) -> float:
        r = C.c_double()
        self._check(self.lib.zkmi_field_mul_bench(self.h, which, n_threads, iters, C.byref(r)),
                    "zkmi_field_mul_bench")
        return r.value

    def ntt_batch(self, data, log_n, batch, inverse=False, coset=False):
        self._check(self.lib.zkmi_ntt_batch(self.h, _ptr(data), log_n, batch, int(inverse),
                                            int(coset)), "zkmi_ntt_batch")
        return data

    def h_batch(self, a, b, c, out, log_n, batch):
        self._check(self.lib.zkmi_h_batch(self.h, _ptr(a), _ptr(b), _ptr(c), _ptr(out), log_n,
                                          batch), "zkmi_h_batch")
        return out

    def ab_coset_batch(self, a, b, out, log_n, batch):
        self._check(self.lib.zkmi_ab_coset_batch(self.h, _ptr(a), _ptr(b), _ptr(out), log_n, batch),
                    "zkmi_ab_coset_batch")
        return out

    def quotient_bases(self, g1_z, log_n):
        """(E, L): uint64 [2^log_n, 8] each, from g1_z [n_z >= 2^log_n - 1, 8] (zkmi_quotient_bases)"""
        n = 1 << log_n
        e, l = np.zeros((n, 8), dtype=np.uint64), np.zeros((n, 8), dtype=np.uint64)
        self._check(self.lib.zkmi_quotient_bases(self.h, _ptr(g1_z), g1_z.shape[0], log_n, _ptr(e),
                                                 _ptr(l)), "zkmi_quotient_bases")
        return e, l

    def msm_bases_load(self, group, bases, n, window_bits=0):
        h = C.c_void_p()
        self._check(self.lib.zkmi_msm_bases_load(self.h, group, _ptr(bases), n, window_bits,
                                                 C.byref(h)), "zkmi_msm_bases_load")
        return h

    def msm_bases_free(self, h):
        self.lib.zkmi_msm_bases_free(self.h, h)

    def msm_batch(self, bases_h, scalars, batch, out):
        self._check(self.lib.zkmi_msm_batch(self.h, bases_h, _ptr(scalars), batch, _ptr(out)),
                    "zkmi_msm_batch")
        return out

    def msm_bases_load_image(self, group, bases, n, window_bits, image):
        h = C.c_void_p()
        self._check(self.lib.zkmi_msm_bases_load_image(self.h, group, _ptr(bases), n, window_bits,
                                                       image, C.byref(h)),
                    "zkmi_msm_bases_load_image")
        return h

    def msm_batch_rows(self, bases_h, scalars, n_rows, row_idx, batch, image, uniform, out):
        self._check(self.lib.zkmi_msm_batch_rows(self.h, bases_h, _ptr(scalars), n_rows,
                                                 _ptr(row_idx), batch, image, uniform, _ptr(out)),
                    "zkmi_msm_batch_rows")
        return out

    def comb_min_groups_per_chunk(self):
        return int(self.lib.zkmi_comb_min_groups_per_chunk())

    def fixed_base_mul(self, group, base, scalars, n, out):
        self._check(self.lib.zkmi_fixed_base_mul(self.h, group, _ptr(base), _ptr(scalars), n,
                                                 _ptr(out)), "zkmi_fixed_base_mul")
        return out

    # ---- key / system handles
    def pk_load(self, desc: PkDesc, msm_window_bits=None):
        """msm_window_bits: window_bits of A, B1, K, Z, B2 (zkmi_pk_load_planned); None = the
        descriptor's window_bits_g1 / g2 or the auto plan"""
        h = C.c_void_p()
        if msm_window_bits is None:
            self._check(self.lib.zkmi_pk_load(self.h, C.byref(desc), C.byref(h)), "zkmi_pk_load")
        else:
            wb = (C.c_uint32 * 5)(*msm_window_bits)
            self._check(self.lib.zkmi_pk_load_planned(self.h, C.byref(desc), wb, C.byref(h)),
                        "zkmi_pk_load_planned")
        return h

    def pk_info(self, h):
        arr = (C.c_uint64 * 10)()
        self._check(self.lib.zkmi_pk_info(h, arr), "zkmi_pk_info")
        info = dict(zip(("g1_windows", "g1_entries_per_base", "g2_windows", "g2_entries_per_base",
                         "g1_table_bytes", "g2_table_bytes", "g1_shared", "g2_shared",
                         "g1_comb_k", "g2_comb_k"), [int(x) for x in arr]))
        # g1_* describe the quotient MSM's tables (Z); the comb plan of every MSM:
        plan = (C.c_uint32 * 10)()
        self._check(self.lib.zkmi_pk_msm_plan(h, plan), "zkmi_pk_msm_plan")
        info["msm_comb_k"] = dict(zip(("A", "B1", "K", "Z", "B2"), [int(x) for x in plan[:5]]))
        info["msm_comb_signed"] = dict(zip(("A", "B1", "K", "Z", "B2"), [int(x) for x in plan[5:]]))
        return info

    def pk_folded(self, h) -> bool:
        return bool(self.lib.zkmi_pk_folded(h))

    def pk_free(self, h):
        self.lib.zkmi_pk_free(self.h, h)

    def cs_load(self, desc: CsDesc):
        h = C.c_void_p()
        self._check(self.lib.zkmi_cs_load(self.h, C.byref(desc), C.byref(h)), "zkmi_cs_load")
        return h

    def cs_free(self, h):
        self.lib.zkmi_cs_free(self.h, h)

    def solve_batch(self, cs_h, inputs, batch, wires_out=None, abc_out=None, status_out=None):
        if status_out is None:
            status_out = np.zeros(batch, dtype=np.int32)
        self._check(self.lib.zkmi_solve_batch(self.h, cs_h, _ptr(inputs), batch, _ptr(wires_out),
                                              _ptr(abc_out), _ptr(status_out)), "zkmi_solve_batch")
        return status_out

    def prove_batch(self, pk_h, cs_h, inputs, batch, rs, proofs_out, status_out):
        self._check(self.lib.zkmi_prove_batch(self.h, pk_h, cs_h, _ptr(inputs), batch, _ptr(rs),
                                              _ptr(proofs_out), _ptr(status_out)),
                    "zkmi_prove_batch")

    def prove_submit(self, pk_h, cs_h, inputs, batch, rs):
        self._check(self.lib.zkmi_prove_submit(self.h, pk_h, cs_h, _ptr(inputs), batch, _ptr(rs)),
                    "zkmi_prove_submit")

    def prove_collect(self, proofs_out, status_out, commitments_out=None):
        if commitments_out is None:
            self._check(self.lib.zkmi_prove_collect(self.h, _ptr(proofs_out), _ptr(status_out)),
                        "zkmi_prove_collect")
        else:
            self._check(self.lib.zkmi_prove_collect_ex(self.h, _ptr(proofs_out), _ptr(status_out),
                                                       _ptr(commitments_out)),
                        "zkmi_prove_collect_ex")

    def prove_witness_batch(self, pk_h, wires, a, b, c, n_constraints, batch, rs, proofs_out):
        self._check(self.lib.zkmi_prove_witness_batch(self.h, pk_h, _ptr(wires), _ptr(a), _ptr(b),
                                                      _ptr(c), n_constraints, batch, _ptr(rs),
                                                      _ptr(proofs_out)),
                    "zkmi_prove_witness_batch")

    def prove_witness_submit(self, pk_h, r1cs_h, wires, a, b, c, n_constraints, batch, rs):
        self._check(self.lib.zkmi_prove_witness_submit(self.h, pk_h, r1cs_h, _ptr(wires), _ptr(a),
                                                       _ptr(b), _ptr(c), n_constraints, batch,
                                                       _ptr(rs)), "zkmi_prove_witness_submit")

    def r1cs_load(self, desc: "R1csDesc"):
        h = C.c_void_p()
        self._check(self.lib.zkmi_r1cs_load(self.h, C.byref(desc), C.byref(h)), "zkmi_r1cs_load")
        return h

    def r1cs_free(self, h):
        self.lib.zkmi_r1cs_free(self.h, h)

    def r1cs_solver_load(self, r1cs_h, desc: "R1csSolverDesc"):
        h = C.c_void_p()
        self._check(self.lib.zkmi_r1cs_solver_load(self.h, r1cs_h, C.byref(desc), C.byref(h)),
                    "zkmi_r1cs_solver_load")
        return h

    def r1cs_solver_free(self, h):
        self.lib.zkmi_r1cs_solver_free(self.h, h)

    def r1cs_solver_info(self, h):
        arr = (C.c_uint64 * 8)()
        self._check(self.lib.zkmi_r1cs_solver_info(h, arr), "zkmi_r1cs_solver_info")
        return dict(zip(("n_instr", "lanes_per_proof", "n_terms", "longest", "n_inversions",
                         "n_wires", "n_constraints", "n_inputs"), [int(x) for x in arr]))

    def r1cs_solve_batch(self, solver_h, inputs, batch, wires_out=None, abc_out=None,
                         status_out=None):
        if status_out is None:
            status_out = np.zeros(batch, dtype=np.int32)
        self._check(self.lib.zkmi_r1cs_solve_batch(self.h, solver_h, _ptr(inputs), batch,
                                                   _ptr(wires_out), _ptr(abc_out),
                                                   _ptr(status_out)), "zkmi_r1cs_solve_batch")
        return status_out

    def prove_r1cs_submit(self, pk_h, solver_h, inputs, batch, rs):
        self._check(self.lib.zkmi_prove_r1cs_submit(self.h, pk_h, solver_h, _ptr(inputs), batch,
                                                    _ptr(rs)), "zkmi_prove_r1cs_submit")

    def plonk_pk_load_trace(self, desc: "PlonkTraceDesc"):
        h = C.c_void_p()
        self._check(self.lib.zkmi_plonk_pk_load_trace(self.h, C.byref(desc), C.byref(h)),
                    "zkmi_plonk_pk_load_trace")
        return h

    def scs_load(self, desc: "ScsDesc"):
        h = C.c_void_p()
        self._check(self.lib.zkmi_scs_load(self.h, C.byref(desc), C.byref(h)), "zkmi_scs_load")
        return h

    def scs_free(self, h):
        self.lib.zkmi_scs_free(self.h, h)

    def scs_solver_load(self, scs_h, desc: "ScsSolverDesc"):
        h = C.c_void_p()
        self._check(self.lib.zkmi_scs_solver_load(self.h, scs_h, C.byref(desc), C.byref(h)),
                    "zkmi_scs_solver_load")
        return h

    def scs_solver_free(self, h):
        self.lib.zkmi_scs_solver_free(self.h, h)

    def scs_solver_info(self, h):
        arr = (C.c_uint64 * 8)()
        self._check(self.lib.zkmi_scs_solver_info(h, arr), "zkmi_scs_solver_info")
        return dict(zip(("n_instr", "lanes_per_proof", "n_records", "n_steps", "n_inversions",
                         "n_wires", "n_gates", "n_inputs"), [int(x) for x in arr]))

    def scs_solve_batch(self, solver_h, inputs, batch, wires_out=None, status_out=None):
        if status_out is None:
            status_out = np.zeros(batch, dtype=np.int32)
        self._check(self.lib.zkmi_scs_solve_batch(self.h, solver_h, _ptr(inputs), batch,
                                                  _ptr(wires_out), _ptr(status_out)),
                    "zkmi_scs_solve_batch")
        return status_out

    def host_alloc(self, shape, dtype=np.uint64):
        """numpy array over page-locked memory from zkmi_host_alloc (free with host_free)."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self.lib.zkmi_host_alloc(self.h, nbytes)
        if not p:
            raise ZkmiError(f"zkmi_host_alloc({nbytes}) failed")
        buf = (C.c_uint8 * nbytes).from_address(p)
        arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[arr.ctypes.data] = p
        return arr

    def host_free(self, arr):
        p = getattr(self, "_pinned", {}).pop(arr.ctypes.data, None)
        if p:
            self.lib.zkmi_host_free(self.h, p)

    def set_copy_threads(self, n):
        self._check(self.lib.zkmi_set_copy_threads(self.h, n), "zkmi_set_copy_threads")

    def set_solve_waves_per_block(self, w):
        """Wavefronts per workgroup of the solve kernel: 1, 2, 4 or 8; 0 restores the default."""
        rc = self.lib.zkmi_set_solve_waves_per_block(self.h, w)
        if rc != 0:
            raise ZkmiError(f"zkmi_set_solve_waves_per_block({w}) refused ({rc}): "
                            "0 (default), 1, 2, 4 or 8")

    def last_timings(self):
        arr = (C.c_double * 8)()
        self.lib.zkmi_last_timings(self.h, arr)
        return list(arr)
