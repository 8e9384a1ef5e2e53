// The packed VLIW witness program: the one definition of the format that frontend/compile.py
// (build_vprogram) writes, zkmi_cs_load accepts and solve_vliw_kernel (solve.hip) runs.
// Host-compilable: tests/native/vprog_check.cpp runs the loader's checks without a GPU
// (tests/test_native_vprog.py, which also holds the Python constants against these).
//
// A program is n_rows rows of (1 + S) quads of four 32-bit words, S = sub-lanes per proof (a power
// of two, 1 .. 64): one header quad, then the operand quad of every sub-lane.
//
//   operand quad  (op | assert << 5 | class << 6 | k << 9, dst, a, b)
//     op      opcode, 5 bits; OP_END = idle sub-lane
//     assert  OP_ABC only: the solver checks a * b == c for this row
//     class   the step's class, 3 bits, in EVERY quad of a CLS_M .. CLS_BINV row, the idle ones
//             too: the kernel needs no header load for them.  Classes above 7 do not fit: their
//             quads carry 0 here and the kernel reads the class from the header.
//     k       the constraint row an emitting op writes (OP_MULABC, OP_XORABC, OP_ABC: every row
//             0 .. n_constraints - 1 exactly once per program); OP_FMA / OP_FMAC: the addend's slot
//     dst, a, b   value-file slots (slot i < n_wires is wire i), except: b is a constant index for
//             OP_MULC, OP_ADDC, OP_FMAC, OP_SETC; OP_ABC reads (dst, a, b) as the row's (a, b, c);
//             OP_BITS has b = count | width << 16
//   header quad   (class | VH_CONT on a unit's continuation rows, n, n rows, aux)
//
// Rows by class:
//   CLS_M     OP_MUL, OP_MULABC, OP_MULC, OP_FMA, OP_FMAC      dst = a * b (+ slot k)
//   CLS_X     OP_XORABC, OP_XOR              dst = a + b - 2ab; OP_XORABC emits the row (2a, b, 2ab)
//   CLS_A     OP_ADD, OP_SUB, OP_ADDC, OP_NEG, OP_COPY, OP_SETC
//   CLS_R     OP_ABC                         copies the operands of constraint k into a, b, c
//   CLS_I     OP_INV, OP_DIV (0 -> 0), and the byte-op hints OP_BXOR / OP_BAND on the low words of
//             the plain integers (the scheduler keeps those in steps of their own, CLS_B_SCHED,
//             which never appears in a program)
//   CLS_BITS  one OP_BITS in sub-lane 0: `count` limbs of `width` bits (width 0 / 1: bits) of slot a
//             into slots dst .., count * max(width, 1) <= 256; the sub-lanes split the limbs
//   CLS_LIMBS up to S short OP_BITS (count <= 16), one per sub-lane, class bits 0, idle quads all
//             zero, quad 0 active
//   CLS_BINV  unit: header (class, n pairs, n rows, 0), quads (class << 6); then n rows =
//             ceil(n pairs / S) continuation rows of (OP_PAIR, dst, src, 0) quads: dst = 1 / src
//             (0 -> 0) with one inversion per sub-lane.  The dst rows double as scratch: no dst is
//             any pair's src.
//   CLS_HIST  unit: header (class, n queries, n rows, table size), quad 0 = (OP_HIST, first wire),
//             other quads zero; then ceil(n / S) continuation rows of (OP_HQ, 0, query slot, 0),
//             packed without gaps: wire first + j = #{queries equal to j}, j < table size
//   CLS_EMUL  unit like CLS_HIST: header (class, na + nb, n rows, aux), quad 0 = (OP_EMUL, first
//             wire, 0, aux), aux = nout | na << 8 | first modulus constant << 12; the OP_HQ rows hold
//             the limb slots of a, then of b, least significant first.  a = sum a_i 2^(64 i) (a limb
//             may exceed 64 bits), b likewise, p = the four 64-bit constants: the nout - 4 limbs of
//             floor(a b / p), then the four of a b mod p, into consecutive wires (emul.h)
//   CLS_COMMIT  one row: header (class, n operands, 0, commitment index), quad 0 = (OP_COMMIT,
//             challenge wire, 0, index), indices 0, 1, .. in program order.  Never executed: the
//             host ends a kernel launch in front of it, commits, and writes the challenge.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>
#if defined(__HIPCC__)
#define ZK_VPROG_FN __host__ __device__ __forceinline__
#else
#define ZK_VPROG_FN inline
#endif

namespace zk {

enum { OP_END = 0, OP_ADD, OP_SUB, OP_MUL, OP_MULC, OP_ADDC, OP_NEG, OP_INV, OP_BITS, OP_SETC,
       OP_ABC, OP_COPY, OP_DIV, OP_BATCHINV, OP_PAIR, OP_MULABC, OP_XORABC, OP_XOR, OP_FMAC, OP_FMA,
       OP_HIST, OP_HQ, OP_COMMIT, OP_BXOR, OP_BAND, OP_EMUL };
enum { CLS_M = 1, CLS_X, CLS_A, CLS_R, CLS_I, CLS_BITS, CLS_BINV, CLS_HIST, CLS_COMMIT, CLS_B_SCHED,
       CLS_EMUL, CLS_LIMBS };

// operand quad, word 0
ZK_VPROG_FN uint32_t vq_op(uint32_t w) { return w & 0x1fu; }
ZK_VPROG_FN uint32_t vq_assert(uint32_t w) { return w & 0x20u; }
ZK_VPROG_FN uint32_t vq_cls(uint32_t w) { return (w >> 6) & 7u; }
ZK_VPROG_FN uint32_t vq_k(uint32_t w) { return w >> 9; }
// header quad, word 0
constexpr uint32_t VH_CONT = 0x100u;
ZK_VPROG_FN uint32_t vh_cls(uint32_t w) { return w & 0xffu; }
// OP_BITS, word 3
ZK_VPROG_FN uint32_t vbits_count(uint32_t w) { return w & 0xffffu; }
ZK_VPROG_FN uint32_t vbits_width(uint32_t w) { return w >> 16; }
// OP_EMUL aux
ZK_VPROG_FN uint32_t vemul_nout(uint32_t aux) { return aux & 0xffu; }
ZK_VPROG_FN uint32_t vemul_na(uint32_t aux) { return (aux >> 8) & 0xfu; }
ZK_VPROG_FN uint32_t vemul_const0(uint32_t aux) { return aux >> 12; }

// ---- the loader's checks (host only) ----
struct VprogShape {
  uint32_t n_wires, n_slots, n_consts, n_constraints, n_rows, S;
};

// The `nrows` continuation rows of the unit whose header is row r: header word 0 = cls | VH_CONT,
// then S quads; quad(i, q) sees quad i of the unit and returns false to refuse it.  Returns the
// refused row, or 0.
template <class F>
inline uint32_t vprog_walk_unit(const VprogShape& s, const uint32_t* p, uint32_t r, uint32_t cls,
                                uint32_t nrows, F quad) {
  const size_t stride = (size_t)(1 + s.S) * 4;
  for (uint32_t t = 1; t <= nrows; t++) {
    const uint32_t* hh = p + (size_t)(r + t) * stride;
    if (hh[0] != (cls | VH_CONT)) return r + t;
    for (uint32_t l = 0; l < s.S; l++)
      if (!quad((t - 1) * s.S + l, hh + 4 * (1 + l))) return r + t;
  }
  return 0;
}

// Every slot / constant / row index of a program, checked on the host before anything reaches a
// kernel that uses them as addresses.  Returns the empty string and the COMMIT rows (row, wire) in
// commitment order and whether the program holds OP_EMUL units, or what is wrong with it.
inline std::string vprog_validate(const VprogShape& s, const uint32_t* p,
                                  std::vector<std::pair<uint32_t, uint32_t>>* commit_rows,
                                  bool* has_emul) {
  const uint32_t S = s.S;
  if (S == 0 || S > 64 || (S & (S - 1))) return "cs: lanes_per_proof must be a power of two, 1 .. 64";
  commit_rows->clear();
  *has_emul = false;
  const size_t stride = (size_t)(1 + S) * 4;
  std::vector<uint8_t> row_seen(s.n_constraints, 0);
  uint32_t n_abc = 0;
  auto bad = [](uint32_t r) { return "cs: malformed program row " + std::to_string(r); };
  auto slot = [&](uint32_t i) { return i < s.n_slots; };
  auto cst = [&](uint32_t i) { return i < s.n_consts; };
  for (uint32_t r = 0; r < s.n_rows; r++) {
    const uint32_t* h = p + r * stride;
    const uint32_t cls = vh_cls(h[0]);
    if (h[0] & VH_CONT) return bad(r);   // a continuation row outside its unit
    if (cls == CLS_BINV || cls == CLS_HIST || cls == CLS_EMUL) {
      const uint32_t n = h[1], nrows = h[2], aux = h[3];
      const uint32_t* q0 = h + 4;
      if (nrows != (n + S - 1) / S || (uint64_t)r + nrows > (uint64_t)s.n_rows - 1) return bad(r);
      uint32_t at = 0;
      if (cls == CLS_BINV) {
        std::vector<uint32_t> dsts, srcs;
        at = vprog_walk_unit(s, p, r, cls, nrows, [&](uint32_t, const uint32_t* q) {
          if (vq_op(q[0]) == OP_END) return true;
          if (vq_op(q[0]) != OP_PAIR || !slot(q[1]) || !slot(q[2]) || q[1] == q[2]) return false;
          dsts.push_back(q[1]);
          srcs.push_back(q[2]);
          return true;
        });
        if (at) return bad(at);
        if (dsts.size() != n) return bad(r);
        std::sort(srcs.begin(), srcs.end());
        for (uint32_t x : dsts)   // no dst aliases any src (dst rows are the prefix scratch)
          if (std::binary_search(srcs.begin(), srcs.end(), x)) return bad(r);
      } else {
        if (cls == CLS_HIST) {
          if (q0[0] != OP_HIST || aux == 0 || (uint64_t)q0[1] + aux > s.n_wires) return bad(r);
        } else {
          const uint32_t nout = vemul_nout(aux), na = vemul_na(aux);
          if (q0[0] != OP_EMUL || q0[3] != aux || nout < 5 || nout > 12 || na < 1 || na > 4 ||
              n <= na || n - na > 4 || (uint64_t)q0[1] + nout > s.n_wires ||
              (uint64_t)vemul_const0(aux) + 4 > s.n_consts)
            return bad(r);
          *has_emul = true;
        }
        for (uint32_t l = 1; l < S; l++)
          if (h[4 * (1 + l)] != 0) return bad(r);
        uint32_t seen = 0;   // the queries fill the rows without gaps
        at = vprog_walk_unit(s, p, r, cls, nrows, [&](uint32_t i, const uint32_t* q) {
          if (q[0] == OP_END) return !(seen < n && i < n);
          if (q[0] != OP_HQ || !slot(q[2]) || i != seen) return false;
          seen++;
          return true;
        });
        if (at) return bad(at);
        if (seen != n) return bad(r);
      }
      r += nrows;
      continue;
    }
    if (cls == CLS_COMMIT) {
      const uint32_t* q0 = h + 4;
      if (q0[0] != OP_COMMIT || q0[1] >= s.n_wires || h[3] != commit_rows->size() || q0[3] != h[3])
        return bad(r);
      for (uint32_t l = 1; l < S; l++)
        if (h[4 * (1 + l)] != 0) return bad(r);
      commit_rows->emplace_back(r, q0[1]);
      continue;
    }
    if (cls == CLS_LIMBS) {
      bool any = false;
      for (uint32_t l = 0; l < S; l++) {
        const uint32_t* q = h + 4 * (1 + l);
        if (q[0] == 0 && q[1] == 0 && q[2] == 0 && q[3] == 0) {
          if (l == 0) return bad(r);   // the step's class is read from quad 0
          continue;
        }
        const uint32_t n = vbits_count(q[3]);
        if (q[0] != OP_BITS || n == 0 || n > 16 || vbits_width(q[3]) > 16 || !slot(q[2]) ||
            (uint64_t)q[1] + n > s.n_slots)
          return bad(r);
        any = true;
      }
      if (!any) return bad(r);
      continue;
    }
    if (cls < CLS_M || cls > CLS_BITS) return bad(r);
    for (uint32_t l = 0; l < S; l++) {
      const uint32_t* q = h + 4 * (1 + l);
      const uint32_t op = vq_op(q[0]), k = vq_k(q[0]), dst = q[1], a = q[2], b = q[3];
      if (vq_cls(q[0]) != cls) return bad(r);   // every quad carries its step's class
      if (op == OP_END) continue;
      bool ok = false, emits = false;
      switch (cls) {
        case CLS_M:
          emits = op == OP_MULABC;
          ok = (op == OP_MUL || op == OP_MULABC) ? (slot(dst) && slot(a) && slot(b))
               : op == OP_MULC                   ? (slot(dst) && slot(a) && cst(b))
               : op == OP_FMA                    ? (slot(dst) && slot(a) && slot(b) && slot(k))
               : op == OP_FMAC                   ? (slot(dst) && slot(a) && cst(b) && slot(k))
                                                 : false;
          break;
        case CLS_X:
          emits = op == OP_XORABC;
          ok = (op == OP_XORABC || op == OP_XOR) && slot(dst) && slot(a) && slot(b);
          break;
        case CLS_A:
          ok = (op == OP_ADD || op == OP_SUB)    ? (slot(dst) && slot(a) && slot(b))
               : op == OP_ADDC                   ? (slot(dst) && slot(a) && cst(b))
               : (op == OP_NEG || op == OP_COPY) ? (slot(dst) && slot(a))
               : op == OP_SETC                   ? (slot(dst) && cst(b))
                                                 : false;
          break;
        case CLS_R:
          emits = true;
          ok = op == OP_ABC && slot(dst) && slot(a) && slot(b);
          break;
        case CLS_I:
          ok = op == OP_INV ? (slot(dst) && slot(a))
               : (op == OP_DIV || op == OP_BXOR || op == OP_BAND) ? (slot(dst) && slot(a) && slot(b))
                                                                  : false;
          break;
        case CLS_BITS: {
          const uint32_t n = vbits_count(b), wd = vbits_width(b);
          ok = l == 0 && op == OP_BITS && slot(a) && wd <= 16 && n <= 256 &&
               (uint64_t)n * (wd ? wd : 1u) <= 256 && (uint64_t)dst + n <= s.n_slots;
          break;
        }
      }
      if (ok && emits) {
        ok = k < s.n_constraints && !row_seen[k];
        if (ok) {
          row_seen[k] = 1;
          n_abc++;
        }
      }
      if (!ok) return bad(r);
    }
  }
  if (n_abc != s.n_constraints)
    return "cs: program emits " + std::to_string(n_abc) + " constraint rows, expected " +
           std::to_string(s.n_constraints);
  return "";
}

}  // namespace zk
