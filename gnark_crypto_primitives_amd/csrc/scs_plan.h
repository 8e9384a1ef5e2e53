// The solve plan of a gnark-shaped sparse constraint system (PLONK): the one definition of what
// zkmi_scs_solver_load builds from the loaded system (zkmi_scs_load: three wire columns, five
// selectors) and a zkmi_scs_solver_desc, and what scs_solve_kernel (scs_solve.hip) runs.
// Host-compilable: tests/native/scs_plan_check.cpp builds plans and interprets them without a GPU
// (tests/test_native_scs_plan.py).
//
// gnark's solver walks the instructions of a SparseR1CS once per witness and finds, at run time, the
// one wire of each gate that is not solved yet [UPSTREAM-RECALL].  Which wire that is depends on the
// system alone, so the builder does that walk once with a solved-wire bitmap.  The bitmap starts with
// the wires of input_wire; the ONE wire is not special, its gate qL x - 1 = 0 solves it.  A hint input
// is a single term (coef * wire, or a constant) because a variable of gnark's scs builder is a single
// term [UPSTREAM-RECALL]; parity with gnark is unpinned.
//
// A gate  qL a + qR b + qO c + qM a b + qC = 0  over the wires (xa, xb, xc) falls into one of
//   all known   every wire is solved: an assertion.  No record: scs_gate_kernel checks every gate
//               of the solved wires afterwards.
//   LIN         the unknown u takes no part in the product (qM = 0, or u is neither a nor b):
//               x = -rest / k, k = the sum of the linear selectors on u's positions (u may sit in
//               several, e.g. (d, d, d)); -1 / k is computed here, once.
//   DIV         u is exactly one of a, b and qM != 0: x = -rest / (k + qM other), one inversion per
//               proof; a zero divisor flags the proof ZKMI_ERR_UNSATISFIED.
// `rest` is made of known wires only.  The hints are two more classes: INVZERO (x = 1 / v, 0 for
// v = 0) and NBITS (wire outs[target + i] = bit j0 + i of the canonical value of v, in records of
// at most SCS_NBITS_CHUNK bits), v = coef * wire or coef.
//
// Levels and steps: an instruction's level is 1 + the highest level of the producers of the wires it
// reads (inputs: level 0).  The records of one level and one class are packed into steps of S =
// lanes_per_proof records; sub-lane s of a proof runs record s of the step, and a short step is padded
// with records that store nothing.  Hence the two guarantees the kernel relies on:
//   (1) no record of a step reads a wire that a record of the same step writes;
//   (2) every wire a record reads was written in an earlier step, or is an input.
//
// Record = two quads of 32-bit words:
//   quad 0  (wa, wb, wc, target)   the wires of columns a, b, c (hints: wa = the input wire) and the
//                                  wire solved (NBITS: the first entry of the record's outputs in outs)
//   quad 1  (ctl, coef, aux, 0)
//     ctl   bits 0 .. 9    marks (scs_check.h) of qL qR qO qM qC as `rest` takes them: a selector on
//                          a position of the unknown is marked zero; a marked selector takes no product
//           bits 10 .. 11  mark of K (below)
//           bits 12 .. 14  columns a, b, c are read
//           bit 15         the record stores (0: padding)
//           bits 16 .. 17  class, the same in every record of a step
//           bit 18         DIV: the known factor of the product is column a (the unknown sits in b)
//     coef  row of the coefficient table: six field elements qL qR qO qM qC K in gnark's image
//           (the loader lifts the first four to 2^261 images for the 29-bit products);
//           K: LIN -1 / k, DIV k
//     aux   NBITS: j0 | count << 16
//     word 3  0 for the four classes above; otherwise a class of ZKMI_HINTS_STD, which then stands
//             in place of bits 16 .. 17 (those read 0):
//       SK_LIMBS       like NBITS; aux = j0 | count << 16 | width << 24: wire outs[target + i] = bits
//                      [(j0 + i) width, (j0 + i + 1) width) of the canonical value of v
//       SK_BYTEOP      the two terms sit on positions a and b (a constant term: qC for a, K for b,
//                      both in gnark's image, marked like qC); aux = 1 XOR | 2 AND on the low 32 bits
//       SK_COUNT_ZERO  zeroes the rows of wires outs[target .. target + count), aux = count << 16:
//                      their low words are the counters of the lookup
//       SK_COUNT_Q     one query v: adds 1 to the counter of wire outs[target + v] when v < aux, the
//                      table's size (an atomic: queries of one step may meet on a counter)
//       SK_COUNT_END   reads the counters of outs[target .. target + count) back and stores their
//                      field images in place
//     The three COUNT classes are three levels: ZERO at level 1, a query at least one level above
//     ZERO and above its producer, END above every query; the output wires carry END's level.
// A commitment hint (ZKMI_HINT_COMMIT) has no record: the kernel never runs it.  Its wire's level is
// one above the highest level of its committed wires (and no lower than the level of the commitment
// before it), and that level is a barrier: ScsPlan::commits lists, per hint, the first step of the
// barrier level.  Every record at a lower level lies before that step, every record that reads the
// commitment wire behind it; the caller runs the steps up to it, forms the commitment, stores the
// challenge in the wire's row and goes on.
// The records end with S records of padding: the kernel fetches one step ahead.
//
// Every count the kernel loops over and every index it uses as an address comes out of
// scs_plan_build, which has checked it.
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/zkmi.h"
#include "r1cs_plan.h"
#include "scs_check.h"

namespace zk {

enum { SK_LIN = 0, SK_DIV = 1, SK_INVZERO = 2, SK_NBITS = 3,
       // ZKMI_HINTS_STD: in word 3 of quad 1
       SK_LIMBS = 4, SK_BYTEOP = 5, SK_COUNT_ZERO = 6, SK_COUNT_Q = 7, SK_COUNT_END = 8 };
constexpr uint32_t SCS_NONE = 0xffffffffu;      // input_wire: no gate reads it; hint_in_wire: a constant
constexpr uint32_t SCS_NBITS_CHUNK = 16;        // bits per NBITS record
enum {
  SCS_CTL_MARK_K = 10, SCS_CTL_READ = 12, SCS_CTL_STORE = 1u << 15, SCS_CTL_CLASS = 16,
  SCS_CTL_OTHER_A = 1u << 18,
  SCS_CTL_NO_TERMS = 0xfffu   // the five selectors and K marked zero
};
constexpr int SCS_COEF_ROW = 6;                 // field elements per row of the coefficient table

struct ScsRecord {
  uint32_t wa, wb, wc, target;
  uint32_t ctl, coef, aux, xcls;
};
// the class of a record: word 3 where it is set, else bits 16 .. 17 of ctl
inline uint32_t scs_record_class(const ScsRecord& r) { return r.xcls ? r.xcls : (r.ctl >> SCS_CTL_CLASS) & 3; }

struct ScsPlanIn {
  uint32_t n_wires = 0, n_gates = 0, n_public = 0;
  const uint32_t* x[3] = {};        // xa, xb, xc
  const Fr* sel = nullptr;          // 5 x n_gates, gnark's image, reduced
  const zkmi_scs_solver_desc* desc = nullptr;   // host arrays
};
struct ScsPlan {
  uint32_t S = 0, n_instr = 0, n_records = 0, n_steps = 0, n_levels = 0, n_inversions = 0;
  std::vector<ScsRecord> records;   // n_steps x S, then S of padding
  std::vector<Fr> coefs;            // rows of SCS_COEF_ROW; row 0 is all zero
  std::vector<uint32_t> outs;       // output wires of the NBITS records
  std::vector<uint32_t> input_wire; // n_inputs
  // ZKMI_HINTS_STD
  bool std_records = false;         // a record of a class from SK_LIMBS on: scs_solve_kernel<S, 1> runs the plan
  struct Commit {
    uint32_t instr, step, wire;     // the hint's instruction, the first step of its barrier level, its wire
    std::vector<uint32_t> wires;    // the committed wires, operand order
  };
  std::vector<Commit> commits;      // commitment i at [i]; steps do not decrease
};

// S for lanes_per_proof = 0: the power of two in 1 .. 16 nearest to the mean number of records per
// level (the smaller one when two are equally near)
inline uint32_t scs_auto_lanes(uint64_t n_records, uint32_t n_levels) {
  return r1cs_auto_lanes(n_records, n_levels);
}

// Returns the empty string and the plan, or what is wrong with the description.  max_set: the highest
// hint set the caller can run (zkmi_scs_solver_load: ZKMI_HINTS_STD).
inline std::string scs_plan_build(const ScsPlanIn& in, ScsPlan* out, uint32_t max_set = ZKMI_HINTS_BASIC) {
  const std::string pre = "scs solver: ";
  if (!in.desc || !in.x[0] || !in.x[1] || !in.x[2] || !in.sel) return pre + "null argument";
  const zkmi_scs_solver_desc& d = *in.desc;
  if (in.n_wires == 0 || in.n_wires == SCS_NONE || in.n_gates == 0 || in.n_gates > SCS_MAX_GATES)
    return pre + "the system needs 1 .. 2^32 - 2 wires and 1 .. 2^24 gates";
  uint32_t S = d.lanes_per_proof;
  if (S > 64 || (S & (S - 1))) return pre + "lanes_per_proof must be 0 (auto) or a power of two, 1 .. 64";
  if (d.hint_set != ZKMI_HINTS_BASIC && (max_set == ZKMI_HINTS_BASIC || d.hint_set != ZKMI_HINTS_STD))
    return pre + (max_set == ZKMI_HINTS_BASIC
                      ? "hint_set must be ZKMI_HINTS_BASIC (0): this entry solves InvZero and NBits hints only"
                      : "hint_set must be ZKMI_HINTS_BASIC (0) or ZKMI_HINTS_STD (1): this entry has no "
                        "other set (the emulated product, kind 7, is not solved here)");
  const bool std_set = d.hint_set == ZKMI_HINTS_STD;
  if (d.n_inputs < in.n_public || in.n_public > in.n_gates)
    return pre + "n_inputs = " + std::to_string(d.n_inputs) + " is inconsistent with the system's n_public = " +
           std::to_string(in.n_public) + " (the public inputs come first)";
  if (d.n_inputs && !d.input_wire) return pre + "input_wire is null";
  if (d.n_instr == 0 || !d.instr) return pre + "no instructions";
  if (d.n_hints && (!d.hint_kind || !d.hint_in_ptr || !d.hint_out_ptr)) return pre + "hint table: null array";
  uint32_t n_hin = 0, n_hout = 0;
  if (d.n_hints) {
    bool ok = d.hint_in_ptr[0] == 0 && d.hint_out_ptr[0] == 0;
    for (uint32_t h = 0; ok && h < d.n_hints; h++)
      ok = d.hint_in_ptr[h] <= d.hint_in_ptr[h + 1] && d.hint_out_ptr[h] <= d.hint_out_ptr[h + 1];
    if (ok) n_hin = d.hint_in_ptr[d.n_hints], n_hout = d.hint_out_ptr[d.n_hints];
    if (!ok || (n_hin && (!d.hint_in_wire || !d.hint_in_coef)) || (n_hout && !d.hint_out))
      return pre + "hint table: offsets are not monotone from 0, or a null array";
  }
  // the system (zkmi_scs_load has checked it too; a plan must not depend on that)
  static const char* cols[3] = {"xa", "xb", "xc"};
  for (int c = 0; c < 3; c++)
    for (uint32_t g = 0; g < in.n_gates; g++)
      if (in.x[c][g] >= in.n_wires)
        return pre + cols[c] + "[" + std::to_string(g) + "] = " + std::to_string(in.x[c][g]) +
               " is not a wire (n_wires = " + std::to_string(in.n_wires) + ")";

  std::vector<uint8_t> solved(in.n_wires, 0), gate_seen(in.n_gates, 0);
  std::vector<uint32_t> level(in.n_wires, 0);
  for (uint32_t i = 0; i < d.n_inputs; i++) {
    const uint32_t w = d.input_wire[i];
    if (w == SCS_NONE && i >= in.n_public) continue;
    if (w == SCS_NONE || w >= in.n_wires)
      return pre + "input_wire[" + std::to_string(i) + "] = " + std::to_string(w) + " is not a wire" +
             (w == SCS_NONE ? " (a public input has a gate that reads it)" : "");
    if (solved[w])
      return pre + "input_wire[" + std::to_string(i) + "] = " + std::to_string(w) + " repeats an earlier entry";
    if (i < in.n_public && in.x[0][i] != w)
      return pre + "input_wire[" + std::to_string(i) + "] = " + std::to_string(w) + " is not the wire of public gate " +
             std::to_string(i) + ", " + std::to_string(in.x[0][i]);
    solved[w] = 1;
  }

  struct Pending {
    uint32_t cls, level;
    ScsRecord r;
    uint32_t first_out, n_out;   // NBITS: the record's outputs in `houts`
    Fr coef[SCS_COEF_ROW];
  };
  std::vector<Pending> pend;
  std::vector<uint32_t> houts;
  std::vector<uint32_t> xouts;          // the outputs of the std hints: they follow the NBITS records' in outs
  std::vector<ScsPlan::Commit> commits; // .step: the barrier level until the records are packed
  uint32_t n_levels = 0;
  const Fr* hcoef = (const Fr*)d.hint_in_coef;
  const size_t ng = in.n_gates;
  for (uint32_t ii = 0; ii < d.n_instr; ii++) {
    const uint32_t ik = d.instr[2 * ii], idx = d.instr[2 * ii + 1];
    const std::string at = pre + "instruction " + std::to_string(ii);
    Pending p{};
    for (Fr& f : p.coef) f = Fr::zero();
    p.r.ctl = SCS_CTL_NO_TERMS;
    auto set_mark = [&](int q, uint32_t m) { p.r.ctl = (p.r.ctl & ~(3u << (2 * q))) | m << (2 * q); };
    uint32_t lv = 0;
    auto reads = [&](int col, uint32_t w) {
      p.r.ctl |= 1u << (SCS_CTL_READ + col);
      (col == 0 ? p.r.wa : col == 1 ? p.r.wb : p.r.wc) = w;
      lv = std::max(lv, level[w]);
    };
    if (ik == 1) {
      if (idx >= d.n_hints) return at + ": hint index " + std::to_string(idx) + " out of range";
      const uint32_t hk = d.hint_kind[idx];
      const std::string hat = at + " (hint " + std::to_string(idx) + ")";
      if (hk >= ZKMI_HINT_LIMBS && hk <= ZKMI_HINT_EMULMUL && (!std_set || hk == ZKMI_HINT_EMULMUL))
        return hat + ": hints " + r1cs_hint_name(hk) + " are not supported on this entry";
      if (hk == 0 || hk > ZKMI_HINT_EMULMUL)
        return hat + ": hints " + r1cs_hint_name(hk) + " (" + std::to_string(hk) + ") are not supported on this entry";
      const uint32_t in0 = d.hint_in_ptr[idx], nin = d.hint_in_ptr[idx + 1] - in0;
      const uint32_t o0 = d.hint_out_ptr[idx], nout = d.hint_out_ptr[idx + 1] - o0;
      const std::string name = r1cs_hint_name(hk);
      if (hk >= ZKMI_HINT_LIMBS) {
        // ---- ZKMI_HINTS_STD: p0, a constant, then the operands --------------------------------------
        if (nin == 0) return hat + ": " + name + " takes a parameter p0 as its first input";
        if (d.hint_in_wire[in0] != SCS_NONE)
          return hat + ": " + name + ": the parameter p0 reads wire " + std::to_string(d.hint_in_wire[in0]) +
                 "; it must be a constant";
        for (uint32_t t = in0; t < in0 + nin; t++) {
          if (!fr_is_reduced(hcoef[t])) return hat + ": the coefficient of input " + std::to_string(t - in0) + " is not reduced mod r";
          const uint32_t w = d.hint_in_wire[t];
          if (w == SCS_NONE) continue;
          if (w >= in.n_wires) return hat + ": input wire " + std::to_string(w) + " out of range";
          if (!solved[w]) return hat + ": reads wire " + std::to_string(w) + ", which is not solved yet";
        }
        const Fr p0f = from_mont(hcoef[in0]);
        const bool p0_small = !(p0f.v[1] | p0f.v[2] | p0f.v[3] | p0f.v[4] | p0f.v[5] | p0f.v[6] | p0f.v[7]);
        const uint32_t p0 = p0_small ? p0f.v[0] : 0xffffffffu;
        for (uint32_t o = o0; o < o0 + nout; o++) {
          const uint32_t wire = d.hint_out[o];
          if (wire >= in.n_wires) return hat + ": output wire " + std::to_string(wire) + " out of range";
          if (solved[wire]) return hat + ": output wire " + std::to_string(wire) + " is already solved";
          solved[wire] = 1;   // (a wire twice among the outputs is "already solved" at its second entry)
        }
        // term t of the hint on position col: coef * wire through the selector, a constant through
        // qC (col 0) or K (col 1)
        auto term = [&](uint32_t t, int col) {
          const uint32_t w = d.hint_in_wire[t];
          const Fr k = hcoef[t];
          if (w == SCS_NONE) {
            const int q = col == 0 ? 4 : 5;
            p.coef[q] = k;
            const uint32_t m = scs_mark(k) == SCS_MARK_ZERO ? SCS_MARK_ZERO : SCS_MARK_GENERAL;
            if (q == 4) set_mark(4, m);
            else p.r.ctl = (p.r.ctl & ~(3u << SCS_CTL_MARK_K)) | m << SCS_CTL_MARK_K;
          } else {
            p.coef[col] = k;
            set_mark(col, scs_mark(k));
            if (scs_mark(k) != SCS_MARK_ZERO) reads(col, w);
            else lv = std::max(lv, level[w]);
          }
        };
        auto set_levels = [&](uint32_t l) {
          for (uint32_t o = o0; o < o0 + nout; o++) level[d.hint_out[o]] = l;
          n_levels = std::max(n_levels, l);
        };
        // the outputs [j0, j0 + cnt) of the hint as one record of class cls; `first` = the hint's
        // first entry in xouts
        auto chunks = [&](uint32_t cls, uint32_t first, uint32_t aux_hi) {
          p.cls = cls;
          for (uint32_t j0 = 0; j0 < nout; j0 += SCS_NBITS_CHUNK) {
            const uint32_t cnt = std::min(SCS_NBITS_CHUNK, nout - j0);
            p.first_out = first + j0;
            p.r.aux = (cls == SK_LIMBS ? j0 : 0) | cnt << 16 | aux_hi;
            pend.push_back(p);
          }
        };
        if (hk == ZKMI_HINT_LIMBS) {
          if (nin != 2 || nout == 0) return hat + ": " + name + " takes p0 = the width and one value, and has outputs";
          if (p0 < 1 || p0 > 64) return hat + ": " + name + ": the width p0 must be in 1 .. 64";
          if (nout > 0xffffu) return hat + ": " + name + " with more than 65535 outputs";
          term(in0 + 1, 0);
          const uint32_t first = (uint32_t)xouts.size();
          xouts.insert(xouts.end(), d.hint_out + o0, d.hint_out + o0 + nout);
          p.level = lv + 1;
          p.r.ctl |= SCS_CTL_STORE;
          chunks(SK_LIMBS, first, p0 << 24);
          set_levels(lv + 1);
        } else if (hk == ZKMI_HINT_BYTEOP) {
          if (nin != 3 || nout != 1) return hat + ": " + name + " takes p0 = the operation and two values, and has one output";
          if (p0 != 1 && p0 != 2) return hat + ": " + name + ": the operation p0 must be 1 (XOR) or 2 (AND)";
          term(in0 + 1, 0);
          term(in0 + 2, 1);
          p.cls = SK_BYTEOP;
          p.level = lv + 1;
          p.r.ctl |= SCS_CTL_STORE;
          p.r.target = d.hint_out[o0];
          p.r.aux = p0;
          pend.push_back(p);
          set_levels(lv + 1);
        } else if (hk == ZKMI_HINT_COUNT) {
          if (nout == 0 || p0 != nout)
            return hat + ": " + name + ": the table size p0 must be the number of outputs, " + std::to_string(nout);
          const uint32_t first = (uint32_t)xouts.size();
          xouts.insert(xouts.end(), d.hint_out + o0, d.hint_out + o0 + nout);
          const Pending blank = p;
          p.level = 1;
          p.r.ctl |= SCS_CTL_STORE;
          chunks(SK_COUNT_ZERO, first, 0);
          uint32_t top = 1;
          for (uint32_t t = in0 + 1; t < in0 + nin; t++) {
            p = blank;
            lv = 0;
            term(t, 0);
            p.cls = SK_COUNT_Q;
            p.level = std::max(lv + 1, 2u);
            p.r.ctl |= SCS_CTL_STORE;
            p.first_out = first;
            p.r.aux = nout;
            pend.push_back(p);
            top = std::max(top, p.level);
          }
          p = blank;
          p.level = top + 1;
          p.r.ctl |= SCS_CTL_STORE;
          chunks(SK_COUNT_END, first, 0);
          set_levels(top + 1);
        } else {   // ZKMI_HINT_COMMIT
          if (nin < 2 || nout != 1) return hat + ": " + name + " takes p0 = its index and the committed wires, and has one output";
          if (p0 != commits.size())
            return hat + ": " + name + ": the index p0 must count the commitment hints in instruction order, here " +
                   std::to_string(commits.size());
          if (commits.size() >= ZKMI_PLONK_MAX_COMMITMENTS)
            return hat + ": " + name + ": more than " + std::to_string(ZKMI_PLONK_MAX_COMMITMENTS) + " commitments";
          ScsPlan::Commit c;
          c.instr = ii;
          c.wire = d.hint_out[o0];
          uint32_t l = commits.empty() ? 0 : level[commits.back().wire] - 1;
          for (uint32_t t = in0 + 1; t < in0 + nin; t++) {
            const uint32_t w = d.hint_in_wire[t];
            if (w == SCS_NONE || !(hcoef[t] == Fr::one()))
              return hat + ": " + name + ": operand " + std::to_string(t - in0 - 1) + " must be a wire with coefficient 1";
            c.wires.push_back(w);
            l = std::max(l, level[w]);
          }
          c.step = l + 1;   // the barrier level; its first step once the records are packed
          commits.push_back(c);
          set_levels(l + 1);
        }
        continue;
      }
      if (nin != 1 || nout == 0 || (hk == ZKMI_HINT_INVZERO && nout != 1))
        return hat + ": " + name + " takes one input" +
               (hk == ZKMI_HINT_INVZERO ? " and has one output" : " and has outputs");
      if (hk == ZKMI_HINT_NBITS && nout > 0xffffu) return hat + ": NBits with more than 65535 outputs";
      const uint32_t w = d.hint_in_wire[in0];
      const Fr k = hcoef[in0];
      if (!fr_is_reduced(k)) return hat + ": the input's coefficient is not reduced mod r";
      if (w == SCS_NONE) {
        p.coef[4] = k;
        set_mark(4, scs_mark(k) == SCS_MARK_ZERO ? SCS_MARK_ZERO : SCS_MARK_GENERAL);
      } else {
        if (w >= in.n_wires) return hat + ": input wire " + std::to_string(w) + " out of range";
        if (!solved[w]) return hat + ": reads wire " + std::to_string(w) + ", which is not solved yet";
        p.coef[0] = k;
        set_mark(0, scs_mark(k));
        if (scs_mark(k) != SCS_MARK_ZERO) reads(0, w);
      }
      for (uint32_t o = o0; o < o0 + nout; o++) {
        const uint32_t wire = d.hint_out[o];
        if (wire >= in.n_wires) return hat + ": output wire " + std::to_string(wire) + " out of range";
        if (solved[wire]) return hat + ": output wire " + std::to_string(wire) + " is already solved";
        solved[wire] = 1;
        level[wire] = lv + 1;
      }
      p.level = lv + 1;
      p.r.ctl |= SCS_CTL_STORE;
      if (hk == ZKMI_HINT_INVZERO) {
        p.cls = SK_INVZERO;
        p.r.target = d.hint_out[o0];
        pend.push_back(p);
      } else {
        p.cls = SK_NBITS;
        for (uint32_t j0 = 0; j0 < nout; j0 += SCS_NBITS_CHUNK) {
          const uint32_t cnt = std::min(SCS_NBITS_CHUNK, nout - j0);
          p.first_out = (uint32_t)houts.size();
          p.n_out = cnt;
          p.r.aux = j0 | cnt << 16;
          houts.insert(houts.end(), d.hint_out + o0 + j0, d.hint_out + o0 + j0 + cnt);
          pend.push_back(p);
        }
      }
    } else if (ik == 0) {
      if (idx >= in.n_gates) return at + ": gate index " + std::to_string(idx) + " out of range";
      const std::string gat = at + " (gate " + std::to_string(idx) + ")";
      if (gate_seen[idx]) return gat + ": the gate occurs twice";
      gate_seen[idx] = 1;
      const uint32_t pos[3] = {in.x[0][idx], in.x[1][idx], in.x[2][idx]};
      int64_t unk = -1;
      for (uint32_t w : pos) {
        if (solved[w]) continue;
        if (unk >= 0 && (uint32_t)unk != w)
          return gat + ": two unknown wires (" + std::to_string(unk) + ", " + std::to_string(w) + ")";
        unk = w;
      }
      if (unk < 0) continue;   // an assertion: scs_gate_kernel checks it
      if (idx < in.n_public)
        return gat + ": the wire of a public gate is not among input_wire";
      const uint32_t u = (uint32_t)unk;
      Fr q[5];
      for (int s = 0; s < 5; s++) {
        q[s] = in.sel[(size_t)s * ng + idx];
        if (!fr_is_reduced(q[s]))
          return gat + ": selector " + std::to_string(s) + " is not reduced mod r";
      }
      const bool in_a = pos[0] == u, in_b = pos[1] == u, product = !q[3].is_zero();
      if (product && in_a && in_b)
        return gat + ": the unknown wire " + std::to_string(u) + " is both factors of the product (qM != 0)";
      Fr k = Fr::zero();
      for (int s = 0; s < 3; s++) {
        if (pos[s] == u) {
          k = add(k, q[s]);
          continue;
        }
        p.coef[s] = q[s];
        set_mark(s, scs_mark(q[s]));
        if (scs_mark(q[s]) != SCS_MARK_ZERO) reads(s, pos[s]);
      }
      p.coef[4] = q[4];
      set_mark(4, scs_mark(q[4]) == SCS_MARK_ZERO ? SCS_MARK_ZERO : SCS_MARK_GENERAL);
      if (product && (in_a || in_b)) {
        p.cls = SK_DIV;
        p.coef[3] = q[3];
        set_mark(3, scs_mark(q[3]));
        reads(in_a ? 1 : 0, pos[in_a ? 1 : 0]);
        if (in_b) p.r.ctl |= SCS_CTL_OTHER_A;
        p.coef[5] = k;
        p.r.ctl = (p.r.ctl & ~(3u << SCS_CTL_MARK_K)) | scs_mark(k) << SCS_CTL_MARK_K;
      } else {
        p.cls = SK_LIN;
        if (k.is_zero()) return gat + ": the unknown wire " + std::to_string(u) + " has coefficient 0";
        if (product) {
          p.coef[3] = q[3];
          set_mark(3, scs_mark(q[3]));
          reads(0, pos[0]);
          reads(1, pos[1]);
        }
        const Fr kk = neg(inverse(k));
        p.coef[5] = kk;
        p.r.ctl = (p.r.ctl & ~(3u << SCS_CTL_MARK_K)) | scs_mark(kk) << SCS_CTL_MARK_K;
      }
      p.r.target = u;
      p.r.ctl |= SCS_CTL_STORE;
      p.level = lv + 1;
      solved[u] = 1;
      level[u] = lv + 1;
      pend.push_back(p);
    } else {
      return at + ": kind " + std::to_string(ik) + " is neither a gate (0) nor a hint (1)";
    }
    n_levels = std::max(n_levels, lv + 1);
  }
  for (uint32_t g = 0; g < in.n_gates; g++)
    if (!gate_seen[g]) return pre + "gate " + std::to_string(g) + " occurs in no instruction";
  for (uint32_t w = 0; w < in.n_wires; w++)
    if (!solved[w]) return pre + "wire " + std::to_string(w) + " is still unsolved after the last instruction";

  if (S == 0) S = scs_auto_lanes(pend.size(), n_levels ? n_levels : 1);
  std::vector<uint32_t> order(pend.size());
  for (uint32_t i = 0; i < order.size(); i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    return pend[a].level != pend[b].level ? pend[a].level < pend[b].level : pend[a].cls < pend[b].cls;
  });
  ScsPlan& P = *out;
  P = ScsPlan();
  P.S = S;
  P.n_instr = d.n_instr;
  P.n_records = (uint32_t)pend.size();
  P.n_levels = n_levels;
  P.input_wire.assign(d.input_wire, d.input_wire + d.n_inputs);
  P.coefs.assign(SCS_COEF_ROW, Fr::zero());
  std::map<std::array<uint32_t, 8 * SCS_COEF_ROW>, uint32_t> rows;
  {
    std::array<uint32_t, 8 * SCS_COEF_ROW> zero{};
    rows[zero] = 0;
  }
  auto pad_to_step = [&](uint32_t cls) {
    while (P.records.size() % S)
      P.records.push_back(ScsRecord{0, 0, 0, 0, SCS_CTL_NO_TERMS | (cls < SK_LIMBS ? cls : 0) << SCS_CTL_CLASS,
                                    0, 0, cls < SK_LIMBS ? 0 : cls});
  };
  uint32_t nbits_outs = 0;
  for (const Pending& p : pend)
    if (p.cls == SK_NBITS) nbits_outs += p.n_out;
  std::vector<std::pair<uint32_t, uint32_t>> level_step;   // (level, its first step), increasing
  for (size_t i = 0; i < order.size(); i++) {
    Pending& p = pend[order[i]];
    if (i && (pend[order[i - 1]].level != p.level || pend[order[i - 1]].cls != p.cls))
      pad_to_step(pend[order[i - 1]].cls);
    if (level_step.empty() || level_step.back().first != p.level)
      level_step.emplace_back(p.level, (uint32_t)(P.records.size() / S));
    if ((uint64_t)P.records.size() + 2 * S > 0xffffffffull) return pre + "more than 2^32 plan records";
    std::array<uint32_t, 8 * SCS_COEF_ROW> key;
    for (int s = 0; s < SCS_COEF_ROW; s++)
      for (int t = 0; t < 8; t++) key[8 * s + t] = p.coef[s].v[t];
    auto it = rows.find(key);
    if (it == rows.end()) {
      it = rows.emplace(key, (uint32_t)(P.coefs.size() / SCS_COEF_ROW)).first;
      P.coefs.insert(P.coefs.end(), p.coef, p.coef + SCS_COEF_ROW);
    }
    p.r.coef = it->second;
    if (p.cls < SK_LIMBS) {
      p.r.ctl |= p.cls << SCS_CTL_CLASS;
    } else {
      p.r.xcls = p.cls;
      P.std_records = true;
      if (p.cls != SK_BYTEOP) p.r.target = nbits_outs + p.first_out;
    }
    if (p.cls == SK_NBITS) {
      p.r.target = (uint32_t)P.outs.size();
      P.outs.insert(P.outs.end(), houts.begin() + p.first_out, houts.begin() + p.first_out + p.n_out);
    }
    if (p.cls == SK_DIV || p.cls == SK_INVZERO) P.n_inversions++;
    P.records.push_back(p.r);
  }
  if (!order.empty()) pad_to_step(pend[order.back()].cls);
  P.n_steps = (uint32_t)(P.records.size() / S);
  for (uint32_t s = 0; s < S; s++)
    P.records.push_back(ScsRecord{0, 0, 0, 0, SCS_CTL_NO_TERMS, 0, 0, 0});
  P.outs.insert(P.outs.end(), xouts.begin(), xouts.end());
  for (ScsPlan::Commit& c : commits) {
    const uint32_t barrier = c.step;
    c.step = P.n_steps;
    for (const auto& ls : level_step)
      if (ls.first >= barrier) {
        c.step = ls.second;
        break;
      }
  }
  P.commits = std::move(commits);
  return "";
}

// What a record computes, on the host (the device's twin is scs_solve_kernel, scs_solve.hip):
// `ld(w)` reads a wire, `st(w, v)` stores one; returns false when the record divides by zero.  coefs:
// the plan's table in gnark's image.  A lookup counter is the low word of its wire's row, as on the
// device: COUNT_Q reads the row and stores it back with that word one higher.
template <class Load, class Store>
inline bool scs_record_run(const ScsRecord& r, const Fr* coefs, const uint32_t* outs, Load ld, Store st) {
  const Fr* q = coefs + (size_t)r.coef * SCS_COEF_ROW;
  const uint32_t cls = scs_record_class(r);
  auto term = [&](uint32_t mark, const Fr& x, const Fr& k) {
    return mark == SCS_MARK_ZERO ? Fr::zero() : mark == SCS_MARK_ONE ? x : mark == SCS_MARK_MINUS_ONE ? neg(x) : mul(x, k);
  };
  const Fr zero = Fr::zero();
  const Fr va = r.ctl >> SCS_CTL_READ & 1 ? ld(r.wa) : zero, vb = r.ctl >> (SCS_CTL_READ + 1) & 1 ? ld(r.wb) : zero,
           vc = r.ctl >> (SCS_CTL_READ + 2) & 1 ? ld(r.wc) : zero;
  const Fr ta = term(r.ctl & 3, va, q[0]), tb = term((r.ctl >> 2) & 3, vb, q[1]);
  Fr rest = add(add(ta, tb), term((r.ctl >> 4) & 3, vc, q[2]));
  if (((r.ctl >> 8) & 3) != SCS_MARK_ZERO) rest = add(rest, q[4]);
  const uint32_t mm = (r.ctl >> 6) & 3, mk = (r.ctl >> SCS_CTL_MARK_K) & 3;
  const bool store = r.ctl & SCS_CTL_STORE;
  bool ok = true;
  if (cls == SK_LIN) {
    if (mm != SCS_MARK_ZERO) rest = add(rest, term(mm, mul(va, vb), q[3]));
    if (store) st(r.target, term(mk, rest, q[5]));
  } else if (cls == SK_DIV) {
    const Fr den = add(mk == SCS_MARK_ZERO ? zero : q[5], term(mm, r.ctl & SCS_CTL_OTHER_A ? va : vb, q[3]));
    if (store) {
      ok = !den.is_zero();
      st(r.target, neg(mul(rest, inverse(den))));
    }
  } else if (cls == SK_INVZERO) {
    if (store) st(r.target, inverse(rest));
  } else if (cls == SK_LIMBS) {
    const Fr v = from_mont(rest);
    const uint32_t j0 = r.aux & 0xffffu, cnt = (r.aux >> 16) & 0xffu, width = r.aux >> 24;
    for (uint32_t j = 0; store && j < cnt; j++)
      st(outs[r.target + j], r1cs_small(r1cs_limb(v, (j0 + j) * width, width)));
  } else if (cls == SK_BYTEOP) {
    const Fr a = ((r.ctl >> 8) & 3) != SCS_MARK_ZERO ? add(ta, q[4]) : ta, b = mk != SCS_MARK_ZERO ? add(tb, q[5]) : tb;
    const uint32_t u = from_mont(a).v[0], v = from_mont(b).v[0];
    if (store) st(r.target, r1cs_small(r.aux == 1 ? u ^ v : u & v));
  } else if (cls == SK_COUNT_ZERO) {
    for (uint32_t j = 0; store && j < r.aux >> 16; j++) st(outs[r.target + j], zero);
  } else if (cls == SK_COUNT_Q) {
    const Fr v = from_mont(rest);
    if (store && (v.v[1] | v.v[2] | v.v[3] | v.v[4] | v.v[5] | v.v[6] | v.v[7]) == 0 && v.v[0] < r.aux) {
      Fr c = ld(outs[r.target + v.v[0]]);
      c.v[0]++;
      st(outs[r.target + v.v[0]], c);
    }
  } else if (cls == SK_COUNT_END) {
    for (uint32_t j = 0; store && j < r.aux >> 16; j++)
      st(outs[r.target + j], r1cs_small(ld(outs[r.target + j]).v[0]));
  } else {
    const Fr v = from_mont(rest);
    const uint32_t j0 = r.aux & 0xffffu, cnt = r.aux >> 16;
    for (uint32_t j = 0; j < cnt; j++) {
      const uint32_t bit = j0 + j < 256 ? (v.v[(j0 + j) >> 5] >> ((j0 + j) & 31)) & 1u : 0u;
      st(outs[r.target + j], bit ? Fr::one() : Fr::zero());
    }
  }
  return ok;
}

}  // namespace zk
