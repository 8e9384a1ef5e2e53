// The solve plan of a gnark-shaped R1CS: the one definition of what zkmi_r1cs_solver_load builds
// from the loaded matrices and a zkmi_r1cs_solver_desc, and what r1cs_solve_kernel (r1cs_solve.hip)
// runs.  Host-compilable: tests/native/r1cs_plan_check.cpp builds plans and interprets them without
// a GPU (tests/test_native_r1cs_plan.py).
//
// gnark's solver (constraint/bn254 solver.go [UPSTREAM-RECALL]) walks cs.Instructions once per
// witness and finds, at run time, the one wire of each constraint that is not solved yet.  Which
// wire that is depends on the system alone, not on the witness, so the builder does that walk once
// with a solved-wire bitmap (ONE, the public and the secret inputs to begin with) and leaves the
// kernel a list of records with the unknowns resolved.  No scheduling: the plan is the instruction
// list in gnark's order.
//
// Record = two quads of 32-bit words, one per instruction:
//   quad 0  (kind, target, coef, coef_inv)
//     kind      RK_ASSERT    every wire known: check a b = c
//               RK_SOLVE_O   the unknown x has coefficient k in O: x = (a b - c) / k
//               RK_SOLVE_L   ... in L: x = (c / b - a) / k, b = 0 is unsatisfied   (RK_SOLVE_R alike)
//               RK_INVZERO   hint: target = 1 / a, 0 for a = 0       (a = the hint's input expression)
//               RK_NBITS     hint: bit i of the canonical value of a into wire outs[target + i]
//             plans of ZKMI_HINTS_STD only (P.ext says whether a plan holds one; none has an a/b/c row):
//               RK_LIMBS     hint: bits [i coef, (i + 1) coef) of the canonical value of a into wire
//                            outs[target + i], i < k: RK_NBITS with a width, 1 .. 64
//               RK_BYTEOP    hint: target = low 32 bits of a  XOR (coef = 1) | AND (coef = 2)  those of b
//               RK_COUNT_BEGIN / RK_COUNT_Q / RK_COUNT_END   the lookup-multiplicity hint, see below
//               RK_COMMIT    the commitment hint: a phase boundary, never executed -- a launch ends
//                            in front of it and the host supplies wire `target` (P.commits)
//             plans of ZKMI_HINTS_EMULATED only (P.emul says whether a plan holds one):
//               RK_EMUL_STEP / RK_EMUL_END   the emulated-product hint, see below
//     target    the wire solved (RK_NBITS, RK_LIMBS, RK_COUNT_*: the first entry of the hint's output
//               wires in `outs`)
//     coef      RK_SOLVE_*: coefficient word of the unknown (as in the terms below)
//     coef_inv  RK_SOLVE_*: index of 1 / k, appended to the coefficient table (inverted here, once)
//   quad 1  (first term, product rows, unit rows, k)
//     the instruction's KNOWN terms are terms[first .. first + S (product rows + unit rows)), and
//     the next instruction's follow them without a gap:
//     first the terms that need a product, padded to whole rows of S, then those with coefficient
//     +1 / -1, padded likewise -- a row is one term per sub-lane, so the S sub-lanes of a proof never
//     diverge inside a row.  k = constraint row the a, b, c of the instruction go to (RK_NBITS: the
//     number of output wires).
// The lookup-multiplicity hint (one instruction) is a run of records: RK_COUNT_BEGIN (no terms; the
//   sub-lanes zero the k = table size counters, the low words of wires outs[target ..]), then
//   RK_COUNT_Q steps of up to S queries, one per sub-lane: term row r of sub-lane s is term r of
//   query s of the step, padded to the step's longest query, so a sub-lane's own sum is its query and
//   nothing is added across sub-lanes; all rows are product rows (a unit coefficient multiplies by
//   1), k = queries in the step (sub-lanes from k on hold none), coef = table size; then
//   RK_COUNT_END (no terms; the sub-lanes turn the k counters into field images in place).
// The emulated-product hint (one instruction) is a run of records too: RK_EMUL_STEP steps of up to S
//   of its na + nb operand limbs, one per sub-lane, laid out like the queries of RK_COUNT_Q (all rows
//   product rows, a sub-lane's own sum is its limb); target = number of the step's first limb
//   (0 .. na + nb - 1: the limbs of a, then those of b), k = limbs in the step.  Then RK_EMUL_END (no
//   terms): coef = na | nb << 8 | nk << 16, target = the first entry of the hint's output wires in
//   `outs`, k = their number, coef_inv = index of the modulus in the coefficient table: one entry
//   with the modulus as a plain 256-bit integer (not a field image), then the 2^256 images of its
//   four 64-bit limbs.  r1cs_emul_finish below is what the record computes.
// Term = (wire | tag << 30, coefficient index | unit << 30): tag RT_L / RT_R / RT_O names the
//   expression the term belongs to (hints: RT_L; RK_BYTEOP: RT_L and RT_R), RT_PAD a padding term
//   (wire 0, adds nothing);
//   unit 1 / 2 = the coefficient is +1 / -1, as zkmi_r1cs_load marks it.
// The term array ends with R1CS_TERM_SLACK rows of padding terms and the records with one RK_ASSERT
// record without terms: the kernel fetches three rows and one record ahead of what it runs.  Records
// and terms are contiguous, so a launch may run any range [begin, end) of the records.
//
// Every count the kernel loops over and every index it uses as an address comes out of
// r1cs_plan_build, which has checked it: that is what bounds the kernel's accesses and its run time.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/zkmi.h"
#include "emul.h"
#include "ff.h"

namespace zk {

enum {
  RK_ASSERT = 0, RK_SOLVE_O, RK_SOLVE_L, RK_SOLVE_R, RK_INVZERO, RK_NBITS,
  RK_LIMBS, RK_BYTEOP, RK_COUNT_BEGIN, RK_COUNT_Q, RK_COUNT_END, RK_COMMIT,
  RK_EMUL_STEP, RK_EMUL_END
};
enum { RT_L = 0, RT_R = 1, RT_O = 2, RT_PAD = 3 };
constexpr uint32_t R1CS_IDX_MASK = 0x3fffffffu;   // low 30 bits of a term word
constexpr uint32_t R1CS_TERM_SLACK = 3;           // rows of padding terms behind the last instruction

struct R1csTerm {
  uint32_t wire, coef;   // the loaded form: coef = coefficient index | unit << 30
};
struct R1csRecord {
  uint32_t kind, target, coef, coef_inv;
  uint32_t first, mul_rows, unit_rows, k;
};

// The loaded system (zkmi_r1cs, read back to the host) and the caller's solver description.
struct R1csPlanIn {
  uint32_t n_wires = 0, n_constraints = 0, n_coeffs = 0;
  const Fr* coeffs = nullptr;             // 2^261 images (gnark's image times 2^5)
  const uint32_t* ptr[3] = {};            // L, R, O: n_constraints + 1 offsets
  const R1csTerm* terms[3] = {};
  const zkmi_r1cs_solver_desc* desc = nullptr;   // host arrays
};
// A commitment hint: the record a launch stops in front of, and what the proving key must agree with
struct R1csCommit {
  uint32_t instr = 0, record = 0, wire = 0;
  std::vector<uint32_t> hashed, priv;
};
struct R1csPlan {
  uint32_t S = 0, n_instr = 0;
  bool ext = false;                  // holds a record kind from RK_LIMBS on
  bool emul = false;                 // holds RK_EMUL_STEP / RK_EMUL_END records
  std::vector<R1csRecord> records;   // one per instruction (a lookup-multiplicity hint: several) + 1
  std::vector<R1csCommit> commits;   // in instruction order
  std::vector<R1csTerm> terms;       // plan terms: (wire | tag << 30, coef)
  std::vector<Fr> coeffs;            // the system's table, then the inverses (2^261 images) and the
                                     // moduli of the emulated products (see RK_EMUL_END)
  std::vector<uint32_t> outs;        // output wires of the RK_NBITS, RK_LIMBS, RK_COUNT_* and RK_EMUL_END hints
  uint64_t n_terms = 0;              // known terms, without padding
  uint32_t longest = 0;              // most known terms in one instruction
  uint32_t n_inversions = 0;         // RK_SOLVE_L + RK_SOLVE_R + RK_INVZERO
};

// S for lanes_per_proof = 0: the power of two in 1 .. 16 nearest to the mean number of known terms
// per instruction (the smaller one when two are equally near)
inline uint32_t r1cs_auto_lanes(uint64_t n_terms, uint32_t n_instr) {
  const double mean = n_instr ? (double)n_terms / n_instr : 1.0;
  uint32_t best = 1;
  for (uint32_t s = 2; s <= 16; s *= 2) {
    const double d = mean > s ? mean - s : s - mean, db = mean > best ? mean - best : best - mean;
    if (d < db) best = s;
  }
  return best;
}

inline const char* r1cs_hint_name(uint32_t kind) {
  static const char* names[8] = {"kind 0", "InvZero", "NBits", "limbs (kind 3)",
                                 "lookup multiplicities (kind 4)", "commitment (kind 5)",
                                 "byte operation (kind 6)", "emulated product (kind 7)"};
  return kind < 8 ? names[kind] : "of an unknown kind";
}

// bits [pos, pos + wd) of the 256-bit integer v, wd in 1 .. 64; the bits from 256 on are 0
ZK_HD uint64_t r1cs_limb(const Fr& v, uint32_t pos, uint32_t wd) {
  if (pos >= 256) return 0;
  const uint32_t i = pos >> 5, sh = pos & 31;
  const uint64_t two = (uint64_t)(i < 7 ? v.v[i + 1] : 0u) << 32 | v.v[i];
  uint64_t r = two >> sh;
  if (sh && i < 6) r |= (uint64_t)v.v[i + 2] << (64 - sh);
  return wd >= 64 ? r : r & (((uint64_t)1 << wd) - 1);
}
// the 2^256 image of an integer below 2^64
ZK_HD Fr r1cs_small(uint64_t x) {
  Fr m = Fr::zero();
  m.v[0] = (uint32_t)x;
  m.v[1] = (uint32_t)(x >> 32);
  return to_mont(m);
}

// Entry i (wave-uniform) of a register array, read and written as chains of selects over compile-time
// indices: a switch over the entries would let the compiler merge the cases into one access with a
// computed address, and the array would leave the registers for scratch memory.
template <int N>
ZK_HD Fr r1cs_pick(const Fr (&L)[N], uint32_t i) {
  Fr r = L[0];
#pragma unroll
  for (int q = 1; q < N; q++)
#pragma unroll
    for (int t = 0; t < 8; t++) r.v[t] = i == (uint32_t)q ? L[q].v[t] : r.v[t];
  return r;
}
template <int N>
ZK_HD void r1cs_put(Fr (&L)[N], uint32_t i, const Fr& v) {
#pragma unroll
  for (int q = 0; q < N; q++)
#pragma unroll
    for (int t = 0; t < 8; t++) L[q].v[t] = i == (uint32_t)q ? v.v[t] : L[q].v[t];
}
// 64-bit limb i (wave-uniform, below N / 2) of a word array
template <int N, int M>
ZK_HD uint64_t r1cs_limb64(const uint32_t (&T)[M], uint32_t i) {
  uint32_t lo = T[0], hi = T[1];
#pragma unroll
  for (int q = 1; q < N / 2; q++) {
    lo = i == (uint32_t)q ? T[2 * q] : lo;
    hi = i == (uint32_t)q ? T[2 * q + 1] : hi;
  }
  return (uint64_t)hi << 32 | lo;
}

// What an RK_EMUL_END record computes, on the device and in the host interpreters alike.  L: the
// 2^256 images of the na limbs of a, then the nb of b, as the steps gathered them; modulus: the plain
// integer p; pimg: the 2^256 images of its four limbs; par = na | nb << 8 | nk << 16, checked by the
// builder.  store(o, v) gets output o of the hint: nk limbs of floor(a b / p), four of a b mod p
// (emul.h: twelve words per operand), then the carries c_j = (sum_i a_i b_(j-i) - r_j -
// sum_i k_i p_(j-i) + c_(j-1)) 2^-64, formed in the field from the images, as gnark's hint forms them
// from the wire values.  Every count is wave-uniform.
template <class Store>
ZK_HD void r1cs_emul_finish(const Fr (&L)[8], const Fr& modulus, const Fr* pimg, uint32_t par,
                            Store store) {
  const uint32_t na = par & 0xffu, nb = (par >> 8) & 0xffu, nk = (par >> 16) & 0xffu;
  uint32_t A[12], B[12], T[24], Rm[9];
#pragma unroll
  for (int i = 0; i < 12; i++) A[i] = B[i] = 0;
  for (uint32_t q = 0; q < na + nb; q++) {
    const Fr v = from_mont(r1cs_pick(L, q));
    if (q < na)
      emul_acc_at(A, v.v, q);
    else
      emul_acc_at(B, v.v, q - na);
  }
  emul_mul(T, A, B);
  emul_divmod(T, Rm, modulus.v);
  Fr KR[12];   // the images of the quotient's limbs, then the remainder's
#pragma unroll
  for (int i = 0; i < 12; i++) KR[i] = Fr::zero();
  for (uint32_t o = 0; o < nk + 4; o++) {
    const Fr v = r1cs_small(o < nk ? r1cs_limb64<16>(T, o) : r1cs_limb64<8>(Rm, o - nk));
    r1cs_put(KR, o, v);
    store(o, v);
  }
  Fr inv64 = Fr::zero(), prev = Fr::zero();
  inv64.v[6] = 1;   // 2^192: the Montgomery image of 2^-64
  const uint32_t ncols = na + nb - 1 > nk + 3 ? na + nb - 1 : nk + 3;
  for (uint32_t j = 0; j + 1 < ncols; j++) {
    Fr d = prev;
    for (uint32_t i = 0; i < na; i++)
      if (j >= i && j - i < nb) d = add(d, mul(r1cs_pick(L, i), r1cs_pick(L, na + j - i)));
    if (j < 4) d = sub(d, r1cs_pick(KR, nk + j));
    for (uint32_t i = 0; i < nk; i++)
      if (j >= i && j - i < 4) d = sub(d, mul(r1cs_pick(KR, i), pimg[j - i]));
    prev = mul(d, inv64);
    store(nk + 4 + j, prev);
  }
}

// Returns the empty string and the plan, or what is wrong with the description.
inline std::string r1cs_plan_build(const R1csPlanIn& in, R1csPlan* out) {
  const zkmi_r1cs_solver_desc& d = *in.desc;
  const std::string pre = "r1cs solver: ";
  if (in.n_wires == 0 || in.n_wires > R1CS_IDX_MASK || in.n_coeffs == 0 || in.n_coeffs > R1CS_IDX_MASK)
    return pre + "the system needs 1 .. 2^30 - 1 wires and coefficients";
  uint32_t S = d.lanes_per_proof;
  if (S > 64 || (S & (S - 1))) return pre + "lanes_per_proof must be 0 (auto) or a power of two, 1 .. 64";
  // 2 would be the emulated product without the std kinds, which is not offered: the message is the
  // one callers have seen for it since before ZKMI_HINTS_EMULATED
  if (d.hint_set == 2) return pre + "hint_set must be ZKMI_HINTS_BASIC (0) or ZKMI_HINTS_STD (1)";
  if (d.hint_set > ZKMI_HINTS_EMULATED)
    return pre + "hint_set must be ZKMI_HINTS_BASIC (0), ZKMI_HINTS_STD (1) or ZKMI_HINTS_EMULATED (3)";
  const bool std_set = d.hint_set != ZKMI_HINTS_BASIC, emul_set = d.hint_set == ZKMI_HINTS_EMULATED;
  if (d.n_public == 0 || (uint64_t)d.n_public + d.n_secret > in.n_wires)
    return pre + "n_public (which counts the ONE wire) + n_secret must be in 1 .. n_wires";
  if (d.n_instr == 0 || !d.instr) return pre + "no instructions";
  if (d.n_hints && (!d.hint_kind || !d.hint_in_ptr || !d.hint_lc_ptr || !d.hint_out_ptr))
    return pre + "hint table: null array";
  // the hint table's offsets, before any of them is used as an index
  uint32_t n_lc = 0, n_hterms = 0, n_houts = 0;
  if (d.n_hints) {
    bool ok = d.hint_in_ptr[0] == 0 && d.hint_out_ptr[0] == 0;
    for (uint32_t h = 0; ok && h < d.n_hints; h++)
      ok = d.hint_in_ptr[h] <= d.hint_in_ptr[h + 1] && d.hint_out_ptr[h] <= d.hint_out_ptr[h + 1];
    if (ok) {
      n_lc = d.hint_in_ptr[d.n_hints];
      n_houts = d.hint_out_ptr[d.n_hints];
      ok = d.hint_lc_ptr[0] == 0;
      for (uint32_t i = 0; ok && i < n_lc; i++) ok = d.hint_lc_ptr[i] <= d.hint_lc_ptr[i + 1];
      if (ok) n_hterms = d.hint_lc_ptr[n_lc];
    }
    if (!ok || (n_hterms && !d.hint_terms) || (n_houts && !d.hint_out))
      return pre + "hint table: offsets are not monotone from 0, or a null array";
  }
  // the matrices (zkmi_r1cs_load has checked them too; a plan must not depend on that)
  static const char* names[3] = {"L", "R", "O"};
  for (uint32_t s = 0; s < 3; s++) {
    bool ok = in.ptr[s] && in.ptr[s][0] == 0;
    for (uint32_t k = 0; ok && k < in.n_constraints; k++) ok = in.ptr[s][k] <= in.ptr[s][k + 1];
    const uint32_t nnz = ok ? in.ptr[s][in.n_constraints] : 0;
    ok = ok && (nnz == 0 || in.terms[s]);
    for (uint32_t t = 0; ok && t < nnz; t++)
      ok = in.terms[s][t].wire < in.n_wires && (in.terms[s][t].coef & R1CS_IDX_MASK) < in.n_coeffs;
    if (!ok)
      return pre + "malformed matrix " + names[s] +
             " (offsets not monotone from 0, or a term's coefficient / wire index out of range)";
  }
  // +1 / -1 among the lifted coefficients (hint terms arrive unmarked)
  Fr one32 = Fr::one();
  for (int t = 0; t < 5; t++) one32 = add(one32, one32);
  const Fr minus32 = neg(one32);
  auto unit_of = [&](uint32_t cid) {
    return in.coeffs[cid] == one32 ? 1u : in.coeffs[cid] == minus32 ? 2u : 0u;
  };

  std::vector<uint8_t> solved(in.n_wires, 0), row_seen(in.n_constraints, 0);
  for (uint32_t i = 0; i < d.n_public + d.n_secret; i++) solved[i] = 1;

  // pass 1: resolve the unknowns in instruction order
  struct Pending {
    uint32_t kind, target, coef, k;
    std::vector<R1csTerm> mul, unit;   // known terms, tagged
    std::vector<std::vector<R1csTerm>> queries;   // RK_COUNT_BEGIN: the terms of every query;
                                                  // RK_EMUL_END: those of every operand limb
    std::vector<uint32_t> mod;                    // RK_EMUL_END: the modulus, eight words
  };
  std::vector<R1csCommit> commits;
  bool ext = false, emul = false;
  // 2^251 is the Montgomery image of 2^-5: takes a sum of 2^261 images to gnark's image
  Fr down5 = Fr::zero();
  down5.v[7] = 1u << 27;
  std::vector<Pending> pend(d.n_instr);
  std::vector<uint32_t> outs;
  uint64_t n_terms = 0;
  uint32_t longest = 0;
  for (uint32_t ii = 0; ii < d.n_instr; ii++) {
    const uint32_t ik = d.instr[2 * ii], idx = d.instr[2 * ii + 1];
    const std::string at = pre + "instruction " + std::to_string(ii);
    Pending& p = pend[ii];
    auto known = [&](uint32_t wire, uint32_t coef, uint32_t tag) {
      (coef >> 30 ? p.unit : p.mul).push_back(R1csTerm{wire | tag << 30, coef});
    };
    if (ik == 1) {
      if (idx >= d.n_hints) return at + ": hint index " + std::to_string(idx) + " out of range";
      const uint32_t hk = d.hint_kind[idx];
      const std::string hat = at + " (hint " + std::to_string(idx) + ")";
      const bool std_kind = hk == ZKMI_HINT_LIMBS || hk == ZKMI_HINT_COUNT || hk == ZKMI_HINT_COMMIT ||
                            hk == ZKMI_HINT_BYTEOP;
      const bool emul_kind = hk == ZKMI_HINT_EMULMUL, param_kind = std_kind || emul_kind;
      if (hk != ZKMI_HINT_INVZERO && hk != ZKMI_HINT_NBITS && !(std_set && std_kind) &&
          !(emul_set && emul_kind))
        return hat + ": hints " + r1cs_hint_name(hk) + " are not supported on this entry";
      const uint32_t in0 = d.hint_in_ptr[idx], in1 = d.hint_in_ptr[idx + 1];
      const uint32_t o0 = d.hint_out_ptr[idx], o1 = d.hint_out_ptr[idx + 1];
      const uint32_t nin = in1 - in0, nout = o1 - o0;
      const std::string name = r1cs_hint_name(hk);
      if (!param_kind && (nin != 1 || nout == 0 || (hk == ZKMI_HINT_INVZERO && nout != 1)))
        return hat + ": " + name + " takes one input" +
               (hk == ZKMI_HINT_INVZERO ? " and has one output" : " and has outputs");
      if (hk == ZKMI_HINT_LIMBS && (nin != 2 || nout == 0))
        return hat + ": " + name + " takes a width and one input and has outputs";
      if (hk == ZKMI_HINT_COUNT && (nin < 2 || nout == 0))
        return hat + ": " + name + " takes a table size and queries and has outputs";
      if (hk == ZKMI_HINT_BYTEOP && (nin != 3 || nout != 1))
        return hat + ": " + name + " takes an operation and two inputs and has one output";
      if (hk == ZKMI_HINT_COMMIT && (nin < 1 || nout != 1))
        return hat + ": " + name + " takes the number of hashed operands and the operands and has one output";
      if (emul_kind && (nin < 1 || nout == 0))
        return hat + ": " + name + " takes a parameter, operand limbs and four modulus limbs and has outputs";
      // expression e of the hint: every term checked, then handed to `sink`
      std::string bad;
      auto expression = [&](uint32_t e, auto sink) {
        for (uint32_t t = d.hint_lc_ptr[e]; bad.empty() && t < d.hint_lc_ptr[e + 1]; t++) {
          const uint32_t cid = d.hint_terms[t].coeff, wire = d.hint_terms[t].wire;
          if (cid >= in.n_coeffs || wire >= in.n_wires)
            bad = hat + ": a term's coefficient or wire index is out of range";
          else if (!solved[wire])
            bad = hat + ": reads wire " + std::to_string(wire) + ", which is not solved yet";
          else
            sink(wire, cid);
        }
      };
      uint32_t first_expr = in0, p0 = 0;
      if (param_kind) {
        // the constant parameter: terms on ONE alone, a value below 2^32
        Fr sum = Fr::zero();
        expression(in0, [&](uint32_t wire, uint32_t cid) {
          if (wire != 0)
            bad = hat + ": the parameter of " + name + " is not a constant (it reads wire " +
                  std::to_string(wire) + ")";
          sum = add(sum, in.coeffs[cid]);
        });
        if (!bad.empty()) return bad;
        const Fr v = from_mont(mul(sum, down5));
        p0 = (v.v[1] | v.v[2] | v.v[3] | v.v[4] | v.v[5] | v.v[6] | v.v[7]) ? 0xffffffffu : v.v[0];
        first_expr = in0 + 1;
      }
      if (hk == ZKMI_HINT_LIMBS && (p0 < 1 || p0 > 64))
        return hat + ": limb width " + std::to_string(p0) + " is outside 1 .. 64";
      if (hk == ZKMI_HINT_COUNT && p0 != nout)
        return hat + ": table size " + std::to_string(p0) + " is not the number of outputs, " +
               std::to_string(nout);
      if (hk == ZKMI_HINT_BYTEOP && p0 != 1 && p0 != 2)
        return hat + ": byte operation " + std::to_string(p0) + " is neither 1 (XOR) nor 2 (AND)";
      if (hk == ZKMI_HINT_COMMIT && p0 > nin - 1)
        return hat + ": " + std::to_string(p0) + " hashed operands among " + std::to_string(nin - 1);
      const uint32_t na = p0 & 0xffu, nb = (p0 >> 8) & 0xffu, nk = (p0 >> 16) & 0xffu;
      if (emul_kind) {
        if (p0 >> 24 || na < 1 || na > 4 || nb < 1 || nb > 4 || nk < 1 || nk > 8)
          return hat + ": " + name + " with na = " + std::to_string(na) + ", nb = " + std::to_string(nb) +
                 ", nk = " + std::to_string(nk) + " (parameter " + std::to_string(p0) +
                 ") is outside 1 .. 4 limbs per operand and 1 .. 8 quotient limbs";
        if (nin != 1 + na + nb + 4)
          return hat + ": " + name + " takes a parameter, " + std::to_string(na) + " + " + std::to_string(nb) +
                 " operand limbs and 4 modulus limbs, not " + std::to_string(nin) + " expressions";
        const uint32_t ncols = std::max(na + nb - 1, nk + 3);
        if (nout != nk + 4 + ncols - 1)
          return hat + ": " + name + " has " + std::to_string(nk) + " + 4 + " + std::to_string(ncols - 1) +
                 " outputs, not " + std::to_string(nout);
      }
      R1csCommit com;
      for (uint32_t e = first_expr; e < in1; e++) {
        const uint32_t j = e - first_expr;
        if (emul_kind && j >= na + nb) {
          // a limb of the modulus: a constant like the parameter, below 2^64
          const std::string limb = "modulus limb " + std::to_string(j - na - nb) + " of " + name;
          Fr sum = Fr::zero();
          expression(e, [&](uint32_t wire, uint32_t cid) {
            if (wire != 0) bad = hat + ": " + limb + " is not a constant (it reads wire " + std::to_string(wire) + ")";
            sum = add(sum, in.coeffs[cid]);
          });
          if (!bad.empty()) return bad;
          const Fr v = from_mont(mul(sum, down5));
          if (v.v[2] | v.v[3] | v.v[4] | v.v[5] | v.v[6] | v.v[7]) return hat + ": " + limb + " is 2^64 or more";
          p.mod.push_back(v.v[0]);
          p.mod.push_back(v.v[1]);
        } else if (hk == ZKMI_HINT_COUNT || emul_kind) {
          p.queries.emplace_back();
          expression(e, [&](uint32_t wire, uint32_t cid) {
            p.queries.back().push_back(R1csTerm{wire | (uint32_t)RT_L << 30, cid});
          });
          n_terms += p.queries.back().size();
          if (p.queries.back().size() > longest) longest = (uint32_t)p.queries.back().size();
        } else if (hk == ZKMI_HINT_COMMIT) {
          // commit_phase reads wire rows, not expressions
          uint32_t n = 0, w = 0, c = 0;
          expression(e, [&](uint32_t wire, uint32_t cid) { n++, w = wire, c = cid; });
          if (bad.empty() && (n != 1 || in.coeffs[c] != one32))
            return hat + ": commitment operand " + std::to_string(j) +
                   " is not a single wire with coefficient 1";
          (j < p0 ? com.hashed : com.priv).push_back(w);
        } else {
          const uint32_t tag = hk == ZKMI_HINT_BYTEOP && j == 1 ? RT_R : RT_L;
          expression(e, [&](uint32_t wire, uint32_t cid) { known(wire, cid | unit_of(cid) << 30, tag); });
        }
        if (!bad.empty()) return bad;
      }
      if (emul_kind && p.mod[7] == 0) return hat + ": the modulus of " + name + " is below 2^224";
      for (uint32_t o = o0; o < o1; o++) {
        const uint32_t wire = d.hint_out[o];
        if (wire >= in.n_wires) return hat + ": output wire " + std::to_string(wire) + " out of range";
        if (solved[wire]) return hat + ": output wire " + std::to_string(wire) + " is already solved";
        solved[wire] = 1;
      }
      ext = ext || param_kind;
      emul = emul || emul_kind;
      p.coef = 0;
      if (hk == ZKMI_HINT_INVZERO || hk == ZKMI_HINT_BYTEOP) {
        p.kind = hk == ZKMI_HINT_INVZERO ? RK_INVZERO : RK_BYTEOP;
        p.target = d.hint_out[o0];
        p.k = 0;
        if (hk == ZKMI_HINT_BYTEOP) p.coef = p0;
      } else if (hk == ZKMI_HINT_COMMIT) {
        p.kind = RK_COMMIT;
        p.target = d.hint_out[o0];
        p.k = (uint32_t)commits.size();
        com.instr = ii;
        com.wire = p.target;
        commits.push_back(std::move(com));
      } else {
        p.kind = hk == ZKMI_HINT_NBITS ? RK_NBITS : hk == ZKMI_HINT_LIMBS ? RK_LIMBS :
                 emul_kind ? RK_EMUL_END : RK_COUNT_BEGIN;
        p.target = (uint32_t)outs.size();
        p.k = nout;
        if (hk == ZKMI_HINT_LIMBS || emul_kind) p.coef = p0;
        outs.insert(outs.end(), d.hint_out + o0, d.hint_out + o1);
      }
    } else if (ik == 0) {
      if (idx >= in.n_constraints) return at + ": constraint index " + std::to_string(idx) + " out of range";
      const std::string cat = at + " (constraint " + std::to_string(idx) + ")";
      if (row_seen[idx]) return cat + ": the constraint occurs twice";
      row_seen[idx] = 1;
      int64_t unk = -1;
      uint32_t unk_coef = 0, unk_tag = 0;
      for (uint32_t s = 0; s < 3; s++)
        for (uint32_t t = in.ptr[s][idx]; t < in.ptr[s][idx + 1]; t++) {
          const R1csTerm tm = in.terms[s][t];
          if (solved[tm.wire]) {
            known(tm.wire, tm.coef, s);
            continue;
          }
          if (unk >= 0 && (uint32_t)unk != tm.wire)
            return cat + ": two unknown wires (" + std::to_string(unk) + ", " + std::to_string(tm.wire) + ")";
          if (unk >= 0)
            return cat + ": the unknown wire " + std::to_string(unk) +
                   (unk_tag == s ? " occurs twice in one expression" : " occurs in more than one of L, R, O");
          unk = tm.wire;
          unk_coef = tm.coef;
          unk_tag = s;
        }
      p.k = idx;
      p.kind = unk < 0 ? RK_ASSERT : unk_tag == RT_O ? RK_SOLVE_O : unk_tag == RT_L ? RK_SOLVE_L : RK_SOLVE_R;
      p.target = unk < 0 ? 0 : (uint32_t)unk;
      p.coef = unk_coef;
      if (unk >= 0) {
        if (in.coeffs[unk_coef & R1CS_IDX_MASK].is_zero())
          return cat + ": the unknown wire " + std::to_string(unk) + " has coefficient 0";
        solved[unk] = 1;
      }
    } else {
      return at + ": kind " + std::to_string(ik) + " is neither a constraint (0) nor a hint (1)";
    }
    const uint32_t n = (uint32_t)(p.mul.size() + p.unit.size());
    n_terms += n;
    if (n > longest) longest = n;
  }
  for (uint32_t k = 0; k < in.n_constraints; k++)
    if (!row_seen[k]) return pre + "constraint " + std::to_string(k) + " occurs in no instruction";
  for (uint32_t w = 0; w < in.n_wires; w++)
    if (!solved[w]) return pre + "wire " + std::to_string(w) + " is still unsolved after the last instruction";

  if (S == 0) S = r1cs_auto_lanes(n_terms, d.n_instr);
  // pass 2: lay the records and the padded term rows out
  R1csPlan& P = *out;
  P = R1csPlan();
  P.S = S;
  P.n_instr = d.n_instr;
  P.n_terms = n_terms;
  P.longest = longest;
  P.outs = std::move(outs);
  P.ext = ext;
  P.emul = emul;
  P.commits = std::move(commits);
  P.coeffs.assign(in.coeffs, in.coeffs + in.n_coeffs);
  P.records.reserve((size_t)d.n_instr + 1);
  const R1csTerm pad{(uint32_t)RT_PAD << 30, 0};
  std::vector<uint32_t> moduli;   // where the moduli of the emulated products sit in P.coeffs
  // 1 / k from the 2^261 image k 2^5 (as a Montgomery value): inverse() gives (1 / k) 2^-5, ten
  // doublings the image (1 / k) 2^5 again
  auto inverse_261 = [](const Fr& x) {
    Fr r = inverse(x);
    for (int t = 0; t < 10; t++) r = add(r, r);
    return r;
  };
  for (uint32_t ii = 0; ii < d.n_instr; ii++) {
    Pending& p = pend[ii];
    R1csRecord r{p.kind, p.target, p.coef, 0, 0, 0, 0, p.k};
    if (p.kind == RK_COMMIT) P.commits[p.k].record = (uint32_t)P.records.size();
    if (p.kind == RK_COUNT_BEGIN || p.kind == RK_EMUL_END) {
      // begin, the query steps of S queries each (one per sub-lane, term row by term row), end; an
      // emulated product has steps of operand limbs in place of queries, and no begin
      const bool count = p.kind == RK_COUNT_BEGIN;
      r.first = (uint32_t)P.terms.size();
      if (count) P.records.push_back(r);
      for (size_t q0 = 0; q0 < p.queries.size(); q0 += S) {
        const size_t nq = std::min<size_t>(S, p.queries.size() - q0);
        size_t rows = 0;
        for (size_t q = 0; q < nq; q++) rows = std::max(rows, p.queries[q0 + q].size());
        const uint64_t first = P.terms.size();
        if (first + (uint64_t)(rows + R1CS_TERM_SLACK) * S > 0xffffffffull) return pre + "more than 2^32 plan terms";
        P.records.push_back(count ? R1csRecord{RK_COUNT_Q, p.target, p.k, 0, (uint32_t)first, (uint32_t)rows,
                                               0, (uint32_t)nq}
                                  : R1csRecord{RK_EMUL_STEP, (uint32_t)q0, 0, 0, (uint32_t)first,
                                               (uint32_t)rows, 0, (uint32_t)nq});
        P.terms.resize(first + rows * S, pad);
        for (size_t q = 0; q < nq; q++)
          for (size_t t = 0; t < p.queries[q0 + q].size(); t++) P.terms[first + t * S + q] = p.queries[q0 + q][t];
      }
      p.queries = std::vector<std::vector<R1csTerm>>();
      if (count) {
        P.records.push_back(R1csRecord{RK_COUNT_END, p.target, 0, 0, (uint32_t)P.terms.size(), 0, 0, p.k});
        continue;
      }
      // the modulus: once per plan, as a plain integer and as the images of its four limbs
      Fr m;
      for (int t = 0; t < 8; t++) m.v[t] = p.mod[t];
      size_t at = 0;
      while (at < moduli.size() && !(P.coeffs[moduli[at]] == m)) at++;
      if (at == moduli.size()) {
        moduli.push_back((uint32_t)P.coeffs.size());
        P.coeffs.push_back(m);
        for (int t = 0; t < 4; t++) P.coeffs.push_back(r1cs_small((uint64_t)p.mod[2 * t + 1] << 32 | p.mod[2 * t]));
      }
      P.records.push_back(R1csRecord{RK_EMUL_END, p.target, p.coef, moduli[at], (uint32_t)P.terms.size(), 0, 0,
                                     p.k});
      continue;
    }
    if (p.kind == RK_SOLVE_O || p.kind == RK_SOLVE_L || p.kind == RK_SOLVE_R) {
      r.coef_inv = (uint32_t)P.coeffs.size();
      P.coeffs.push_back(inverse_261(in.coeffs[p.coef & R1CS_IDX_MASK]));
    }
    if (p.kind == RK_SOLVE_L || p.kind == RK_SOLVE_R || p.kind == RK_INVZERO) P.n_inversions++;
    r.mul_rows = (uint32_t)((p.mul.size() + S - 1) / S);
    r.unit_rows = (uint32_t)((p.unit.size() + S - 1) / S);
    const uint64_t first = P.terms.size();
    if (first + (uint64_t)(r.mul_rows + r.unit_rows + R1CS_TERM_SLACK) * S > 0xffffffffull)
      return pre + "more than 2^32 plan terms";
    r.first = (uint32_t)first;
    P.terms.insert(P.terms.end(), p.mul.begin(), p.mul.end());
    P.terms.resize(first + (size_t)r.mul_rows * S, pad);
    P.terms.insert(P.terms.end(), p.unit.begin(), p.unit.end());
    P.terms.resize(first + (size_t)(r.mul_rows + r.unit_rows) * S, pad);
    P.records.push_back(r);
    p.mul = std::vector<R1csTerm>();
    p.unit = std::vector<R1csTerm>();
  }
  P.records.push_back(R1csRecord{RK_ASSERT, 0, 0, 0, (uint32_t)P.terms.size(), 0, 0, 0});
  P.terms.resize(P.terms.size() + (size_t)R1CS_TERM_SLACK * S, pad);
  if (P.coeffs.size() > R1CS_IDX_MASK) return pre + "coefficient table overflow";
  return "";
}

}  // namespace zk
