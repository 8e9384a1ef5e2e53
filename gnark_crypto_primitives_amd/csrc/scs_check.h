// Loader checks of the PLONK witness entry: what stands between a caller's sparse constraint system
// (zkmi_scs_desc: gnark's SparseR1CS read as three wire columns and five selectors) or permutation
// (zkmi_plonk_trace_desc.perm: gnark's trace.S) and a kernel that uses their words as row addresses.
// Host-compilable: tests/native/test_scs_check.cpp runs them without a GPU
// (tests/test_native_scs_check.py).
//
// Positions: column c (0 = a, 1 = b, 2 = c) of row r of the domain of size n is position c n + r.
// A permutation is 3n uint32 entries, position -> image position (frontend/scs.py::ScsCircuit.sigma).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "ff.h"

namespace zk {

constexpr uint32_t SCS_MAX_GATES = 1u << 24;

struct ScsShape {
  uint32_t n_wires, n_gates, n_public;
};

// Marks of a selector value, as zkmi_r1cs_load leaves them in its coefficient words (1: the value is
// +1, 2: it is -1, 0: a product is needed), and 3: the value is 0 and the term drops out.
enum { SCS_MARK_GENERAL = 0, SCS_MARK_ONE = 1, SCS_MARK_MINUS_ONE = 2, SCS_MARK_ZERO = 3 };

inline bool fr_is_reduced(const Fr& x) {
  for (int j = 7; j >= 0; j--)
    if (x.v[j] != FrParams::p(j)) return x.v[j] < FrParams::p(j);
  return false;
}
inline uint32_t scs_mark(const Fr& x) {
  if (x.is_zero()) return SCS_MARK_ZERO;
  if (x == Fr::one()) return SCS_MARK_ONE;
  if (x == neg(Fr::one())) return SCS_MARK_MINUS_ONE;
  return SCS_MARK_GENERAL;
}

// the counts alone (what a loader checks before it sizes anything by them)
inline std::string scs_shape_check(const ScsShape& s) {
  if (s.n_wires == 0 || s.n_gates == 0) return "scs: n_wires and n_gates must be positive";
  if (s.n_gates > SCS_MAX_GATES) return "scs: n_gates above 2^24";
  if (s.n_public > s.n_gates) return "scs: more public inputs than gates";
  return "";
}

// The system's own shape: "" when it is accepted, else the reason.  selectors: 5 x n_gates field
// elements (qL, qR, qO, qM, qC; gnark's Montgomery image).  With `marks` (n_gates words), word g gets
// the marks of gate g's five selectors, two bits each, qL lowest.
inline std::string scs_validate(const ScsShape& s, const uint32_t* xa, const uint32_t* xb,
                                const uint32_t* xc, const Fr* selectors, uint32_t* marks = nullptr) {
  if (!xa || !xb || !xc || !selectors) return "scs: xa, xb, xc and selectors must not be null";
  const std::string shape = scs_shape_check(s);
  if (!shape.empty()) return shape;
  const uint32_t* x[3] = {xa, xb, xc};
  static const char* names[3] = {"xa", "xb", "xc"};
  for (int c = 0; c < 3; c++)
    for (uint32_t g = 0; g < s.n_gates; g++)
      if (x[c][g] >= s.n_wires)
        return std::string("scs: ") + names[c] + "[" + std::to_string(g) + "] = " +
               std::to_string(x[c][g]) + " is not a wire (n_wires = " + std::to_string(s.n_wires) + ")";
  for (int q = 0; q < 5; q++)
    for (uint32_t g = 0; g < s.n_gates; g++)
      if (!fr_is_reduced(selectors[(size_t)q * s.n_gates + g]))
        return "scs: selector " + std::to_string(q) + " of gate " + std::to_string(g) +
               " is not reduced mod r";
  if (marks)
    for (uint32_t g = 0; g < s.n_gates; g++) {
      uint32_t w = 0;
      for (int q = 0; q < 5; q++) w |= scs_mark(selectors[(size_t)q * s.n_gates + g]) << (2 * q);
      marks[g] = w;
    }
  return "";
}

// perm: 3n entries, every one below 3n, no image twice
inline std::string scs_perm_validate(const uint32_t* perm, size_t n) {
  if (!perm) return "plonk trace: perm must not be null";
  const size_t total = 3 * n;
  std::vector<uint8_t> seen(total, 0);
  for (size_t p = 0; p < total; p++) {
    if (perm[p] >= total)
      return "plonk trace: perm[" + std::to_string(p) + "] = " + std::to_string(perm[p]) +
             " is not a position (3n = " + std::to_string(total) + ")";
    if (seen[perm[p]])
      return "plonk trace: perm is not a bijection: position " + std::to_string(perm[p]) +
             " is the image of two positions";
    seen[perm[p]] = 1;
  }
  return "";
}

// A wiring against a key's permutation (validated by scs_perm_validate) on the domain n >= n_gates:
// a position on a gate row holds the wire its image holds, a position on a padding row (the columns
// read as zero there) is a fixed point.
inline std::string scs_wiring_check(const ScsShape& s, const uint32_t* xa, const uint32_t* xb,
                                    const uint32_t* xc, const uint32_t* perm, size_t n) {
  if (s.n_gates > n) return "scs: more gates than the key's domain has rows";
  const uint32_t* x[3] = {xa, xb, xc};
  for (size_t p = 0; p < 3 * n; p++) {
    const size_t r = p % n, q = perm[p], rq = q % n;
    if (r >= s.n_gates) {
      if (q != p)
        return "scs: the key's permutation moves position " + std::to_string(p) + " of padding row " +
               std::to_string(r);
      continue;
    }
    if (rq >= s.n_gates || x[q / n][rq] != x[p / n][r])
      return "scs: the wiring contradicts the key's permutation at position " + std::to_string(p) +
             " (column " + std::to_string(p / n) + ", row " + std::to_string(r) + ", wire " +
             std::to_string(x[p / n][r]) + "): its image " + std::to_string(q) +
             " does not hold the same wire";
  }
  return "";
}

}  // namespace zk
