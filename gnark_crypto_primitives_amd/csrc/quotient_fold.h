// The fold plan of a proving key whose quotient MSM takes evaluations (quotient_fold.hip): what
// zkmi_pk_load builds on the host from the O matrix of zkmi_pk_desc.fold_r1cs before any kernel
// runs.  Host-compilable: tests/native/quotient_fold_check.cpp builds plans without a GPU
// (tests/test_native_quotient_fold.py).
//
// With n = 2^log_n, w the n-th root, g = 5, den = 1 / (g^n - 1), Z_k the key's g1_z points
// (Z_(n-1) = infinity) and c_i = <O_i, wires> the prover's
//   sum_k h_k Z_k,  h = cosetiNTT(a_c b_c den) - den iNTT(c)
// is, with both inverse transforms written out,
//   sum_i (a_c b_c)_i E_i  +  sum_w wire_w D_w
//   E_i = (den / n) sum_k g^-k w^-ik Z_k,   L_i = (1 / n) sum_k w^-ik Z_k,
//   D_w = sum_(i < n_constraints) (-den O_iw) L_i.
// E takes the place of Z, and D_w is added to the K base of wire w (a wire K does not hold gets a
// base of its own behind the others).  The plan is O in column order with the scalar -den O_iw of
// every term as a plain integer, the form ec.h's scalar_mul takes, and the K bases' columns.
//
// Every index a kernel uses as an address comes out of fold_plan_build, which has checked it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/zkmi.h"
#include "ff.h"

namespace zk {

// O of the system on the host, and den of the key's domain
struct FoldPlanIn {
  uint32_t n_wires = 0, n_constraints = 0, n_coeffs = 0;
  const Fr* coeffs = nullptr;          // gnark's image
  const uint32_t* o_ptr = nullptr;     // n_constraints + 1 offsets
  const zkmi_term* o_terms = nullptr;
  Fr den = Fr::zero();                 // gnark's image
};
struct FoldPlan {
  std::vector<uint32_t> wires;     // the wires with a term in O whose coefficient is not 0, ascending
  std::vector<uint32_t> col_ptr;   // wires.size() + 1 offsets: the terms of column c
  std::vector<uint32_t> rows;      // constraint of every term; rows ascend inside a column, a row's
                                   // terms on one wire keep the order they have in O
  std::vector<Fr> scalars;         // (-den * coefficient) mod r, plain integer
};

ZK_HD bool fold_fr_reduced(const Fr& x) {
  for (int j = 7; j >= 0; j--)
    if (x.v[j] != FrParams::p(j)) return x.v[j] < FrParams::p(j);
  return false;
}

// den = 1 / (5^n - 1) in gnark's image
inline Fr fold_den(int log_n) {
  Fr five = Fr::zero();
  five.v[0] = 5;
  Fr p = to_mont(five);
  for (int i = 0; i < log_n; i++) p = sqr(p);
  return inverse(sub(p, Fr::one()));
}

// Returns the empty string and the plan, or what is wrong with the description.
inline std::string fold_plan_build(const FoldPlanIn& in, FoldPlan* out) {
  const std::string pre = "pk: fold_r1cs: ";
  if (in.n_constraints == 0 || in.n_wires == 0 || in.n_coeffs == 0 || in.n_coeffs >= (1u << 30) ||
      !in.coeffs)
    return pre + "n_constraints, n_wires and n_coeffs (< 2^30) must be positive";
  for (uint32_t i = 0; i < in.n_coeffs; i++)
    if (!fold_fr_reduced(in.coeffs[i]))
      return pre + "coefficient " + std::to_string(i) + " is not reduced mod r";
  bool ok = in.o_ptr && in.o_ptr[0] == 0;
  for (uint32_t k = 0; ok && k < in.n_constraints; k++) ok = in.o_ptr[k] <= in.o_ptr[k + 1];
  const uint32_t nnz = ok ? in.o_ptr[in.n_constraints] : 0;
  ok = ok && (nnz == 0 || in.o_terms);
  for (uint32_t t = 0; ok && t < nnz; t++)
    ok = in.o_terms[t].coeff < in.n_coeffs && in.o_terms[t].wire < in.n_wires;
  if (!ok)
    return pre + "malformed matrix O (offsets not monotone from 0, or a term's coefficient / wire "
                 "index out of range)";
  // -den * coefficient once per table entry; a zero coefficient adds nothing and leaves the plan
  const Fr nden = neg(in.den);
  std::vector<Fr> sc(in.n_coeffs);
  std::vector<uint8_t> zero(in.n_coeffs);
  for (uint32_t i = 0; i < in.n_coeffs; i++) {
    zero[i] = in.coeffs[i].is_zero();
    sc[i] = from_mont(mul(nden, in.coeffs[i]));
  }
  // counting sort by wire: rows stay in order inside a column
  std::vector<uint32_t> count(in.n_wires, 0);
  for (uint32_t t = 0; t < nnz; t++)
    if (!zero[in.o_terms[t].coeff]) count[in.o_terms[t].wire]++;
  FoldPlan& P = *out;
  P = FoldPlan();
  std::vector<uint32_t> at(in.n_wires, 0);
  uint32_t total = 0;
  for (uint32_t w = 0; w < in.n_wires; w++) {
    if (!count[w]) continue;
    P.wires.push_back(w);
    P.col_ptr.push_back(total);
    at[w] = total;
    total += count[w];
  }
  P.col_ptr.push_back(total);
  P.rows.resize(total);
  P.scalars.resize(total);
  for (uint32_t k = 0; k < in.n_constraints; k++)
    for (uint32_t t = in.o_ptr[k]; t < in.o_ptr[k + 1]; t++) {
      const zkmi_term& tm = in.o_terms[t];
      if (zero[tm.coeff]) continue;
      P.rows[at[tm.wire]] = k;
      P.scalars[at[tm.wire]++] = sc[tm.coeff];
    }
  return std::string();
}

// The K bases of the folded key: k_wire_out = k_wire, then every wire of the plan that k_wire does
// not hold, ascending (ONE and the public wires: at the end, so that the groups of the batch-
// varying private wires in front stay whole); col_of_base[j] = the plan's column whose D is added to
// base j, or -1.  A wire that k_wire holds twice takes its column once.
inline void fold_k_merge(const FoldPlan& P, const std::vector<uint32_t>& k_wire, uint32_t n_wires,
                         std::vector<uint32_t>* k_wire_out, std::vector<int32_t>* col_of_base) {
  std::vector<int32_t> col_of_wire(n_wires, -1);
  for (size_t c = 0; c < P.wires.size(); c++) col_of_wire[P.wires[c]] = (int32_t)c;
  *k_wire_out = k_wire;
  col_of_base->assign(k_wire.size(), -1);
  for (size_t j = 0; j < k_wire.size(); j++) {
    const uint32_t w = k_wire[j];
    if (w < n_wires && col_of_wire[w] >= 0) {
      (*col_of_base)[j] = col_of_wire[w];
      col_of_wire[w] = -1;
    }
  }
  for (size_t c = 0; c < P.wires.size(); c++)
    if (col_of_wire[P.wires[c]] >= 0) {
      k_wire_out->push_back(P.wires[c]);
      col_of_base->push_back((int32_t)c);
    }
}

}  // namespace zk
