// Host check of csrc/quotient_fold.h (tests/test_native_quotient_fold.py builds it plain and with
// -fsanitize=address,undefined): the fold plan of a hand-made O against a dense matrix, every
// scalar against (-den * coefficient) mod r from the 256-bit arithmetic below, the K merge, and the
// refusals.  Prints one line per check; exit status 1 at the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "quotient_fold.h"

using namespace zk;

// ---- 256-bit reference arithmetic mod r, nothing shared with ff.h ---------------------------------
struct U256 {
  uint64_t w[4];
};
static const U256 RMOD = {{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull,
                           0x30644e72e131a029ull}};
static bool geq(const U256& a, const U256& b) {
  for (int i = 3; i >= 0; i--)
    if (a.w[i] != b.w[i]) return a.w[i] > b.w[i];
  return true;
}
static U256 sub_raw(const U256& a, const U256& b) {
  U256 r;
  unsigned __int128 borrow = 0;
  for (int i = 0; i < 4; i++) {
    const unsigned __int128 d = (unsigned __int128)a.w[i] - b.w[i] - borrow;
    r.w[i] = (uint64_t)d;
    borrow = (d >> 64) & 1;
  }
  return r;
}
// a + b mod r for a, b < r (r < 2^254: the sum fits)
static U256 addm(const U256& a, const U256& b) {
  U256 r;
  unsigned __int128 carry = 0;
  for (int i = 0; i < 4; i++) {
    const unsigned __int128 s = (unsigned __int128)a.w[i] + b.w[i] + carry;
    r.w[i] = (uint64_t)s;
    carry = s >> 64;
  }
  return geq(r, RMOD) ? sub_raw(r, RMOD) : r;
}
static U256 mulm(const U256& a, const U256& b) {
  U256 acc = {{0, 0, 0, 0}};
  for (int i = 255; i >= 0; i--) {
    acc = addm(acc, acc);
    if ((b.w[i >> 6] >> (i & 63)) & 1) acc = addm(acc, a);
  }
  return acc;
}
static U256 powm(U256 a, const U256& e) {
  U256 r = {{1, 0, 0, 0}};
  for (int i = 255; i >= 0; i--) {
    r = mulm(r, r);
    if ((e.w[i >> 6] >> (i & 63)) & 1) r = mulm(r, a);
  }
  return r;
}
static U256 small(uint64_t x) { return U256{{x, 0, 0, 0}}; }
static U256 negm(const U256& a) { return geq(small(0), a) ? a : sub_raw(RMOD, a); }
// x * 2^256 mod r: gnark's image, as 8 x u32
static Fr image(const U256& x) {
  U256 m = x;
  for (int i = 0; i < 256; i++) m = addm(m, m);
  Fr r;
  for (int i = 0; i < 4; i++) {
    r.v[2 * i] = (uint32_t)m.w[i];
    r.v[2 * i + 1] = (uint32_t)(m.w[i] >> 32);
  }
  return r;
}
static bool same(const Fr& a, const U256& b) {
  for (int i = 0; i < 4; i++)
    if (a.v[2 * i] != (uint32_t)b.w[i] || a.v[2 * i + 1] != (uint32_t)(b.w[i] >> 32)) return false;
  return true;
}

static void fail(const char* what) {
  std::printf("FAILED: %s\n", what);
  std::exit(1);
}

int main() {
  const int log_n = 4;   // den depends on the domain alone
  // den = 1 / (5^16 - 1) by Fermat, and through ff.h
  U256 rm2 = sub_raw(RMOD, small(2));
  const U256 den = powm(sub_raw(powm(small(5), small(16)), small(1)), rm2);
  if (!same(from_mont(fold_den(log_n)), den)) fail("fold_den");
  std::printf("ok den\n");

  // coefficient table: 1, -1, 7, a large value, 0, 2^253 + 11
  std::vector<U256> cv = {small(1), sub_raw(RMOD, small(1)), small(7),
                          U256{{0x123456789abcdef0ull, 0xfedcba9876543210ull, 0x0f1e2d3c4b5a6978ull,
                                0x2000000000000000ull}},
                          small(0), U256{{11, 0, 0, 0x2000000000000000ull}}};
  std::vector<Fr> coeffs;
  for (const U256& c : cv) coeffs.push_back(image(c));

  // O by hand: 9 wires, 13 constraints.  wire 0 (ONE): a term in every row, two in row 4; wire 1
  // (public): rows 2, 9; wire 2 (public): none; wire 3: none (empty column); wire 4: one term;
  // wire 5: only a term with coefficient 0 (leaves the plan); wire 6: rows 0, 6, 12; wire 7: rows 3,
  // 11 (K lacks it); wire 8: row 12
  const uint32_t NW = 9, NC = 13;
  std::vector<std::vector<zkmi_term>> rows(NC);
  for (uint32_t k = 0; k < NC; k++) rows[k].push_back({k % 4 == 3 ? 5u : k % 4, 0});
  rows[4].push_back({3, 0});
  rows[2].insert(rows[2].begin(), {2, 1});
  rows[9].push_back({1, 1});
  rows[7].push_back({0, 4});
  rows[5].insert(rows[5].begin(), {4, 5});
  rows[0].push_back({3, 6});
  rows[6].insert(rows[6].begin(), {2, 6});
  rows[12].push_back({5, 6});
  rows[3].push_back({1, 7});
  rows[11].push_back({2, 7});
  rows[12].push_back({0, 8});
  std::vector<uint32_t> o_ptr = {0};
  std::vector<zkmi_term> terms;
  for (auto& r : rows) {
    for (auto& t : r) terms.push_back(t);
    o_ptr.push_back((uint32_t)terms.size());
  }
  FoldPlanIn in;
  in.n_wires = NW;
  in.n_constraints = NC;
  in.n_coeffs = (uint32_t)coeffs.size();
  in.coeffs = coeffs.data();
  in.o_ptr = o_ptr.data();
  in.o_terms = terms.data();
  in.den = fold_den(log_n);
  FoldPlan P;
  std::string err = fold_plan_build(in, &P);
  if (!err.empty()) fail(err.c_str());

  // the dense matrix: per (row, wire) the coefficient indices in O's order
  std::vector<std::vector<uint32_t>> dense(NC * NW);
  for (uint32_t k = 0; k < NC; k++)
    for (auto& t : rows[k])
      if (t.coeff != 4) dense[k * NW + t.wire].push_back(t.coeff);
  std::vector<uint32_t> want_wires;
  for (uint32_t w = 0; w < NW; w++) {
    bool any = false;
    for (uint32_t k = 0; k < NC; k++) any = any || !dense[k * NW + w].empty();
    if (any) want_wires.push_back(w);
  }
  if (P.wires != want_wires || want_wires != std::vector<uint32_t>{0, 1, 4, 6, 7, 8}) fail("wires");
  if (P.col_ptr.size() != P.wires.size() + 1 || P.col_ptr[0] != 0) fail("col_ptr shape");
  const U256 nden = negm(den);
  uint32_t at = 0;
  for (size_t c = 0; c < P.wires.size(); c++) {
    if (P.col_ptr[c] != at) fail("col_ptr");
    for (uint32_t k = 0; k < NC; k++)
      for (uint32_t cid : dense[k * NW + P.wires[c]]) {
        if (at >= P.rows.size() || P.rows[at] != k) fail("term order");
        if (!same(P.scalars[at], mulm(nden, cv[cid]))) fail("scalar");
        at++;
      }
  }
  if (P.col_ptr.back() != at || P.rows.size() != at || P.scalars.size() != at) fail("term count");
  if (P.col_ptr[1] - P.col_ptr[0] != 14 || P.col_ptr[3] - P.col_ptr[2] != 1) fail("column lengths");
  std::printf("ok plan terms=%u columns=%zu\n", at, P.wires.size());

  // K holds the private wires 3 .. 6 and 8 (not 7), wire 6 twice
  std::vector<uint32_t> kw = {3, 4, 5, 6, 6, 8}, kw_out;
  std::vector<int32_t> cob;
  fold_k_merge(P, kw, NW, &kw_out, &cob);
  if (kw_out != std::vector<uint32_t>{3, 4, 5, 6, 6, 8, 0, 1, 7}) fail("k_wire_out");
  if (cob != std::vector<int32_t>{-1, 2, -1, 3, -1, 5, 0, 1, 4}) fail("col_of_base");
  std::printf("ok merge bases=%zu\n", kw_out.size());

  // refusals
  const std::string bad_o = "pk: fold_r1cs: malformed matrix O (offsets not monotone from 0, or a "
                            "term's coefficient / wire index out of range)";
  {
    std::vector<zkmi_term> t2 = terms;
    t2[5].wire = NW;
    FoldPlanIn i2 = in;
    i2.o_terms = t2.data();
    if (fold_plan_build(i2, &P) != bad_o) fail("wire out of range accepted");
  }
  {
    std::vector<zkmi_term> t2 = terms;
    t2[terms.size() - 1].coeff = in.n_coeffs;
    FoldPlanIn i2 = in;
    i2.o_terms = t2.data();
    if (fold_plan_build(i2, &P) != bad_o) fail("coefficient index out of range accepted");
  }
  {
    std::vector<uint32_t> p2 = o_ptr;
    p2[4] = p2[5] + 1;
    FoldPlanIn i2 = in;
    i2.o_ptr = p2.data();
    if (fold_plan_build(i2, &P) != bad_o) fail("non-monotone o_ptr accepted");
    p2 = o_ptr;
    p2[0] = 1;
    if (fold_plan_build(i2, &P) != bad_o) fail("o_ptr[0] != 0 accepted");
  }
  {
    std::vector<Fr> c2 = coeffs;
    for (int i = 0; i < 8; i++) c2[2].v[i] = FrParams::p(i);   // r itself
    FoldPlanIn i2 = in;
    i2.coeffs = c2.data();
    if (fold_plan_build(i2, &P) != "pk: fold_r1cs: coefficient 2 is not reduced mod r")
      fail("coefficient >= r accepted");
  }
  {
    FoldPlanIn i2 = in;
    i2.n_coeffs = 0;
    if (fold_plan_build(i2, &P).empty()) fail("empty coefficient table accepted");
  }
  std::printf("ok refusals\n");
  return 0;
}
