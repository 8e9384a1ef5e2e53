// Host build of csrc/r1cs_plan.h for the tests/test_native_r1cs_{plan,hints,emul}.py: a stand-alone
// program that reads a gnark-shaped system dumped by the test, builds the solve plan for every
// requested number of sub-lanes and interprets it on the host with ff.h and emul.h -- the arithmetic
// of r1cs_solve_kernel, record by record and sub-lane by sub-lane: a step of a lookup count or of an
// emulated product gives each sub-lane its own column of the step's rows, the closing record of an
// emulated product is r1cs_emul_finish, the function the kernel calls.  The hint set comes with the
// description, so one program serves ZKMI_HINTS_BASIC, ZKMI_HINTS_STD and ZKMI_HINTS_EMULATED.  No
// hashing here: at a commitment record the interpreter takes the commitment wire's value from the
// test.
//
//   r1cs_plan_check IN OUT S_FIRST S_LAST
// IN: arrays of 32-bit words, each preceded by its length: header (n_wires, n_public, n_secret,
//   n_constraints, n_hints, hint_set), coeffs (8 words each, gnark's Montgomery image), then for L, R,
//   O the offsets and the terms (coefficient index, wire), instr, hint_kind, hint_in_ptr, hint_lc_ptr,
//   hint_terms, hint_out_ptr, hint_out, inputs (batch x n_inputs x 8 words), commitment values (batch
//   x commitments x 8 words; empty for a system without commitments).
// stdout: one line per S: the plan's figures, its emul flag and a checksum of everything written, or
//   the refusal.
// OUT: per accepted S: S, ext, records, terms, outs, the commitments (instruction, record, wire, hashed
//   wires, private wires), number of coefficients, batch, then per input: status, wires, a, b, c.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "r1cs_plan.h"

using namespace zk;

static std::vector<uint32_t> read_array(FILE* f) {
  uint32_t n = 0;
  if (fread(&n, 4, 1, f) != 1) {
    fprintf(stderr, "truncated input\n");
    exit(2);
  }
  std::vector<uint32_t> v(n);
  if (n && fread(v.data(), 4, n, f) != n) {
    fprintf(stderr, "truncated input\n");
    exit(2);
  }
  return v;
}

static uint64_t fnv = 1469598103934665603ull;
static void put(FILE* f, const void* p, size_t words) {
  if (words == 0) return;   // an empty vector's data() may be null
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < words * 4; i++) fnv = (fnv ^ b[i]) * 1099511628211ull;
  fwrite(p, 4, words, f);
}
static void put_u32(FILE* f, uint32_t x) { put(f, &x, 1); }

// a b 2^-261 as the device forms it: the Montgomery product (. 2^-256) times 2^-5
static Fr fmulp(const Fr& a, const Fr& b) {
  Fr k = Fr::zero();
  k.v[7] = 1u << 27;   // 2^251: the Montgomery image of 2^-5
  return mul(mul(a, b), k);
}

// column sl of the rows of a step record (RK_COUNT_Q, RK_EMUL_STEP): that sub-lane's own sum
static Fr column(const R1csPlan& P, const R1csRecord& r, uint32_t sl, const std::vector<Fr>& w) {
  Fr q = Fr::zero();
  for (uint32_t row = 0; row < r.mul_rows; row++) {
    const R1csTerm tm = P.terms[r.first + (size_t)row * P.S + sl];
    if (tm.wire >> 30 == RT_PAD) continue;
    q = add(q, fmulp(w[tm.wire & R1CS_IDX_MASK], P.coeffs[tm.coef & R1CS_IDX_MASK]));
  }
  return q;
}

// One proof through the plan.  Returns 0 or ZKMI_ERR_UNSATISFIED; -100 if a record is out of shape.
static int interpret(const R1csPlan& P, uint32_t n_inputs, const Fr* inputs, const Fr* commit_values,
                     std::vector<Fr>& w, std::vector<Fr>& a, std::vector<Fr>& b, std::vector<Fr>& c) {
  int st = 0;
  w[0] = Fr::one();
  for (uint32_t i = 0; i < n_inputs; i++) w[1 + i] = inputs[i];
  Fr L[8];
  for (int q = 0; q < 8; q++) L[q] = Fr::zero();
  for (size_t i = 0; i + 1 < P.records.size(); i++) {
    const R1csRecord& r = P.records[i];
    if (r.kind == RK_COUNT_Q) {
      for (uint32_t sl = 0; sl < r.k; sl++) {
        const Fr v = from_mont(column(P, r, sl, w));
        if ((v.v[1] | v.v[2] | v.v[3] | v.v[4] | v.v[5] | v.v[6] | v.v[7]) == 0 && v.v[0] < r.coef)
          w[P.outs[r.target + v.v[0]]].v[0]++;
      }
      continue;
    }
    if (r.kind == RK_EMUL_STEP) {
      // limbs target .. target + k - 1, one per sub-lane
      if (r.k == 0 || r.k > P.S || r.target + r.k > 8 || r.unit_rows) return -100;
      for (uint32_t sl = 0; sl < r.k; sl++) L[r.target + sl] = column(P, r, sl, w);
      continue;
    }
    if (r.kind == RK_EMUL_END) {
      if (r.mul_rows || r.unit_rows || (size_t)r.coef_inv + 5 > P.coeffs.size()) return -100;
      bool ok = true;
      r1cs_emul_finish(L, P.coeffs[r.coef_inv], &P.coeffs[r.coef_inv + 1], r.coef, [&](uint32_t o, const Fr& v) {
        if (o < r.k)
          w[P.outs[r.target + o]] = v;
        else
          ok = false;
      });
      if (!ok) return -100;
      continue;
    }
    Fr s[3] = {Fr::zero(), Fr::zero(), Fr::zero()};
    const size_t n = (size_t)(r.mul_rows + r.unit_rows) * P.S;
    for (size_t t = 0; t < n; t++) {
      const R1csTerm tm = P.terms[r.first + t];
      const uint32_t tag = tm.wire >> 30, unit = tm.coef >> 30;
      if (tag == RT_PAD) continue;
      const Fr x = w[tm.wire & R1CS_IDX_MASK];
      const bool product = t < (size_t)r.mul_rows * P.S;
      const Fr v = product ? fmulp(x, P.coeffs[tm.coef & R1CS_IDX_MASK]) : unit == 2 ? neg(x) : x;
      s[tag] = add(s[tag], v);
    }
    const Fr kinv = P.coeffs[r.coef_inv];
    Fr x = Fr::zero();
    switch (r.kind) {
      case RK_NBITS: {
        const Fr v = from_mont(s[0]);
        for (uint32_t j = 0; j < r.k; j++) {
          const uint32_t bit = j < 256 ? (v.v[j >> 5] >> (j & 31)) & 1u : 0u;
          w[P.outs[r.target + j]] = bit ? Fr::one() : Fr::zero();
        }
        continue;
      }
      case RK_LIMBS: {
        const Fr v = from_mont(s[0]);
        for (uint32_t j = 0; j < r.k; j++) w[P.outs[r.target + j]] = r1cs_small(r1cs_limb(v, j * r.coef, r.coef));
        continue;
      }
      case RK_BYTEOP: {
        const uint32_t u = from_mont(s[0]).v[0], v = from_mont(s[1]).v[0];
        w[r.target] = r1cs_small(r.coef == 1 ? u ^ v : u & v);
        continue;
      }
      case RK_COUNT_BEGIN:
        for (uint32_t j = 0; j < r.k; j++) w[P.outs[r.target + j]] = Fr::zero();
        continue;
      case RK_COUNT_END:
        for (uint32_t j = 0; j < r.k; j++) w[P.outs[r.target + j]] = r1cs_small(w[P.outs[r.target + j]].v[0]);
        continue;
      case RK_COMMIT:
        w[r.target] = commit_values[r.k];
        continue;
      case RK_INVZERO:
        w[r.target] = inverse(s[0]);
        continue;
      case RK_ASSERT:
        if (mul(s[0], s[1]) != s[2]) st = ZKMI_ERR_UNSATISFIED;
        break;
      case RK_SOLVE_O: {
        const Fr ab = mul(s[0], s[1]);
        x = fmulp(sub(ab, s[2]), kinv);
        s[2] = ab;
        break;
      }
      default: {   // RK_SOLVE_L, RK_SOLVE_R
        const int mine = r.kind == RK_SOLVE_L ? 0 : 1, other = 1 - mine;
        if (s[other].is_zero()) st = ZKMI_ERR_UNSATISFIED;
        const Fr q = mul(s[2], inverse(s[other]));
        x = fmulp(sub(q, s[mine]), kinv);
        s[mine] = q;
      }
    }
    if (r.kind != RK_ASSERT) w[r.target] = x;
    a[r.k] = s[0];
    b[r.k] = s[1];
    c[r.k] = s[2];
  }
  return st;
}

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: r1cs_plan_check IN OUT S_FIRST S_LAST\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  FILE* o = fopen(argv[2], "wb");
  if (!f || !o) {
    fprintf(stderr, "cannot open the files\n");
    return 2;
  }
  const std::vector<uint32_t> hdr = read_array(f), cw = read_array(f);
  std::vector<uint32_t> ptr[3], tw[3];
  for (int s = 0; s < 3; s++) {
    ptr[s] = read_array(f);
    tw[s] = read_array(f);
  }
  const std::vector<uint32_t> instr = read_array(f), hkind = read_array(f), in_ptr = read_array(f),
                              lc_ptr = read_array(f), hterms = read_array(f), out_ptr = read_array(f),
                              houts = read_array(f), inw = read_array(f), cvw = read_array(f);
  fclose(f);
  if (hdr.size() != 6) return 2;
  const uint32_t n_wires = hdr[0], n_public = hdr[1], n_secret = hdr[2], n_constraints = hdr[3],
                 n_hints = hdr[4];
  const uint32_t n_coeffs = (uint32_t)(cw.size() / 8), n_inputs = n_public - 1 + n_secret;
  // what zkmi_r1cs_load does to the system: coefficients lifted by 2^5, +1 / -1 marked in the terms
  std::vector<Fr> coeffs(n_coeffs);
  std::vector<uint8_t> unit(n_coeffs);
  const Fr one = Fr::one(), minus_one = neg(Fr::one());
  for (uint32_t i = 0; i < n_coeffs; i++) {
    Fr x;
    memcpy(x.v, &cw[8 * (size_t)i], 32);
    unit[i] = x == one ? 1 : x == minus_one ? 2 : 0;
    for (int t = 0; t < 5; t++) x = add(x, x);
    coeffs[i] = x;
  }
  std::vector<R1csTerm> terms[3];
  for (int s = 0; s < 3; s++)
    for (size_t t = 0; t + 1 < tw[s].size(); t += 2) {
      const uint32_t cid = tw[s][t], wire = tw[s][t + 1];
      terms[s].push_back(R1csTerm{wire, cid | (uint32_t)(cid < n_coeffs ? unit[cid] : 0) << 30});
    }
  std::vector<zkmi_term> ht;
  for (size_t t = 0; t + 1 < hterms.size(); t += 2) ht.push_back(zkmi_term{hterms[t], hterms[t + 1]});
  zkmi_r1cs_solver_desc d;
  memset(&d, 0, sizeof d);
  d.n_public = n_public;
  d.n_secret = n_secret;
  d.n_instr = (uint32_t)(instr.size() / 2);
  d.n_hints = n_hints;
  d.instr = instr.data();
  d.hint_kind = hkind.data();
  d.hint_in_ptr = in_ptr.data();
  d.hint_lc_ptr = lc_ptr.data();
  d.hint_terms = ht.data();
  d.hint_out_ptr = out_ptr.data();
  d.hint_out = houts.data();
  d.hint_set = hdr[5];
  R1csPlanIn in;
  in.n_wires = n_wires;
  in.n_constraints = n_constraints;
  in.n_coeffs = n_coeffs;
  in.coeffs = coeffs.data();
  for (int s = 0; s < 3; s++) {
    in.ptr[s] = ptr[s].data();
    in.terms[s] = terms[s].data();
  }
  in.desc = &d;
  const size_t batch = n_inputs ? inw.size() / ((size_t)n_inputs * 8) : 0;
  for (int S = atoi(argv[3]); S <= atoi(argv[4]); S++) {
    d.lanes_per_proof = (uint32_t)S;
    R1csPlan P;
    const std::string err = r1cs_plan_build(in, &P);
    if (!err.empty()) {
      printf("S=%d refused: %s\n", S, err.c_str());
      continue;
    }
    fnv = 1469598103934665603ull;
    put_u32(o, P.S);
    put_u32(o, P.ext);
    put_u32(o, (uint32_t)P.records.size());
    put(o, P.records.data(), P.records.size() * 8);
    put_u32(o, (uint32_t)P.terms.size());
    put(o, P.terms.data(), P.terms.size() * 2);
    put_u32(o, (uint32_t)P.outs.size());
    put(o, P.outs.data(), P.outs.size());
    put_u32(o, (uint32_t)P.commits.size());
    for (const R1csCommit& cm : P.commits) {
      put_u32(o, cm.instr);
      put_u32(o, cm.record);
      put_u32(o, cm.wire);
      put_u32(o, (uint32_t)cm.hashed.size());
      put(o, cm.hashed.data(), cm.hashed.size());
      put_u32(o, (uint32_t)cm.priv.size());
      put(o, cm.priv.data(), cm.priv.size());
    }
    put_u32(o, (uint32_t)P.coeffs.size());
    put_u32(o, (uint32_t)batch);
    if (cvw.size() != batch * P.commits.size() * 8) {
      fprintf(stderr, "commitment values: %zu words for %zu proofs x %zu commitments\n", cvw.size(), batch,
              P.commits.size());
      return 2;
    }
    std::vector<Fr> w(n_wires), a(n_constraints), b(n_constraints), c(n_constraints);
    for (size_t p = 0; p < batch; p++) {
      std::vector<Fr> inputs(n_inputs);
      memcpy(inputs.data(), &inw[p * n_inputs * 8], (size_t)n_inputs * 32);
      std::vector<Fr> cv(P.commits.size());
      if (!cv.empty()) memcpy(cv.data(), &cvw[p * cv.size() * 8], cv.size() * 32);
      put_u32(o, (uint32_t)interpret(P, n_inputs, inputs.data(), cv.data(), w, a, b, c));
      put(o, w.data(), (size_t)n_wires * 8);
      put(o, a.data(), (size_t)n_constraints * 8);
      put(o, b.data(), (size_t)n_constraints * 8);
      put(o, c.data(), (size_t)n_constraints * 8);
    }
    printf("S=%d ok lanes=%u emul=%d instr=%u terms=%llu longest=%u inversions=%u plan_terms=%zu coeffs=%zu "
           "fnv=%016llx\n", S, P.S, (int)P.emul, P.n_instr, (unsigned long long)P.n_terms, P.longest,
           P.n_inversions, P.terms.size(), P.coeffs.size(), (unsigned long long)fnv);
  }
  fclose(o);
  return 0;
}
