// Host check of csrc/scs_plan.h (tests/test_native_scs_plan.py, tests/test_native_scs_std_plan.py):
// reads a sparse system, a solver description and a batch of inputs, builds the plan for every
// lanes_per_proof in [first, last], asserts the plan's two guarantees on every step -- with the three
// phases of a lookup count and the boundaries of the commitment hints --, interprets it with
// scs_record_run and checks every gate of the wires it solved but the rows of the commitments (the
// status is the OR of a zero divisor and a gate that does not hold).
//   usage: scs_plan_check IN OUT first last max_set
// max_set: the highest hint set the caller can run, the third argument of scs_plan_build
// (0 = ZKMI_HINTS_BASIC, 1 = ZKMI_HINTS_STD).
// IN: sections of (count, count uint32 words): header (n_wires, n_gates, n_public, n_inputs, n_hints,
// hint_set), xa, xb, xc, selectors, input_wire, instr, hint_kind, hint_in_ptr, hint_in_wire,
// hint_in_coef, hint_out_ptr, hint_out, inputs, and the gate rows the check skips (committed rows and
// commitment rows, which hold by construction; empty for a system without commitments).
// A commitment's challenge is a stand-in the Python side repeats: 1 + index + sum_j (j + 1) v_j over
// the committed values, in the field.
// stdout, per lane count: "S=<s> error: <message>" or
// "S=<s> ok lanes records steps levels inversions std hash | instr step wire n_wires | ..." (hash: of
// the records, the coefficient table and outs; one group per commitment hint).
// OUT, per accepted plan: S, batch, then per proof status and n_wires x 8 words.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scs_plan.h"

using namespace zk;

static std::vector<uint32_t> section(FILE* f) {
  uint32_t n = 0;
  if (fread(&n, 4, 1, f) != 1) {
    fprintf(stderr, "short input\n");
    exit(2);
  }
  std::vector<uint32_t> v(n);
  if (n && fread(v.data(), 4, n, f) != n) {
    fprintf(stderr, "short input\n");
    exit(2);
  }
  return v;
}

static void fail(uint32_t S, uint32_t step, const char* what, uint32_t wire) {
  printf("S=%u guarantee broken at step %u: %s (wire %u)\n", S, step, what, wire);
  exit(1);
}

static Fr small(uint64_t x) { return r1cs_small(x); }

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const uint32_t max_set = (uint32_t)atoi(argv[5]);
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const auto header = section(f), xa = section(f), xb = section(f), xc = section(f), sel = section(f),
             input_wire = section(f), instr = section(f), hint_kind = section(f), hint_in_ptr = section(f),
             hint_in_wire = section(f), hint_in_coef = section(f), hint_out_ptr = section(f),
             hint_out = section(f), inputs = section(f), skip_rows = section(f);
  fclose(f);
  if (header.size() != 6) return 2;
  const uint32_t n_wires = header[0], n_gates = header[1], n_inputs = header[3];
  std::vector<Fr> fsel(sel.size() / 8), fcoef(hint_in_coef.size() / 8), fin(inputs.size() / 8);
  if (!sel.empty()) memcpy((void*)fsel.data(), sel.data(), fsel.size() * 32);
  if (!hint_in_coef.empty()) memcpy((void*)fcoef.data(), hint_in_coef.data(), fcoef.size() * 32);
  if (!inputs.empty()) memcpy((void*)fin.data(), inputs.data(), fin.size() * 32);
  zkmi_scs_solver_desc d{};
  d.n_inputs = n_inputs;
  d.input_wire = input_wire.data();
  d.n_instr = (uint32_t)(instr.size() / 2);
  d.n_hints = header[4];
  d.instr = instr.data();
  d.hint_kind = hint_kind.data();
  d.hint_in_ptr = hint_in_ptr.data();
  d.hint_in_wire = hint_in_wire.data();
  d.hint_in_coef = fcoef.data();
  d.hint_out_ptr = hint_out_ptr.data();
  d.hint_out = hint_out.data();
  d.hint_set = header[5];
  ScsPlanIn in;
  in.n_wires = n_wires;
  in.n_gates = n_gates;
  in.n_public = header[2];
  in.x[0] = xa.data();
  in.x[1] = xb.data();
  in.x[2] = xc.data();
  in.sel = fsel.data();
  in.desc = &d;
  if (xa.size() != n_gates || xb.size() != n_gates || xc.size() != n_gates || fsel.size() != 5 * (size_t)n_gates ||
      input_wire.size() != n_inputs)
    return 2;
  std::vector<uint8_t> skip(n_gates, 0);
  for (uint32_t g : skip_rows)
    if (g < n_gates) skip[g] = 1;
  const size_t batch = n_inputs ? fin.size() / n_inputs : 1;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  for (uint32_t S = (uint32_t)atoi(argv[3]); S <= (uint32_t)atoi(argv[4]); S++) {
    d.lanes_per_proof = S;
    ScsPlan P;
    const std::string err = scs_plan_build(in, &P, max_set);
    if (!err.empty()) {
      printf("S=%u error: %s\n", S, err.c_str());
      continue;
    }
    if (P.records.size() != ((size_t)P.n_steps + 1) * P.S) fail(S, 0, "records are not n_steps + 1 steps", 0);
    // the two guarantees, step by step: -2 = never written, -1 = an input, else the writing step.
    // A counter: zeroed[w] = the step that zeroed it, counted[w] = the last step that counted in its
    // table; its wire is written, for the readers, by COUNT_END alone.
    std::vector<int64_t> when(n_wires, -2), zeroed(n_wires, -2), counted(n_wires, -2);
    for (uint32_t w : P.input_wire)
      if (w != SCS_NONE) when[w] = -1;
    uint32_t stores = 0, next_commit = 0, last_boundary = 0;
    bool any_std = false;
    for (uint32_t t = 0; t <= P.n_steps; t++) {
      // the commitments whose boundary is here: their committed wires are written, their wire is
      // written between step t - 1 and step t
      for (; next_commit < P.commits.size() && P.commits[next_commit].step == t; next_commit++) {
        const ScsPlan::Commit& c = P.commits[next_commit];
        if (c.step < last_boundary) fail(S, t, "boundaries decrease", c.wire);
        last_boundary = c.step;
        for (uint32_t w : c.wires)
          if (w >= n_wires || when[w] == -2 || when[w] >= (int64_t)t)
            fail(S, t, "a committed wire is not written before the boundary", w);
        if (c.wire >= n_wires || when[c.wire] != -2) fail(S, t, "the commitment wire is written twice", c.wire);
        when[c.wire] = (int64_t)t - 1;
      }
      const uint32_t cls = scs_record_class(P.records[(size_t)t * P.S]);
      for (uint32_t s = 0; s < P.S; s++) {
        const ScsRecord& r = P.records[(size_t)t * P.S + s];
        if (r.coef >= P.coefs.size() / SCS_COEF_ROW) fail(S, t, "coefficient row out of range", r.coef);
        if (t < P.n_steps && scs_record_class(r) != cls) fail(S, t, "two classes in one step", s);
        if (r.xcls && ((r.ctl >> SCS_CTL_CLASS) & 3)) fail(S, t, "a std record with class bits in ctl", s);
        if (r.xcls && (r.xcls < SK_LIMBS || r.xcls > SK_COUNT_END)) fail(S, t, "unknown class", r.xcls);
        if (t == P.n_steps && ((r.ctl & SCS_CTL_STORE) || r.xcls)) fail(S, t, "the slack stores", s);
        const uint32_t rd[3] = {r.wa, r.wb, r.wc};
        for (int c = 0; c < 3; c++)
          if (r.ctl >> (SCS_CTL_READ + c) & 1) {
            if (rd[c] >= n_wires) fail(S, t, "read out of range", rd[c]);
            if (when[rd[c]] == -2 || when[rd[c]] >= (int64_t)t)
              fail(S, t, "reads a wire that no earlier step wrote", rd[c]);
          }
      }
      for (uint32_t s = 0; s < P.S; s++) {
        const ScsRecord& r = P.records[(size_t)t * P.S + s];
        if (!(r.ctl & SCS_CTL_STORE)) continue;
        stores++;
        const uint32_t k = scs_record_class(r);
        any_std = any_std || k >= SK_LIMBS;
        const bool listed = k == SK_NBITS || k == SK_LIMBS || k == SK_COUNT_ZERO || k == SK_COUNT_END;
        if (k == SK_COUNT_Q) {
          // the whole table is zeroed earlier and not read back yet
          if (r.aux == 0 || (uint64_t)r.target + r.aux > P.outs.size()) fail(S, t, "table out of range", r.target);
          for (uint32_t j = 0; j < r.aux; j++) {
            const uint32_t w = P.outs[r.target + j];
            if (w >= n_wires) fail(S, t, "counter out of range", w);
            if (zeroed[w] == -2 || zeroed[w] >= (int64_t)t) fail(S, t, "counts before the counter is zeroed", w);
            if (when[w] != -2) fail(S, t, "counts after the read-back", w);
            counted[w] = t;
          }
          continue;
        }
        const uint32_t cnt = listed ? (r.aux >> 16) & (k == SK_LIMBS ? 0xffu : 0xffffu) : 1;
        if (k == SK_LIMBS && (r.aux >> 24 < 1 || r.aux >> 24 > 64)) fail(S, t, "limb width", r.aux >> 24);
        if (k == SK_BYTEOP && r.aux != 1 && r.aux != 2) fail(S, t, "byte operation", r.aux);
        for (uint32_t j = 0; j < cnt; j++) {
          if (listed && r.target + j >= P.outs.size()) fail(S, t, "output index out of range", r.target + j);
          const uint32_t w = listed ? P.outs[r.target + j] : r.target;
          if (w >= n_wires) fail(S, t, "store out of range", w);
          if (when[w] != -2) fail(S, t, "writes a wire twice", w);
          if (k == SK_COUNT_ZERO) {
            if (zeroed[w] != -2) fail(S, t, "zeroes a counter twice", w);
            zeroed[w] = t;
            continue;
          }
          if (k == SK_COUNT_END && (zeroed[w] == -2 || zeroed[w] >= (int64_t)t || counted[w] >= (int64_t)t))
            fail(S, t, "reads a counter back in or before a step that writes it", w);
          if (k != SK_COUNT_END && zeroed[w] != -2) fail(S, t, "writes a counter", w);
          when[w] = t;
        }
      }
    }
    if (next_commit != P.commits.size()) fail(S, P.n_steps, "a boundary behind the last step", next_commit);
    if (stores != P.n_records) fail(S, 0, "storing records differ from n_records", stores);
    if (any_std != P.std_records) fail(S, 0, "std_records is wrong", any_std);
    for (uint32_t w = 0; w < n_wires; w++)
      if (when[w] == -2) fail(S, P.n_steps, "wire never written", w);
    // FNV-1a over the records, the coefficient table and outs: two plans with the same figure are the
    // same record for record
    uint64_t fnv = 1469598103934665603ull;
    auto mix = [&](const void* p, size_t bytes) {
      for (size_t i = 0; i < bytes; i++) fnv = (fnv ^ ((const uint8_t*)p)[i]) * 1099511628211ull;
    };
    mix(P.records.data(), P.records.size() * sizeof(ScsRecord));
    mix((const void*)P.coefs.data(), P.coefs.size() * 32);
    mix(P.outs.data(), P.outs.size() * 4);
    printf("S=%u ok %u %u %u %u %u %u %016llx", S, P.S, P.n_records, P.n_steps, P.n_levels, P.n_inversions,
           (unsigned)P.std_records, (unsigned long long)fnv);
    for (const ScsPlan::Commit& c : P.commits)
      printf(" | %u %u %u %u", c.instr, c.step, c.wire, (unsigned)c.wires.size());
    printf("\n");
    const uint32_t head[2] = {P.S, (uint32_t)batch};
    fwrite(head, 4, 2, o);
    for (size_t b = 0; b < batch; b++) {
      std::vector<Fr> w(n_wires, Fr::zero());
      for (uint32_t i = 0; i < n_inputs; i++)
        if (P.input_wire[i] != SCS_NONE) w[P.input_wire[i]] = fin[b * n_inputs + i];
      int32_t status = 0;
      // all reads of a step before its writes, as the sub-lanes of a wavefront run it; the counts of
      // a step apply one after the other, as the atomics do
      std::vector<std::pair<uint32_t, Fr>> writes;
      size_t ci = 0;
      for (uint32_t t = 0; t <= P.n_steps; t++) {
        for (; ci < P.commits.size() && P.commits[ci].step == t; ci++) {
          Fr h = small(1 + ci);
          for (size_t j = 0; j < P.commits[ci].wires.size(); j++)
            h = add(h, mul(small(j + 1), w[P.commits[ci].wires[j]]));
          w[P.commits[ci].wire] = h;
        }
        if (t == P.n_steps) break;
        writes.clear();
        const bool counting = scs_record_class(P.records[(size_t)t * P.S]) == SK_COUNT_Q;
        for (uint32_t s = 0; s < P.S; s++)
          if (!scs_record_run(P.records[(size_t)t * P.S + s], P.coefs.data(), P.outs.data(),
                              [&](uint32_t x) { return w[x]; },
                              [&](uint32_t x, const Fr& v) {
                                if (counting)
                                  w[x] = v;
                                else
                                  writes.emplace_back(x, v);
                              }))
            status = ZKMI_ERR_UNSATISFIED;
        for (auto& wv : writes) w[wv.first] = wv.second;
      }
      // every gate of the solved wires but the rows of the commitments
      for (uint32_t g = 0; g < n_gates; g++) {
        if (skip[g]) continue;
        const Fr a = w[xa[g]], bb = w[xb[g]], c = w[xc[g]];
        const Fr* q = fsel.data() + g;
        Fr sum = add(add(mul(q[0], a), mul(q[n_gates], bb)), mul(q[2 * (size_t)n_gates], c));
        sum = add(add(sum, mul(q[3 * (size_t)n_gates], mul(a, bb))), q[4 * (size_t)n_gates]);
        if (g < in.n_public) sum = sub(sum, a);
        if (!sum.is_zero()) status = ZKMI_ERR_UNSATISFIED;
      }
      fwrite(&status, 4, 1, o);
      fwrite((const void*)w.data(), 32, n_wires, o);
    }
  }
  fclose(o);
  return 0;
}
