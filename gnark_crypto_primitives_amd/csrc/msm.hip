// Batched multi-scalar multiplication over fixed bases: out[p] = sum_i s[i][p] * P_i, p < batch.
//
// Replaces G1Jac.MultiExp / G2Jac.MultiExp (gnark-crypto ecc/bn254/multiexp*.go) as groth16.Prove
// calls them - four G1 and one G2 MSM per proof over the proving key's bases
// [UPSTREAM-RECALL, SURVEY.md §3.2 step 5].  The result is the affine group element, which is
// canonical, so it equals gnark's bucket-method result bit for bit.
//
// MI355X-first design.  gnark runs Pippenger per proof because a CPU sees one
// proof at a time.  Here a batch of proofs shares the bases, and the bases are fixed for the
// lifetime of the circuit, so the work is organised the other way round: multiples of the bases are
// precomputed in HBM, one lane = one proof, and every step is ONE mixed addition of a gathered
// table entry into a register-resident XYZZ accumulator -- no buckets, no bucket reduction, no
// sorting, no atomics.  Three table layouts, chosen per key by the additions they need within
// the HBM budget:
//   * comb tables (default for keys of >= 4096 bases): a joint table of all subset sums of every
//     group of k consecutive bases, 254 one-bit windows: 254 / k additions per (base, proof)
//     (k = 18 / 19 for the Arbo-160 key).  Window index = a grid dimension; the 254 window sums of
//     a proof are combined by Horner's rule.  Groups whose scalars are the same in every proof of
//     the batch are summed once per batch (comb_common_sums), the others per lane.
//   * one shared table per base (d * P, d = 1..2^(c-1)), ceil(255 / c) signed-digit windows with
//     their own accumulators, Horner combine (explicit window_bits 100 + c).
//   * per-window tables (d * 2^(shift_j) * P for every window j), all windows into one
//     accumulator: no Horner tail, the right shape for small keys and for the one-base delta
//     multiples of the assembly.
// The bound is the vector integer ALU (v_mad_u64_u32), not HBM; both fractions are reported by
// bench.py.
//
// Algorithmic bytes per launch: n * sizeof(affine) + batch * n * 32.
//
// This file: the window plans and the entry points of zkmi_internal.h, which pick the group's
// coordinate field and go on in the templates of msm_impl.h.  msm_g2.hip is the second translation
// unit of the MSM.
#include "msm_impl.h"
#include "comb_plan.h"

namespace zk {

// ---- window plans ----------------------------------------------------------------------------------
WinPlan plan_with_windows(int W) {
  WinPlan p;
  if (W < 16) W = 16;     // 16-bit windows at most
  if (W > 64) W = 64;
  p.W = W;
  const int c0 = 255 / W, rem = 255 - c0 * W;
  uint32_t off = 0;
  for (int j = 0; j < W; j++) {
    p.bits[j] = (uint8_t)(j < rem ? c0 + 1 : c0);
    p.off[j] = off;
    off += 1u << (p.bits[j] - 1);
  }
  p.per_base = off;
  return p;
}
WinPlan plan_uniform(int c) {   // ceil(255 / c) windows of c bits (covers >= 255 bits)
  WinPlan p;
  p.W = (255 + c - 1) / c;
  uint32_t off = 0;
  for (int j = 0; j < p.W; j++) {
    p.bits[j] = (uint8_t)c;
    p.off[j] = off;
    off += 1u << (c - 1);
  }
  p.per_base = off;
  return p;
}
WinPlan plan_shared(int c) {   // ceil(255 / c) windows over ONE table of 2^(c-1) multiples
  WinPlan p;
  if (c < 4) c = 4;     // at most 64 windows
  if (c > 16) c = 16;   // digits are stored as int16
  p.shared = 1;
  p.W = (255 + c - 1) / c;
  for (int j = 0; j < p.W; j++) {
    p.bits[j] = (uint8_t)(j + 1 < p.W ? c : 255 - (p.W - 1) * c);
    p.off[j] = 0;
  }
  p.per_base = 1u << (c - 1);
  return p;
}
WinPlan plan_comb(int k, bool signed_tables) {
  WinPlan p;
  if (k < 2) k = 2;
  if (k > 21) k = 21;
  if (!signed_tables && k > 20) k = 20;
  p.comb = (uint8_t)k;
  p.comb_signed = signed_tables ? 1 : 0;
  p.W = COMB_W + (signed_tables ? 1 : 0);   // + the parity-correction window
  p.per_base = 0;
  return p;
}
// Comb plan with one group size per group of the key (comb_plan.h, where the prices of the
// additions are; zkmi_pk_load plans each MSM on its own with comb_plan_search)
void plan_comb_for_budget(size_t n1, size_t n2, double usable_bytes, int* k1, int* k2, bool* sg1,
                          bool* sg2, bool allow_signed) {
  comb_plan_equal(n1, n2, usable_bytes, k1, k2, sg1, sg2, allow_signed);
}
// Widths of the shared tables of a key: the (c1, c2) that minimises n1 * W(c1) + 3 * n2 * W(c2)
// (a G2 mixed addition costs about three G1 ones) among those whose tables fit `usable_bytes`.
void plan_shared_for_budget(size_t n1, size_t n2, double usable_bytes, int* c1, int* c2) {
  double best = 1e300;
  *c1 = *c2 = 4;
  for (int a = 4; a <= 16; a++)
    for (int b = 4; b <= 16; b++) {
      const double bytes = (double)n1 * (1u << (a - 1)) * 64.0 + (double)n2 * (1u << (b - 1)) * 128.0;
      if (bytes > usable_bytes) continue;
      const double cost = (double)n1 * ((255 + a - 1) / a) + 3.0 * (double)n2 * ((255 + b - 1) / b);
      if (cost < best) {
        best = cost;
        *c1 = a;
        *c2 = b;
      }
    }
}
WinPlan plan_windows_for_budget(size_t n_total, int group, double budget_bytes) {
  const double entry = group == 1 ? 64.0 : 128.0;
  for (int W = 16; W <= 64; W++) {
    WinPlan p = plan_with_windows(W);
    if ((double)n_total * p.per_base * entry <= budget_bytes) return p;
  }
  return plan_with_windows(64);
}

// the G2 side of the table builds and of the launch routines is instantiated in msm_g2.hip
extern template int build_comb<Fq2>(zkmi_ctx*, const Affine<Fq2>*, size_t, const WinPlan&, int,
                                    Affine<Fq2>*, int*, Affine<Fq2>*);
extern template int build_impl<Fq2>(zkmi_ctx*, const Affine<Fq2>*, size_t, const WinPlan&,
                                    Affine<Fq2>*);
extern template int run_impl<Fq2>(zkmi_ctx*, const zkmi_msm_bases*, const Fr*, const uint32_t*,
                                  size_t, size_t, XYZZ<Fq2>*, bool, XYZZ<Fq2>*, hipStream_t,
                                  const uint8_t*, bool);

// fn(F{}) with the coordinate field of the group: Fq for G1, Fq2 for G2
template <class Fn>
static auto by_group(int group, Fn&& fn) {
  return group == 1 ? fn(Fq{}) : fn(Fq2{});
}

int msm_bases_build(zkmi_ctx* ctx, int group, const void* bases_dev, size_t n, const WinPlan& plan,
                    zkmi_msm_bases** out, int image) {
  if (group != 1 && group != 2) {
    ctx->err = "group must be 1 (G1) or 2 (G2)";
    return ZKMI_ERR_ARG;
  }
  auto* b = new zkmi_msm_bases();
  b->group = group;
  b->n = n;
  b->plan = plan;
  b->image = image;
  const size_t entry = group == 1 ? sizeof(G1Affine) : sizeof(G2Affine);
  b->n_groups = plan.comb ? (n + plan.comb - 1) / plan.comb : 0;
  b->table_bytes = plan.comb ? b->n_groups * ((size_t)1 << (plan.comb - plan.comb_signed)) * entry
                             : n * (size_t)plan.per_base * entry;
  if (n == 0) {
    *out = b;
    return ZKMI_OK;
  }
  hipError_t e = hipMalloc(&b->table, b->table_bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    ctx->err = "hipMalloc of MSM window table failed (" + std::to_string(b->table_bytes) +
               " bytes): " + hipGetErrorString(e);
    delete b;
    return ZKMI_ERR_OOM;
  }
  if (hipMalloc(&b->inf, n) != hipSuccess) {
    (void)hipGetLastError();
    hipFree(b->table);
    delete b;
    return ZKMI_ERR_OOM;
  }
  const int rc = by_group(group, [&](auto f) {
    using F = decltype(f);
    const Affine<F>* bases = (const Affine<F>*)bases_dev;
    hipLaunchKernelGGL((msm_inf_flags<F>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       ctx->stream, bases, (uint32_t)n, b->inf);
    return plan.comb ? build_comb<F>(ctx, bases, n, plan, image, (Affine<F>*)b->table,
                                     &b->entries_may_be_inf, &stotal_of(b, f))
                     : build_impl<F>(ctx, bases, n, plan, (Affine<F>*)b->table);
  });
  if (rc) {
    hipFree(b->table);
    hipFree(b->inf);
    delete b;
    return rc;
  }
  *out = b;
  return ZKMI_OK;
}

int msm_horner_run(zkmi_ctx* ctx, hipStream_t stream, int count,
                   const zkmi_msm_bases* const* bases, void* const* wsums, void* const* outs,
                   size_t Bp) {
  if (count < 1 || count > 4) return ZKMI_ERR_ARG;
  const WinPlan& plan = bases[0]->plan;
  by_group(bases[0]->group, [&](auto f) {
    using F = decltype(f);
    if (plan.comb) {
      HornerArgsRW<F> hw{};
      for (int i = 0; i < count; i++) {
        hw.wsum[i] = (XYZZ<F>*)wsums[i];
        hw.out[i] = (XYZZ<F>*)outs[i];
        hw.stotal[i] = stotal_of(bases[i], f);
      }
      launch_comb_horner<F>(stream, hw, count, Bp, plan);
    } else {
      HornerArgs<F> ha{};
      for (int i = 0; i < count; i++) {
        ha.wsum[i] = (const XYZZ<F>*)wsums[i];
        ha.out[i] = (XYZZ<F>*)outs[i];
      }
      hipLaunchKernelGGL((msm_horner<F>), dim3((unsigned)(Bp / 64), (unsigned)count), dim3(64), 0,
                         stream, ha, Bp, plan);
    }
  });
  ZK_HIP(hipGetLastError());
  return ZKMI_OK;
}

int msm_run(zkmi_ctx* ctx, const zkmi_msm_bases* bases, const Fr* scalars, const uint32_t* row_idx,
            size_t Bp, size_t batch, void* out_xyzz, bool scalars_f, void* wsum_out,
            hipStream_t finish_stream, const uint8_t* row_varies, bool dense) {
  return by_group(bases->group, [&](auto f) -> int {
    using F = decltype(f);
    if (bases->n == 0) {
      // no bases: the result is the identity, and on the deferred path so is every window sum
      const bool sums = wsum_out && (bases->plan.shared || bases->plan.comb);
      const size_t cnt = sums ? (size_t)bases->plan.W * Bp : Bp;
      hipLaunchKernelGGL((fill_inf<F>), dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, ctx->stream,
                         (XYZZ<F>*)(sums ? wsum_out : out_xyzz), cnt);
      ZK_HIP(hipGetLastError());
      return ZKMI_OK;
    }
    if (batch == 0 || batch > Bp) {
      ctx->err = "msm: batch must be in [1, Bp]";
      return ZKMI_ERR_ARG;
    }
    return run_impl<F>(ctx, bases, scalars, row_idx, Bp, batch, (XYZZ<F>*)out_xyzz, scalars_f,
                       (XYZZ<F>*)wsum_out, finish_stream, row_varies, dense);
  });
}

int msm_rows_vary(zkmi_ctx* ctx, const Fr* rows, size_t n_rows, size_t Bp, size_t batch,
                  uint8_t* flags) {
  if (n_rows == 0) return ZKMI_OK;
  hipLaunchKernelGGL(rows_vary_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, ctx->stream,
                     rows, (const uint32_t*)nullptr, (uint32_t)n_rows, Bp, batch, flags);
  ZK_HIP(hipGetLastError());
  return ZKMI_OK;
}

int xyzz_to_affine(zkmi_ctx* ctx, int group, const void* in, void* out, size_t n) {
  if (n == 0) return ZKMI_OK;
  by_group(group, [&](auto f) {
    using F = decltype(f);
    hipLaunchKernelGGL((xyzz_to_affine_kernel<F>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0,
                       ctx->stream, (const XYZZ<F>*)in, (Affine<F>*)out, n);
  });
  ZK_HIP(hipGetLastError());
  return ZKMI_OK;
}

}  // namespace zk
