// Key-load half of the quotient in evaluation form (quotient_fold.h has the identity and the host
// plan): the change of basis that the prover used to apply to every batch's quotient, applied once
// to the key's bases instead.
//   1. E and L: two n-point DFTs over G1 with kernel w^-1 on the g1_z points, pre-scaled by
//      (den / n) g^-k and by 1 / n.  Radix 2, decimation in time on bit-reversed input; one lane
//      per butterfly (T = w Q by double-and-add, then P + T and P - T by mixed addition, both back
//      to affine), one launch per stage, E and L side by side in every launch.  A one-off of about
//      n log n scalar multiplications; nothing here is on the prove path.
//   2. D_w = sum_i (-den O_iw) L_i: one lane per term of O for the product, one lane per wire for
//      the sum over its column.
//   3. K'_j = K_j + D of its wire; wires that K does not hold arrive as infinity and leave as D.
// Infinity (Z_(n-1), empty sums) and P = +-T go through ec.h's own branches.
#include "zkmi_internal.h"
#include "quotient_fold.h"

namespace zk {

__device__ __forceinline__ uint32_t fold_bitrev(uint32_t x, int bits) {
  return __brev(x) >> (32 - bits);
}

// pts[which * n + bitrev(k)] = s_k * Z_k; which = 0: s_k = (den / n) g^-k (the plan's
// coset_inv_den), which = 1: s_k = 1 / n.  Z_k = infinity from n_z on.
__global__ __launch_bounds__(64) void qb_prescale_kernel(const G1Affine* __restrict__ z,
                                                         uint32_t n_z, G1Affine* __restrict__ pts,
                                                         int log_n,
                                                         const Fr* __restrict__ coset_inv_den,
                                                         Fr n_inv) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x, n = 1u << log_n;
  if (t >= 2 * n) return;
  const uint32_t which = t >> log_n, k = t & (n - 1);
  G1Affine r = G1Affine::inf();
  if (k < n_z) {
    const Fr s = from_mont(which ? n_inv : coset_inv_den[k]);
    r = to_affine(scalar_mul(z[k], s.v));
  }
  pts[(size_t)which * n + fold_bitrev(k, log_n)] = r;
}

// stage s of both transforms: butterfly t of a transform pairs i0 = (t >> s << (s + 1)) + j and
// i1 = i0 + 2^s, j = t mod 2^s, with the twiddle w^-(j n / 2^(s+1)); j = 0 needs no product
__global__ __launch_bounds__(64) void qb_stage_kernel(G1Affine* __restrict__ pts, int log_n, int s,
                                                      const Fr* __restrict__ tw_inv) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x, n = 1u << log_n, half = n >> 1;
  if (t >= n) return;
  const uint32_t which = t >= half ? 1u : 0u, bt = t - which * half;
  const uint32_t j = bt & ((1u << s) - 1u);
  const size_t i0 = (size_t)which * n + (((size_t)(bt >> s)) << (s + 1)) + j, i1 = i0 + (1u << s);
  const G1Affine p = pts[i0], q = pts[i1];
  G1XYZZ tp = G1XYZZ::from_affine(q);
  if (j) {
    const Fr w = from_mont(tw_inv[(size_t)j << (log_n - 1 - s)]);
    tp = scalar_mul(q, w.v);
  }
  G1XYZZ tm = tp;
  tm.y = neg(tm.y);
  madd(tp, p);
  madd(tm, p);
  pts[i0] = to_affine(tp);
  pts[i1] = to_affine(tm);
}

// prod[t] = scalars[t] * L[rows[t]]
__global__ __launch_bounds__(64) void fold_terms_kernel(const G1Affine* __restrict__ l_pts,
                                                        const uint32_t* __restrict__ rows,
                                                        const Fr* __restrict__ scalars,
                                                        uint32_t n_terms,
                                                        G1XYZZ* __restrict__ prod) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x;
  if (t >= n_terms) return;
  const Fr s = scalars[t];
  prod[t] = scalar_mul(l_pts[rows[t]], s.v);
}

// dcol[c] = sum of the products of column c
__global__ __launch_bounds__(64) void fold_cols_kernel(const G1XYZZ* __restrict__ prod,
                                                       const uint32_t* __restrict__ col_ptr,
                                                       uint32_t n_cols, G1XYZZ* __restrict__ dcol) {
  const uint32_t c = blockIdx.x * 64 + threadIdx.x;
  if (c >= n_cols) return;
  G1XYZZ acc = G1XYZZ::inf();
  for (uint32_t t = col_ptr[c]; t < col_ptr[c + 1]; t++) padd(acc, prod[t]);
  dcol[c] = acc;
}

// k[j] += dcol[col_of_base[j]] where there is a column
__global__ __launch_bounds__(64) void fold_k_kernel(G1Affine* __restrict__ k,
                                                    const int32_t* __restrict__ col_of_base,
                                                    uint32_t n_k, const G1XYZZ* __restrict__ dcol) {
  const uint32_t j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n_k) return;
  const int32_t c = col_of_base[j];
  if (c < 0) return;
  G1XYZZ acc = dcol[c];
  madd(acc, k[j]);
  k[j] = to_affine(acc);
}

static unsigned blocks64(size_t lanes) { return (unsigned)((lanes + 63) / 64); }

// device buffers of one fold, freed together
struct FoldScratch {
  std::vector<void*> p;
  ~FoldScratch() {
    for (void* x : p) hipFree(x);
  }
  template <class T>
  int get(zkmi_ctx* ctx, T** out, size_t count) {
    void* x = nullptr;
    ZK_HIP(hipMalloc(&x, (count ? count : 1) * sizeof(T)));
    p.push_back(x);
    *out = (T*)x;
    return ZKMI_OK;
  }
  template <class T>
  int put(zkmi_ctx* ctx, T** out, const std::vector<T>& host) {
    int rc = get(ctx, out, host.size());
    if (rc) return rc;
    if (!host.empty())
      ZK_HIP(hipMemcpy(*out, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return ZKMI_OK;
  }
};

int quotient_bases_dev(zkmi_ctx* ctx, const NttPlan* plan, const G1Affine* z_dev, uint32_t n_z,
                       G1Affine* pts) {
  const int lg = plan->log_n;
  const size_t n = (size_t)1 << lg;
  if (n_z > n - 1) n_z = (uint32_t)(n - 1);
  hipLaunchKernelGGL(qb_prescale_kernel, dim3(blocks64(2 * n)), dim3(64), 0, ctx->stream, z_dev, n_z,
                     pts, lg, plan->coset_inv_den, plan->n_inv);
  for (int s = 0; s < lg; s++)
    hipLaunchKernelGGL(qb_stage_kernel, dim3(blocks64(n)), dim3(64), 0, ctx->stream, pts, lg, s,
                       plan->tw_inv);
  ZK_HIP(hipGetLastError());
  return ZKMI_OK;
}

static bool fold_read(void* dst, const void* src, size_t bytes) {
  return bytes == 0 || (src && hipMemcpy(dst, src, bytes, hipMemcpyDefault) == hipSuccess);
}

int quotient_fold_key(zkmi_ctx* ctx, const zkmi_pk_desc* d, const std::vector<uint32_t>& k_wire,
                      FoldedKey* out) {
  const zkmi_r1cs_desc& f = *d->fold_r1cs;
  out->folded = false;
  // the description on the host, checked before anything reads it as an index
  if (f.n_constraints == 0 || f.n_wires == 0 || f.n_coeffs == 0 || f.n_coeffs >= (1u << 30) ||
      !f.coeffs || !f.o_ptr) {
    ctx->err = "pk: fold_r1cs: n_constraints, n_wires and n_coeffs (< 2^30) must be positive, "
               "coeffs and o_ptr given";
    return ZKMI_ERR_ARG;
  }
  std::vector<Fr> coeffs(f.n_coeffs);
  std::vector<uint32_t> o_ptr((size_t)f.n_constraints + 1);
  if (!fold_read(coeffs.data(), f.coeffs, coeffs.size() * sizeof(Fr)) ||
      !fold_read(o_ptr.data(), f.o_ptr, o_ptr.size() * 4)) {
    (void)hipGetLastError();
    ctx->err = "pk: fold_r1cs: cannot read the coefficient table or the row offsets of O";
    return ZKMI_ERR_ARG;
  }
  bool ok = o_ptr[0] == 0;
  for (uint32_t k = 0; ok && k < f.n_constraints; k++) ok = o_ptr[k] <= o_ptr[k + 1];
  std::vector<zkmi_term> terms(ok ? o_ptr[f.n_constraints] : 0);
  if (ok && !fold_read(terms.data(), f.o_terms, terms.size() * sizeof(zkmi_term))) {
    (void)hipGetLastError();
    ctx->err = "pk: fold_r1cs: cannot read the terms of O";
    return ZKMI_ERR_ARG;
  }
  FoldPlanIn in;
  in.n_wires = f.n_wires;
  in.n_constraints = f.n_constraints;
  in.n_coeffs = f.n_coeffs;
  in.coeffs = coeffs.data();
  in.o_ptr = o_ptr.data();
  in.o_terms = terms.data();
  in.den = fold_den((int)d->log_n);
  FoldPlan P;
  const std::string err = fold_plan_build(in, &P);
  if (!err.empty()) {
    ctx->err = err;
    return ZKMI_ERR_ARG;
  }
  // a system that does not fit the key leaves it as it is
  const size_t n = (size_t)1 << d->log_n;
  if (d->log_n < 8 || d->n_commitments || f.n_wires != d->n_wires || f.n_constraints > n)
    return ZKMI_OK;
  std::vector<int32_t> col_of_base;
  fold_k_merge(P, k_wire, d->n_wires, &out->k_wire, &col_of_base);
  const size_t n_k = out->k_wire.size(), n_terms = P.rows.size(), n_cols = P.wires.size();

  NttPlan* plan;
  int rc = get_plan(ctx, (int)d->log_n, &plan);
  if (rc) return rc;
  FoldScratch S;
  G1Affine *z, *pts, *k;
  G1XYZZ *prod, *dcol;
  uint32_t *rows, *col_ptr;
  int32_t* cols;
  Fr* scalars;
  if ((rc = S.get(ctx, &z, n - 1)) || (rc = S.get(ctx, &pts, 2 * n)) || (rc = S.get(ctx, &k, n_k)) ||
      (rc = S.get(ctx, &prod, n_terms)) || (rc = S.get(ctx, &dcol, n_cols)) ||
      (rc = S.put(ctx, &rows, P.rows)) || (rc = S.put(ctx, &col_ptr, P.col_ptr)) ||
      (rc = S.put(ctx, &cols, col_of_base)) || (rc = S.put(ctx, &scalars, P.scalars)))
    return rc;
  ZK_HIP(hipMemset(k, 0, (n_k ? n_k : 1) * sizeof(G1Affine)));   // the appended bases: infinity
  ZK_HIP(hipMemcpy(z, d->g1_z, (n - 1) * sizeof(G1Affine), hipMemcpyDefault));
  if (d->n_k) ZK_HIP(hipMemcpy(k, d->g1_k, (size_t)d->n_k * sizeof(G1Affine), hipMemcpyDefault));
  ZK_HIP(hipStreamSynchronize(nullptr));   // the kernels run on the context's own stream
  if ((rc = quotient_bases_dev(ctx, plan, z, (uint32_t)(n - 1), pts))) return rc;
  if (n_terms) {
    hipLaunchKernelGGL(fold_terms_kernel, dim3(blocks64(n_terms)), dim3(64), 0, ctx->stream, pts + n,
                       rows, scalars, (uint32_t)n_terms, prod);
    hipLaunchKernelGGL(fold_cols_kernel, dim3(blocks64(n_cols)), dim3(64), 0, ctx->stream, prod,
                       col_ptr, (uint32_t)n_cols, dcol);
    hipLaunchKernelGGL(fold_k_kernel, dim3(blocks64(n_k)), dim3(64), 0, ctx->stream, k, cols,
                       (uint32_t)n_k, dcol);
  }
  ZK_HIP(hipGetLastError());
  out->e.resize(n);
  out->k.resize(n_k);
  ZK_HIP(hipMemcpyAsync(out->e.data(), pts, n * sizeof(G1Affine), hipMemcpyDeviceToHost,
                        ctx->stream));
  if (n_k)
    ZK_HIP(hipMemcpyAsync(out->k.data(), k, n_k * sizeof(G1Affine), hipMemcpyDeviceToHost,
                          ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  out->folded = true;
  return ZKMI_OK;
}

}  // namespace zk

extern "C" int zkmi_quotient_bases(zkmi_ctx* ctx, const void* g1_z, size_t n_z, int log_n,
                                   void* e_out, void* l_out) {
  using namespace zk;
  ZK_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = require_idle(ctx))) return rc;
  if (log_n < 1 || log_n > 28 || !g1_z || !e_out || !l_out || n_z + 1 < ((size_t)1 << log_n)) {
    ctx->err = "quotient_bases: log_n in [1,28], n_z >= 2^log_n - 1, no null array";
    return ZKMI_ERR_ARG;
  }
  NttPlan* plan;
  if ((rc = get_plan(ctx, log_n, &plan))) return rc;
  const size_t n = (size_t)1 << log_n;
  FoldScratch S;
  G1Affine *z, *pts;
  if ((rc = S.get(ctx, &z, n - 1)) || (rc = S.get(ctx, &pts, 2 * n))) return rc;
  ZK_HIP(hipMemcpy(z, g1_z, (n - 1) * sizeof(G1Affine), hipMemcpyDefault));
  ZK_HIP(hipStreamSynchronize(nullptr));   // the kernels run on the context's own stream
  if ((rc = quotient_bases_dev(ctx, plan, z, (uint32_t)(n - 1), pts))) return rc;
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  ZK_HIP(hipMemcpy(e_out, pts, n * sizeof(G1Affine), hipMemcpyDefault));
  ZK_HIP(hipMemcpy(l_out, pts + n, n * sizeof(G1Affine), hipMemcpyDefault));
  return ZKMI_OK;
}
