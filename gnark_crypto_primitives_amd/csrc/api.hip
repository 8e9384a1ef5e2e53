// C-ABI of libzkmi.so (include/zkmi.h) and the Groth16 prove pipeline that strings the kernels
// together: solve -> quotient -> 4 G1 MSMs + 1 G2 MSM -> assembly.  The quotient is six transforms
// (compute_h_bi; gnark's seven below 2^8), or the four that take a and b to the coset when the key
// was loaded with its quotient bases in evaluation form (compute_ab_coset_bi, quotient_fold.hip).
// Stands in for groth16.Prove in gnark backend/groth16/bn254/prove.go [UPSTREAM-RECALL,
// SURVEY.md §3.2].  There is no CPU fallback anywhere in this file.
#include <algorithm>

#include "zkmi_internal.h"
#include "comb_plan.h"
#include "ff29.h"
#include "ec29.h"

using namespace zk;

namespace zk {

void sync_side_streams(zkmi_ctx* ctx) {
  for (hipStream_t q : {ctx->stream2, ctx->stream3, ctx->stream4})
    if (q) hipStreamSynchronize(q);
}

int ensure_scratch(zkmi_ctx* ctx, DevBuf& s, size_t bytes, void** out) {
  if (s.bytes < bytes) {
    if (s.p) {
      // nothing queued on any of the context's streams may still use the old buffer
      hipStreamSynchronize(ctx->stream);
      sync_side_streams(ctx);
      hipFree(s.p);
      s.p = nullptr;
      s.bytes = 0;
    }
    hipError_t e = hipMalloc(&s.p, bytes);
    if (e != hipSuccess) {
      ctx->err = "hipMalloc(" + std::to_string(bytes) + " B) failed: " + hipGetErrorString(e) +
                 " (the working set of this batch does not fit beside the MSM tables: load the key"
                 " with zkmi_pk_desc.max_batch >= the batch size, or with a table_budget_bytes cap)";
      s.p = nullptr;
      return ZKMI_ERR_OOM;
    }
    s.bytes = bytes;
  }
  if (out) *out = s.p;
  return ZKMI_OK;
}

// Guard of every entry point that is not part of the Groth16 pipeline.  With no batch in flight,
// nothing on any stream uses set 0's buffers, so after this check those entry points may borrow
// them (value file, a, b, c, misc) as their own scratch.
int require_idle(zkmi_ctx* ctx) {
  if (!ctx->sets[0].pending && !ctx->sets[1].pending) return ZKMI_OK;
  ctx->err = "a submitted prove batch is in flight; collect it first";
  return ZKMI_ERR_ARG;
}

// ---- elementwise field kernels --------------------------------------------------------------------
template <class P>
__global__ __launch_bounds__(256) void field_mul_kernel(const Fp<P>* a, const Fp<P>* b, Fp<P>* r,
                                                        size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) r[i] = mul(a[i], b[i]);
}

// `iters` dependent products per lane, two independent chains to expose ILP
template <class P>
__global__ __launch_bounds__(256) void field_mul_bench_kernel(Fp<P>* io, int iters) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  Fp<P> x = io[i], y = io[i];
  y.v[0] ^= 1;
  for (int k = 0; k < iters; k++) {
    x = mul(x, y);
    y = mul(y, x);
  }
  io[i] = add(x, y);
}

// the same measurement for the 9 x 29-bit representation used inside the G1 MSM (ff29.h)
__global__ __launch_bounds__(256) void field_mul_bench_f29_kernel(Fq* io, int iters) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  Fq29 x = unpack29<Fq29Params>(io[i].v), y = x;
  y.v[0] ^= 1;
  for (int k = 0; k < iters; k++) {
    x = mul(x, y);
    y = mul(y, x);
  }
  pack_canonical<Fq29Params>(io[i].v, norm(add(x, y)));
}

// ---- parity hook for the 9 x 29-bit forms (zkmi_ff29_op) ------------------------------------------
// One lane per element, one wavefront per block.  The form is applied to the raw limbs as they are
// in memory: nothing is unpacked or normalised, so operands at the edges of a form's contract reach
// it unchanged.  Ops 0..3 are the asm chains of ff29_asm.h, 4..7 the C++ forms of ff29.h compiled
// for the device, 8 and 9 pack_canonical with and without wred (8 words out, the ninth zero).
enum { FF29_MUL_ASM, FF29_SQR_ASM, FF29_MUL_ADD2_ASM, FF29_MUL_ASM_S, FF29_MUL, FF29_SQR,
       FF29_MUL_ADD2, FF29_MUL_ILP, FF29_WRED_PACK, FF29_PACK, FF29_N_OPS };
static constexpr int ff29_arity(int op) {
  if (op == FF29_MUL_ADD2_ASM || op == FF29_MUL_ADD2) return 4;
  if (op == FF29_SQR_ASM || op == FF29_SQR || op == FF29_WRED_PACK || op == FF29_PACK) return 1;
  return 2;
}
template <class P>
__device__ __forceinline__ F29<P> ld_raw29(const int32_t* p) {
  F29<P> r;
#pragma unroll
  for (int l = 0; l < 9; l++) r.v[l] = p[l];
  return r;
}
template <class P, int OP>
__global__ __launch_bounds__(64) void ff29_op_kernel(const int32_t* __restrict__ in,
                                                     int32_t* __restrict__ out, size_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int AR = ff29_arity(OP);
  for (size_t w = blockIdx.x; w * 64 < n; w += gridDim.x) {
    // mul_asm_s: the b operand of the wave's first element, at an address that depends on the block
    // index alone, so that (as ntt.hip's ldc29 twiddles) it reaches the asm in SGPRs
    F29<P> bs = F29<P>::zero();
    if constexpr (OP == FF29_MUL_ASM_S) bs = ld_raw29<P>(in + w * 64 * (AR * 9) + 9);
    const size_t i = w * 64 + threadIdx.x;
    if (i >= n) continue;
    const int32_t* e = in + i * (AR * 9);
    const F29<P> a = ld_raw29<P>(e);
    F29<P> r = F29<P>::zero();
    if constexpr (OP == FF29_MUL_ASM) r = mul_asm(a, ld_raw29<P>(e + 9));
    if constexpr (OP == FF29_SQR_ASM) r = sqr_asm(a);
    if constexpr (OP == FF29_MUL_ADD2_ASM)
      r = mul_add2_asm(a, ld_raw29<P>(e + 9), ld_raw29<P>(e + 18), ld_raw29<P>(e + 27));
    if constexpr (OP == FF29_MUL_ASM_S) r = mul_asm_s(a, bs);
    if constexpr (OP == FF29_MUL) r = mul(a, ld_raw29<P>(e + 9));
    if constexpr (OP == FF29_SQR) r = sqr(a);
    if constexpr (OP == FF29_MUL_ADD2)
      r = mul_add2(a, ld_raw29<P>(e + 9), ld_raw29<P>(e + 18), ld_raw29<P>(e + 27));
    if constexpr (OP == FF29_MUL_ILP) r = mul_ilp(a, ld_raw29<P>(e + 9));
    if constexpr (OP == FF29_WRED_PACK || OP == FF29_PACK) {
      uint32_t img[8];
      pack_canonical<P>(img, OP == FF29_WRED_PACK ? wred(a) : a);
#pragma unroll
      for (int l = 0; l < 8; l++) r.v[l] = (int32_t)img[l];
      r.v[8] = 0;
    }
#pragma unroll
    for (int l = 0; l < 9; l++) out[i * 9 + l] = r.v[l];
  }
#endif
}
typedef void (*ff29_kernel_t)(const int32_t*, int32_t*, size_t);
template <class P, int OP = 0>
static ff29_kernel_t ff29_kernel(int op) {
  if constexpr (OP < FF29_N_OPS)
    return op == OP ? ff29_op_kernel<P, OP> : ff29_kernel<P, OP + 1>(op);
  else
    return nullptr;
}

// ---- proof assembly ---------------------------------------------------------------------------------
// Ar = sumA + alpha + r*delta ; Bs1 = sumB1 + beta + s*delta ; Bs = sumB2 + beta2 + s*delta2 ;
// Krs = sumK + sumZ - rs*delta + s*Ar + r*Bs1.
// The multiples of the fixed points delta / delta2 come from one-base window tables through the
// MSM kernel itself (26-32 mixed additions instead of a 254-step double-and-add); only
// s*Ar + r*Bs1 has per-proof bases and is done here with a joint double-and-add.
struct PkConsts {
  G1Affine alpha, beta1;
  G2Affine beta2;
};
struct ProofOut {
  G1Affine ar, krs;
  G2Affine bs;
};

// rs rows: [0] r, [1] s (inputs) -> [2] = -r*s
__global__ __launch_bounds__(64) void rs_prep_kernel(Fr* rs, size_t Bp) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bp) return;
  bi_st(rs, 2, i, Bp, neg(mul(bi_ld(rs, 0, i, Bp), bi_ld(rs, 1, i, Bp))));
}

// 2 * acc on the 29-bit lazy representation (dbl-2008-s-1; same bounds as ec29.h's mdbl29 with the
// accumulator's own x (|x| < 5p) and y (|y| < 2p) in the place of the affine point: every product
// stays below 25 p^2).  G1 has odd order: y != 0 for every finite point.
__device__ __forceinline__ void dbl29(G1Acc29& acc) {
  if (acc.inf) return;
  const Fq29 u = norm(add(acc.y, acc.y));
  const Fq29 v = msqr(u);
  const Fq29 w = mmul(u, v);
  const Fq29 s = mmul(acc.x, v);
  const Fq29 x2 = msqr(acc.x);
  const Fq29 m = norm(add(add(x2, x2), x2));
  const Fq29 x3 = norm(sub(msqr(m), add(s, s)));       // (-3.5p, 2.5p)
  const Fq29 y3 = norm(sub(mmul(m, sub(s, x3)), mmul(w, acc.y)));   // (-2p, 2p)
  acc.zz = mmul(v, acc.zz);
  acc.zzz = mmul(w, acc.zzz);
  acc.x = x3;
  acc.y = y3;
}

__global__ __launch_bounds__(64) void assemble_kernel(const G1XYZZ* sA, const G1XYZZ* sB1,
                                                      const G1XYZZ* sK, const G1XYZZ* sZ,
                                                      const G1XYZZ* tR, const G1XYZZ* tS,
                                                      const G1XYZZ* tNRS, const Fr* rs, size_t Bp,
                                                      PkConsts pk, ProofOut* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bp) return;
  const Fr r = from_mont(bi_ld(rs, 0, i, Bp)), s = from_mont(bi_ld(rs, 1, i, Bp));
  G1XYZZ AR = sA[i];
  madd(AR, pk.alpha);
  padd(AR, tR[i]);
  const G1Affine ar = to_affine(AR);
  G1XYZZ BS1 = sB1[i];
  madd(BS1, pk.beta1);
  padd(BS1, tS[i]);
  const G1Affine bs1 = to_affine(BS1);
  // s*ar + r*bs1, one shared doubling chain, on the 29-bit representation of the MSM inner loop
  // (a 16-wavefront latency chain: what counts is the instruction count per bit, 19 products of
  // ~230 instructions instead of 17 of ~550 on ff.h)
  const bool ar_fin = !ar.is_inf(), bs_fin = !bs1.is_inf();
  const Fq29 ax = from_std<Fq29Params>(ar.x), ay = from_std<Fq29Params>(ar.y);
  const Fq29 bx = from_std<Fq29Params>(bs1.x), by = from_std<Fq29Params>(bs1.y);
  G1Acc29 acc29 = G1Acc29::infinity();
  for (int w = 7; w >= 0; w--) {
    const uint32_t sw = s.v[w], rw = r.v[w];
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      dbl29(acc29);
      if (((sw >> b) & 1u) && ar_fin) madd29(acc29, ax, ay);
      if (((rw >> b) & 1u) && bs_fin) madd29(acc29, bx, by);
    }
  }
  G1XYZZ acc = to_std(acc29);
  padd(acc, sK[i]);
  padd(acc, sZ[i]);
  padd(acc, tNRS[i]);
  out[i].ar = ar;
  out[i].krs = to_affine(acc);
}

__global__ __launch_bounds__(64) void assemble_g2_kernel(const G2XYZZ* sB2, const G2XYZZ* tS2,
                                                         size_t Bp, G2Affine beta2, ProofOut* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Bp) return;
  G2XYZZ BS = sB2[i];
  madd(BS, beta2);
  padd(BS, tS2[i]);
  out[i].bs = to_affine(BS);
}

// ---- HBM working set of a pipeline set (zkmi_ctx::ProveSet) -------------------------------------
// Byte counts used both by the allocation (prove_set_begin) and by the planner
// (prove_working_set_bytes).  The sums buffer:
struct SumsView {
  G1XYZZ *sA, *sB1, *sK, *sZ, *tR, *tS, *tNRS;
  G2XYZZ *sB2, *tS2;
  ProofOut* proofs;
  G1XYZZ* w1[4];   // deferred window sums of A, B1, K, Z ([<= 256][Bp] each)
  G2XYZZ* w2;
  SumsView(void* base, size_t Bp) {
    char* m = (char*)base;
    sA = (G1XYZZ*)m;   m += Bp * 128;
    sB1 = (G1XYZZ*)m;  m += Bp * 128;
    sK = (G1XYZZ*)m;   m += Bp * 128;
    sZ = (G1XYZZ*)m;   m += Bp * 128;
    tR = (G1XYZZ*)m;   m += Bp * 128;
    tS = (G1XYZZ*)m;   m += Bp * 128;
    tNRS = (G1XYZZ*)m; m += Bp * 128;
    sB2 = (G2XYZZ*)m;  m += Bp * 256;
    tS2 = (G2XYZZ*)m;  m += Bp * 256;
    proofs = (ProofOut*)m;  m += Bp * 256;
    for (int i = 0; i < 4; i++) {
      w1[i] = (G1XYZZ*)m;
      m += 256 * Bp * 128;
    }
    w2 = (G2XYZZ*)m;
  }
};
static size_t sums_bytes(size_t Bp) { return Bp * (7 * 128 + 2 * 256 + 256 + 256 * (4 * 128 + 256)); }

// the other buffers of a pipeline set: value file of `value_rows`, a, b, c over the domain of n,
// misc = r/s (Bp x 96) + status (Bp x 4) + the staging area of `n_staged` input rows and r/s
struct SetBytes {
  size_t slots, abc, misc;
};
static SetBytes prove_set_bytes(size_t value_rows, size_t n, size_t n_staged, size_t batch, size_t Bp) {
  return {value_rows * Bp * 32, n * Bp * 32, Bp * (96 + 4) + batch * (n_staged * 32 + 64)};
}

int device_view(zkmi_ctx* ctx, const void* src, size_t bytes, void* stage, const void** out) {
  *out = src;
  if (pointer_kind(src) == PTR_DEVICE) return ZKMI_OK;
  ZK_HIP(hipMemcpyAsync(stage, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  *out = stage;
  return ZKMI_OK;
}

int prove_set_begin(zkmi_ctx* ctx, const zkmi_pk* pk, size_t value_rows, size_t n_staged,
                    size_t batch, const void* rs, hipStream_t* main, char** stage) {
  zkmi_ctx::ProveSet& S = ctx->sets[ctx->next_submit];
  if (S.pending) {
    ctx->err = "prove: two batches already in flight; collect one first";
    return ZKMI_ERR_ARG;
  }
  const size_t Bp = round_up(batch, 64);
  const SetBytes sb = prove_set_bytes(value_rows, (size_t)1 << pk->log_n, n_staged, batch, Bp);
  // Size the other set too, so that steady-state submits never allocate -- but only while that
  // set is idle: a pending set keeps raw pointers into its buffers (S.rs, S.commit_pts, ...), and
  // its solve / quotient / MSM kernels may be running on them.  A pending set is resized by its
  // own next submit, after its collect.
  int rc;
  for (zkmi_ctx::ProveSet* T : {&ctx->sets[ctx->next_submit ^ 1], &S}) {
    if (T->pending) continue;
    if ((rc = ensure_scratch(ctx, T->slots, sb.slots)) || (rc = ensure_scratch(ctx, T->a, sb.abc)) ||
        (rc = ensure_scratch(ctx, T->b, sb.abc)) || (rc = ensure_scratch(ctx, T->c, sb.abc)) ||
        (rc = ensure_scratch(ctx, T->misc, sb.misc)) ||
        (rc = ensure_scratch(ctx, T->sums, sums_bytes(Bp))))
      return rc;
  }
  char* const staged = (char*)S.misc.p + Bp * 100;
  S.rs = S.misc.p;
  S.st = (char*)S.misc.p + Bp * 96;
  if (stage) *stage = staged;
  S.heavy_enqueued = false;
  S.batch = batch;
  S.Bp = Bp;
  S.pk = pk;
  *main = ctx->stream;
  ctx->stream = ctx->stream2;   // the helpers launch on ctx->stream
  hipEventRecord(S.ev0, ctx->stream);
  const void* rs_dev;
  rc = device_view(ctx, rs, batch * 64, staged + batch * n_staged * 32, &rs_dev);
  if (!rc) rc = transpose_in(ctx, rs_dev, S.rs, 2, batch, Bp, 32);
  return rc ? prove_set_end(ctx, *main, rc) : ZKMI_OK;
}

int prove_set_end(zkmi_ctx* ctx, hipStream_t main, int rc) {
  zkmi_ctx::ProveSet& S = ctx->sets[ctx->next_submit];
  hipEventRecord(S.ev1, ctx->stream);
  ctx->stream = main;
  if (rc) {
    sync_side_streams(ctx);   // nothing of a failed submit stays queued on caller memory
    return rc;
  }
  S.pending = true;
  ctx->next_submit ^= 1;
  return ZKMI_OK;
}

}  // namespace zk

// ===================================================================================================
extern "C" {

int zkmi_init(int device, zkmi_ctx** out) {
  if (!out) return ZKMI_ERR_ARG;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return ZKMI_ERR_NO_DEVICE;
  if (device < 0 || device >= count) return ZKMI_ERR_ARG;
  if (hipSetDevice(device) != hipSuccess) return ZKMI_ERR_HIP;
  auto* ctx = new zkmi_ctx();
  ctx->device = device;
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return ZKMI_ERR_HIP;
  }
  if (hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking) != hipSuccess) {
    hipStreamDestroy(ctx->stream);
    delete ctx;
    return ZKMI_ERR_HIP;
  }
  if (hipStreamCreateWithFlags(&ctx->stream3, hipStreamNonBlocking) != hipSuccess) {
    hipStreamDestroy(ctx->stream2);
    hipStreamDestroy(ctx->stream);
    delete ctx;
    return ZKMI_ERR_HIP;
  }
  if (hipStreamCreateWithFlags(&ctx->stream4, hipStreamNonBlocking) != hipSuccess) {
    hipStreamDestroy(ctx->stream3);
    hipStreamDestroy(ctx->stream2);
    hipStreamDestroy(ctx->stream);
    delete ctx;
    return ZKMI_ERR_HIP;
  }
  for (auto& st : ctx->sets) {
    hipEventCreate(&st.ev0);
    hipEventCreate(&st.ev1);
    for (auto& e : st.evq) hipEventCreate(&e);
    for (auto& e : st.eva) hipEventCreate(&e);
    hipEventCreateWithFlags(&st.tail_ev, hipEventDisableTiming);
    for (auto& p : st.msm_ev) {
      hipEventCreate(&p[0]);
      hipEventCreate(&p[1]);
    }
  }
  for (auto& e : ctx->ev) hipEventCreate(&e);
  for (auto& e : ctx->part_ev) hipEventCreateWithFlags(&e, hipEventDisableTiming);
  for (auto& e : ctx->acc_ev) hipEventCreateWithFlags(&e, hipEventDisableTiming);
  for (auto& e : ctx->dig_ev) hipEventCreateWithFlags(&e, hipEventDisableTiming);
  ctx->plans.reserve(32);
  *out = ctx;
  return ZKMI_OK;
}

void zkmi_destroy(zkmi_ctx* ctx) {
  if (!ctx) return;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  sync_side_streams(ctx);
  for (auto& st : ctx->sets) {
    if (st.ev0) hipEventDestroy(st.ev0);
    if (st.ev1) hipEventDestroy(st.ev1);
    for (auto& e : st.evq)
      if (e) hipEventDestroy(e);
    for (auto& e : st.eva)
      if (e) hipEventDestroy(e);
    if (st.tail_ev) hipEventDestroy(st.tail_ev);
    for (auto& p : st.msm_ev) {
      if (p[0]) hipEventDestroy(p[0]);
      if (p[1]) hipEventDestroy(p[1]);
    }
  }
  hipStreamDestroy(ctx->stream2);
  hipStreamDestroy(ctx->stream3);
  hipStreamDestroy(ctx->stream4);
  for (auto& p : ctx->plans) free_plan(p);
  for (auto& st : ctx->sets)
    for (DevBuf* b : {&st.slots, &st.a, &st.b, &st.c, &st.misc, &st.sums, &st.commit})
      if (b->p) hipFree(b->p);
  for (DevBuf* b : {&ctx->ntt_tmp, &ctx->ntt_top, &ctx->build_tmp, &ctx->msm_digits, &ctx->msm_sint,
                    &ctx->msm_rowvar, &ctx->msm_part[0], &ctx->msm_part[1], &ctx->side_part2, &ctx->side_part3})
    if (b->p) hipFree(b->p);
  witness_ring_free(ctx);
  for (auto& e : ctx->ev)
    if (e) hipEventDestroy(e);
  for (auto& e : ctx->part_ev)
    if (e) hipEventDestroy(e);
  for (auto& e : ctx->acc_ev)
    if (e) hipEventDestroy(e);
  for (auto& e : ctx->dig_ev)
    if (e) hipEventDestroy(e);
  hipStreamDestroy(ctx->stream);
  delete ctx;
}

const char* zkmi_last_error(zkmi_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int zkmi_sync(zkmi_ctx* ctx) {
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}

void* zkmi_stream(zkmi_ctx* ctx) { return (void*)ctx->stream; }

int zkmi_field_mul(zkmi_ctx* ctx, int which, const void* a, const void* b, void* r, size_t n) {
  ZK_HIP(hipSetDevice(ctx->device));
  Staged sa(ctx), sb(ctx), sr(ctx);
  int rc;
  if ((rc = sa.in(a, n * 32)) || (rc = sb.in(b, n * 32)) || (rc = sr.out(r, n * 32))) return rc;
  if (n == 0) return ZKMI_OK;
  unsigned g = (unsigned)((n + 255) / 256);
  if (g > 8192) g = 8192;
  if (which == 0)
    hipLaunchKernelGGL((field_mul_kernel<FrParams>), dim3(g), dim3(256), 0, ctx->stream,
                       (const Fr*)sa.dev, (const Fr*)sb.dev, (Fr*)sr.dev, n);
  else
    hipLaunchKernelGGL((field_mul_kernel<FqParams>), dim3(g), dim3(256), 0, ctx->stream,
                       (const Fq*)sa.dev, (const Fq*)sb.dev, (Fq*)sr.dev, n);
  ZK_HIP(hipGetLastError());
  if ((rc = sr.finish())) return rc;
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}

int zkmi_ff29_op(zkmi_ctx* ctx, int field, int op, const int32_t* in, int32_t* out, size_t n) {
  ZK_HIP(hipSetDevice(ctx->device));
  const ff29_kernel_t k = field == 0   ? ff29_kernel<Fr29Params>(op)
                          : field == 1 ? ff29_kernel<Fq29Params>(op)
                                       : nullptr;
  if (!k) {
    ctx->err = "ff29_op: field must be 0 (fr) or 1 (fq), op in [0, 9]";
    return ZKMI_ERR_ARG;
  }
  if (n == 0) return ZKMI_OK;
  Staged si(ctx), so(ctx);
  int rc;
  if ((rc = si.in(in, n * ff29_arity(op) * 36)) || (rc = so.out(out, n * 36))) return rc;
  const size_t waves = (n + 63) / 64;
  hipLaunchKernelGGL(k, dim3((unsigned)std::min(waves, (size_t)65536)), dim3(64), 0, ctx->stream,
                     (const int32_t*)si.dev, (int32_t*)so.dev, n);
  ZK_HIP(hipGetLastError());
  if ((rc = so.finish())) return rc;
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}

int zkmi_field_mul_bench(zkmi_ctx* ctx, int which, size_t n_threads, int iters, double* rate) {
  ZK_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = require_idle(ctx))) return rc;
  n_threads = round_up(n_threads, 256);
  void* buf;
  if ((rc = ensure_scratch(ctx, ctx->sets[0].misc, n_threads * 32, &buf))) return rc;
  // every byte 0x11: top limb 0x11111111 < 0x30644e72, so the element is < p
  ZK_HIP(hipMemsetAsync(buf, 0x11, n_threads * 32, ctx->stream));
  auto launch = [&]() {
    if (which == 0)
      hipLaunchKernelGGL((field_mul_bench_kernel<FrParams>), dim3((unsigned)(n_threads / 256)),
                         dim3(256), 0, ctx->stream, (Fr*)buf, iters);
    else if (which == 2)
      hipLaunchKernelGGL(field_mul_bench_f29_kernel, dim3((unsigned)(n_threads / 256)), dim3(256),
                         0, ctx->stream, (Fq*)buf, iters);
    else
      hipLaunchKernelGGL((field_mul_bench_kernel<FqParams>), dim3((unsigned)(n_threads / 256)),
                         dim3(256), 0, ctx->stream, (Fq*)buf, iters);
  };
  launch();  // warm-up
  ZK_HIP(hipEventRecord(ctx->ev[6], ctx->stream));
  launch();
  ZK_HIP(hipEventRecord(ctx->ev[7], ctx->stream));
  ZK_HIP(hipEventSynchronize(ctx->ev[7]));
  float ms = 0;
  ZK_HIP(hipEventElapsedTime(&ms, ctx->ev[6], ctx->ev[7]));
  *rate = (double)n_threads * iters * 2.0 / (ms * 1e-3);
  return ZKMI_OK;
}

int zkmi_ntt_batch(zkmi_ctx* ctx, void* data, int log_n, size_t batch, int inverse, int coset) {
  ZK_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = require_idle(ctx))) return rc;
  if (batch == 0) return ZKMI_OK;
  NttPlan* plan;
  if ((rc = get_plan(ctx, log_n, &plan))) return rc;
  const size_t n = (size_t)1 << log_n, Bp = round_up(batch, 64);
  Staged sd(ctx), so(ctx);
  if ((rc = sd.in(data, batch * n * 32)) || (rc = so.out(data, batch * n * 32))) return rc;
  void *t0, *t1;
  if ((rc = ensure_scratch(ctx, ctx->sets[0].a, n * Bp * 32, &t0)) ||
      (rc = ensure_scratch(ctx, ctx->sets[0].b, n * Bp * 32, &t1)))
    return rc;
  if ((rc = transpose_in(ctx, sd.dev, t0, n, batch, Bp, 32))) return rc;
  if ((rc = ntt_bi(ctx, plan, (const Fr*)t0, (Fr*)t1, Bp, inverse != 0, coset != 0, n))) return rc;
  if ((rc = transpose_out(ctx, t1, so.dev, n, batch, Bp, 32))) return rc;
  if ((rc = so.finish())) return rc;
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}

int zkmi_h_batch(zkmi_ctx* ctx, const void* a, const void* b, const void* c, void* h_out,
                 int log_n, size_t batch) {
  ZK_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = require_idle(ctx))) return rc;
  if (batch == 0) return ZKMI_OK;
  NttPlan* plan;
  if ((rc = get_plan(ctx, log_n, &plan))) return rc;
  const size_t n = (size_t)1 << log_n, Bp = round_up(batch, 64);
  Staged sa(ctx), sb(ctx), sc(ctx), sh(ctx);
  if ((rc = sa.in(a, batch * n * 32)) || (rc = sb.in(b, batch * n * 32)) ||
      (rc = sc.in(c, batch * n * 32)) || (rc = sh.out(h_out, batch * n * 32)))
    return rc;
  void* t[4];
  DevBuf* tb[4] = {&ctx->sets[0].a, &ctx->sets[0].b, &ctx->sets[0].c, &ctx->ntt_tmp};
  for (int i = 0; i < 4; i++)
    if ((rc = ensure_scratch(ctx, *tb[i], n * Bp * 32, &t[i]))) return rc;
  if ((rc = transpose_in(ctx, sa.dev, t[0], n, batch, Bp, 32)) ||
      (rc = transpose_in(ctx, sb.dev, t[1], n, batch, Bp, 32)) ||
      (rc = transpose_in(ctx, sc.dev, t[2], n, batch, Bp, 32)))
    return rc;
  Fr* h;
  if ((rc = compute_h_bi(ctx, plan, (Fr*)t[0], (Fr*)t[1], (Fr*)t[2], (Fr*)t[3], Bp, n, &h)))
    return rc;
  if ((rc = transpose_out(ctx, h, sh.dev, n, batch, Bp, 32))) return rc;
  if ((rc = sh.finish())) return rc;
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}

int zkmi_ab_coset_batch(zkmi_ctx* ctx, const void* a, const void* b, void* out, int log_n,
                        size_t batch) {
  ZK_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = require_idle(ctx))) return rc;
  if (batch == 0) return ZKMI_OK;
  NttPlan* plan;
  if ((rc = get_plan(ctx, log_n, &plan))) return rc;
  const size_t n = (size_t)1 << log_n, Bp = round_up(batch, 64);
  Staged sa(ctx), sb(ctx), so(ctx);
  if ((rc = sa.in(a, batch * n * 32)) || (rc = sb.in(b, batch * n * 32)) ||
      (rc = so.out(out, batch * n * 32)))
    return rc;
  void* t[3];
  DevBuf* tb[3] = {&ctx->sets[0].a, &ctx->sets[0].b, &ctx->ntt_tmp};
  for (int i = 0; i < 3; i++)
    if ((rc = ensure_scratch(ctx, *tb[i], n * Bp * 32, &t[i]))) return rc;
  if ((rc = transpose_in(ctx, sa.dev, t[0], n, batch, Bp, 32)) ||
      (rc = transpose_in(ctx, sb.dev, t[1], n, batch, Bp, 32)))
    return rc;
  Fr* u;
  if ((rc = compute_ab_coset_bi(ctx, plan, (Fr*)t[0], (Fr*)t[1], (Fr*)t[2], Bp, n, &u))) return rc;
  if ((rc = transpose_out(ctx, u, so.dev, n, batch, Bp, 32))) return rc;
  if ((rc = so.finish())) return rc;
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}

// window_bits: 0 = as many bits per window as the table budget allows (windows of mixed width
// summing to exactly 255 bits); 2..16 = uniform windows of that width.  If the table cannot be
// allocated the plan is relaxed (more, narrower windows) until it fits.
static int bases_load_plan(zkmi_ctx* ctx, int group, const void* bases_dev, size_t n, WinPlan plan,
                           bool may_relax, zkmi_msm_bases** out, int image = MSM_IMAGE_STD) {
  for (;;) {
    int rc = msm_bases_build(ctx, group, bases_dev, n, plan, out, image);
    if (rc != ZKMI_ERR_OOM || !may_relax) return rc;
    if (plan.comb) {
      if (plan.comb <= 8) return rc;
      plan = plan_comb(plan.comb - 1, plan.comb_signed != 0);
    } else if (plan.shared) {
      if (plan.bits[0] <= 4) return rc;
      plan = plan_shared(plan.bits[0] - 1);
    } else {
      if (plan.W >= 64) return rc;
      plan = plan_with_windows(plan.W + 1);
    }
  }
}

// explicit window_bits of the C-ABI: 2..16 = per-window tables, uniform width; 100 + c = one
// shared table of c-bit signed digits per base (c in 4..16)
// 200 + k = comb tables over groups of k bases (k in 2..20); 300 + k = sign-pattern comb tables
// (k in 3..21: 2^(k-1) entries per group, the auto plan's choice)
static bool window_bits_ok(int wb) {
  return wb == 0 || (wb >= 2 && wb <= 16) || (wb >= 104 && wb <= 116) ||
         (wb >= 202 && wb <= 220) || (wb >= 303 && wb <= 321);
}
static WinPlan plan_explicit(int wb) {
  return wb >= 300   ? plan_comb(wb - 300, true)
         : wb >= 200 ? plan_comb(wb - 200, false)
         : wb >= 100 ? plan_shared(wb - 100)
                     : plan_uniform(wb);
}
// HBM the prover needs beside the tables to prove batches of up to `max_batch` with a key of this
// shape: two pipeline sets (value file, a, b, c, staged inputs, sums, commitment
// buffers), the NTT scratch, the MSM integer scalars + digits + two partial-sum buffers (with what
// the MSM tails read beside the sums: lane-0 digits and the list of the uniform groups), the
// table-build scratch that stays allocated, and a margin for the allocator.
// The three limb-8 planes of the quotient's transforms (ntt.hip) cost nothing for a folded key,
// whose sets lend their unused c buffer; an unfolded key's are scratch of the context.
static double prove_working_set_bytes(uint32_t log_n, size_t n_slots, size_t n_in, size_t max_batch,
                                      size_t n_msm_max, size_t n_commitments, bool folded) {
  const size_t Bp = round_up(max_batch ? max_batch : 1024, 64);
  const size_t n = (size_t)1 << log_n;
  const SetBytes sb = prove_set_bytes(n_slots, n, n_in, Bp, Bp);
  const double set = (double)(sb.slots + 3 * sb.abc + sb.misc + sums_bytes(Bp) +
                              commit_buffer_bytes(n_commitments, Bp));
  const double digits = 254.0 * (double)((n_msm_max + 15) / 16) * Bp * 4;   // comb, k >= 16
  const double sint = (double)n_msm_max * Bp * 32;
  // two partial-sum buffers (msm_part_layout.h): 21 blocks of [255][Bp] G2 accumulators, lane 0's
  // digits of the uniform groups [255][G] and the list of those groups [G], as the digits at k >= 16
  const double partials = 2 * (21.0 * 254 * Bp * 256 + 256.0 * (double)((n_msm_max + 15) / 16) * 4);
  // device half of the witness entry's staging ring (witness.hip): three chunks of ~64 MB, or of
  // one 64-proof column block of the wire matrix when that is larger (n_in = n_wires here)
  const double ring = 3.0 * std::max(68e6, (double)n_in * 32 * 64);
  const double planes = (folded || log_n < 8) ? 0.0 : 3.0 * (double)n * Bp * 4;
  return 2 * set + (double)n * Bp * 32 + planes + digits + sint + partials + ring + 2e9 + 1e9;
}
static double free_hbm_bytes() {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)64 << 30;
  return (double)free_b;
}
// standalone base sets (zkmi_msm_bases_load): working set of a 1024-wide zkmi_msm_batch
static double usable_table_bytes_standalone(size_t n) {
  const double ws = (double)n * 1024 * 32 * 2 + 254.0 * ((n + 15) / 16) * 1024 * 4 +
                    21.0 * 254 * 1024 * 256 + 3e9;
  const double usable = free_hbm_bytes() - ws;
  return usable > 0 ? usable : 0.0;
}

int zkmi_msm_bases_load(zkmi_ctx* ctx, int group, const void* bases, size_t n, int window_bits,
                        zkmi_msm_bases** out) {
  return zkmi_msm_bases_load_image(ctx, group, bases, n, window_bits, 0, out);
}

int zkmi_msm_bases_load_image(zkmi_ctx* ctx, int group, const void* bases, size_t n,
                              int window_bits, int image, zkmi_msm_bases** out) {
  ZK_HIP(hipSetDevice(ctx->device));
  if (!out) return ZKMI_ERR_ARG;
  if (image != 0 && image != 1) {
    ctx->err = "image must be 0 (x * 2^256) or 1 (x * 2^261)";
    return ZKMI_ERR_ARG;
  }
  if (!window_bits_ok(window_bits)) {
    ctx->err = "window_bits must be 0 (auto), in [2,16], 100 + [4,16], 200 + [2,20] or 300 + [3,21]";
    return ZKMI_ERR_ARG;
  }
  Staged sb(ctx);
  int rc = sb.in(bases, n * (group == 1 ? 64 : 128));
  if (rc) return rc;
  WinPlan plan;
  if (window_bits) {
    plan = plan_explicit(window_bits);
  } else {
    // per-window tables need no Horner tail: keep them when they reach as few windows as the
    // shared table would (small base sets); otherwise one shared table per base, or comb tables
    const double usable = usable_table_bytes_standalone(n);
    plan = plan_windows_for_budget(n, group, (group == 1 ? 0.64 : 0.34) * usable);
    int c1, c2;
    plan_shared_for_budget(group == 1 ? n : 0, group == 2 ? n : 0, 0.9 * usable, &c1, &c2);
    const WinPlan ps = plan_shared(group == 1 ? c1 : c2);
    if (ps.W < plan.W) plan = ps;
    if (n >= 64) {
      int k1, k2;
      bool s1, s2;
      comb_plan_equal(group == 1 ? n : 0, group == 2 ? n : 0, 0.9 * usable, &k1, &k2, &s1, &s2, true);
      const int k = group == 1 ? k1 : k2;
      if ((double)COMB_W / k < (double)plan.W) plan = plan_comb(k, group == 1 ? s1 : s2);
    }
  }
  return bases_load_plan(ctx, group, sb.dev, n, plan, window_bits == 0, out,
                         image ? MSM_IMAGE_F : MSM_IMAGE_STD);
}

void zkmi_msm_bases_free(zkmi_ctx* ctx, zkmi_msm_bases* b) {
  if (!b) return;
  if (ctx) {
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
  }
  if (b->table) hipFree(b->table);
  if (b->inf) hipFree(b->inf);
  delete b;
}

uint32_t zkmi_comb_min_groups_per_chunk(void) { return COMB_MIN_GROUPS_PER_CHUNK; }

int zkmi_msm_batch(zkmi_ctx* ctx, const zkmi_msm_bases* bases, const void* scalars, size_t batch,
                   void* out) {
  ZK_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = require_idle(ctx))) return rc;
  if (batch == 0) return ZKMI_OK;
  const size_t n = bases->n, Bp = round_up(batch, 64);
  const size_t pt = bases->group == 1 ? 64 : 128;
  Staged ss(ctx), so(ctx);
  if ((rc = ss.in(scalars, batch * n * 32)) || (rc = so.out(out, batch * pt))) return rc;
  void *sbi, *acc, *aff;
  if ((rc = ensure_scratch(ctx, ctx->sets[0].a, (n ? n : 1) * Bp * 32, &sbi)) ||
      (rc = ensure_scratch(ctx, ctx->sets[0].b, Bp * pt * 2, &acc)) ||
      (rc = ensure_scratch(ctx, ctx->sets[0].c, Bp * pt, &aff)))
    return rc;
  if ((rc = transpose_in(ctx, ss.dev, sbi, n, batch, Bp, 32))) return rc;
  if ((rc = msm_run(ctx, bases, (const Fr*)sbi, nullptr, Bp, batch, acc))) return rc;
  if ((rc = xyzz_to_affine(ctx, bases->group, acc, aff, Bp))) return rc;
  ZK_HIP(hipMemcpyAsync(so.dev, aff, batch * pt, hipMemcpyDeviceToDevice, ctx->stream));
  if ((rc = so.finish())) return rc;
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}

int zkmi_msm_batch_rows(zkmi_ctx* ctx, const zkmi_msm_bases* bases, const void* scalars,
                        size_t n_rows, const uint32_t* row_idx, size_t batch, int image, int uniform,
                        void* out) {
  ZK_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = require_idle(ctx))) return rc;
  if (batch == 0) return ZKMI_OK;
  const size_t n = bases->n, Bp = round_up(batch, 64);
  if ((image != 0 && image != 1) || uniform < 0 || uniform > 2 || n_rows == 0) {
    ctx->err = "msm_batch_rows: image in {0, 1}, uniform in {0, 1, 2}, n_rows > 0";
    return ZKMI_ERR_ARG;
  }
  std::vector<uint32_t> idx(n);
  if (row_idx) {
    if (n && hipMemcpy(idx.data(), row_idx, n * sizeof(uint32_t), hipMemcpyDefault) != hipSuccess) {
      (void)hipGetLastError();
      ctx->err = "msm_batch_rows: cannot read row_idx";
      return ZKMI_ERR_ARG;
    }
  } else {
    for (size_t i = 0; i < n; i++) idx[i] = (uint32_t)i;
  }
  // every row number is range-checked on the host before a kernel uses it
  for (uint32_t r : idx)
    if (r >= n_rows) {
      ctx->err = "msm_batch_rows: row_idx holds a row >= n_rows";
      return ZKMI_ERR_ARG;
    }
  const size_t pt = bases->group == 1 ? 64 : 128;
  Staged ss(ctx), so(ctx), si(ctx);
  if ((rc = ss.in(scalars, batch * n_rows * 32)) || (rc = so.out(out, batch * pt)) ||
      (rc = si.in(idx.data(), n * sizeof(uint32_t))))
    return rc;
  void *sbi, *acc, *aff, *flags = nullptr;
  if ((rc = ensure_scratch(ctx, ctx->sets[0].a, n_rows * Bp * 32, &sbi)) ||
      (rc = ensure_scratch(ctx, ctx->sets[0].b, Bp * pt * 2, &acc)) ||
      (rc = ensure_scratch(ctx, ctx->sets[0].c, Bp * pt, &aff)))
    return rc;
  if ((rc = transpose_in(ctx, ss.dev, sbi, n_rows, batch, Bp, 32))) return rc;
  if (uniform == 1 && ((rc = ensure_scratch(ctx, ctx->msm_rowvar, n_rows, &flags)) ||
                       (rc = msm_rows_vary(ctx, (const Fr*)sbi, n_rows, Bp, batch, (uint8_t*)flags))))
    return rc;
  if ((rc = msm_run(ctx, bases, (const Fr*)sbi, (const uint32_t*)si.dev, Bp, batch, acc, image == 1,
                    nullptr, nullptr, (const uint8_t*)flags, uniform == 2)))
    return rc;
  if ((rc = xyzz_to_affine(ctx, bases->group, acc, aff, Bp))) return rc;
  ZK_HIP(hipMemcpyAsync(so.dev, aff, batch * pt, hipMemcpyDeviceToDevice, ctx->stream));
  if ((rc = so.finish())) return rc;
  ZK_HIP(hipStreamSynchronize(ctx->stream));   // idx is read by the queued copy until here
  return ZKMI_OK;
}

int zkmi_fixed_base_mul(zkmi_ctx* ctx, int group, const void* base, const void* scalars, size_t n,
                        void* out) {
  // an MSM over ONE base with the scalars playing the role of the batch
  ZK_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = require_idle(ctx))) return rc;
  if (n == 0) return ZKMI_OK;
  zkmi_msm_bases* b = nullptr;
  if ((rc = zkmi_msm_bases_load(ctx, group, base, 1, 8, &b))) return rc;
  const size_t Bp = round_up(n, 64);
  const size_t pt = group == 1 ? 64 : 128;
  Staged ss(ctx), so(ctx);
  void *sbi = nullptr, *acc = nullptr, *aff = nullptr;
  if ((rc = ss.in(scalars, n * 32)) || (rc = so.out(out, n * pt)) ||
      (rc = ensure_scratch(ctx, ctx->sets[0].a, Bp * 32, &sbi)) ||
      (rc = ensure_scratch(ctx, ctx->sets[0].b, Bp * pt * 2, &acc)) ||
      (rc = ensure_scratch(ctx, ctx->sets[0].c, Bp * pt, &aff))) {
    zkmi_msm_bases_free(ctx, b);
    return rc;
  }
  rc = transpose_in(ctx, ss.dev, sbi, 1, n, Bp, 32);   // one row of n scalars, batch-inner
  if (!rc) rc = msm_run(ctx, b, (const Fr*)sbi, nullptr, Bp, n, acc);
  if (!rc) rc = xyzz_to_affine(ctx, group, acc, aff, Bp);
  if (!rc) {
    hipMemcpyAsync(so.dev, aff, n * pt, hipMemcpyDeviceToDevice, ctx->stream);
    rc = so.finish();
  }
  hipStreamSynchronize(ctx->stream);
  zkmi_msm_bases_free(ctx, b);
  return rc;
}

// ---- proving key / constraint system -------------------------------------------------------------
static int upload_u32(zkmi_ctx* ctx, const uint32_t* src, size_t n, uint32_t** out) {
  *out = nullptr;
  if (n == 0) return ZKMI_OK;
  ZK_HIP(hipMalloc((void**)out, n * 4));
  ZK_HIP(hipMemcpy(*out, src, n * 4, hipMemcpyDefault));
  return ZKMI_OK;
}

void zkmi_pk_free(zkmi_ctx* ctx, zkmi_pk* pk) {
  if (!pk) return;
  if (ctx) hipSetDevice(ctx->device);
  zkmi_msm_bases_free(ctx, pk->A);
  zkmi_msm_bases_free(ctx, pk->B1);
  zkmi_msm_bases_free(ctx, pk->K);
  zkmi_msm_bases_free(ctx, pk->Z);
  zkmi_msm_bases_free(ctx, pk->B2);
  zkmi_msm_bases_free(ctx, pk->D1);
  zkmi_msm_bases_free(ctx, pk->D2);
  commit_keys_free(ctx, pk);
  if (pk->idx3) hipFree(pk->idx3);
  if (pk->a_wire) hipFree(pk->a_wire);
  if (pk->b_wire) hipFree(pk->b_wire);
  if (pk->k_wire) hipFree(pk->k_wire);
  delete pk;
}

// wire index of every retained base from a gnark-style infinity map ([]bool, one byte per wire)
static int wires_from_infinity(zkmi_ctx* ctx, const uint8_t* inf, uint32_t n_wires, uint32_t want,
                               const char* name, std::vector<uint32_t>* out) {
  std::vector<uint8_t> host(n_wires);
  if (n_wires && hipMemcpy(host.data(), inf, n_wires, hipMemcpyDefault) != hipSuccess) {
    ctx->err = std::string("pk: cannot read ") + name;
    return ZKMI_ERR_HIP;
  }
  out->clear();
  for (uint32_t i = 0; i < n_wires; i++)
    if (!host[i]) out->push_back(i);
  if (out->size() != want) {
    ctx->err = std::string("pk: ") + name + " retains " + std::to_string(out->size()) +
               " wires but the key holds " + std::to_string(want) + " points";
    return ZKMI_ERR_ARG;
  }
  return ZKMI_OK;
}

int zkmi_pk_load(zkmi_ctx* ctx, const zkmi_pk_desc* d, zkmi_pk** out) {
  return zkmi_pk_load_planned(ctx, d, nullptr, out);
}

int zkmi_pk_load_planned(zkmi_ctx* ctx, const zkmi_pk_desc* d, const uint32_t* msm_window_bits,
                         zkmi_pk** out) {
  ZK_HIP(hipSetDevice(ctx->device));
  if (!d || !out) return ZKMI_ERR_ARG;
  if (msm_window_bits)
    for (int i = 0; i < COMB_PLAN_MSMS; i++)
      if (msm_window_bits[i] == 0 || !window_bits_ok((int)msm_window_bits[i])) {
        ctx->err = "pk: msm_window_bits must be in [2,16], 100 + [4,16], 200 + [2,20] or 300 + [3,21]";
        return ZKMI_ERR_ARG;
      }
  // the G1 window sums are finished together (zkmi_prove_collect_ex): all four stop at them, or none
  if (msm_window_bits)
    for (int i = 0; i < COMB_MSM_Z; i++)
      if ((msm_window_bits[i] >= 100) != (msm_window_bits[COMB_MSM_Z] >= 100)) {
        ctx->err = "pk: msm_window_bits of A, B1, K and Z must all be per-window plans or none";
        return ZKMI_ERR_ARG;
      }
  if (d->log_n < 1 || d->log_n > 28) {
    ctx->err = "pk: log_n out of range [1,28]";
    return ZKMI_ERR_ARG;
  }
  // gnark allocates pk.G1.Z with Domain.Cardinality entries and uses the first n - 1
  // [UPSTREAM-RECALL]: longer arrays are accepted and truncated
  if (d->n_z + 1 < (1u << d->log_n)) {
    ctx->err = "pk: n_z must be at least 2^log_n - 1";
    return ZKMI_ERR_ARG;
  }
  const uint32_t n_z = (1u << d->log_n) - 1;
  // wire index of every base: explicit arrays, or gnark's InfinityA / InfinityB / nbPublic
  std::vector<uint32_t> wa, wb, wk;
  {
    int rc;
    struct { const uint32_t* p; uint32_t n; const char* name; std::vector<uint32_t>* v; } idx[3] = {
        {d->a_wire, d->n_a, "a_wire", &wa}, {d->b_wire, d->n_b, "b_wire", &wb},
        {d->k_wire, d->n_k, "k_wire", &wk}};
    for (auto& t : idx) {
      if (!t.p) continue;
      t.v->resize(t.n);
      if (t.n && hipMemcpy(t.v->data(), t.p, (size_t)t.n * 4, hipMemcpyDefault) != hipSuccess) {
        ctx->err = std::string("pk: cannot read ") + t.name;
        return ZKMI_ERR_HIP;
      }
    }
    if (!d->a_wire) {
      if (!d->infinity_a) {
        ctx->err = "pk: neither a_wire nor infinity_a given";
        return ZKMI_ERR_ARG;
      }
      if ((rc = wires_from_infinity(ctx, d->infinity_a, d->n_wires, d->n_a, "infinity_a", &wa)))
        return rc;
    }
    if (!d->b_wire) {
      if (!d->infinity_b) {
        ctx->err = "pk: neither b_wire nor infinity_b given";
        return ZKMI_ERR_ARG;
      }
      if ((rc = wires_from_infinity(ctx, d->infinity_b, d->n_wires, d->n_b, "infinity_b", &wb)))
        return rc;
    }
    if (!d->k_wire) {
      if (d->n_public < 1 || d->n_public > d->n_wires ||
          (d->n_commitments == 0 && d->n_wires - d->n_public != d->n_k)) {
        ctx->err = "pk: without k_wire, n_public must satisfy n_wires - n_public == n_k";
        return ZKMI_ERR_ARG;
      }
      // gnark's setup leaves the private committed wires and the commitment wires out of G1.K
      std::vector<uint8_t> taken(d->n_wires, 0);
      for (uint32_t i = 0; i < d->n_commitments && d->commitments; i++) {
        const zkmi_commitment_desc& c = d->commitments[i];
        std::vector<uint32_t> pw(c.n_private);
        if (c.n_private && (!c.private_wires || hipMemcpy(pw.data(), c.private_wires, (size_t)c.n_private * 4,
                                                           hipMemcpyDefault) != hipSuccess)) {
          ctx->err = "pk: cannot read the private wires of commitment " + std::to_string(i);
          return ZKMI_ERR_ARG;
        }
        for (uint32_t w : pw)
          if (w < d->n_wires) taken[w] = 1;
        if (c.commitment_wire < d->n_wires) taken[c.commitment_wire] = 1;
      }
      wk.clear();
      for (uint32_t w = d->n_public; w < d->n_wires; w++)
        if (!taken[w]) wk.push_back(w);
      if (wk.size() != d->n_k) {
        ctx->err = "pk: n_k does not match n_wires - n_public - committed wires";
        return ZKMI_ERR_ARG;
      }
    }
    // every wire index is range-checked on the host before any kernel can use it as a row number
    for (auto& t : idx)
      for (uint32_t w : *t.v)
        if (w >= d->n_wires) {
          ctx->err = std::string("pk: ") + t.name + " holds a wire index >= n_wires";
          return ZKMI_ERR_ARG;
        }
  }
  if (!window_bits_ok((int)d->window_bits_g1) || !window_bits_ok((int)d->window_bits_g2)) {
    ctx->err = "pk: window_bits must be 0 (auto), in [2,16], 100 + [4,16], 200 + [2,20] or 300 + [3,21]";
    return ZKMI_ERR_ARG;
  }
  if (d->msm_chunk_factor > 64) {
    ctx->err = "pk: msm_chunk_factor must be in [0,64]";
    return ZKMI_ERR_ARG;
  }
  // Quotient in evaluation form: E in the place of Z (n bases), the c term folded into the K bases
  // (quotient_fold.h).  The results wait on the host and every device buffer of the fold is freed
  // again, so the tables below are planned against the same free HBM as those of an unfolded key.
  FoldedKey fold;
  if (d->fold_r1cs) {
    const int frc = quotient_fold_key(ctx, d, wk, &fold);
    if (frc) return frc;
  }
  const uint32_t n_kb = fold.folded ? (uint32_t)fold.k_wire.size() : d->n_k;
  const uint32_t n_zb = fold.folded ? n_z + 1 : n_z;
  auto* pk = new zkmi_pk();
  pk->log_n = d->log_n;
  pk->n_wires = d->n_wires;
  pk->n_a = d->n_a;
  pk->n_b = d->n_b;
  pk->n_k = n_kb;
  pk->n_z = n_zb;
  pk->folded = fold.folded;
  pk->fold_n_constraints = fold.folded ? d->fold_r1cs->n_constraints : 0;
  pk->max_batch = d->max_batch ? d->max_batch : 1024;
  int rc;
  // commitment keys first (per-window tables of the Pedersen bases, 2 x 33 KB per committed wire at
  // the widest setting): the plan below is sized against the HBM that is free AFTER them
  if ((rc = commit_keys_load(ctx, d, pk))) {
    zkmi_pk_free(ctx, pk);
    return rc;
  }
  // One window plan per group for the whole key; comb plans then get a group size per MSM (below).
  // Auto plans are sized against the free HBM minus
  // the working set of the largest batch the caller will prove (and the caller's own cap).
  const bool auto1 = d->window_bits_g1 == 0, auto2 = d->window_bits_g2 == 0;
  const size_t n1 = (size_t)d->n_a + d->n_b + n_kb + n_zb;
  const size_t n_msm_max = std::max(std::max((size_t)d->n_a, (size_t)d->n_b),
                                    std::max((size_t)n_kb, (size_t)n_zb));
  const size_t n_slots = d->n_slots_hint ? d->n_slots_hint : (size_t)d->n_wires + d->n_wires / 20;
  const double ws = prove_working_set_bytes(d->log_n, n_slots, d->n_wires, pk->max_batch, n_msm_max,
                                            pk->commits.size(), pk->folded);
  double usable = free_hbm_bytes() - ws;
  if (usable < 0) usable = 0;
  if (d->table_budget_bytes && (double)d->table_budget_bytes < usable)
    usable = (double)d->table_budget_bytes;
  // auto: per-window tables when they reach as few windows as a shared table would (small keys:
  // no Horner tail), otherwise one shared table per base
  int sc1 = 0, sc2 = 0;
  plan_shared_for_budget(n1, d->n_b, 0.98 * usable, &sc1, &sc2);
  WinPlan p1 = auto1 ? plan_windows_for_budget(n1, 1, 0.64 * usable)
                     : plan_explicit((int)d->window_bits_g1);
  WinPlan p2 = auto2 ? plan_windows_for_budget(d->n_b, 2, 0.34 * usable)
                     : plan_explicit((int)d->window_bits_g2);
  if (auto1 && sc1 && plan_shared(sc1).W < p1.W) p1 = plan_shared(sc1);
  if (auto2 && sc2 && plan_shared(sc2).W < p2.W) p2 = plan_shared(sc2);
  // comb tables (joint tables over k bases) when they need fewer additions per base still; small
  // keys keep the layouts above (their MSMs are latency, not throughput).  Each MSM gets a group
  // size of its own (comb_plan.h): the dense quotient MSM executes every group of every proof, the
  // wire MSMs only the groups that vary over the batch, so Z takes more of the bytes.
  WinPlan pm[COMB_PLAN_MSMS] = {p1, p1, p1, p1, p2};   // A, B1, K, Z, B2
  if (n1 >= 4096) {
    const size_t nm[COMB_PLAN_MSMS] = {auto1 ? d->n_a : 0u, auto1 ? d->n_b : 0u, auto1 ? n_kb : 0u,
                                       auto1 ? n_zb : 0u, auto2 ? d->n_b : 0u};
    const CombPlan eq = comb_plan_equal5(nm, 0.98 * usable, d->sparse_witness == 0);
    const CombPlan cp = comb_plan_search(nm, 0.98 * usable, d->sparse_witness == 0);
    for (int i = 0; i < COMB_PLAN_MSMS; i++) {
      const bool g2 = comb_msm_is_g2(i);
      if ((g2 ? auto2 : auto1) && (double)COMB_W / eq.k[i] < (double)(g2 ? p2 : p1).W)
        pm[i] = plan_comb(cp.k[i], cp.sg[i]);
    }
  }
  // sparse_witness = 2: (almost) every wire is a bit.  The wire MSMs then execute one addition per
  // group (window 0) whatever the group size, so they get small subset-sum tables and the dense
  // quotient MSM (h . Z) gets the HBM: the widest table that fits, sign patterns allowed.
  if (d->sparse_witness >= 2 && auto1 && auto2 && n1 >= 4096 && n_zb >= 4096) {
    const int kw = 12;
    const double wire_bytes =
        (double)((d->n_a + kw - 1) / kw + (d->n_b + kw - 1) / kw + (n_kb + kw - 1) / kw) *
            (double)(1u << kw) * 64.0 +
        (double)((d->n_b + kw - 1) / kw) * (double)(1u << kw) * 128.0;
    if (wire_bytes < 0.5 * usable) {
      int kz = 0, k2 = 0;
      bool sz = true, s2 = true;
      comb_plan_equal(n_zb, 0, 0.98 * usable - wire_bytes, &kz, &k2, &sz, &s2, true);
      for (int i = 0; i < COMB_PLAN_MSMS; i++) pm[i] = plan_comb(kw, false);
      pm[COMB_MSM_Z] = plan_comb(kz, sz);
    }
  }
  // an explicit plan per MSM (zkmi_pk_load_planned) replaces all of the above
  bool relax[COMB_PLAN_MSMS] = {auto1, auto1, auto1, auto1, auto2};
  if (msm_window_bits)
    for (int i = 0; i < COMB_PLAN_MSMS; i++) {
      pm[i] = plan_explicit((int)msm_window_bits[i]);
      relax[i] = false;
    }
  // The wire MSMs read the value file, which the solver leaves in the F image; the quotient MSM
  // reads h, which the NTT leaves in gnark's image, or the coset evaluations of a folded key, which
  // it leaves in the F image (compute_ab_coset_bi, out_f): sign-pattern tables are built native to
  // those, so that the digit pass reads all of them as they are.
  // (A batch that enters with gnark-image wires pays one conversion pass per wire MSM.)
  auto load = [&](int group, const void* pts, size_t n, const WinPlan& plan, bool relax,
                  zkmi_msm_bases** out, int image) -> int {
    Staged sb(ctx);
    int r = sb.in(pts, n * (group == 1 ? 64 : 128));
    if (r) return r;
    r = bases_load_plan(ctx, group, sb.dev, n, plan, relax, out, image);
    if (!r) (*out)->chunk_factor = d->msm_chunk_factor;
    return r;
  };
  if ((rc = upload_u32(ctx, wa.data(), d->n_a, &pk->a_wire)) ||
      (rc = upload_u32(ctx, wb.data(), d->n_b, &pk->b_wire)) ||
      (rc = upload_u32(ctx, fold.folded ? fold.k_wire.data() : wk.data(), n_kb, &pk->k_wire)) ||
      (rc = load(1, d->g1_a, d->n_a, pm[COMB_MSM_A], relax[COMB_MSM_A], &pk->A, MSM_IMAGE_F)) ||
      (rc = load(1, d->g1_b, d->n_b, pm[COMB_MSM_B1], relax[COMB_MSM_B1], &pk->B1, MSM_IMAGE_F)) ||
      (rc = load(1, fold.folded ? (const void*)fold.k.data() : d->g1_k, n_kb, pm[COMB_MSM_K],
                 relax[COMB_MSM_K], &pk->K, MSM_IMAGE_F)) ||
      (rc = load(1, fold.folded ? (const void*)fold.e.data() : d->g1_z, n_zb, pm[COMB_MSM_Z],
                 relax[COMB_MSM_Z], &pk->Z, fold.folded ? MSM_IMAGE_F : MSM_IMAGE_STD)) ||
      (rc = load(2, d->g2_b, d->n_b, pm[COMB_MSM_B2], relax[COMB_MSM_B2], &pk->B2, MSM_IMAGE_F))) {
    zkmi_pk_free(ctx, pk);
    return rc;
  }
  {
    const uint32_t idx[3] = {0, 1, 2};
    if ((rc = upload_u32(ctx, idx, 3, &pk->idx3)) ||
        (rc = zkmi_msm_bases_load(ctx, 1, d->g1_delta, 1, 8, &pk->D1)) ||
        (rc = zkmi_msm_bases_load(ctx, 2, d->g2_delta, 1, 8, &pk->D2))) {
      zkmi_pk_free(ctx, pk);
      return rc;
    }
    pk->D1->side = pk->D2->side = 2;   // run on the assembly stream (enqueue_heavy)
  }
  hipMemcpy(&pk->alpha, d->g1_alpha, 64, hipMemcpyDefault);
  hipMemcpy(&pk->beta1, d->g1_beta, 64, hipMemcpyDefault);
  hipMemcpy(&pk->delta1, d->g1_delta, 64, hipMemcpyDefault);
  hipMemcpy(&pk->beta2, d->g2_beta, 128, hipMemcpyDefault);
  hipMemcpy(&pk->delta2, d->g2_delta, 128, hipMemcpyDefault);
  *out = pk;
  return ZKMI_OK;
}

int zkmi_pk_info(const zkmi_pk* pk, uint64_t* info) {
  if (!pk || !info) return ZKMI_ERR_ARG;
  info[0] = (uint64_t)pk->Z->plan.W;
  info[1] = pk->Z->plan.per_base;
  info[2] = (uint64_t)pk->B2->plan.W;
  info[3] = pk->B2->plan.per_base;
  info[4] = pk->A->table_bytes + pk->B1->table_bytes + pk->K->table_bytes + pk->Z->table_bytes;
  info[5] = pk->B2->table_bytes;
  info[6] = pk->Z->plan.shared;
  info[7] = pk->B2->plan.shared;
  info[8] = pk->Z->plan.comb;
  info[9] = pk->B2->plan.comb;
  return ZKMI_OK;
}

int zkmi_pk_msm_plan(const zkmi_pk* pk, uint32_t* plan) {
  if (!pk || !plan) return ZKMI_ERR_ARG;
  const zkmi_msm_bases* ms[COMB_PLAN_MSMS] = {pk->A, pk->B1, pk->K, pk->Z, pk->B2};
  for (int i = 0; i < COMB_PLAN_MSMS; i++) {
    plan[i] = ms[i]->plan.comb;
    plan[COMB_PLAN_MSMS + i] = ms[i]->plan.comb_signed;
  }
  return ZKMI_OK;
}

int zkmi_pk_folded(const zkmi_pk* pk) { return pk && pk->folded ? 1 : 0; }

void zkmi_cs_free(zkmi_ctx* ctx, zkmi_cs* cs) {
  if (!cs) return;
  if (ctx) hipSetDevice(ctx->device);
  if (cs->program) hipFree(cs->program);
  if (cs->consts) hipFree(cs->consts);
  delete cs;
}

int zkmi_cs_load(zkmi_ctx* ctx, const zkmi_cs_desc* d, zkmi_cs** out) {
  ZK_HIP(hipSetDevice(ctx->device));
  if (!d || !out) return ZKMI_ERR_ARG;
  auto* cs = new zkmi_cs();
  // every slot / constant / row index is checked on the host before anything reaches a kernel
  const std::string err =
      vprog_validate({d->n_wires, d->n_slots, d->n_consts, d->n_constraints, d->n_rows,
                      d->lanes_per_proof},
                     d->program, &cs->commit_rows, &cs->has_emul);
  if (!err.empty()) {
    delete cs;
    ctx->err = err;
    return ZKMI_ERR_ARG;
  }
  cs->n_wires = d->n_wires;
  cs->n_public = d->n_public;
  cs->n_secret = d->n_secret;
  cs->n_constraints = d->n_constraints;
  cs->n_slots = d->n_slots;
  cs->n_rows = d->n_rows;
  cs->n_consts = d->n_consts;
  cs->lanes_per_proof = d->lanes_per_proof;
  int rc = upload_u32(ctx, d->program, (size_t)d->n_rows * (1 + d->lanes_per_proof) * 4,
                      &cs->program);
  if (rc) {
    delete cs;
    return rc;
  }
  if (d->n_consts) {
    if (hipMalloc((void**)&cs->consts, (size_t)d->n_consts * 32) != hipSuccess ||
        hipMemcpy(cs->consts, d->consts, (size_t)d->n_consts * 32, hipMemcpyDefault) !=
            hipSuccess) {
      ctx->err = "cs: constant pool upload failed";
      zkmi_cs_free(ctx, cs);
      return ZKMI_ERR_HIP;
    }
    // the solver works in the 2^261 domain (solve.hip)
    if ((rc = array_to_f_domain(ctx, cs->consts, d->n_consts)) ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) {
      zkmi_cs_free(ctx, cs);
      return rc ? rc : ZKMI_ERR_HIP;
    }
  }
  *out = cs;
  return ZKMI_OK;
}

// inputs proof-major -> slot rows 1..n_in
static int stage_inputs(zkmi_ctx* ctx, const zkmi_cs* cs, const void* inputs_dev, size_t batch,
                        size_t Bp, Fr* slots) {
  const size_t n_in = cs->n_public - 1 + cs->n_secret;
  int rc = transpose_in(ctx, inputs_dev, slots + Bp, n_in, batch, Bp, 32);
  if (rc) return rc;
  return rows_to_f_domain(ctx, slots + Bp, n_in, Bp);
}

int zkmi_solve_batch(zkmi_ctx* ctx, const zkmi_cs* cs, const void* inputs, size_t batch,
                     void* wires_out, void* abc_out, int32_t* status_out) {
  ZK_HIP(hipSetDevice(ctx->device));
  int rc;
  if ((rc = require_idle(ctx))) return rc;
  if (batch == 0) return ZKMI_OK;
  if (!cs->commit_rows.empty()) {
    ctx->err = "solve_batch: this system has commitments; its commitment wires come from the "
               "proving key's Pedersen bases: use zkmi_prove_submit";
    return ZKMI_ERR_ARG;
  }
  const size_t Bp = round_up(batch, 64);
  const size_t n_in = cs->n_public - 1 + cs->n_secret;
  const size_t nc = cs->n_constraints ? cs->n_constraints : 1;
  Staged si(ctx), sw(ctx), sabc(ctx), sst(ctx);
  if ((rc = si.in(inputs, batch * n_in * 32))) return rc;
  if (wires_out && (rc = sw.out(wires_out, batch * (size_t)cs->n_wires * 32))) return rc;
  if (abc_out && (rc = sabc.out(abc_out, 3 * batch * (size_t)cs->n_constraints * 32))) return rc;
  if ((rc = sst.out(status_out, batch * 4))) return rc;
  void *slots, *a, *b, *c, *st;
  zkmi_ctx::ProveSet& S = ctx->sets[0];
  if ((rc = ensure_scratch(ctx, S.slots, (size_t)cs->n_slots * Bp * 32, &slots)) ||
      (rc = ensure_scratch(ctx, S.a, nc * Bp * 32, &a)) ||
      (rc = ensure_scratch(ctx, S.b, nc * Bp * 32, &b)) ||
      (rc = ensure_scratch(ctx, S.c, nc * Bp * 32, &c)) ||
      (rc = ensure_scratch(ctx, S.misc, Bp * 4, &st)))
    return rc;
  if ((rc = stage_inputs(ctx, cs, si.dev, batch, Bp, (Fr*)slots))) return rc;
  if ((rc = solve_bi(ctx, cs, (Fr*)slots, (Fr*)a, (Fr*)b, (Fr*)c, (int32_t*)st, Bp))) return rc;
  // back to gnark's image for the caller
  if (wires_out && ((rc = rows_to_std_domain(ctx, (Fr*)slots, cs->n_wires, Bp)) ||
                    (rc = transpose_out(ctx, slots, sw.dev, cs->n_wires, batch, Bp, 32))))
    return rc;
  if (abc_out) {
    if ((rc = rows_to_std_domain(ctx, (Fr*)a, cs->n_constraints, Bp)) ||
        (rc = rows_to_std_domain(ctx, (Fr*)b, cs->n_constraints, Bp)) ||
        (rc = rows_to_std_domain(ctx, (Fr*)c, cs->n_constraints, Bp)))
      return rc;
    const size_t stride = batch * (size_t)cs->n_constraints * 32;
    if ((rc = transpose_out(ctx, a, sabc.dev, cs->n_constraints, batch, Bp, 32)) ||
        (rc = transpose_out(ctx, b, (char*)sabc.dev + stride, cs->n_constraints, batch, Bp, 32)) ||
        (rc = transpose_out(ctx, c, (char*)sabc.dev + 2 * stride, cs->n_constraints, batch, Bp,
                            32)))
      return rc;
  }
  ZK_HIP(hipMemcpyAsync(sst.dev, st, batch * 4, hipMemcpyDeviceToDevice, ctx->stream));
  if ((rc = sw.finish()) || (rc = sabc.finish()) || (rc = sst.finish())) return rc;
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return ZKMI_OK;
}

// Stage 1 of a prove: inputs -> value file, witness solve.  Runs on stream2 so that it overlaps
// the NTT/MSM kernels of the previously submitted batch (the solve is a 16-wavefront latency chain).
int zkmi_prove_submit(zkmi_ctx* ctx, const zkmi_pk* pk, const zkmi_cs* cs, const void* inputs,
                      size_t batch, const void* rs) {
  ZK_HIP(hipSetDevice(ctx->device));
  if (batch == 0) {
    ctx->err = "prove: empty batch";
    return ZKMI_ERR_ARG;
  }
  if (pk->n_wires != cs->n_wires) {
    ctx->err = "prove: proving key and constraint system disagree on the number of wires";
    return ZKMI_ERR_ARG;
  }
  if (cs->n_constraints > (1u << pk->log_n)) {
    ctx->err = "prove: domain smaller than the number of constraints";
    return ZKMI_ERR_ARG;
  }
  if (pk->folded && cs->n_constraints != pk->fold_n_constraints) {
    ctx->err = "prove: the key was folded (zkmi_pk_desc.fold_r1cs) with a system of " +
               std::to_string(pk->fold_n_constraints) + " constraints, this one has " +
               std::to_string(cs->n_constraints);
    return ZKMI_ERR_ARG;
  }
  if (cs->commit_rows.size() != pk->commits.size()) {
    ctx->err = "prove: the constraint system has " + std::to_string(cs->commit_rows.size()) +
               " commitments, the proving key " + std::to_string(pk->commits.size());
    return ZKMI_ERR_ARG;
  }
  for (size_t i = 0; i < pk->commits.size(); i++)
    if (cs->commit_rows[i].second != pk->commits[i].wire) {
      ctx->err = "prove: commitment " + std::to_string(i) + " lands on different wires in the "
                 "constraint system and in the proving key";
      return ZKMI_ERR_ARG;
    }
  const size_t n_in = cs->n_public - 1 + cs->n_secret;
  hipStream_t main;
  char* stage;
  int rc = prove_set_begin(ctx, pk, cs->n_slots, n_in, batch, rs, &main, &stage);
  if (rc) return rc;
  zkmi_ctx::ProveSet& S = ctx->sets[ctx->next_submit];
  const size_t Bp = S.Bp;
  S.cs = cs;
  S.n_constraints = cs->n_constraints;
  S.f_domain = true;
  Fr *slots = (Fr*)S.slots.p, *a = (Fr*)S.a.p, *b = (Fr*)S.b.p, *c = (Fr*)S.c.p;
  int32_t* st = (int32_t*)S.st;
  // caller buffers are consumed before this function returns only if they are host memory
  // (pageable copies are synchronous); device buffers must stay valid until the collect
  const void* in_dev;
  rc = device_view(ctx, inputs, batch * n_in * 32, stage, &in_dev);
  if (!rc) rc = stage_inputs(ctx, cs, in_dev, batch, Bp, slots);
  if (!rc && cs->commit_rows.empty()) {
    rc = solve_bi(ctx, cs, slots, a, b, c, st, Bp);
  } else if (!rc) {
    // commitment extension: the program stops at every COMMIT row; the commitment is an MSM over
    // the wires solved so far, its hash becomes the commitment wire's value (commit.hip: the
    // host blocks on this stream for the hash -- the main stream keeps running the previous
    // batch's MSMs meanwhile)
    rc = solve_init(ctx, slots, st, Bp);
    uint32_t begin = 0;
    for (size_t i = 0; !rc && i < cs->commit_rows.size(); i++) {
      rc = solve_rows(ctx, cs, slots, a, b, c, st, Bp, begin, cs->commit_rows[i].first);
      if (!rc) rc = commit_phase(ctx, S, (uint32_t)i, true);
      begin = cs->commit_rows[i].first + 1;
    }
    if (!rc) rc = solve_rows(ctx, cs, slots, a, b, c, st, Bp, begin, cs->n_rows);
    if (!rc) rc = commit_finish_submit(ctx, S);
  }
  return prove_set_end(ctx, main, rc);
}

// The ALU-heavy part of stage 2 (quotient, five MSMs, the one-base delta MSMs) of set `si`, on the
// main stream.  Everything it touches besides the set's own buffers (NTT scratch, MSM digits) is
// only used on the main stream, so consecutive batches simply queue up behind each other; the two
// MSM partial-sum buffers are also read by the MSM tails on stream4, under part_ev (msm_impl.h).
static int enqueue_heavy(zkmi_ctx* ctx, int si) {
  zkmi_ctx::ProveSet& S = ctx->sets[si];
  const zkmi_pk* pk = S.pk;
  const bool fd = S.f_domain;
  const size_t Bp = S.Bp, batch = S.batch, n = (size_t)1 << pk->log_n;
  NttPlan* plan;
  int rc = get_plan(ctx, (int)pk->log_n, &plan);
  if (rc) return rc;
  void* t0;
  if ((rc = ensure_scratch(ctx, ctx->ntt_tmp, n * Bp * 32, &t0))) return rc;
  SumsView v(S.sums.p, Bp);
  Fr* rs_bi = (Fr*)S.rs;
  Fr* slots = (Fr*)S.slots.p;
  ZK_HIP(hipStreamWaitEvent(ctx->stream, S.ev1, 0));
  hipEventRecord(S.evq[0], ctx->stream);
  // h: the quotient's coefficients, or (folded key) the coset evaluations of a b.  There nobody
  // reads S.c and the set's solve is over (ev1), so its n * Bp * 32 bytes hold the three limb-8
  // planes of the transforms; an unfolded key's come from the context (ntt_top)
  Fr* h;
  if ((rc = pk->folded ? compute_ab_coset_bi(ctx, plan, (Fr*)S.a.p, (Fr*)S.b.p, (Fr*)t0, Bp,
                                             S.n_constraints, &h, fd, (int32_t*)S.c.p, true)
                       : compute_h_bi(ctx, plan, (Fr*)S.a.p, (Fr*)S.b.p, (Fr*)S.c.p, (Fr*)t0, Bp,
                                      S.n_constraints, &h, fd)))
    return rc;
  hipEventRecord(S.evq[1], ctx->stream);
  S.msm_ev_used = 0;
  ctx->msm_ev_set = si;
  // shared-table plans: stop at the window sums, the Horner step runs with the assembly
  const bool d1 = pk->Z->plan.shared || pk->Z->plan.comb;
  const bool d2 = pk->B2->plan.shared || pk->B2->plan.comb;
  // The tails of the five MSMs (msm_run's finish stream) run on stream4, not on the assembly
  // stream: there the tail of this batch's A would queue behind the previous batch's assembly
  // (~26 ms), and K, which takes A's partial-sum buffer, would hold the main stream until it is read.
  hipStream_t q3 = ctx->stream3, q4 = ctx->stream4;
  // comb plans: A, B1, K and B2 walk overlapping rows of the value file, so which wires vary over
  // the batch is found once for all four; the quotient's scalars are dense
  uint8_t* rv = nullptr;
  if (pk->A->plan.comb || pk->B2->plan.comb) {
    void* p;
    if ((rc = ensure_scratch(ctx, ctx->msm_rowvar, pk->n_wires, &p)) ||
        (rc = msm_rows_vary(ctx, slots, pk->n_wires, Bp, batch, (uint8_t*)p))) {
      ctx->msm_ev_set = -1;
      return rc;
    }
    rv = (uint8_t*)p;
  }
  if ((rc = msm_run(ctx, pk->A, slots, pk->a_wire, Bp, batch, v.sA, fd, d1 ? v.w1[0] : nullptr, q4,
                    rv)) ||
      (rc = msm_run(ctx, pk->B1, slots, pk->b_wire, Bp, batch, v.sB1, fd, d1 ? v.w1[1] : nullptr, q4,
                    rv)) ||
      (rc = msm_run(ctx, pk->K, slots, pk->k_wire, Bp, batch, v.sK, fd, d1 ? v.w1[2] : nullptr, q4,
                    rv)) ||
      (rc = msm_run(ctx, pk->Z, h, nullptr, Bp, batch, v.sZ, pk->folded, d1 ? v.w1[3] : nullptr,
                    q4, nullptr, true))) {
    ctx->msm_ev_set = -1;
    return rc;
  }
  hipEventRecord(S.evq[2], ctx->stream);
  rc = msm_run(ctx, pk->B2, slots, pk->b_wire, Bp, batch, v.sB2, fd, d2 ? v.w2 : nullptr, q4, rv);
  ctx->msm_ev_set = -1;
  if (rc) return rc;
  hipEventRecord(S.evq[3], ctx->stream);
  // stream4 is in order: behind B2's tail, the window sums of all five MSMs are complete
  ZK_HIP(hipEventRecord(S.tail_ev, q4));
  // The multiples of delta (r, s, -rs times delta1; s times delta2) are four one-base MSMs of sixteen
  // wavefronts each: latency, not work.  They run on the assembly stream, which is where their
  // results are used, with their own partial-sum scratch (side = 2) -- on the main stream they were
  // 4.2 ms per batch during which 240 CUs idled.
  {
    hipStream_t main_stream = ctx->stream;
    ZK_HIP(hipStreamWaitEvent(q3, S.ev1, 0));   // r, s staged by the submit
    ctx->stream = q3;
    hipLaunchKernelGGL(rs_prep_kernel, dim3((unsigned)(Bp / 64)), dim3(64), 0, q3, rs_bi, Bp);
    (void)((rc = msm_run(ctx, pk->D1, rs_bi, pk->idx3 + 0, Bp, batch, v.tR)) ||
           (rc = msm_run(ctx, pk->D1, rs_bi, pk->idx3 + 1, Bp, batch, v.tS)) ||
           (rc = msm_run(ctx, pk->D1, rs_bi, pk->idx3 + 2, Bp, batch, v.tNRS)) ||
           (rc = msm_run(ctx, pk->D2, rs_bi, pk->idx3 + 1, Bp, batch, v.tS2)));
    ctx->stream = main_stream;
    if (rc) return rc;
  }
  if ((rc = commit_pok(ctx, S))) return rc;   // commitment extension: proof of knowledge
  hipEventRecord(S.evq[4], ctx->stream);
  S.heavy_enqueued = true;
  return ZKMI_OK;
}

// Stage 2: quotient, MSMs, assembly of the oldest submitted batch; blocks until its proofs are
// in proofs_out / status_out.  The latency-bound assembly (16 wavefronts) runs on a third stream
// and, when another batch is already submitted, that batch's quotient + MSM kernels are queued on
// the main stream BEFORE waiting, so the assembly of batch k overlaps the quotient of batch k+1.
int zkmi_prove_collect(zkmi_ctx* ctx, void* proofs_out, int32_t* status_out) {
  return zkmi_prove_collect_ex(ctx, proofs_out, status_out, nullptr);
}

int zkmi_prove_collect_ex(zkmi_ctx* ctx, void* proofs_out, int32_t* status_out,
                          void* commitments_out) {
  ZK_HIP(hipSetDevice(ctx->device));
  const int si = ctx->next_collect;
  zkmi_ctx::ProveSet& S = ctx->sets[si];
  if (!S.pending) {
    ctx->err = "prove: nothing submitted";
    return ZKMI_ERR_ARG;
  }
  if (!S.pk->commits.empty() && !commitments_out) {
    ctx->err = "prove: this key has commitments: collect with zkmi_prove_collect_ex";
    return ZKMI_ERR_ARG;
  }
  const zkmi_pk* pk = S.pk;
  const size_t batch = S.batch, Bp = S.Bp;
  int rc;
  if (!S.heavy_enqueued && (rc = enqueue_heavy(ctx, si))) return rc;
  SumsView v(S.sums.p, Bp);
  hipStream_t q3 = ctx->stream3;
  ZK_HIP(hipStreamWaitEvent(q3, S.evq[4], 0));
  ZK_HIP(hipStreamWaitEvent(q3, S.tail_ev, 0));   // the window sums the Horner steps read
  hipEventRecord(S.eva[0], q3);
  if (pk->Z->plan.shared || pk->Z->plan.comb) {
    void* ws[4] = {v.w1[0], v.w1[1], v.w1[2], v.w1[3]};
    void* os[4] = {v.sA, v.sB1, v.sK, v.sZ};
    const zkmi_msm_bases* ms[4] = {pk->A, pk->B1, pk->K, pk->Z};
    // One launch for the four when their window sums combine alike.  Comb plans: 254 one-bit
    // windows whatever the group size, so only the table kind has to agree (the correction window of
    // sign-pattern tables; stotal is per MSM).  Shared tables: the same window widths.
    bool same = true;
    for (int i = 0; i < 3; i++)
      same = same && (ms[i]->plan.comb != 0) == (pk->Z->plan.comb != 0) &&
             ms[i]->plan.comb_signed == pk->Z->plan.comb_signed &&
             (pk->Z->plan.comb || (ms[i]->plan.shared && ms[i]->plan.bits[0] == pk->Z->plan.bits[0]));
    if (same) {
      if ((rc = msm_horner_run(ctx, q3, 4, ms, ws, os, Bp))) return rc;
    } else {
      for (int i = 0; i < 4; i++)
        if ((rc = msm_horner_run(ctx, q3, 1, ms + i, ws + i, os + i, Bp))) return rc;
    }
  }
  if (pk->B2->plan.shared || pk->B2->plan.comb) {
    void* ws[1] = {v.w2};
    void* os[1] = {v.sB2};
    const zkmi_msm_bases* ms[1] = {pk->B2};
    if ((rc = msm_horner_run(ctx, q3, 1, ms, ws, os, Bp))) return rc;
  }
  PkConsts pc{pk->alpha, pk->beta1, pk->beta2};
  hipLaunchKernelGGL(assemble_kernel, dim3((unsigned)(Bp / 64)), dim3(64), 0, q3, v.sA, v.sB1, v.sK,
                     v.sZ, v.tR, v.tS, v.tNRS, (const Fr*)S.rs, Bp, pc, v.proofs);
  hipLaunchKernelGGL(assemble_g2_kernel, dim3((unsigned)(Bp / 64)), dim3(64), 0, q3, v.sB2, v.tS2,
                     Bp, pk->beta2, v.proofs);
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipMemcpyAsync(proofs_out, v.proofs, batch * 256, hipMemcpyDefault, q3));
  ZK_HIP(hipMemcpyAsync(status_out, S.st, batch * 4, hipMemcpyDefault, q3));
  if (const size_t nc = pk->commits.size()) {
    // per proof: Commitments[0 .. n-1], then CommitmentPok
    const size_t pitch = (nc + 1) * 64;
    for (size_t i = 0; i < nc; i++)
      ZK_HIP(hipMemcpy2DAsync((char*)commitments_out + i * 64, pitch,
                              (const char*)S.commit_pts + i * Bp * 64, 64, 64, batch, hipMemcpyDefault, q3));
    ZK_HIP(hipMemcpy2DAsync((char*)commitments_out + nc * 64, pitch,
                            (const char*)S.commit_pok + Bp * 128, 64, 64, batch, hipMemcpyDefault, q3));
  }
  hipEventRecord(S.eva[1], q3);
  // look ahead: queue the next batch's heavy kernels before blocking on this batch's assembly
  zkmi_ctx::ProveSet& N = ctx->sets[si ^ 1];
  if (N.pending && !N.heavy_enqueued && (rc = enqueue_heavy(ctx, si ^ 1))) return rc;
  // wait for THIS batch's copies only: the look-ahead has queued the next batch's multiples of
  // delta behind them on the same stream
  ZK_HIP(hipEventSynchronize(S.eva[1]));
  S.pending = false;
  S.heavy_enqueued = false;
  ctx->next_collect ^= 1;
  float ms = 0;
  hipEventElapsedTime(&ms, S.ev0, S.ev1);
  ctx->timings[0] = ms;
  for (int i = 0; i < 3; i++) {
    hipEventElapsedTime(&ms, S.evq[i], S.evq[i + 1]);
    ctx->timings[1 + i] = ms;
  }
  hipEventElapsedTime(&ms, S.eva[0], S.eva[1]);
  ctx->timings[4] = ms;
  hipEventElapsedTime(&ms, S.evq[0], S.evq[4]);
  ctx->timings[5] = ms;  // quotient + MSMs on the main stream (solve and assembly overlap neighbours)
  ctx->timings[6] = ctx->timings[7] = 0;
  for (int i = 0; i < S.msm_ev_used; i++) {
    hipEventElapsedTime(&ms, S.msm_ev[i][0], S.msm_ev[i][1]);
    ctx->timings[S.msm_ev_group[i] == 1 ? 6 : 7] += ms;
  }
  return ZKMI_OK;
}

int zkmi_prove_batch(zkmi_ctx* ctx, const zkmi_pk* pk, const zkmi_cs* cs, const void* inputs,
                     size_t batch, const void* rs, void* proofs_out, int32_t* status_out) {
  if (batch == 0) return ZKMI_OK;
  int rc;
  if ((rc = require_idle(ctx)) || (rc = zkmi_prove_submit(ctx, pk, cs, inputs, batch, rs))) return rc;
  return zkmi_prove_collect(ctx, proofs_out, status_out);
}

int zkmi_last_timings(zkmi_ctx* ctx, double* ms_out) {
  for (int i = 0; i < 8; i++) ms_out[i] = ctx->timings[i];
  return ZKMI_OK;
}

}  // extern "C"
