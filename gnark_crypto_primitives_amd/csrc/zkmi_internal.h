// Internal declarations shared by the HIP translation units of libzkmi.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/zkmi.h"
#include "ec.h"
#include "vprog.h"   // the witness program format: opcodes, classes, loader checks

namespace zk {

// Device layout used everywhere on the hot path: "batch-inner".  A logical matrix of field
// elements [row][proof] is stored with the proof index fastest, so that the 64 lanes of a
// wavefront work on 64 different proofs at the same row: loads/stores are 2 KiB contiguous per
// wave, and everything indexed by row (twiddles, constants, window-table slices, program words)
// is wave-uniform and comes through the scalar unit.  Bp = batch rounded up to 64.
// Within a row the two 16-byte halves of the elements are stored as two planes
// ([row][half][proof]): a lane's 32-byte element is then two dwordx4 accesses that are each
// perfectly coalesced across the wave (1 KiB contiguous).  With the halves interleaved
// ([row][proof][half]) every vector store wrote 16 of each 32 bytes and rocprofv3 showed 3x read /
// 6x write amplification on the NTT passes (profiles/r01_pmc_*.csv).

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

// Constants of the domain of size n = 2^log_n (w its generator, g = 5 the coset shift), built by
// get_plan and freed by free_plan (ntt.hip).  Each is named with the kernel argument it feeds.
struct NttPlan {
  int log_n = 0;
  // gnark's image (x * 2^256, ff.h).  Device tables:
  Fr* tw_fwd = nullptr;     // w^i, i < n/2: `tw` of the ff.h passes, forward
  Fr* tw_inv = nullptr;     // w^-i, i < n/2: `tw`, inverse
  Fr* coset_fwd = nullptr;  // g^i, i < n: `pre` of a forward coset transform on the ff.h passes
  Fr* coset_inv = nullptr;  // g^-i / n, i < n: `post` of inverse coset transform, ff.h and 29-bit
  Fr* coset_inv_den = nullptr;  // g^-i / (n (g^n - 1)): `post` of the quotient's final transform
  // and factors passed by value:
  Fr n_inv;                 // 1/n: `post_uniform` of an inverse transform, ff.h and 29-bit
  Fr den;                   // 1/(g^n - 1): `den` of pointwise_h_kernel
  Fr ninv_den;              // den / n: `post_uniform` of the quotient's transform of c
  // The F domain (x * 2^261, canonical, packed 8 x u32: ff29.h).  Device tables:
  Fr* tw29_fwd = nullptr;      // w^i: `tw` of the 29-bit passes, forward half of a fused pass
  Fr* tw29_inv = nullptr;      // w^-i: `tw` of the 29-bit passes, inverse half of a fused pass
  Fr* coset29_fwd = nullptr;   // g^i: `pre` of a forward coset transform on the 29-bit passes
  Fr* coset29n_fwd = nullptr;  // g^i / n: `factor` of the fused pass inverse -> coset forward
};

}  // namespace zk

struct zkmi_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  std::vector<zk::NttPlan> plans;
  hipEvent_t ev[8] = {};
  double timings[8] = {};
  // HBM working set shared by both pipeline sets, grown on demand (ensure_scratch), freed in
  // zkmi_destroy.  These run on the main stream only, so consecutive batches queue up behind
  // each other:
  zk::DevBuf ntt_tmp;                // NTT temporary of the quotient
  zk::DevBuf ntt_top;                // limb-8 planes of the 29-bit transform chains (ntt.hip)
  zk::DevBuf build_tmp;              // table-build inversion scratch; proof-of-knowledge temporary
  zk::DevBuf msm_digits, msm_sint;   // MSM digits, converted scalars (comb_scalars_kernel)
  zk::DevBuf msm_rowvar;             // which value-file rows vary over the batch (enqueue_heavy)
  // MSM chunk partials and what else an MSM's tail reads (msm_part_layout.h); [1] only for
  // deferred tails (part_ev)
  zk::DevBuf msm_part[2];
  // Side bases (zkmi_msm_bases::side) run while the main stream may be running an MSM on
  // msm_part[0], so each side stream has its own partials:
  zk::DevBuf side_part2;             // stream2: commitment MSMs of a submit
  zk::DevBuf side_part3;             // stream3: multiples of delta beside the assembly
  // software pipeline over batches: the latency-bound witness solve of batch k+1 runs on
  // `stream2` (16 wavefronts at batch 1024) underneath the NTT/MSM kernels of batch k.
  // `stream3` runs the 16-wavefront assembly of batch k underneath the quotient kernels of batch k+1.
  // `stream4` runs the tail of every proving-key MSM (common sums, sums over the chunk partials)
  // beside the next MSM's kernels.  It is a stream of its own because the tail of batch k+1's
  // first MSMs must not queue behind batch k's assembly on stream3: the main stream waits for it
  // (part_ev) before it reuses a partial-sum buffer.
  hipStream_t stream2 = nullptr, stream3 = nullptr, stream4 = nullptr;
  struct ProveSet {
    bool pending = false;
    bool heavy_enqueued = false;   // quotient + MSMs of this batch are already on the main stream
    // Buffers owned by the set, sized by prove_set_begin (set 0's are also borrowed by the
    // standalone entry points, see require_idle); a pending set's are never regrown.
    // misc = r/s, status and staged inputs; sums = MSM results, delta multiples, window sums,
    // assembled proofs (SumsView); commit = commitment buffers (commit.hip)
    zk::DevBuf slots, a, b, c, misc, sums, commit;
    hipEvent_t evq[5] = {};        // main stream: start, after NTTs, after G1 MSMs, after G2, done
    hipEvent_t eva[2] = {};        // stream3: assembly start / end
    hipEvent_t tail_ev = nullptr;  // stream4: the window sums of all five MSMs are complete
    hipEvent_t msm_ev[8][2] = {};  // around every proving-key msm_accumulate launch
    int msm_ev_group[8] = {};
    int msm_ev_used = 0;
    size_t batch = 0, Bp = 0;
    const zkmi_pk* pk = nullptr;
    const zkmi_cs* cs = nullptr;      // null for zkmi_prove_witness_batch (solved by the caller)
    size_t n_constraints = 0;         // rows of a, b, c that hold data (the rest of the domain is 0)
    bool f_domain = true;             // value file and a, b, c in the solver's 2^261 domain
    void *rs = nullptr, *st = nullptr;        // r/s and status, carved from misc
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // solve start / end on stream2
    // commitment extension, carved from `commit`: Pedersen commitments of the batch
    // (n_commitments x Bp G1 affine) and the per-proof powers of the folding challenge
    // (n_commitments x Bp fr, in the value file's domain), written by the submit; proof of
    // knowledge (Bp XYZZ -> affine) by the collect
    void *commit_pts = nullptr, *commit_ch = nullptr, *commit_pok = nullptr, *commit_acc = nullptr;
    std::vector<zk::Fr> commit_host;   // commitment wire values (plain integers), n x batch
  } sets[2];
  int next_submit = 0, next_collect = 0;
  // set whose proving-key MSM launches are currently being bracketed with HIP events (or null)
  int msm_ev_set = -1;
  // deferred MSM tails (msm_run with a finish stream): the chunk partials of consecutive MSMs
  // alternate between two buffers; part_ev[k] = last reduction that read buffer k has finished
  // (recorded on the finish stream), acc_ev[k] = last accumulate that wrote it (main stream),
  // dig_ev[k] = the split and digit kernels that wrote its lists and lane-0 digits (main stream)
  hipEvent_t part_ev[2] = {}, acc_ev[2] = {}, dig_ev[2] = {};
  bool part_ev_valid[2] = {false, false};
  unsigned part_next = 0;
  // witness entry (witness.hip): ring of three pinned host chunks + three device chunks through
  // which proof-major host arrays stream in (done[i]: the transpose that consumed chunk i)
  struct StageRing {
    void* pinned[3] = {};
    void* dev[3] = {};
    hipEvent_t done[3] = {};
    bool busy[3] = {false, false, false};
    size_t bytes = 0;
    unsigned next = 0;
  } ring;
  int copy_threads = 0;   // host threads that fill a pinned chunk from pageable memory; 0 = 4
  int solve_waves = 0;    // wavefronts per workgroup of solve_vliw_kernel; 0 = the default (solve.hip)
};

// Window plan of a fixed-base table: W windows whose sizes sum to exactly 255 bits (scalars are
// below 2^254, so the top window also absorbs the last signed-digit carry).  `rem` windows of
// (c0 + 1) bits come first, then W - rem windows of c0 bits.  Window j of base i holds the
// 2^(bits_j - 1) positive multiples d * 2^(shift_j) * P_i at entry offset i*per_base + off_j.
struct WinPlan {
  int W = 0;
  uint32_t per_base = 0;   // table entries per base
  uint8_t bits[64] = {};
  uint32_t off[64] = {};
  // shared = 1: ONE table d * P_i, d = 1..2^(c-1), serves every window (off[j] = 0); the windows
  // are accumulated separately and combined with Horner's rule at the end (msm.hip)
  uint8_t shared = 0;
  // comb = k > 0: joint table over groups of k consecutive bases, T[g][m] = sum_{i in m} P_{gk+i}
  // for every non-empty subset m (2^k entries, entry 0 unused), 254 one-bit windows: 254 / k mixed
  // additions per (base, proof).  W = 254; bits/off are not used.
  uint8_t comb = 0;
  // comb_signed: the comb table holds sign patterns, entry e = P_(k-1) + sum_{i<k-1} +-P_i
  // (2^(k-1) entries per group); W = 255: window 254 is the parity correction (msm.hip)
  uint8_t comb_signed = 0;
};

struct zkmi_msm_bases {
  int group = 1;        // 1 = G1, 2 = G2
  size_t n = 0;         // number of bases
  WinPlan plan;
  // affine entries in the 2^261 domain.  Per-window plan: d * 2^(shift_j) * P_i at
  // i * per_base + off_j + (d - 1); shared: d * P_i at i * per_base + (d - 1); comb: entry m of
  // group g at g * 2^k + m (2^(k-1) for sign-pattern tables)
  void* table = nullptr;
  size_t table_bytes = 0;
  uint8_t* inf = nullptr;  // device, n flags: base i is the point at infinity (skipped)
  size_t n_groups = 0;     // comb plans: ceil(n / k)
  int entries_may_be_inf = 0;  // comb plans: some subset of a group sums to the identity
  uint32_t chunk_factor = 0;   // (window, chunk) blocks in flight / wave slots; 0 = default
  // signed comb tables: the scalar image the table is native to (MSM_IMAGE_*: its bases were
  // scaled so that the digit pass reads scalars of that image as they are), and the sum of all
  // scaled bases (G1 / G2 by `group`)
  int image = 0;
  zk::G1Affine stotal1 = {};
  zk::G2Affine stotal2 = {};
  // side = 1: per-window plan run on the second stream (commitment MSMs of a submit, beside the
  // previous batch's MSMs on the main stream): its own partial-sum scratch, no deferred tails.
  // side = 2: the same for the one-base tables of delta, run on the assembly stream
  int side = 0;
};

// one commitment of a key (zkmi_commitment_desc on the device)
struct zkmi_commit_key {
  uint32_t n_private = 0, n_hashed = 0, wire = 0;
  std::vector<uint32_t> hashed;     // host copy (rows read back for the hash)
  std::vector<uint32_t> priv;       // host copy (zkmi_prove_r1cs_submit compares it with the solver's)
  uint32_t* private_dev = nullptr;  // device: wire index of every basis point
  zkmi_msm_bases* basis = nullptr;  // side tables
  zkmi_msm_bases* sigma = nullptr;  // main-stream tables (proof of knowledge)
};

struct zkmi_pk {
  uint32_t log_n = 0, n_wires = 0, n_a = 0, n_b = 0, n_k = 0, n_z = 0, max_batch = 1024;
  uint32_t *a_wire = nullptr, *b_wire = nullptr, *k_wire = nullptr;  // device
  zkmi_msm_bases *A = nullptr, *B1 = nullptr, *K = nullptr, *Z = nullptr, *B2 = nullptr;
  zkmi_msm_bases *D1 = nullptr, *D2 = nullptr;  // one-base tables of delta (G1, G2)
  uint32_t* idx3 = nullptr;                      // device {0, 1, 2}
  zk::G1Affine alpha, beta1, delta1;
  zk::G2Affine beta2, delta2;
  std::vector<zkmi_commit_key> commits;   // commitment extension (empty for a plain key)
  // quotient in evaluation form (quotient_fold.h): Z holds E (n bases, n_z = n), K the bases with
  // the c term folded in (n_k counts the appended ones); the prover runs compute_ab_coset_bi
  bool folded = false;
  uint32_t fold_n_constraints = 0;   // rows of the O that was folded in
};

struct zkmi_cs {
  uint32_t n_wires = 0, n_public = 0, n_secret = 0, n_constraints = 0, n_slots = 0, n_rows = 0,
           n_consts = 0, lanes_per_proof = 1;
  uint32_t* program = nullptr;  // device
  zk::Fr* consts = nullptr;     // device
  // COMMIT rows of the program in order: (row index, commitment index); the solver kernel is
  // launched once per segment between them
  std::vector<std::pair<uint32_t, uint32_t>> commit_rows;
  // the program holds OP_EMUL units (std/math/emulated product hints): the solver variant with the
  // big-integer division arm is launched
  bool has_emul = false;
};

// the R1CS matrices of zkmi_r1cs_load (witness.hip)
struct zkmi_r1cs {
  uint32_t n_wires = 0, n_constraints = 0, n_coeffs = 0;
  uint32_t* ptr[3] = {};   // device, n_constraints + 1 offsets each (L, R, O)
  uint2* terms[3] = {};    // device, x = wire, y = coefficient index | kind << 30
  size_t nnz[3] = {};
  zk::Fr* coeffs = nullptr;   // device, 2^261 images (gnark's Montgomery image times 2^5: fmulp)
};

// the sparse constraint system of zkmi_scs_load (plonk.hip; checks: scs_check.h)
struct zkmi_scs {
  uint32_t n_wires = 0, n_gates = 0, n_public = 0;
  uint32_t* x[3] = {};         // device, n_gates wire indices each: columns a, b, c
  uint32_t* marks = nullptr;   // device, n_gates words: scs_check.h marks of the five selectors
  zk::Fr* sel = nullptr;       // device, 5 x n_gates: qL qR qO qM as 2^261 images, qC as loaded
  std::vector<uint32_t> hx[3]; // host copies, for the wiring check against a key's permutation
  mutable uint64_t checked_key = 0;   // serial of the trace-loaded key the wiring was last checked against
};

namespace zk {

#if defined(__HIPCC__)
// element (row, b) of a batch-inner matrix with row pitch Bp
__device__ __forceinline__ Fr bi_ld(const Fr* base, size_t row, size_t b, size_t Bp) {
  const uint4* p = reinterpret_cast<const uint4*>(base) + row * 2 * Bp + b;
  const uint4 lo = p[0], hi = p[Bp];
  Fr r;
  r.v[0] = lo.x; r.v[1] = lo.y; r.v[2] = lo.z; r.v[3] = lo.w;
  r.v[4] = hi.x; r.v[5] = hi.y; r.v[6] = hi.z; r.v[7] = hi.w;
  return r;
}
__device__ __forceinline__ void bi_st(Fr* base, size_t row, size_t b, size_t Bp, const Fr& x) {
  uint4* p = reinterpret_cast<uint4*>(base) + row * 2 * Bp + b;
  p[0] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
  p[Bp] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
}
// write-once streams (the solver's a, b, c rows): non-temporal, so that they do not evict the MSM
// table lines the kernels running beside the solve are hitting in L2 / Infinity Cache
__device__ __forceinline__ void bi_st_nt(Fr* base, size_t row, size_t b, size_t Bp, const Fr& x) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  u32x4* p = reinterpret_cast<u32x4*>(base) + row * 2 * Bp + b;
  u32x4 lo = {x.v[0], x.v[1], x.v[2], x.v[3]}, hi = {x.v[4], x.v[5], x.v[6], x.v[7]};
  __builtin_nontemporal_store(lo, p);
  __builtin_nontemporal_store(hi, p + Bp);
}
#endif

#define ZK_HIP(call)                                                         \
  do {                                                                       \
    hipError_t _e = (call);                                                  \
    if (_e != hipSuccess) {                                                  \
      ctx->err = std::string(#call) + ": " + hipGetErrorString(_e);          \
      return ZKMI_ERR_HIP;                                                   \
    }                                                                        \
  } while (0)

static inline size_t round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }

// waits for everything queued on the context's side streams (stream2, stream3, stream4)
void sync_side_streams(zkmi_ctx* ctx);
// grows `buf` to at least `bytes` (synchronising the context's streams first if it held memory)
int ensure_scratch(zkmi_ctx* ctx, DevBuf& buf, size_t bytes, void** out = nullptr);
// ZKMI_OK when no Groth16 batch is in flight, else ZKMI_ERR_ARG with ctx->err set
int require_idle(zkmi_ctx* ctx);
// where a caller's pointer lives (hipPointerGetAttributes)
enum { PTR_PAGEABLE = 0, PTR_PINNED = 1, PTR_DEVICE = 2 };
int pointer_kind(const void* p);
void witness_ring_free(zkmi_ctx* ctx);
// witness.hip: one proof-major caller array [batch][rows] of fr (pageable, page-locked or device
// memory) -> batch-inner rows of `dst` on ctx->stream, host memory through the context's pinned ring.
// Pageable memory has been consumed on return; the rest when the stream has passed the copies.
int stage_rows(zkmi_ctx* ctx, const void* src, size_t rows, size_t batch, size_t Bp, void* dst);
// scs_solve.hip: the solver's own copy of its system and its inputs per proof; the solve of a batch on
// ctx->stream: the caller's inputs (proof-major, host or device) through `staged` [n_inputs][Bp] to
// their wires in `w` [n_wires][Bp], then every other wire; status[p] is written for a proof that
// divides by zero and left alone otherwise
const zkmi_scs* scs_solver_system(const zkmi_scs_solver* s);
uint32_t scs_solver_inputs(const zkmi_scs_solver* s);
int scs_solver_run(zkmi_ctx* ctx, const zkmi_scs_solver* s, const void* inputs, size_t batch, size_t Bp,
                   Fr* staged, Fr* w, int32_t* status);
// The same in pieces, for a plan with commitment hints (ZKMI_HINTS_STD; scs_plan.h): the inputs, then
// the steps [begin, end) between the boundaries.  Commitment hint i: the first step of its barrier
// level, its wire, its committed wires in operand order on the host and on the device.
struct ScsSolverCommit {
  uint32_t step, wire, n_wires;
  const uint32_t *wires, *wires_dev;
};
uint32_t scs_solver_steps(const zkmi_scs_solver* s);
size_t scs_solver_commits(const zkmi_scs_solver* s);
ScsSolverCommit scs_solver_commit(const zkmi_scs_solver* s, size_t i);
int scs_solver_stage(zkmi_ctx* ctx, const zkmi_scs_solver* s, const void* inputs, size_t batch, size_t Bp,
                     Fr* staged, Fr* w);
int scs_solver_run_steps(zkmi_ctx* ctx, const zkmi_scs_solver* s, Fr* w, int32_t* status, size_t Bp,
                         uint32_t begin, uint32_t end);

// The loaders of the two gnark-shaped solvers (r1cs_solve.hip, scs_solve.hip): n elements of a caller
// array (host or device) into a host vector, and into device memory of their own; false: the copy or
// the allocation failed (the sticky error is cleared)
template <class T>
static bool fetch(std::vector<T>& dst, const void* src, size_t n) {
  dst.resize(n);
  if (n == 0) return true;
  if (!src || hipMemcpy(dst.data(), src, n * sizeof(T), hipMemcpyDefault) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return true;
}
template <class T>
static bool upload(T** dst, const void* src, size_t n) {
  if (hipMalloc((void**)dst, (n ? n : 1) * sizeof(T)) != hipSuccess ||
      (n && hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyDefault) != hipSuccess)) {
    (void)hipGetLastError();
    return false;
  }
  return true;
}

// The solvers' kernels are templates in the number of lanes per proof: f(std::integral_constant<int, S>())
// for S in {1, 2, 4, 8, 16, 32, 64}; false, and f not called, for any other S
template <class F>
static bool with_lanes(uint32_t S, F&& f) {
  switch (S) {
    case 1: f(std::integral_constant<int, 1>()); return true;
    case 2: f(std::integral_constant<int, 2>()); return true;
    case 4: f(std::integral_constant<int, 4>()); return true;
    case 8: f(std::integral_constant<int, 8>()); return true;
    case 16: f(std::integral_constant<int, 16>()); return true;
    case 32: f(std::integral_constant<int, 32>()); return true;
    case 64: f(std::integral_constant<int, 64>()); return true;
    default: return false;
  }
}

// RAII staging of a caller buffer (host or device) as device memory
struct Staged {
  zkmi_ctx* ctx;
  void* dev = nullptr;
  void* host = nullptr;  // non-null when a copy back is pending
  size_t bytes = 0;
  bool owned = false;
  Staged(zkmi_ctx* c) : ctx(c) {}
  int in(const void* p, size_t n) {
    bytes = n;
    if (n == 0) return ZKMI_OK;
    if (pointer_kind(p) == PTR_DEVICE) {
      dev = const_cast<void*>(p);
      return ZKMI_OK;
    }
    ZK_HIP(hipMalloc(&dev, n));
    owned = true;
    ZK_HIP(hipMemcpyAsync(dev, p, n, hipMemcpyHostToDevice, ctx->stream));
    return ZKMI_OK;
  }
  int out(void* p, size_t n) {
    bytes = n;
    if (n == 0) return ZKMI_OK;
    if (pointer_kind(p) == PTR_DEVICE) {
      dev = p;
      return ZKMI_OK;
    }
    ZK_HIP(hipMalloc(&dev, n));
    owned = true;
    host = p;
    return ZKMI_OK;
  }
  int finish() {
    if (host && dev) {
      ZK_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
      ZK_HIP(hipStreamSynchronize(ctx->stream));
      host = nullptr;
    }
    return ZKMI_OK;
  }
  ~Staged() {
    if (owned && dev) {
      hipStreamSynchronize(ctx->stream);
      hipFree(dev);
    }
  }
};
// a caller array as device memory: used in place, or (host memory) copied into `stage` on
// ctx->stream
int device_view(zkmi_ctx* ctx, const void* src, size_t bytes, void* stage, const void** out);

// One Groth16 submit (zkmi_prove_submit, zkmi_prove_witness_submit) on set ctx->next_submit.
// prove_set_begin sizes that set and the idle one (value file of `value_rows`, `n_staged` input
// rows staged through misc), stages r/s, and switches ctx->stream to stream2 (saved in *main)
// after recording ev0; *stage = the set's staging area for host inputs.  On failure nothing is
// left switched.  prove_set_end(rc) records ev1 and restores the stream; the set becomes pending
// when rc == 0, otherwise stream2 is drained so that nothing queued still reads caller memory.
int prove_set_begin(zkmi_ctx* ctx, const zkmi_pk* pk, size_t value_rows, size_t n_staged,
                    size_t batch, const void* rs, hipStream_t* main, char** stage);
int prove_set_end(zkmi_ctx* ctx, hipStream_t main, int rc);

// layout conversion (proof-major <-> batch-inner), rows x batch elements of `elem_bytes`
int transpose_in(zkmi_ctx* ctx, const void* src_pm, void* dst_bi, size_t rows, size_t batch,
                 size_t Bp, size_t elem_bytes);
int transpose_out(zkmi_ctx* ctx, const void* src_bi, void* dst_pm, size_t rows, size_t batch,
                  size_t Bp, size_t elem_bytes);

// ntt.hip
int get_plan(zkmi_ctx* ctx, int log_n, NttPlan** out);
void free_plan(NttPlan& p);   // the plan's device tables
// src -> dst (distinct buffers), batch-inner [n][Bp]; rows >= n_valid of src are read as zero
int ntt_bi(zkmi_ctx* ctx, const NttPlan* plan, const Fr* src, Fr* dst, size_t Bp, bool inverse,
           bool coset, size_t n_valid);
// full quotient: a,b,c batch-inner [n][Bp] (rows >= n_valid zero) -> h in `a_out`; t0,t1 scratch
// abc_f: a, b, c are in the F domain (solver output); the result h is always in gnark's image
// top: three planes [n][Bp] of int32 for the limb form of a, b and t0 between the passes (ntt.hip,
// log_n >= 8); null = the context's own (ntt_top)
int compute_h_bi(zkmi_ctx* ctx, const NttPlan* plan, Fr* a, Fr* b, Fr* c, Fr* t0, size_t Bp,
                 size_t n_valid, Fr** h_out, bool abc_f = false, int32_t* top = nullptr);

// the quotient of a folded key: the n coset evaluations of a * b in gnark's image, or with out_f
// in the F domain (x * 2^261, canonical), *u_out = b
// (log_n >= 8; a, b, top as compute_h_bi's, both overwritten)
int compute_ab_coset_bi(zkmi_ctx* ctx, const NttPlan* plan, Fr* a, Fr* b, Fr* t0, size_t Bp,
                        size_t n_valid, Fr** u_out, bool abc_f = false, int32_t* top = nullptr,
                        bool out_f = false);

// quotient_fold.hip: what zkmi_pk_load puts in the place of g1_z, g1_k and k_wire when
// zkmi_pk_desc.fold_r1cs folds (host copies; the device buffers of the fold are gone on return)
struct FoldedKey {
  bool folded = false;
  std::vector<G1Affine> e, k;
  std::vector<uint32_t> k_wire;
};
// k_wire: the key's K wires on the host.  ZKMI_ERR_ARG for a malformed fold_r1cs; folded stays
// false, with ZKMI_OK, for a system or a key that the fold does not serve
int quotient_fold_key(zkmi_ctx* ctx, const zkmi_pk_desc* d, const std::vector<uint32_t>& k_wire,
                      FoldedKey* out);
// pts[0, n) = E, pts[n, 2n) = L from the first min(n_z, n - 1) points of z_dev (device arrays)
int quotient_bases_dev(zkmi_ctx* ctx, const NttPlan* plan, const G1Affine* z_dev, uint32_t n_z,
                       G1Affine* pts);

// msm.hip (the templates behind these are in msm_impl.h)
constexpr int COMB_W = 254;   // one-bit windows of a comb plan: scalars are below 2^254
// fewest varying groups that are worth a chunk of their own (msm_impl.h comb_eff_chunks)
constexpr uint32_t COMB_MIN_GROUPS_PER_CHUNK = 32;
// window plans: per-window tables (of W windows; of c-bit windows), one shared table of c-bit
// windows, comb tables over groups of k bases
WinPlan plan_with_windows(int W);
WinPlan plan_uniform(int c);
WinPlan plan_shared(int c);
WinPlan plan_comb(int k, bool signed_tables = true);
// smallest number of windows whose per-window tables for n_total bases fit `budget_bytes`
WinPlan plan_windows_for_budget(size_t n_total, int group, double budget_bytes);
// comb group sizes / shared-table widths of a key's G1 and G2 bases whose tables fit `usable_bytes`
void plan_comb_for_budget(size_t n1, size_t n2, double usable_bytes, int* k1, int* k2, bool* sg1,
                          bool* sg2, bool allow_signed = true);
void plan_shared_for_budget(size_t n1, size_t n2, double usable_bytes, int* c1, int* c2);
// image: the canonical image most scalars of this base set will arrive in, gnark's (x * 2^256) or
// the F domain (x * 2^261).  Only sign-pattern comb plans use it: their table is built over the
// bases times (2 * 2^256)^-1 resp. (2 * 2^261)^-1 mod r, so that the signs of every window are
// bits of the image itself (comb_sign.h) and scalars of that image need no pass of their own.
// Scalars of the other image still work (one conversion pass); every other plan needs the plain
// integer, in which small values stay small, and ignores `image`.
enum { MSM_IMAGE_STD = 0, MSM_IMAGE_F = 1 };
int msm_bases_build(zkmi_ctx* ctx, int group, const void* bases_dev, size_t n, const WinPlan& plan,
                    zkmi_msm_bases** out, int image = MSM_IMAGE_STD);
// scalars batch-inner: element (row, b) at scalars[row * Bp + b]; row_idx (device, may be null)
// maps base i to its scalar row.  out_xyzz: Bp accumulators.
// scalars_f: the scalars are in the F domain (solver output) instead of gnark's image
// batch = the lanes that hold real proofs (<= Bp): comb plans sum the groups whose scalars are the
// same in all of them once per batch; the results of the padding lanes are then unspecified.
// With wsum_out (shared-table and comb plans only) msm_run stops at the W window sums ([W][Bp] XYZZ)
// and the caller finishes with msm_horner_run -- 255 dependent doublings per proof, latency-bound,
// which the prover runs on its assembly stream under the next batch's kernels.  With finish_stream
// (comb plans; the prover passes stream4) the tail of the MSM runs there: the common sums of the
// uniform groups (ordered after the digit pass by an event) and the sums over the chunk partials
// (ordered after the accumulate launch by another; the partials of consecutive MSMs alternate
// between two buffers), so the main stream holds nothing but the split, the digit pass and the
// accumulate kernel.
// Comb plans, which groups are uniform: row_varies (device, may be null) = msm_rows_vary's flags
// of the rows of `scalars`, shared by every MSM that reads the same rows; dense = do not look,
// every group varies (scalars with no structure, such as the quotient's).  With neither, msm_run
// compares the rows of its own bases.
int msm_run(zkmi_ctx* ctx, const zkmi_msm_bases* bases, const Fr* scalars, const uint32_t* row_idx,
            size_t Bp, size_t batch, void* out_xyzz, bool scalars_f = false,
            void* wsum_out = nullptr, hipStream_t finish_stream = nullptr,
            const uint8_t* row_varies = nullptr, bool dense = false);
// flags[row] = 1 when row `row` of the batch-inner matrix differs between two of its first `batch`
// lanes, else 0 (n_rows flags, device)
int msm_rows_vary(zkmi_ctx* ctx, const Fr* rows, size_t n_rows, size_t Bp, size_t batch,
                  uint8_t* flags);
// Horner step of up to four deferred MSMs of one group (same plan) in one launch on `stream`
int msm_horner_run(zkmi_ctx* ctx, hipStream_t stream, int count,
                   const zkmi_msm_bases* const* bases, void* const* wsums, void* const* outs,
                   size_t Bp);
// XYZZ -> affine, n points of `group`
int xyzz_to_affine(zkmi_ctx* ctx, int group, const void* in, void* out, size_t n);

// solve.hip
// slots [n_slots][Bp] with rows 0..n_inputs pre-filled; writes every wire row, a/b/c rows
// [0, n_constraints) and status[Bp] (0 or ZKMI_ERR_UNSATISFIED)
// The solver's value file and its a/b/c outputs are in the F domain (x * 2^261, see solve.hip);
// inputs must be converted with rows_to_f_domain after staging.
int solve_bi(zkmi_ctx* ctx, const zkmi_cs* cs, Fr* slots, Fr* a, Fr* b, Fr* c, int32_t* status,
             size_t Bp);
// the two halves of solve_bi for programs with COMMIT rows: initialise ONE row and status, then run
// program rows [row_begin, row_end)
int solve_init(zkmi_ctx* ctx, Fr* slots, int32_t* status, size_t Bp);
int solve_rows(zkmi_ctx* ctx, const zkmi_cs* cs, Fr* slots, Fr* a, Fr* b, Fr* c, int32_t* status,
               size_t Bp, uint32_t row_begin, uint32_t row_end);

// commit.hip: commitment extension of the prover
// bytes of a set's commitment buffers for a key with n_commitments (0 for a plain key)
size_t commit_buffer_bytes(size_t n_commitments, size_t Bp);
// the commitments of set S at a COMMIT row of the solver path (or all of them, witness path):
// MSM over the key's basis from the value file, hash_to_field on the host, challenge into the wire
int commit_phase(zkmi_ctx* ctx, zkmi_ctx::ProveSet& S, uint32_t index, bool write_wire);
// folding challenge powers for the proof of knowledge (after the last commit_phase)
int commit_finish_submit(zkmi_ctx* ctx, zkmi_ctx::ProveSet& S);
// proof of knowledge on ctx->stream (main stream, enqueue_heavy)
int commit_pok(zkmi_ctx* ctx, zkmi_ctx::ProveSet& S);
// host: G1Affine.Marshal() (64 bytes) and fr.Hash(msg, dst, 1)[0] in gnark's image, shared with the
// PLONK commitments (plonk.hip)
void g1_marshal(uint8_t out[64], const G1Affine& d);
Fr hash_to_fr_dst(const uint8_t* msg, size_t len, const char* dst);
int commit_keys_load(zkmi_ctx* ctx, const zkmi_pk_desc* d, zkmi_pk* pk);
void commit_keys_free(zkmi_ctx* ctx, zkmi_pk* pk);
int rows_to_f_domain(zkmi_ctx* ctx, Fr* base, size_t rows, size_t Bp);
int rows_to_std_domain(zkmi_ctx* ctx, Fr* base, size_t rows, size_t Bp);
int array_to_f_domain(zkmi_ctx* ctx, Fr* a, size_t n);

}  // namespace zk
