/* zkmi.h -- C-ABI of the MI355X-native Groth16/BN254 prover hot path (libzkmi.so).
 *
 * The reference (vocdoni/gnark-crypto-primitives) has no FFI boundary of its own: its circuits
 * reach the prover only through gnark (go.mod:8-9) from test call sites such as
 * tree/test/verifier_bn254_test.go:41 (frontend.Compile) and :67 (assert.SolvingSucceeded ->
 * solver; groth16.Prove under the prover_checks build tag).  Each entry point below names the
 * gnark / gnark-crypto interface it stands in for [UPSTREAM-RECALL, SURVEY.md §3.2, §8b]; the cgo
 * stub a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions (chosen so a cgo caller passes unsafe.Pointer(&slice[0]) with zero copies):
 *   - fr.Element / fp.Element: 4 x uint64 little-endian limbs, Montgomery form, R = 2^256.
 *   - G1Affine = {X, Y} 64 B; G2Affine = {X.A0, X.A1, Y.A0, Y.A1} 128 B; infinity = all zero.
 *   - Every pointer argument may be a host pointer or a HIP device pointer (detected with
 *     hipPointerGetAttributes); device pointers avoid the PCIe copy.
 *   - "batch" arrays are proof-major: element (proof p, index i) at [p * stride + i].
 *   - All functions return 0 on success or a negative zkmi_status; they never abort.  A context
 *     is thread-compatible (one caller at a time); distinct contexts are independent.
 */
#ifndef ZKMI_H
#define ZKMI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zkmi_ctx zkmi_ctx;
typedef struct zkmi_pk zkmi_pk;
typedef struct zkmi_cs zkmi_cs;
typedef struct zkmi_r1cs_desc zkmi_r1cs_desc; /* defined with zkmi_r1cs_load below */

enum zkmi_status {
  ZKMI_OK = 0,
  ZKMI_ERR_ARG = -1,
  ZKMI_ERR_HIP = -2,
  ZKMI_ERR_NO_DEVICE = -3,
  ZKMI_ERR_OOM = -4,
  ZKMI_ERR_UNSATISFIED = -5 /* at least one proof's witness does not satisfy the system */
};

/* -- context ----------------------------------------------------------------------------- */
/* Selects HIP device `device`, creates the streams and the NTT twiddle cache.  Fails with
 * ZKMI_ERR_NO_DEVICE when no gfx950 device is visible: there is no CPU fallback. */
int zkmi_init(int device, zkmi_ctx** out);
void zkmi_destroy(zkmi_ctx* ctx);
const char* zkmi_last_error(zkmi_ctx* ctx);
/* Blocks until all work queued on the context's stream has finished. */
int zkmi_sync(zkmi_ctx* ctx);
/* HIP stream (hipStream_t) the context launches on -- for callers that time with HIP events. */
void* zkmi_stream(zkmi_ctx* ctx);

/* -- field / group primitives (parity tests; a Go shim that keeps gnark's own solver) ------- */
/* r[i] = a[i] * b[i] in fr (which = 0) or fp (which = 1).   stands in for fr.Element.Mul / fp.Element.Mul */
int zkmi_field_mul(zkmi_ctx* ctx, int which, const void* a, const void* b, void* r, size_t n);
/* Parity hook for the 9 x 29-bit field forms every hot kernel multiplies with (csrc/ff29.h and the
 * generated csrc/ff29_asm.h; tests/test_gpu_primitives.py::test_ff29_asm_products).  One lane per
 * element applies form `op` of `field` (0 = fr, 1 = fq) to raw signed limbs, which are neither
 * unpacked nor normalised on the way in:
 *   in  [n][arity][9] int32, out [n][9] int32; n = 0 is a no-op, n need not be a multiple of 64;
 *   op 0 mul_asm (a, b)   1 sqr_asm (a)   2 mul_add2_asm (a, b, c, d: a b + c d)   3 mul_asm_s (a, b)
 *      4 mul   5 sqr   6 mul_add2   7 mul_ilp      -- the C++ forms, compiled for the device
 *      8 pack_canonical(wred(a))   9 pack_canonical(a)   -- 8 packed words in out[0..7], out[8] = 0
 *   mul_asm_s takes a wave-uniform b: element i uses the b operand of element 64 * (i / 64), loaded
 *   through a wave-uniform index so that it reaches the asm in SGPRs, as the NTT's twiddles do; the
 *   b operands of the other elements are read by nobody.
 * An unknown field or op returns ZKMI_ERR_ARG. */
int zkmi_ff29_op(zkmi_ctx* ctx, int field, int op, const int32_t* in, int32_t* out, size_t n);
/* Throughput microbenchmark: every lane runs `iters` dependent Montgomery products; returns
 * products per second in *rate (integer-ALU roofline measurement).  which: 0 = fr,
 * 1 = fp (8 x 32-bit limbs, ff.h), 2 = fp in the 9 x 29-bit form the G1 MSM uses (ff29.h). */
int zkmi_field_mul_bench(zkmi_ctx* ctx, int which, size_t n_threads, int iters, double* rate);

/* Batched NTT over fr, natural order in and out, in place.  stands in for
 * fft.Domain.FFT / FFTInverse (gnark-crypto ecc/bn254/fr/fft) with fft.OnCoset() = `coset`.
 *   data: batch x 2^log_n fr elements, proof-major. */
int zkmi_ntt_batch(zkmi_ctx* ctx, void* data, int log_n, size_t batch, int inverse, int coset);

/* h = coefficients of (A.B - C)/Z_H.   stands in for computeH in gnark
 * backend/groth16/bn254/prove.go.  a, b, c: batch x 2^log_n evaluations (zero padded);
 * h_out: batch x 2^log_n coefficients, natural order. */
int zkmi_h_batch(zkmi_ctx* ctx, const void* a, const void* b, const void* c, void* h_out,
                 int log_n, size_t batch);
/* Parity hooks of the quotient in evaluation form (zkmi_pk_desc.fold_r1cs), conventions of
 * zkmi_h_batch.  out: batch x 2^log_n, the evaluations of a.b on the coset 5<w>, natural order:
 * coset FFT of the inverse FFT of a, times the same of b (log_n >= 8). */
int zkmi_ab_coset_batch(zkmi_ctx* ctx, const void* a, const void* b, void* out, int log_n,
                        size_t batch);
/* The bases that a folded key puts in the place of pk.G1.Z, from the first 2^log_n - 1 points of
 * g1_z (n_z >= 2^log_n - 1; Z_(n-1) = infinity), n = 2^log_n affine points each, on the host:
 *   e_out[i] = den / n . sum_k 5^-k w^-ik Z_k,  l_out[i] = 1 / n . sum_k w^-ik Z_k,
 *   den = 1 / (5^n - 1). */
int zkmi_quotient_bases(zkmi_ctx* ctx, const void* g1_z, size_t n_z, int log_n, void* e_out,
                        void* l_out);

/* Fixed-base MSM handle: bases are uploaded once and expanded into HBM-resident tables of signed
 * window multiples.  group: 1 = G1, 2 = G2.
 *   window_bits = 0: widest windows the free HBM allows, ONE table d*P (d = 1..2^(c-1)) per base
 *                    shared by all windows, per-window accumulators combined by Horner's rule;
 *   100 + c (c in 4..16): that layout with an explicit width;
 *   c in 2..16: the per-window layout (a table d*2^(c*j)*P for every window j, one accumulator);
 *   200 + k (k in 2..20): comb tables -- one joint table of all subset sums per group of k bases,
 *                    254 one-bit windows (254 / k additions per base and proof);
 *   300 + k (k in 3..21): sign-pattern comb tables -- every scalar rewritten as a sum of 254 signed
 *                    powers of two, one entry P_(k-1) + sum_{i<k-1} +-P_i per sign pattern
 *                    (2^(k-1) entries serve k bases: one more base per group than 200 + k in the
 *                    same HBM, but no digit is ever "nothing to add"), 255 windows (254 + a parity
 *                    correction).  The auto plan's choice for dense witnesses (the Arbo-160 key:
 *                    319 for G1).
 *   Auto picks the layout with the fewest additions that fits. */
typedef struct zkmi_msm_bases zkmi_msm_bases;
int zkmi_msm_bases_load(zkmi_ctx* ctx, int group, const void* bases, size_t n, int window_bits,
                        zkmi_msm_bases** out);
void zkmi_msm_bases_free(zkmi_ctx* ctx, zkmi_msm_bases* b);
/* out[p] = sum_i scalars[p][i] * bases[i].   stands in for G1Jac/G2Jac.MultiExp (gnark-crypto
 * ecc/bn254/multiexp.go) called once per proof with the same bases.
 *   scalars: batch x n fr elements (Montgomery), proof-major; out: batch affine points. */
int zkmi_msm_batch(zkmi_ctx* ctx, const zkmi_msm_bases* bases, const void* scalars, size_t batch,
                   void* out);
/* The two calls above with the choices the prover makes inside spelled out (tests, tools).
 *   image: the canonical image the scalars are in, 0 = x * 2^256 (Montgomery, as everywhere in this
 *          header), 1 = x * 2^261 (the witness solver's).  A sign-pattern comb table is built native
 *          to the image given at the load and reads such scalars as they are; scalars of the other
 *          image cost one conversion pass.  Every combination gives the same points.
 *   scalars: batch x n_rows fr elements, proof-major; base i takes row row_idx[i] (n entries, each
 *          below n_rows; NULL: row i).
 *   uniform: how comb plans find the groups whose scalars the whole batch shares: 0 = from the
 *          rows of the bases, inside the MSM; 1 = from one pass over all n_rows rows before it;
 *          2 = not at all (every group is summed per proof). */
int zkmi_msm_bases_load_image(zkmi_ctx* ctx, int group, const void* bases, size_t n,
                              int window_bits, int image, zkmi_msm_bases** out);
int zkmi_msm_batch_rows(zkmi_ctx* ctx, const zkmi_msm_bases* bases, const void* scalars,
                        size_t n_rows, const uint32_t* row_idx, size_t batch, int image, int uniform,
                        void* out);
/* Comb tables: fewest groups with batch-varying scalars that are worth a chunk (a row of
 * accumulate blocks and a partial sum of its own) in one MSM launch. */
uint32_t zkmi_comb_min_groups_per_chunk(void);
/* out[i] = scalars[i] * base.   stands in for curve.BatchScalarMultiplicationG1/G2 used by
 * groth16.Setup (gnark backend/groth16/bn254/setup.go). */
int zkmi_fixed_base_mul(zkmi_ctx* ctx, int group, const void* base, const void* scalars, size_t n,
                        void* out);

/* -- proving key --------------------------------------------------------------------------- */
/* Mirrors gnark's groth16 bn254 ProvingKey: Domain, G1{Alpha,Beta,Delta,A,B,Z,K}, G2{Beta,Delta,B},
 * InfinityA / InfinityB [UPSTREAM-RECALL, SURVEY.md §3.2].  Which wire each retained base belongs
 * to can be given either way:
 *   - gnark's own fields: infinity_a / infinity_b (one byte per wire, Go []bool: 1 = the point is
 *     at infinity and absent from g1_a / g1_b / g2_b) with a_wire = b_wire = NULL, and n_public
 *     (pk.G1.K holds wires n_public .. n_wires-1 in order) with k_wire = NULL;
 *   - or explicit index arrays a_wire / b_wire / k_wire (what this repo's own setup emits).
 * n_a / n_b / n_k are always the lengths of g1_a / g1_b (= g2_b) / g1_k. */
/* One commitment of gnark's Groth16 commitment extension (api.Commit; std/rangecheck and the
 * lookup arguments build on it): constraint.Groth16Commitment {PrivateCommitted,
 * PublicAndCommitmentCommitted, CommitmentIndex} and pedersen.ProvingKey {Basis, BasisExpSigma} of
 * pk.CommitmentKeys[i] [UPSTREAM-RECALL, SURVEY.md §3.2 step 6].  The prover commits to the private
 * wires (MSM over basis), derives the commitment wire's value by hash_to_field over the commitment
 * and the hashed wires' values (RFC 9380 expand_message_xmd, SHA-256, DST "bsb22-commitment"), and
 * proves knowledge with the same scalars over basis_exp_sigma (folded over all commitments with
 * powers of Hash(commitment wire values, DST "G16-BSB22")). */
typedef struct {
  uint32_t n_private;            /* basis points = committed private wires */
  uint32_t n_hashed;             /* public wires / earlier commitment wires hashed with it */
  uint32_t commitment_wire;      /* wire that receives the challenge */
  uint32_t reserved;
  const uint32_t* private_wires; /* n_private wire indices, basis order */
  const uint32_t* hashed_wires;  /* n_hashed wire indices */
  const void* basis;             /* n_private G1 affine */
  const void* basis_exp_sigma;   /* n_private G1 affine */
} zkmi_commitment_desc;

typedef struct {
  uint32_t log_n;       /* domain size 2^log_n */
  uint32_t n_wires;     /* columns of the constraint system, including ONE */
  uint32_t n_a, n_b, n_k, n_z;
  const uint32_t* a_wire; /* n_a: wire index of g1_a[i] (InfinityA filtered out), or NULL */
  const uint32_t* b_wire; /* n_b: wire index of g1_b[i] and g2_b[i], or NULL */
  const uint32_t* k_wire; /* n_k: wire index of g1_k[i] (private wires), or NULL */
  const void* g1_a;
  const void* g1_b;
  const void* g1_k;
  const void* g1_z; /* n_z >= 2^log_n - 1 points; the first 2^log_n - 1 are used */
  const void* g2_b;
  const void* g1_alpha;
  const void* g1_beta;
  const void* g1_delta;
  const void* g2_beta;
  const void* g2_delta;
  uint32_t window_bits_g1; /* as zkmi_msm_bases_load: 0 = default */
  uint32_t window_bits_g2;
  /* gnark-shaped alternative to the index arrays (used when the matching *_wire is NULL) */
  const uint8_t* infinity_a; /* n_wires bytes */
  const uint8_t* infinity_b; /* n_wires bytes */
  uint32_t n_public;         /* public wires including ONE */
  /* -- HBM plan (all optional: 0 = default) -- */
  /* Largest batch that will be proved with this key.  The auto window plan (window_bits = 0) sizes
   * the MSM tables so that the prover's working set for max_batch -- two pipeline sets of value
   * file + a, b, c, the NTT scratch, MSM digits and partial sums -- still fits beside them
   * (wider batches get narrower tables instead of ZKMI_ERR_OOM at prove time).  0 = 1024. */
  uint32_t max_batch;
  /* Upper bound for the key's MSM tables in bytes (G1 + G2), e.g. to leave room for a second key
   * on the same GPU.  0 = whatever the free HBM minus the working set allows. */
  uint64_t table_budget_bytes;
  /* Value slots of the constraint system that will be solved with this key (zkmi_cs_desc.n_slots)
   * for the working-set estimate; 0 = n_wires + 5 %. */
  uint32_t n_slots_hint;
  /* Comb / shared-table MSMs: (window, chunk) blocks in flight as a multiple of the chip's wave
   * slots (measured best: 16 for comb, 8 for shared tables).  0 = default. */
  uint32_t msm_chunk_factor;
  /* 1 = most wire values of this circuit are bits or small integers (e.g. Keccak, bit
   * decompositions): the auto plan then keeps subset-sum comb tables for every MSM, whose zero
   * digits are skipped, instead of sign-pattern tables (one more base per group for the same HBM,
   * but no digit of a sign pattern is ever "nothing to add").  2 = (almost) all wires are bits: the
   * wire MSMs additionally get small tables (one addition per group is all they execute) and the
   * quotient MSM, whose scalars are dense, takes the freed HBM with its own, wider plan.
   * 0 = dense field elements (Poseidon). */
  uint32_t sparse_witness;
  /* Commitment extension: 0 / NULL for a plain Groth16 key.  With k_wire = NULL the library leaves
   * the private committed wires and the commitment wires out of pk.G1.K, as gnark's setup does. */
  uint32_t n_commitments;
  const zkmi_commitment_desc* commitments;
  /* Quotient in evaluation form; NULL = off.  The constraint system the key belongs to (a host
   * struct; only n_wires, n_constraints, n_coeffs, coeffs, o_ptr and o_terms are read).  The prover's
   * sum_k h_k Z_k is linear in the evaluations of a.b on the coset and in c, and c = O.w is linear in
   * the wires, so the change of basis is applied once, here, to the bases: pk.G1.Z becomes its
   * 2^log_n-point image E and every G1.K base takes the share of its wire's O column (ONE and the
   * public wires that O touches get bases of their own).  Proving then needs neither the transform
   * of c nor the final inverse transform.  The key is folded when log_n >= 8, n_commitments = 0 and
   * the system's n_wires / n_constraints fit the key; otherwise it loads as without this field
   * (zkmi_pk_folded tells).  A malformed system (the checks of zkmi_r1cs_load) is ZKMI_ERR_ARG.
   * With a folded key:
   *   - the c given to zkmi_prove_witness_submit(r1cs = NULL, ...) is ignored; c must be O.w, which
   *     gnark's solution.C is, and the system proved must be the one given here;
   *   - proofs of satisfied witnesses are byte for byte those of the unfolded key; the proofs of
   *     unsatisfied witnesses, which are flagged in status_out and never valid, are other bytes
   *     than the unfolded key writes. */
  const zkmi_r1cs_desc* fold_r1cs;
} zkmi_pk_desc;
/* Copies the key to the device and builds the MSM window tables; host buffers may be freed
 * afterwards.  One-off per circuit (gnark's icicle backend does the same lazily). */
int zkmi_pk_load(zkmi_ctx* ctx, const zkmi_pk_desc* desc, zkmi_pk** out);
/* The same with an explicit table plan for each of the key's five MSMs: msm_window_bits[5] = the
 * window_bits (as zkmi_msm_bases_load; 0 is not accepted) of A, B1, K, Z and B2, in this order, in
 * the place of window_bits_g1 / window_bits_g2 and of the auto plan.  NULL = zkmi_pk_load.  The auto
 * plan of a key of 4096 or more G1 bases gives each MSM a comb group size of its own: the quotient
 * MSM (Z), whose scalars are dense, a wider table than the wire MSMs, which execute only the
 * groups that vary over the batch (zkmi_pk_msm_plan tells what was chosen). */
int zkmi_pk_load_planned(zkmi_ctx* ctx, const zkmi_pk_desc* desc, const uint32_t* msm_window_bits,
                         zkmi_pk** out);
void zkmi_pk_free(zkmi_ctx* ctx, zkmi_pk* pk);
/* Window plan chosen for the key: info[0] = windows per G1 scalar, [1] = table entries per G1
 * base, [2] = windows per G2 scalar, [3] = table entries per G2 base, [4] = G1 table bytes (all
 * four MSMs), [5] = G2 table bytes, [6] / [7] = 1 when the G1 / G2 tables are shared-table plans,
 * [8] / [9] = group size k of the G1 / G2 comb tables (0 otherwise; then [0] / [2] = 254). */
int zkmi_pk_info(const zkmi_pk* pk, uint64_t* info /* 10 */);
/* Comb plan per MSM: plan[0..4] = group size k of the comb tables of A, B1, K, Z and B2 (0: not a
 * comb plan), plan[5..9] = 1 when they are sign-pattern tables.  zkmi_pk_info's [0], [1], [6] and
 * [8] describe Z, its [2], [3], [7] and [9] B2. */
int zkmi_pk_msm_plan(const zkmi_pk* pk, uint32_t* plan /* 10 */);
/* 1 when the key was loaded with its quotient bases in evaluation form (fold_r1cs), else 0. */
int zkmi_pk_folded(const zkmi_pk* pk);

/* -- constraint system (witness program) ----------------------------------------------------- */
/* What cs.R1CS.Solve needs, in the scheduled form produced by
 * gnark_crypto_primitives_amd.frontend.compile_circuit: the circuit's field
 * operations packed into steps of up to `lanes_per_proof` independent operations of one class;
 * the GPU runs a step with that many lanes of a wavefront per proof.
 *   program: n_rows x (1 + lanes_per_proof) x 4 words.  Row = header (class, active, aux, 0) +
 *   one operand quad per sub-lane (op | check << 5 | class << 6 | constraint_row << 9, dst slot,
 *   a, b).  Systems with commitments hold one COMMIT row per commitment (header class 9, aux =
 *   commitment index): the solver stops in front of it, the prover commits, hashes, writes the
 *   challenge into the commitment wire and resumes (zkmi_prove_submit needs a key whose
 *   n_commitments matches).  Unit rows with operand rows behind them: multiplicities of a lookup
 *   table (class 8: gnark std/lookup/logderivarg's count hint) and the quotient / remainder of a
 *   multi-limb product by a 4 x 64-bit modulus (class 11: the mulHint of gnark's std/math/emulated;
 *   header (11, na + nb, rows, nout | na << 8 | first modulus constant << 12), the limb slots of the
 *   two operands in the rows that follow, nout consecutive wires written). */
typedef struct {
  uint32_t n_wires, n_public, n_secret, n_constraints;
  uint32_t n_slots, n_rows, n_consts;
  uint32_t lanes_per_proof; /* a power of two, 1 .. 64 */
  const uint32_t* program;
  const void* consts;      /* n_consts fr elements, Montgomery */
} zkmi_cs_desc;
int zkmi_cs_load(zkmi_ctx* ctx, const zkmi_cs_desc* desc, zkmi_cs** out);
void zkmi_cs_free(zkmi_ctx* ctx, zkmi_cs* cs);

/* Witness solve only.  stands in for cs.R1CS.Solve (gnark constraint/bn254).
 *   inputs: batch x (n_public - 1 + n_secret) fr elements, Montgomery, proof-major
 *   wires_out (optional): batch x n_wires ; abc_out (optional): 3 x batch x n_constraints
 *   status_out: per proof, 0 or ZKMI_ERR_UNSATISFIED */
int zkmi_solve_batch(zkmi_ctx* ctx, const zkmi_cs* cs, const void* inputs, size_t batch,
                     void* wires_out, void* abc_out, int32_t* status_out);

/* Full Groth16 prove for a batch of independent witnesses.  stands in for groth16.Prove(ccs, pk,
 * fullWitness) called `batch` times (gnark backend/groth16/bn254/prove.go).
 *   inputs: as zkmi_solve_batch
 *   rs: batch x 2 fr elements (Montgomery): the prover's blinding scalars r, s.  gnark samples
 *       them inside Prove; they are an input here so results are reproducible.
 *   proofs_out: batch x 256 B: Ar (G1) | Krs (G1) | Bs (G2), the field order of gnark's Proof
 *   status_out: per proof */
int zkmi_prove_batch(zkmi_ctx* ctx, const zkmi_pk* pk, const zkmi_cs* cs, const void* inputs,
                     size_t batch, const void* rs, void* proofs_out, int32_t* status_out);

/* The same prove split in two so that consecutive batches overlap: `submit` stages the inputs and
 * runs the witness solve on a second HIP stream, `collect` runs quotient + MSMs + assembly of the
 * OLDEST submitted batch and blocks until its proofs are written.  At most two batches may be in
 * flight; submit(k+1) before collect(k) hides the latency-bound solve of batch k+1 under batch
 * k's MSMs, and collect(k) queues batch k+1's quotient and MSM kernels before it waits, so batch
 * k's (equally latency-bound) assembly runs underneath them on a third stream.
 * Device-pointer inputs / rs must stay valid until the matching collect.  While a batch is in
 * flight the other entry points of the same context return ZKMI_ERR_ARG. */
int zkmi_prove_submit(zkmi_ctx* ctx, const zkmi_pk* pk, const zkmi_cs* cs, const void* inputs,
                      size_t batch, const void* rs);
int zkmi_prove_collect(zkmi_ctx* ctx, void* proofs_out, int32_t* status_out);
/* The same for keys with the commitment extension: commitments_out receives, per proof,
 * (n_commitments + 1) G1 affine points: proof.Commitments[0..n-1] then proof.CommitmentPok.
 * zkmi_prove_collect on such a key returns ZKMI_ERR_ARG (a proof without them cannot verify). */
int zkmi_prove_collect_ex(zkmi_ctx* ctx, void* proofs_out, int32_t* status_out,
                          void* commitments_out);

/* -- the gnark drop-in entry: prove from SOLVED witnesses --------------------------------------- */
/* For a caller that keeps gnark's own solver (cs.Solve -> solution.W, and optionally solution.A,
 * .B, .C) and hands quotient, MSMs and assembly to the GPU -- the place of groth16.Prove(ccs, pk,
 * fullWitness) (reference call sites: tree/test/verifier_bn254_test.go:41,67; what gnark's icicle
 * backend accelerates [UPSTREAM-RECALL, SURVEY.md §3.2, §8b]).  No zkmi_cs is needed.
 *
 * Page-locked host memory for the batch arrays.  A shim assembles a batch from per-proof witness
 * vectors anyway; assembling it in memory from zkmi_host_alloc lets the DMA engine read it in place
 * (no staging copy, truly asynchronous submit).  Ordinary (pageable) memory is accepted everywhere
 * and staged through a ring of pinned chunks owned by the context. */
void* zkmi_host_alloc(zkmi_ctx* ctx, size_t bytes);
void zkmi_host_free(zkmi_ctx* ctx, void* p);
/* Host threads that copy pageable memory into the pinned ring (0 = default 4). */
int zkmi_set_copy_threads(zkmi_ctx* ctx, int threads);
/* Wavefronts per workgroup of the witness solve kernel: 1, 2, 4 or 8 (0 = default).  The solve of
 * one batch runs beside the MSMs of another; packed into whole workgroups its wavefronts occupy
 * fewer compute units.  Results do not depend on it.  Any other value is ZKMI_ERR_ARG. */
int zkmi_set_solve_waves_per_block(zkmi_ctx* ctx, int waves);

/* The R1CS matrices, so that a caller ships the wire vector only and a = L.w, b = R.w, c = O.w are
 * formed on the GPU ("zkmi_cs_load ... CSR A,B,C").  Mirrors gnark's
 * constraint.R1CS [UPSTREAM-RECALL]: a coefficient table (cs.Coefficients, fr Montgomery) and, per
 * constraint, three linear expressions of terms {coefficient index, wire index} (constraint.Term
 * {CID, VID}); *_ptr are n_constraints + 1 offsets into the term arrays, starting at 0. */
typedef struct {
  uint32_t coeff; /* index into coeffs */
  uint32_t wire;  /* column: 0 = ONE, then public, secret, internal wires */
} zkmi_term;
struct zkmi_r1cs_desc {
  uint32_t n_wires, n_constraints, n_coeffs;
  const void* coeffs; /* n_coeffs fr elements, Montgomery, reduced */
  const uint32_t* l_ptr;
  const zkmi_term* l_terms;
  const uint32_t* r_ptr;
  const zkmi_term* r_terms;
  const uint32_t* o_ptr;
  const zkmi_term* o_terms;
};
typedef struct zkmi_r1cs zkmi_r1cs;
/* Validates every index on the host, copies the matrices to the device; host buffers may be freed
 * afterwards. */
int zkmi_r1cs_load(zkmi_ctx* ctx, const zkmi_r1cs_desc* desc, zkmi_r1cs** out);
void zkmi_r1cs_free(zkmi_ctx* ctx, zkmi_r1cs* r1cs);

/* Stage 1 of a prove from solved witnesses; the matching zkmi_prove_collect returns the proofs.
 * Pipelines exactly like zkmi_prove_submit (two batches in flight, same streams, same HBM plan):
 * batch k+1 streams in over PCIe underneath batch k's MSM kernels.
 *   wires: batch x pk.n_wires fr elements (Montgomery, gnark's image), proof-major: the full wire
 *          vector including the ONE wire at index 0; 16-byte aligned
 *   r1cs != NULL: a = b = c = NULL, n_constraints = 0 or the loaded system's; the device forms
 *          a, b, c and checks a.b = c (per-proof ZKMI_ERR_UNSATISFIED in collect's status_out)
 *   r1cs == NULL: a, b, c: batch x n_constraints fr elements each (<L_k,w>, <R_k,w>, <O_k,w>,
 *          solution.A/B/C); taken as they are (status_out = 0); the library pads to the domain
 *          (a key folded with zkmi_pk_desc.fold_r1cs does not read c: it must be O.w of that system)
 *   rs: batch x 2 fr, as zkmi_prove_batch
 * Pageable host arrays have been consumed when the call returns; page-locked and device arrays
 * must stay valid until the matching collect. */
int zkmi_prove_witness_submit(zkmi_ctx* ctx, const zkmi_pk* pk, const zkmi_r1cs* r1cs,
                              const void* wires, const void* a, const void* b, const void* c,
                              size_t n_constraints, size_t batch, const void* rs);
/* Blocking form: zkmi_prove_witness_submit(r1cs = NULL) + zkmi_prove_collect (returns
 * ZKMI_ERR_ARG while submitted batches are in flight). */
int zkmi_prove_witness_batch(zkmi_ctx* ctx, const zkmi_pk* pk, const void* wires, const void* a,
                             const void* b, const void* c, size_t n_constraints, size_t batch,
                             const void* rs, void* proofs_out);

/* -- the gnark drop-in entry: solve AND prove from inputs --------------------------------------- */
/* For a caller that holds a gnark ccs and no witness program (zkmi_cs): the GPU solves the
 * gnark-shaped system itself, in place of cs.Solve on the caller's CPUs.  The description adds
 * to the loaded matrices what gnark's solver walks [UPSTREAM-RECALL]: the instruction order
 * (cs.Instructions: constraints and hint calls interleaved) and the hint table.  The caller names no
 * solve wire: as gnark does at run time, the library finds the one wire of each constraint that no
 * earlier instruction has solved (ONE, the public and the secret inputs are solved to begin with).
 * Hints are named by kind number; a shim maps gnark's hint names to them.  Supported kinds: */
enum zkmi_hint_kind {
  ZKMI_HINT_INVZERO = 1, /* solver.InvZeroHint: one input x, one output 1/x, or 0 for x = 0 */
  ZKMI_HINT_NBITS = 2,   /* bits.NBits: one input, output i = bit i of its canonical value */
  /* The kinds below are accepted under hint_set = ZKMI_HINTS_STD and ZKMI_HINTS_EMULATED only.
   * Their first input expression is a constant parameter p0: terms on wire 0 (ONE) alone, evaluated
   * at load time. */
  ZKMI_HINT_LIMBS = 3,   /* p0 = width (1 .. 64), one value expression; output j = bits
                            [j width, (j + 1) width) of its canonical value, bits from 256 on are 0 */
  ZKMI_HINT_COUNT = 4,   /* p0 = table size = number of outputs; every further input is a query;
                            output j = number of queries whose canonical value is j (a query >= size
                            counts nowhere) */
  ZKMI_HINT_COMMIT = 5,  /* p0 = n_hashed, then the n_hashed hashed operands, then the private ones,
                            one output: the commitment wire.  Every operand is one solved wire with
                            coefficient 1.  A phase boundary of zkmi_prove_r1cs_submit, which needs the
                            key's commitment keys; refused by zkmi_r1cs_solve_batch */
  ZKMI_HINT_BYTEOP = 6,  /* p0 = 1 XOR | 2 AND, two expressions, one output: the operation on the low
                            32 bits of their canonical values */
  /* Accepted under hint_set = ZKMI_HINTS_EMULATED only: the product hint of std/math/emulated
   * [UPSTREAM-RECALL].  p0 = na | nb << 8 | nk << 16, then na limb expressions of a, nb of b and four
   * of the modulus p: 1 + na + nb + 4 inputs.  a = sum a_i 2^(64 i), where a limb may exceed 64 bits
   * (lazy additions); b likewise.  The four modulus expressions are constants like p0 (an empty
   * expression is 0), each below 2^64.  Outputs, in order: nk 64-bit limbs of floor(a b / p), four
   * 64-bit limbs of a b mod p, then ncols - 1 carries, ncols = max(na + nb - 1, nk + 3): as field
   * elements, c_j = (sum_i a_i b_(j-i) - r_j - sum_i k_i p_(j-i) + c_(j-1)) 2^-64.
   * Limits: 1 <= na, nb <= 4, 1 <= nk <= 8, 2^224 <= p < 2^256 (checked at load time).  The
   * caller's circuit keeps a, b < 2^384 and the quotient below 2^(64 nk): the integers are held in
   * twelve 32-bit words per operand, and beyond that the quotient and remainder outputs are
   * unspecified -- never a fault. */
  ZKMI_HINT_EMULMUL = 7
};
/* The numbers are those of this repository's frontend; the parity of the hints' names and operand
 * order with gnark's own is not pinned.  Unknown kinds are refused by name at load time under every
 * hint set, kind 7 under ZKMI_HINTS_BASIC and ZKMI_HINTS_STD. */
enum zkmi_hint_set {
  ZKMI_HINTS_BASIC = 0, /* InvZero and NBits; every other kind is refused by name at load time */
  ZKMI_HINTS_STD = 1,   /* additionally limbs, lookup multiplicities, commitment, byte operations */
  /* Read the field as bits: 1 = the kinds of ZKMI_HINTS_STD, 2 = the emulated product.  Every
   * emulated circuit range-checks its limbs through the std kinds, so 2 alone is not offered and is
   * refused. */
  ZKMI_HINTS_EMULATED = 3 /* the kinds of ZKMI_HINTS_STD and the emulated product (kind 7) */
};
typedef struct {
  uint32_t n_public;  /* public wires including ONE */
  uint32_t n_secret;
  uint32_t n_instr, n_hints;
  const uint32_t* instr;        /* n_instr x 2: (0 = constraint | 1 = hint, index), in solve order;
                                   every constraint exactly once */
  const uint32_t* hint_kind;    /* n_hints */
  const uint32_t* hint_in_ptr;  /* n_hints + 1: hint h reads the expressions hint_in_ptr[h] .. [h + 1] */
  const uint32_t* hint_lc_ptr;  /* one more than expressions: offsets into hint_terms */
  const zkmi_term* hint_terms;  /* coefficient indices into the loaded system's table */
  const uint32_t* hint_out_ptr; /* n_hints + 1 offsets into hint_out */
  const uint32_t* hint_out;     /* wires the hints write */
  uint32_t lanes_per_proof;     /* lanes of a wavefront that share one proof's terms: a power of two,
                                   1 .. 64; 0 = the power of two in 1 .. 16 nearest to the mean number
                                   of terms per instruction */
  uint32_t hint_set;            /* enum zkmi_hint_set; 0 = ZKMI_HINTS_BASIC.  The last field: it takes
                                   the place of what was tail padding behind lanes_per_proof, so
                                   sizeof and every other offset are those of a struct without it, and
                                   a caller that zero-initialises the struct gets the basic set */
} zkmi_r1cs_solver_desc;
typedef struct zkmi_r1cs_solver zkmi_r1cs_solver;
/* Builds the solve plan on the host (csrc/r1cs_plan.h) and uploads it; `r1cs` and the host arrays
 * may be freed afterwards.  ZKMI_ERR_ARG with a message that names the instruction when a
 * constraint has two unknown wires, its unknown occurs twice, a hint reads an unsolved wire, an
 * index is out of range, a constraint occurs twice or never, a wire stays unsolved, a hint is of
 * a kind outside desc->hint_set, or a hint's operands, outputs or parameter do not fit its kind. */
int zkmi_r1cs_solver_load(zkmi_ctx* ctx, const zkmi_r1cs* r1cs, const zkmi_r1cs_solver_desc* desc,
                          zkmi_r1cs_solver** out);
void zkmi_r1cs_solver_free(zkmi_ctx* ctx, zkmi_r1cs_solver* solver);
/* info[0] = instructions, [1] = lanes per proof, [2] = terms of all instructions (the unknowns'
 * own excluded), [3] = terms of the longest instruction, [4] = field inversions per proof,
 * [5] = n_wires, [6] = n_constraints, [7] = inputs per proof (n_public - 1 + n_secret). */
int zkmi_r1cs_solver_info(const zkmi_r1cs_solver* solver, uint64_t* info /* 8 */);
/* Witness solve only, the conventions of zkmi_solve_batch: inputs batch x (n_public - 1 + n_secret),
 * wires_out (optional) batch x n_wires, abc_out (optional) 3 x batch x n_constraints, status_out per
 * proof 0 or ZKMI_ERR_UNSATISFIED (an assertion fails, or the factor a solve divides by is 0).
 * A solver whose plan holds commitment hints is refused: their values need a proving key
 * (zkmi_prove_r1cs_submit). */
int zkmi_r1cs_solve_batch(zkmi_ctx* ctx, const zkmi_r1cs_solver* solver, const void* inputs,
                          size_t batch, void* wires_out, void* abc_out, int32_t* status_out);
/* Stage 1 of a prove from inputs; the matching zkmi_prove_collect returns the proofs.  Pipelines
 * exactly like zkmi_prove_submit (two batches in flight, same streams, same HBM plan).  A key with
 * commitments needs a solver loaded with ZKMI_HINTS_STD or ZKMI_HINTS_EMULATED whose commitment
 * hints match the key's commitments one by one (commitment wire, hashed and private wires, in order): the solve stops at
 * each, the commitment is formed and hashed into its wire, and zkmi_prove_collect_ex returns
 * commitments and proof of knowledge.  Every mismatch is refused before anything is queued. */
int zkmi_prove_r1cs_submit(zkmi_ctx* ctx, const zkmi_pk* pk, const zkmi_r1cs_solver* solver,
                           const void* inputs, size_t batch, const void* rs);

/* -- PLONK (BASELINE config 5 names this backend) ----------------------------------------------- */
/* Stands in for plonk.Prove of gnark backend/plonk/bn254 [UPSTREAM-RECALL]: KZG commitments over
 * the SRS, blinded wire polynomials, permutation grand product, quotient on the coset 5<w_4n>
 * split in three, linearisation and two openings.  The Fiat-Shamir hashing stays on the host, as
 * in gnark, between five round calls; protocol and transcript: DESIGN.md (parity unpinned: the
 * reference holds no PLONK vector).  All arrays: fr in gnark's Montgomery image; batch arrays are
 * proof-major; host or device pointers. */
typedef struct zkmi_plonk_pk zkmi_plonk_pk;
typedef struct {
  uint32_t log_n;          /* domain 2^log_n >= number of gates, 4 .. 24 */
  uint32_t n_public;       /* public inputs (without ONE): the first n_public gates */
  const void* coef;        /* 8 x n: qL, qR, qO, qM, qC, S1, S2, S3 in coefficient form */
  const void* coset;       /* 8 x 4n: the same polynomials on the coset 5 <w_4n>, natural order */
  const void* sigma;       /* 3 x n: S1, S2, S3 values on the domain (k_c w^r of the image position) */
  const void* omega;       /* n: w^i */
  const void* coset_x;     /* 4n: 5 w_4n^j */
  const void* l1_coset;    /* 4n: L_1 on the coset */
  const void* zh_inv;      /* 4: 1 / Z_H on the coset (period 4) */
  const void* srs_g1;      /* n + 6 G1 affine points: [tau^i]_1 */
  uint32_t window_bits;    /* MSM table plan of the SRS, as zkmi_msm_bases_load */
  uint32_t max_batch;      /* 0 = 64 */
  /* Optional (lag_k = 0: unused): commit the wire columns a, b, c in the Lagrange basis, as gnark
   * does with its Lagrange-form SRS [UPSTREAM-RECALL], instead of their coefficient forms.  The
   * scalars are then the witness values themselves: for circuits whose wires are mostly bits or
   * small integers (Keccak, bit decompositions) almost every digit of the subset-sum tables is
   * zero and skipped.  lag_g1[c] (c = 0, 1, 2 for a, b, c): n + 2 G1 points in the order the MSM
   * groups them (lag_k per group); lag_rows[c][j] = row of column c whose value multiplies point j:
   * a gate row r < n for [L_r(tau)]_1, n / n + 1 for the blinding points [tau^(n+1) - tau]_1 /
   * [tau^n - 1]_1 (scalars b1 / b2 of the column).  Order rows of large values first; only speed
   * depends on the order.  Same commitments as in coefficient form. */
  const void* lag_g1[3];
  const uint32_t* lag_rows[3];
  uint32_t lag_k;          /* bases per subset-sum table of the Lagrange points, 4 .. 16; 0 = off */
} zkmi_plonk_pk_desc;
int zkmi_plonk_pk_load(zkmi_ctx* ctx, const zkmi_plonk_pk_desc* desc, zkmi_plonk_pk** out);
void zkmi_plonk_pk_free(zkmi_ctx* ctx, zkmi_plonk_pk* pk);
/* Round 1: witness solve (cs: the circuit's gate rows, frontend/scs.py), blinding (blind: batch x 9
 * fr: b1 X + b2 for a, b, c and b7 X^2 + b8 X + b9 for z), commits_out: batch x 3 G1 ([a] [b] [c]). */
int zkmi_plonk_round1(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_cs* cs, const void* inputs,
                      size_t batch, const void* blind, void* commits_out, int32_t* status_out);
/* Round 2: beta_gamma: batch x 2 fr; commit_z_out: batch G1. */
int zkmi_plonk_round2(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const void* beta_gamma, void* commit_z_out);
/* Round 3: alpha: batch fr; commits_t_out: batch x 3 G1 ([t_lo] [t_mid] [t_hi], n + 2 coefficients each). */
int zkmi_plonk_round3(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const void* alpha, void* commits_t_out);
/* Round 4: zeta_zetaw: batch x 2 fr (zeta, zeta w); evals_out: batch x 6 fr: a, b, c, S1, S2 at zeta,
 * z at zeta w. */
int zkmi_plonk_round4(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const void* zeta_zetaw, void* evals_out);
/* Round 5: scalars: batch x 14 fr (coefficients of the linearisation polynomial: qM, qL, qR, qO, S3,
 * z, t_lo, t_mid, t_hi; its constant term minus sum v^i e_i; v; zeta; zeta w; z(zeta w));
 * commits_w_out: batch x 2 G1 ([W_zeta] [W_zeta_w]). */
int zkmi_plonk_round5(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const void* scalars, void* commits_w_out);

/* plonk.Prove for a batch in one call: the five rounds above with the Fiat-Shamir transcript (SHA-256,
 * DESIGN.md §3.6) computed on the host inside the library between them.  vk_digest: the 32-byte
 * digest of the verifying key that opens the transcript (plonk.py: ProvingKey.vk_digest).
 *   proofs_out: batch x 768 bytes: 9 G1 affine points ([a] [b] [c] [z] [t_lo] [t_mid] [t_hi]
 *   [W_zeta] [W_zeta_w]) then 6 fr (a, b, c, S1, S2 at zeta, z at zeta w), gnark's Montgomery image. */
int zkmi_plonk_prove(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_cs* cs, const void* inputs,
                     size_t batch, const void* blind, const uint8_t* vk_digest, void* proofs_out,
                     int32_t* status_out);

/* -- the gnark drop-in entry of the PLONK prover --------------------------------------------------- */
/* For a caller that holds gnark's own objects [UPSTREAM-RECALL]: the proving key as a trace
 * (plonk.ProvingKey: selector values on the domain and a permutation), a constraint.SparseR1CS, and
 * solved wires -- no zkmi_cs and no expanded key.  Parity with gnark (gate convention of the public
 * rows, transcript) is unpinned, as for the rest of the PLONK prover.
 *
 * zkmi_plonk_pk_load_trace: the key from its trace form.  Everything else zkmi_plonk_pk_desc takes
 * as data (w^i, the sigma values, the eight coefficient forms and their coset evaluations, the coset
 * points, L_1 and 1 / Z_H on the coset) is computed on the GPU at load time; a key loaded this way
 * proves exactly what the same key loaded through zkmi_plonk_pk_load proves. */
typedef struct {
  uint32_t log_n;          /* as zkmi_plonk_pk_desc */
  uint32_t n_public;       /* as zkmi_plonk_pk_desc */
  const void* selectors;   /* 5 x n fr: qL, qR, qO, qM, qC as values on the domain (Montgomery); rows
                              past the last gate are zero */
  const uint32_t* perm;    /* 3n entries of 32 bits (3n <= 3 * 2^24 fits): position c n + r (column
                              c = 0, 1, 2 for a, b, c; row r) -> its image position; gnark's trace.S
                              narrowed from int64.  Must be a bijection of [0, 3n) */
  const void* srs_g1;      /* the remaining fields: as zkmi_plonk_pk_desc */
  uint32_t window_bits;
  uint32_t max_batch;
  const void* lag_g1[3];
  const uint32_t* lag_rows[3];
  uint32_t lag_k;
} zkmi_plonk_trace_desc;
/* Refuses, with a message: a perm entry >= 3n, a perm that is not a bijection, and whatever
 * zkmi_plonk_pk_load refuses.  The key keeps a host copy of perm for the wiring check below; the
 * caller's arrays (host or device) may be freed afterwards.  Free with zkmi_plonk_pk_free. */
int zkmi_plonk_pk_load_trace(zkmi_ctx* ctx, const zkmi_plonk_trace_desc* desc, zkmi_plonk_pk** out);

/* The sparse constraint system: gate g reads wire xa[g], xb[g], xc[g] in columns a, b, c and asserts
 *   qL a + qR b + qO c + qM a b + qC + PI_g = 0,   PI_g = -a_g for g < n_public, else 0
 * (public input g is the value in column a of row g). */
typedef struct {
  uint32_t n_wires, n_gates, n_public; /* n_public <= n_gates <= 2^24 */
  const uint32_t* xa;                  /* n_gates wire indices each, below n_wires */
  const uint32_t* xb;
  const uint32_t* xc;
  const void* selectors;               /* 5 x n_gates fr: the trace's values, Montgomery, reduced */
} zkmi_scs_desc;
typedef struct zkmi_scs zkmi_scs;
/* Validates every index on the host (csrc/scs_check.h), copies the system to the device; the caller's
 * arrays (host or device) may be freed afterwards. */
int zkmi_scs_load(zkmi_ctx* ctx, const zkmi_scs_desc* desc, zkmi_scs** out);
void zkmi_scs_free(zkmi_ctx* ctx, zkmi_scs* scs);

/* Round 1 from solved witnesses, in the place of zkmi_plonk_round1; rounds 2 .. 5 follow as usual.
 *   scs != NULL (wire form): wires = batch x scs.n_wires fr (Montgomery, reduced), proof-major,
 *          16-byte aligned, in pageable, page-locked (zkmi_host_alloc) or device memory; a = b = c =
 *          NULL; n_gates = 0 or the loaded system's.  The device gathers the three columns, checks
 *          every gate (per-proof ZKMI_ERR_UNSATISFIED in status_out); the copy constraints hold by
 *          construction.
 *   scs == NULL (column form): wires = NULL; a, b, c = batch x n_gates fr each, proof-major, taken
 *          as they are (status_out = 0); the library pads to the domain.
 * Giving both forms or neither is ZKMI_ERR_ARG.  Also refused, before anything is staged: n_gates
 * above 2^log_n, a system whose n_public differs from the key's, batch outside [1, max_batch] and,
 * for a key loaded from its trace form, a wiring that contradicts the key's permutation (checked on
 * the host at the first prove of a (key, system) pair; a key from zkmi_plonk_pk_load has no
 * permutation to compare).  The arrays have been consumed when the call returns. */
int zkmi_plonk_round1_witness(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_scs* scs,
                              const void* wires, const void* a, const void* b, const void* c,
                              size_t n_gates, size_t batch, const void* blind, void* commits_out,
                              int32_t* status_out);
/* zkmi_plonk_prove from solved witnesses: zkmi_plonk_round1_witness, then the same four rounds and
 * the same transcript, whose public inputs are the values in column a of rows 0 .. n_public - 1. */
int zkmi_plonk_prove_witness(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_scs* scs,
                             const void* wires, const void* a, const void* b, const void* c,
                             size_t n_gates, size_t batch, const void* blind,
                             const uint8_t* vk_digest, void* proofs_out, int32_t* status_out);

/* -- PLONK: circuits that call api.Commit (BSB22; the Qcp selector columns) ------------------------- */
/* What gnark's PLONK backend does for api.Commit [UPSTREAM-RECALL]; parity unpinned, as for the rest
 * of the PLONK prover.  A key carries n_c <= ZKMI_PLONK_MAX_COMMITMENTS commitments.  Commitment i has
 * its committed rows C_i (gate rows, public rows counted, ascending), where the selector Qcp_i is 1,
 * and its commitment row r_i; the gate equation becomes
 *   qL a + qR b + qO c + qM a b + qC + PI'_g + sum_i Qcp_i,g pi2_i,g = 0,   PI'_(r_i) = +H_i.
 * pi2_i is the Lagrange-form polynomial that holds a_g on C_i, the caller's blinding scalars at row
 * r_i and at the last row of the key's domain, 2^log_n - 1 (where both coincide, the second one), and
 * zero elsewhere; [pi2_i] its KZG commitment; H_i = hash_to_field([pi2_i].Marshal(), "BSB22-Plonk").
 * Transcript: alpha = H("alpha", beta, [pi2_0], .., [z]); v absorbs the Qcp_i(zeta) after the six
 * evaluations; the linearisation polynomial gains sum_i Qcp_i(zeta) pi2_i(X), the opening at zeta
 * v^(6+i) Qcp_i(X).  DESIGN.md §3.6. */
#define ZKMI_PLONK_MAX_COMMITMENTS 8
typedef struct {
  uint32_t n_rows;        /* |C_i| >= 1 */
  uint32_t row;           /* r_i: not in rows */
  const uint32_t* rows;   /* C_i: n_rows gate rows, ascending, below 2^log_n - 1 */
  const uint32_t* slots;  /* n_rows value-file slots of the committed operands (wire-backed slots of
                             the zkmi_cs program, in rows order): what zkmi_plonk_prove_ex reads at the
                             program's COMMIT row; NULL for a key that only proves from solved wires */
  const void* lag_g1;     /* n_rows + 2 G1 affine points: [L_g(tau)]_1 for g in rows order, then for
                             the two blinding rows r_i and 2^log_n - 1 */
  uint32_t lag_k;         /* bases per subset-sum table of these points, 4 .. 16; 0 = auto */
} zkmi_plonk_commit_desc;
/* Attaches the commitments to a key from either loader, before its first prove and once.  The
 * library builds Qcp_i (coefficient form and coset evaluations) on the GPU and loads the tables of
 * the Lagrange points.  Refused with a message (csrc/plonk_commit_check.h), nothing attached: n = 0
 * or above 8, rows not ascending / not unique / outside the domain, row among its own rows, a
 * blinding row inside C_i, a second call, a call after a prove. */
int zkmi_plonk_pk_set_commitments(zkmi_ctx* ctx, zkmi_plonk_pk* pk,
                                  const zkmi_plonk_commit_desc* descs, uint32_t n);
/* The commitment step alone (a shim's replacement for gnark's bsb22 hint calls it while gnark
 * solves): values = batch x n_rows fr, blind2 = batch x 2 fr (Montgomery, proof-major) ->
 * commit_out = batch x 64 bytes ([pi2_index] affine, Montgomery), h_out = batch fr (H, Montgomery). */
int zkmi_plonk_commit_hint(zkmi_ctx* ctx, zkmi_plonk_pk* pk, uint32_t index, const void* values,
                           const void* blind2, size_t batch, void* commit_out, void* h_out);
/* zkmi_plonk_prove / zkmi_plonk_prove_witness for keys with commitments: blind_commit = batch x
 * 2 n_c fr (per commitment the scalars at r_i and at the last row), commit_out = batch x n_c x 96
 * bytes ([pi2_i] affine, then Qcp_i(zeta)).  With a key without commitments and both NULL they return
 * what the plain entries return.  The plain entries and the round-by-round calls refuse a key with
 * commitments (ZKMI_ERR_ARG).  From inputs, the program's COMMIT rows must be the key's commitments
 * in order; from solved wires or columns, a proof whose a[r_i] differs from H_i is flagged
 * ZKMI_ERR_UNSATISFIED. */
int zkmi_plonk_prove_ex(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_cs* cs, const void* inputs,
                        size_t batch, const void* blind, const void* blind_commit,
                        const uint8_t* vk_digest, void* proofs_out, void* commit_out,
                        int32_t* status_out);
int zkmi_plonk_prove_witness_ex(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_scs* scs,
                                const void* wires, const void* a, const void* b, const void* c,
                                size_t n_gates, size_t batch, const void* blind,
                                const void* blind_commit, const uint8_t* vk_digest, void* proofs_out,
                                void* commit_out, int32_t* status_out);

/* -- PLONK: solve a gnark-shaped SparseR1CS on the GPU from inputs ----------------------------------- */
/* The third PLONK entry, the twin of zkmi_r1cs_solver_load / zkmi_prove_r1cs_submit: the caller holds
 * gnark's sparse system (zkmi_scs_load), its instruction order and its hints, and no witness program
 * of this repository's frontend; spr.Solve runs on the GPU.  The caller names no solve wire: the
 * loader walks `instr` once with a solved-wire bitmap that starts with the wires of input_wire (the
 * ONE wire is not special, its gate qL x - 1 = 0 solves it) and finds each gate's one unknown
 * (csrc/scs_plan.h).  A hint input is a single term, coef * wire or a constant,
 * because a variable of gnark's scs builder is a single term [UPSTREAM-RECALL]; parity unpinned.
 * Hints: ZKMI_HINT_INVZERO and ZKMI_HINT_NBITS under hint_set = ZKMI_HINTS_BASIC, where kinds 3 .. 7
 * are refused by name.  Under hint_set = ZKMI_HINTS_STD additionally kinds 3 .. 6, each input still a
 * single term and the first one the constant parameter p0:
 *   ZKMI_HINT_LIMBS   p0 = width (1 .. 64), one value; output j = bits [j width, (j + 1) width) of its
 *                     canonical value, bits from 256 on are 0
 *   ZKMI_HINT_COUNT   p0 = table size = number of outputs, then the queries; output j = the number of
 *                     queries equal to j, a query >= size counts nowhere
 *   ZKMI_HINT_COMMIT  p0 = the commitment's index (0, 1, .. in instruction order, at most
 *                     ZKMI_PLONK_MAX_COMMITMENTS), then the committed wires in the order of the key's
 *                     `rows`, each a wire with coefficient 1; one output, the commitment wire.  The hint
 *                     stands in front of the gate of its commitment row.  Its value needs the key:
 *                     zkmi_plonk_prove_scs_ex
 *   ZKMI_HINT_BYTEOP  p0 = 1 XOR | 2 AND, two values; one output, the operation on their low 32 bits
 * Kind 7 (the emulated product) is refused by name under both sets, and so is every other hint_set. */
typedef struct {
  uint32_t n_inputs;            /* values per proof, public first: the inputs of zkmi_plonk_prove */
  const uint32_t* input_wire;   /* n_inputs: wire each input lands on; 0xFFFFFFFF = no gate reads it */
  uint32_t n_instr, n_hints;
  const uint32_t* instr;        /* n_instr x 2: (0 = gate | 1 = hint, index), solve order; every gate once */
  const uint32_t* hint_kind;    /* n_hints: enum zkmi_hint_kind */
  const uint32_t* hint_in_ptr;  /* n_hints + 1 */
  const uint32_t* hint_in_wire; /* per hint input: a wire, or 0xFFFFFFFF for a constant */
  const void*     hint_in_coef; /* per hint input: fr, Montgomery: value = coef * wire, or coef alone */
  const uint32_t* hint_out_ptr; /* n_hints + 1 */
  const uint32_t* hint_out;
  uint32_t lanes_per_proof;     /* power of two 1..64; 0 = auto */
  uint32_t hint_set;            /* ZKMI_HINTS_BASIC (0) or ZKMI_HINTS_STD (1); anything else refused, naming
                                   the sets.  The last field: it takes the values a later set defines */
} zkmi_scs_solver_desc;
typedef struct zkmi_scs_solver zkmi_scs_solver;
/* Builds and checks the solve plan on the host and uploads it with a copy of the system; the system
 * and the caller's arrays (host memory) may be freed afterwards.  ZKMI_ERR_ARG with a message that
 * names the instruction for whatever the plan refuses (csrc/scs_plan.h lists it); nothing is loaded
 * then. */
int zkmi_scs_solver_load(zkmi_ctx* ctx, const zkmi_scs* scs, const zkmi_scs_solver_desc* desc,
                         zkmi_scs_solver** out);
void zkmi_scs_solver_free(zkmi_ctx* ctx, zkmi_scs_solver* solver);
/* info: [0] instructions, [1] lanes per proof, [2] solve records, [3] steps, [4] inversions per
 * proof, [5] n_wires, [6] n_gates, [7] inputs per proof. */
int zkmi_scs_solver_info(const zkmi_scs_solver* solver, uint64_t* info /* 8 */);
/* The witness solve alone: inputs = batch x n_inputs fr (Montgomery, proof-major, host or device) ->
 * wires_out = batch x n_wires fr (may be NULL), status_out = per proof 0 or ZKMI_ERR_UNSATISFIED (a
 * solve divides by zero, or a gate does not hold: every gate is checked afterwards, so the status is
 * what zkmi_plonk_prove_witness reports for the same wires).  A solver whose plan holds commitment
 * hints is refused: their values need a proving key (zkmi_plonk_prove_scs_ex). */
int zkmi_scs_solve_batch(zkmi_ctx* ctx, const zkmi_scs_solver* solver, const void* inputs, size_t batch,
                         void* wires_out, int32_t* status_out);
/* zkmi_plonk_round1_witness / zkmi_plonk_prove_witness (wire form) with the wires solved on the GPU
 * from the inputs: same columns, same transcript, same records.  Refused before anything is queued:
 * a key with commitments, an n_public that differs from the key's, batch outside [1, max_batch], more
 * wires than the 4n work buffer holds and, for a trace-loaded key, a wiring that contradicts the
 * key's permutation, a solver whose plan holds commitment hints. */
int zkmi_plonk_round1_scs(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_scs_solver* solver,
                          const void* inputs, size_t batch, const void* blind, void* commits_out,
                          int32_t* status_out);
int zkmi_plonk_prove_scs(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_scs_solver* solver,
                         const void* inputs, size_t batch, const void* blind, const uint8_t* vk_digest,
                         void* proofs_out, int32_t* status_out);
/* zkmi_plonk_prove_scs for keys with commitments, the twin of zkmi_plonk_prove_witness_ex (blind_commit
 * and commit_out as there): a solver loaded with ZKMI_HINTS_STD whose commitment hints are the key's
 * commitments one by one.  The solve stops at each commitment's boundary, the commitment is formed
 * from the committed wires and hashed, H_i goes into the commitment wire, and the solve goes on; the
 * wire-form path follows unchanged.  Refused before anything is queued: what zkmi_plonk_prove_scs
 * refuses (but for the key's commitments), a number of commitment hints that differs from the key's
 * commitments, a hint whose committed wires are not xa[rows[j]] of the key's commitment in order or
 * whose output is not xa[row].  With a key without commitments, a solver without commitment hints and
 * both pointers NULL it returns what zkmi_plonk_prove_scs returns.  status_out: the OR of a zero
 * divisor, the gate check and the commitment check. */
int zkmi_plonk_prove_scs_ex(zkmi_ctx* ctx, zkmi_plonk_pk* pk, const zkmi_scs_solver* solver,
                            const void* inputs, size_t batch, const void* blind, const void* blind_commit,
                            const uint8_t* vk_digest, void* proofs_out, void* commit_out,
                            int32_t* status_out);

/* Per-stage device time of the last zkmi_prove_collect / zkmi_prove_batch in milliseconds, from
 * HIP events on the library's streams: [0] solve (stage 1, second stream), [1] quotient (NTTs +
 * pointwise; with a folded key the transforms of a and b alone), [2] G1 MSMs, [3] G2 MSM, [4] assembly (third stream; overlaps the next batch's
 * quotient when one is submitted), [5] main-stream span = [1] + [2] + [3] + delta multiples,
 * [6] sum over the four G1 msm_accumulate launches alone (one event pair around each launch),
 * [7] the G2 msm_accumulate launch alone.  With comb tables the launch that sums the groups whose
 * scalars the whole batch shares is outside the pair: it runs beside the accumulate launch, on the
 * stream of the MSM tails. */
int zkmi_last_timings(zkmi_ctx* ctx, double* ms_out /* 8 doubles */);

#ifdef __cplusplus
}
#endif
#endif
