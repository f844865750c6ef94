/* amdzk — C ABI of the MI355X (gfx950) Halo2/KZG prover backend.
 *
 * This is the drop-in boundary. The reference (anon-aadhaar-halo2) consumes the
 * prover only through the Rust API of
 *     halo2_proofs 0.2.0 @ PSE v2023_01_20   (/root/reference/Cargo.lock:469-471)
 *     halo2curves  0.3.1                      (/root/reference/Cargo.lock:484-486)
 * re-exported by halo2-base (/root/reference/src/lib.rs:15-18, src/signal.rs:1-5,
 * src/conditional_secrets.rs:1-5, src/timestamp.rs:1-4, src/chip.rs:6). A fork of halo2_proofs
 * patched in with Cargo [patch] redirects the functions named next to each entry point below to
 * this library (INTEGRATION.md shows the `extern "C"` block and the call sites).
 *
 * Number format = halo2curves' in-memory format, so Rust slices cross the boundary untouched:
 *   Fr / Fq      : 4 x u64 little-endian limbs, Montgomery form, R = 2^256            (32 B)
 *   G1Affine     : {x: Fq, y: Fq}; (0,0) is the identity                              (64 B)
 *   G1 (Jacobian): {x, y, z: Fq}; z = 0 is the identity                               (96 B)
 * Points returned by this library are always normalised: z = 1 (Montgomery one) or the identity
 * (0, 1, 0) — equal as group elements to what the CPU prover computes; its own (x,y,z) depend on
 * rayon's thread count, and every caller normalises before writing to the transcript.
 *
 * Ownership: the caller owns every host buffer; the library never keeps a host pointer after a call
 * returns. Device objects are opaque handles freed by the caller.
 * Errors: every function returns 0 on success and a negative amdzk_status on failure; the message is
 * available from amdzk_last_error(). Nothing throws or aborts across this boundary.
 * Threading: one amdzk_ctx per (GPU, host thread). Calls on one ctx are ordered on one HIP stream.
 * There is NO CPU fallback: without a usable gfx950 device amdzk_init fails with AMDZK_E_NO_DEVICE.
 */
#ifndef AMDZK_H
#define AMDZK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct amdzk_ctx amdzk_ctx;
typedef struct amdzk_srs amdzk_srs;

typedef enum {
  AMDZK_OK = 0,
  AMDZK_E_NO_DEVICE = -1,
  AMDZK_E_INVALID = -2,   /* bad argument (null pointer, size mismatch, k out of range) */
  AMDZK_E_HIP = -3,       /* a HIP runtime call failed */
  AMDZK_E_NOMEM = -4,
  AMDZK_E_UNSUPPORTED = -5
} amdzk_status;

/* basis selector for MSM: ParamsKZG.g (monomial) or ParamsKZG.g_lagrange */
#define AMDZK_BASIS_G 0
#define AMDZK_BASIS_G_LAGRANGE 1
/* The inclusive prefix sums of g_lagrange, S_i = g_lagrange[0] + ... + g_lagrange[i]: sum_i z[i] g_lagrange[i] =
 * sum_i d[i] S_i with d[i] = z[i] - z[i+1] (d[n-1] = z[n-1]), so a column that rarely changes from row to row is
 * committed through its few non-zero differences (the permutation products, create_proof). Derived, not uploaded and not
 * in the SRS file: built once per amdzk_srs when the first proving key whose circuit has permutation columns is made on
 * it (amdzk_keygen*, amdzk_pk_read); until then an MSM over this basis fails with AMDZK_E_INVALID. MSM only:
 * amdzk_srs_get does not serve it. */
#define AMDZK_BASIS_G_LAGRANGE_PREFIX 2

/* flags for amdzk_ntt_fr* */
#define AMDZK_NTT_SCALE_NINV 1u /* multiply the result by 1/2^log_n (EvaluationDomain::ifft's divisor) */

/* ---- context ------------------------------------------------------------------------------- */
int amdzk_init(int device_id, amdzk_ctx** out);
void amdzk_destroy(amdzk_ctx* ctx);
const char* amdzk_last_error(const amdzk_ctx* ctx);
/* ABI version of this header: major*1000 + minor. */
int amdzk_version(void);
/* "amdzk <abi> src=<16 hex digits> arch=gfx950": the hash is over the comment-stripped kernel sources and build flags the
 * binary was made from (csrc/Makefile stamps it; the same function as bench.kernel_src_hash()). A static string. */
const char* amdzk_build_info(void);
/* Run subsequent work of this ctx on an existing hipStream_t (e.g. torch's current stream);
 * NULL restores the ctx's own stream. */
int amdzk_set_stream(amdzk_ctx* ctx, void* hip_stream);
/* HIP's current device is per host thread; a ctx belongs to ONE device. Every entry point below pins the calling
 * thread to the ctx's device for the duration of the call and restores the caller's device afterwards, so a ctx
 * may be created on one thread and used from another (one call at a time). amdzk_ctx_device returns that device;
 * the *_check_affinity calls verify that the ctx's stream, workspaces and tables / a pointer / a proving key's
 * buffers really live there (AMDZK_E_INVALID with a message otherwise) — a cheap assertion for multi-GPU hosts. */
int amdzk_ctx_device(const amdzk_ctx* ctx);
int amdzk_ctx_check_affinity(amdzk_ctx* ctx);
int amdzk_ptr_check_affinity(amdzk_ctx* ctx, const void* dptr);
/* How this context's calls wait for the device: AMDZK_WAIT_SPIN (default; hipStreamSynchronize — lowest latency, the
 * waiting thread keeps a core busy) or AMDZK_WAIT_BLOCK: the thread POLLS a completion event — hipEventQuery, 20 us of
 * yielding, then 50-us sleeps — and leaves its core to the threads that have kernels to launch. Every polled wait ends up
 * to one sleep quantum (about 50 us) late and a proof has 8-10 of them, so a lone proof is about 0.3-0.5 ms slower; it is
 * for hosts that keep more proofs in flight than they have cores to spare — one GPU's share of an 8-GPU host is 2 cores on
 * the reference box, where spinning costs 17 % of the rate, DESIGN.md §5. (The runtime's own blocking waits are not used:
 * hipEventBlockingSync events still spin on this ROCm.) Default from AMDZK_HOST_WAIT=spin|block when the ctx is made.
 * A host process that runs the device with hipDeviceScheduleBlockingSync (hipSetDeviceFlags) gets polling waits on EVERY
 * host wait of this library whatever this setting says: amdzk_init reads hipGetDeviceFlags and the library then never
 * enters the runtime's blocking waits (first screen). */
#define AMDZK_WAIT_SPIN 0
#define AMDZK_WAIT_BLOCK 1
int amdzk_set_host_wait(amdzk_ctx* ctx, int mode);
int amdzk_sync(amdzk_ctx* ctx);

/* ---- device memory (plain hipMalloc'd bytes; any device pointer of the same GPU is accepted by
 *      the *_dev entry points, including torch tensors' data_ptr()) ------------------------- */
int amdzk_dev_alloc(amdzk_ctx* ctx, size_t bytes, void** dptr);
int amdzk_dev_free(amdzk_ctx* ctx, void* dptr);
int amdzk_dev_upload(amdzk_ctx* ctx, void* dptr, const void* host, size_t bytes);
int amdzk_dev_download(amdzk_ctx* ctx, void* host, const void* dptr, size_t bytes);
int amdzk_dev_memset(amdzk_ctx* ctx, void* dptr, int byte, size_t bytes);
/* Streaming one witness per proof (what a caller of create_proof after Circuit::synthesize,
 * /root/reference/src/lib.rs:328-397, does): synthesize into pinned host memory (amdzk_host_alloc), start the
 * upload of the NEXT proof's witness with amdzk_dev_upload_async — it runs on a second HIP stream of the ctx,
 * beside the kernels of the proof in progress — and call amdzk_upload_fence before the create_proof that reads
 * it: work submitted to the ctx after the fence runs after every upload issued before it. The fence never blocks
 * the host: uploads that have already finished (the pipelined case) cost one event query and put no dependency on
 * the ctx's stream; one still in flight is waited for on the device. The source of an asynchronous upload must stay untouched until a fence + amdzk_sync, or the
 * create_proof that follows the fence, has returned. */
int amdzk_host_alloc(amdzk_ctx* ctx, size_t bytes, void** hptr);
int amdzk_host_free(amdzk_ctx* ctx, void* hptr);
int amdzk_dev_upload_async(amdzk_ctx* ctx, void* dptr, const void* host, size_t bytes);
int amdzk_upload_fence(amdzk_ctx* ctx);

/* ---- SRS: replaces the resident part of poly::kzg::commitment::ParamsKZG {g, g_lagrange} [UP]
 * g, g_lagrange: n = 2^k G1Affine each (either may be NULL if that basis is never used).
 * The bases are uploaded once and expanded on the device into per-window multiples
 * (2^(c*w) * g[i]) so that every MSM is bucket-accumulation only (MSM). */
int amdzk_srs_upload(amdzk_ctx* ctx, const uint64_t* g, const uint64_t* g_lagrange, uint32_t k,
                     amdzk_srs** out);
/* ParamsKZG::setup(k, rng) [UP] with the trapdoor s supplied by the caller (as unsafe as upstream's
 * setup: tests and benchmarks only): g[i] = s^i G, g_lagrange[i] = L_i(s) G, built on the device.
 * g_out / g_lagrange_out (2^k G1Affine each, host) may be NULL.
 * s: four Montgomery words. Refused with AMDZK_E_INVALID, *out untouched and the ctx usable afterwards:
 *   - s >= r as words: no field element;
 *   - s^n = 1 (n = 2^k; s = 1 at every k): s is a point omega^i of the domain, s - omega^i has no inverse and
 *     every L_i(s) would come out 0. Upstream panics there (invert().unwrap()). */
int amdzk_srs_setup(amdzk_ctx* ctx, uint32_t k, const uint64_t s[4], amdzk_srs** out, uint64_t* g_out,
                    uint64_t* g_lagrange_out);
/* ParamsKZG::{write, read} [UP]: k (u32 LE) | n x g | n x g_lagrange (halo2curves 32-byte compressed
 * G1: x little-endian, bit 7 of byte 31 = parity of y, all-zero = identity) | g2 | s_g2 (64 bytes each,
 * opaque to the prover and passed through). Point (de)compression runs on the device; read rejects
 * encodings that are not on the curve. */
size_t amdzk_srs_serialized_size(uint32_t k);
int amdzk_srs_write(amdzk_ctx* ctx, const amdzk_srs* srs, const uint8_t g2[64], const uint8_t s_g2[64],
                    uint8_t* out, size_t cap);
int amdzk_srs_read(amdzk_ctx* ctx, const uint8_t* data, size_t len, amdzk_srs** out,
                   uint8_t g2_out[64], uint8_t s_g2_out[64]);
/* ParamsKZG::downsize(new_k) [UP]: params for a smaller domain from the same trapdoor: g[..2^new_k]
 * is kept and g_lagrange recomputed with arithmetic::g_to_lagrange (below). Upstream shrinks in place;
 * here a new handle is returned and `srs` stays valid (free both). Fails if new_k > k. */
int amdzk_srs_downsize(amdzk_ctx* ctx, const amdzk_srs* srs, uint32_t new_k, amdzk_srs** out);
/* ParamsKZG::get_g() [UP] (basis 0) / the g_lagrange vector (basis 1): 2^k G1Affine to the host. */
int amdzk_srs_get(amdzk_ctx* ctx, const amdzk_srs* srs, int basis, uint64_t* out);
void amdzk_srs_free(amdzk_ctx* ctx, amdzk_srs* srs);
/* arithmetic::g_to_lagrange(g_projective, k) [UP]: g_lagrange = (1/n) FFT_{omega^-1}(g) over G1 — radix-2
 * butterflies whose twiddle products are scalar multiplications — normalised to affine.
 * g, g_lagrange_out: 2^k G1Affine on the host. */
int amdzk_g_to_lagrange(amdzk_ctx* ctx, const uint64_t* g, uint32_t k, uint64_t* g_lagrange_out);

/* ---- MSM: replaces arithmetic::best_multiexp(coeffs, bases) as called from
 * ParamsKZG::commit / commit_lagrange [UP].
 * scalars: len x Fr (len <= 2^k; bases[0..len) are used, as `&g[..len]` in the original).
 * out: one normalised Jacobian point (12 x u64). */
int amdzk_msm_g1(amdzk_ctx* ctx, const amdzk_srs* srs, int basis, const uint64_t* scalars,
                 size_t len, uint64_t out_jacobian[12]);
/* ncols independent MSMs over the same bases in one submission (one per committed column). */
int amdzk_msm_g1_batch(amdzk_ctx* ctx, const amdzk_srs* srs, int basis,
                       const uint64_t* const* scalars, size_t ncols, size_t len,
                       uint64_t* out_jacobian /* ncols x 12 */);
/* Same, scalars already resident: column c starts at d_scalars + c*col_stride (in Fr elements). */
int amdzk_msm_g1_dev(amdzk_ctx* ctx, const amdzk_srs* srs, int basis, const void* d_scalars,
                     size_t ncols, size_t len, size_t col_stride,
                     uint64_t* out_jacobian /* host, ncols x 12 */);

/* Same over the resident table, but column c is read from d_cols[c]: a HOST array of ncols device pointers (any device
 * memory of this GPU, `len` Fr each) — columns that live in different buffers, committed in one submission without a copy.
 * This is the MSM amdzk_create_proof_batch commits a step of a whole batch with; only the counting sort's scalar loads
 * differ from amdzk_msm_g1_dev, and the points are equal word for word. Every d_cols[c] must be 16-byte aligned (the
 * kernel reads a scalar as two 16-byte loads; 32-byte alignment is not needed) and readable for len * 32 bytes; columns may
 * overlap or repeat. max_scratch_bytes: the workspace one submission may take; 0 = the library's default, which is what a
 * caller wants (16 GiB: at the k = 15 shape a column costs about 15 MiB of counting-sort and bucket lists, so a batch of
 * ten proofs' 1410 advice columns goes as two runs of 705 — five times the 141 columns that already fill the chip for one
 * proof — and two contexts hold their scratch in a ninth of the MI355X's 288 GB). A batch that needs more, or has more than
 * 65535 columns, is cut into the fewest equal runs of columns that fit; a smaller bound only makes more runs (tests use it
 * to reach that path at small sizes). */
int amdzk_msm_g1_cols_dev(amdzk_ctx* ctx, const amdzk_srs* srs, int basis, const void* const* d_cols,
                          size_t ncols, size_t len, size_t max_scratch_bytes,
                          uint64_t* out_jacobian /* host, ncols x 12 */);

/* ---- MSM over the caller's own bases: arithmetic::best_multiexp(coeffs, bases) [UP] wherever the bases are not a resident
 * ParamsKZG — the verifier's MSMKZG::eval, a commitment under other parameters, a one-off check, any len (no power of
 * two needed). No amdzk_srs and no window table: one bucket set per window and sum_w 2^(c w) S_w (DESIGN.md §3.1
 * "Caller-supplied bases"), so nothing is paid per point beyond the MSM itself. Slower per call than amdzk_msm_g1* over a
 * resident table; far faster than building a table for a few MSMs (INTEGRATION.md says where the routes cross).
 * bases: len G1Affine (64 B each, (0,0) = identity), any len; not modified. As upstream, points are NOT checked to be on
 * the curve. One normalised Jacobian point out; len = 0 gives the identity (0, 1, 0).
 * Refused with a message: null pointers, ncols = 0 (AMDZK_E_INVALID); ncols x windows > 65535, len >= 2^31
 * (AMDZK_E_UNSUPPORTED). The ctx stays usable. */
int amdzk_msm_g1_bases(amdzk_ctx* ctx, const uint64_t* scalars, const uint64_t* bases, size_t len,
                       uint64_t out_jacobian[12]);
/* ncols scalar columns over the same bases in one submission. */
int amdzk_msm_g1_bases_batch(amdzk_ctx* ctx, const uint64_t* const* scalars, size_t ncols,
                             const uint64_t* bases, size_t len, uint64_t* out_jacobian /* ncols x 12 */);
/* scalars and bases already resident (any device pointer of this GPU): column c at d_scalars + c*col_stride (Fr
 * elements, col_stride >= len), d_bases: len G1Affine, read only. */
int amdzk_msm_g1_bases_dev(amdzk_ctx* ctx, const void* d_scalars, size_t ncols, size_t len,
                           size_t col_stride, const void* d_bases,
                           uint64_t* out_jacobian /* host, ncols x 12 */);
/* What the three calls above will do for this shape: window bits, windows = ceil(255 / window bits), and the bytes of
 * workspace the ctx will hold for it (the copy of the bases included; the host-pointer forms stage scalars and bases in
 * ncols*len*32 + len*64 bytes more). Pure host code, callable without a device (like amdzk_debug_limb_program); the
 * same status as the calls for a shape they refuse. Any output pointer may be NULL. */
int amdzk_msm_g1_bases_plan(size_t ncols, size_t len, uint32_t* window_bits, uint32_t* windows,
                            size_t* scratch_bytes);

/* ---- NTT: replaces arithmetic::best_fft(a, omega, log_n) [UP] (rows a3, a4).
 * In place, natural order in, natural order out: a[j] <- sum_i a[i] * omega^(i*j). */
int amdzk_ntt_fr(amdzk_ctx* ctx, uint64_t* a, uint32_t log_n, const uint64_t omega[4],
                 uint32_t flags);
/* ncols resident columns, column c at d_a + c*col_stride (Fr elements), each of 2^log_n. */
int amdzk_ntt_fr_dev(amdzk_ctx* ctx, void* d_a, uint32_t log_n, const uint64_t omega[4],
                     uint32_t flags, size_t ncols, size_t col_stride);

/* ncols host vectors of 2^log_n in one submission. */
int amdzk_ntt_fr_batch(amdzk_ctx* ctx, uint64_t* const* cols, size_t ncols, uint32_t log_n,
                       const uint64_t omega[4], uint32_t flags);

/* ---- representation changes on resident data: Fr::from_raw (canonical 4 x u64 -> Montgomery) and
 * Fr::to_repr (Montgomery -> canonical), n elements in place. Values must be < r. */
int amdzk_fr_from_raw_dev(amdzk_ctx* ctx, void* d_a, size_t n);
int amdzk_fr_to_repr_dev(amdzk_ctx* ctx, void* d_a, size_t n);

/* ---- EvaluationDomain: replaces poly::domain::EvaluationDomain [UP] (rows a4-a6).
 * amdzk_domain_new(j, k) = EvaluationDomain::new(j, k): j = cs.degree(), n = 2^k,
 * extended_k = smallest e with 2^e >= n*(j-1). Columns are device-resident; `col_stride` and the
 * in/out strides are in Fr elements. */
typedef struct amdzk_domain amdzk_domain;
int amdzk_domain_new(amdzk_ctx* ctx, uint32_t j, uint32_t k, amdzk_domain** out);
void amdzk_domain_free(amdzk_ctx* ctx, amdzk_domain* dom);
uint32_t amdzk_domain_k(const amdzk_domain* dom);
uint32_t amdzk_domain_extended_k(const amdzk_domain* dom);
/* what: 0 omega, 1 omega_inv, 2 extended_omega, 3 extended_omega_inv, 4 g_coset (= Fr::ZETA),
 * 5 g_coset_inv, 6 ifft_divisor, 7 extended_ifft_divisor */
int amdzk_domain_constant(const amdzk_domain* dom, int what, uint64_t out[4]);
/* lagrange_to_coeff / coeff_to_lagrange: in place on ncols columns of 2^k. */
int amdzk_lagrange_to_coeff_dev(amdzk_ctx* ctx, const amdzk_domain* dom, void* d_cols, size_t ncols,
                                size_t col_stride);
int amdzk_coeff_to_lagrange_dev(amdzk_ctx* ctx, const amdzk_domain* dom, void* d_cols, size_t ncols,
                                size_t col_stride);
/* coeff_to_extended: 2^k coefficients in -> 2^extended_k evaluations on the zeta coset out
 * (distribute_powers_zeta, zero padding and the NTT in one pass structure). d_ext != d_coeff. */
int amdzk_coeff_to_extended_dev(amdzk_ctx* ctx, const amdzk_domain* dom, const void* d_coeff,
                                size_t in_stride, void* d_ext, size_t out_stride, size_t ncols);
/* extended_to_coeff: in place on 2^extended_k values; the first n*(j-1) entries are the result. */
int amdzk_extended_to_coeff_dev(amdzk_ctx* ctx, const amdzk_domain* dom, void* d_ext, size_t ncols,
                                size_t col_stride);
/* divide_by_vanishing_poly: a[i] *= 1/((zeta*extended_omega^i)^n - 1), in place. */
int amdzk_divide_by_vanishing_dev(amdzk_ctx* ctx, const amdzk_domain* dom, void* d_ext, size_t ncols,
                                  size_t col_stride);

/* ---- create_proof: replaces plonk::{keygen_pk, create_proof} [UP] for
 * KZGCommitmentScheme<Bn256> + ProverSHPLONK (or ProverGWC, AMDZK_MULTIOPEN_GWC) + Blake2bWrite/Challenge255
 * (or the EVM transcript, or the caller's own: amdzk_create_proof_opts), one circuit instance (amdzk_create_proof_multi:
 * several), advice in up to three challenge phases (amdzk_keygen_phased). The circuit arrives as plain data: what ConstraintSystem holds after
 * Circuit::configure (/root/reference/src/lib.rs:295-326 etc.) and selector compression.
 *
 * Expressions are postfix u32 words, op << 24 | payload:
 *   1 CONST  payload = index into `constants`      2 FIXED / 3 ADVICE / 4 INSTANCE
 *   5 NEG   6 ADD   7 MUL                              payload = column << 8 | (rotation + 128)
 *   8 SCALE  payload = index into `constants` (multiply the top of stack by that constant)
 *   9 CHALLENGE  payload = challenge index (Expression::Challenge; keys made by amdzk_keygen_phased only)
 * `expr_offsets[e] .. expr_offsets[e+1]` delimits expression e inside `expr_words`. The first
 * num_gates expressions are the gate polynomials in order; then, per lookup l,
 * lookup_shape[2l] input expressions followed by lookup_shape[2l+1] table expressions. */
typedef struct amdzk_circuit {
  uint32_t k, num_fixed, num_advice, num_instance, blinding_factors, cs_degree;
  uint32_t num_advice_queries;   const int32_t* advice_queries;   /* (column, rotation) pairs, query order */
  uint32_t num_fixed_queries;    const int32_t* fixed_queries;
  uint32_t num_instance_queries; const int32_t* instance_queries;
  uint32_t num_gates, num_lookups, num_exprs;
  const uint32_t* lookup_shape;  /* 2 x num_lookups */
  const uint32_t* expr_offsets;  /* num_exprs + 1 */
  const uint32_t* expr_words;
  uint32_t num_constants;        const uint64_t* constants;       /* Fr, Montgomery */
  uint32_t num_perm_columns;     const uint32_t* perm_columns;    /* (kind: 0 advice 1 fixed 2 instance, index) */
} amdzk_circuit;
typedef struct amdzk_pk amdzk_pk;
/* fixed_values: num_fixed x 2^k Fr (Lagrange, row-major per column). perm_mapping: for permutation
 * column i and row j the pair (i', j') of permutation::keygen::Assembly::mapping, as
 * perm_mapping[2*(i*n + j) + {0,1}]. transcript_repr: VerifyingKey::transcript_repr (upstream derives
 * it from the Debug string of the pinned VK; the caller supplies it). The proving key owns the
 * per-proof workspace: one proof at a time per key.
 * An expression is compiled in the order it is written, so a right-nested one, (a*b) + ((c*d) + (...)), holds one stack
 * entry per level; the stack lives in LDS. Every keygen (this one, _ex, _phased, _sigma, amdzk_pk_read) refuses a circuit
 * whose compiled programs need more LDS than the device gives a workgroup (its opt-in maximum of shared memory per
 * block) with AMDZK_E_UNSUPPORTED and a message that names the program, its depth and the depth that fits — about 30
 * levels at 160 KiB; nest to the left, ((a*b) + (c*d)) + ..., to stay shallow. The ctx stays usable. */
int amdzk_keygen(amdzk_ctx* ctx, const amdzk_srs* srs, const amdzk_circuit* circuit,
                 const uint64_t* fixed_values, const uint32_t* perm_mapping,
                 const uint64_t transcript_repr[4], amdzk_pk** out);
/* The same with the key's modes as explicit flags (amdzk_keygen takes them from the environment: AMDZK_FULL_COSETS=1,
 * AMDZK_SERIAL=1), so that two keys of one process can differ:
 *   AMDZK_KEYGEN_FULL_COSETS  evaluate the quotient numerator on all 2^(extended_k - k) cosets of upstream's extended
 *                             domain instead of cs_degree - 1 of them: upstream's own computation, byte-identical
 *                             also for witnesses that do NOT satisfy the circuit (satisfying ones are identical either way)
 *   AMDZK_KEYGEN_SERIAL       one proof's kernels on the caller's stream only, strictly one after another (no lanes:
 *                             see amdzk_create_proof) */
#define AMDZK_KEYGEN_FULL_COSETS 1u
#define AMDZK_KEYGEN_SERIAL 2u
int amdzk_keygen_ex(amdzk_ctx* ctx, const amdzk_srs* srs, const amdzk_circuit* circuit,
                    const uint64_t* fixed_values, const uint32_t* perm_mapping,
                    const uint64_t transcript_repr[4], uint32_t flags, amdzk_pk** out);
/* ---- challenge phases: ConstraintSystem::{advice_column_in, challenge_usable_after} [UP]. advice_phase[c] is the phase
 * (0, 1 or 2) of advice column c, challenge_phase[i] the phase after whose commitments challenge i is squeezed; expression
 * word 9 CHALLENGE names challenge i. As upstream: a phase above 0 needs an advice column in the phase before it, a
 * challenge's phase needs an advice column, every challenge index is below num_challenges — each violation is
 * AMDZK_E_INVALID with a message, and the ctx stays usable. phases = NULL is amdzk_keygen_ex (through it and amdzk_keygen a
 * CHALLENGE word is a bad expression word). A challenge is one more per-proof slot of the key's constant table, beside
 * theta, beta, gamma and y: nothing derived at keygen depends on its value, and a lookup whose table expression contains
 * one is compressed and sorted per proof. A table without later phases and without challenges gives exactly the key
 * amdzk_keygen_ex gives. */
typedef struct amdzk_phases {
  uint32_t num_challenges;
  const uint8_t* advice_phase;    /* num_advice */
  const uint8_t* challenge_phase; /* num_challenges */
} amdzk_phases;
int amdzk_keygen_phased(amdzk_ctx* ctx, const amdzk_srs* srs, const amdzk_circuit* circuit, const amdzk_phases* phases,
                        const uint64_t* fixed_values, const uint32_t* perm_mapping, const uint64_t transcript_repr[4],
                        uint32_t flags, amdzk_pk** out);
/* ---- keys that outlive the process: ProvingKey::read / ProvingKey::write [UP]. Upstream stores and reads back the sigma
 * columns (permutation::ProvingKey::permutations, Lagrange form), not the mapping they were made from.
 *
 * amdzk_keygen_sigma is amdzk_keygen_phased with those columns in place of perm_mapping: sigma_values is
 * num_perm_columns x 2^k Fr, Montgomery, Lagrange form, column after column — sigma_i(omega^j) = delta^i' omega^j' for
 * (i', j') = mapping[i][j]. Both routes share everything behind the upload of these columns, and a key made either way
 * from the same circuit is the same key. The values are NOT checked to be a permutation of delta^i omega^j, as upstream's
 * read does not check them. phases may be NULL. Refusals are keygen's: a null sigma_values with num_perm_columns > 0 is
 * AMDZK_E_INVALID, and the ctx stays usable. */
int amdzk_keygen_sigma(amdzk_ctx* ctx, const amdzk_srs* srs, const amdzk_circuit* circuit, const amdzk_phases* phases /* may be NULL */,
                       const uint64_t* fixed_values, const uint64_t* sigma_values, const uint64_t transcript_repr[4], uint32_t flags,
                       amdzk_pk** out);
/* The key's columns, for a fork's ProvingKey::write of a key made on the device. what: 0 the fixed columns (Lagrange),
 * 1 the sigma columns (Lagrange), 2 the fixed columns as coefficients, 3 the sigma columns as coefficients; num_fixed (or
 * num_perm_columns) x 2^k Fr, column after column. out = NULL queries *count (in Fr elements), as amdzk_pk_inspect does;
 * cap is in Fr elements. A workspace clone returns its root key's columns. */
int amdzk_pk_export(amdzk_ctx* ctx, const amdzk_pk* pk, int what, uint64_t* out, size_t cap /* Fr */, size_t* count);
/* The key file: everything keygen took except the SRS and the mode flags (AMDZK_KEYGEN_* describe a deployment, not a key:
 * amdzk_pk_read takes them as amdzk_keygen_ex does). Little-endian, no padding, deterministic for a given key, and
 * self-delimiting — `len` must be exactly the size the header implies:
 *   "AMDZKPK\0" (8 bytes) | format version u32 = 1
 *   amdzk_circuit in declaration order, as keygen's caller passed it: k, num_fixed, num_advice, num_instance,
 *     blinding_factors, cs_degree (u32 each) | num_advice_queries u32, advice_queries 2 x i32 each | the same for
 *     fixed_queries and instance_queries | num_gates, num_lookups, num_exprs (u32) | lookup_shape 2 x num_lookups u32 |
 *     expr_offsets (num_exprs + 1) u32 | expr_words expr_offsets[num_exprs] u32 | num_constants u32, constants 4 x u64 each |
 *     num_perm_columns u32, perm_columns 2 x u32 each
 *   has-phases u8 (1: keygen was given an amdzk_phases); if 1: num_challenges u32 | advice_phase num_advice x u8 |
 *     challenge_phase num_challenges x u8
 *   transcript_repr 4 x u64
 *   fixed commitments num_fixed x 64 B | permutation commitments num_perm_columns x 64 B (as amdzk_pk_commitments)
 *   fixed columns num_fixed x 2^k x 32 B | sigma columns num_perm_columns x 2^k x 32 B (Lagrange, Montgomery)
 *   BLAKE2b-512 (64 B) of all bytes before it, personalisation "amdzk_pk_blob_v1" (hashlib.blake2b(person=...))
 * Cosets and compiled programs are not stored: amdzk_pk_read rebuilds them with keygen's own transforms and commitments,
 * then compares the commitments it computed with the stored ones — a mismatch (AMDZK_E_INVALID, the message says that the
 * key was made under other parameters) is how a key file paired with the wrong SRS is caught. A key that was read is a
 * root key: amdzk_pk_clone_workspace, every amdzk_create_proof* and amdzk_pk_write (the same bytes again) work on it.
 * amdzk_pk_read keeps no pointer into `data`. Refused with AMDZK_E_INVALID and a message that starts "pk_read:", the ctx
 * usable afterwards: bad magic or version, any length mismatch or truncation, a digest mismatch, an internally
 * inconsistent header (the checks keygen makes on a circuit, and column / constant / challenge indices out of range), k
 * different from the SRS's. Columns are limited to 65536 of a kind (fixed, advice, instance, permutation: an expression
 * word addresses a column with 16 bits).
 * These header checks are stricter than keygen, which takes a circuit on trust where nothing it runs depends on it: every
 * query, used by an expression or not, must name a column of the circuit and a rotation in -128 .. 127, and every
 * expression must be a well-formed stack program. So that write followed by read never fails, amdzk_pk_write applies the
 * same checks to the key it is given: a key keygen accepted but amdzk_pk_read would refuse is not written
 * (AMDZK_E_INVALID, "pk_write: ..." with the reason), and amdzk_pk_serialized_size is 0 for it.
 * amdzk_pk_write: out = NULL queries *written; cap >= amdzk_pk_serialized_size(pk). Works on a clone (its root's file). */
size_t amdzk_pk_serialized_size(const amdzk_pk* pk);
int amdzk_pk_write(amdzk_ctx* ctx, const amdzk_pk* pk, uint8_t* out, size_t cap, size_t* written);
int amdzk_pk_read(amdzk_ctx* ctx, const amdzk_srs* srs, const uint8_t* data, size_t len, uint32_t flags, amdzk_pk** out);
/* The shape of a key file. Pure host code, callable without a device (like amdzk_msm_g1_bases_plan): it runs every check
 * amdzk_pk_read makes before touching the device — the digest included — and allocates nothing in proportion to a count
 * that `len` does not back. AMDZK_E_INVALID for a file amdzk_pk_read would refuse. Any output pointer may be NULL. */
int amdzk_pk_blob_info(const uint8_t* data, size_t len, uint32_t* k, uint32_t* num_fixed, uint32_t* num_advice,
                       uint32_t* num_perm_columns, uint32_t* num_challenges);
/* amdzk_pk_blob_info's verdict with its reason, also without a device: the same return code, and in msg (at most msg_cap
 * bytes, NUL-terminated; may be NULL) the message amdzk_pk_read would leave in its ctx for this file — "pk_read: bad magic
 * ...", "pk_read: digest mismatch ...", "pk_read: length mismatch ..." — or "" for a file it accepts. */
int amdzk_pk_blob_check(const uint8_t* data, size_t len, char* msg, size_t msg_cap);
void amdzk_pk_free(amdzk_ctx* ctx, amdzk_pk* pk);
int amdzk_pk_check_affinity(amdzk_ctx* ctx, const amdzk_pk* pk);
/* VerifyingKey commitments: fixed columns (num_fixed x G1Affine), permutation (num_perm_columns x G1Affine). */
int amdzk_pk_commitments(const amdzk_pk* pk, uint64_t* fixed_out, uint64_t* perm_out);
/* instances[c]: instance_lens[c] public inputs of instance column c (host). d_advice: num_advice
 * witness columns of 2^k rows, device-resident, column c at d_advice + c*advice_stride (untouched:
 * blinding happens on an internal copy). rng_seed: ChaCha20Rng::seed_from_u64(seed) drives every
 * Fr::random draw in upstream order. proof_out may be NULL to query *proof_len. */
int amdzk_create_proof(amdzk_ctx* ctx, amdzk_pk* pk, const uint64_t* const* instances,
                       const size_t* instance_lens, const void* d_advice, size_t advice_stride,
                       uint64_t rng_seed, uint8_t* proof_out, size_t proof_cap, size_t* proof_len);
/* Same with a choice of TranscriptWrite: Blake2bWrite/Challenge255 (32-byte compressed points,
 * little-endian scalars) or halo2-solidity-verifier's Keccak256Transcript/ChallengeEvm — the wire
 * format /root/reference/solidity_verifier_contract/contract.sol reads (64-byte uncompressed points,
 * 32-byte big-endian scalars, contract.sol:77-112). */
#define AMDZK_TRANSCRIPT_BLAKE2B 0
#define AMDZK_TRANSCRIPT_KECCAK256_EVM 1
/* OR into `transcript_kind` to open with poly::kzg::multiopen::ProverGWC instead of ProverSHPLONK
 * (SURVEY.md §8(a) row a12): one witness commitment W_z = (sum_j v^j p_j - sum_j v^j p_j(z)) / (X - z) per
 * distinct evaluation point z, points in first-seen query order. */
#define AMDZK_MULTIOPEN_GWC 0x100
int amdzk_create_proof_ex(amdzk_ctx* ctx, amdzk_pk* pk, const uint64_t* const* instances,
                          const size_t* instance_lens, const void* d_advice, size_t advice_stride,
                          uint64_t rng_seed, int transcript_kind, uint8_t* proof_out,
                          size_t proof_cap, size_t* proof_len);
/* ---- several circuit instances in ONE proof: upstream's create_proof(params, pk, &[circuit; N], &[instances; N], rng,
 * transcript) [UP] takes slices; the reference passes one circuit (/root/reference/src/lib.rs:299-300 uses
 * phase 0 only; later phases: amdzk_keygen_phased + amdzk_create_proof_opts). Per-circuit steps run circuit after circuit in upstream's order — instance
 * values absorbed, advice blinded and committed, lookups permuted, permutation products, lookup products, then the advice /
 * permutation / lookup evaluations and openings — while the challenges, the random polynomial and h(X) exist once (h folds the
 * instances' terms in one chain with y).
 * A key owns ONE instance's per-proof workspace: amdzk_pk_clone_workspace makes a handle that shares `pk`'s key material
 * (fixed / permutation columns and cosets, programs, domain) and owns one more workspace. It is a complete key for
 * amdzk_create_proof* too (the cheap way to several proofs of one circuit in flight). The handles of one key — the one
 * keygen returned and its clones — are freed (amdzk_pk_free) in any order: the last one frees the key material. */
int amdzk_pk_clone_workspace(amdzk_ctx* ctx, const amdzk_pk* pk, amdzk_pk** out);
/* pks[c]: instance c's workspace — the key or clones of it, pairwise different, all on this ctx's device.
 * instances[c][col] / instance_lens[c][col] and d_advice[c] (+ advice_stride) as for amdzk_create_proof_ex; one RNG stream
 * and one transcript for the whole proof. n_circuits = 1 is amdzk_create_proof_ex. More than one instance runs on the
 * caller's stream only (no lanes). */
int amdzk_create_proof_multi(amdzk_ctx* ctx, amdzk_pk* const* pks, size_t n_circuits,
                             const uint64_t* const* const* instances, const size_t* const* instance_lens,
                             const void* const* d_advice, size_t advice_stride, uint64_t rng_seed,
                             int transcript_kind, uint8_t* proof_out, size_t proof_cap, size_t* proof_len);
size_t amdzk_proof_size_multi(const amdzk_pk* pk, size_t n_circuits, int transcript_kind);
/* Exact byte length of the proof for this key, transcript and multiopen scheme (transcript_kind as for
 * amdzk_create_proof_ex, including AMDZK_MULTIOPEN_GWC); a function of the circuit shape only. (GWC writes one point per
 * distinct opening point: rotations equal modulo n count once.) */
size_t amdzk_proof_size(const amdzk_pk* pk, int transcript_kind);
/* For callers whose `R: RngCore` is not ChaCha20Rng::seed_from_u64: draw
 * amdzk_proof_random_count(pk) scalars with Fr::random(&mut rng) and pass them (Montgomery Fr, in
 * draw order); the prover consumes them exactly where upstream's create_proof draws. */
size_t amdzk_proof_random_count(const amdzk_pk* pk);
int amdzk_create_proof_scalars(amdzk_ctx* ctx, amdzk_pk* pk, const uint64_t* const* instances,
                               const size_t* instance_lens, const void* d_advice,
                               size_t advice_stride, const uint64_t* scalars, size_t scalar_count,
                               int transcript_kind, uint8_t* proof_out, size_t proof_cap,
                               size_t* proof_len);

/* ---- create_proof with challenge phases and / or a caller-owned transcript.
 * Order of a phased proof (upstream's create_proof at the pin): for each phase p = 0, 1, 2 and, inside it, for each
 * circuit instance: the instance's advice columns of phase p in column-index order get their blinding_factors + 1
 * blinding tails, one unused blind is drawn per column of the phase, the columns are committed and the commitments
 * written; after all instances one squeeze_challenge per challenge whose phase is p, in challenge-index order. theta
 * follows the last phase; everything behind theta is as for any proof. Fr::random draws: the advice block is phase, then
 * instance, then the phase's column tails, then its blinds; amdzk_proof_random_count and every later block are unchanged.
 *
 * amdzk_phase_fn: later-phase witnesses depend on the challenges, so the caller computes them in a callback. It is called
 * once per phase >= 1 (for all instances together) before the library reads that phase's columns from d_advice; phase-0
 * columns must be present when the proof starts. challenges: num_challenges x 4 words, Montgomery; those of phases not yet
 * finished are zero. Work the callback enqueues on hip_stream (the ctx's stream) is ordered before the read; anything
 * else must be complete when it returns. It may call amdzk_dev_*, amdzk_upload_fence and amdzk_sync on the same ctx, and no
 * proving function on the same key. A non-zero return ends the proof with AMDZK_E_INVALID (the workspace is left quiet, as
 * after any failed proof). A key with later phases proved without a callback is refused with a message. */
typedef int (*amdzk_phase_fn)(void* user, uint32_t phase, const uint64_t* challenges, uint32_t num_challenges, void* hip_stream);
/* A caller-owned TranscriptWrite (`&mut T: TranscriptWrite` on the other side): the library forwards every call and keeps
 * no bytes. Scalars are Montgomery Fr (4 words), points G1Affine (8 words), never the identity (the library refuses to write
 * it, as upstream's transcripts do). Every member returns 0 on success; non-zero ends the proof with AMDZK_E_INVALID.
 * squeeze_challenge writes a Montgomery Fr below the modulus; words that are not below it end the proof with
 * AMDZK_E_INVALID, "create_proof: a squeezed challenge is not below the modulus" ("multiopen: ..." for amdzk_multiopen_dev),
 * before the value is used — as the read transcripts' squeezes are refused (AMDZK_PROOF_BAD_TRANSCRIPT).
 * The challenges are then the CALLER's values, and some values have no proof here. Refused with AMDZK_E_UNSUPPORTED, the
 * transcript advanced by what was called (everything in front of that squeeze has been written) and the workspace quiet:
 *   beta = 0 on a key with permutation columns — "create_proof: the challenge beta is zero (probability 2^-254): the
 *     factored permutation terms need 1 / beta" (upstream proves it);
 *   x = 0 — "create_proof: the challenge x is zero (probability 2^-254): rotations of x coincide", before anything is
 *     evaluated at x (upstream merges the coinciding points by value and proves; the key's opening plan tells points apart
 *     by rotation mod n);
 *   SHPLONK's u equal to an opening point that is not in the first point set — "create_proof: the challenge u is one of the
 *     opening points (probability 2^-254)", behind the first opening commitment (upstream panics on 1 / z_0(u)); GWC has no
 *     such value.
 * y = 0 on a circuit whose last constraint vanishes is upstream's own refusal: an h(X) commitment is the identity. Every
 * other value — 0, 1, r - 1, a root of unity (x^n = 1 included), equal challenges — gives upstream's bytes. With a built-in
 * transcript each of these has the probability named. */
typedef struct amdzk_transcript {
  void* user;
  int (*common_point)(void* user, const uint64_t xy[8]);
  int (*common_scalar)(void* user, const uint64_t s[4]);
  int (*write_point)(void* user, const uint64_t xy[8]);
  int (*write_scalar)(void* user, const uint64_t s[4]);
  int (*squeeze_challenge)(void* user, uint64_t out[4]);
} amdzk_transcript;
/* size = sizeof(amdzk_proof_opts) as the caller compiled it (a smaller value than the fields below need is refused).
 * transcript_kind as for amdzk_create_proof_ex; with `transcript` set only its AMDZK_MULTIOPEN_GWC bit counts, proof_out
 * is unused and *proof_len comes back 0 (the bytes are the caller's). scalars != NULL: the caller's Fr::random draws
 * (amdzk_create_proof_scalars; scalar_count >= amdzk_proof_random_count(pk) for one instance), else ChaCha20Rng::seed_from_u64(rng_seed). */
typedef struct amdzk_proof_opts {
  size_t size;
  int transcript_kind;
  const amdzk_transcript* transcript; /* NULL: the built-in transcript transcript_kind names */
  amdzk_phase_fn phase_fn;            /* NULL: the key must have phase-0 advice only */
  void* phase_user;
  uint64_t rng_seed;
  const uint64_t* scalars;
  size_t scalar_count;
} amdzk_proof_opts;
/* pks / n_circuits / instances / instance_lens / d_advice as for amdzk_create_proof_multi (n_circuits = 1: one key). A key
 * without later phases and challenges takes exactly the path of amdzk_create_proof_multi and gives its bytes. */
int amdzk_create_proof_opts(amdzk_ctx* ctx, amdzk_pk* const* pks, size_t n_circuits,
                            const uint64_t* const* const* instances, const size_t* const* instance_lens,
                            const void* const* d_advice, size_t advice_stride, const amdzk_proof_opts* opts,
                            uint8_t* proof_out, size_t proof_cap, size_t* proof_len);

/* ---- a batch of independent proofs of ONE circuit from one host thread, advanced in lock-step on the caller's stream:
 * what a proving service, or a rank that owns a shard of a batch, calls instead of one thread and one ctx per proof in flight.
 * Each step of create_proof runs for all proofs of the batch before the next: a step's commitments of ALL proofs are one MSM
 * submission (amdzk_msm_g1_cols_dev's kernel: the columns stay in their workspaces), and each step has one host wait and
 * one download for the batch instead of one per proof (DESIGN.md §3.4 lists what is merged). Every proof has its own
 * transcript, RNG stream and challenges: proof b's bytes are exactly those of
 *   amdzk_create_proof_ex(ctx, pks[b], instances[b], instance_lens[b], d_advice[b], advice_stride, rng_seeds[b], transcript_kind, ..)
 * (with `scalars`: amdzk_create_proof_scalars), written to proofs_out + b*proof_stride with proof_lens[b] their length;
 * proof_stride >= amdzk_proof_size(pk, transcript_kind). n_proofs = 1 is that call.
 * pks[b]: the key or workspace clones of it (amdzk_pk_clone_workspace), pairwise different, all on this ctx's device — the
 * rule of amdzk_create_proof_multi. Instance lengths may differ between proofs. The batch runs on the caller's stream only
 * (no lanes, no latency mode of the commitments) whether the key was made with AMDZK_KEYGEN_SERIAL or not.
 * size = sizeof(amdzk_batch_opts) as the caller compiled it. rng_seeds: n_proofs seeds (ChaCha20Rng::seed_from_u64 each), or
 * scalars: per proof amdzk_proof_random_count(pk) caller-drawn Fr (scalar_count of them each); scalars wins if both are set.
 * Refused with a message, the ctx stays usable: AMDZK_E_UNSUPPORTED for a key with later phases or challenges
 * (amdzk_create_proof_opts proves those one at a time, amdzk_create_proof_batch_opts as a batch); AMDZK_E_INVALID for n_proofs = 0, null arguments, a too-small `size`, duplicate or
 * foreign workspaces, proof_stride too small, neither seeds nor scalars. A refused call starts no proof and says so for
 * every proof: statuses[b] (if given) = the returned status and proof_lens[b] (if given) = 0 for all b < n_proofs; its
 * message starts with "create_proof_batch:", never with "proof <b>:".
 * One bad witness does not cost the batch: a proof whose lookup input is not in its table, whose commitment is the identity
 * or whose beta is 0 (with a caller's transcript: any refusal listed at amdzk_transcript) gets its status in statuses[b] (may be NULL) and proof_lens[b] = 0 and drops out; the others finish
 * with their exact bytes. Returns AMDZK_OK if every proof succeeded, else the status of the first failing proof, whose usual
 * message amdzk_last_error carries behind "proof <b>: ". After a failure the workspaces are quiet, as after a failed single
 * proof. A HIP or out-of-memory error ends the whole batch with that status for every unfinished proof. */
typedef struct amdzk_batch_opts {
  size_t size;
  int transcript_kind;             /* as amdzk_create_proof_ex, AMDZK_MULTIOPEN_GWC included */
  const uint64_t* rng_seeds;       /* n_proofs seeds, or NULL if scalars is set */
  const uint64_t* const* scalars;  /* optional: per proof, the caller's Fr::random draws (amdzk_create_proof_scalars) */
  size_t scalar_count;
} amdzk_batch_opts;
int amdzk_create_proof_batch(amdzk_ctx* ctx, amdzk_pk* const* pks, size_t n_proofs,
                             const uint64_t* const* const* instances, const size_t* const* instance_lens,
                             const void* const* d_advice, size_t advice_stride, const amdzk_batch_opts* opts,
                             uint8_t* proofs_out, size_t proof_stride, size_t* proof_lens /* n_proofs */,
                             int* statuses /* n_proofs, may be NULL */);

/* ---- the lock-step batch for what amdzk_create_proof_batch refuses (ABI 1015): keys with challenge phases, proofs with a
 * caller-owned transcript, and DIFFERENT circuits in one batch. amdzk_create_proof_batch itself is unchanged.
 * Keys: pks[b] may be any key or workspace clone on this ctx's device, the handles pairwise different, all keys made on the
 * SAME amdzk_srs handle (hence the same k). Circuits, phase tables, proof sizes and random counts may differ from proof to
 * proof: the small circuits' commitments ride in the big one's MSM submissions.
 * Bytes: proof b's bytes, and the calls its caller's transcript receives, are exactly those of
 *   amdzk_create_proof_opts(ctx, &pks[b], 1, ..) with seed or scalars b, transcripts[b] and a callback that fills proof b's columns
 * (a key without phases: amdzk_create_proof_ex). A proof with its own transcript has proof_lens[b] = 0 and status 0.
 * proof_stride >= the largest amdzk_proof_size among the proofs with a built-in transcript; scalar_count >= every key's
 * amdzk_proof_random_count. transcript_kind: the built-in kind of the proofs without a transcript of their own; its
 * AMDZK_MULTIOPEN_GWC bit counts for all proofs.
 * Order: phases run p = 0 ... P - 1, P the largest phase count in the batch. In phase p every live proof whose key has the
 * phase copies in, blinds and transforms its columns of the phase; ONE MSM submission and one host wait commit them for the
 * whole batch; each proof then writes its points and squeezes its own challenges of phase p into its own constant table
 * (amdzk_pk_inspect(pks[b], 3, ..) afterwards returns proof b's challenges). A proof with fewer phases sits the later ones
 * out. Behind theta the batch is amdzk_create_proof_batch's. Host waits per batch: that call's, plus P - 1.
 * amdzk_batch_phase_fn: called once per phase p >= 1 for the WHOLE batch — never per proof — before that phase's copy-in, if
 * and only if some live proof's key has the phase. wanted[b] = 1: proof b is live and its key has advice columns in `phase`.
 * challenges: proof b's at challenges + 4 * b * challenge_stride (Montgomery; challenge_stride = the largest num_challenges
 * among the batch's keys): the values of the phases that have finished, zero elsewhere, all zero for proofs that dropped out
 * or are not wanted. Work enqueued on hip_stream is ordered before the copy-in. The callback may call, on the same ctx,
 * amdzk_dev_*, amdzk_upload_fence, amdzk_sync and amdzk_witness_run / amdzk_witness_run_dev on a handle of this ctx (one run
 * computes a phase's cells of the whole batch, the challenges among its inputs); no proving function on a key of the batch.
 * proof_rc (n_proofs, zero on entry): a non-zero proof_rc[b] drops proof b alone with AMDZK_E_INVALID ("proof b: .. the phase
 * callback refused it in phase p"); a non-zero return drops every wanted proof. The other proofs finish with their exact bytes.
 * transcripts: NULL, or n_proofs entries; a NULL entry = the built-in transcript. All five members must be set (checked up
 * front). They are called from the calling thread only, proof after proof in ascending b within a step; a non-zero return
 * drops that proof at the step boundary, as does a refusal to write the identity; a squeezed challenge that is not below
 * the modulus, or one of the degenerate values listed at amdzk_transcript, drops that proof before the value is used.
 * Failures are amdzk_create_proof_batch's: a failing proof gets its status, length 0 and "proof <b>: ..", the others finish —
 * proof 0 included; HIP and out-of-memory errors end the batch; the workspaces are quiet afterwards.
 * Refused as a whole with AMDZK_E_INVALID (every status = the returned code, every length 0, the message starts with
 * "create_proof_batch_opts:"): nulls, n_proofs = 0, a too-small `size`, neither seeds nor scalars, shared workspaces, a key
 * made on another amdzk_srs (the message names the proof), a key with advice in later phases while phase_fn is NULL, a null
 * transcript member, advice_stride < n, proof_stride or scalar_count too small, an unknown transcript kind. */
typedef int (*amdzk_batch_phase_fn)(void* user, uint32_t phase, size_t n_proofs, const uint8_t* wanted, const uint64_t* challenges,
                                    size_t challenge_stride, int* proof_rc, void* hip_stream);
typedef struct amdzk_batch_proof_opts {
  size_t size;
  int transcript_kind;                        /* built-in kind for proofs without their own transcript; the GWC bit counts for all */
  const uint64_t* rng_seeds;                  /* n_proofs seeds, or NULL if scalars is set */
  const uint64_t* const* scalars;             /* optional: per proof, the caller's Fr::random draws */
  size_t scalar_count;
  const amdzk_transcript* const* transcripts; /* NULL, or n_proofs entries; a NULL entry = built-in */
  amdzk_batch_phase_fn phase_fn;              /* NULL: every key must have phase-0 advice only */
  void* phase_user;
} amdzk_batch_proof_opts;
int amdzk_create_proof_batch_opts(amdzk_ctx* ctx, amdzk_pk* const* pks, size_t n_proofs,
                                  const uint64_t* const* const* instances, const size_t* const* instance_lens,
                                  const void* const* d_advice, size_t advice_stride, const amdzk_batch_proof_opts* opts,
                                  uint8_t* proofs_out, size_t proof_stride, size_t* proof_lens /* n_proofs */,
                                  int* statuses /* n_proofs, may be NULL */);

/* ---- the PLONK layer function by function: the kernels create_proof runs,
 * callable on their own on device-resident columns — for a fork that replaces upstream one function at a time and
 * for the isolated parity tests (tests/test_gpu_plonk_ops.py). Small operands come from the host. */
/* ff::BatchInvert [UP] in place: non-zero elements are inverted, zeros stay zero. */
int amdzk_batch_invert_dev(amdzk_ctx* ctx, void* d_a, size_t n);
/* poly::batch_invert_assigned [UP] (what create_proof does to the synthesized Assigned<F> cells before it commits to them,
 * SURVEY.md Appendix A step 3): out[i] = num[i] * den[i]^-1, zero where den[i] = 0. A Trivial cell is (x, 1), Zero is (0, 1);
 * d_den = NULL means all cells are trivial. In place (d_out = d_num) is allowed. */
int amdzk_batch_invert_assigned_dev(amdzk_ctx* ctx, const void* d_num, const void* d_den, size_t n, void* d_out);
/* The running product of permutation::prover::Argument::commit and lookup::prover::commit_product [UP]: column c
 * (n elements at d_cols + c*col_stride) is replaced by z with z[0] = 1, z[i] = z[i-1] * f[i-1]; with chain != 0 the
 * permutation argument's last_z is threaded through the columns: z_c[0] = z_{c-1}[chain_row]. */
int amdzk_grand_product_dev(amdzk_ctx* ctx, void* d_cols, size_t ncols, size_t n, size_t col_stride,
                            int chain, size_t chain_row);
/* permutation::prover::Argument::commit [UP] up to the blinding, on the columns pk's workspace holds (the advice and instance
 * columns of its last proof) and the given beta and gamma (Montgomery Fr): rows 0 ... usable (= 2^k - blinding_factors - 1)
 * of the product columns, nsets x (usable + 1) Fr, column after column, to `out` on the host. route 0: fractions, inversion
 * and running products over every row; 1: from the cells that are off the identity permutation alone, which a key lists
 * when they are at most half of its usable cells (refused otherwise); -1: the route pk's proofs take. Both give the same
 * words. *cells_out: the listed cells; *sparse_out: 1 when proofs take route 1 (either may be NULL; out = NULL only
 * queries them). Overwrites pk's per-proof workspace. */
int amdzk_perm_products_dev(amdzk_ctx* ctx, amdzk_pk* pk, const uint64_t beta[4], const uint64_t gamma[4], int route,
                            uint64_t* out, size_t* cells_out, int* sparse_out);
/* arithmetic::eval_polynomial [UP] for nq (polynomial, point) pairs: out[q] = d_polys[q](points[q]). d_polys: host
 * array of device pointers to n coefficients; points and out on the host. */
int amdzk_eval_poly_dev(amdzk_ctx* ctx, const void* const* d_polys, const uint64_t* points, size_t nq,
                        uint32_t n, uint64_t* out);
/* d_out = (accumulate ? d_out : 0) + sum_j coefs[j] * d_polys[j] over n coefficients (multiopen's linear
 * combinations). d_out must not alias an input. */
int amdzk_poly_axpy_dev(amdzk_ctx* ctx, const void* const* d_polys, const uint64_t* coefs, size_t m,
                        void* d_out, size_t n, int accumulate);
/* arithmetic::kate_division [UP] in place: a(X) -> (a(X) - a(root)) / (X - root); n coefficients, the top one 0. */
int amdzk_kate_div_dev(amdzk_ctx* ctx, void* const* d_polys, const uint64_t* roots, size_t npolys, uint32_t n);
/* poly::kzg::multiopen::{ProverSHPLONK, ProverGWC}::create_proof(params, rng, transcript, queries) [UP] (row a12) over the
 * CALLER's polynomials and points: the opening argument on its own, for a fork that keeps upstream's create_proof and swaps
 * only this, and for any use of the resident SRS as a KZG commitment scheme (commit, then open).
 * d_polys: host array of n_polys device pointers, 2^k coefficients each (k the SRS's), Montgomery; read only, may alias. A
 * polynomial's identity is its INDEX (upstream's PolynomialPointer compares addresses: map addresses to indices). points:
 * n_points x 4 words, Montgomery Fr, any values below r; two indices with equal values are one point. queries: (polynomial index,
 * point index) pairs in upstream's query order; duplicates are allowed. Entries of d_polys no query names are not read.
 * SHPLONK (scheme 0): queries are grouped commitment -> point set (first seen first), point set -> commitments (sets
 * compared as sorted values, first seen first), the super point set in ascending canonical order; squeeze y, squeeze v,
 * write [h(X)] with h = sum_i v^i (sum_j y^j (P_ij - R_ij)) / Z_{S_i}; squeeze u; write
 * [(sum_i v^i z_i(u) (L_i - R_i(u)) - Z_T(u) h) / (X - u) / z_0(u)]. Two points.
 * GWC (scheme AMDZK_MULTIOPEN_GWC): squeeze v; queries grouped by point value, points first seen first, a point's queries
 * in their order, duplicates kept; per point z write [(sum_j v^j p_j - sum_j v^j p_j(z)) / (X - z)]. One point per
 * distinct point value.
 * transcript: required; only squeeze_challenge and write_point are called, in the order above. evals: NULL, and the
 * evaluations p(z) are computed on the device; or n_queries x 4 words, evals[i] = the evaluation query i claims. Supplied
 * evaluations are TRUSTED, NOT CHECKED — as upstream trusts ProverQuery::eval: a wrong value gives no error here (and, since
 * every division drops its remainder as upstream's kate_division does, not even other points: what the verifier checks the
 * points against is the evaluation the CALLER wrote to the transcript, which this call never sees). SHPLONK reads the first
 * query of every (polynomial, point value) pair, GWC every query's own.
 * out_points (may be NULL): the written points, G1Affine, in write order, out_cap of them at most; *n_out (may be NULL)
 * their number. Scratch is the ctx's: one reservation of amdzk_multiopen_plan's scratch_bytes, grown on demand and kept
 * (shared with the other calls of this section); the call runs on the ctx's stream only and returns with it idle. No cap
 * on sets, points or queries but memory.
 * Refused with a message that starts "multiopen:", the ctx stays usable and the stream is idle: AMDZK_E_INVALID for null
 * arguments, a missing transcript or transcript member, a too-small opts->size, n_queries = 0, an index out of range, a
 * queried null polynomial, out_cap < n_out with out_points set, an SRS without AMDZK_BASIS_G, a point ("point <i> is not
 * below the modulus": every one of the n_points, queried or not) or a supplied evaluation ("evaluation <i> ...") that is not
 * below r — both before any scratch is reserved or the transcript touched —, a non-zero return of a transcript member, a
 * squeezed challenge that is not below r, and a commitment that is the identity (e.g. every queried polynomial zero: the
 * library refuses to write the identity, as upstream's transcripts do); AMDZK_E_UNSUPPORTED for SHPLONK's u equal to an
 * opening point outside the first point set ("the challenge u is one of the opening points": upstream panics on
 * 1 / z_0(u); behind the first written point); AMDZK_E_NOMEM when the scratch cannot be allocated. Every other challenge
 * and point value — 0, 1, r - 1, roots of unity, u on a point of the first set only — gives upstream's points. A refusal
 * after the first squeeze leaves the caller's transcript advanced by what was called. */
typedef struct amdzk_open_query {
  uint32_t poly;  /* index into d_polys */
  uint32_t point; /* index into points */
} amdzk_open_query;
typedef struct amdzk_multiopen_opts {
  size_t size;                        /* sizeof(amdzk_multiopen_opts) as the caller compiled it; too small is refused */
  int scheme;                         /* 0 SHPLONK, AMDZK_MULTIOPEN_GWC for GWC */
  const amdzk_transcript* transcript; /* required */
  const uint64_t* evals;              /* optional, n_queries x 4 Montgomery: trusted, not checked; NULL = computed */
} amdzk_multiopen_opts;
int amdzk_multiopen_dev(amdzk_ctx* ctx, const amdzk_srs* srs, const void* const* d_polys, size_t n_polys,
                        const uint64_t* points, size_t n_points, const amdzk_open_query* queries,
                        size_t n_queries, const amdzk_multiopen_opts* opts,
                        uint64_t* out_points /* may be NULL; n_out x 8 */, size_t out_cap, size_t* n_out);
/* What amdzk_multiopen_dev will do for these queries over polynomials of 2^k coefficients; pure host code, callable without
 * a device (like amdzk_msm_g1_bases_plan), the sets built exactly as the call builds them, and the call's status for a
 * shape it refuses. n_sets: SHPLONK's point sets, or GWC's distinct points. n_out: points written (2, or n_sets).
 * set_of_poly (may be NULL, n_polys entries): SHPLONK, the set polynomial i falls in; GWC, the first point (in write
 * order) polynomial i is opened at; UINT32_MAX for a polynomial no query names. Any output pointer may be NULL.
 * scratch_bytes = polys * 2^k * 32 + round_up(ptrs * 8, 256) + frs * 32, where with Q queries, E distinct (polynomial,
 * point value) pairs, C distinct queried polynomials, S = n_sets, P = sum_i |S_i| and M = max_i |S_i|:
 *   SHPLONK: polys = S + P + 1 (the L_i, the (set, point) quotients, h), ptrs = E + C + 2 P + S + 2,
 *            frs = 2 E + C + 2 P + P M + S + 3;
 *   GWC:     polys = S (the W_z), ptrs = E + Q + S, frs = 2 E + Q + 2 S.
 * (The MSM's and the kernels' own temporaries are the ctx's usual workspaces and are not in this figure.) */
int amdzk_multiopen_plan(const uint64_t* points, size_t n_points, const amdzk_open_query* queries,
                         size_t n_queries, size_t n_polys, uint32_t k, int scheme, uint32_t* n_sets,
                         uint32_t* n_out, size_t* scratch_bytes, uint32_t* set_of_poly);
/* lookup::prover::permute_expression_pair [UP] for nlookups pairs of n rows (column l at + l*n, Montgomery form):
 * d_inputs is sorted in place into A', d_permuted_tables_out receives S' (first occurrences aligned, leftovers in
 * ascending order assigned from the last repeated row backwards); rows >= usable come back zero for the caller to
 * blind. Only rows < usable of either column count: an input value that none of its table's rows < usable holds is
 * refused with AMDZK_E_INVALID "lookup <l> input not in table" (l: one of the failing lookups), the outputs are then
 * unspecified and the ctx stays usable. n: a power of two >= 2, usable <= n. usable = 0: nothing is permuted, the call
 * succeeds and both outputs are all zero. usable = n: the permutation of all n rows, no row is zeroed. nlookups = 0
 * succeeds and touches nothing. d_tables is only read. */
int amdzk_permute_expression_pair_dev(amdzk_ctx* ctx, void* d_inputs, const void* d_tables,
                                      void* d_permuted_tables_out, size_t nlookups, uint32_t n, uint32_t usable);
/* evaluation::Evaluator::evaluate_h + divide_by_vanishing_poly + extended_to_coeff + the split into pieces [UP]:
 * d_polys = the key's NP = A + I + 2L + nsets + L committed polynomials in coefficient form, n each, at
 * d_polys + i*poly_stride, in the order advice | instance | A' | S' | permutation products | lookup products;
 * challenges as Montgomery Fr. Writes the cs_degree - 1 pieces of h(X) (n coefficients each, consecutive) to
 * d_pieces_out. Overwrites the key's per-proof workspace. */
int amdzk_quotient_eval_dev(amdzk_ctx* ctx, amdzk_pk* pk, const void* d_polys, size_t poly_stride,
                            const uint64_t theta[4], const uint64_t beta[4], const uint64_t gamma[4],
                            const uint64_t y[4], void* d_pieces_out);
/* What the last create_proof on this key left in its workspace (test hook): what = 0 the NP committed polynomials in
 * coefficient form [NP][n]; 1 the challenges theta, beta, gamma, y; 2 the pieces of h(X) [cs_degree - 1][n]; 3 the
 * num_challenges phase challenges of the last proof (amdzk_keygen_phased). out may be NULL to query *count (in Fr elements). */
int amdzk_pk_inspect(amdzk_ctx* ctx, const amdzk_pk* pk, int what, uint64_t* out, size_t cap, size_t* count);

/* ---- check a witness: the constraint checks of dev::MockProver::verify [UP] on the device — does this witness satisfy this
 * circuit, and if not, which constraints fail and where? What every test of the reference calls (MockProver::run + verify)
 * before any proof is made; instances / instance_lens / d_advice / advice_stride as for amdzk_create_proof (the advice is
 * read as it is: no blinding). The call returns AMDZK_OK whenever the check RAN, whether or not the witness is good:
 * *n_failures is the number of constraints with at least one failing row (the witness satisfies the circuit iff it is 0),
 * and `out` receives the first min(cap, *n_failures) entries ordered by kind, then by index; out = NULL only queries the
 * count. One entry per failing constraint, never per row: `count` failing rows and the smallest of them, `first_row`;
 * `reserved` is 0.
 *
 * Semantics: upstream's MockProver::verify_at_rows(usable, usable) without its region and cell-assignment bookkeeping,
 * which does not cross this boundary. n = 2^k and u = n - (blinding_factors + 1).
 *   Gates. Gate polynomial g fails at row r < u when it evaluates to a non-zero residue there. Rotations wrap modulo n.
 *     Cells at rows >= u are read as they are: the key's fixed values, the caller's advice, and 0 for instance columns
 *     beyond instance_lens. A gate failing only at rows >= u is not reported. (Upstream would call a usable-row gate that
 *     reads such cells "poisoned" and fail it; this check does not: it evaluates what is there.)
 *   Lookups. Lookup l fails at row r < u when the tuple of its input expressions at r equals no tuple of its table
 *     expressions at any row < u. The search runs on theta-compressed values, with theta taken from theta_seed. A
 *     single-expression lookup is exact. With m expressions a false accept needs a root of a degree-(m - 1) polynomial in
 *     a theta chosen independently of the witness: at most u (m - 1) / r per row (r the order of the field, about 2^254).
 *     There are no false rejects.
 *   Copies. Permutation column i fails at row j, over all n rows, when the value of cell (i, j) differs from the value of
 *     the cell (i', j') that sigma_i(omega^j) = delta^i' omega^j' names. A broken two-cycle therefore reports both of its
 *     columns.
 *   Phases and instances. A phased key (amdzk_keygen_phased) takes the caller's challenge values, so a fork can check phase
 *     by phase. The call checks one circuit instance; for N instances the caller loops.
 *   Workspace. The call overwrites the key's per-proof workspace, as amdzk_quotient_eval_dev does. It runs on the ctx's
 *     stream only and returns with that stream idle. It works on root keys, workspace clones, keys from amdzk_keygen_sigma,
 *     and keys read from a key file. The first check on a key decodes its sigma columns back to (column, row) pairs —
 *     2^k x num_perm_columns x 8 bytes, kept with the root key, shared by its clones, never written to the key file.
 * Field values (advice, instances, challenges) must be below the modulus, as everywhere in this header.
 * Refused with a message that starts "check_witness:", the ctx and the key stay usable — AMDZK_E_INVALID for: null arguments;
 * an instance column longer than u ("instance column <c> too long (InstanceTooLarge)", create_proof's wording); missing
 * challenges, or challenges of the wrong number, for a key that has them (and challenges for a key that has none); a
 * too-small opts->size; a sigma value that is not delta^i omega^j for a column and row of this circuit (amdzk_keygen_sigma
 * does not check its input) — the message names the column and the row. */
#define AMDZK_CHECK_GATE   0  /* index = gate polynomial (expression e < num_gates) */
#define AMDZK_CHECK_LOOKUP 1  /* index = lookup l */
#define AMDZK_CHECK_COPY   2  /* index = position in perm_columns */
typedef struct amdzk_check_failure {
  uint32_t kind;
  uint32_t index;
  uint32_t first_row;
  uint32_t reserved;
  uint64_t count;
} amdzk_check_failure;
typedef struct amdzk_check_opts {
  size_t size;                 /* sizeof(amdzk_check_opts) as compiled by the caller; too small is refused */
  uint64_t theta_seed;         /* the theta that compresses multi-expression lookups: first Fr::random of ChaCha20Rng::seed_from_u64 */
  const uint64_t* challenges;  /* num_challenges x 4, Montgomery; required iff the key has challenges */
  uint32_t num_challenges;
} amdzk_check_opts;
int amdzk_check_witness(amdzk_ctx* ctx, amdzk_pk* pk, const uint64_t* const* instances, const size_t* instance_lens,
                        const void* d_advice, size_t advice_stride, const amdzk_check_opts* opts /* NULL: defaults */,
                        amdzk_check_failure* out, size_t cap, size_t* n_failures);

/* ---- verify proofs up to the pairing: plonk::verify_proof [UP] for one proof or a batch, everything except the one pairing.
 * For every well-formed proof b the call re-derives the transcript, computes the vanishing identity at x from the proof's
 * evaluations (l_0, l_last, l_blind in closed form, instance columns from the public inputs) and folds the opening
 * argument into two G1 sums, as upstream's verifier does before it hands a guard to its strategy:
 *   SHPLONK  L_b = z_0(u) h2      R_b = sum_i v^i z_i(u) sum_j y^j (C_ij - r_ij(u) G) - Z_T(u) h1 + u z_0(u) h2
 *   GWC      L_b = sum_i u^i W_i  R_b = sum_i u^i (z_i W_i + C_i - e_i G)
 * with G = g[0] of the key's SRS and the h(X) commitment expanded into its pieces with powers of x^n. The result is
 * L = sum_b rho_b L_b and R = sum_b rho_b R_b in pair_out (L then R, G1Affine, (0, 0) = the identity):
 *   every well-formed proof of the batch is valid  <=>  e(L, [s]_2) = e(R, [1]_2)     (up to the choice of rho)
 * The pairing stays with the caller, who holds s_g2 (AccumulatorStrategy / BatchVerifier pair once per batch, SingleStrategy
 * once per proof); G2 stays opaque to this library. rho_b belongs to position b of the batch, whichever proofs drop out.
 * rho MUST be unpredictable to whoever made the proofs: take combine_seed from the operating system's generator for every
 * call, or pass your own combine_scalars. (n_proofs = 1 without combine_scalars uses rho_0 = 1: one proof's pair is
 * deterministic.) After a failed pairing, find the culprit by calling again on subsets of the batch.
 *
 * instances[b * n_circuits + c][col] / instance_lens[...][col]: the public inputs of circuit instance c of proof b, as for
 * amdzk_create_proof_multi. proofs[b] / proof_lens[b]: the bytes amdzk_create_proof* wrote with a built-in transcript; a proof
 * made with any other transcript is read through opts->transcripts[b] (amdzk_transcript_read, below).
 * Keys with challenge phases are read in upstream's phased order; n_circuits > 1 reads what amdzk_create_proof_multi wrote.
 *
 * The call returns AMDZK_OK whenever it RAN, as amdzk_check_witness does. A malformed proof gets its status and offset in
 * statuses[b] and drops out of both sums; the others are unaffected. If no proof is well formed both points are the
 * identity. A well-formed proof that is FALSE is not detected here: it makes the pair fail the caller's pairing.
 * Decoding (point decompression with its curve check, range checks, Montgomery conversion) runs in one launch over every
 * (proof, element) pair; the sums are one two-column MSM over the decoded points, the key's commitments and G. Two host
 * waits per call. The call does not touch the key's per-proof workspace (a proof may be running on the key from another
 * ctx); it uses only the ctx's scratch, runs on the ctx's stream and returns with it idle. Works on root keys, workspace
 * clones and keys read from a key file.
 * Refused with a message that starts "verify_proofs:", the ctx and the key stay usable — AMDZK_E_INVALID for: null
 * arguments; n_proofs = 0; a too-small opts->size; an unknown transcript kind; a combine_scalars entry >= r.
 * opts = NULL: Blake2b + SHPLONK, one circuit instance, combine_seed 0 (one proof, or tests). */
#define AMDZK_PROOF_WELL_FORMED 0
#define AMDZK_PROOF_BAD_LENGTH 1   /* proof_lens[b] != amdzk_proof_size_multi(pk, n_circuits, transcript_kind) */
#define AMDZK_PROOF_BAD_POINT 2    /* x or y >= q, not on the curve, or the identity's encoding */
#define AMDZK_PROOF_BAD_SCALAR 3   /* an evaluation >= r */
#define AMDZK_PROOF_BAD_INSTANCE 4 /* an instance value >= r, or a column longer than the usable rows */
typedef struct amdzk_proof_status {
  uint32_t status;
  uint32_t offset; /* byte offset of the first offending element in the proof (BAD_POINT, BAD_SCALAR; for a proof read through a
                      transcript: the element's index in read order); the column index for BAD_INSTANCE; the completed read_*
                      calls for BAD_TRANSCRIPT; else 0 */
} amdzk_proof_status;
/* A caller-owned TranscriptRead (`&mut T: TranscriptRead` on the other side; ABI 1013), the mirror image of amdzk_transcript:
 * the library asks the caller's transcript for every element of the proof and for every challenge, keeps no hash of its own for
 * such a proof and uses the challenges the callback returns — the Fiat-Shamir binding is the caller's transcript's business,
 * as upstream. read_point writes a G1Affine (8 words, Montgomery), read_scalar and squeeze_challenge a Montgomery Fr (4 words).
 * Every member returns 0 on success. For proof b with opts->transcripts[b] set the library calls, from the calling thread,
 * proof after proof in ascending b and never concurrently: common_scalar(transcript_repr); one common_scalar per public input
 * (circuit instance, then column, then row); then read_point / read_scalar / squeeze_challenge in exactly the order
 * amdzk_create_proof_opts documents for write_point / write_scalar / squeeze_challenge (phases, N circuit instances, SHPLONK
 * or GWC). common_point is part of the interface and is not called by the verifier.
 * What read_point / read_scalar hand back is NOT trusted: it is checked in the same decode launch as the bytes of the other
 * proofs — a point must have both coordinates < q, be on y^2 = x^3 + 3 and not be (0, 0) (AMDZK_PROOF_BAD_POINT), a scalar
 * must be < r (AMDZK_PROOF_BAD_SCALAR); `offset` is then the element's index in read order. There is no conversion.
 * AMDZK_PROOF_BAD_TRANSCRIPT: a member returned non-zero, a member is NULL, a squeezed challenge is >= r, or the squeezed x
 * is degenerate — x = 0 (the rotations of x coincide; the prover refuses it too) or x^n = 1 (the vanishing identity divides by
 * x^n - 1: upstream's verifier panics); `offset` = the number of read_* calls completed for that proof (for a degenerate x:
 * the reads in front of x's squeeze), and no further member is called for it. The proof drops out like any malformed
 * proof; the single-key, _vk and _mixed calls and their decide forms report it alike. Every other challenge value is
 * folded as upstream folds it: u on an opening point gives upstream's pair, whose L may be the identity (verdict 0). */
typedef struct amdzk_transcript_read {
  void* user;
  int (*common_point)(void* user, const uint64_t xy[8]);
  int (*common_scalar)(void* user, const uint64_t s[4]);
  int (*read_point)(void* user, uint64_t xy_out[8]);
  int (*read_scalar)(void* user, uint64_t s_out[4]);
  int (*squeeze_challenge)(void* user, uint64_t out[4]);
} amdzk_transcript_read;
#define AMDZK_PROOF_BAD_TRANSCRIPT 5 /* the caller's read transcript failed or squeezed x = 0 or an x with x^n = 1 (amdzk_transcript_read) */
/* size: sizeof(amdzk_verify_opts) as compiled by the caller. The size of the struct before `transcripts` was added (every
 * field in front of it) stays accepted and means transcripts = NULL; any other smaller value is refused.
 * transcripts: NULL, or n_proofs entries. transcripts[b] == NULL: proof b is the bytes proofs[b] / proof_lens[b] read with the
 * built-in transcript of transcript_kind; else proof b comes from that transcript, proofs[b] / proof_lens[b] are not read
 * (proofs / proof_lens may be NULL when every proof has a transcript) and of transcript_kind only AMDZK_MULTIOPEN_GWC counts.
 * One batch may mix both. With transcripts == NULL nothing changes: pair_out, statuses and verdicts are word for word those
 * of a library without the field. */
typedef struct amdzk_verify_opts {
  size_t size;
  int transcript_kind;             /* as amdzk_create_proof_ex, AMDZK_MULTIOPEN_GWC included */
  uint32_t n_circuits;             /* circuit instances per proof (amdzk_create_proof_multi); 0 means 1 */
  uint64_t combine_seed;           /* rho_b = the b-th Fr::random of ChaCha20Rng::seed_from_u64(combine_seed) ... */
  const uint64_t* combine_scalars; /* ... or the caller's own: n_proofs x 4 words, Montgomery; wins if set */
  const amdzk_transcript_read* const* transcripts; /* NULL, or n_proofs caller-owned read transcripts (NULL entries: bytes) */
} amdzk_verify_opts;
int amdzk_verify_proofs(amdzk_ctx* ctx, const amdzk_pk* pk, size_t n_proofs, const uint64_t* const* const* instances,
                        const size_t* const* instance_lens, const uint8_t* const* proofs, const size_t* proof_lens,
                        const amdzk_verify_opts* opts /* NULL: defaults */, amdzk_proof_status* statuses /* n_proofs */,
                        uint64_t pair_out[16]);

/* ---- pairing: BN254 optimal ate on the device, and proofs DECIDED in one call.
 * Conventions are the published BN254 / EIP-197 ones (csrc/fq12.cuh states them; the reference repository holds no G2 data, so
 * parity is unpinned): Fq2 = Fq[u]/(u^2 + 1), xi = 9 + u, Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v); G2 = the order-r
 * subgroup of the twist y^2 = x^3 + 3/xi; EIP-197's G2 generator; e(P, Q) = f^((p^12 - 1)/r) with the EXACT exponent (the fixed
 * power c of a Fuentes-Castaneda style chain is c = 1), so a GT value is canonical and comparable across implementations.
 * In-memory formats are halo2curves':
 *   G2Affine : {x.c0, x.c1, y.c0, y.c1}, 16 x u64, Montgomery R = 2^256; all zero is the identity            (128 B)
 *   Gt / Fq12: 12 Fq in declaration order c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1, 48 x u64               (384 B)
 *
 * amdzk_g2: ONE G2 point prepared for pairing — the line coefficients of every step of the Miller loop (halo2curves'
 * G2Prepared), computed on the host and resident on the ctx's device. amdzk_g2_prepare refuses, with AMDZK_E_INVALID and a
 * message that starts "g2_prepare:": null arguments, a coordinate >= q, a point that is not on the twist, the identity.
 * Membership in the order-r subgroup is NOT checked (as for in-memory points upstream): a point of the twist outside G2
 * gives a meaningless GT value, never a fault. Free with amdzk_g2_free once no call is using it. */
typedef struct amdzk_g2 amdzk_g2;
int amdzk_g2_prepare(amdzk_ctx* ctx, const uint64_t q[16], amdzk_g2** out);
void amdzk_g2_free(amdzk_ctx* ctx, amdzk_g2* g2);
/* The G2 half of ParamsKZG::setup [UP] with the caller's trapdoor s (Montgomery, as for amdzk_srs_setup, and as unsafe):
 * g2 = the generator, s_g2 = s * g2. Host work. The 64-byte compressed G2 encoding of the SRS file is NOT produced here
 * (amdzk_g2_compress below makes it): amdzk_srs_write / amdzk_srs_read keep passing those fields through. */
int amdzk_g2_setup(amdzk_ctx* ctx, const uint64_t s[4], uint64_t g2_out[16], uint64_t s_g2_out[16]);
/* The 64-byte G2 fields of the SRS file <-> G2Affine words, and membership in G2. Pure host code with no ctx,
 * callable without a device (csrc/g2codec.hpp). The format is halo2curves 0.3.1's G2Compressed, made by the macro that makes the
 * 32-byte G1 form of amdzk_srs_write: bytes 0-31 x.c0 and bytes 32-63 x.c1, canonical little-endian; bit 7 of byte 63 = the
 * parity of the canonical y.c0; bit 6 of byte 63 is always 0 (x.c1 < q < 2^254); 64 zero bytes <-> the identity (16 zero words).
 * Like the G1 sign bit the convention is recalled, not pinned by a fixture.
 * amdzk_g2_compress refuses what amdzk_g2_prepare refuses except the identity: a coordinate >= q, a point off the twist.
 * amdzk_g2_decompress clears bit 7, refuses an x.c0 or x.c1 >= q (a set bit 6 is one), gives the identity for x = 0 with a clear
 * sign bit and refuses x = 0 with the bit set; otherwise y = sqrt(x^3 + 3/xi) in Fq2 with the root whose y.c0 has the bit's
 * parity, and a non-residue is refused. The result is on the twist; membership in G2 is amdzk_g2_check's business.
 * Every refusal is AMDZK_E_INVALID with a message that starts "g2_compress:" / "g2_decompress:", written NUL-terminated into
 * msg (msg_cap bytes; msg may be NULL); "" on success.
 * amdzk_g2_check: *status = 0 in G2 | 1 a coordinate >= q | 2 not on the twist | 3 the identity | 4 on the twist, outside the
 * order-r subgroup ([r]Q != O: the definition, 254 doublings on the host). Returns AMDZK_E_INVALID for a null argument only. */
int amdzk_g2_compress(const uint64_t q[16], uint8_t out[64], char* msg, size_t msg_cap);
int amdzk_g2_decompress(const uint8_t in[64], uint64_t q_out[16], char* msg, size_t msg_cap);
int amdzk_g2_check(const uint64_t q[16], int* status);
/* n independent products over the same m prepared points: gt_i = prod_{j<m} e(P[i*m + j], Q_j).
 * g1: n*m G1Affine (host); (0,0) = the identity, which contributes the factor 1 — so a product whose G1 entries are ALL the
 * identity is 1 and reads is_one = 1. Points are NOT checked to be on the curve (as the MSM's bases).
 * is_one (n bytes, may be NULL): gt_i == 1.  gt_out (n x 48 words, may be NULL).
 * One lane per (product, pair) for the Miller loops, one lane per product for the final exponentiation: a lone product is
 * SLOWER than a CPU's pairing; n products cost about the latency of one while n stays below the chip's lane count
 * (profiles/pairing.txt). Refused with AMDZK_E_INVALID and "pairing_products:": nulls, m = 0, n = 0, m above
 * AMDZK_PAIRING_MAX_M, n above 2^20; the ctx stays usable. Runs on the ctx's stream and returns with it idle. */
#define AMDZK_PAIRING_MAX_M 16
int amdzk_pairing_products(amdzk_ctx* ctx, const amdzk_g2* const* qs, size_t m, const uint64_t* g1, size_t n, uint8_t* is_one,
                           uint64_t* gt_out);
/* Is this SRS an SRS? The structure of the resident g / g_lagrange against the file's g2 / s_g2 (G2Affine words, e.g. from
 * amdzk_g2_decompress), checked on the device with the table MSM, the NTT and the pairing. With n = 2^k and a
 * random rho:  A = sum_{i<=n-2} rho^i g[i],  B = sum_{i<=n-2} rho^i g[i+1],  C = sum_j c_j g[j] with c = the coefficients of the
 * polynomial that is rho^i at omega^i (inverse NTT with the domain's omega^-1 and 1/n),  E = sum_i rho^i g_lagrange[i].
 *   AMDZK_SRS_CHECK_G2       amdzk_g2_check gives status 0 for g2 and for s_g2 (host).
 *   AMDZK_SRS_CHECK_CURVE    every resident g[i], g_lagrange[i] has coordinates < q, is on y^2 = x^3 + 3 and is not (0, 0);
 *                            report->curve_basis / curve_index name the first offender, G before G_LAGRANGE, smallest index.
 *   AMDZK_SRS_CHECK_POWERS   A and B are not the identity and e(A, s_g2) e(-B, g2) = 1. n = 1 has no pair g[i], g[i+1]: the
 *                            check ran and passes vacuously (A = B = the identity).
 *   AMDZK_SRS_CHECK_LAGRANGE C = E as points.
 * Order and dependence: G2, then CURVE, then POWERS, then LAGRANGE. A check that cannot mean anything is NOT RUN, its bit of
 * report->ran stays clear: POWERS and LAGRANGE when CURVE was run and failed (an MSM over off-curve points means nothing);
 * POWERS when g2 or s_g2 has a non-zero amdzk_g2_check status (report->g2_status is filled whether or not G2 was asked for);
 * LAGRANGE when POWERS was not run or failed (it is sound only given POWERS); and any check that reads a basis which is not
 * resident (amdzk_srs_upload with a NULL pointer) — CURVE goes over the bases that are. The SRS is consistent iff
 * report->failed == 0 and report->ran covers what was asked. report->points: A, B, C, E as G1Affine, (0, 0) = the identity,
 * zero where the sum was not computed: for tests and diagnosis.
 * Soundness (derived, not measured). If some g[i+1] != s g[i] (s defined by s_g2 = s g2), the discrete logarithm of B - s A is
 * a non-zero polynomial of degree <= n - 2 in rho. Given POWERS, g[j] = s^j g[0] and C = p(s) g[0] for the polynomial p above,
 * while E = sum_i rho^i g_lagrange[i]: a wrong g_lagrange[i] makes E - C a non-zero polynomial of degree <= n - 1 in rho. So a
 * bad SRS passes with probability at most (2n - 3)/r over rho — for a rho that whoever made the file could not know. rho is the
 * first Fr::random of ChaCha20Rng::seed_from_u64(opts->seed) (as amdzk_check_opts.theta_seed), so a 64-bit seed from the OS
 * generator bounds a guessing adversary at 2^-64; pass opts->rho (4 words, Montgomery, < r; wins if set) for the full bound.
 * Not checked: the derived prefix-sum basis and the window tables, which are the library's own work.
 * Returns AMDZK_OK whenever it ran, whatever it found (as amdzk_check_witness). Refused with AMDZK_E_INVALID and "srs_check:":
 * null srs / g2 / s_g2 / report, an opts->size below this library's, unknown check bits, rho >= r; the ctx stays usable. Runs
 * on the ctx's stream and returns with it idle. */
#define AMDZK_SRS_CHECK_G2       1u
#define AMDZK_SRS_CHECK_CURVE    2u
#define AMDZK_SRS_CHECK_POWERS   4u
#define AMDZK_SRS_CHECK_LAGRANGE 8u
typedef struct amdzk_srs_check_opts {
  size_t size;         /* sizeof(amdzk_srs_check_opts) as compiled by the caller; too small is refused */
  uint32_t checks;     /* AMDZK_SRS_CHECK_* bits; 0 = all */
  uint64_t seed;       /* rho = first Fr::random of ChaCha20Rng::seed_from_u64(seed) ... */
  const uint64_t* rho; /* ... or the caller's own, 4 words Montgomery, < r; wins if set */
} amdzk_srs_check_opts;
typedef struct amdzk_srs_report {
  uint32_t ran;           /* bit per check that ran */
  uint32_t failed;        /* bit per check that ran and failed */
  uint32_t g2_status[2];  /* amdzk_g2_check of g2, s_g2 */
  uint32_t curve_basis;   /* CURVE failed: AMDZK_BASIS_G or AMDZK_BASIS_G_LAGRANGE of the first offending point ... */
  uint32_t reserved;
  uint64_t curve_index;   /* ... and its index; 0, 0 otherwise */
  uint64_t points[32];    /* A, B, C, E */
} amdzk_srs_report;
int amdzk_srs_check(amdzk_ctx* ctx, const amdzk_srs* srs, const uint64_t g2[16], const uint64_t s_g2[16],
                    const amdzk_srs_check_opts* opts /* NULL: all checks, seed 0 */, amdzk_srs_report* report);
/* plonk::verify_proof [UP] with a verdict per proof, in one call: amdzk_verify_proofs and the pairing(s) behind it.
 * s_g2, g2: the prepared [s]_2 and [1]_2 of the SRS the key was made on (amdzk_g2_setup, or the caller's own points).
 * flags = 0 — every proof by itself with weight 1, as SingleStrategy would:
 *   verdicts[b] = 1  iff  proof b is well formed and e(L_b, s_g2) = e(R_b, g2);  *n_valid (may be NULL) counts them.
 *   opts->combine_* are ignored: no random weight enters a verdict, the result is deterministic. The decode launch and the
 *   host half are amdzk_verify_proofs' own, once for the batch; the per-proof pairs come from the caller-supplied-bases MSM
 *   in runs of at most AMDZK_DECIDE_RUN proofs (2 columns per proof over the key's commitments, G and that run's decoded
 *   points: scratch is linear in the batch, one host wait more per run); ONE pairing launch over all proofs finishes.
 * flags = AMDZK_DECIDE_COMBINED — upstream's BatchVerifier: the two-column path of amdzk_verify_proofs with rho from opts
 *   (which must then be unpredictable, see above) and ONE check; every well-formed proof's verdict is that check's result.
 * In both modes a malformed proof has verdict 0 and its status in statuses[b] (as amdzk_verify_proofs); a pair with L or R
 * the identity has verdict 0 (a pair of identities must not read as valid), so a batch without a well-formed proof has
 * n_valid = 0. Refusals are amdzk_verify_proofs' own plus null s_g2 / g2 / verdicts and unknown flag bits, with the prefix
 * "verify_proofs_decide:". Not checked: subgroup membership of the G2 points, and that s_g2 / g2 belong to the key's SRS. */
#define AMDZK_DECIDE_COMBINED 1u
#define AMDZK_DECIDE_RUN 16
int amdzk_verify_proofs_decide(amdzk_ctx* ctx, const amdzk_pk* pk, const amdzk_g2* s_g2, const amdzk_g2* g2, uint32_t flags,
                               size_t n_proofs, const uint64_t* const* const* instances, const size_t* const* instance_lens,
                               const uint8_t* const* proofs, const size_t* proof_lens, const amdzk_verify_opts* opts,
                               amdzk_proof_status* statuses, uint8_t* verdicts /* n_proofs */, size_t* n_valid);

/* ---- the opening argument verified alone (ABI 1013): poly::kzg::multiopen::{VerifierSHPLONK, VerifierGWC}::verify_proof [UP]
 * over the CALLER's commitments, the counterpart of amdzk_multiopen_dev ("commit, then open" over a resident SRS, checked
 * without a PLONK proof around it).
 * g: the G of the SRS the commitments were made over (g[0], G1Affine). commitments: n_coms x 8 words, G1Affine, (0, 0) = the
 * identity (a zero polynomial's commitment) is allowed. points / queries as for amdzk_multiopen_dev with `poly` indexing
 * commitments; grouping, point ordering and the duplicate rule are the prover's (csrc/opening.hpp): equal point values are
 * one point, SHPLONK uses the first query of each (commitment, point value) pair, GWC every query's own. evals: required,
 * n_queries x 4 words, evals[i] = the evaluation query i claims.
 * Read order (only squeeze_challenge and read_point are called): SHPLONK squeeze y, squeeze v, read h1, squeeze u, read h2;
 * GWC squeeze v, read one W per distinct point value in first-seen order, squeeze u.
 * pair_out: L then R, G1Affine, (0, 0) = the identity, with "the openings are valid iff e(L, [s]_2) = e(R, [1]_2)" — the two
 * sums of amdzk_verify_proofs' comment with C_ij the caller's commitments, g in G's place and no h(X) expansion.
 * Device work: one launch checks every commitment and every point that was read (coordinates < q, on the curve; a read point
 * may not be (0, 0)), one two-column MSM over the commitments, the read points and g. amdzk_multiopen_decide adds one
 * amdzk_pairing_products call with m = 2: *verdict = 1 iff the check holds; a pair containing the identity gives 0.
 * No cap on sets, points or queries but memory (commitments and read points together stay below 2^30, where the check's
 * status word ends: 64 GiB of points). Commitments given as linear combinations of other commitments (upstream's
 * CommitmentReference::MSM) are NOT built: pass plain commitments.
 * Refused with a message that starts "multiopen_verify:", the ctx stays usable and the stream is idle: AMDZK_E_INVALID for null
 * arguments, a too-small opts->size, a missing transcript or member, n_queries = 0, an index out of range, an eval or a point
 * value >= r, a commitment or a read point that fails its check (the message names which), a non-zero return of a transcript
 * member, a squeezed challenge >= r; AMDZK_E_NOMEM when scratch cannot be allocated. */
typedef struct amdzk_multiopen_verify_opts {
  size_t size;                             /* sizeof(amdzk_multiopen_verify_opts) as the caller compiled it; too small is refused */
  int scheme;                              /* 0 SHPLONK, AMDZK_MULTIOPEN_GWC for GWC */
  const amdzk_transcript_read* transcript; /* required */
} amdzk_multiopen_verify_opts;
int amdzk_multiopen_verify(amdzk_ctx* ctx, const uint64_t g[8], const uint64_t* commitments, size_t n_coms,
                           const uint64_t* points, size_t n_points, const amdzk_open_query* queries,
                           const uint64_t* evals, size_t n_queries, const amdzk_multiopen_verify_opts* opts,
                           uint64_t pair_out[16]);
int amdzk_multiopen_decide(amdzk_ctx* ctx, const uint64_t g[8], const uint64_t* commitments, size_t n_coms,
                           const uint64_t* points, size_t n_points, const amdzk_open_query* queries,
                           const uint64_t* evals, size_t n_queries, const amdzk_multiopen_verify_opts* opts,
                           const amdzk_g2* s_g2, const amdzk_g2* g2, uint8_t* verdict);

/* ---- verifying keys: verify and decide proofs without a proving key.
 * amdzk_vk is what plonk::verify_proof [UP] reads of its VerifyingKey and its params: the circuit description,
 * transcript_repr, omega, the commitments of the fixed and the permutation columns, and G = g[0] of the SRS the key was made
 * on. Host data only, a few KB: it holds no device buffer and no pointer to an amdzk_srs or an amdzk_pk — both may be freed
 * before the key is used. A verifier process is a ctx and a key file: no amdzk_srs, no amdzk_pk.
 *
 * amdzk_keygen_vk — plonk::keygen_vk [UP]: the verifying key alone. Arguments as amdzk_keygen_phased / amdzk_keygen_sigma;
 * with num_perm_columns > 0 EXACTLY ONE of perm_mapping and sigma_values is non-NULL (both or neither: AMDZK_E_INVALID,
 * "keygen_vk:"). There are no mode flags: AMDZK_KEYGEN_* say how to prove. Device work: the upload of the F + S Lagrange
 * columns (the sigma columns computed from the mapping as keygen does) and their commitments over AMDZK_BASIS_G_LAGRANGE —
 * keygen's own steps, without the rest of keygen. Nothing proportional to the extended domain is allocated: no coset, no
 * compiled program, no per-proof workspace; (F + S) * 2^k * 32 bytes while the call runs, nothing but the key after it.
 * Runs on the ctx's stream and returns with it idle. Refusals are keygen's own checks with keygen's own prefixes
 * ("keygen: ...", and "circuit: ..." for a query, a constant or challenge index or an expression word out of range and for a
 * malformed expression: the expressions are not compiled here, the checks of the key file's reader stand in for the
 * compiler's, before anything is uploaded), plus, with "keygen_vk:", the rule above, an SRS without AMDZK_BASIS_G or without
 * AMDZK_BASIS_G_LAGRANGE, and an SRS of another k; the ctx stays usable. The verifier indexes by a key's queries and
 * expression words unchecked, so NO amdzk_vk exists whose description those checks refuse: amdzk_vk_from_pk refuses, with
 * "vk_from_pk:", the proving key of a circuit that keygen took on trust (a query that no expression uses may name any column). The key is the key amdzk_vk_from_pk gives for
 * amdzk_keygen_phased / amdzk_keygen_sigma on the same inputs: amdzk_vk_write gives equal bytes for the two.
 * amdzk_vk_from_pk — ProvingKey::get_vk [UP]: works on root keys, workspace clones, keys from amdzk_keygen_sigma and keys
 * read from a key file. */
typedef struct amdzk_vk amdzk_vk;
int amdzk_keygen_vk(amdzk_ctx* ctx, const amdzk_srs* srs, const amdzk_circuit* circuit, const amdzk_phases* phases /* may be NULL */,
                    const uint64_t* fixed_values, const uint32_t* perm_mapping /* or NULL */, const uint64_t* sigma_values /* or NULL */,
                    const uint64_t transcript_repr[4], amdzk_vk** out);
int amdzk_vk_from_pk(amdzk_ctx* ctx, const amdzk_pk* pk, amdzk_vk** out);
void amdzk_vk_free(amdzk_ctx* ctx, amdzk_vk* vk);
int amdzk_vk_commitments(const amdzk_vk* vk, uint64_t* fixed_out, uint64_t* perm_out);        /* as amdzk_pk_commitments */
size_t amdzk_vk_proof_size_multi(const amdzk_vk* vk, size_t n_circuits, int transcript_kind); /* = amdzk_proof_size_multi */
/* The verifying-key file: this library's own format (not upstream's VerifyingKey::write, which stores no circuit).
 * Little-endian, no padding, deterministic, self-delimiting (csrc/vkblob.hpp):
 *   "AMDZKVK\0" | version u32 = 1 | the proving-key file's sections from amdzk_circuit through the permutation commitments,
 *   byte for byte (circuit, has-phases and phase table, transcript_repr, fixed commitments, permutation commitments) |
 *   G (64 B, G1Affine, Montgomery) | has-g2 u8 | if 1: g2 then s_g2, 128 B each, G2Affine as above |
 *   BLAKE2b-512 of every byte before it, personalisation "amdzk_vk_blob_v1".
 * amdzk_vk_write: g2 / s_g2 (both or neither) are the SRS's [1]_2 and [s]_2, so that the file is all a verifier needs;
 * out = NULL queries *written. amdzk_vk_read needs no SRS and makes no device call; g2_out / s_g2_out / has_g2 may be NULL, the points are written
 * only when the file has them. amdzk_vk_blob_info and amdzk_vk_blob_check are pure host code, callable without a device:
 * every check amdzk_vk_read makes, and the reason as amdzk_vk_read would word it ("" for a good file).
 * Refused with AMDZK_E_INVALID and a message that starts "vk_read:", the ctx stays usable: bad magic or version; any
 * truncation or length mismatch; a digest mismatch; every header inconsistency amdzk_pk_read refuses; a commitment
 * coordinate >= q; a commitment that is neither on the curve nor (0, 0) (an all-zero fixed column commits to the identity,
 * which is legal); a G off the curve or the identity; a has-g2 byte other than 0 or 1; with has-g2 = 1 a G2 coordinate >= q,
 * a point off the twist or the identity (amdzk_g2_prepare's checks). Membership of the G2 points in the order-r subgroup is
 * NOT checked, as everywhere in this library. amdzk_vk_write checks what it wrote with the same reader, so a written file
 * always reads back, and writing what was read gives the same bytes. */
size_t amdzk_vk_serialized_size(const amdzk_vk* vk, int with_g2);
int amdzk_vk_write(amdzk_ctx* ctx, const amdzk_vk* vk, const uint64_t g2[16] /* may be NULL */, const uint64_t s_g2[16] /* NULL iff g2 is */,
                   uint8_t* out, size_t cap, size_t* written);
int amdzk_vk_read(amdzk_ctx* ctx, const uint8_t* data, size_t len, amdzk_vk** out, uint64_t g2_out[16], uint64_t s_g2_out[16], int* has_g2);
int amdzk_vk_blob_info(const uint8_t* data, size_t len, uint32_t* k, uint32_t* num_fixed, uint32_t* num_advice,
                       uint32_t* num_perm_columns, uint32_t* num_challenges, int* has_g2);
int amdzk_vk_blob_check(const uint8_t* data, size_t len, char* msg, size_t msg_cap);
/* amdzk_verify_proofs and amdzk_verify_proofs_decide with a verifying key in the proving key's place: the same code over the
 * same operands (the key's G is uploaded with its commitments instead of being copied from the SRS), hence the same
 * contracts word for word — message prefixes, statuses, the run length, the weights, the identity rule — and, for the same
 * circuit, SRS, proofs and options, equal pair_out, equal statuses and equal verdicts. */
int amdzk_verify_proofs_vk(amdzk_ctx* ctx, const amdzk_vk* vk, size_t n_proofs, const uint64_t* const* const* instances,
                           const size_t* const* instance_lens, const uint8_t* const* proofs, const size_t* proof_lens,
                           const amdzk_verify_opts* opts /* NULL: defaults */, amdzk_proof_status* statuses /* n_proofs */,
                           uint64_t pair_out[16]);
int amdzk_verify_proofs_decide_vk(amdzk_ctx* ctx, const amdzk_vk* vk, const amdzk_g2* s_g2, const amdzk_g2* g2, uint32_t flags,
                                  size_t n_proofs, const uint64_t* const* const* instances, const size_t* const* instance_lens,
                                  const uint8_t* const* proofs, const size_t* proof_lens, const amdzk_verify_opts* opts,
                                  amdzk_proof_status* statuses, uint8_t* verdicts /* n_proofs */, size_t* n_valid);

/* ---- proofs of DIFFERENT circuits verified and decided in one call (ABI 1016): what
 * amdzk_create_proof_batch_opts produces, taken back. Every item brings its own key — a proving key or a verifying key, exactly
 * one of pk / vk —, its own transcript kind, instance count, public inputs and proof (bytes, or the caller's read transcript).
 * Circuits, k, phase tables and proof sizes may differ from item to item. Upstream's AccumulatorStrategy fed by verify_proof
 * calls under different verifying keys and paired once is amdzk_verify_proofs_decide_mixed with AMDZK_DECIDE_COMBINED.
 * THE ONE RULE: every key was made over the same G (g[0] of its SRS) — compared by value, so keys over an SRS and over its
 * amdzk_srs_downsize, and verifying keys read from files, go together; s_g2 / g2 are that setup's. The rule sees G, not the
 * trapdoor: every amdzk_srs_setup starts from the same generator, so a key over ANOTHER trapdoor passes it — its items are
 * well formed and fail their pairing, exactly as under amdzk_verify_proofs_decide with the wrong s_g2.
 * Semantics are amdzk_verify_proofs' and amdzk_verify_proofs_decide's own, item by item: statuses[b] is the status and offset
 * the single-key call gives that proof under that key (AMDZK_PROOF_BAD_LENGTH against the item's own layout); rho_b belongs to
 * position b (the b-th draw of combine_seed, or combine_scalars[b]; one item without combine_scalars: 1);
 * pair_out = sum_b rho_b (L_b, R_b). amdzk_verify_proofs_decide_mixed with flags = 0: verdicts[b] is item b's own check with
 * weight 1 and ONE pairing launch serves all items; AMDZK_DECIDE_COMBINED: one check for the batch. The identity rule,
 * AMDZK_DECIDE_RUN and the bound of 2^20 items stay. A batch whose items all name one key gives the single-key call's words.
 * Device work: items are grouped by (key handle, n_circuits, transcript kind), first seen first; ONE decode launch covers every
 * (item, element) pair of every group (blocks of 64 threads, no block straddles two items); the combined pair is ONE two-column
 * MSM over every group's commitments, G and every item's decoded points; per proof, a run's MSM carries the commitments of the
 * groups present in it. Two host waits per call plus one per run in per-proof mode. The G of every distinct key comes down with
 * the status words: the rule costs no wait. Read transcripts are called in ascending b.
 * Refused with AMDZK_E_INVALID and a message that starts "verify_proofs_mixed:" (both calls), naming the item, the ctx stays
 * usable and the stream is idle: null arguments; n_items = 0 or > 2^20; both or neither of pk / vk; a too-small opts->size; an
 * unknown transcript kind; a key without a circuit description; a combine_scalars entry >= r; unknown flags; and, before any
 * MSM, the first item whose key's G differs from item 0's. Every item is validated before anything is uploaded. (A batch
 * without a well-formed item returns before anything is uploaded: identities, n_valid = 0, the rule unjudged.) */
typedef struct amdzk_verify_item {
  const amdzk_pk* pk;                       /* exactly one of pk / vk is non-NULL */
  const amdzk_vk* vk;
  int transcript_kind;                      /* as amdzk_verify_opts.transcript_kind, AMDZK_MULTIOPEN_GWC included */
  uint32_t n_circuits;                      /* circuit instances of this proof; 0 means 1 */
  const uint64_t* const* const* instances;  /* [circuit][column], as one proof's slice of amdzk_verify_proofs' array */
  const size_t* const* instance_lens;
  const uint8_t* proof;                     /* not read when transcript != NULL */
  size_t proof_len;
  const amdzk_transcript_read* transcript;  /* NULL: the bytes above; else only AMDZK_MULTIOPEN_GWC of transcript_kind counts */
} amdzk_verify_item;
typedef struct amdzk_verify_mixed_opts {
  size_t size;                     /* sizeof(amdzk_verify_mixed_opts) as the caller compiled it; too small is refused */
  uint64_t combine_seed;           /* as amdzk_verify_opts */
  const uint64_t* combine_scalars; /* n_items x 4 words, Montgomery; wins if set */
} amdzk_verify_mixed_opts;
int amdzk_verify_proofs_mixed(amdzk_ctx* ctx, const amdzk_verify_item* items, size_t n_items, const amdzk_verify_mixed_opts* opts /* NULL: seed 0 */,
                              amdzk_proof_status* statuses /* n_items */, uint64_t pair_out[16]);
int amdzk_verify_proofs_decide_mixed(amdzk_ctx* ctx, const amdzk_g2* s_g2, const amdzk_g2* g2, uint32_t flags, const amdzk_verify_item* items,
                                     size_t n_items, const amdzk_verify_mixed_opts* opts, amdzk_proof_status* statuses,
                                     uint8_t* verdicts /* n_items */, size_t* n_valid);

/* ---- witness programs: the advice cells of a batch of proofs computed on the device (ABI 1014).
 * Every create_proof starts from the advice columns, and every entry point above takes them as given (d_advice). For the
 * halo2-base style circuits of the reference, `synthesize` is a fixed straight-line computation over a few per-proof inputs:
 * field additions and products, bit and limb decompositions, carries, selects, landing in cells that are fixed per circuit.
 * A witness program carries that arithmetic across this boundary as DATA, the way amdzk_circuit carries the constraint
 * system: compiled once per circuit, then run for a whole batch, writing straight into the buffers that
 * amdzk_create_proof_batch (or amdzk_check_witness) reads. What is not field arithmetic — the quotient and remainder of a big
 * product, a native hash — is computed by the host per proof and enters as an input (a "hint"; a Poseidon digest can be
 * written into the resident input table by amdzk_poseidon_hash_dev, below).
 *
 * A program is a list of nodes in SSA order: node i names only nodes < i. A node's value is one Fr per proof of the batch.
 * All ops are total; canon(x) is the canonical integer of x in [0, r). Fields of amdzk_wnode an op does not use are ignored.
 *   AMDZK_W_INPUT   a        input a of this proof (a < n_inputs)
 *   AMDZK_W_CONST   a        constants[a] (a < n_constants)
 *   AMDZK_W_ADD     a b      a + b            AMDZK_W_SUB a b   a - b          (in Fr; a, b, c below are node indices)
 *   AMDZK_W_MUL     a b      a * b            AMDZK_W_NEG a     -a
 *   AMDZK_W_INV     a        a^-1, and 0 for 0 (as amdzk_batch_invert_dev)
 *   AMDZK_W_SELECT  a b c    b if a != 0, else c
 *   AMDZK_W_IS_ZERO a        1 if a == 0, else 0
 *   AMDZK_W_EQ      a b      1 if a == b, else 0
 *   AMDZK_W_LT      a b      1 if canon(a) < canon(b), else 0
 *   AMDZK_W_BITS    a, b = lo, c = len    (canon(a) >> lo) mod 2^len; lo and len are immediates, len >= 1, lo + len <= 256
 *                            (bit extraction, limb decomposition, and >> for carries)
 *   AMDZK_W_AND     a b      canon(a) & canon(b)
 *   AMDZK_W_XOR     a b      (canon(a) ^ canon(b)) mod r
 * There is no division by a variable and no op that serves one gadget: those are compositions of the above, or hints.
 * Phase-dependent programs need nothing more: a later phase's program can be run from an amdzk_phase_fn callback with the
 * challenges among its inputs — for a whole batch, from the amdzk_batch_phase_fn of amdzk_create_proof_batch_opts, which
 * hands every proof's challenges to ONE call per phase.
 *
 * amdzk_witness_compile validates the description, levelizes it (INPUT and CONST are level 0, every other node is one level
 * above its highest operand), orders the nodes by level, uploads the tables and keeps no pointer into the caller's arrays.
 * Refused with AMDZK_E_INVALID and a message that starts "witness:" — null arguments (an array pointer may be NULL only when
 * its count is 0), a too-small desc->size, k > 31, an unknown op, an operand >= its own node index, an input or constant
 * index out of range, a constant >= r, BITS with len = 0 or lo + len > 256, a cell with column >= num_advice or
 * row >= 2^k or node >= n_nodes, a cell named twice, a public node >= n_nodes. Because every index a kernel follows is checked
 * here, a run reads and writes nothing outside its tables, its workspace and the named cells.
 *
 * amdzk_witness_run: inputs[b] = the n_inputs x 4 words of proof b on the host (Montgomery, < r). d_advice[b] (a HOST array of
 * n_proofs device pointers) and advice_stride (Fr per column, >= 2^k) are as for amdzk_create_proof_batch: column c of proof
 * b at d_advice[b] + c * advice_stride; the buffers are pairwise different, non-null and on this ctx's device. The value of
 * cells[j].node is written to its (column, row) of every proof. With AMDZK_WITNESS_ZERO_FILL all num_advice x 2^k cells of
 * every proof are zeroed first; without it, cells that no amdzk_wcell names keep what they hold. The (advice_stride - 2^k)
 * elements between two columns are never written. publics_out (may be NULL): n_proofs x n_publics x 4 words, proof-major,
 * the values of the nodes in `publics` (the instance values of the proof), Montgomery.
 * Workspace: one run of P proofs holds (n_nodes + n_publics) x P x 32 + 256 bytes (every node's value for every proof of the
 * run, the publics gathered for the copy back, a status word); the host-pointer form stages n_proofs x n_inputs x 32 bytes
 * more. The workspace belongs to the amdzk_witness handle and only grows. max_scratch_bytes bounds the first figure; 0 = the
 * library's default (16 GiB). A batch that needs more is cut into the fewest equal runs of proofs that fit — R runs of
 * P = ceil(n_proofs / R) proofs, the last one shorter — and a run is also held below 2^31 (node, proof) items per level.
 * The results do not depend on the cut. A bound below one proof's workspace is refused (AMDZK_E_INVALID).
 * Execution: one work item per (node of a level, proof); a level wider than fused_width items is one kernel launch, and every
 * maximal stretch of consecutive levels of at most fused_width items each is ONE launch of a single workgroup that puts a
 * workgroup barrier between levels; then one launch scatters the cells and one gathers the publics. Ordering between
 * launches is stream order alone. The call runs on the ctx's stream and returns with it idle: work submitted afterwards on
 * the ctx sees the cells. One amdzk_witness is used by one call at a time.
 * Refused with a message that starts "witness:", the ctx stays usable and NOTHING has been written to any d_advice —
 * AMDZK_E_INVALID: null arguments, n_proofs = 0, a null or repeated d_advice pointer or one that is not device memory of this
 * ctx's GPU, advice_stride < 2^k, input_stride < n_inputs, unknown flag bits, an input value >= r (host form: checked on the
 * host; _dev form: by a check launch before anything else, whose status word names the first offender); AMDZK_E_UNSUPPORTED:
 * sizes whose workspace arithmetic would overflow, or a program of which one proof does not fit the default workspace.
 *
 * amdzk_witness_run_dev: the same with the inputs resident: input a of proof b at d_inputs + (b * input_stride + a) Fr.
 * The host-pointer form stages its inputs and runs the same code.
 *
 * amdzk_witness_plan: pure host code, callable without a device (like amdzk_msm_g1_bases_plan). Runs every validation of
 * amdzk_witness_compile and reports, for a run of n_proofs with the default max_scratch_bytes: *levels = the number of
 * levels (1 + the longest operand path; 0 for an empty program); *launches = the kernel launches amdzk_witness_run makes for
 * the levels, the scatter (if n_cells > 0) and the gather (if n_publics > 0), summed over its runs — the zero fill adds one
 * per call and the _dev form's input check one per call; *fused_width = the widest level, in (node, proof) items, that still
 * goes into a single-workgroup launch; *scratch_bytes = the workspace formula above for the run's P. Any output pointer may
 * be NULL; msg (may be NULL) receives the refusal's message, truncated to msg_cap. */
#define AMDZK_W_INPUT 0
#define AMDZK_W_CONST 1
#define AMDZK_W_ADD 2
#define AMDZK_W_SUB 3
#define AMDZK_W_MUL 4
#define AMDZK_W_NEG 5
#define AMDZK_W_INV 6
#define AMDZK_W_SELECT 7
#define AMDZK_W_IS_ZERO 8
#define AMDZK_W_EQ 9
#define AMDZK_W_LT 10
#define AMDZK_W_BITS 11
#define AMDZK_W_AND 12
#define AMDZK_W_XOR 13
#define AMDZK_WITNESS_ZERO_FILL 1u
typedef struct amdzk_witness amdzk_witness;
typedef struct amdzk_wnode { /* 16 bytes */
  uint32_t op;
  uint32_t a;
  uint32_t b;
  uint32_t c;
} amdzk_wnode;
typedef struct amdzk_wcell {
  uint32_t node;
  uint32_t column; /* advice column < num_advice */
  uint32_t row;    /* < 2^k */
} amdzk_wcell;
typedef struct amdzk_witness_desc {
  size_t size;               /* sizeof(amdzk_witness_desc) as compiled by the caller; too small is refused */
  uint32_t k;                /* rows = 2^k: the bound of amdzk_wcell.row */
  uint32_t num_advice;       /* the bound of amdzk_wcell.column */
  uint32_t n_inputs;         /* per-proof inputs (Montgomery Fr, < r) */
  uint32_t n_constants;
  const uint64_t* constants; /* n_constants x 4 words, Montgomery, < r */
  uint32_t n_nodes;
  const amdzk_wnode* nodes;
  uint32_t n_cells;
  const amdzk_wcell* cells;  /* node -> advice cell; a cell named twice is refused; a node may go to several cells */
  uint32_t n_publics;
  const uint32_t* publics;   /* nodes returned to the host per proof (instance values); repeats allowed */
} amdzk_witness_desc;
int amdzk_witness_plan(const amdzk_witness_desc* desc, size_t n_proofs, uint32_t* levels, uint32_t* launches, uint32_t* fused_width,
                       size_t* scratch_bytes, char* msg, size_t msg_cap);
int amdzk_witness_compile(amdzk_ctx* ctx, const amdzk_witness_desc* desc, amdzk_witness** out);
void amdzk_witness_free(amdzk_ctx* ctx, amdzk_witness* w);
int amdzk_witness_run(amdzk_ctx* ctx, amdzk_witness* w, size_t n_proofs, const uint64_t* const* inputs, void* const* d_advice,
                      size_t advice_stride, uint32_t flags, size_t max_scratch_bytes, uint64_t* publics_out);
int amdzk_witness_run_dev(amdzk_ctx* ctx, amdzk_witness* w, size_t n_proofs, const void* d_inputs, size_t input_stride,
                          void* const* d_advice, size_t advice_stride, uint32_t flags, size_t max_scratch_bytes,
                          uint64_t* publics_out);

/* ---- Poseidon over Fr: batched permutations and sponges on the device (ABI 1017).
 * The reference computes its nullifier natively with the `poseidon` crate (Poseidon::<Fr, 5, 4>::new(8, 57), update over
 * about 950 elements, squeeze). The spec crosses this boundary as DATA, the way amdzk_circuit does: the library generates no
 * constants, and what it computes for the constants it is given is stated here in full. The S-box is x^5 only.
 * Parity unpinned: the semantics below are the pinned crate's update / squeeze as recalled; the crate's source is not in
 * this tree, and no test compares with it.
 *
 * Permutation. For round ρ = 0 .. r_f + r_p − 1:
 * - `s[i] += rc[ρ][i]` for every i.
 * - `s[i] = s[i]^5` for every i when ρ < r_f/2 or ρ ≥ r_f/2 + r_p. Otherwise for i = 0 only.
 * - `s = M·s`, that is `s'[i] = Σ_j M[i][j]·s[j]`.
 *
 * Sponge.
 * - The state starts as `initial_state`.
 * - Inputs are taken in chunks of `rate`. Chunk element i is added to `s[1 + i]`, then the state is permuted.
 * - The last chunk is the m = len mod rate left-over elements followed by ONE. That is m + 1 ≤ rate elements; positions
 *   beyond them get nothing. One more permutation follows, also when m = 0 and when len = 0.
 * - The output is `s[1]`.
 * - A sponge of `len` inputs is ⌊len / rate⌋ + 1 permutations.
 *
 * Values in memory are halo2curves' Fr: 4 x u64 little-endian, Montgomery with R = 2^256, below r. Results are canonical
 * (below r) and exact. The textbook round constants and the full MDS matrix are wanted, not the crate's optimised
 * (sparse-matrix) form of the partial rounds.
 *
 * amdzk_poseidon_check_desc: pure host code, callable without a device (like amdzk_witness_plan). Runs every validation of
 * amdzk_poseidon_compile; msg (may be NULL) receives the refusal's message, truncated to msg_cap.
 * amdzk_poseidon_compile validates the description, converts the constants once to the form the kernels multiply by (Montgomery
 * radix 2^261, as the NTT's twiddles), uploads them and keeps no pointer into the caller's arrays. amdzk_poseidon_free releases
 * the handle (NULL is a no-op). One amdzk_poseidon is used by one call at a time, on the ctx's device it was compiled on.
 * amdzk_poseidon_permute_dev: n_states states of t Fr, state b at d_states + b * state_stride Fr, permuted in place — the
 * primitive under any other sponge convention. The (state_stride - t) elements between two states are never written.
 * amdzk_poseidon_hash: inputs[b] = the lens[b] x 4 words of sponge b on the host (may be NULL when lens[b] = 0); out receives
 * n x 4 words, digest b at out + 4 b. The host form checks its inputs (< r), stages them and runs the _dev form's code.
 * amdzk_poseidon_hash_dev: the inputs resident, input a of sponge b at d_inputs + (b * input_stride + a) Fr (d_inputs may be
 * NULL when every length is 0). lens: a HOST array of n lengths, or NULL for "all `len`" (`len` is ignored otherwise). Digest
 * b goes to d_out + b * out_stride Fr and nothing else is written: d_out may be an instance buffer or the input table of
 * amdzk_witness_run_dev. d_out must not overlap the inputs. Precondition: the resident values are below r (as
 * amdzk_fr_to_repr_dev; they are not checked).
 * Execution: one sponge (or state) per group of eight adjacent lanes, state element i in lane i, a 256-thread block carries
 * 32; sponges of different lengths share a launch, a wavefront runs to its longest. The calls run on the ctx's stream and
 * return with it idle.
 * Refused with a message that starts "poseidon:", the ctx stays usable and nothing has been written — AMDZK_E_INVALID: null
 * arguments (initial_state alone may be NULL), a too-small desc->size, t outside 2..8, rate outside 1..t-1, r_f odd or below
 * 2, a round constant, MDS entry or initial-state element >= r, n = 0, state_stride < t, input_stride below the longest
 * length, out_stride = 0, a device pointer that is not device memory of this ctx's GPU (amdzk_ptr_check_affinity's test), a
 * handle compiled on another device, an input >= r in the host form; AMDZK_E_UNSUPPORTED: (r_f + r_p) * t > 1536 (the round
 * constants of a spec stay in a block's LDS), a length of 2^31 or more, 2^31 or more sponges or states in one call, sizes
 * whose byte counts overflow size_t. Cut larger calls into runs. */
typedef struct amdzk_poseidon amdzk_poseidon;
typedef struct amdzk_poseidon_desc {
  size_t size;                      /* sizeof(amdzk_poseidon_desc) as compiled by the caller; too small is refused */
  uint32_t t;                       /* 2 <= t <= 8 */
  uint32_t rate;                    /* 1 <= rate <= t-1 */
  uint32_t r_f;                     /* even and >= 2 */
  uint32_t r_p;                     /* >= 0 */
  const uint64_t* round_constants;  /* (r_f + r_p) x t Fr, Montgomery, < r */
  const uint64_t* mds;              /* t x t Fr, row-major, Montgomery, < r */
  const uint64_t* initial_state;    /* t Fr, or NULL = (2^64, 0, ..., 0) */
} amdzk_poseidon_desc;
int amdzk_poseidon_check_desc(const amdzk_poseidon_desc* desc, char* msg, size_t msg_cap);
int amdzk_poseidon_compile(amdzk_ctx* ctx, const amdzk_poseidon_desc* desc, amdzk_poseidon** out);
void amdzk_poseidon_free(amdzk_ctx* ctx, amdzk_poseidon* p);
int amdzk_poseidon_permute_dev(amdzk_ctx* ctx, amdzk_poseidon* p, void* d_states, size_t n_states, size_t state_stride);
int amdzk_poseidon_hash(amdzk_ctx* ctx, amdzk_poseidon* p, const uint64_t* const* inputs, const size_t* lens, size_t n, uint64_t* out);
int amdzk_poseidon_hash_dev(amdzk_ctx* ctx, amdzk_poseidon* p, const void* d_inputs, size_t input_stride, const size_t* lens, size_t len,
                            size_t n, void* d_out, size_t out_stride);

/* Test hooks for the host pass that prepares quotient-domain programs for the limb-resident interpreter (bounds in
 * units of p, placement of the weak reductions, fusion of `t*x` with the accumulate): the pass on caller-supplied words
 * `op << 24 | arg` (opcodes: csrc/plonk_kernels.hpp ExprOp) — pure host code, callable without a device — and the
 * finalised h(X) program of a key. out may be NULL to query *out_n. */
int amdzk_debug_limb_program(const uint32_t* words, size_t n, uint32_t* out, size_t cap, size_t* out_n, uint32_t* depth);
int amdzk_pk_h_program(const amdzk_pk* pk, uint32_t* out, size_t cap, size_t* out_n);

/* ---- timing / profiling hooks used by bench.py (HIP events on this ctx's stream) ------------ */
int amdzk_timer_start(amdzk_ctx* ctx);
int amdzk_timer_stop(amdzk_ctx* ctx, float* ms); /* synchronises on the stop event */
/* When enabled, every kernel launch of this ctx is bracketed by HIP events; query by kernel name. */
int amdzk_prof_enable(amdzk_ctx* ctx, int on);
int amdzk_prof_reset(amdzk_ctx* ctx);
int amdzk_prof_get(amdzk_ctx* ctx, const char* kernel_name, uint64_t* launches, double* total_ms);
/* Writes a '\n'-separated list "name launches total_ms" into buf. Returns bytes needed. */
size_t amdzk_prof_dump(amdzk_ctx* ctx, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* AMDZK_H */
