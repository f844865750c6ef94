// The proof path: create_proof for KZG + SHPLONK or GWC + Blake2b or Keccak, one or several circuit instances, up to
// three phases — halo2_proofs 0.2.0 @ PSE v2023_01_20 [UP]:
//   plonk::prover::create_proof, plonk::{permutation,lookup,vanishing}::prover,
//   poly::kzg::multiopen::{shplonk::ProverSHPLONK, gwc::ProverGWC}.
// The key it proves with is keygen.hip's (pk.hpp), its programs program.hip's. The order of transcript operations and RNG
// draws follows SURVEY.md Appendix A and is stated in ONE place, prove_steps, over a driver: Solo runs it for one proof
// (lanes, several instances, the caller's phase callback), Gang for a lock-step batch (merged MSMs and evaluations). The
// steps themselves are Prover's; the two batch entry points share one refusal routine (batch_refusals) behind two adapters.
//
// Control flow, Fiat-Shamir and the O(columns) bookkeeping stay on the host; every O(n) step is a
// kernel on resident columns: all committed columns of a phase go through ONE batched MSM, all
// polynomials through ONE batched iNTT and ONE batched coset NTT, and the whole h(X) numerator is
// ONE interpreter launch. Host<->device traffic per proof: the blinding scalars and the random
// polynomial up (n*32 B), commitments and evaluations down. The lookup permutation
// (permute_expression_pair) also runs on the device (bitonic sort of the
// canonical values + multiset alignment).
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <deque>
#include <map>
#include <memory>
#include <string>

#include "hostcrypto.hpp"
#include "opening.hpp"
#include "pk.hpp"

using namespace bn254;
using zkhost::Blake2bWrite;
using zkhost::ChaCha20Rng;

// Source of the prover's Fr::random draws, addressed by position in upstream's draw order (DrawLayout): draw j is
// either block ctr0 + j of ChaCha20Rng::seed_from_u64's key stream — every Fr::random this prover makes is exactly one
// 64-byte block, so the device generates any run of draws straight into place (the blinding tails and the random
// polynomial; the host used to draw ~1,800 scalars per proof at 0.3 us each) — or the caller's scalars[j], drawn from
// its own RngCore (amdzk_create_proof_scalars, which checks their number against the layout).
struct RandomSource {
  uint32_t key[8] = {};
  uint64_t ctr0 = 0;
  const uint64_t* scalars = nullptr;  // non-null: the caller's draws, 4 words (Montgomery) each
  RandomSource() = default;
  explicit RandomSource(uint64_t seed) {
    const ChaCha20Rng rng(seed);
    memcpy(key, rng.key(), sizeof(key));
    ctr0 = rng.block_counter();
  }
};

namespace {

// lookup::prover::permute_expression_pair for L lookups at once, on Montgomery-form columns of n rows each:
// A (compressed inputs, [L][n]) is sorted in place into A', S ([L][n]) receives the aligned table S'; rows >= usable
// of both come back zero (the caller blinds them). T: the compressed tables (read only). Ts / left: [L][n] scratch,
// flags: 4 x L x (n + 8) u32 scratch. Canonical keys (numeric order = upstream's Ord for Fr), rows >= usable padded
// with an all-ones sentinel (> any canonical value) so the power-of-two sort leaves the real rows in front.
// Ts_sorted: the first `presorted` tables as keygen left them (canonical, padded, sorted), or null. Enqueues the whole
// permutation on ctx's stream; d_err receives 1 + the index of a lookup whose input is not in its table (0: none) —
// zk_permute_check reads it.
int zk_permute_expression_pairs(amdzk_ctx* ctx, Fr* A, const Fr* T, Fr* Ts, Fr* S, Fr* left, uint32_t* flags, int* d_err, size_t L, uint32_t n,
                                uint32_t usable, const Fr* Ts_sorted = nullptr, size_t presorted = 0) {
  if (L == 0) return AMDZK_OK;
  if (presorted > L || (presorted && !Ts_sorted)) ZK_FAIL(ctx, AMDZK_E_INVALID, "permute_expression_pairs: bad presorted tables");
  const size_t rest = L - presorted;
  Fr* Tr = Ts + presorted * n;
  if (presorted) ZK_TRY(d2d(ctx, Ts, Ts_sorted, presorted * n * 32));
  ZK_TRY(amdzk_fr_to_repr_dev(ctx, A, L * n));
  // rows >= usable of `cols` columns at p, to `byte`; usable == n leaves no such row, and no zero-width memset is issued
  auto fill_tail = [&](Fr* p, int byte, size_t cols) {
    return usable < n ? hipMemset2DAsync(p + usable, (size_t)n * 32, byte, (size_t)(n - usable) * 32, cols, ctx->stream) : hipSuccess;
  };
  ZK_HIP(ctx, fill_tail(A, 0xFF, L));
  if (rest) {
    ZK_TRY(d2d(ctx, Tr, T + presorted * n, rest * n * 32));
    ZK_TRY(amdzk_fr_to_repr_dev(ctx, Tr, rest * n));
    ZK_HIP(ctx, fill_tail(Tr, 0xFF, rest));
  }
  ZK_HIP(ctx, hipMemsetAsync(d_err, 0, sizeof(int), ctx->stream));
  ZK_TRY(zk_lookup_permute(ctx, A, Ts, S, left, L, n, usable, flags, (size_t)n + 8, d_err, presorted));
  ZK_HIP(ctx, fill_tail(A, 0, L));
  ZK_HIP(ctx, fill_tail(S, 0, L));
  ZK_TRY(amdzk_fr_from_raw_dev(ctx, A, L * n));
  ZK_TRY(amdzk_fr_from_raw_dev(ctx, S, L * n));
  return AMDZK_OK;
}

// the word zk_permute_expression_pairs left in d_err, once its work on ctx's stream is done
int zk_permute_check(amdzk_ctx* ctx, const int* d_err) {
  int herr = 0;
  ZK_TRY(d2h(ctx, &herr, d_err, sizeof(int)));
  if (herr) ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof: lookup %d input not in table (ConstraintSystemFailure)", herr - 1);
  return AMDZK_OK;
}

// MSM of ncols resident columns -> affine points on the host, in two halves: commit_launch enqueues the kernels on
// `ctx`'s stream (a lane or the caller's ctx) and returns; commit_finish copies the result down and waits for that
// stream only. Between the two the host enqueues work on other lanes. One commitment batch per lane at a time (the
// result sits in the lane's MSM workspace until it is finished).
struct PendingCommit {
  amdzk_ctx* ctx = nullptr;
  G1X* d_res = nullptr;
  size_t ncols = 0;
};
int commit_launch(amdzk_ctx* ctx, const KeyMaterial& K, int basis, const Fr* d_cols, size_t ncols, PendingCommit& pc) {
  pc.ctx = ctx;
  pc.ncols = ncols;
  pc.d_res = nullptr;
  if (ncols == 0) return AMDZK_OK;
  return zk_msm_dev_xyzz(ctx, K.srs, basis, d_cols, ncols, K.n, K.n, &pc.d_res);
}
int commit_finish(PendingCommit& pc, std::vector<G1Affine>& out) {
  amdzk_ctx* ctx = pc.ctx;
  const size_t ncols = pc.ncols;
  out.resize(ncols);
  if (ncols == 0) return AMDZK_OK;
  std::vector<uint64_t> jac(12 * ncols);
  ZK_TRY(zk_msm_finish(ctx, pc.d_res, ncols, jac.data()));
  for (size_t i = 0; i < ncols; i++) {
    const G1Jac* j = reinterpret_cast<const G1Jac*>(&jac[12 * i]);
    if (j->z.is_zero()) {
      out[i].x = Fq::zero();
      out[i].y = Fq::zero();
    } else {
      out[i].x = j->x;
      out[i].y = j->y;
    }
  }
  return AMDZK_OK;
}

// permutation::prover::Argument::commit up to the blinding: rows 0 ... usable of the nsets product columns into pk->zp(), from
// the workspace's columns and the beta and gamma of its constant table, on ctx's stream.
// Dense: the fraction program over every row, the inversion of nsets * n denominators and a running product per column,
// chained through last_z. Sparse (keys whose lists say so, KeyMaterial::perm_sparse): the same values from the perm_m listed
// cells alone — their numerators and denominators side by side in the fraction columns, which are free until the row
// differences are written there, ONE running product over all of them (last_z makes the sets one chain) and a gather.
int perm_products_unblinded(amdzk_ctx* ctx, const amdzk_pk* pk, bool sparse) {
  const KeyMaterial& K = *pk->key;
  const size_t n = K.n, ns = K.nsets, usable = n - (K.bf + 1);
  if (!sparse) {
    ZK_TRY(run_program(ctx, pk, pk->prog_pfrac, false, pk->d_outs_pfrac, nullptr, "expr_perm_fractions"));
    ZK_TRY(zk_batch_invert(ctx, pk->frac, pk->scratch, ns * n));
    ZK_TRY(zk_mul_elem(ctx, pk->zp(), pk->frac, ns * n));
    return zk_running_product(ctx, pk->zp(), ns, n, n, true, usable, pk->scan_tmp);
  }
  const size_t m = K.perm_m;
  Fr *den = pk->frac, *num = pk->frac + m + 1;
  ZK_TRY(zk_perm_frac_sparse(ctx, K.perm_list, (uint32_t)m, pk->d_perm_cols, K.sigma_lag, K.dxw_lag, n, K.S, K.chunk, pk->d_consts + K.c_beta,
                             pk->d_consts + K.c_gamma, num, den));
  ZK_TRY(zk_batch_invert(ctx, den, pk->scratch, m));
  ZK_TRY(zk_mul_elem(ctx, num, den, m));
  ZK_TRY(zk_running_product(ctx, num, 1, m + 1, m + 1, false, 0, pk->scan_tmp));
  return zk_perm_fill(ctx, num, K.perm_rank, K.perm_off, (uint32_t)usable, (uint32_t)ns, pk->zp(), n);
}

Fr rotate_omega(const KeyMaterial& K, const Fr& x, int rot) {
  return rot >= 0 ? mul(x, pow_u64(K.omega, (uint64_t)rot)) : mul(x, pow_u64(K.omega_inv, (uint64_t)(-rot)));
}

void trace_fr(const char* label, const Fr& v) {
  if (!getenv("AMDZK_TRACE")) return;
  uint8_t b[32];
  zkhost::fr_to_repr(v, b);
  fprintf(stderr, "[amdzk] %s ", label);
  for (int i = 31; i >= 0; i--) fprintf(stderr, "%02x", b[i]);
  fprintf(stderr, "\n");
}
void trace_pt(const char* label, const G1Affine& p) {
  if (!getenv("AMDZK_TRACE")) return;
  uint8_t b[32];
  zkhost::fq_to_repr(p.x, b);
  fprintf(stderr, "[amdzk] %s x=", label);
  for (int i = 31; i >= 0; i--) fprintf(stderr, "%02x", b[i]);
  fprintf(stderr, "\n");
}

}  // namespace

int commit_cols(amdzk_ctx* ctx, const KeyMaterial& K, int basis, const Fr* d_cols, size_t ncols, std::vector<G1Affine>& out) {
  PendingCommit pc;
  ZK_TRY(commit_launch(ctx, K, basis, d_cols, ncols, pc));
  return commit_finish(pc, out);
}

// plonk::evaluation::Evaluator::evaluate_h + divide_by_vanishing_poly + extended_to_coeff + the split into pieces
// (SURVEY.md §8(a) rows a6, a7, a10): from the committed polynomials in coefficient form (pk->PQ, arena order) and the
// challenges in pk->consts to the degree-1 pieces of h(X) in pk->hpieces. The numerator is evaluated on nc cosets of
// the size-n subgroup (poly.hip, zk_quotient_plan), then divided by X^n - 1, interpolated per coset and recombined.
static int quotient_from_cosets(amdzk_ctx* ctx, amdzk_pk* pk) {
  const KeyMaterial& K = *pk->key;
  ZK_TRY(upload_consts261(ctx, pk));
  ZK_TRY(upload_ypow(ctx, pk));
  // the program writes h where its first group of terms is flushed: a constraint system without a single term has none
  if (!K.h_terms) ZK_HIP(ctx, hipMemsetAsync(pk->hq, 0, (size_t)K.ext * 32, ctx->stream));
  ZK_TRY(run_program(ctx, pk, pk->prog_h, true, nullptr, pk->hq, "expr_evaluate_h"));
  ZK_TRY(zk_cosets_to_pieces(ctx, K.dom, pk->hq, pk->hpieces, K.qdeg));
  return AMDZK_OK;
}
static int quotient_pieces(amdzk_ctx* ctx, amdzk_pk* pk) {
  const KeyMaterial& K = *pk->key;
  ZK_TRY(zk_coeff_to_cosets_r261(ctx, K.dom, pk->PQ, K.n, pk->PC, K.ext, K.NP));
  return quotient_from_cosets(ctx, pk);
}

namespace {

// Where upstream's Fr::random draws of one create_proof over NC circuit instances fall. Blocks in
// draw order, each holding the NC instances' shares one after another: advice (per column bf + 1 tails, column-major,
// then one unused blind per column); lookups (per lookup bf + 1 tails of A', bf + 1 of S', two unused blinds);
// permutation products, then lookup products (per set / lookup bf tails and an unused blind); the random polynomial's n
// coefficients and its blind; the h pieces' blinds. A blinding tail of column c, row i is draw first + c * stride + i.
struct DrawLayout {
  size_t col;                              // stride of a column's draws: advice, permutation and lookup products (bf + 1)
  size_t lk_col;                           // stride of a lookup's draws in the lookups block
  size_t per_adv, per_lk, per_pz, per_lz;  // one instance's share of each block
  size_t adv, lk, pz, lz, rnd, h, total;   // first draw of each block; all draws
  DrawLayout(const KeyMaterial& K, size_t NC)
      : col((size_t)K.bf + 1), lk_col(2 * col + 2), per_adv((size_t)K.A * (col + 1)), per_lk((size_t)K.L * lk_col),
        per_pz((size_t)K.nsets * col), per_lz((size_t)K.L * col), adv(0), lk(NC * per_adv), pz(lk + NC * per_lk),
        lz(pz + NC * per_pz), rnd(lz + NC * per_lz), h(rnd + K.n + 1), total(h + K.qdeg) {}
  size_t advice(size_t ci) const { return adv + ci * per_adv; }
  // A key with challenge phases (upstream loops over cs.phases() outside the loop over the circuits): the advice block is
  // phase, then instance, then the bf + 1 tails of each of the phase's columns in column order, then one blind per column.
  // first_in_phase: the columns of phases below p (NC instances each); cols_in_phase: those of p itself.
  size_t advice_phase(size_t NC, size_t first_in_phase, size_t cols_in_phase, size_t ci) const {
    return adv + (NC * first_in_phase + ci * cols_in_phase) * (col + 1);
  }
  size_t lookup(size_t ci) const { return lk + ci * per_lk; }  // the A' tails; the S' tails follow at + col
  size_t perm_product(size_t ci) const { return pz + ci * per_pz; }
  size_t lookup_product(size_t ci) const { return lz + ci * per_lz; }
};

// A commitment batch begun on a lane and collected when the transcript needs it. On one stream (serial) it is
// collected at once: a context holds one batch's result at a time.
struct Commit {
  PendingCommit pc;
  std::vector<G1Affine> pts;
  bool begun = false, done = false;
};

// A commitment batch a Prover of a gang (amdzk_create_proof_batch) hands to the gang instead of launching it: `ncols`
// columns of n at `cols`. The gang commits the batches of all its provers in ONE submission and hands the points back:
// into `into` (the prover writes them when its order says so) or, with a label, straight to the prover's transcript.
struct DeferredCommit {
  int basis;
  const Fr* cols;
  size_t ncols;
  Commit* into;
  const char* label;
};

// The multiopen argument's lists for pks[0..NC) (amdzk_pk::Multiopen): the evaluations in proof order, then h_poly's;
// the queries in upstream order and their grouping (opening.hpp). Built once per key (per list of instance keys).
int build_multiopen(amdzk_ctx* ctx, amdzk_pk* const* pks, size_t NC, amdzk_pk::Multiopen& mo) {
  amdzk_pk* const pk = pks[0];
  const KeyMaterial& K = *pk->key;
  const size_t n = K.n;
  const uint32_t S = K.S, L = K.L, ns = K.nsets, bf = K.bf;
  // distinct POINTS: rotations that differ by a multiple of n name the same point x * omega^rot (upstream keeps a set's
  // points in a BTreeSet of field elements), as in the verifier's plan (verifier.hpp); two of them in one set would make
  // the set's interpolation divide by zero
  auto rot_mod = [&](int rot) { return ((int64_t)rot % (int64_t)n + (int64_t)n) % (int64_t)n; };
  auto rot_id = [&](int rot) -> uint32_t {
    for (size_t i = 0; i < mo.rots.size(); i++)
      if (rot_mod(mo.rots[i]) == rot_mod(rot)) return (uint32_t)i;
    mo.rots.push_back(rot);
    return (uint32_t)mo.rots.size() - 1;
  };
  auto addq = [&](const Fr* p, int rot) { mo.ev.push_back({p, rot}); };
  // written evaluations: advice (instance after instance), fixed, random, sigma, permutation products (instance after
  // instance), lookups (instance after instance)
  for (size_t ci = 0; ci < NC; ci++)
    for (auto& q : K.advice_queries) addq(pks[ci]->q_adv() + (size_t)q.first * n, q.second);
  for (auto& q : K.fixed_queries) addq(K.fixed_poly + (size_t)q.first * n, q.second);
  addq(pk->rnd, 0);
  for (uint32_t i = 0; i < S; i++) addq(K.sigma_poly + (size_t)i * n, 0);
  for (size_t ci = 0; ci < NC; ci++)
    for (uint32_t s = 0; s < ns; s++) {
      addq(pks[ci]->q_zp() + (size_t)s * n, 0);
      addq(pks[ci]->q_zp() + (size_t)s * n, 1);
      if (s + 1 < ns) addq(pks[ci]->q_zp() + (size_t)s * n, -(int)(bf + 1));
    }
  for (size_t ci = 0; ci < NC; ci++)
    for (uint32_t l = 0; l < L; l++) {
      addq(pks[ci]->q_zl() + (size_t)l * n, 0);
      addq(pks[ci]->q_zl() + (size_t)l * n, 1);
      addq(pks[ci]->q_la() + (size_t)l * n, 0);
      addq(pks[ci]->q_la() + (size_t)l * n, -1);
      addq(pks[ci]->q_ls() + (size_t)l * n, 0);
    }
  mo.n_written = mo.ev.size();
  addq(pk->hpoly, 0);
  // 8. multiopen queries in upstream order
  std::map<std::pair<const Fr*, int>, uint32_t> where;
  for (size_t i = 0; i < mo.ev.size(); i++) where.emplace(mo.ev[i], (uint32_t)i);
  std::map<const Fr*, uint32_t> com_of;  // polynomial -> commitment id, first seen first
  bool missing = false;
  auto addpq = [&](const Fr* p, int rot) {
    auto it = where.find({p, rot});
    if (it == where.end()) {
      missing = true;
      return;
    }
    const uint32_t com = com_of.emplace(p, (uint32_t)mo.com_poly.size()).first->second;
    if (com == mo.com_poly.size()) mo.com_poly.push_back(p);
    mo.q.push_back({com, rot_id(rot)});
    mo.q_ev.push_back(it->second);
  };
  // per instance: advice queries, the permutation argument's openings, the lookups' openings; then what exists once
  for (size_t ci = 0; ci < NC; ci++) {
    amdzk_pk* const pk = pks[ci];
    for (auto& q : K.advice_queries) addpq(pk->q_adv() + (size_t)q.first * n, q.second);
    for (uint32_t s = 0; s < ns; s++) {
      addpq(pk->q_zp() + (size_t)s * n, 0);
      addpq(pk->q_zp() + (size_t)s * n, 1);
    }
    for (int s = (int)ns - 2; s >= 0; s--) addpq(pk->q_zp() + (size_t)s * n, -(int)(bf + 1));
    for (uint32_t l = 0; l < L; l++) {
      addpq(pk->q_zl() + (size_t)l * n, 0);
      addpq(pk->q_la() + (size_t)l * n, 0);
      addpq(pk->q_ls() + (size_t)l * n, 0);
      addpq(pk->q_la() + (size_t)l * n, -1);
      addpq(pk->q_zl() + (size_t)l * n, 1);
    }
  }
  for (auto& q : K.fixed_queries) addpq(K.fixed_poly + (size_t)q.first * n, q.second);
  for (uint32_t i = 0; i < S; i++) addpq(K.sigma_poly + (size_t)i * n, 0);
  addpq(pk->hpoly, 0);
  addpq(pk->rnd, 0);
  if (missing) {
    mo = amdzk_pk::Multiopen();
    pk->mo_multi_keys.clear();
    ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof: a multiopen query has no evaluation");
  }
  // rotation ids are first seen first among the QUERIES: that is GWC's output order
  mo.grp = opening::group(mo.q.data(), mo.q.size(), mo.com_poly.size(), mo.rots.size());
  for (auto& e : mo.ev) mo.ev_rot.push_back(rot_id(e.second));
  const size_t pairs = mo.grp.set_points;
  if (mo.grp.sets.size() > K.max_sets) {
    mo = amdzk_pk::Multiopen();
    ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "create_proof: more than %u rotation sets", K.max_sets);
  }
  if (std::max<size_t>(pairs, 1) > pk->sets_Q_pairs) {
    const void* outgrown = pk->sets_Q;  // (stays allocated until the handle goes; no longer an arena)
    ZK_TRY(dalloc(ctx, pk, &pk->sets_Q, std::max<size_t>(pairs, 1) * n));
    pk->arenas.erase(std::remove_if(pk->arenas.begin(), pk->arenas.end(), [&](const std::pair<void*, size_t>& a) { return outgrown && a.first == outgrown; }),
                     pk->arenas.end());
    pk->arenas.push_back({(void*)pk->sets_Q, std::max<size_t>(pairs, 1) * n * sizeof(Fr)});
    pk->sets_Q_pairs = std::max<size_t>(pairs, 1);
  }
  mo.built = true;
  return AMDZK_OK;
}

// What a caller-owned transcript said so far: its own error, or a squeezed challenge that is no residue (CallbackWrite).
// Asked at every step boundary, and before a challenge is looked at.
int transcript_status(amdzk_ctx* ctx, const zkhost::TranscriptWrite& T) {
  if (T.failed) ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof: the caller's transcript reported an error");
  if (T.noncanonical) ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof: a squeezed challenge is not below the modulus");
  return AMDZK_OK;
}

// One create_proof in flight: what its steps share, and the steps themselves (prove_steps below states their order, for a
// proof alone and for the members of a batch alike). A step the transcript waits for comes in two halves — *_enqueue: all
// the work up to the commitments' launch; *_write: their points into the transcript — and the driver collects the
// commitments in between (Solo: nothing to do, the halves launch and finish their own batches; Gang: one merged MSM).
// pks[c] holds instance c's workspace; `pk` is pks[0]: what the proof has once (transcript representative, random
// polynomial, h(X), multiopen buffers, staging); every per-circuit step runs in a loop over the instances with `pk`
// shadowed by that instance's key.
// Lanes: M = the caller's ctx (everything the transcript waits for), B and C = its auxiliary streams (common.hpp).
// M carries the chain commitment -> challenge -> next phase; B takes each phase's columns to coefficient form and to
// the quotient domain as soon as they are blinded (out of place: the commitments and the next phase's programs keep
// reading the Lagrange values); C computes the lookup products beside the permutation products and commits the random
// polynomial at the very start. Only the ORDER OF TRANSCRIPT WRITES is upstream's;
// the arithmetic between two challenges is unordered there too. With AMDZK_KEYGEN_SERIAL, or while per-kernel
// profiling is on, B = C = M and everything below degenerates to one stream.
struct Prover {
  amdzk_ctx* const ctx;
  amdzk_pk* const* const pks;
  amdzk_pk* const pk;
  const KeyMaterial& K;
  const size_t NC, n, usable;
  const uint32_t A, I, L, ns, bf;
  amdzk_ctx *const M, *const B, *const C;
  const bool serial;
  zkhost::TranscriptWrite& T;
  const RandomSource& rng;
  const DrawLayout draws;
  Commit cm_rnd;
  std::vector<Commit> cm_adv, cm_lk, cm_zp, cm_zl;  // per instance, between the two halves of their step
  // the multiopen lists (the key's) and what the evaluation step leaves for the opening argument
  amdzk_pk::Multiopen* mo = nullptr;
  std::vector<Fr> rot_pt, evals;  // the points x * omega^rot, once per distinct rotation; the evaluations
  opening::Shplonk sh;
  // the caller's columns: instances_all[ci][col] / instance_lens_all[ci][col] (either may be null), d_advice_all[ci]
  const uint64_t* const* const* instances_all = nullptr;
  const size_t* const* instance_lens_all = nullptr;
  const void* const* d_advice_all = nullptr;
  size_t advice_stride = 0;
  Fr sh_v;  // SHPLONK's v, squeezed in front of its first commitment and used again for its second
  // Member of a gang (serial, one instance): commit_begin / commit_write leave their batch here instead of launching it
  std::vector<DeferredCommit>* sink = nullptr;
  // a phased key between phases_begin and the last phase_write: the challenges so far (zero: not yet squeezed), the advice
  // columns of the phases below and of the phase in flight, and that phase's batches, one per (instance, run of columns)
  std::vector<Fr> chal;
  size_t adv_before = 0, adv_in_phase = 0;
  std::deque<Commit> cm_phase;
  std::vector<const Fr*> ev_pp;             // evaluations_prepare: the (polynomial, point) pairs
  std::vector<Fr> ev_pts;
  const bool ttrace = getenv("AMDZK_TRACE_TIME") != nullptr;
  double tlast;

  Prover(amdzk_ctx* ctx, amdzk_pk* const* pks, size_t NC, amdzk_ctx* B, amdzk_ctx* C, zkhost::TranscriptWrite& T, const RandomSource& rng)
      : ctx(ctx), pks(pks), pk(pks[0]), K(*pk->key), NC(NC), n(K.n), usable(K.n - (K.bf + 1)), A(K.A), I(K.I), L(K.L), ns(K.nsets),
        bf(K.bf), M(ctx), B(B), C(C), serial(B == ctx), T(T), rng(rng), draws(K, NC), cm_adv(NC), cm_lk(NC), cm_zp(NC), cm_zl(NC), tlast(now_ms()) {}

  static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  void tick(const char* label) {
    if (!ttrace) return;
    zk_host_wait(ctx, ctx->stream);
    const double t = now_ms();
    fprintf(stderr, "[amdzk-time] %-28s %8.3f ms\n", label, t - tlast);
    tlast = t;
  }
  Fr challenge(const char* label) {
    const Fr c = T.squeeze_challenge();
    trace_fr(label, c);
    return c;
  }
  int lane_id(amdzk_ctx* l) const { return l == M ? 0 : l == B ? 1 : 2; }
  // a failure on a lane is reported through the caller's ctx
  int on_lane(amdzk_ctx* l, int r) {
    if (r != AMDZK_OK && l != ctx) ctx->err = l->err;
    return r;
  }
  int upload_small_on(amdzk_ctx* l, const std::vector<Fr>& v, size_t off_elems) {
    if (off_elems + v.size() > pk->small_cap) ZK_FAIL(ctx, AMDZK_E_NOMEM, "create_proof: small buffer overflow");
    return on_lane(l, h2d_staged(l, pk, pk->small_l[lane_id(l)] + off_elems, v.data(), v.size() * 32));
  }
  int write_points(const std::vector<G1Affine>& pts, const char* label) {
    for (auto& p : pts) {
      trace_pt(label, p);
      if (!T.write_point(p)) ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof: %s commitment is the identity (cannot write points at infinity to the transcript)", label);
    }
    return AMDZK_OK;
  }
  // Blinding tails on lane l: rows [row0, row0 + cnt) of ncols columns, column c's row row0 + i taking draw
  // first_draw + c * stride + i. A seeded ChaCha20Rng generates them on the device straight into their rows; the
  // caller's scalars are gathered here, uploaded (staged through pinned memory) and scattered.
  int blind(amdzk_ctx* l, Fr* d_cols, uint32_t ncols, size_t row0, uint32_t cnt, size_t first_draw, size_t stride) {
    if (!rng.scalars)
      return on_lane(l, zk_chacha20_blind_rows(l, d_cols, n, row0, cnt, ncols, rng.key, rng.ctr0 + first_draw, (uint32_t)stride, zkhost::fr_r3()));
    std::vector<Fr> v((size_t)ncols * cnt);
    for (uint32_t c = 0; c < ncols; c++) memcpy(&v[(size_t)c * cnt], rng.scalars + 4 * (first_draw + c * stride), (size_t)cnt * 32);
    ZK_TRY(upload_small_on(l, v, 0));
    return on_lane(l, zk_scatter_rows(l, d_cols, n, row0, pk->small_l[lane_id(l)], cnt, ncols));
  }
  int commit_end(Commit& c) {
    if (c.begun && !c.done) ZK_TRY(on_lane(c.pc.ctx, commit_finish(c.pc, c.pts)));
    c.done = true;
    return AMDZK_OK;
  }
  int commit_begin(amdzk_ctx* l, int basis, const Fr* d_cols, size_t ncols, Commit& c) {
    if (sink) {  // the gang launches it with the other provers' and fills c.pts
      c.begun = true;
      if (ncols) sink->push_back(DeferredCommit{basis, d_cols, ncols, &c, nullptr});
      else c.done = true;
      return AMDZK_OK;
    }
    ZK_TRY(on_lane(l, commit_launch(l, K, basis, d_cols, ncols, c.pc)));
    c.begun = true;
    if (serial) ZK_TRY(commit_end(c));
    return AMDZK_OK;
  }
  // commit on the caller's stream and write the points at once (the commitments the transcript waits for alone)
  int commit_write(int basis, const Fr* d_cols, size_t ncols, const char* label) {
    if (sink) {
      if (ncols) sink->push_back(DeferredCommit{basis, d_cols, ncols, nullptr, label});
      return AMDZK_OK;
    }
    std::vector<G1Affine> cm;
    ZK_TRY(commit_cols(ctx, K, basis, d_cols, ncols, cm));
    return write_points(cm, label);
  }
  // columns [first, first + count) of the arena, blinded on lane `after`: coefficients (PQ) and quotient-domain values (PC) on B
  // after_l1: the columns' commitment batch has already been launched on `after`; the transforms start behind its
  // level-1 kernel (both fill the chip: side by side they only stretch each other) and run beside its tail and beside
  // the next phase's latency-bound kernels instead
  int transforms_on_B(amdzk_pk* pk, amdzk_ctx* after, size_t first, size_t count, bool after_l1 = false) {
    if (!count) return AMDZK_OK;
    if (after_l1) ZK_TRY(zk_stream_after_l1(B, after));
    else ZK_TRY(zk_stream_after(B, after));
    ZK_TRY(on_lane(B, zk_lagrange_to_coeff(B, K.dom, pk->P + first * n, n, pk->PQ + first * n, n, count)));
    return on_lane(B, zk_coeff_to_cosets_r261(B, K.dom, pk->PQ + first * n, n, pk->PC + first * K.ext, K.ext, count));
  }
  // d_out = sum_j coefs[j] polys[j] (len elements each) on lane l, through l's pointer-table and small slices; `extra`
  // follows the coefficients in the small slice, for the kernel the caller launches next
  int lincomb(amdzk_ctx* l, const std::vector<const Fr*>& polys, const std::vector<Fr>& coefs, Fr* d_out, size_t len,
              const std::vector<Fr>& extra = {}) {
    const int li = lane_id(l);
    ZK_TRY(on_lane(l, h2d_staged(l, pk, pk->ptrs_l[li], polys.data(), polys.size() * sizeof(Fr*))));
    ZK_TRY(upload_small_on(l, coefs, 0));
    ZK_TRY(upload_small_on(l, extra, coefs.size()));
    return on_lane(l, zk_lincomb(l, (const Fr* const*)pk->ptrs_l[li], pk->small_l[li], (uint32_t)polys.size(), d_out, len, false));
  }
  // challenges into their slots of every instance's constant table, and the span of slots they cover up to the device
  int put_consts(std::initializer_list<std::pair<uint32_t KeyMaterial::*, Fr>> vals) {
    for (size_t ci = 0; ci < NC; ci++) {
      amdzk_pk* const pk = pks[ci];
      uint32_t lo = UINT32_MAX, hi = 0;
      for (auto& v : vals) {
        const uint32_t s = K.*v.first;
        pk->consts[s] = v.second;
        lo = std::min(lo, s);
        hi = std::max(hi, s);
      }
      ZK_TRY(h2d_staged(ctx, pk, pk->d_consts + lo, &pk->consts[lo], (size_t)(hi + 1 - lo) * 32));
    }
    return AMDZK_OK;
  }

  // 0. vk, instances
  int instances() {
    T.common_scalar(K.transcript_repr);
    for (size_t ci = 0; ci < NC && I; ci++) {  // columns are zero beyond the caller's values: clear on the device, upload only what was given
      amdzk_pk* const pk = pks[ci];
      const uint64_t* const* instances = instances_all ? instances_all[ci] : nullptr;
      const size_t* instance_lens = instance_lens_all ? instance_lens_all[ci] : nullptr;
      ZK_HIP(ctx, hipMemsetAsync(pk->inst(), 0, (size_t)I * n * 32, ctx->stream));
      std::vector<Fr> iv;
      for (uint32_t c = 0; c < I; c++) {
        const size_t len = instance_lens ? instance_lens[c] : 0;
        if (len > usable) ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof: instance column %u too long (InstanceTooLarge)", c);
        if (!len) continue;
        if (!instances || !instances[c]) ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof: instance column %u is null", c);
        iv.resize(len);
        for (size_t i = 0; i < len; i++) {
          memcpy(iv[i].l, instances[c] + 4 * i, 32);
          T.common_scalar(iv[i]);
        }
        ZK_TRY(h2d_staged(ctx, pk, pk->inst() + (size_t)c * n, iv.data(), len * 32));
        // without room in the pinned staging area the copy reads `iv` asynchronously: finish it before the next column reuses it
        if (!pk->pin || len * 32 > pk->pin_cap) ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
      }
    }
    return AMDZK_OK;
  }
  // The random polynomial of the vanishing argument (step 5) depends on nothing but the RNG, at a position of the draws
  // the key fixes: it is made now and committed on lane C while M commits the advice columns.
  int random_poly() {
    ZK_TRY(zk_stream_after(C, M));  // the previous proof on this key may still be reading rnd on M's stream
    if (!rng.scalars) ZK_TRY(on_lane(C, zk_chacha20_fr_random(C, pk->rnd, n, rng.key, rng.ctr0 + draws.rnd, zkhost::fr_r3())));
    else ZK_TRY(on_lane(C, h2d(C, pk->rnd, rng.scalars + 4 * draws.rnd, n * 32)));  // the caller's buffer outlives the call
    return commit_begin(C, AMDZK_BASIS_G, pk->rnd, 1, cm_rnd);
  }
  // challenge i of a phased key into its slot of every instance's constant table (host copy and device)
  int put_challenge(uint32_t i, const Fr& v) {
    for (size_t ci = 0; ci < NC; ci++) {
      amdzk_pk* const pk = pks[ci];
      const uint32_t s = K.c_chal0 + i;
      pk->consts[s] = v;
      ZK_TRY(h2d_staged(ctx, pk, pk->d_consts + s, &pk->consts[s], 32));
    }
    return AMDZK_OK;
  }
  // 1. advice, phase after phase (a key without challenge phases: everything in phase 0). enqueue: copy in, blind the
  // unusable rows of every column, launch the commitments; write: their points, then the phase's challenges.
  int advice_enqueue(uint32_t p) {
    if (!K.phased()) {
      for (size_t ci = 0; ci < NC && p == 0; ci++) ZK_TRY(plain_enqueue(ci));
      return AMDZK_OK;
    }
    if (p == 0) ZK_TRY(phases_begin());
    return p < K.nphases ? phase_enqueue(p) : AMDZK_OK;
  }
  int advice_write(uint32_t p) {
    if (K.phased()) return p < K.nphases ? phase_write(p) : AMDZK_OK;
    for (size_t ci = 0; ci < NC && p == 0; ci++) {
      ZK_TRY(commit_end(cm_adv[ci]));
      ZK_TRY(write_points(cm_adv[ci].pts, "advice"));
    }
    return AMDZK_OK;
  }
  int advice_done() {
    ZK_TRY(commit_end(cm_rnd));  // long done; lane C's MSM workspace is free for the lookup products' commitment
    tick(K.phased() ? "advice (phased)" : "advice");
    return AMDZK_OK;
  }
  // A key with challenge phases (amdzk_keygen_phased), upstream's order: phase after phase, and inside a phase instance
  // after instance, the phase's columns (runs of consecutive columns of the arena) are copied in, blinded, committed and
  // written; then the phase's challenges are squeezed into their constant slots. Phases >= 1 start with the caller's
  // callback (the driver's phase_callback), which fills their columns of d_advice from the challenges so far.
  // The challenges start at zero (the last proof's values are gone); [the callback]; the phase's runs of columns copied
  // in, blinded, transformed and their commitments launched — one batch per run, finished at once without a sink (a
  // context holds one batch's result at a time), handed to the gang with one; then the points written in that order and
  // the phase's challenges squeezed.
  int phases_begin() {
    chal.assign(K.num_challenges, Fr::zero());
    for (uint32_t i = 0; i < K.num_challenges; i++) ZK_TRY(put_challenge(i, chal[i]));
    adv_before = 0;
    return AMDZK_OK;
  }
  int phase_enqueue(uint32_t p) {
    std::vector<std::pair<uint32_t, uint32_t>> runs;  // (first column, count)
    size_t in_phase = 0;
    for (uint32_t c = 0; c < A; c++)
      if (K.advice_phase[c] == p) {
        if (!runs.empty() && runs.back().first + runs.back().second == c) runs.back().second++;
        else runs.push_back({c, 1});
        in_phase++;
      }
    cm_phase.clear();
    for (size_t ci = 0; ci < NC; ci++) {
      amdzk_pk* const pk = pks[ci];
      size_t j0 = 0;  // position of the run's first column among the phase's columns
      for (auto& run : runs) {
        const uint32_t c0 = run.first, cnt = run.second;
        Fr* const cols = pk->adv() + (size_t)c0 * n;
        ZK_HIP(ctx, hipMemcpy2DAsync(cols, n * 32, (const Fr*)d_advice_all[ci] + (size_t)c0 * advice_stride, advice_stride * 32, n * 32, cnt,
                                     hipMemcpyDeviceToDevice, ctx->stream));
        ZK_TRY(blind(M, cols, cnt, usable, bf + 1, draws.advice_phase(NC, adv_before, in_phase, ci) + j0 * draws.col, draws.col));
        cm_phase.emplace_back();
        Commit& cm = cm_phase.back();
        if (!serial) ZK_TRY(commit_begin(M, AMDZK_BASIS_G_LAGRANGE, cols, cnt, cm));
        ZK_TRY(transforms_on_B(pk, M, c0, cnt, cm.begun));
        if (!cm.begun) ZK_TRY(commit_begin(M, AMDZK_BASIS_G_LAGRANGE, cols, cnt, cm));
        if (!sink) ZK_TRY(commit_end(cm));
        j0 += cnt;
      }
      if (p == 0) ZK_TRY(transforms_on_B(pk, M, A, I));  // the instance columns ride with the first phase
    }
    adv_in_phase = in_phase;
    return AMDZK_OK;
  }
  int phase_write(uint32_t p) {
    for (auto& cm : cm_phase) ZK_TRY(write_points(cm.pts, "advice"));
    cm_phase.clear();
    for (uint32_t i = 0; i < K.num_challenges; i++)
      if (K.challenge_phase[i] == p) {
        chal[i] = challenge("phase challenge");
        ZK_TRY(transcript_status(ctx, T));  // before the phase callback is handed it
        ZK_TRY(put_challenge(i, chal[i]));
      }
    adv_before += adv_in_phase;
    return AMDZK_OK;
  }
  // an unphased key's advice, instance ci: everything up to the commitment's launch (with a sink: its hand-over to the gang)
  int plain_enqueue(size_t ci) {
    const void* d_advice = d_advice_all ? d_advice_all[ci] : nullptr;
    amdzk_pk* const pk = pks[ci];
    if (A) {
      ZK_HIP(ctx, hipMemcpy2DAsync(pk->adv(), n * 32, d_advice, advice_stride * 32, n * 32, A, hipMemcpyDeviceToDevice, ctx->stream));
      ZK_TRY(blind(M, pk->adv(), A, usable, bf + 1, draws.advice(ci), draws.col));
    }
    Commit& cm = cm_adv[ci] = Commit();
    if (A && !serial) ZK_TRY(commit_begin(M, AMDZK_BASIS_G_LAGRANGE, pk->adv(), A, cm));
    ZK_TRY(transforms_on_B(pk, M, 0, (size_t)A + I, cm.begun));
    if (A && !cm.begun) ZK_TRY(commit_begin(M, AMDZK_BASIS_G_LAGRANGE, pk->adv(), A, cm));
    return AMDZK_OK;
  }
  // 2. lookups: compress, permute (on the device), blind, commit — every instance's enqueue, then every instance's write
  int lookups_enqueue() {
    for (size_t ci = 0; ci < NC && L; ci++) ZK_TRY(lookups_enqueue(ci));
    return AMDZK_OK;
  }
  int lookups_write() {
    for (size_t ci = 0; ci < NC && L; ci++) ZK_TRY(lookups_write(ci));
    tick("lookups_permuted");
    return AMDZK_OK;
  }
  int lookups_enqueue(size_t ci) {
    amdzk_pk* const pk = pks[ci];
    ZK_TRY(run_program(ctx, pk, pk->prog_compress, false, pk->d_outs_compress, nullptr, "expr_lookup_compress"));
    ZK_TRY(d2d(ctx, pk->la(), pk->ci, (size_t)L * n * 32));
    ZK_TRY(zk_permute_expression_pairs(ctx, pk->la(), pk->ct, pk->lk_ts, pk->ls(), pk->lk_left, pk->lk_flags, pk->d_err, L, (uint32_t)n,
                                       (uint32_t)usable, K.lk_ts_const, K.lk_const));
    // the "input not in table" word comes down behind the permutation and is read once the host has waited for this
    // phase's commitment anyway (it used to be a host wait of its own in the middle of the phase: 0.1 ms of idle device)
    *pk->h_err = 0;
    ZK_HIP(ctx, hipMemcpyAsync(pk->h_err, pk->d_err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    tick("  lookup: device permute");
    ZK_TRY(blind(M, pk->la(), L, usable, bf + 1, draws.lookup(ci), draws.lk_col));
    ZK_TRY(blind(M, pk->ls(), L, usable, bf + 1, draws.lookup(ci) + draws.col, draws.lk_col));
    Commit& cm = cm_lk[ci] = Commit();
    if (!serial) ZK_TRY(commit_begin(M, AMDZK_BASIS_G_LAGRANGE, pk->la(), 2 * L, cm));
    ZK_TRY(transforms_on_B(pk, M, (size_t)A + I, 2 * (size_t)L, cm.begun));
    if (!cm.begun) ZK_TRY(commit_begin(M, AMDZK_BASIS_G_LAGRANGE, pk->la(), 2 * L, cm));
    return AMDZK_OK;
  }
  int lookups_write(size_t ci) {
    amdzk_pk* const pk = pks[ci];
    ZK_TRY(commit_end(cm_lk[ci]));  // the wait behind which the error word is down
    if (*pk->h_err) ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof: lookup %d input not in table (ConstraintSystemFailure)", *pk->h_err - 1);
    const std::vector<G1Affine>& cm = cm_lk[ci].pts;
    for (uint32_t l = 0; l < L; l++) {
      std::vector<G1Affine> two = {cm[l], cm[L + l]};
      ZK_TRY(write_points(two, "lookup_permuted"));
    }
    return AMDZK_OK;
  }
  int lookup_products(size_t ci, bool ordered_behind_m) {
    amdzk_pk* const pk = pks[ci];
    if (!ordered_behind_m) ZK_TRY(zk_stream_after(C, M));  // beta, gamma and the permuted columns are in place
    ZK_TRY(on_lane(C, run_program(C, pk, pk->prog_lfrac, false, pk->d_outs_lfrac, nullptr, "expr_lookup_fractions")));
    ZK_TRY(on_lane(C, zk_batch_invert(C, pk->frac2, pk->scratch2, (size_t)L * n)));
    ZK_TRY(on_lane(C, zk_mul_elem(C, pk->zl(), pk->frac2, (size_t)L * n)));
    ZK_TRY(on_lane(C, zk_running_product(C, pk->zl(), L, n, n, false, 0, pk->scan_tmp2)));
    ZK_TRY(blind(C, pk->zl(), L, n - bf, bf, draws.lookup_product(ci), draws.col));
    // ... and their commitment, enqueued BEFORE the permutation chain: the lookup chain is the shorter one, so its
    // level-1 kernel runs while M is still in fractions, inversion and scans rather than beside M's own level-1 kernel.
    // (Measured: 18.8-19.3 ms per proof either way — what one lane gains the other loses; kept for the simpler order.)
    if (serial) ZK_TRY(transforms_on_B(pk, C, (size_t)A + I + 2 * L + ns, L));
    ZK_TRY(commit_begin(C, AMDZK_BASIS_G_LAGRANGE, pk->zl(), L, cm_zl[ci]));
    if (!serial) ZK_TRY(transforms_on_B(pk, C, (size_t)A + I + 2 * L + ns, L, true));
    return AMDZK_OK;
  }
  int perm_products(size_t ci) {  // fractions, inversion, running products, blinding: everything in front of the commitment
    amdzk_pk* const pk = pks[ci];
    ZK_TRY(perm_products_unblinded(ctx, pk, K.perm_sparse));
    tick("  perm: fractions, inversion, running product");
    ZK_TRY(blind(M, pk->zp(), ns, n - bf, bf, draws.perm_product(ci), draws.col));
    // What is committed is the columns' row differences, over the prefix sums of g_lagrange: the same points (Abel
    // summation), and a product column only changes on the rows of a copy cycle and in its blinding tail. frac is free
    // from the running product until the next proof's fractions; zp() keeps the values for the transforms and openings.
    return zk_row_diff(M, pk->zp(), pk->frac, ns, n, n, n);
  }
  int perm_commit(size_t ci) {
    amdzk_pk* const pk = pks[ci];
    if (serial) ZK_TRY(transforms_on_B(pk, M, (size_t)A + I + 2 * L, ns));
    return commit_begin(M, AMDZK_BASIS_G_LAGRANGE_PREFIX, pk->frac, ns, cm_zp[ci]);
  }
  // 3. + 4. permutation grand products on M, lookup grand products on C (they depend on beta and gamma only, not on
  // each other). (Several instances: every instance's permutation products are committed before the first lookup product.)
  int products_enqueue() {
    if (!serial) {
      // Lanes (one instance): the HOST enqueues M's chain first — seven launches the transcript waits for — and lane C's
      // lookup products (a dozen launches and a commitment batch's fourteen) while M's fractions and inversion run: the
      // device used to sit 0.48 ms behind beta / gamma waiting for M's first kernel (profiles/r03zz_timeline_single_proof.txt).
      if (L) ZK_TRY(zk_stream_after(C, M));  // C starts behind beta, gamma and the permuted columns — NOT behind M's products below
      if (ns) ZK_TRY(perm_products(0));
      if (L) ZK_TRY(lookup_products(0, true));
      if (ns) ZK_TRY(perm_commit(0));
      if (ns) ZK_TRY(transforms_on_B(pk, M, (size_t)A + I + 2 * L, ns, true));
      return AMDZK_OK;
    }
    for (size_t ci = 0; ci < NC && L; ci++) ZK_TRY(lookup_products(ci, false));
    for (size_t ci = 0; ci < NC && ns; ci++) {
      ZK_TRY(perm_products(ci));
      ZK_TRY(perm_commit(ci));
    }
    return AMDZK_OK;
  }
  int products_write() {
    for (size_t ci = 0; ci < NC; ci++) {
      ZK_TRY(commit_end(cm_zp[ci]));
      ZK_TRY(write_points(cm_zp[ci].pts, "perm_z"));
    }
    tick("perm_products");
    for (size_t ci = 0; ci < NC; ci++) {
      ZK_TRY(commit_end(cm_zl[ci]));
      ZK_TRY(write_points(cm_zl[ci].pts, "lookup_z"));
    }
    tick("lookup_products");
    return AMDZK_OK;
  }
  // 6. h(X): every committed column is on the quotient domain once lane B has drained
  int vanishing(const Fr& y) {
    ZK_TRY(zk_stream_after(M, B));
    for (size_t ci = 0; ci < NC; ci++) ZK_TRY(quotient_from_cosets(ctx, pks[ci]));  // theta, beta, gamma, delta powers, y are all known by now
    if (NC > 1) {
      // evaluate_h folds the instances' terms in ONE Horner chain with y, instance after instance: with K terms per instance
      // the numerator is sum_c y^(K (NC - 1 - c)) * numerator_c, and the division by X^n - 1, the interpolation and the cut
      // into pieces are linear — so the pieces are the same combination of the instances' pieces.
      std::vector<const Fr*> pp(NC);
      std::vector<Fr> cf(NC);
      const Fr yK = pow_u64(y, K.h_terms);
      Fr cur = Fr::one();
      for (size_t ci = NC; ci-- > 0;) {
        pp[ci] = pks[ci]->hpieces;
        cf[ci] = cur;
        cur = mul(cur, yK);
      }
      const size_t len = (size_t)K.qdeg * n;
      ZK_TRY(lincomb(M, pp, cf, pk->scratch, len));  // scratch holds >= ext >= qdeg * n
      ZK_TRY(d2d(ctx, pk->hpieces, pk->scratch, len * 32));
    }
    ZK_TRY(commit_write(AMDZK_BASIS_G, pk->hpieces, K.qdeg, "h_piece"));  // consecutive n-blocks
    tick("h_eval+commit");
    return AMDZK_OK;
  }
  // 7. evaluations: h_poly = sum_i piece_i * x^(n i), then one list of (polynomial, rotation) in proof order and the
  //    extra evaluation SHPLONK needs (h_poly at x; random at x is already in the list)
  //    — in three parts: h_poly and the pairs (ev_pp, ev_pts); [the driver's evaluate_step fills `evals`: one launch behind
  //    one wait for this proof alone, or for all the members of a gang]; the written evaluations
  int evaluations_prepare(const Fr& x) {
    {
      const Fr xn = pow_u64(x, n);
      std::vector<const Fr*> pp(K.qdeg);
      std::vector<Fr> cf(K.qdeg);
      Fr cur = Fr::one();
      for (uint32_t i = 0; i < K.qdeg; i++) {
        pp[i] = pk->hpieces + (size_t)i * n;
        cf[i] = cur;
        cur = mul(cur, xn);
      }
      ZK_TRY(lincomb(M, pp, cf, pk->hpoly, n));
    }
    mo = NC == 1 ? &pk->mo : &pk->mo_multi;
    if (NC > 1) {  // the cached lists name the polynomials of one particular list of instance keys
      std::vector<const amdzk_pk*> keys(pks, pks + NC);
      if (keys != pk->mo_multi_keys) {
        pk->mo_multi = amdzk_pk::Multiopen();
        pk->mo_multi_keys = keys;
      }
    }
    if (!mo->built) ZK_TRY(build_multiopen(ctx, pks, NC, *mo));
    const size_t nrot = mo->rots.size();
    rot_pt.resize(nrot);
    for (size_t r = 0; r < nrot; r++) rot_pt[r] = rotate_omega(K, x, mo->rots[r]);
    const size_t nq = mo->ev.size();
    if (nq > pk->ptrs_cap || 2 * nq > pk->small_cap) ZK_FAIL(ctx, AMDZK_E_NOMEM, "create_proof: too many queries (%zu)", nq);
    ev_pp.resize(nq);
    ev_pts.resize(nq);
    for (size_t i = 0; i < nq; i++) ev_pp[i] = mo->ev[i].first, ev_pts[i] = rot_pt[mo->ev_rot[i]];
    return AMDZK_OK;
  }
  int evaluations_write() {
    for (size_t i = 0; i < mo->n_written; i++) T.write_scalar(evals[i]);
    tick("evals");
    return AMDZK_OK;
  }
  // 9a. GWC (multiopen/gwc/prover.rs [UP]): queries grouped by point in first-seen order;
  // per point z:  W_z = (sum_j v^j p_j - sum_j v^j p_j(z)) / (X - z), committed and written in that order.
  int gwc(const Fr& v) {
    const std::vector<std::vector<uint32_t>>& gw = mo->grp.gw;  // one per distinct point (= distinct rotation), first seen first
    const size_t np = gw.size();
    if (np > 16) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "create_proof: more than 16 opening points");
    for (size_t i = 0; i < np; i++) {
      const size_t m = gw[i].size();
      if (m > pk->ptrs_cap || m + 1 > pk->small_cap) ZK_FAIL(ctx, AMDZK_E_NOMEM, "create_proof: opening set too large");
      std::vector<const Fr*> polys(m);
      std::vector<Fr> cf(m);
      Fr cur = Fr::one(), eb = Fr::zero();
      for (size_t j = 0; j < m; j++) {
        polys[j] = mo->com_poly[mo->q[gw[i][j]].com];
        cf[j] = cur;
        eb = add(eb, mul(cur, evals[mo->q_ev[gw[i][j]]]));
        cur = mul(cur, v);
      }
      Fr* Wi = pk->sets_N + i * n;
      ZK_TRY(lincomb(M, polys, cf, Wi, n, {eb}));
      ZK_TRY(zk_sub_low(ctx, Wi, pk->small + m, 1));
    }
    std::vector<Fr*> pp(np);
    std::vector<Fr> roots(np);
    for (size_t i = 0; i < np; i++) {
      pp[i] = pk->sets_N + i * n;
      roots[i] = rot_pt[i];
    }
    ZK_TRY(h2d_staged(ctx, pk, pk->ptrs, pp.data(), np * sizeof(Fr*)));
    ZK_TRY(upload_small_on(M, roots, 0));
    ZK_TRY(zk_kate_div(ctx, (Fr* const*)pk->ptrs, pk->small, np, (uint32_t)n));
    return commit_write(AMDZK_BASIS_G, pk->sets_N, np, "gwc_w");
  }
  // 9b. SHPLONK (multiopen/shplonk/prover.rs [UP]), up to its first commitment h(X)
  int shplonk(const Fr& ys, const Fr& v) {
    const opening::Grouping& g = mo->grp;
    const size_t nr = g.sets.size(), maxm = g.maxm;
    if (nr > 16) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "create_proof: more than 16 rotation sets");
    sh = opening::shplonk_sets(g, rot_pt.data(), [&](uint32_t q) { return evals[mo->q_ev[q]]; }, ys, v);
    // L_i = sum_j y^j P_ij ; N_i = (L_i - R_i) / prod_t (X - p_t), R_i = sum_j y^j R_ij. The division runs once, not once
    // per point: 1 / prod_t (X - p_t) = sum_t c_t / (X - p_t) with c_t = 1 / prod_{s != t} (p_t - p_s) (the points of a
    // set are distinct), and L_i - R_i vanishes at every p_t, so N_i = sum_t c_t Q_it with Q_it = (L_i - R_i) / (X - p_t)
    // — all (set, point) quotients in ONE division launch, then h(X) = sum_i v^i N_i = sum_it (v^i c_it) Q_it in one
    // linear combination. Exact arithmetic, same polynomial. The L_i of different sets are independent: one lane each.
    amdzk_ctx* lanes3[3] = {M, B, C};
    for (size_t i = 0; i < nr; i++) {
      const size_t m = g.sets[i].coms.size();
      if (m > pk->ptrs_cap || m > pk->small_cap / 2) ZK_FAIL(ctx, AMDZK_E_NOMEM, "create_proof: rotation set too large");
      std::vector<const Fr*> polys(m);
      std::vector<Fr> cf(m);
      Fr cur = Fr::one();
      for (size_t j = 0; j < m; j++) {
        polys[j] = mo->com_poly[g.coms[g.sets[i].coms[j]]];
        cf[j] = cur;
        cur = mul(cur, ys);
      }
      amdzk_ctx* ln = lanes3[i % 3];
      if (ln != M && i < 3) ZK_TRY(zk_stream_after(ln, M));  // the evaluations above came off M; hpoly is in place
      ZK_TRY(lincomb(ln, polys, cf, pk->sets_L + i * n, n));
    }
    ZK_TRY(zk_stream_after(M, B));
    ZK_TRY(zk_stream_after(M, C));
    const size_t nq = sh.root.size();
    if (2 * nq > pk->ptrs_cap || nq * (maxm + 2) > pk->small_cap) ZK_FAIL(ctx, AMDZK_E_NOMEM, "create_proof: too many opening points");
    std::vector<const Fr*> q_src(nq);
    std::vector<Fr*> q_dst(nq);
    for (size_t q = 0; q < nq; q++) q_src[q] = pk->sets_L + sh.row_set[q] * n, q_dst[q] = pk->sets_Q + q * n;
    void** pt = (void**)pk->ptrs;
    ZK_TRY(h2d_staged(ctx, pk, pt, q_dst.data(), nq * sizeof(Fr*)));
    ZK_TRY(h2d_staged(ctx, pk, pt + nq, q_src.data(), nq * sizeof(Fr*)));
    ZK_TRY(upload_small_on(M, sh.root, 0));
    ZK_TRY(upload_small_on(M, sh.row_low, nq));
    ZK_TRY(upload_small_on(M, sh.coef, nq + sh.row_low.size()));
    ZK_TRY(zk_kate_div_from(ctx, (Fr* const*)pt, (const Fr* const*)(pt + nq), pk->small, pk->small + nq, (uint32_t)maxm, nq, (uint32_t)n));
    ZK_TRY(zk_lincomb(ctx, (const Fr* const*)pt, pk->small + nq + sh.row_low.size(), (uint32_t)nq, pk->hx, n, false));
    return commit_write(AMDZK_BASIS_G, pk->hx, 1, "shplonk_h1");
  }
  // ... and its second: l(X) = sum_i v^i z_i (L_i - r_i) - zt(u) h(X);  then / (X - u) / z_0 — the factor 1 / z_0 rides
  // in on the coefficients (opening::shplonk_final).
  int shplonk_final(const Fr& v, const Fr& u) {
    const size_t nr = mo->grp.sets.size();
    const opening::Final f = opening::shplonk_final(mo->grp, sh, rot_pt.data(), v, u);
    // 1 / z_0(u) = 0 would zero every coefficient (upstream's invert().unwrap() panics here)
    if (f.z0_zero) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "create_proof: the challenge u is one of the opening points (probability 2^-254)");
    std::vector<const Fr*> pp(nr + 1);
    for (size_t i = 0; i < nr; i++) pp[i] = pk->sets_L + i * n;
    pp[nr] = pk->hx;
    Fr* lx = pk->sets_Q;  // reuse
    ZK_TRY(lincomb(M, pp, f.cf, lx, n, {f.cterm, u}));
    std::vector<Fr*> one_p = {lx};
    ZK_TRY(h2d_staged(ctx, pk, (void**)pk->ptrs + nr + 1, one_p.data(), sizeof(Fr*)));
    ZK_TRY(zk_kate_div_from(ctx, (Fr* const*)((void**)pk->ptrs + nr + 1), nullptr, pk->small + nr + 2, pk->small + nr + 1, 1, 1, (uint32_t)n));
    return commit_write(AMDZK_BASIS_G, lx, 1, "shplonk_h2");
  }
};

// beta = 0 on a key with permutation columns: the permutation factors are evaluated as beta (sigma + w) and
// beta (delta^j X + w) with w = (v + gamma) / beta
int beta_usable(amdzk_ctx* ctx, const KeyMaterial& K, const Fr& beta) {
  if (K.S && beta.is_zero()) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "create_proof: the challenge beta is zero (probability 2^-254): the factored permutation terms need 1 / beta");
  return AMDZK_OK;
}
// x = 0: every rotation of x is the one point 0. Upstream merges opening points by value; the key's opening plan groups
// them by rotation and would divide by p_t - p_s = 0 (opening::shplonk_sets).
int x_usable(amdzk_ctx* ctx, const Fr& x) {
  if (x.is_zero()) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "create_proof: the challenge x is zero (probability 2^-254): rotations of x coincide");
  return AMDZK_OK;
}

// pks[i] is a handle of pks[0]'s key and none of the handles before it: what every entry point over several handles asks
// of each, under its own prefix and its own noun for what a handle stands for.
int check_handle(amdzk_ctx* ctx, const char* who, const char* noun, amdzk_pk* const* pks, size_t i) {
  if (pks[i]->key != pks[0]->key) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: %s %zu's key is not the first key or a workspace clone of it", who, noun, i);
  for (size_t d = 0; d < i; d++)
    if (pks[d] == pks[i]) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: %ss %zu and %zu share one workspace", who, noun, d, i);
  return AMDZK_OK;
}

// The transcript one proof writes to — the caller's, or the built-in one of `kind` — and its random source: owned
// together, by a proof alone and by every member of a gang. The Prover keeps references into it.
struct ProofIO {
  zkhost::Blake2bWrite t_blake;
  zkhost::Keccak256Write t_keccak;
  std::unique_ptr<zkhost::CallbackWrite> t_caller;
  RandomSource rng;
  ProofIO(const amdzk_transcript* caller, const RandomSource& rng) : t_caller(caller ? new zkhost::CallbackWrite(*caller) : nullptr), rng(rng) {}
  ProofIO(const ProofIO&) = delete;
  zkhost::TranscriptWrite& T(int kind) {  // kind: without the AMDZK_MULTIOPEN_GWC bit
    if (t_caller) return *t_caller;
    return kind == AMDZK_TRANSCRIPT_BLAKE2B ? (zkhost::TranscriptWrite&)t_blake : (zkhost::TranscriptWrite&)t_keccak;
  }
};

// THE ORDER of create_proof, stated once (plonk/prover.rs [UP]): instances, advice phase after
// phase, theta, the permuted lookup columns, beta and gamma, the permutation and lookup products, the random polynomial,
// y, h(X), x, the evaluations, the opening argument. Inside a step everything is written circuit instance after circuit
// instance; the challenges, the random polynomial and h(X) exist once.
// The driver says for whom and how the shared work is done:
//   each(f)            f for every live prover; a failure ends that prover's proof, and so does its transcript's status
//   commit_step()      collects the commitments the provers launched or deferred in the step before
//   evaluate_step()    fills every prover's `evals` from the pairs evaluations_prepare left
//   phase_callback(p)  the caller's synthesize of phase p >= 1
// Solo (one proof, lanes or one stream, NC instances) and Gang (a lock-step batch) below are the two drivers.
// A caller-owned transcript that reported an error, or squeezed words that are no residue, ends its proof: asked behind
// every squeeze before the challenge is used, behind the written evaluations, and by the drivers at every step boundary.
template <class Driver>
int prove_steps(Driver& D, bool use_gwc, uint32_t phases) {
  amdzk_ctx* const ctx = D.ctx;
  ZK_TRY(D.each([&](Prover& P) -> int {
    ZK_TRY(P.instances());
    ZK_TRY(transcript_status(ctx, P.T));
    return P.random_poly();
  }));
  ZK_TRY(D.commit_step());  // the random polynomial (a gang; alone it stays on lane C until the advice is written)
  for (uint32_t p = 0; p < phases; p++) {
    if (p > 0) ZK_TRY(D.phase_callback(p));
    ZK_TRY(D.each([&](Prover& P) -> int { return P.advice_enqueue(p); }));
    ZK_TRY(D.commit_step());
    ZK_TRY(D.each([&](Prover& P) -> int {
      ZK_TRY(P.advice_write(p));
      return p + 1 == phases ? P.advice_done() : AMDZK_OK;
    }));
  }
  ZK_TRY(D.each([&](Prover& P) -> int {
    const Fr theta = P.challenge("theta");
    ZK_TRY(transcript_status(ctx, P.T));
    ZK_TRY(P.put_consts({{&KeyMaterial::c_theta, theta}}));
    return P.lookups_enqueue();
  }));
  ZK_TRY(D.commit_step());
  ZK_TRY(D.each([&](Prover& P) -> int {
    ZK_TRY(P.lookups_write());
    const Fr beta = P.challenge("beta");
    const Fr gamma = P.challenge("gamma");
    ZK_TRY(transcript_status(ctx, P.T));
    ZK_TRY(beta_usable(ctx, P.K, beta));
    ZK_TRY(P.put_consts({{&KeyMaterial::c_beta, beta}, {&KeyMaterial::c_gamma, gamma}, {&KeyMaterial::c_betainv, inv(beta)}}));
    P.tick("  perm: challenges+consts");
    return P.products_enqueue();
  }));
  ZK_TRY(D.commit_step());  // the lookup products over g_lagrange, the permutation products' differences over its prefix sums
  ZK_TRY(D.each([&](Prover& P) -> int {
    ZK_TRY(P.products_write());
    ZK_TRY(P.write_points(P.cm_rnd.pts, "random_poly"));  // 5. vanishing: the random polynomial, committed at the start
    const Fr y = P.challenge("y");
    ZK_TRY(transcript_status(ctx, P.T));
    ZK_TRY(P.put_consts({{&KeyMaterial::c_y, y}}));
    return P.vanishing(y);
  }));
  ZK_TRY(D.commit_step());  // the h pieces, written as they come back
  ZK_TRY(D.each([&](Prover& P) -> int {
    const Fr x = P.challenge("x");
    ZK_TRY(transcript_status(ctx, P.T));
    ZK_TRY(x_usable(ctx, x));
    return P.evaluations_prepare(x);
  }));
  ZK_TRY(D.evaluate_step());
  ZK_TRY(D.each([&](Prover& P) -> int {
    ZK_TRY(P.evaluations_write());
    ZK_TRY(transcript_status(ctx, P.T));
    if (use_gwc) {
      const Fr v = P.challenge("gwc_v");
      ZK_TRY(transcript_status(ctx, P.T));
      return P.gwc(v);
    }
    const Fr ys = P.challenge("shplonk_y");
    P.sh_v = P.challenge("shplonk_v");
    ZK_TRY(transcript_status(ctx, P.T));
    return P.shplonk(ys, P.sh_v);
  }));
  ZK_TRY(D.commit_step());
  if (!use_gwc) {
    ZK_TRY(D.each([&](Prover& P) -> int {
      const Fr u = P.challenge("u");
      ZK_TRY(transcript_status(ctx, P.T));
      return P.shplonk_final(P.sh_v, u);
    }));
    ZK_TRY(D.commit_step());
  }
  return D.each([&](Prover& P) -> int {
    P.tick("multiopen");
    return AMDZK_OK;
  });
}

// The driver of one proof on its own: one Prover with its lanes and its NC instances. Without a sink the halves of a step
// launch their own commitment batches and finish them (commit_end) where they write them, so there is nothing to collect.
struct Solo {
  amdzk_ctx* const ctx;
  Prover& P;
  amdzk_phase_fn phase_fn;  // amdzk_proof_opts: the caller's synthesize of phases >= 1
  void* phase_user;
  template <class F>
  int each(F f) {
    ZK_TRY(f(P));
    return transcript_status(ctx, P.T);
  }
  int commit_step() { return AMDZK_OK; }
  int phase_callback(uint32_t p) {
    const int r = phase_fn(phase_user, p, (const uint64_t*)P.chal.data(), P.K.num_challenges, (void*)ctx->stream);
    if (r != 0) ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof: the phase callback returned %d in phase %u", r, p);
    return AMDZK_OK;
  }
  // the pairs through the key's own pointer table and small buffer: one launch, one download
  int evaluate_step() {
    amdzk_pk* const pk = P.pk;
    const size_t nq = P.ev_pp.size();
    ZK_TRY(h2d_staged(ctx, pk, pk->ptrs, P.ev_pp.data(), nq * sizeof(Fr*)));
    ZK_TRY(P.upload_small_on(P.M, P.ev_pts, 0));
    ZK_TRY(zk_poly_eval(ctx, (const Fr* const*)pk->ptrs, pk->small, pk->small + nq, nq, (uint32_t)P.n));
    P.evals.resize(nq);
    return d2h(ctx, P.evals.data(), pk->small + nq, nq * 32);
  }
};

// What amdzk_create_proof_opts adds to a proof: the caller's transcript and its synthesize of the later phases.
struct ProofExtras {
  const amdzk_transcript* transcript = nullptr;
  amdzk_phase_fn phase_fn = nullptr;
  void* phase_user = nullptr;
};

// One proof over NC instances of the circuit (upstream's `circuits: &[C]`, `instances: &[&[&[F]]]`): pks[c] holds
// instance c's workspace — the key itself for c = 0, workspace clones of it for the others (amdzk_pk_clone_workspace).
// Its refusals, its lanes and the Solo driver; the order is prove_steps'.
int create_proof_body(amdzk_ctx* ctx, amdzk_pk* const* pks, size_t NC, const uint64_t* const* const* instances_all,
                      const size_t* const* instance_lens_all, const void* const* d_advice_all, size_t advice_stride, const RandomSource& rng,
                      int transcript_kind, uint8_t* proof_out, size_t proof_cap, size_t* proof_len, const ProofExtras& ex) {
  const KeyMaterial& K = *pks[0]->key;
  if (!proof_len) ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof: null argument");
  for (size_t c = 0; c < NC; c++) {
    if (!pks[c] || (K.A && (!d_advice_all || !d_advice_all[c]))) ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof: null argument (circuit %zu)", c);
    ZK_TRY(check_handle(ctx, "create_proof", "circuit", pks, c));
  }
  if (advice_stride < K.n) ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof: advice stride < n");
  if (K.nphases > 1 && !ex.phase_fn)
    ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof: the key has advice in %u phases: amdzk_create_proof_opts with a phase callback is needed", K.nphases);
  const bool use_gwc = (transcript_kind & AMDZK_MULTIOPEN_GWC) != 0;
  transcript_kind &= ~AMDZK_MULTIOPEN_GWC;
  if (!ex.transcript && transcript_kind != AMDZK_TRANSCRIPT_BLAKE2B && transcript_kind != AMDZK_TRANSCRIPT_KECCAK256_EVM)
    ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof: unknown transcript kind %d", transcript_kind);
  if (ex.transcript && (!ex.transcript->common_point || !ex.transcript->common_scalar || !ex.transcript->write_point ||
                        !ex.transcript->write_scalar || !ex.transcript->squeeze_challenge))
    ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof: amdzk_transcript has a null member");
  for (size_t c = 0; c < NC; c++) ZK_TRY(zk_pk_poison(ctx, pks[c]));
  amdzk_ctx *B = ctx, *C = ctx;  // the lanes (Prover)
  if (K.use_lanes && NC == 1) {  // several instances: one stream (each lane holds one commitment batch's result at a time)
    ZK_TRY(zk_lane(ctx, 0, &B));
    ZK_TRY(zk_lane(ctx, 1, &C));
  }
  const bool serial = B == ctx;
  // latency mode of the commitments (common.hpp): while this proof runs on lanes; the caller's setting comes back at the end
  struct LatencyMode {
    amdzk_ctx* c[3];
    bool keep[3];
    LatencyMode(amdzk_ctx* m, amdzk_ctx* b, amdzk_ctx* cc, bool on) : c{m, b, cc} {
      for (int i = 0; i < 3; i++) keep[i] = c[i]->msm_latency_mode, c[i]->msm_latency_mode = on || keep[i];
    }
    ~LatencyMode() {
      for (int i = 0; i < 3; i++) c[i]->msm_latency_mode = keep[i];
    }
  } latency_mode(ctx, B, C, !serial && !(getenv("AMDZK_LATENCY_MODE") && atoi(getenv("AMDZK_LATENCY_MODE")) == 0));

  ProofIO io(ex.transcript, rng);
  zkhost::TranscriptWrite& T = io.T(transcript_kind);
  Prover P(ctx, pks, NC, B, C, T, io.rng);
  P.instances_all = instances_all;
  P.instance_lens_all = instance_lens_all;
  P.d_advice_all = d_advice_all;
  P.advice_stride = advice_stride;
  Solo solo{ctx, P, ex.phase_fn, ex.phase_user};
  ZK_TRY(prove_steps(solo, use_gwc, std::max<uint32_t>(K.nphases, 1)));
  *proof_len = T.proof.size();
  if (proof_out) {
    if (proof_cap < T.proof.size()) ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof: proof buffer too small (%zu < %zu)", proof_cap, T.proof.size());
    memcpy(proof_out, T.proof.data(), T.proof.size());
  }
  return AMDZK_OK;
}

int create_proof_impl(amdzk_ctx* ctx, amdzk_pk* const* pks, size_t ncirc, const uint64_t* const* const* instances,
                      const size_t* const* instance_lens, const void* const* d_advice, size_t advice_stride, const RandomSource& rng,
                      int transcript_kind, uint8_t* proof_out, size_t proof_cap, size_t* proof_len, const ProofExtras& ex = ProofExtras()) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  if (!pks || ncirc == 0 || !pks[0]) ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof: no proving key");
  // a failed proof may have left work on the lanes: the key's workspace must be quiet before it is used again
  return zk_quiet_if_refused(
      ctx, create_proof_body(ctx, pks, ncirc, instances, instance_lens, d_advice, advice_stride, rng, transcript_kind, proof_out, proof_cap, proof_len, ex), true);
}


// amdzk_create_proof_batch / _batch_opts: B independent proofs — of one circuit, or of different circuits on one SRS —
// advanced in lock-step on the caller's stream: prove_steps' other driver. Every member is a Prover of its own (one
// instance, no lanes, a sink for its commitments) with its own key, transcript, random source and workspace; what the
// members of a step have in common is done once for all of them:
//   * every commitment step — the random polynomial, advice (per challenge phase: one step each), A' / S', the permutation and lookup products (together),
//     the h pieces, SHPLONK's two or GWC's witnesses — is ONE pointer-table MSM (zk_msm_dev_xyzz_cols) over the live
//     members' columns, one host wait and one download, the points handed back per member (DeferredCommit);
//   * the lookup permutations' error words are read behind that step's wait;
//   * the evaluations of all members are one zk_poly_eval over the concatenated (polynomial, point) pairs and one download.
// One launch per member on the same stream: the compress / fraction / h(X) programs (their constant tables differ), the
// transforms, the lookup permutation, inversions and running products, the linear combinations and divisions of the
// opening argument, ChaCha blinding. No arithmetic differs from the single path, so the bytes do not either.
// A member whose witness fails (lookup input not in its table, a commitment that is the identity, beta = 0) gets its status
// and leaves the gang; the others go on. A failure of the device or of memory ends the batch for all.
struct Gang {
  struct Member {
    size_t index = 0;
    amdzk_pk* pk = nullptr;
    std::unique_ptr<ProofIO> io;  // amdzk_batch_proof_opts::transcripts[index], if the proof has one, or the built-in kind
    std::unique_ptr<Prover> P;
    std::vector<DeferredCommit> deferred;
    bool live = true;
    int status = AMDZK_OK;
    std::string err;
    zkhost::TranscriptWrite& T() { return P->T; }
  };
  amdzk_ctx* const ctx;
  std::vector<std::unique_ptr<Member>> members;
  int fatal = AMDZK_OK;  // a status that is not one witness's: the batch ends
  amdzk_batch_phase_fn phase_fn = nullptr;  // amdzk_batch_proof_opts: the batch's synthesize of phases >= 1
  void* phase_user = nullptr;
  size_t challenge_stride = 0;  // the largest number of challenges among the members' keys
  explicit Gang(amdzk_ctx* ctx) : ctx(ctx) {}

  void fail(Member& m, int r) {
    m.live = false;
    m.status = r;
    m.err = "proof " + std::to_string(m.index) + ": " + ctx->err;
    m.deferred.clear();
    if (r == AMDZK_E_HIP || r == AMDZK_E_NOMEM) fatal = r;
  }
  // one step of every live member, in index order
  template <class F>
  int each(F f) {
    for (auto& m : members) {
      if (!m->live) continue;
      const int r = f(*m->P);
      if (r != AMDZK_OK) fail(*m, r);
      else transcript_ok(*m);
      if (fatal != AMDZK_OK) return fatal;
    }
    return AMDZK_OK;
  }
  // a caller-owned transcript that reported an error ends its proof at the step boundary
  void transcript_ok(Member& m) {
    if (!m.live) return;
    const int r = transcript_status(ctx, m.T());
    if (r != AMDZK_OK) fail(m, r);
  }
  // device scratch of the gang's own (pointer tables, evaluation points and results). Valid until the next call (the slot may grow).
  // The kernels dereference the tables: never poisoned (workspace.hpp).
  int scratch(size_t bytes, char** out) { return zk_ws_reserve(ctx, ZK_WS_STAGING, bytes, (void**)out, true); }

  // The commitment batches the live members left in their sinks, as ONE submission per basis (a step has one basis; the products' step
  // two: the lookup products over g_lagrange, the permutation products' differences over its prefix sums), then
  // per member in the order it deferred them: into the Commit it named, or written to its transcript under the label.
  int commit_step() {
    for (int basis = 0; basis < AMDZK_NUM_BASES; basis++) {
      std::vector<const Fr*> cols;
      for (auto& m : members)
        if (m->live)
          for (auto& d : m->deferred)
            if (d.basis == basis)
              for (size_t c = 0; c < d.ncols; c++) cols.push_back(d.cols + c * m->pk->key->n);
      if (cols.empty()) continue;
      amdzk_pk* const pk0 = members[0]->pk;  // srs, n and the staging ring: any member's
      char* d_tab = nullptr;
      ZK_TRY(scratch(cols.size() * sizeof(Fr*), &d_tab));
      ZK_TRY(h2d_staged(ctx, pk0, d_tab, cols.data(), cols.size() * sizeof(Fr*)));
      G1X* d_res = nullptr;
      ZK_TRY(zk_msm_dev_xyzz_cols(ctx, pk0->key->srs, basis, (const Fr* const*)d_tab, cols.size(), pk0->key->n, 0, &d_res));
      PendingCommit pc;
      pc.ctx = ctx;
      pc.d_res = d_res;
      pc.ncols = cols.size();
      std::vector<G1Affine> pts;
      ZK_TRY(commit_finish(pc, pts));  // the wait: `cols` (if it went up unstaged) has been read
      size_t at = 0;
      for (auto& m : members) {
        if (!m->live) continue;
        for (auto& d : m->deferred) {
          if (d.basis != basis) continue;
          std::vector<G1Affine> mine(pts.begin() + at, pts.begin() + at + d.ncols);
          at += d.ncols;
          if (d.into) {
            d.into->pts.swap(mine);
            d.into->done = true;
          } else if (m->live) {
            const int r = m->P->write_points(mine, d.label);
            if (r != AMDZK_OK) {  // (clears m->deferred: leave its loop)
              const size_t rest_from = &d - m->deferred.data();
              for (size_t j = rest_from + 1; j < m->deferred.size(); j++)
                if (m->deferred[j].basis == basis) at += m->deferred[j].ncols;
              fail(*m, r);
              break;
            }
          }
        }
      }
    }
    for (auto& m : members) {
      m->deferred.clear();
      transcript_ok(*m);
    }
    return fatal;
  }

  // The callback of phase p >= 1 (amdzk_batch_phase_fn), once for the whole batch, if some live member's key has the phase.
  // The gang holds nothing across it: its device scratch is per step, and every member's work is on the stream.
  int phase_callback(uint32_t p) {
    const size_t N = members.size();
    std::vector<uint8_t> wanted(N, 0);
    std::vector<uint64_t> ch(std::max<size_t>(4 * N * challenge_stride, 1), 0);
    std::vector<int> rc(N, 0);
    bool any = false;
    for (auto& m : members)
      if (m->live && m->pk->key->nphases > p) {
        wanted[m->index] = 1;
        any = true;
        if (!m->P->chal.empty()) memcpy(&ch[4 * m->index * challenge_stride], m->P->chal.data(), m->P->chal.size() * 32);
      }
    if (!any) return AMDZK_OK;
    const int r = phase_fn(phase_user, p, N, wanted.data(), ch.data(), challenge_stride, rc.data(), (void*)ctx->stream);
    for (auto& m : members) {
      if (!m->live) continue;
      char b[160];
      if (r != 0 && wanted[m->index]) snprintf(b, sizeof(b), "create_proof: the phase callback returned %d in phase %u", r, p);
      else if (r == 0 && rc[m->index] != 0) snprintf(b, sizeof(b), "create_proof: the phase callback refused it in phase %u", p);
      else continue;
      ctx->err = b;
      fail(*m, AMDZK_E_INVALID);
    }
    return AMDZK_OK;
  }

  // all live members' evaluations (Prover::evaluations_prepare left the pairs) in one launch, one wait, one download
  int evaluate_step() {
    std::vector<const Fr*> pp;
    std::vector<Fr> pts;
    for (auto& m : members)
      if (m->live) {
        pp.insert(pp.end(), m->P->ev_pp.begin(), m->P->ev_pp.end());
        pts.insert(pts.end(), m->P->ev_pts.begin(), m->P->ev_pts.end());
      }
    const size_t nq = pp.size();
    if (!nq) return AMDZK_OK;
    amdzk_pk* const pk0 = members[0]->pk;
    const size_t o_pts = ws_round_up(nq * sizeof(Fr*), 256);
    char* d = nullptr;
    ZK_TRY(scratch(o_pts + 2 * nq * 32, &d));
    Fr* d_pts = (Fr*)(d + o_pts);
    ZK_TRY(h2d_staged(ctx, pk0, d, pp.data(), nq * sizeof(Fr*)));
    ZK_TRY(h2d_staged(ctx, pk0, d_pts, pts.data(), nq * 32));
    ZK_TRY(zk_poly_eval(ctx, (const Fr* const*)d, d_pts, d_pts + nq, nq, (uint32_t)pk0->key->n));
    std::vector<Fr> out(nq);
    ZK_TRY(d2h(ctx, out.data(), d_pts + nq, nq * 32));
    size_t at = 0;
    for (auto& m : members)
      if (m->live) {
        const size_t k = m->P->ev_pp.size();
        m->P->evals.assign(out.begin() + at, out.begin() + at + k);
        at += k;
      }
    return AMDZK_OK;
  }

};

}  // namespace

extern "C" {

// Number of Fr::random draws one create_proof makes for this key (DrawLayout).
size_t amdzk_proof_random_count(const amdzk_pk* pk) { return pk ? DrawLayout(*pk->key, 1).total : 0; }

// Length of the proof create_proof writes for this key: commitments — advice, 2 per lookup (A', S'), one per
// permutation set, one per lookup product, the random polynomial, the h pieces, SHPLONK's two — then the
// evaluations: advice and fixed queries, the random polynomial, sigma columns, 3 per permutation set but 2
// for the last, 5 per lookup. With AMDZK_MULTIOPEN_GWC the two SHPLONK points become one per opening point.
// Distinct evaluation points of the proof's queries = distinct rotations modulo n (omega^r x and omega^(r + n) x are one
// point, as in build_multiopen and the verifier's plan): what ProverGWC writes one witness commitment for.
static size_t opening_point_count(const KeyMaterial& K) {
  std::vector<int64_t> rots = {0};  // sigma columns, h(X), the random polynomial
  auto note = [&](int r) {
    const int64_t m = ((int64_t)r % (int64_t)K.n + (int64_t)K.n) % (int64_t)K.n;
    if (std::find(rots.begin(), rots.end(), m) == rots.end()) rots.push_back(m);
  };
  for (auto& q : K.advice_queries) note(q.second);
  for (auto& q : K.fixed_queries) note(q.second);
  if (K.nsets) note(1);
  if (K.nsets > 1) note(-(int)(K.bf + 1));
  if (K.L) {
    note(1);
    note(-1);
  }
  return rots.size();
}

size_t amdzk_proof_size(const amdzk_pk* pk, int format) { return amdzk_proof_size_multi(pk, 1, format); }

// create_proof with the caller's randomness: `scalars` = amdzk_proof_random_count(pk) Fr elements
// (Montgomery), drawn by the caller with Fr::random(&mut rng) in order.
int amdzk_create_proof_scalars(amdzk_ctx* ctx, amdzk_pk* pk, const uint64_t* const* instances, const size_t* instance_lens,
                               const void* d_advice, size_t advice_stride, const uint64_t* scalars, size_t scalar_count, int transcript_kind,
                               uint8_t* proof_out, size_t proof_cap, size_t* proof_len) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  if (!pk || !scalars) ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof_scalars: null argument");
  if (scalar_count < amdzk_proof_random_count(pk))
    ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof_scalars: %zu scalars given, %zu needed", scalar_count, amdzk_proof_random_count(pk));
  RandomSource rs;
  rs.scalars = scalars;
  return create_proof_impl(ctx, &pk, 1, &instances, &instance_lens, &d_advice, advice_stride, rs, transcript_kind, proof_out, proof_cap, proof_len);
}

int amdzk_create_proof(amdzk_ctx* ctx, amdzk_pk* pk, const uint64_t* const* instances, const size_t* instance_lens, const void* d_advice,
                       size_t advice_stride, uint64_t rng_seed, uint8_t* proof_out, size_t proof_cap, size_t* proof_len) {
  ZK_ENTER(ctx);
  return amdzk_create_proof_ex(ctx, pk, instances, instance_lens, d_advice, advice_stride, rng_seed, AMDZK_TRANSCRIPT_BLAKE2B, proof_out,
                               proof_cap, proof_len);
}

int amdzk_create_proof_ex(amdzk_ctx* ctx, amdzk_pk* pk, const uint64_t* const* instances, const size_t* instance_lens, const void* d_advice,
                          size_t advice_stride, uint64_t rng_seed, int transcript_kind, uint8_t* proof_out, size_t proof_cap,
                          size_t* proof_len) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  return create_proof_impl(ctx, &pk, 1, &instances, &instance_lens, &d_advice, advice_stride, RandomSource(rng_seed), transcript_kind, proof_out,
                           proof_cap, proof_len);
}

// plonk::create_proof(params, pk, &[circuit; N], &[instances; N], rng, transcript) [UP]: n_circuits instances of the
// key's circuit in ONE proof. pks[c]: instance c's workspace — pks[0] the key (or a clone), the others workspace clones of
// the same key, all different. instances[c][col] / instance_lens[c][col] and d_advice[c] as for amdzk_create_proof_ex.
int amdzk_create_proof_multi(amdzk_ctx* ctx, amdzk_pk* const* pks, size_t n_circuits, const uint64_t* const* const* instances,
                             const size_t* const* instance_lens, const void* const* d_advice, size_t advice_stride, uint64_t rng_seed,
                             int transcript_kind, uint8_t* proof_out, size_t proof_cap, size_t* proof_len) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  if (!pks || n_circuits == 0) ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof_multi: no circuits");
  return create_proof_impl(ctx, pks, n_circuits, instances, instance_lens, d_advice, advice_stride, RandomSource(rng_seed), transcript_kind,
                           proof_out, proof_cap, proof_len);
}

// create_proof with everything optional in one struct: the transcript (built-in or the caller's), the callback that
// synthesizes the later phases of a phased key, the randomness (seed or the caller's scalars).
int amdzk_create_proof_opts(amdzk_ctx* ctx, amdzk_pk* const* pks, size_t n_circuits, const uint64_t* const* const* instances,
                            const size_t* const* instance_lens, const void* const* d_advice, size_t advice_stride, const amdzk_proof_opts* opts,
                            uint8_t* proof_out, size_t proof_cap, size_t* proof_len) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  if (!pks || n_circuits == 0 || !pks[0]) ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof_opts: no circuits");
  if (!opts) ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof_opts: null options");
  if (opts->size < sizeof(amdzk_proof_opts))
    ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof_opts: amdzk_proof_opts.size is %zu, this library needs %zu", opts->size, sizeof(amdzk_proof_opts));
  RandomSource rs;
  if (opts->scalars) {
    const size_t need = DrawLayout(*pks[0]->key, n_circuits).total;
    if (opts->scalar_count < need) ZK_FAIL(ctx, AMDZK_E_INVALID, "create_proof_opts: %zu scalars given, %zu needed", opts->scalar_count, need);
    rs.scalars = opts->scalars;
  } else {
    rs = RandomSource(opts->rng_seed);
  }
  ProofExtras ex;
  ex.transcript = opts->transcript;
  ex.phase_fn = opts->phase_fn;
  ex.phase_user = opts->phase_user;
  return create_proof_impl(ctx, pks, n_circuits, instances, instance_lens, d_advice, advice_stride, rs, opts->transcript_kind, proof_out, proof_cap,
                           proof_len, ex);
}

// The body of both batch entry points, behind their refusals: one Gang member per proof, the run, and every proof's bytes,
// length and status. A proof with a transcript of its own has length 0: the bytes are its caller's.
static int prove_gang(amdzk_ctx* ctx, amdzk_pk* const* pks, size_t n_proofs, const uint64_t* const* const* instances,
                      const size_t* const* instance_lens, const void* const* d_advice, size_t advice_stride,
                      const amdzk_batch_proof_opts& o, uint8_t* proofs_out, size_t proof_stride, size_t* proof_lens, int* statuses) {
  const bool use_gwc = (o.transcript_kind & AMDZK_MULTIOPEN_GWC) != 0;
  const int kind = o.transcript_kind & ~AMDZK_MULTIOPEN_GWC;
  // (every member owns its arenas from here to the end of the batch: poisoned once, in front of the first step)
  for (size_t b = 0; b < n_proofs; b++) ZK_TRY(zk_pk_poison(ctx, pks[b]));
  Gang g(ctx);
  g.phase_fn = o.phase_fn;
  g.phase_user = o.phase_user;
  uint32_t phases = 1;  // the largest phase count among the members' keys: the others sit the later phases out
  for (size_t b = 0; b < n_proofs; b++) {
    std::unique_ptr<Gang::Member> m(new Gang::Member);
    m->index = b;
    m->pk = pks[b];
    phases = std::max(phases, pks[b]->key->nphases);
    g.challenge_stride = std::max<size_t>(g.challenge_stride, pks[b]->key->num_challenges);
    RandomSource rng;
    if (o.scalars) rng.scalars = o.scalars[b];
    else rng = RandomSource(o.rng_seeds[b]);
    m->io.reset(new ProofIO(o.transcripts ? o.transcripts[b] : nullptr, rng));
    m->P.reset(new Prover(ctx, &pks[b], 1, ctx, ctx, m->io->T(kind), m->io->rng));  // B = C = ctx: one stream, no lanes
    m->P->sink = &m->deferred;
    m->P->instances_all = instances ? instances + b : nullptr;
    m->P->instance_lens_all = instance_lens ? instance_lens + b : nullptr;
    m->P->d_advice_all = d_advice ? d_advice + b : nullptr;
    m->P->advice_stride = advice_stride;
    g.members.push_back(std::move(m));
  }
  const int run = prove_steps(g, use_gwc, phases);
  int first = AMDZK_OK;
  std::string first_err;
  for (auto& m : g.members) {
    if (m->live && run != AMDZK_OK) {  // the batch ended under it
      m->live = false;
      m->status = run;
      m->err = ctx->err;
    }
    if (m->live && m->T().proof.size() > proof_stride) {  // (cannot happen: amdzk_proof_size is exact)
      m->live = false;
      m->status = AMDZK_E_INVALID;
      m->err = "proof " + std::to_string(m->index) + ": create_proof: proof buffer too small";
    }
    if (statuses) statuses[m->index] = m->status;
    proof_lens[m->index] = m->live ? m->T().proof.size() : 0;
    if (m->live && !m->T().proof.empty()) memcpy(proofs_out + m->index * proof_stride, m->T().proof.data(), m->T().proof.size());
    else if (!m->live && first == AMDZK_OK) first = m->status, first_err = m->err;
  }
  if (first != AMDZK_OK) ctx->err = first_err;
  return zk_quiet_if_refused(ctx, first, true);  // a failed proof may have left work behind: the workspaces must be quiet before they are used again
}

// What either batch entry point was asked for, in amdzk_create_proof_batch_opts' terms. `who` prefixes the refusals.
// strict (amdzk_create_proof_batch): every handle is the first key or a workspace clone of it, no challenge phases, and
// therefore no callback and no transcripts of the caller's. opts_size: where the caller's options say their size (null: no
// options were given); `o` holds their fields once that size is large enough.
struct BatchCall {
  const char* who;
  bool strict;
  const char* opts_name;
  size_t opts_need;
  const size_t* opts_size;
  amdzk_batch_proof_opts o;
};

// The refusals of both batch entry points: AMDZK_OK, or the batch is refused as a whole.
static int batch_refusals(amdzk_ctx* ctx, const BatchCall& c, amdzk_pk* const* pks, size_t n_proofs, const void* const* d_advice,
                          size_t advice_stride, const uint8_t* proofs_out, size_t proof_stride, const size_t* proof_lens) {
  const char* const who = c.who;
  const amdzk_batch_proof_opts& o = c.o;
  if (!pks || n_proofs == 0) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: no proofs", who);
  if (!c.opts_size || !proof_lens) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: null argument", who);
  if (*c.opts_size < c.opts_need)
    ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: %s.size is %zu, this library needs %zu", who, c.opts_name, *c.opts_size, c.opts_need);
  if (!o.rng_seeds && !o.scalars) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: neither rng_seeds nor scalars", who);
  size_t psize = 0;
  bool builtin = false;
  for (size_t b = 0; b < n_proofs; b++) {
    if (!pks[b]) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: null key (proof %zu)", who, b);
    const KeyMaterial& K = *pks[b]->key;
    if (c.strict) ZK_TRY(check_handle(ctx, who, "proof", pks, b));  // the first key's, and no handle twice
    if (K.srs != pks[0]->key->srs)
      ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: proof %zu's key was made on another amdzk_srs than proof 0's: the batch commits over one SRS", who, b);
    for (size_t d = 0; d < b; d++)
      if (pks[d] == pks[b]) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: proofs %zu and %zu share one workspace", who, d, b);
    if (K.A && (!d_advice || !d_advice[b])) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: null advice (proof %zu)", who, b);
    if (o.scalars && !o.scalars[b]) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: null scalars (proof %zu)", who, b);
    if (c.strict && K.phased())
      ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "%s: the key has challenge phases or challenges: prove it with amdzk_create_proof_opts", who);
    if (K.nphases > 1 && !o.phase_fn)
      ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: proof %zu's key has advice in %u phases: a phase callback is needed", who, b, K.nphases);
    if (advice_stride < K.n) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: advice stride < n", who);
    const size_t draws = DrawLayout(K, 1).total;
    if (o.scalars && o.scalar_count < draws) {
      if (c.strict) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: %zu scalars given, %zu needed", who, o.scalar_count, draws);
      ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: %zu scalars given, proof %zu needs %zu", who, o.scalar_count, b, draws);
    }
    const amdzk_transcript* t = o.transcripts ? o.transcripts[b] : nullptr;
    if (t && (!t->common_point || !t->common_scalar || !t->write_point || !t->write_scalar || !t->squeeze_challenge))
      ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: amdzk_transcript of proof %zu has a null member", who, b);
    if (!t) {
      builtin = true;
      psize = std::max(psize, amdzk_proof_size(pks[b], o.transcript_kind));
    }
  }
  if (builtin) {  // some proof's bytes are written here
    const int kind = o.transcript_kind & ~AMDZK_MULTIOPEN_GWC;
    if (kind != AMDZK_TRANSCRIPT_BLAKE2B && kind != AMDZK_TRANSCRIPT_KECCAK256_EVM) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: unknown transcript kind %d", who, kind);
    if (!proofs_out) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: null argument", who);
    if (proof_stride < psize) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: proof_stride %zu < proof size %zu", who, proof_stride, psize);
  }
  return AMDZK_OK;
}

// Both batch entry points behind their adapters. A batch that is refused as a whole starts no proof, and every proof says so.
static int proof_batch(amdzk_ctx* ctx, const BatchCall& c, amdzk_pk* const* pks, size_t n_proofs, const uint64_t* const* const* instances,
                       const size_t* const* instance_lens, const void* const* d_advice, size_t advice_stride, uint8_t* proofs_out,
                       size_t proof_stride, size_t* proof_lens, int* statuses) {
  const int r = batch_refusals(ctx, c, pks, n_proofs, d_advice, advice_stride, proofs_out, proof_stride, proof_lens);
  if (r == AMDZK_OK)
    return prove_gang(ctx, pks, n_proofs, instances, instance_lens, d_advice, advice_stride, c.o, proofs_out, proof_stride, proof_lens, statuses);
  for (size_t b = 0; b < n_proofs; b++) {
    if (statuses) statuses[b] = r;
    if (proof_lens) proof_lens[b] = 0;
  }
  return r;
}

// n_proofs independent proofs of one circuit from one host thread, advanced in lock-step (Gang above). pks[b]: proof b's
// workspace — the key or workspace clones of it, pairwise different. Bytes: those of n_proofs amdzk_create_proof_ex /
// amdzk_create_proof_scalars calls.
int amdzk_create_proof_batch(amdzk_ctx* ctx, amdzk_pk* const* pks, size_t n_proofs, const uint64_t* const* const* instances,
                             const size_t* const* instance_lens, const void* const* d_advice, size_t advice_stride,
                             const amdzk_batch_opts* opts, uint8_t* proofs_out, size_t proof_stride, size_t* proof_lens, int* statuses) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  BatchCall c = {"create_proof_batch", true, "amdzk_batch_opts", sizeof(amdzk_batch_opts), opts ? &opts->size : nullptr, {}};
  if (opts && opts->size >= sizeof(amdzk_batch_opts)) {
    c.o.transcript_kind = opts->transcript_kind;
    c.o.rng_seeds = opts->rng_seeds;
    c.o.scalars = opts->scalars;
    c.o.scalar_count = opts->scalar_count;
  }
  return proof_batch(ctx, c, pks, n_proofs, instances, instance_lens, d_advice, advice_stride, proofs_out, proof_stride, proof_lens, statuses);
}

// amdzk_create_proof_batch for what it refuses: keys with challenge phases, proofs with the caller's transcript, and different
// circuits on one SRS (include/amdzk.h).
int amdzk_create_proof_batch_opts(amdzk_ctx* ctx, amdzk_pk* const* pks, size_t n_proofs, const uint64_t* const* const* instances,
                                  const size_t* const* instance_lens, const void* const* d_advice, size_t advice_stride,
                                  const amdzk_batch_proof_opts* opts, uint8_t* proofs_out, size_t proof_stride, size_t* proof_lens, int* statuses) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  BatchCall c = {"create_proof_batch_opts", false, "amdzk_batch_proof_opts", sizeof(amdzk_batch_proof_opts), opts ? &opts->size : nullptr, {}};
  if (opts && opts->size >= sizeof(amdzk_batch_proof_opts)) c.o = *opts;
  return proof_batch(ctx, c, pks, n_proofs, instances, instance_lens, d_advice, advice_stride, proofs_out, proof_stride, proof_lens, statuses);
}

// Byte length of the proof amdzk_create_proof_multi writes for n_circuits instances (amdzk_proof_size for one).
size_t amdzk_proof_size_multi(const amdzk_pk* pk, size_t n_circuits, int format) {
  if (!pk || n_circuits == 0) return 0;
  const KeyMaterial& K = *pk->key;
  const int transcript_kind = format & 0xff;
  const size_t openings = (format & AMDZK_MULTIOPEN_GWC) ? opening_point_count(K) : 2;
  const size_t points = n_circuits * ((size_t)K.A + 2 * (size_t)K.L + K.nsets + K.L) + 1 + K.qdeg + openings;
  const size_t scalars = n_circuits * (K.advice_queries.size() + (K.nsets ? 3 * (size_t)K.nsets - 1 : 0) + 5 * (size_t)K.L) +
                         K.fixed_queries.size() + 1 + K.S;
  return points * (transcript_kind == AMDZK_TRANSCRIPT_KECCAK256_EVM ? 64 : 32) + scalars * 32;
}

// ---- function-by-function entry points of the PLONK layer: the same kernels create_proof runs,
// callable on their own — by the isolated parity tests and by a fork that replaces upstream one function at a time.

// evaluate_h and the quotient: d_polys = the NP = A + I + 2L + nsets + L committed polynomials in COEFFICIENT form, n
// each, in the key's arena order [advice | instance | permuted inputs A' | permuted tables S' | permutation products
// | lookup products]; the challenges as Montgomery Fr. Writes the cs_degree - 1 pieces of h(X) (n coefficients each)
// to d_pieces_out. Uses (and overwrites) the key's per-proof workspace.
int amdzk_quotient_eval_dev(amdzk_ctx* ctx, amdzk_pk* pk, const void* d_polys, size_t poly_stride, const uint64_t theta[4],
                            const uint64_t beta[4], const uint64_t gamma[4], const uint64_t y[4], void* d_pieces_out) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  if (!pk || !d_polys || !theta || !beta || !gamma || !y || !d_pieces_out) ZK_FAIL(ctx, AMDZK_E_INVALID, "quotient_eval: null argument");
  const KeyMaterial& K = *pk->key;
  if (poly_stride < K.n) ZK_FAIL(ctx, AMDZK_E_INVALID, "quotient_eval: stride < n");
  ZK_HIP(ctx, hipMemcpy2DAsync(pk->PQ, K.n * 32, d_polys, poly_stride * 32, K.n * 32, K.NP, hipMemcpyDeviceToDevice, ctx->stream));
  memcpy(pk->consts[K.c_theta].l, theta, 32);
  memcpy(pk->consts[K.c_beta].l, beta, 32);
  memcpy(pk->consts[K.c_gamma].l, gamma, 32);
  memcpy(pk->consts[K.c_y].l, y, 32);
  if (K.S && pk->consts[K.c_beta].is_zero()) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "quotient_eval: beta is zero");
  pk->consts[K.c_betainv] = inv(pk->consts[K.c_beta]);
  ZK_TRY(quotient_pieces(ctx, pk));
  ZK_TRY(d2d(ctx, d_pieces_out, pk->hpieces, (size_t)K.qdeg * K.n * 32));
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  return AMDZK_OK;
}

// permutation::prover::Argument::commit before the blinding, on the columns the key's workspace holds (the advice and
// instance columns of its last proof): rows 0 ... usable (= n - blinding_factors - 1) of the nsets product columns to `out`,
// nsets x (usable + 1) Fr on the host, column after column. route 0: the fraction program over every row; 1: from the
// key's list of cells that are off the identity permutation (refused for a key that keeps none: more than half of its
// cells are listed); -1: the route the key's proofs take. *cells_out = the listed cells, *sparse_out = whether proofs
// take route 1 (either may be NULL; out = NULL only queries them). Overwrites the key's per-proof workspace.
int amdzk_perm_products_dev(amdzk_ctx* ctx, amdzk_pk* pk, const uint64_t beta[4], const uint64_t gamma[4], int route, uint64_t* out,
                            size_t* cells_out, int* sparse_out) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  if (!pk) ZK_FAIL(ctx, AMDZK_E_INVALID, "perm_products: null key");
  const KeyMaterial& K = *pk->key;
  if (cells_out) *cells_out = K.perm_m;
  if (sparse_out) *sparse_out = K.perm_sparse ? 1 : 0;
  if (!out) return AMDZK_OK;
  if (!beta || !gamma) ZK_FAIL(ctx, AMDZK_E_INVALID, "perm_products: null argument");
  if (route < -1 || route > 1) ZK_FAIL(ctx, AMDZK_E_INVALID, "perm_products: unknown route %d", route);
  if (route == 1 && !K.perm_sparse) ZK_FAIL(ctx, AMDZK_E_INVALID, "perm_products: the key keeps no list of cells (%zu listed)", K.perm_m);
  if (!K.S) return AMDZK_OK;
  memcpy(pk->consts[K.c_beta].l, beta, 32);
  memcpy(pk->consts[K.c_gamma].l, gamma, 32);
  if (pk->consts[K.c_beta].is_zero()) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "perm_products: beta is zero");
  pk->consts[K.c_betainv] = inv(pk->consts[K.c_beta]);
  ZK_TRY(h2d(ctx, pk->d_consts + K.c_beta, &pk->consts[K.c_beta], (size_t)(K.c_betainv + 1 - K.c_beta) * 32));
  ZK_TRY(perm_products_unblinded(ctx, pk, route < 0 ? K.perm_sparse : route == 1));
  const size_t rows = K.n - K.bf;  // usable + 1
  ZK_HIP(ctx, hipMemcpy2DAsync(out, rows * 32, pk->zp(), K.n * 32, rows * 32, K.nsets, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  return AMDZK_OK;
}

// lookup::prover::permute_expression_pair for nlookups (input, table) pairs of n rows each, Montgomery form,
// column l at + l * n: d_inputs is sorted in place into A', d_permuted_tables_out receives S'; rows >= usable of both
// are zero. Fails with "not in table" when an input value is missing from its table.
int amdzk_permute_expression_pair_dev(amdzk_ctx* ctx, void* d_inputs, const void* d_tables, void* d_permuted_tables_out, size_t nlookups,
                                      uint32_t n, uint32_t usable) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  if (!d_inputs || !d_tables || !d_permuted_tables_out) ZK_FAIL(ctx, AMDZK_E_INVALID, "permute_expression_pair: null argument");
  if (n < 2 || (n & (n - 1)) || usable > n) ZK_FAIL(ctx, AMDZK_E_INVALID, "permute_expression_pair: n must be a power of two >= usable");
  char* ws = nullptr;  // Ts[L][n] | left[L][n] | flags 4 x L x (n + 8) | err
  const size_t L = nlookups, col = L * (size_t)n * 32, fl = 4 * L * ((size_t)n + 8) * 4;
  ZK_TRY(zk_ws_reserve(ctx, ZK_WS_PERMUTE, 2 * col + fl + 256, (void**)&ws));
  if (L == 0) return AMDZK_OK;
  ZK_TRY(zk_permute_expression_pairs(ctx, (Fr*)d_inputs, (const Fr*)d_tables, (Fr*)ws, (Fr*)d_permuted_tables_out, (Fr*)(ws + col),
                                     (uint32_t*)(ws + 2 * col), (int*)(ws + 2 * col + fl), L, n, usable));
  return zk_permute_check(ctx, (const int*)(ws + 2 * col + fl));
}

}  // extern "C"
