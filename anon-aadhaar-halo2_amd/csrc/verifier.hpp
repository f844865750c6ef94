// The host half of amdzk_verify_proofs (include/amdzk.h): plonk::verify_proof [UP] from the decoded proof
// elements up to one scalar per base for each of the two sums of the final pairing check. Host-only: no HIP include,
// compiles with g++ (tests/native/verifier_check.cpp runs it alone, also under ASan + UBSan; tests/native/
// verifier_read_check.cpp through the caller's read transcript). A proof is walked in read order once (run_transcript) over
// a Source — the built-in transcripts or the caller's callbacks — which leaves its Challenges; fold_challenges is the rest.
//
// Inputs are plain data: the circuit as keygen was given it (pkblob::Desc), the number of circuit instances per proof, the
// transcript kind, transcript_repr, omega, the public inputs, the proof's points and scalars already decoded (affine /
// Montgomery: verify.hip's decode kernel, or a test) and the proof's weight rho. Output: for every base one scalar of
//   L = z_0(u) h2                                                   (SHPLONK)      L = sum_i u^i W_i                    (GWC)
//   R = sum_i v^i z_i(u) sum_j y^j (C_ij - r_ij(u) G) - Z_T(u) h1 + u z_0(u) h2    R = sum_i u^i (z_i W_i + C_i - e_i G)
// both times rho, so that the proof is valid iff e(L, [s]_2) = e(R, [1]_2). Bases are numbered
//   [0, NP)  the proof's own points in the order they are read | NP + c  fixed commitment c | NP + F + i  permutation
//   commitment i | NP + F + S  G = g[0] of the SRS.
// The h(X) commitment is no base: its scalar is spread over the pieces with powers of x^n.
#pragma once
#include <stdint.h>
#include <string.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "opening.hpp"
#include "pkblob.hpp"
#include "workspace.hpp"

namespace verifier {

using bn254::Fr;
using bn254::G1Affine;

constexpr uint32_t NO_SCALAR = 0xffffffffu;

// Where everything is: the byte layout of a proof (a function of the circuit, the number of instances and the transcript
// kind alone), the read order, the query list in the prover's order and its grouping for the opening argument (opening.hpp).
struct Plan {
  const pkblob::Desc* d = nullptr;
  uint32_t N = 1;
  bool evm = false, gwc = false;
  uint32_t k = 0, A = 0, F = 0, I = 0, S = 0, L = 0, nsets = 0, chunk = 0, qdeg = 0, bf = 0, nphases = 1;
  uint64_t n = 0;
  std::vector<uint8_t> adv_phase;  // per advice column (all 0 for a key without phases)
  struct Elem {
    uint32_t offset;    // byte offset in the proof
    uint32_t is_point;  // 1: a point (32 bytes compressed, or 64 bytes x | y), 0: a scalar (32 bytes)
    uint32_t index;     // among the proof's points / scalars, in read order
  };
  std::vector<Elem> elems;  // in read order
  uint32_t NP = 0, NS = 0;  // points and scalars of one proof
  size_t proof_bytes = 0;
  // points
  std::vector<uint32_t> adv_pt, la_pt, ls_pt, z_pt, lz_pt;  // [c * A + col], [c * L + l] x 2, [c * nsets + s], [c * L + l]
  uint32_t rand_pt = 0, h_pt = 0, open_pt = 0;              // h_pt: first of qdeg pieces; open_pt: h1, h2 or the W_z
  // scalars
  std::vector<uint32_t> adv_sc, z_sc, lk_sc;  // [c] first advice evaluation; [c * nsets + s] first of 2 or 3; [c * L + l] first of 5
  uint32_t fix_sc = 0, rand_sc = 0, sig_sc = 0;
  std::map<std::pair<int, int>, uint32_t> advice_q, fixed_q, instance_q;  // (column, rotation) -> query index
  // bases
  uint32_t base_fixed = 0, base_perm = 0, base_g = 0, key_h = 0, n_bases = 0;
  struct Query {
    uint32_t key;  // base index, or key_h
    int32_t rot;
    uint32_t sc;   // scalar index of the claimed evaluation, NO_SCALAR: the vanishing identity's
    uint32_t rot_id;
  };
  std::vector<Query> queries;
  std::vector<int32_t> rots;  // distinct evaluation points as rotations of x, first seen first
  opening::Grouping grp;      // over (key, rot_id): SHPLONK's rotation sets, GWC's queries of every distinct point
};

inline int plan_fail(std::string* err, const char* msg) {
  if (err) *err = std::string("verify_proofs: ") + msg;
  return AMDZK_E_INVALID;
}

// d must have passed pkblob::validate (every key has). transcript_kind as for amdzk_create_proof_ex.
inline int make_plan(const pkblob::Desc& d, uint32_t n_circuits, int transcript_kind, Plan* out, std::string* err) {
  Plan& p = *out;
  p = Plan();
  const int tk = transcript_kind & 0xff;
  if ((transcript_kind & ~(0xff | AMDZK_MULTIOPEN_GWC)) || (tk != AMDZK_TRANSCRIPT_BLAKE2B && tk != AMDZK_TRANSCRIPT_KECCAK256_EVM))
    return plan_fail(err, "unknown transcript kind");
  if (n_circuits == 0 || n_circuits > (1u << 16)) return plan_fail(err, "n_circuits out of range");
  p.d = &d, p.N = n_circuits, p.evm = tk == AMDZK_TRANSCRIPT_KECCAK256_EVM, p.gwc = (transcript_kind & AMDZK_MULTIOPEN_GWC) != 0;
  p.k = d.k, p.n = (uint64_t)1 << d.k, p.A = d.num_advice, p.F = d.num_fixed, p.I = d.num_instance, p.S = d.num_perm_columns();
  p.L = d.num_lookups, p.chunk = d.cs_degree - 2, p.nsets = (p.S + p.chunk - 1) / p.chunk, p.qdeg = d.cs_degree - 1, p.bf = d.blinding_factors;
  p.adv_phase.assign(p.A, 0);
  if (d.has_phases) p.adv_phase = d.advice_phase;
  p.nphases = 1;
  for (uint8_t ph : p.adv_phase) p.nphases = ph + 1u > p.nphases ? ph + 1u : p.nphases;
  for (uint8_t ph : d.challenge_phase) p.nphases = ph + 1u > p.nphases ? ph + 1u : p.nphases;
  const uint32_t N = p.N, psz = p.evm ? 64 : 32;
  size_t off = 0;
  auto point = [&]() {
    p.elems.push_back({(uint32_t)off, 1, p.NP});
    off += psz;
    return p.NP++;
  };
  auto scalar = [&]() {
    p.elems.push_back({(uint32_t)off, 0, p.NS});
    off += 32;
    return p.NS++;
  };
  for (size_t i = 0; i < d.advice_queries.size(); i += 2) p.advice_q[{d.advice_queries[i], d.advice_queries[i + 1]}] = (uint32_t)(i / 2);
  for (size_t i = 0; i < d.fixed_queries.size(); i += 2) p.fixed_q[{d.fixed_queries[i], d.fixed_queries[i + 1]}] = (uint32_t)(i / 2);
  for (size_t i = 0; i < d.instance_queries.size(); i += 2) p.instance_q[{d.instance_queries[i], d.instance_queries[i + 1]}] = (uint32_t)(i / 2);
  // everything a later index must find
  for (size_t i = 0; i < d.perm_columns.size(); i += 2) {
    const uint32_t kind = d.perm_columns[i];
    const std::pair<int, int> key{(int)d.perm_columns[i + 1], 0};
    const auto& m = kind == 0 ? p.advice_q : kind == 1 ? p.fixed_q : p.instance_q;
    if (!m.count(key)) return plan_fail(err, "a permutation column is not queried at rotation 0");
  }
  for (uint32_t w : d.expr_words) {
    const uint32_t op = w >> 24, pl = w & 0xffffffu;
    if (op < 2 || op > 4) continue;
    const std::pair<int, int> key{(int)(pl >> 8), (int)(pl & 0xff) - 128};
    const auto& m = op == 3 ? p.advice_q : op == 2 ? p.fixed_q : p.instance_q;
    if (!m.count(key)) return plan_fail(err, "an expression reads a cell that is in no query list");
  }
  const size_t nq_adv = d.advice_queries.size() / 2, nq_fix = d.fixed_queries.size() / 2;
  // read order: advice commitments phase after phase, inside a phase instance after instance
  p.adv_pt.assign((size_t)N * p.A, 0);
  for (uint32_t ph = 0; ph < p.nphases; ph++)
    for (uint32_t c = 0; c < N; c++)
      for (uint32_t a = 0; a < p.A; a++)
        if (p.adv_phase[a] == ph) p.adv_pt[(size_t)c * p.A + a] = point();
  p.la_pt.resize((size_t)N * p.L), p.ls_pt.resize((size_t)N * p.L), p.lz_pt.resize((size_t)N * p.L), p.z_pt.resize((size_t)N * p.nsets);
  for (uint32_t c = 0; c < N; c++)
    for (uint32_t l = 0; l < p.L; l++) p.la_pt[(size_t)c * p.L + l] = point(), p.ls_pt[(size_t)c * p.L + l] = point();
  for (uint32_t c = 0; c < N; c++)
    for (uint32_t s = 0; s < p.nsets; s++) p.z_pt[(size_t)c * p.nsets + s] = point();
  for (uint32_t c = 0; c < N; c++)
    for (uint32_t l = 0; l < p.L; l++) p.lz_pt[(size_t)c * p.L + l] = point();
  p.rand_pt = point();
  p.h_pt = p.NP;
  for (uint32_t i = 0; i < p.qdeg; i++) point();
  p.adv_sc.resize(N), p.z_sc.resize((size_t)N * p.nsets), p.lk_sc.resize((size_t)N * p.L);
  for (uint32_t c = 0; c < N; c++) {
    p.adv_sc[c] = p.NS;
    for (size_t q = 0; q < nq_adv; q++) scalar();
  }
  p.fix_sc = p.NS;
  for (size_t q = 0; q < nq_fix; q++) scalar();
  p.rand_sc = scalar();
  p.sig_sc = p.NS;
  for (uint32_t i = 0; i < p.S; i++) scalar();
  for (uint32_t c = 0; c < N; c++)
    for (uint32_t s = 0; s < p.nsets; s++) {
      p.z_sc[(size_t)c * p.nsets + s] = scalar();
      scalar();
      if (s + 1 < p.nsets) scalar();
    }
  for (uint32_t c = 0; c < N; c++)
    for (uint32_t l = 0; l < p.L; l++) {
      p.lk_sc[(size_t)c * p.L + l] = scalar();
      for (int i = 0; i < 4; i++) scalar();
    }
  // bases behind the proof's points (the opening points are appended to NP below)
  // queries, in the prover's order
  const int32_t last_rot = -(int32_t)(p.bf + 1);
  std::vector<Plan::Query> qs;
  auto Q = [&](uint32_t key, int32_t rot, uint32_t sc) { qs.push_back({key, rot, sc, 0}); };
  // keys of the VK and of h are patched once NP is final: mark them with the top bits
  constexpr uint32_t VK = 0x80000000u, HK = 0xc0000000u;
  for (uint32_t c = 0; c < N; c++) {
    for (size_t q = 0; q < nq_adv; q++) Q(p.adv_pt[(size_t)c * p.A + d.advice_queries[2 * q]], d.advice_queries[2 * q + 1], p.adv_sc[c] + (uint32_t)q);
    for (uint32_t s = 0; s < p.nsets; s++) {
      const uint32_t z = p.z_pt[(size_t)c * p.nsets + s], e = p.z_sc[(size_t)c * p.nsets + s];
      Q(z, 0, e);
      Q(z, 1, e + 1);
    }
    for (uint32_t s = p.nsets > 0 ? p.nsets - 1 : 0; s-- > 0;) Q(p.z_pt[(size_t)c * p.nsets + s], last_rot, p.z_sc[(size_t)c * p.nsets + s] + 2);
    for (uint32_t l = 0; l < p.L; l++) {
      const size_t i = (size_t)c * p.L + l;
      const uint32_t e = p.lk_sc[i];  // lz(x), lz(wx), la(x), la(w^-1 x), ls(x)
      Q(p.lz_pt[i], 0, e);
      Q(p.la_pt[i], 0, e + 2);
      Q(p.ls_pt[i], 0, e + 4);
      Q(p.la_pt[i], -1, e + 3);
      Q(p.lz_pt[i], 1, e + 1);
    }
  }
  for (size_t q = 0; q < nq_fix; q++) Q(VK | (uint32_t)d.fixed_queries[2 * q], d.fixed_queries[2 * q + 1], p.fix_sc + (uint32_t)q);
  for (uint32_t i = 0; i < p.S; i++) Q(VK | (p.F + i), 0, p.sig_sc + i);
  Q(HK, 0, NO_SCALAR);
  Q(p.rand_pt, 0, p.rand_sc);
  // distinct points: rotations that differ by a multiple of n name the same point
  auto rot_mod = [&](int32_t r) { return (uint64_t)(((int64_t)r % (int64_t)p.n + (int64_t)p.n) % (int64_t)p.n); };
  for (auto& q : qs) {
    uint32_t id = 0;
    for (; id < p.rots.size(); id++)
      if (rot_mod(p.rots[id]) == rot_mod(q.rot)) break;
    if (id == p.rots.size()) p.rots.push_back(q.rot);
    q.rot_id = id;
  }
  p.open_pt = p.NP;
  const uint32_t n_open = p.gwc ? (uint32_t)p.rots.size() : 2;
  for (uint32_t i = 0; i < n_open; i++) point();
  p.proof_bytes = off;
  p.base_fixed = p.NP, p.base_perm = p.NP + p.F, p.base_g = p.NP + p.F + p.S, p.key_h = p.base_g + 1, p.n_bases = p.base_g + 1;
  for (auto& q : qs) {
    if ((q.key & HK) == HK) q.key = p.key_h;
    else if (q.key & VK) q.key = p.base_fixed + (q.key & ~VK);
  }
  p.queries = qs;
  std::vector<opening::Query> oq;
  for (auto& q : qs) oq.push_back({q.key, q.rot_id});
  p.grp = opening::group(oq.data(), oq.size(), p.key_h + 1, p.rots.size());
  return AMDZK_OK;
}

// ---- small field helpers
inline Fr fr_small(uint64_t v) {
  Fr a = Fr::zero();
  a.l[0] = (uint32_t)v, a.l[1] = (uint32_t)(v >> 32);
  return bn254::to_mont(a);
}
inline bool fr_canonical_words(const uint64_t w[4]) {  // Montgomery or not: a residue below the modulus
  Fr a;
  memcpy(a.l, w, 32);
  return bn254::reduce_once(a) == a;
}
inline Fr fr_pow2k(Fr a, uint32_t k) {
  for (uint32_t i = 0; i < k; i++) a = bn254::sqr(a);
  return a;
}
inline Fr fr_pow_signed(const Fr& w, const Fr& winv, int64_t e) { return e >= 0 ? bn254::pow_u64(w, (uint64_t)e) : bn254::pow_u64(winv, (uint64_t)(-e)); }

// ---- where a proof's challenges come from. The verifier walks a proof in read order once (run_transcript) and hands every
// step to a Source: the public inputs, the elements, the squeezes. A member returns false when the source failed; the walk
// ends there.
class Source {
 public:
  virtual ~Source() {}
  virtual bool common_scalar(const Fr& s) = 0;
  virtual bool element(size_t e, const Plan::Elem& el) = 0;  // element e of the read order is next
  virtual bool squeeze(Fr* out) = 0;
};

// The built-in transcripts: the write classes absorb what the device has already decoded (no decompression here).
class BuiltinSource : public Source {
 public:
  BuiltinSource(bool evm, const G1Affine* pts, const Fr* scs) : T_(evm ? (zkhost::TranscriptWrite&)tk_ : (zkhost::TranscriptWrite&)tb_), pts_(pts), scs_(scs) {}
  bool common_scalar(const Fr& s) override { return T_.common_scalar(s), true; }
  bool element(size_t, const Plan::Elem& el) override {
    if (el.is_point) T_.common_point(pts_[el.index]);
    else T_.common_scalar(scs_[el.index]);
    return true;
  }
  bool squeeze(Fr* out) override { return *out = T_.squeeze_challenge(), true; }

 private:
  zkhost::Blake2bWrite tb_;
  zkhost::Keccak256Write tk_;
  zkhost::TranscriptWrite& T_;
  const G1Affine* pts_;
  const Fr* scs_;
};

// The caller's TranscriptRead (include/amdzk.h, amdzk_transcript_read): elements are READ from it, 64 bytes of Montgomery words
// per point and 32 per scalar, to raw + raw_offset[e] — unchecked: the decode launch checks them (verify.hip, the third
// element form). reads: read_* calls completed, which is AMDZK_PROOF_BAD_TRANSCRIPT's offset.
class CallbackSource : public Source {
 public:
  CallbackSource(const amdzk_transcript_read* t, uint8_t* raw, const uint32_t* raw_offset) : t_(t), raw_(raw), off_(raw_offset) {}
  bool usable() const { return t_ && t_->common_point && t_->common_scalar && t_->read_point && t_->read_scalar && t_->squeeze_challenge; }
  bool common_scalar(const Fr& s) override { return t_->common_scalar(t_->user, (const uint64_t*)s.l) == 0; }
  bool element(size_t e, const Plan::Elem& el) override {
    uint64_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if ((el.is_point ? t_->read_point(t_->user, w) : t_->read_scalar(t_->user, w)) != 0) return false;
    memcpy(raw_ + off_[e], w, el.is_point ? 64 : 32);
    reads++;
    return true;
  }
  bool squeeze(Fr* out) override {
    uint64_t w[4] = {0, 0, 0, 0};
    if (t_->squeeze_challenge(t_->user, w) != 0 || !fr_canonical_words(w)) return false;
    memcpy(out->l, w, 32);
    return true;
  }
  uint32_t reads = 0;

 private:
  const amdzk_transcript_read* t_;
  uint8_t* raw_;
  const uint32_t* off_;
};

// Byte offsets of a proof's elements in the callback form: 64 bytes per point, 32 per scalar, in read order.
inline size_t raw_offsets(const Plan& p, std::vector<uint32_t>* off) {
  size_t at = 0;
  off->clear();
  for (const Plan::Elem& el : p.elems) off->push_back((uint32_t)at), at += el.is_point ? 64 : 32;
  return at;
}

// Everything a proof's transcript decides.
struct Challenges {
  std::vector<Fr> chal;  // the circuit's own, by challenge index
  Fr theta, beta, gamma, y, x;
  Fr v, u, yy;  // the opening argument's (yy: SHPLONK only)
};

// AMDZK_PROOF_BAD_INSTANCE: a value >= r, or a column longer than the usable rows. cols / lens: N x num_instance.
inline bool instances_ok(const Plan& p, const uint64_t* const* const* inst, const size_t* const* lens, uint32_t* bad_col) {
  const uint64_t usable = p.n - (p.bf + 1);
  for (uint32_t c = 0; c < p.N; c++)
    for (uint32_t i = 0; i < p.I; i++) {
      const size_t len = lens[c][i];
      bool ok = len <= usable && (len == 0 || inst[c][i] != nullptr);
      for (size_t j = 0; ok && j < len; j++) ok = fr_canonical_words(inst[c][i] + 4 * j);
      if (!ok) {
        if (bad_col) *bad_col = i;
        return false;
      }
    }
  return true;
}

// One proof's transcript from its first byte to its last, element after element in read order, challenges where the prover
// squeezed them. inst / lens: the N circuit instances' public inputs (instances_ok). false: the source failed (never the
// built-in one) or x is degenerate — x = 0, where the rotations of x coincide and the prover refuses too, or x^n = 1, where
// the vanishing identity divides by x^n - 1 and upstream's verifier panics (a hash gives either with probability 2^-254 and
// n 2^-254) — and the walk ends right behind x's squeeze; *out is then unusable.
inline bool run_transcript(const Plan& p, Source& T, const Fr& transcript_repr, const uint64_t* const* const* inst, const size_t* const* lens,
                           Challenges* out) {
  const pkblob::Desc& d = *p.d;
  const uint32_t N = p.N;
  if (!T.common_scalar(transcript_repr)) return false;
  for (uint32_t c = 0; c < N; c++)
    for (uint32_t i = 0; i < p.I; i++)
      for (size_t j = 0; j < lens[c][i]; j++) {
        Fr v;
        memcpy(v.l, inst[c][i] + 4 * j, 32);
        if (!T.common_scalar(v)) return false;
      }
  size_t e = 0;
  auto take = [&](size_t count) {
    for (size_t i = 0; i < count; i++, e++)
      if (!T.element(e, p.elems[e])) return false;
    return true;
  };
  out->chal.assign(d.num_challenges, Fr::zero());
  for (uint32_t ph = 0; ph < p.nphases; ph++) {
    size_t cnt = 0;
    for (uint8_t a : p.adv_phase) cnt += a == ph;
    if (!take(cnt * N)) return false;
    for (uint32_t i = 0; i < d.num_challenges; i++)
      if (d.challenge_phase[i] == ph && !T.squeeze(&out->chal[i])) return false;
  }
  if (!T.squeeze(&out->theta) || !take(2 * (size_t)N * p.L) || !T.squeeze(&out->beta) || !T.squeeze(&out->gamma)) return false;
  out->yy = out->v = out->u = Fr::zero();
  if (!take((size_t)N * p.nsets + (size_t)N * p.L + 1) || !T.squeeze(&out->y) || !take(p.qdeg) || !T.squeeze(&out->x)) return false;
  if (out->x.is_zero() || fr_pow2k(out->x, p.k) == Fr::one()) return false;
  if (!take(p.NS)) return false;
  if (p.gwc) return T.squeeze(&out->v) && take(p.rots.size()) && T.squeeze(&out->u);
  return T.squeeze(&out->yy) && T.squeeze(&out->v) && take(1) && T.squeeze(&out->u) && take(1);
}

// One proof behind its transcript. pts: NP affine points, scs: NS scalars (Montgomery), both in read order and well formed;
// ch: what run_transcript gave for them. Lout / Rout: n_bases scalars each, overwritten.
inline void fold_challenges(const Plan& p, const Fr& omega, const uint64_t* const* const* inst, const size_t* const* lens, const Fr* scs,
                            const Fr& rho, const Challenges& ch, Fr* Lout, Fr* Rout) {
  using namespace bn254;
  const pkblob::Desc& d = *p.d;
  const uint32_t N = p.N;
  const std::vector<Fr>& chal = ch.chal;
  const Fr theta = ch.theta, beta = ch.beta, gamma = ch.gamma, y = ch.y, x = ch.x;
  // ---- the vanishing identity at x
  const Fr one = Fr::one(), omega_inv = inv(omega);
  const Fr xn = fr_pow2k(x, p.k);
  const Fr xn1 = sub(xn, one);
  const Fr xn1_over_n = mul(xn1, inv(fr_small(p.n)));
  auto lagrange_at = [&](const Fr& pt, int64_t row) {  // l_row(pt) = w^row (pt^n - 1) / (n (pt - w^row)); pt^n = x^n for a rotation of x
    const Fr wi = fr_pow_signed(omega, omega_inv, row);
    return mul(mul(wi, xn1_over_n), inv(sub(pt, wi)));
  };
  const Fr l0 = lagrange_at(x, 0), l_last = lagrange_at(x, -(int64_t)(p.bf + 1));
  Fr l_blind = Fr::zero();
  for (uint32_t i = 1; i <= p.bf; i++) l_blind = add(l_blind, lagrange_at(x, -(int64_t)i));
  const Fr l_active = sub(one, add(l_last, l_blind));
  const Fr delta = zkhost::fr_delta();
  const size_t nq_inst = d.instance_queries.size() / 2;
  Fr acc = Fr::zero();
  std::vector<Fr> stack, inst_e(nq_inst);
  for (uint32_t c = 0; c < N; c++) {
    for (size_t q = 0; q < nq_inst; q++) {  // instance columns at x from the public inputs
      const uint32_t col = (uint32_t)d.instance_queries[2 * q];
      const Fr pt = mul(x, fr_pow_signed(omega, omega_inv, d.instance_queries[2 * q + 1]));
      Fr s = Fr::zero(), wj = one;
      for (size_t j = 0; j < lens[c][col]; j++) {
        Fr v;
        memcpy(v.l, inst[c][col] + 4 * j, 32);
        s = add(s, mul(mul(v, wj), inv(sub(pt, wj))));
        wj = mul(wj, omega);
      }
      inst_e[q] = mul(s, xn1_over_n);
    }
    const Fr* adv_e = scs + p.adv_sc[c];
    const Fr* fix_e = scs + p.fix_sc;
    auto cell = [&](uint32_t kind, int col, int rot) -> Fr {  // kind: 0 advice, 1 fixed, 2 instance
      const std::pair<int, int> key{col, rot};
      if (kind == 0) return adv_e[p.advice_q.find(key)->second];
      if (kind == 1) return fix_e[p.fixed_q.find(key)->second];
      return inst_e[p.instance_q.find(key)->second];
    };
    auto expr = [&](uint32_t ei) -> Fr {  // the postfix words of expression ei at x
      stack.clear();
      for (uint32_t i = d.expr_offsets[ei]; i < d.expr_offsets[ei + 1]; i++) {
        const uint32_t w = d.expr_words[i], op = w >> 24, pl = w & 0xffffffu;
        Fr cst;
        switch (op) {
          case 1: memcpy(cst.l, d.constants.data() + 4 * (size_t)pl, 32), stack.push_back(cst); break;
          case 2: stack.push_back(cell(1, (int)(pl >> 8), (int)(pl & 0xff) - 128)); break;
          case 3: stack.push_back(cell(0, (int)(pl >> 8), (int)(pl & 0xff) - 128)); break;
          case 4: stack.push_back(cell(2, (int)(pl >> 8), (int)(pl & 0xff) - 128)); break;
          case 5: stack.back() = neg(stack.back()); break;
          case 6: cst = stack.back(), stack.pop_back(), stack.back() = add(stack.back(), cst); break;
          case 7: cst = stack.back(), stack.pop_back(), stack.back() = mul(stack.back(), cst); break;
          case 8: memcpy(cst.l, d.constants.data() + 4 * (size_t)pl, 32), stack.back() = mul(stack.back(), cst); break;
          default: stack.push_back(chal[pl]); break;  // 9 CHALLENGE (validate admits nothing else)
        }
      }
      return stack.back();
    };
    auto term = [&](const Fr& v) { acc = add(mul(acc, y), v); };
    for (uint32_t g = 0; g < d.num_gates; g++) term(expr(g));
    if (p.nsets) {
      auto Z = [&](uint32_t s, int which) { return scs[p.z_sc[(size_t)c * p.nsets + s] + which]; };  // 0: x, 1: wx, 2: w^last x
      term(mul(sub(one, Z(0, 0)), l0));
      const Fr zl = Z(p.nsets - 1, 0);
      term(mul(sub(sqr(zl), zl), l_last));
      for (uint32_t s = 1; s < p.nsets; s++) term(mul(sub(Z(s, 0), Z(s - 1, 2)), l0));
      Fr cur = mul(beta, x);
      for (uint32_t s = 0; s < p.nsets; s++) {
        const uint32_t c0 = s * p.chunk, c1 = c0 + p.chunk < p.S ? c0 + p.chunk : p.S;
        Fr left = Z(s, 1), right = Z(s, 0);
        for (uint32_t j = c0; j < c1; j++) {
          const Fr v = cell(d.perm_columns[2 * j], (int)d.perm_columns[2 * j + 1], 0);
          left = mul(left, add(add(v, mul(beta, scs[p.sig_sc + j])), gamma));
          right = mul(right, add(add(v, cur), gamma));
          cur = mul(cur, delta);
        }
        term(mul(sub(left, right), l_active));
      }
    }
    uint32_t ei = d.num_gates;
    for (uint32_t l = 0; l < p.L; l++) {
      Fr ci = Fr::zero(), ct = Fr::zero();
      for (uint32_t i = 0; i < d.lookup_shape[2 * l]; i++) ci = add(mul(ci, theta), expr(ei++));
      for (uint32_t i = 0; i < d.lookup_shape[2 * l + 1]; i++) ct = add(mul(ct, theta), expr(ei++));
      const Fr* le = scs + p.lk_sc[(size_t)c * p.L + l];
      const Fr z = le[0], znext = le[1], a = le[2], aprev = le[3], s = le[4];
      term(mul(sub(one, z), l0));
      term(mul(sub(sqr(z), z), l_last));
      term(mul(sub(mul(mul(znext, add(a, beta)), add(s, gamma)), mul(z, mul(add(ci, beta), add(ct, gamma)))), l_active));
      term(mul(sub(a, s), l0));
      term(mul(mul(sub(a, s), sub(a, aprev)), l_active));
    }
  }
  const Fr expected_h = mul(acc, inv(xn1));
  // ---- the opening argument's scalars
  for (uint32_t i = 0; i < p.n_bases; i++) Lout[i] = Rout[i] = Fr::zero();
  auto add_key = [&](uint32_t key, const Fr& s) {  // R += s * commitment(key)
    if (key != p.key_h) {
      Rout[key] = add(Rout[key], s);
      return;
    }
    Fr t = s;  // h = sum_i x^(n i) h_i
    for (uint32_t i = 0; i < p.qdeg; i++) {
      Rout[p.h_pt + i] = add(Rout[p.h_pt + i], t);
      t = mul(t, xn);
    }
  };
  auto eval_of = [&](const Plan::Query& q) { return q.sc == NO_SCALAR ? expected_h : scs[q.sc]; };
  std::vector<Fr> pt(p.rots.size());
  for (size_t i = 0; i < pt.size(); i++) pt[i] = mul(x, fr_pow_signed(omega, omega_inv, p.rots[i]));
  const Fr v = ch.v, u = ch.u;
  if (p.gwc) {
    Fr up = rho;
    for (size_t i = 0; i < p.rots.size(); i++) {
      const uint32_t W = p.open_pt + (uint32_t)i;
      Lout[W] = add(Lout[W], up);
      Rout[W] = add(Rout[W], mul(up, pt[i]));
      Fr vp = up, eb = Fr::zero();
      for (uint32_t qi : p.grp.gw[i]) {
        add_key(p.queries[qi].key, vp);
        eb = add(eb, mul(vp, eval_of(p.queries[qi])));
        vp = mul(vp, v);
      }
      Rout[p.base_g] = sub(Rout[p.base_g], eb);
      up = mul(up, u);
    }
    return;
  }
  const Fr yy = ch.yy;
  const opening::Grouping& g = p.grp;
  const opening::Shplonk sh = opening::shplonk_sets(g, pt.data(), [&](uint32_t qi) { return eval_of(p.queries[qi]); }, yy, v);
  const opening::AtU at = opening::at_u(g, pt.data(), u);
  Fr vp = rho;
  for (size_t si = 0; si < g.sets.size(); si++) {
    const std::vector<Fr> wgt = opening::weights_at(sh, si, u);  // sum_j y^j r_ij(u) = sum_t wgt[t] E_i[t]
    Fr ru = Fr::zero(), coef = mul(vp, at.z[si]);
    for (size_t t = 0; t < wgt.size(); t++) ru = add(ru, mul(wgt[t], sh.E[si][t]));
    Rout[p.base_g] = sub(Rout[p.base_g], mul(coef, ru));
    for (uint32_t c : g.sets[si].coms) {
      add_key(g.coms[c], coef);
      coef = mul(coef, yy);
    }
    vp = mul(vp, v);
  }
  const Fr zt = at.zt, z0 = at.z0;
  const uint32_t h1 = p.open_pt, h2 = p.open_pt + 1;
  const Fr rz0 = mul(rho, z0);
  Rout[h1] = sub(Rout[h1], mul(rho, zt));
  Rout[h2] = add(Rout[h2], mul(rz0, u));
  Lout[h2] = add(Lout[h2], rz0);
}

// One proof read with the built-in transcript of the plan: run_transcript over the decoded elements, then fold_challenges.
inline void fold_proof(const Plan& p, const Fr& transcript_repr, const Fr& omega, const uint64_t* const* const* inst, const size_t* const* lens,
                       const G1Affine* pts, const Fr* scs, const Fr& rho, Fr* Lout, Fr* Rout) {
  BuiltinSource T(p.evm, pts, scs);
  Challenges ch;
  run_transcript(p, T, transcript_repr, inst, lens, &ch);
  fold_challenges(p, omega, inst, lens, scs, rho, ch, Lout, Rout);
}

// ---- a verify call (verify.hip, verify_core), possibly over DIFFERENT keys (amdzk_verify_proofs_mixed, whose name the types
// below carry). Items that name the same key handle, the same number of circuit instances and the same transcript kind form a
// GROUP: one Plan, one element table, one raw-form table and one block of commitments; a call over one key is one group and
// does not need group_items. Both functions below are pure: tests/native/verifier_mixed_check.cpp and workspace_check.cpp run
// them alone.
struct MixedKey {
  const void* key;  // the key handle the item names (a proving key's or a verifying key's)
  uint32_t n_circuits;
  int kind;  // the transcript kind that counts for the item (a read-transcript item: the opening scheme's bit alone)
  bool operator<(const MixedKey& o) const {
    return key != o.key ? key < o.key : n_circuits != o.n_circuits ? n_circuits < o.n_circuits : kind < o.kind;
  }
};
// item -> group, groups numbered first seen first; firsts[g]: the first item of group g
inline std::vector<uint32_t> group_items(const MixedKey* keys, size_t n_items, std::vector<size_t>* firsts) {
  std::map<MixedKey, uint32_t> seen;
  std::vector<uint32_t> of(n_items);
  firsts->clear();
  for (size_t b = 0; b < n_items; b++) {
    auto it = seen.find(keys[b]);
    if (it == seen.end()) {
      it = seen.emplace(keys[b], (uint32_t)firsts->size()).first;
      firsts->push_back(b);
    }
    of[b] = it->second;
  }
  return of;
}

// What the decode launch reads (verify.hip, proof_decode_kernel). A block of MIXED_BLOCK threads decodes
// elements [first, first + MIXED_BLOCK) of ONE item: no block straddles two items, so its records are wave-uniform.
constexpr uint32_t MIXED_BLOCK = 64;
struct MixedItemRec {
  uint64_t staging;          // byte offset of the item's bytes (or read-transcript words) in the staging area, a multiple of 32
  uint64_t points, scalars;  // its first decoded point / scalar
  uint32_t group;
  uint32_t raw;  // 1: the read-transcript form
};
struct MixedGroupRec {
  uint32_t elems;  // the group's first entry in the element table and in the raw-form table
  uint32_t E;
  uint32_t evm;
  uint32_t reserved;
};
struct MixedBlockRec {
  uint32_t item, first;
};
static_assert(sizeof(MixedItemRec) == 32 && sizeof(MixedGroupRec) == 16 && sizeof(MixedBlockRec) == 8, "device records");

struct MixedGroupShape {
  size_t E, NP, NS, nvk;         // elements, points, scalars of one proof; fixed + permutation commitments of the key
  size_t proof_bytes, raw_bytes;  // one proof in the byte form and in the read-transcript form
};
// The ONE device reservation of a verify call (ZK_WS_STARTUP) and its mirror in pinned memory. [0, g) goes UP in one copy (the
// G of a proving key then follows device to device into key_g, and key 0's from there into g); the decoder fills points and
// scalars; [status, msm) comes DOWN in one copy: the status words, one G per distinct key — the "same G" rule is judged on
// what came down —, the commitments, the points and the scalars.
struct MixedLayout {
  size_t staging;    // the items' bytes, item b at item_staging[b], item_stride[b] bytes
  size_t items;      // MixedItemRec[n_items]
  size_t groups;     // MixedGroupRec[n_groups]
  size_t blocks;     // MixedBlockRec[n_blocks]
  size_t elems;      // uint2[n_elems]: every group's element table, group g at group_elems[g]
  size_t elems_raw;  // the same in the read-transcript form (no bytes when no item has one)
  size_t status;     // uint32_t[n_items]
  size_t key_g;      // G1Affine[n_keys]: G of every distinct key, first seen first
  // commitments | G | points are CONTIGUOUS: the base array of the combined MSM
  size_t vk;         // G1Affine[nvk]: every group's fixed and permutation commitments, group g at group_vk[g]
  size_t g;          // G1Affine: the G of item 0's key
  size_t points;     // G1Affine[n_points], item b at item_points[b]
  size_t scalars;    // Fr[n_scalars], item b at item_scalars[b]
  size_t msm;        // Fr[2][nvk + 1 + n_points] combined; per proof Fr[2 * run][run_len], ONE run's columns
  size_t run_bases;  // per proof: G1Affine[run_len], one run's commitments | G | points
  size_t bytes, up_bytes, down_bytes;
  size_t n_blocks, n_elems, n_points, n_scalars, nvk, staging_bytes;
  size_t run, run_len;  // per proof: items per MSM, and the most bases one run has
  std::vector<size_t> item_staging, item_stride, item_points, item_scalars;
  std::vector<size_t> group_elems, group_vk;
};
// item_group[b] < n_groups; item_raw[b] != 0: item b comes through a read transcript (item_raw == nullptr: none does).
inline MixedLayout mixed_layout(const MixedGroupShape* shapes, size_t n_groups, const uint32_t* item_group, const uint8_t* item_raw, size_t n_items,
                                size_t n_keys, bool per_proof) {
  MixedLayout L;
  L.group_elems.resize(n_groups), L.group_vk.resize(n_groups);
  L.n_elems = L.nvk = 0;
  for (size_t g = 0; g < n_groups; g++) {
    L.group_elems[g] = L.n_elems, L.n_elems += shapes[g].E;
    L.group_vk[g] = L.nvk, L.nvk += shapes[g].nvk;
  }
  L.item_staging.resize(n_items), L.item_stride.resize(n_items), L.item_points.resize(n_items), L.item_scalars.resize(n_items);
  L.n_blocks = L.n_points = L.n_scalars = L.staging_bytes = 0;
  bool any_raw = false;
  for (size_t b = 0; b < n_items; b++) {
    const MixedGroupShape& s = shapes[item_group[b]];
    const bool raw = item_raw && item_raw[b];
    any_raw |= raw;
    L.item_staging[b] = L.staging_bytes, L.item_stride[b] = ws_round_up(raw ? s.raw_bytes : s.proof_bytes, 32);
    L.staging_bytes += L.item_stride[b];
    L.item_points[b] = L.n_points, L.n_points += s.NP;
    L.item_scalars[b] = L.n_scalars, L.n_scalars += s.NS;
    L.n_blocks += (s.E + MIXED_BLOCK - 1) / MIXED_BLOCK;
  }
  // runs of AMDZK_DECIDE_RUN consecutive positions: the commitments of the groups present, G, the run's points
  L.run = n_items < AMDZK_DECIDE_RUN ? n_items : AMDZK_DECIDE_RUN, L.run_len = 0;
  std::vector<uint8_t> present(n_groups, 0);
  for (size_t b0 = 0; per_proof && b0 < n_items; b0 += L.run) {
    const size_t b1 = b0 + L.run < n_items ? b0 + L.run : n_items;
    size_t len = 1;
    for (size_t b = b0; b < b1; b++) {
      const uint32_t g = item_group[b];
      len += shapes[g].NP + (present[g] ? 0 : shapes[g].nvk);
      present[g] = 1;
    }
    for (size_t b = b0; b < b1; b++) present[item_group[b]] = 0;
    L.run_len = len > L.run_len ? len : L.run_len;
  }
  WsLayout w;
  L.staging = w.take(L.staging_bytes), L.items = w.take(n_items * sizeof(MixedItemRec)), L.groups = w.take(n_groups * sizeof(MixedGroupRec));
  L.blocks = w.take(L.n_blocks * sizeof(MixedBlockRec)), L.elems = w.take(L.n_elems * 8), L.elems_raw = w.take(any_raw ? L.n_elems * 8 : 0);
  L.status = w.take(n_items * 4), L.key_g = w.take(n_keys * sizeof(G1Affine));
  L.vk = w.take(L.nvk * sizeof(G1Affine), 1), L.g = w.take(sizeof(G1Affine), 1), L.points = w.take(L.n_points * sizeof(G1Affine), 1);
  L.scalars = w.take(L.n_scalars * sizeof(Fr));
  L.msm = per_proof ? w.take(2 * L.run * L.run_len * sizeof(Fr)) : w.take(2 * (L.nvk + 1 + L.n_points) * sizeof(Fr), 1);
  L.run_bases = w.take(per_proof ? L.run_len * sizeof(G1Affine) : 0, 1);
  L.bytes = w.bytes(), L.up_bytes = L.g, L.down_bytes = L.msm - L.status;
  return L;
}

}  // namespace verifier
