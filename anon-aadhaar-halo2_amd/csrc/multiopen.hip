// poly::kzg::multiopen::{ProverSHPLONK, ProverGWC}::create_proof [UP] over the CALLER's
// polynomials, points and transcript: amdzk_multiopen_dev / amdzk_multiopen_plan (include/amdzk.h).
//
// The grouping and the scalars are opening.hpp's, shared with the proof path (prover.hip Prover::{gwc, shplonk,
// shplonk_final}) and the verifier; the kernels are the proof path's too — zk_poly_eval, zk_lincomb, zk_kate_div_from, the
// MSM over AMDZK_BASIS_G. The driver is this file's own: points are arbitrary field elements
// instead of rotations of x, polynomials are the caller's buffers instead of a key's workspace, scratch is the ctx's
// (ZK_WS_TABLES, one reservation per call whose size the plan reports) instead of a key's, and nothing is capped at 16
// sets or points or at a key's pointer table: launches whose grid.y would pass 65535 are cut into runs by the host.
// Everything runs on the caller's stream. No kernel lives here.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "hostcrypto.hpp"
#include "opening.hpp"
#include "plonk_kernels.hpp"

using namespace bn254;

namespace {

constexpr size_t MO_MAX_GRID_Y = 65535;  // polynomials per division launch, columns per commitment batch

// a call's one reservation; a size that cannot be had is the call's own refusal
int mo_reserve(amdzk_ctx* ctx, const char* who, size_t bytes, char** ws) {
  const int r = zk_ws_reserve(ctx, ZK_WS_TABLES, bytes, (void**)ws);
  if (r != AMDZK_E_NOMEM) return r;
  (void)hipGetLastError();  // the failed allocation's sticky status
  ZK_FAIL(ctx, AMDZK_E_NOMEM, "%s: %zu bytes of scratch cannot be allocated", who, bytes);
}

Fr canon_of(const uint64_t* mont) {
  Fr a;
  memcpy(a.l, mont, 32);
  return from_mont(a);
}
bool fr_words_canonical(const uint64_t* w) {
  Fr a;
  memcpy(a.l, w, 32);
  return reduce_once(a) == a;
}
struct CanonLess {
  bool operator()(const Fr& a, const Fr& b) const { return opening::canon_less(a, b); }
};

// What both schemes are built from: the distinct point VALUES the queries name (ids in first-seen query order, which is
// GWC's output order; rank = position in ascending canonical order, which is the order of upstream's BTreeSets), the
// distinct queried polynomials ("commitments", first seen first) and the distinct (polynomial, point) pairs, whose
// evaluations the call needs once each.
struct MoSets {
  size_t n = 0;
  bool gwc = false;
  std::vector<uint32_t> dp_index;  // distinct point -> one point index that carries its value
  std::vector<uint32_t> dp_rank, rank_dp;
  std::vector<uint32_t> q_dp;    // query -> distinct point
  std::vector<uint32_t> q_pair;  // query -> (polynomial, point) pair
  std::vector<std::pair<uint32_t, uint32_t>> pairs;  // pair -> (polynomial index, distinct point)
  std::vector<uint32_t> pair_query;                  // pair -> its first query
  opening::Grouping g;  // over (polynomial index, rank): SHPLONK's sets, GWC's queries per point
  uint32_t n_sets = 0, n_out = 0;
  // the call's one reservation: polynomials first, then the pointer tables, then the field-element tables
  size_t poly_count = 0, ptr_count = 0, fr_count = 0, ptr_bytes = 0, scratch_bytes = 0;
};

bool mul_ok(size_t a, size_t b, size_t* out) { return !__builtin_mul_overflow(a, b, out); }
bool add_ok(size_t a, size_t b, size_t* out) { return !__builtin_add_overflow(a, b, out); }

// The sets and sizes of one call. why: the refusal's text behind "multiopen: ".
int mo_build(const uint64_t* points, size_t n_points, const amdzk_open_query* queries, size_t n_queries, size_t n_polys, uint32_t k, int scheme,
             MoSets& s, uint32_t* set_of_poly, char why[200]) {
  why[0] = 0;
  if (!points || !queries) return snprintf(why, 200, "null argument"), AMDZK_E_INVALID;
  if (scheme != 0 && scheme != AMDZK_MULTIOPEN_GWC) return snprintf(why, 200, "unknown scheme %d", scheme), AMDZK_E_INVALID;
  if (n_queries == 0) return snprintf(why, 200, "no queries"), AMDZK_E_INVALID;
  if (k > 30) return snprintf(why, 200, "k = %u out of range", k), AMDZK_E_INVALID;
  if (n_queries >= UINT32_MAX || n_polys >= UINT32_MAX || n_points >= UINT32_MAX)
    return snprintf(why, 200, "more than 2^32 - 2 queries, polynomials or points"), AMDZK_E_INVALID;
  for (size_t i = 0; i < n_queries; i++)
    if (queries[i].poly >= n_polys || queries[i].point >= n_points)
      return snprintf(why, 200, "query %zu names polynomial %u of %zu, point %u of %zu", i, queries[i].poly, n_polys, queries[i].point, n_points),
             AMDZK_E_INVALID;
  s.n = (size_t)1 << k;
  s.gwc = scheme == AMDZK_MULTIOPEN_GWC;
  // distinct point values among the queried indices
  std::vector<uint32_t> dp_of_index(n_points, UINT32_MAX);
  std::map<Fr, uint32_t, CanonLess> dp_of_value;
  s.q_dp.resize(n_queries);
  for (size_t i = 0; i < n_queries; i++) {
    const uint32_t pi = queries[i].point;
    if (dp_of_index[pi] == UINT32_MAX) {
      const Fr c = canon_of(points + 4 * (size_t)pi);
      auto it = dp_of_value.find(c);
      if (it == dp_of_value.end()) {
        it = dp_of_value.emplace(c, (uint32_t)s.dp_index.size()).first;
        s.dp_index.push_back(pi);
      }
      dp_of_index[pi] = it->second;
    }
    s.q_dp[i] = dp_of_index[pi];
  }
  const size_t ndp = s.dp_index.size();
  s.dp_rank.resize(ndp);
  s.rank_dp.resize(ndp);
  {
    uint32_t r = 0;
    for (auto& e : dp_of_value) s.rank_dp[r] = e.second, s.dp_rank[e.second] = r++;  // the map iterates in ascending canonical order
  }
  // distinct (polynomial, point) pairs
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> pair_of;
  s.q_pair.resize(n_queries);
  for (size_t i = 0; i < n_queries; i++) {
    const std::pair<uint32_t, uint32_t> key{queries[i].poly, s.q_dp[i]};
    auto it = pair_of.find(key);
    if (it == pair_of.end()) {
      it = pair_of.emplace(key, (uint32_t)s.pairs.size()).first;
      s.pairs.push_back(key);
      s.pair_query.push_back((uint32_t)i);
    }
    s.q_pair[i] = it->second;
  }
  const size_t E = s.pairs.size();
  std::vector<opening::Query> q(n_queries);
  for (size_t i = 0; i < n_queries; i++) q[i] = {queries[i].poly, s.dp_rank[s.q_dp[i]]};
  s.g = opening::group(q.data(), n_queries, n_polys, ndp);
  if (set_of_poly)
    for (size_t i = 0; i < n_polys; i++) set_of_poly[i] = UINT32_MAX;
  size_t ptrs = 0, frs = 0, polys = 0;
  bool ok = true;
  if (s.gwc) {
    if (set_of_poly)
      for (size_t i = 0; i < n_queries; i++) set_of_poly[queries[i].poly] = std::min(set_of_poly[queries[i].poly], s.q_dp[i]);
    s.n_sets = s.n_out = (uint32_t)ndp;
    // pointers: the pairs to evaluate | every query's polynomial | the W_z;  elements: points and results of the
    // evaluations | v^j per query | sum_j v^j eval per point | the points
    polys = ndp;
    ptrs = E + n_queries + ndp;
    frs = 2 * E + n_queries + 2 * ndp;
  } else {
    if (set_of_poly)
      for (size_t i = 0; i < s.g.sets.size(); i++)
        for (uint32_t c : s.g.sets[i].coms) set_of_poly[s.g.coms[c]] = (uint32_t)i;
    s.n_sets = (uint32_t)s.g.sets.size();
    s.n_out = 2;
    const size_t S = s.g.sets.size(), C = s.g.coms.size(), P = s.g.set_points;
    // pointers: the pairs to evaluate | the polynomials set after set | destinations and sources of the P divisions |
    // the L_i and h(X) | l(X);  elements: points and results of the evaluations | y^j per commitment | the roots, the
    // R_i (maxm coefficients each) and the v^i c_it of the P divisions | the S + 1 final coefficients, the constant term, u
    size_t low = 0;
    ok = mul_ok(P, s.g.maxm, &low);
    polys = S + P + 1;
    ptrs = E + C + 2 * P + S + 2;
    ok = ok && add_ok(2 * E + C + 2 * P + S + 3, low, &frs);
  }
  size_t poly_bytes = 0, fr_bytes = 0;
  ok = ok && mul_ok(polys, s.n * 32, &poly_bytes) && mul_ok(frs, 32, &fr_bytes);
  s.poly_count = polys;
  s.ptr_count = ptrs;
  s.fr_count = frs;
  s.ptr_bytes = ws_round_up(ptrs * sizeof(void*), 256);
  ok = ok && add_ok(poly_bytes, s.ptr_bytes, &s.scratch_bytes) && add_ok(s.scratch_bytes, fr_bytes, &s.scratch_bytes);
  if (!ok) return snprintf(why, 200, "the scratch size of this shape does not fit 64 bits"), AMDZK_E_NOMEM;
  return AMDZK_OK;
}

// The call's tables on the device: pointers and field elements are appended to a host image in the order the launches
// use them and uploaded run by run; the image lives as long as the call, so no copy outlives its source.
struct MoTables {
  void** d_ptrs = nullptr;
  Fr* d_frs = nullptr;
  std::vector<const void*> ptrs;
  std::vector<Fr> frs;
  size_t ptrs_up = 0, frs_up = 0;  // what has been uploaded
  size_t ptr_cap = 0, fr_cap = 0;
  size_t put(const void* p) { return ptrs.push_back(p), ptrs.size() - 1; }
  size_t put(const Fr& f) { return frs.push_back(f), frs.size() - 1; }
  size_t skip_frs(size_t cnt) {  // room the device fills
    const size_t at = frs.size();
    frs.resize(at + cnt, Fr::zero());
    return at;
  }
  int upload(amdzk_ctx* ctx) {
    if (ptrs.size() > ptr_cap || frs.size() > fr_cap) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen: internal error: the tables outgrew the plan");
    if (ptrs.size() > ptrs_up)
      ZK_HIP(ctx, hipMemcpyAsync(d_ptrs + ptrs_up, ptrs.data() + ptrs_up, (ptrs.size() - ptrs_up) * sizeof(void*), hipMemcpyHostToDevice, ctx->stream));
    if (frs.size() > frs_up)
      ZK_HIP(ctx, hipMemcpyAsync(d_frs + frs_up, frs.data() + frs_up, (frs.size() - frs_up) * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    ptrs_up = ptrs.size();
    frs_up = frs.size();
    return AMDZK_OK;
  }
};

struct Call {
  amdzk_ctx* ctx;
  const amdzk_srs* srs;
  const void* const* d_polys;
  const uint64_t* points;
  const MoSets& s;
  zkhost::CallbackWrite T;
  MoTables tab;
  Fr* d_poly = nullptr;        // poly_count x n
  std::vector<Fr> pair_eval;   // per (polynomial, point) pair
  std::vector<Fr> query_eval;  // per query (GWC)
  std::vector<G1Affine> written;
  const size_t n;

  Call(amdzk_ctx* ctx, const amdzk_srs* srs, const void* const* d_polys, const uint64_t* points, const MoSets& s, const amdzk_transcript& t)
      : ctx(ctx), srs(srs), d_polys(d_polys), points(points), s(s), T(t), n(s.n) {
    // the reservations are exact: a vector that grew would move under a copy in flight
    tab.ptrs.reserve(s.ptr_count);
    tab.frs.reserve(s.fr_count);
    tab.ptr_cap = s.ptr_count;
    tab.fr_cap = s.fr_count;
  }
  Fr point(uint32_t dp) const {
    Fr z;
    memcpy(z.l, points + 4 * (size_t)s.dp_index[dp], 32);
    return z;
  }
  int t_ok() {
    if (T.failed) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen: the caller's transcript reported an error");
    if (T.noncanonical) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen: a squeezed challenge is not below the modulus");
    return AMDZK_OK;
  }
  int challenge(Fr* c) {
    *c = T.squeeze_challenge();
    return t_ok();
  }
  // commit ncols consecutive polynomials over AMDZK_BASIS_G and write them in order
  int commit_write(const Fr* d_cols, size_t ncols, const char* label) {
    for (size_t first = 0; first < ncols; first += MO_MAX_GRID_Y) {
      const size_t cnt = std::min(MO_MAX_GRID_Y, ncols - first);
      G1X* d_res = nullptr;
      ZK_TRY(zk_msm_dev_xyzz(ctx, srs, AMDZK_BASIS_G, d_cols + first * n, cnt, n, n, &d_res));
      std::vector<uint64_t> jac(12 * cnt);
      ZK_TRY(zk_msm_finish(ctx, d_res, cnt, jac.data()));
      for (size_t i = 0; i < cnt; i++) {
        const G1Jac* j = reinterpret_cast<const G1Jac*>(&jac[12 * i]);
        G1Affine p;
        p.x = j->z.is_zero() ? Fq::zero() : j->x;
        p.y = j->z.is_zero() ? Fq::zero() : j->y;
        if (!T.write_point(p))
          ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen: %s commitment %zu is the identity (cannot write points at infinity to the transcript)", label,
                  first + i);
        ZK_TRY(t_ok());
        written.push_back(p);
      }
    }
    return AMDZK_OK;
  }
  // (d_dst[i] = (d_src[i] - low_i) / (X - root_i)) for cnt polynomials, in runs the grid takes
  int divide(size_t dst_at, bool with_src, size_t src_at, size_t root_at, size_t low_at, uint32_t low_stride, size_t cnt) {
    for (size_t first = 0; first < cnt; first += MO_MAX_GRID_Y) {
      const size_t run = std::min(MO_MAX_GRID_Y, cnt - first);
      ZK_TRY(zk_kate_div_from(ctx, (Fr* const*)(tab.d_ptrs + dst_at + first), with_src ? (const Fr* const*)(tab.d_ptrs + src_at + first) : nullptr,
                              tab.d_frs + root_at + first, tab.d_frs + low_at + first * low_stride, low_stride, run, (uint32_t)n));
    }
    return AMDZK_OK;
  }

  // the evaluations of every (polynomial, point) pair: zk_poly_eval, or the caller's (the pair's first query; GWC: every
  // query its own)
  int evaluations(const amdzk_open_query* queries, size_t n_queries, const uint64_t* evals) {
    const size_t E = s.pairs.size();
    pair_eval.resize(E);
    if (evals) {
      for (size_t e = 0; e < E; e++) memcpy(pair_eval[e].l, evals + 4 * (size_t)s.pair_query[e], 32);
    } else {
      const size_t p_at = tab.ptrs.size();
      for (size_t e = 0; e < E; e++) tab.put(d_polys[s.pairs[e].first]);
      const size_t z_at = tab.frs.size();
      for (size_t e = 0; e < E; e++) tab.put(point(s.pairs[e].second));
      const size_t o_at = tab.skip_frs(E);
      ZK_TRY(tab.upload(ctx));
      ZK_TRY(zk_poly_eval(ctx, (const Fr* const*)(tab.d_ptrs + p_at), tab.d_frs + z_at, tab.d_frs + o_at, E, (uint32_t)n));
      ZK_HIP(ctx, hipMemcpyAsync(pair_eval.data(), tab.d_frs + o_at, E * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
      ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
    }
    if (s.gwc) {
      query_eval.resize(n_queries);
      for (size_t i = 0; i < n_queries; i++) {
        if (evals) memcpy(query_eval[i].l, evals + 4 * i, 32);
        else query_eval[i] = pair_eval[s.q_pair[i]];
      }
    }
    return AMDZK_OK;
  }

  // multiopen/gwc/prover.rs [UP]: per point z, W_z = (sum_j v^j p_j - sum_j v^j p_j(z)) / (X - z). One linear combination
  // per point; the subtraction of the constant rides in on the division's loads, and all divisions are one launch.
  int gwc(const amdzk_open_query* queries) {
    Fr v;
    ZK_TRY(challenge(&v));
    const size_t Z = s.dp_index.size();
    auto gw = [&](size_t z) -> const std::vector<uint32_t>& { return s.g.gw[s.dp_rank[z]]; };  // output order: first seen first
    std::vector<size_t> p_at(Z), c_at(Z);
    for (size_t z = 0; z < Z; z++) {
      p_at[z] = tab.ptrs.size();
      for (uint32_t q : gw(z)) tab.put(d_polys[queries[q].poly]);
    }
    std::vector<Fr> eb(Z, Fr::zero());
    for (size_t z = 0; z < Z; z++) {
      c_at[z] = tab.frs.size();
      Fr cur = Fr::one();
      for (uint32_t q : gw(z)) {
        tab.put(cur);
        eb[z] = add(eb[z], mul(cur, query_eval[q]));
        cur = mul(cur, v);
      }
    }
    const size_t w_at = tab.ptrs.size();
    for (size_t z = 0; z < Z; z++) tab.put(d_poly + z * n);
    const size_t eb_at = tab.frs.size();
    for (size_t z = 0; z < Z; z++) tab.put(eb[z]);
    const size_t root_at = tab.frs.size();
    for (size_t z = 0; z < Z; z++) tab.put(point((uint32_t)z));
    ZK_TRY(tab.upload(ctx));
    for (size_t z = 0; z < Z; z++)
      ZK_TRY(zk_lincomb(ctx, (const Fr* const*)(tab.d_ptrs + p_at[z]), tab.d_frs + c_at[z], (uint32_t)gw(z).size(), d_poly + z * n, n, false));
    ZK_TRY(divide(w_at, false, 0, root_at, eb_at, 1, Z));
    return commit_write(d_poly, Z, "gwc_w");
  }

  // multiopen/shplonk/prover.rs [UP] in opening.hpp's formulation: L_i = sum_j y^j P_ij, all (set, point) quotients
  // Q_it = (L_i - R_i) / (X - p_t) in one division, h(X) = sum_it v^i c_it Q_it.
  int shplonk() {
    Fr y, v;
    ZK_TRY(challenge(&y));
    ZK_TRY(challenge(&v));
    const opening::Grouping& g = s.g;
    const size_t S = g.sets.size(), P = g.set_points, maxm = g.maxm;
    Fr* const d_L = d_poly;
    Fr* const d_Q = d_poly + S * n;
    Fr* const d_hx = d_poly + (S + P) * n;
    std::vector<Fr> rank_pt(s.rank_dp.size());
    for (size_t r = 0; r < rank_pt.size(); r++) rank_pt[r] = point(s.rank_dp[r]);
    const opening::Shplonk sh = opening::shplonk_sets(g, rank_pt.data(), [&](uint32_t q) { return pair_eval[s.q_pair[q]]; }, y, v);
    // tables of the first half
    std::vector<size_t> p_at(S), c_at(S);
    for (size_t i = 0; i < S; i++) {
      p_at[i] = tab.ptrs.size();
      for (uint32_t c : g.sets[i].coms) tab.put(d_polys[g.coms[c]]);
    }
    for (size_t i = 0; i < S; i++) {
      c_at[i] = tab.frs.size();
      Fr cur = Fr::one();
      for (size_t j = 0; j < g.sets[i].coms.size(); j++) tab.put(cur), cur = mul(cur, y);
    }
    const size_t dst_at = tab.ptrs.size();
    for (size_t q = 0; q < P; q++) tab.put(d_Q + q * n);
    const size_t src_at = tab.ptrs.size();
    for (size_t q = 0; q < P; q++) tab.put(d_L + sh.row_set[q] * n);
    const size_t root_at = tab.frs.size();
    for (const Fr& f : sh.root) tab.put(f);
    const size_t low_at = tab.frs.size();
    for (const Fr& f : sh.row_low) tab.put(f);
    const size_t coef_at = tab.frs.size();
    for (const Fr& f : sh.coef) tab.put(f);
    ZK_TRY(tab.upload(ctx));
    for (size_t i = 0; i < S; i++)
      ZK_TRY(zk_lincomb(ctx, (const Fr* const*)(tab.d_ptrs + p_at[i]), tab.d_frs + c_at[i], (uint32_t)g.sets[i].coms.size(), d_L + i * n, n, false));
    ZK_TRY(divide(dst_at, true, src_at, root_at, low_at, (uint32_t)maxm, P));
    ZK_TRY(zk_lincomb(ctx, (const Fr* const*)(tab.d_ptrs + dst_at), tab.d_frs + coef_at, (uint32_t)P, d_hx, n, false));
    ZK_TRY(commit_write(d_hx, 1, "shplonk_h1"));

    // second half: l(X) = sum_i v^i z_i(u) (L_i - R_i(u)) - Z_T(u) h(X), then / (X - u), with 1 / z_0(u) folded into
    // the coefficients
    Fr u;
    ZK_TRY(challenge(&u));
    const opening::Final f = opening::shplonk_final(g, sh, rank_pt.data(), v, u);
    if (f.z0_zero) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "multiopen: the challenge u is one of the opening points (probability 2^-254)");
    Fr* const d_lx = d_Q;  // the quotients are folded into h(X): their first buffer is free
    const size_t fp_at = tab.ptrs.size();
    for (size_t i = 0; i < S; i++) tab.put(d_L + i * n);
    tab.put(d_hx);
    const size_t lx_at = tab.put(d_lx);
    const size_t fc_at = tab.frs.size();
    for (const Fr& c : f.cf) tab.put(c);
    const size_t ct_at = tab.put(f.cterm);
    const size_t u_at = tab.put(u);
    ZK_TRY(tab.upload(ctx));
    ZK_TRY(zk_lincomb(ctx, (const Fr* const*)(tab.d_ptrs + fp_at), tab.d_frs + fc_at, (uint32_t)(S + 1), d_lx, n, false));
    ZK_TRY(divide(lx_at, false, 0, u_at, ct_at, 1, 1));
    return commit_write(d_lx, 1, "shplonk_h2");
  }
};

int multiopen_body(amdzk_ctx* ctx, const amdzk_srs* srs, const void* const* d_polys, size_t n_polys, const uint64_t* points, size_t n_points,
                   const amdzk_open_query* queries, size_t n_queries, const amdzk_multiopen_opts* opts, uint64_t* out_points, size_t out_cap,
                   size_t* n_out, MoSets& s, std::unique_ptr<Call>& call) {
  if (n_out) *n_out = 0;
  if (!srs || !d_polys || !points || !queries || !opts) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen: null argument");
  if (opts->size < sizeof(amdzk_multiopen_opts))
    ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen: amdzk_multiopen_opts.size %zu < %zu", opts->size, sizeof(amdzk_multiopen_opts));
  const amdzk_transcript* t = opts->transcript;
  if (!t) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen: a transcript is required");
  if (!t->common_point || !t->common_scalar || !t->write_point || !t->write_scalar || !t->squeeze_challenge)
    ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen: amdzk_transcript has a null member");
  char why[200];
  const int pr = mo_build(points, n_points, queries, n_queries, n_polys, zk_srs_k(srs), opts->scheme, s, nullptr, why);
  if (pr != AMDZK_OK) ZK_FAIL(ctx, pr, "multiopen: %s", why);
  // every point and every supplied evaluation, as amdzk_multiopen_verify asks: the grouping compares residues, the scalars
  // are computed with them
  for (size_t i = 0; i < n_points; i++)
    if (!fr_words_canonical(points + 4 * i)) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen: point %zu is not below the modulus", i);
  for (size_t i = 0; opts->evals && i < n_queries; i++)
    if (!fr_words_canonical(opts->evals + 4 * i)) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen: evaluation %zu is not below the modulus", i);
  for (size_t i = 0; i < n_queries; i++)
    if (!d_polys[queries[i].poly]) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen: polynomial %u (query %zu) is a null pointer", queries[i].poly, i);
  if (out_points && out_cap < s.n_out) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen: room for %zu points, %u will be written", out_cap, s.n_out);
  if (!zk_srs_has_basis(srs, AMDZK_BASIS_G)) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen: the parameters have no basis g (AMDZK_BASIS_G)");
  char* ws = nullptr;
  ZK_TRY(mo_reserve(ctx, "multiopen", s.scratch_bytes, &ws));
  call.reset(new Call(ctx, srs, d_polys, points, s, *t));
  Call& c = *call;
  c.d_poly = (Fr*)ws;
  c.tab.d_ptrs = (void**)(ws + s.poly_count * s.n * 32);
  c.tab.d_frs = (Fr*)(ws + s.poly_count * s.n * 32 + s.ptr_bytes);
  ZK_TRY(c.evaluations(queries, n_queries, opts->evals));
  if (s.gwc) ZK_TRY(c.gwc(queries));
  else ZK_TRY(c.shplonk());
  if (n_out) *n_out = c.written.size();
  if (out_points) memcpy(out_points, c.written.data(), c.written.size() * sizeof(G1Affine));
  return AMDZK_OK;
}

// ---- the verifier's side: multiopen/{shplonk, gwc}/verifier.rs [UP] over the caller's commitments (amdzk_multiopen_verify).
// The grouping is mo_build's, the scalars are opening.hpp's, exactly as verifier.hpp folds a proof's opening argument — with
// the caller's commitments as the bases, no h(X) expansion and weight 1. Everything the transcript decides is read on the
// host first; the device then checks the points and runs the one MSM. Bases: the commitments | the read points | g.
int mo_verify_body(amdzk_ctx* ctx, const uint64_t* g, const uint64_t* commitments, size_t n_coms, const uint64_t* points, size_t n_points,
                   const amdzk_open_query* queries, const uint64_t* evals, size_t n_queries, const amdzk_multiopen_verify_opts* opts, G1Affine pair[2],
                   std::vector<G1Affine>& bases, std::vector<Fr>& sc, uint32_t& status) {
  if (!g || !commitments || !points || !queries || !evals || !opts || !pair) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen_verify: null argument");
  if (opts->size < sizeof(amdzk_multiopen_verify_opts))
    ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen_verify: amdzk_multiopen_verify_opts.size %zu < %zu", opts->size, sizeof(amdzk_multiopen_verify_opts));
  const amdzk_transcript_read* t = opts->transcript;
  if (!t) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen_verify: a transcript is required");
  if (!t->common_point || !t->common_scalar || !t->read_point || !t->read_scalar || !t->squeeze_challenge)
    ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen_verify: amdzk_transcript_read has a null member");
  MoSets s;
  char why[200];
  const int pr = mo_build(points, n_points, queries, n_queries, n_coms, 0, opts->scheme, s, nullptr, why);
  if (pr != AMDZK_OK) ZK_FAIL(ctx, pr, "multiopen_verify: %s", why);
  for (size_t i = 0; i < n_points; i++)
    if (!fr_words_canonical(points + 4 * i)) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen_verify: point %zu is not below the modulus", i);
  for (size_t i = 0; i < n_queries; i++)
    if (!fr_words_canonical(evals + 4 * i)) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen_verify: evaluation %zu is not below the modulus", i);
  const size_t n_read = s.n_out, nb = n_coms + n_read + 1, G = nb - 1;
  if (nb >= ((size_t)1 << 30)) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen_verify: more than 2^30 - 2 commitments and points");
  bases.assign(nb, G1Affine());
  memcpy((void*)bases.data(), commitments, n_coms * sizeof(G1Affine));
  memcpy((void*)&bases[G], g, sizeof(G1Affine));
  sc.assign(2 * nb, Fr::zero());
  Fr* const Lc = sc.data();
  Fr* const Rc = sc.data() + nb;
  auto squeeze = [&](Fr* c) -> int {
    uint64_t w[4] = {0, 0, 0, 0};
    if (t->squeeze_challenge(t->user, w) != 0) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen_verify: the caller's transcript reported an error");
    if (!fr_words_canonical(w)) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen_verify: a squeezed challenge is not below the modulus");
    memcpy(c->l, w, 32);
    return (int)AMDZK_OK;
  };
  auto read = [&](size_t i) -> int {
    uint64_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (t->read_point(t->user, w) != 0) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen_verify: the caller's transcript reported an error");
    memcpy((void*)&bases[n_coms + i], w, sizeof(G1Affine));
    return (int)AMDZK_OK;
  };
  auto point = [&](uint32_t dp) {
    Fr z;
    memcpy(z.l, points + 4 * (size_t)s.dp_index[dp], 32);
    return z;
  };
  auto eval = [&](uint32_t q) {
    Fr e;
    memcpy(e.l, evals + 4 * (size_t)q, 32);
    return e;
  };
  Fr v, u;
  if (s.gwc) {
    ZK_TRY(squeeze(&v));
    for (size_t z = 0; z < n_read; z++) ZK_TRY(read(z));
    ZK_TRY(squeeze(&u));
    Fr up = Fr::one();
    for (size_t z = 0; z < n_read; z++) {  // L = sum_z u^z W_z, R = sum_z u^z (p_z W_z + sum_j v^j (C_j - e_j g))
      const size_t W = n_coms + z;
      Lc[W] = up;
      Rc[W] = mul(up, point((uint32_t)z));
      Fr vp = up, eb = Fr::zero();
      for (uint32_t q : s.g.gw[s.dp_rank[z]]) {
        Rc[queries[q].poly] = add(Rc[queries[q].poly], vp);
        eb = add(eb, mul(vp, eval(q)));
        vp = mul(vp, v);
      }
      Rc[G] = sub(Rc[G], eb);
      up = mul(up, u);
    }
  } else {
    Fr y;
    ZK_TRY(squeeze(&y));
    ZK_TRY(squeeze(&v));
    ZK_TRY(read(0));
    ZK_TRY(squeeze(&u));
    ZK_TRY(read(1));
    const opening::Grouping& gr = s.g;
    std::vector<Fr> rank_pt(s.rank_dp.size());
    for (size_t r = 0; r < rank_pt.size(); r++) rank_pt[r] = point(s.rank_dp[r]);
    const opening::Shplonk sh = opening::shplonk_sets(gr, rank_pt.data(), [&](uint32_t q) { return eval(s.pair_query[s.q_pair[q]]); }, y, v);
    const opening::AtU at = opening::at_u(gr, rank_pt.data(), u);
    Fr vp = Fr::one();
    for (size_t si = 0; si < gr.sets.size(); si++) {  // R = sum_i v^i z_i(u) sum_j y^j (C_ij - r_ij(u) g) - Z_T(u) h1 + u z_0(u) h2
      const std::vector<Fr> wgt = opening::weights_at(sh, si, u);
      Fr ru = Fr::zero(), coef = mul(vp, at.z[si]);
      for (size_t k = 0; k < wgt.size(); k++) ru = add(ru, mul(wgt[k], sh.E[si][k]));
      Rc[G] = sub(Rc[G], mul(coef, ru));
      for (uint32_t c : gr.sets[si].coms) {
        Rc[gr.coms[c]] = add(Rc[gr.coms[c]], coef);
        coef = mul(coef, y);
      }
      vp = mul(vp, v);
    }
    const size_t h1 = n_coms, h2 = n_coms + 1;
    Rc[h1] = sub(Rc[h1], at.zt);
    Rc[h2] = add(Rc[h2], mul(at.z0, u));
    Lc[h2] = at.z0;  // L = z_0(u) h2
  }
  // ---- the device: bases | status word | the two columns
  WsLayout w;
  w.take(nb * sizeof(G1Affine), 1);
  const size_t o_status = w.take(256, 1), o_sc = w.take(2 * nb * sizeof(Fr), 1), total = w.bytes();
  char* ws = nullptr;
  ZK_TRY(mo_reserve(ctx, "multiopen_verify", total, &ws));
  ZK_HIP(ctx, hipMemcpyAsync(ws, bases.data(), nb * sizeof(G1Affine), hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(ctx, hipMemcpyAsync(ws + o_sc, sc.data(), 2 * nb * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
  ZK_TRY(zk_points_check_dev(ctx, (G1Affine*)ws, nb, n_coms, (uint32_t*)(ws + o_status)));
  ZK_HIP(ctx, hipMemcpyAsync(&status, ws + o_status, sizeof(status), hipMemcpyDeviceToHost, ctx->stream));
  G1X* d_res = nullptr;
  ZK_TRY(zk_msm_bases_dev_xyzz(ctx, (const Fr*)(ws + o_sc), 2, nb, nb, (const G1Affine*)ws, &d_res));
  uint64_t jac[24];
  ZK_TRY(zk_msm_finish(ctx, d_res, 2, jac));  // the call's one host wait
  if (status != 0xffffffffu) {
    const size_t i = status >> 2;
    if (i < n_coms) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen_verify: commitment %zu has a coordinate >= q or is not on the curve", i);
    if (i < G) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen_verify: read point %zu has a coordinate >= q, is not on the curve or is the identity", i - n_coms);
    ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen_verify: g has a coordinate >= q, is not on the curve or is the identity");
  }
  for (int c = 0; c < 2; c++) {
    const G1Jac* j = reinterpret_cast<const G1Jac*>(jac + 12 * c);
    pair[c].x = j->z.is_zero() ? Fq::zero() : j->x;
    pair[c].y = j->z.is_zero() ? Fq::zero() : j->y;
  }
  return AMDZK_OK;
}

// the body, and a stream left idle whatever it said (the host images of the tables outlive every copy enqueued from them)
int mo_verify(amdzk_ctx* ctx, const uint64_t* g, const uint64_t* commitments, size_t n_coms, const uint64_t* points, size_t n_points,
              const amdzk_open_query* queries, const uint64_t* evals, size_t n_queries, const amdzk_multiopen_verify_opts* opts, G1Affine pair[2]) {
  std::vector<G1Affine> bases;
  std::vector<Fr> sc;
  uint32_t status = 0;
  return zk_quiet_if_refused(ctx, mo_verify_body(ctx, g, commitments, n_coms, points, n_points, queries, evals, n_queries, opts, pair, bases, sc, status));
}

}  // namespace

extern "C" {

int amdzk_multiopen_verify(amdzk_ctx* ctx, const uint64_t g[8], const uint64_t* commitments, size_t n_coms, const uint64_t* points, size_t n_points,
                           const amdzk_open_query* queries, const uint64_t* evals, size_t n_queries, const amdzk_multiopen_verify_opts* opts,
                           uint64_t pair_out[16]) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  if (!pair_out) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen_verify: null argument");
  G1Affine pair[2];
  ZK_TRY(mo_verify(ctx, g, commitments, n_coms, points, n_points, queries, evals, n_queries, opts, pair));
  memcpy(pair_out, pair, sizeof(pair));
  return AMDZK_OK;
}

int amdzk_multiopen_decide(amdzk_ctx* ctx, const uint64_t g[8], const uint64_t* commitments, size_t n_coms, const uint64_t* points, size_t n_points,
                           const amdzk_open_query* queries, const uint64_t* evals, size_t n_queries, const amdzk_multiopen_verify_opts* opts,
                           const amdzk_g2* s_g2, const amdzk_g2* g2, uint8_t* verdict) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  if (!s_g2 || !g2 || !verdict) ZK_FAIL(ctx, AMDZK_E_INVALID, "multiopen_verify: null argument");
  *verdict = 0;
  G1Affine pair[2];
  ZK_TRY(mo_verify(ctx, g, commitments, n_coms, points, n_points, queries, evals, n_queries, opts, pair));
  if (pair[0].is_inf() || pair[1].is_inf()) return AMDZK_OK;  // a pair with the identity must not read as valid
  const G1Affine g1[2] = {pair[0], a_neg(pair[1])};
  const amdzk_g2* qs[2] = {s_g2, g2};
  uint8_t one = 0;
  ZK_TRY(zk_pairing_products(ctx, "multiopen_verify", qs, 2, g1, 1, &one, nullptr));
  *verdict = one;
  return AMDZK_OK;
}

int amdzk_multiopen_plan(const uint64_t* points, size_t n_points, const amdzk_open_query* queries, size_t n_queries, size_t n_polys, uint32_t k,
                         int scheme, uint32_t* n_sets, uint32_t* n_out, size_t* scratch_bytes, uint32_t* set_of_poly) {
  MoSets s;
  char why[200];
  const int r = mo_build(points, n_points, queries, n_queries, n_polys, k, scheme, s, set_of_poly, why);
  if (r != AMDZK_OK) return r;
  if (n_sets) *n_sets = s.n_sets;
  if (n_out) *n_out = s.n_out;
  if (scratch_bytes) *scratch_bytes = s.scratch_bytes;
  return AMDZK_OK;
}

int amdzk_multiopen_dev(amdzk_ctx* ctx, const amdzk_srs* srs, const void* const* d_polys, size_t n_polys, const uint64_t* points, size_t n_points,
                        const amdzk_open_query* queries, size_t n_queries, const amdzk_multiopen_opts* opts, uint64_t* out_points, size_t out_cap,
                        size_t* n_out) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  MoSets s;
  std::unique_ptr<Call> call;  // owns the host images of the tables: it outlives every copy enqueued from them
  // whatever the call enqueued has run before the caller sees a refusal
  return zk_quiet_if_refused(ctx, multiopen_body(ctx, srs, d_polys, n_polys, points, n_points, queries, n_queries, opts, out_points, out_cap, n_out, s, call));
}

}  // extern "C"
