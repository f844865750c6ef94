// The multiopen argument's host arithmetic, once, for its three users: the proof path (prover.hip), the stand-alone
// multiopen (multiopen.hip) and the verifier (verifier.hpp) — poly::kzg::multiopen::{shplonk, gwc} [UP]. Host-only: no HIP
// include, compiles with g++ (tests/native/opening_check.cpp runs it alone, also under ASan + UBSan). Inputs are indices and
// field elements, never device pointers, keys or contexts: each user keeps its own device driver and maps ids to what it has.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <map>
#include <vector>

#include "bn254.cuh"

namespace opening {

using bn254::Fr;

// ---- 1. grouping: integers only, so a key builds it once. Ids are opaque small integers: commitments below n_coms, points
// below n_pts. The proof path and the verifier name points by rotation id (first seen first), the stand-alone call by rank.
struct Query {
  uint32_t com, pt;
};
struct Grouping {
  std::vector<uint32_t> coms;                         // distinct commitment ids, first seen first
  std::vector<std::vector<uint32_t>> com_pts, com_q;  // per commitment: its point ids ascending | the first query of each pair
  struct Set {                                        // SHPLONK's construct_intermediate_sets
    std::vector<uint32_t> pts;                        // point ids, ascending
    std::vector<uint32_t> coms;                       // positions in `coms`, first seen first
  };
  std::vector<Set> sets;                  // distinct point-id sets, first seen first
  size_t set_points = 0, maxm = 0;        // sum_i |S_i|, max_i |S_i|
  std::vector<std::vector<uint32_t>> gw;  // GWC: per point id its queries, in their original order
};
inline Grouping group(const Query* q, size_t nq, size_t n_coms, size_t n_pts) {
  Grouping g;
  std::vector<uint32_t> at(n_coms, UINT32_MAX);
  g.gw.resize(n_pts);
  for (size_t i = 0; i < nq; i++) {
    g.gw[q[i].pt].push_back((uint32_t)i);
    uint32_t& c = at[q[i].com];
    if (c == UINT32_MAX) c = (uint32_t)g.coms.size(), g.coms.push_back(q[i].com), g.com_pts.emplace_back(), g.com_q.emplace_back();
    g.com_q[c].push_back((uint32_t)i);
  }
  for (size_t c = 0; c < g.coms.size(); c++) {  // by point, the first query of a (commitment, point) pair in front; the others go
    std::vector<uint32_t>& qs = g.com_q[c];
    std::stable_sort(qs.begin(), qs.end(), [&](uint32_t a, uint32_t b) { return q[a].pt < q[b].pt; });
    qs.erase(std::unique(qs.begin(), qs.end(), [&](uint32_t a, uint32_t b) { return q[a].pt == q[b].pt; }), qs.end());
    for (uint32_t i : qs) g.com_pts[c].push_back(q[i].pt);
  }
  std::map<std::vector<uint32_t>, uint32_t> set_of;
  for (size_t c = 0; c < g.coms.size(); c++) {
    const auto it = set_of.emplace(g.com_pts[c], (uint32_t)g.sets.size());
    if (it.second) g.sets.push_back({g.com_pts[c], {}});
    g.sets[it.first->second].coms.push_back((uint32_t)c);
  }
  for (const Grouping::Set& st : g.sets) g.set_points += st.pts.size(), g.maxm = std::max(g.maxm, st.pts.size());
  return g;
}

// ---- 4. a < b as integers, both canonical (bn254::from_mont): upstream's Ord for Fr
inline bool canon_less(const Fr& a, const Fr& b) {
  for (int i = 7; i >= 0; i--)
    if (a.l[i] != b.l[i]) return a.l[i] < b.l[i];
  return false;
}
inline Fr eval_small(const std::vector<Fr>& poly, const Fr& x) {
  Fr acc = Fr::zero();
  for (size_t i = poly.size(); i-- > 0;) acc = bn254::add(bn254::mul(acc, x), poly[i]);
  return acc;
}

// ---- 2. SHPLONK up to h(X). Per set i with points p_t in ascending canonical order, as upstream's BTreeSet holds them:
// R_i(X) = sum_j y^j R_ij(X), R_ij the interpolation of commitment j's evaluations. Interpolation is linear, so R_i is the
// interpolation of E_i[t] = sum_j y^j eval_ij[t]: R_i = sum_t E_i[t] c_it prod_{s != t} (X - p_s), c_it = 1 / prod_{s != t}
// (p_t - p_s) — one product per evaluation instead of one small interpolation per polynomial, and ONE field inversion for
// all c_it: on the proof path the host works here with the GPU idle.
struct Shplonk {
  std::vector<std::vector<uint32_t>> order;  // per set: positions in Set::pts by ascending point (the identity for ranks)
  std::vector<std::vector<Fr>> pts, c, E, low;  // per set: p_t | c_it | E_i[t] | R_i in coefficients
  // The division table, one row per (set, point) in that order: (L_i - R_i) / prod_t (X - p_t) = sum_t c_it (L_i - R_i) /
  // (X - p_t), since the points of a set are distinct and L_i - R_i vanishes at each; h(X) = sum_it v^i c_it Q_it.
  std::vector<uint32_t> row_set;
  std::vector<Fr> root, row_low, coef;  // p_t | R_i zero-padded to maxm coefficients | v^i c_it
};
// pt: the point values by id; eval(q): the evaluation that query q claims (asked for the first query of every kept pair)
template <class Eval>
Shplonk shplonk_sets(const Grouping& g, const Fr* pt, Eval eval, const Fr& y, const Fr& v) {
  using namespace bn254;
  const size_t S = g.sets.size();
  Shplonk sh;
  sh.order.resize(S), sh.pts.resize(S), sh.c.resize(S), sh.E.resize(S), sh.low.resize(S);
  std::vector<Fr> cn(g.gw.size()), dens;
  for (size_t id = 0; id < cn.size(); id++) cn[id] = from_mont(pt[id]);
  for (size_t i = 0; i < S; i++) {
    const std::vector<uint32_t>& ids = g.sets[i].pts;
    const size_t m = ids.size();
    std::vector<uint32_t>& order = sh.order[i];
    for (size_t t = 0; t < m; t++) order.push_back((uint32_t)t);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return canon_less(cn[ids[a]], cn[ids[b]]); });
    for (size_t t = 0; t < m; t++) sh.pts[i].push_back(pt[ids[order[t]]]);
    for (size_t t = 0; t < m; t++) {
      Fr den = Fr::one();
      for (size_t s = 0; s < m; s++)
        if (s != t) den = mul(den, sub(sh.pts[i][t], sh.pts[i][s]));
      dens.push_back(den);  // non-zero: the points of a set are distinct values
    }
  }
  // Montgomery's trick: prefix products, one inversion, walk back
  std::vector<Fr> pre(dens.size() + 1, Fr::one());
  for (size_t k = 0; k < dens.size(); k++) pre[k + 1] = mul(pre[k], dens[k]);
  Fr acc = inv(pre[dens.size()]);
  size_t at = dens.size();
  for (size_t i = S; i-- > 0;) {
    sh.c[i].resize(sh.pts[i].size());
    for (size_t t = sh.pts[i].size(); t-- > 0;) sh.c[i][t] = mul(acc, pre[--at]), acc = mul(acc, dens[at]);
  }
  Fr vpow = Fr::one();
  for (size_t i = 0; i < S; i++) {
    const std::vector<Fr>& p = sh.pts[i];
    const size_t m = p.size();
    sh.E[i].assign(m, Fr::zero());
    Fr yp = Fr::one();
    for (uint32_t c : g.sets[i].coms) {
      for (size_t t = 0; t < m; t++) sh.E[i][t] = add(sh.E[i][t], mul(yp, eval(g.com_q[c][sh.order[i][t]])));
      yp = mul(yp, y);
    }
    sh.low[i].assign(m, Fr::zero());
    for (size_t t = 0; t < m; t++) {
      std::vector<Fr> num(1, Fr::one());  // prod_{s != t} (X - p_s), ascending coefficients
      for (size_t s = 0; s < m; s++) {
        if (s == t) continue;
        num.push_back(Fr::zero());
        for (size_t d = num.size() - 1; d > 0; d--) num[d] = sub(num[d - 1], mul(p[s], num[d]));
        num[0] = neg(mul(p[s], num[0]));
      }
      const Fr w = mul(sh.E[i][t], sh.c[i][t]);
      for (size_t d = 0; d < m; d++) sh.low[i][d] = add(sh.low[i][d], mul(w, num[d]));
    }
    for (size_t t = 0; t < m; t++) {
      sh.row_set.push_back((uint32_t)i);
      sh.root.push_back(p[t]);
      sh.coef.push_back(mul(vpow, sh.c[i][t]));
      for (size_t d = 0; d < g.maxm; d++) sh.row_low.push_back(d < m ? sh.low[i][d] : Fr::zero());
    }
    vpow = mul(vpow, v);
  }
  return sh;
}

// ---- 3. SHPLONK behind u. Unscaled, for the verifier: Z_T(u) = prod over all points (u - p), z_i(u) = the same over the
// points outside set i, z_0(u), and a set's Lagrange weights at u from the shared c_it.
struct AtU {
  Fr zt, z0;
  std::vector<Fr> z;
};
inline AtU at_u(const Grouping& g, const Fr* pt, const Fr& u) {
  using namespace bn254;
  const size_t n_pts = g.gw.size();
  std::vector<Fr> diff(n_pts);
  AtU a{Fr::one(), Fr::one(), {}};
  for (size_t id = 0; id < n_pts; id++) diff[id] = sub(u, pt[id]), a.zt = mul(a.zt, diff[id]);
  for (const Grouping::Set& st : g.sets) {
    Fr zi = Fr::one();
    size_t k = 0;  // the set's ids are ascending: walk them beside id
    for (size_t id = 0; id < n_pts; id++) {
      if (k < st.pts.size() && st.pts[k] == id) k++;
      else zi = mul(zi, diff[id]);
    }
    a.z.push_back(zi);
  }
  if (!a.z.empty()) a.z0 = a.z[0];
  return a;
}
inline std::vector<Fr> weights_at(const Shplonk& sh, size_t i, const Fr& u) {  // c_it prod_{s != t} (u - p_s)
  std::vector<Fr> w = sh.c[i];
  for (size_t t = 0; t < w.size(); t++)
    for (size_t s = 0; s < w.size(); s++)
      if (s != t) w[t] = bn254::mul(w[t], bn254::sub(u, sh.pts[i][s]));
  return w;
}
// For the provers: l(X) = sum_i cf[i] L_i + cf[S] h(X) - cterm with cf[i] = v^i z_i(u) / z_0(u), cf[S] = -Z_T(u) / z_0(u),
// cterm = sum_i cf[i] R_i(u), so that l(X) / (X - u) is the second commitment. z0_zero: u is one of the opening points and
// nothing here is usable (inv(0) = 0); the caller decides what to say.
struct Final {
  bool z0_zero;
  std::vector<Fr> cf;
  Fr cterm;
};
inline Final shplonk_final(const Grouping& g, const Shplonk& sh, const Fr* pt, const Fr& v, const Fr& u) {
  using namespace bn254;
  const AtU a = at_u(g, pt, u);
  const size_t S = g.sets.size();
  Final f{a.z0.is_zero(), std::vector<Fr>(S + 1), Fr::zero()};
  const Fr z0inv = inv(a.z0);
  Fr cur = z0inv;
  for (size_t i = 0; i < S; i++) {
    f.cf[i] = mul(cur, a.z[i]);
    f.cterm = add(f.cterm, mul(f.cf[i], eval_small(sh.low[i], u)));
    cur = mul(cur, v);
  }
  f.cf[S] = mul(neg(a.zt), z0inv);
  return f;
}

}  // namespace opening
