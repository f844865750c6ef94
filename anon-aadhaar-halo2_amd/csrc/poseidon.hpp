// Poseidon over Fr (include/amdzk.h "Poseidon over Fr") — the host half: the validation, the plain
// statement of the semantics (pos::permute, pos::sponge over bn254.cuh's 8 x 32-bit field) and the LANE STEP of the kernels
// of poseidon.hip (pos::lane_absorb, pos::lane_sbox, pos::lane_mix over fp29.cuh's 29-bit limbs). The lane step is ZK_HD, so
// that a host loop over eight "lanes" (pos::lanes_permute, pos::lanes_sponge; tests/native/poseidon_check.cpp) runs the same
// code the device runs, under FP29_CHECK_BOUNDS with its preconditions as hard failures. Nothing here touches the device: a
// plain host compiler builds this file.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/amdzk.h"
#include "fp29.cuh"

namespace pos {

using bn254::Fr;
using bn254::Fr29;
using bn254::Fr29P;

constexpr uint32_t MAX_T = 8;
constexpr uint32_t GROUP = 8;            // lanes of one sponge: state element i in lane i, lanes >= t idle
constexpr uint32_t BLOCK = 256;          // 32 sponges
constexpr uint32_t MAX_RC = 1536;        // (r_f + r_p) * t: the round constants of a spec stay in a block's LDS (48 KiB)
constexpr uint64_t MAX_N = 0x7fffffffu;  // sponges or states of one call; also the longest input

// ---- the validated spec: values as the caller gave them (Montgomery radix 2^256, below r)
struct Spec {
  uint32_t t = 0, rate = 0, r_f = 0, r_p = 0;
  std::vector<Fr> rc;   // (r_f + r_p) x t
  std::vector<Fr> mds;  // t x t, row-major
  Fr init[MAX_T];
  uint32_t rounds() const { return r_f + r_p; }
};

inline int refuse(std::string& err, int code, const char* fmt, uint64_t x = 0, uint64_t y = 0, uint64_t z = 0) {
  char b[256];
  snprintf(b, sizeof(b), fmt, (unsigned long long)x, (unsigned long long)y, (unsigned long long)z);
  err = std::string("poseidon: ") + b;
  return code;
}

inline Fr load_fr(const uint64_t* words, size_t i) {
  Fr v;
  memcpy(v.l, words + 4 * i, 32);
  return v;
}

inline int check(const amdzk_poseidon_desc* d, Spec& s, std::string& err) {
  if (!d) return refuse(err, AMDZK_E_INVALID, "null description");
  if (d->size < sizeof(amdzk_poseidon_desc)) return refuse(err, AMDZK_E_INVALID, "desc->size %llu is too small (%llu)", d->size, sizeof(amdzk_poseidon_desc));
  if (d->t < 2 || d->t > MAX_T) return refuse(err, AMDZK_E_INVALID, "t = %llu is outside 2..8", d->t);
  if (d->rate < 1 || d->rate > d->t - 1) return refuse(err, AMDZK_E_INVALID, "rate = %llu is outside 1..t-1 = %llu", d->rate, d->t - 1);
  if (d->r_f < 2 || (d->r_f & 1)) return refuse(err, AMDZK_E_INVALID, "r_f = %llu is not an even number >= 2", d->r_f);
  if (!d->round_constants || !d->mds) return refuse(err, AMDZK_E_INVALID, "null round_constants or mds");
  if (d->r_f > MAX_RC || d->r_p > MAX_RC || (d->r_f + d->r_p) * d->t > MAX_RC)
    return refuse(err, AMDZK_E_UNSUPPORTED, "(r_f + r_p) * t = (%llu + %llu) * %llu is above 1536", d->r_f, d->r_p, d->t);
  s = Spec();
  s.t = d->t;
  s.rate = d->rate;
  s.r_f = d->r_f;
  s.r_p = d->r_p;
  s.rc.resize((size_t)s.rounds() * s.t);
  for (size_t i = 0; i < s.rc.size(); i++) {
    s.rc[i] = load_fr(d->round_constants, i);
    if (!bn254::is_canonical(s.rc[i])) return refuse(err, AMDZK_E_INVALID, "round constant %llu of round %llu is not below the modulus", i % s.t, i / s.t);
  }
  s.mds.resize((size_t)s.t * s.t);
  for (size_t i = 0; i < s.mds.size(); i++) {
    s.mds[i] = load_fr(d->mds, i);
    if (!bn254::is_canonical(s.mds[i])) return refuse(err, AMDZK_E_INVALID, "mds[%llu][%llu] is not below the modulus", i / s.t, i % s.t);
  }
  for (uint32_t i = 0; i < MAX_T; i++) s.init[i] = Fr::zero();
  if (d->initial_state) {
    for (uint32_t i = 0; i < s.t; i++) {
      s.init[i] = load_fr(d->initial_state, i);
      if (!bn254::is_canonical(s.init[i])) return refuse(err, AMDZK_E_INVALID, "initial_state[%llu] is not below the modulus", i);
    }
  } else {
    Fr c = Fr::zero();
    c.l[2] = 1;  // the integer 2^64
    s.init[0] = bn254::to_mont(c);
  }
  return AMDZK_OK;
}

// ---- the semantics, stated plainly over the 8 x 32-bit field. s: t elements.
inline void permute(const Spec& sp, Fr* s) {
  const uint32_t t = sp.t, half = sp.r_f / 2;
  for (uint32_t rho = 0; rho < sp.rounds(); rho++) {
    for (uint32_t i = 0; i < t; i++) s[i] = bn254::add(s[i], sp.rc[(size_t)rho * t + i]);
    const bool full = rho < half || rho >= half + sp.r_p;
    for (uint32_t i = 0; i < (full ? t : 1u); i++) {
      const Fr x2 = bn254::mul(s[i], s[i]);
      s[i] = bn254::mul(bn254::mul(x2, x2), s[i]);
    }
    Fr o[MAX_T];
    for (uint32_t i = 0; i < t; i++) {
      o[i] = Fr::zero();
      for (uint32_t j = 0; j < t; j++) o[i] = bn254::add(o[i], bn254::mul(sp.mds[(size_t)i * t + j], s[j]));
    }
    for (uint32_t i = 0; i < t; i++) s[i] = o[i];
  }
}
inline Fr sponge(const Spec& sp, const Fr* in, size_t len) {
  Fr s[MAX_T];
  for (uint32_t i = 0; i < sp.t; i++) s[i] = sp.init[i];
  size_t a = 0;
  for (; len - a >= sp.rate; a += sp.rate) {
    for (uint32_t i = 0; i < sp.rate; i++) s[1 + i] = bn254::add(s[1 + i], in[a + i]);
    permute(sp, s);
  }
  const uint32_t m = (uint32_t)(len - a);  // < rate
  for (uint32_t i = 0; i < m; i++) s[1 + i] = bn254::add(s[1 + i], in[a + i]);
  s[1 + m] = bn254::add(s[1 + m], Fr::one());
  permute(sp, s);
  return s[1];
}

// ---- what the kernels read: every constant packed canonical in Montgomery radix 2^261 (fr29_const_to_r261, the form
// f29_mul and f29_wide_madd multiply a radix-2^261 state by): [ rc: rounds x t | mds: t x t | initial state: t ].
struct Compiled {
  uint32_t t = 0, rate = 0, r_f = 0, r_p = 0;
  std::vector<Fr> k;
  uint32_t rounds() const { return r_f + r_p; }
  size_t rc_off() const { return 0; }
  size_t mds_off() const { return (size_t)rounds() * t; }
  size_t init_off() const { return mds_off() + (size_t)t * t; }
};
inline Compiled compile(const Spec& s) {
  Compiled c;
  c.t = s.t;
  c.rate = s.rate;
  c.r_f = s.r_f;
  c.r_p = s.r_p;
  c.k.reserve(s.rc.size() + s.mds.size() + s.t);
  for (const Fr& v : s.rc) c.k.push_back(bn254::fr29_const_to_r261(v));
  for (const Fr& v : s.mds) c.k.push_back(bn254::fr29_const_to_r261(v));
  for (uint32_t i = 0; i < s.t; i++) c.k.push_back(bn254::fr29_const_to_r261(s.init[i]));
  return c;
}

// ---- the lane step. A state element is x * 2^261 on nine 29-bit limbs, normalised, from entry to exit. Loop-carried
// bound: below 2p after a permutation, below 4p after the absorption that may follow it (bounds in units of p = r).

// v normalised and below n p, judged by the top limb (which is what fp29.cuh's own checks look at)
#define POS_REQUIRE_BELOW(v, n, what)                                                        \
  do {                                                                                       \
    for (int i_ = 0; i_ < 8; i_++) F29_REQUIRE((v).l[i_] < (1u << 29), what ": not normalised"); \
    F29_REQUIRE((v).l[8] < (n) * (Fr29P::p(8) + 1), what ": value too large");               \
  } while (0)

// Entry and exit: x * 2^256 packed canonical <-> x * 2^261, one product each.
ZK_HD Fr29 lane_enter(const Fr& x) { return bn254::f29_mul(bn254::fr29_unpack(x), bn254::f29_k_in<Fr29P>()); }  // below 2p
ZK_HD Fr lane_exit(const Fr29& s) {                                                                             // s below 4p
  POS_REQUIRE_BELOW(s, 4u, "lane_exit");
  return bn254::f29_pack_canonical<bn254::FrP>(bn254::f29_mul(s, bn254::f29_k_out<Fr29P>()));  // 4 p^2 -> below 2p -> canonical
}

// What lane `lane` of a sponge of `len` inputs takes in before permutation c (c <= len / rate): input a = c * rate + lane - 1
// when a < len, ONE when a = len, nothing beyond and nothing in lanes 0 and > rate. load(a): input a, packed radix 2^256,
// below r. s below 2p; result below 4p, normalised.
template <class L>
ZK_HD Fr29 lane_absorb(uint32_t lane, uint32_t rate, const Fr29& s, uint32_t c, uint32_t len, L&& load) {
  POS_REQUIRE_BELOW(s, 2u, "lane_absorb");
  if (lane == 0 || lane > rate) return s;
  const uint64_t a = (uint64_t)c * rate + (lane - 1);
  if (a > len) return s;
  const Fr29 x = a < len ? lane_enter(load((uint32_t)a)) : bn254::f29_one<Fr29P>();  // below 2p
  return bn254::f29_add(s, x);                                                      // below 4p
}

// This lane's element through the round constant and the S-box layer. s below 4p, normalised; rc canonical. `full`: a full
// round. Result normalised: below 2p where the S-box is taken (every lane of a full round, lane 0 of a partial one), below
// 5p where the element is kept.
ZK_HD Fr29 lane_sbox(uint32_t lane, const Fr29& s, const Fr29& rc, bool full) {
  POS_REQUIRE_BELOW(s, 4u, "lane_sbox");
  POS_REQUIRE_BELOW(rc, 1u, "lane_sbox constant");
  const Fr29 x = bn254::f29_add(s, rc);       // below 5p
  const Fr29 x2 = bn254::f29_sqr(x);          // 25 p^2 -> below 2p
  const Fr29 x4 = bn254::f29_sqr(x2);         // 4 p^2 -> below 2p
  const Fr29 x5 = bn254::f29_mul(x4, x);      // 10 p^2 -> below 2p
  const bool take = full || lane == 0;
  Fr29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = take ? x5.l[i] : x.l[i];
  return r;
}

// This lane's row of M·s: sum_j row[j] * y(j) with ONE reduction. row: t x 9 limbs, the lane's MDS row, canonical radix
// 2^261, normalised; y(j): element j after lane_sbox (on the device: a broadcast within the group), below 5p, normalised.
// A column of the sum takes six terms of 9 * 2^58 (fp29.cuh, f29_wide_madd): t = 7, 8 carry after the sixth. The sum is
// below t * 5 p^2 <= 40 p^2: the result is below 40 / 169.3 + 1 < 2p, normalised.
template <class G>
ZK_HD Fr29 lane_mix(uint32_t t, const uint32_t* row, G&& y) {
  bn254::F29Wide w;
  bn254::f29_wide_zero(w);
#pragma unroll
  for (uint32_t j = 0; j < MAX_T; j++) {
    if (j < t) {
      const Fr29 yj = y(j);
      POS_REQUIRE_BELOW(yj, 5u, "lane_mix element");
      for (int i = 0; i < 9; i++) F29_REQUIRE(row[9 * j + i] < (1u << 29), "lane_mix: MDS limb not normalised");
      bn254::f29_wide_madd(w, yj, row + 9 * j);
      if (j == 5 && t > 6) bn254::f29_wide_carry(w);
    }
  }
  bn254::f29_wide_carry(w);
  return bn254::f29_wide_redc<Fr29P>(w);
}

// ---- the host loop over eight lanes: the kernels' control flow with an array in place of the wavefront
inline void unpack_row(const Compiled& c, uint32_t el, uint32_t* row /* MAX_T x 9 */) {
  for (uint32_t j = 0; j < MAX_T; j++) {
    Fr29 m;
    for (int i = 0; i < 9; i++) m.l[i] = 0;
    if (j < c.t) m = bn254::fr29_unpack(c.k[c.mds_off() + (size_t)el * c.t + j]);
    for (int i = 0; i < 9; i++) row[9 * j + i] = m.l[i];
  }
}
inline void lanes_permute(const Compiled& c, Fr29 s[GROUP]) {
  const uint32_t t = c.t, half = c.r_f / 2;
  uint32_t rows[GROUP][MAX_T * 9];
  for (uint32_t lane = 0; lane < GROUP; lane++) unpack_row(c, lane < t ? lane : t - 1, rows[lane]);
  for (uint32_t rho = 0; rho < c.rounds(); rho++) {
    const bool full = rho < half || rho >= half + c.r_p;
    Fr29 y[GROUP], o[GROUP];
    for (uint32_t lane = 0; lane < GROUP; lane++)
      y[lane] = lane_sbox(lane, s[lane], bn254::fr29_unpack(c.k[c.rc_off() + (size_t)rho * t + (lane < t ? lane : t - 1)]), full);
    for (uint32_t lane = 0; lane < GROUP; lane++) o[lane] = lane_mix(t, rows[lane], [&](uint32_t j) { return y[j]; });
    for (uint32_t lane = 0; lane < GROUP; lane++) s[lane] = o[lane];
  }
}
// states in and out packed radix 2^256 (t elements); lanes >= t carry a copy of lane t - 1's start, as idle lanes of the
// kernel carry something within the bounds
inline void lanes_permute_state(const Compiled& c, Fr* state) {
  Fr29 s[GROUP];
  for (uint32_t lane = 0; lane < GROUP; lane++) s[lane] = lane_enter(state[lane < c.t ? lane : c.t - 1]);
  lanes_permute(c, s);
  for (uint32_t lane = 0; lane < c.t; lane++) state[lane] = lane_exit(s[lane]);
}
inline Fr lanes_sponge(const Compiled& c, const Fr* in, uint32_t len) {
  Fr29 s[GROUP];
  for (uint32_t lane = 0; lane < GROUP; lane++) s[lane] = bn254::fr29_unpack(c.k[c.init_off() + (lane < c.t ? lane : c.t - 1)]);
  const uint32_t count = len / c.rate + 1;
  for (uint32_t p = 0; p < count; p++) {
    for (uint32_t lane = 0; lane < c.t; lane++) s[lane] = lane_absorb(lane, c.rate, s[lane], p, len, [&](uint32_t a) { return in[a]; });
    lanes_permute(c, s);
  }
  return lane_exit(s[1]);
}

}  // namespace pos
