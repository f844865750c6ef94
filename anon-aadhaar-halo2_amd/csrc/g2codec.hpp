// g2codec.hpp — the 64-byte G2 fields of the SRS file <-> G2Affine words, and membership in G2: what is
// behind amdzk_g2_compress / amdzk_g2_decompress / amdzk_g2_check. Host only, plain C++ over pairing.hpp's Fq2 and G2
// arithmetic, with no HIP and no ctx in it (tests/native/g2_codec_check.cpp builds it with the host compiler alone).
// The format is halo2curves 0.3.1's G2Compressed [UP recall], made by the macro that makes the 32-byte G1 form
// (srs.hip g1_compress_kernel / g1_decompress_kernel): x.c0 | x.c1, canonical little-endian; bit 7 of byte 63 = the parity of
// the canonical y.c0 (y.to_bytes()[0] & 1, Fq2::to_bytes being c0 | c1); 64 zero bytes = the identity. Bit 6 of byte 63 is
// always 0 (x.c1 < q < 2^254), so a set bit 6 reads as "x >= q".
#pragma once
#include <stdint.h>
#include <string.h>

#include "pairing.hpp"

namespace g2codec {
using namespace bn254;
using pairing::Fq2;
using pairing::G2Affine;

// amdzk_g2_check's statuses
constexpr int G2_IN_GROUP = 0, G2_COORD_TOO_LARGE = 1, G2_OFF_TWIST = 2, G2_IDENTITY = 3, G2_OUTSIDE_SUBGROUP = 4;

// (q - sub) >> shift as an exponent of f2_pow; sub < 2^32 and q's low word is above it, so no borrow leaves word 0
inline void q_minus_shifted(uint32_t sub, int shift, uint32_t e[8]) {
  uint32_t w[8];
  for (int i = 0; i < 8; i++) w[i] = FqP::p(i);
  w[0] -= sub;
  for (int i = 0; i < 8; i++) e[i] = (w[i] >> shift) | (i < 7 ? w[i + 1] << (32 - shift) : 0u);
}

// A square root in Fq2 for q = 3 mod 4 (Adj, Rodriguez-Henriquez, "Square root computation over even extension fields",
// algorithm 9): a1 = a^((q-3)/4), alpha = a1^2 a = a^((q-1)/2), x0 = a1 a = a^((q+1)/4); alpha^(q+1) = -1 exactly when a is
// a non-residue; the root is u x0 when alpha = -1 and (1 + alpha)^((q-1)/2) x0 otherwise. Whatever came out is squared and
// compared, so a false return is "a has no root" with nothing taken on trust.
inline bool f2_sqrt(const Fq2& a, Fq2* out) {
  if (a.is_zero()) {
    *out = a;
    return true;
  }
  uint32_t e34[8], e12[8];
  q_minus_shifted(3, 2, e34);
  q_minus_shifted(1, 1, e12);
  const Fq2 a1 = pairing::f2_pow(a, e34);
  const Fq2 alpha = pairing::f2_mul(pairing::f2_sqr(a1), a), x0 = pairing::f2_mul(a1, a);
  const Fq2 minus_one = pairing::f2_neg(pairing::f2_one());
  Fq2 x;
  if (alpha == minus_one) {
    x = Fq2{neg(x0.c1), x0.c0};  // u x0
  } else {
    x = pairing::f2_mul(pairing::f2_pow(pairing::f2_add(pairing::f2_one(), alpha), e12), x0);
  }
  *out = x;
  return pairing::f2_sqr(x) == a;
}

inline bool g2_coords_canonical(const G2Affine& p) {
  return is_canonical(p.x.c0) && is_canonical(p.x.c1) && is_canonical(p.y.c0) && is_canonical(p.y.c1);
}

// [r]Q = O: the definition of G2 inside the twist (whose cofactor 2q - r is about 2^254). q on the twist and finite.
inline bool g2_in_subgroup(const G2Affine& q) {
  uint64_t r[4];
  for (int i = 0; i < 4; i++) r[i] = (uint64_t)FrP::p(2 * i) | ((uint64_t)FrP::p(2 * i + 1) << 32);
  return pairing::g2_mul(q, r).is_inf();
}

inline int g2_status(const uint64_t w[16]) {
  const G2Affine p = pairing::g2_from_words(w);
  if (!g2_coords_canonical(p)) return G2_COORD_TOO_LARGE;
  if (p.is_inf()) return G2_IDENTITY;
  if (!pairing::g2_on_twist(p)) return G2_OFF_TWIST;
  return g2_in_subgroup(p) ? G2_IN_GROUP : G2_OUTSIDE_SUBGROUP;
}

// nullptr, or why the point has no encoding
inline const char* g2_compress(const uint64_t w[16], uint8_t out[64]) {
  const G2Affine p = pairing::g2_from_words(w);
  if (!g2_coords_canonical(p)) return "a coordinate is not below the modulus";
  memset(out, 0, 64);
  if (p.is_inf()) return nullptr;
  if (!pairing::g2_on_twist(p)) return "the point is not on the twist";
  const Fq c0 = from_mont(p.x.c0), c1 = from_mont(p.x.c1), y0 = from_mont(p.y.c0);
  for (int i = 0; i < 8; i++)
    for (int b = 0; b < 4; b++) {
      out[4 * i + b] = (uint8_t)(c0.l[i] >> (8 * b));
      out[32 + 4 * i + b] = (uint8_t)(c1.l[i] >> (8 * b));
    }
  out[63] |= (uint8_t)((y0.l[0] & 1u) << 7);
  return nullptr;
}

// nullptr, or why the bytes are no point's encoding
inline const char* g2_decompress(const uint8_t in[64], uint64_t w[16]) {
  Fq c[2];
  for (int h = 0; h < 2; h++)
    for (int i = 0; i < 8; i++)
      c[h].l[i] = (uint32_t)in[32 * h + 4 * i] | ((uint32_t)in[32 * h + 4 * i + 1] << 8) | ((uint32_t)in[32 * h + 4 * i + 2] << 16) |
                  ((uint32_t)in[32 * h + 4 * i + 3] << 24);
  const uint32_t ysign = c[1].l[7] >> 31;
  c[1].l[7] &= 0x7fffffffu;
  if (!is_canonical(c[0]) || !is_canonical(c[1])) return "x is not below the modulus (x >= q)";
  if (c[0].is_zero() && c[1].is_zero()) {
    if (ysign) return "x = 0 with the sign bit set is no point's encoding";
    memset(w, 0, 16 * sizeof(uint64_t));
    return nullptr;
  }
  G2Affine p;
  p.x = Fq2{to_mont(c[0]), to_mont(c[1])};
  const Fq2 rhs = pairing::f2_add(pairing::f2_mul(pairing::f2_sqr(p.x), p.x), pairing::consts().twist_b);
  if (!f2_sqrt(rhs, &p.y)) return "x^3 + 3/xi is not a square: no point of the twist has this x";
  if ((from_mont(p.y.c0).l[0] & 1u) != ysign) p.y = pairing::f2_neg(p.y);
  pairing::g2_to_words(p, w);
  return nullptr;
}

}  // namespace g2codec
