// fq12.cuh — the BN254 extension tower and the device half of the optimal ate pairing, on the 9 x 29-bit form of fp29.cuh.
//
// Conventions (the published BN254 / EIP-197 ones; tests/pairing_ref.py restates them). The reference repository holds no
// G2 data and calls no pairing, so — as for the other recalled formats of DESIGN.md §4 — parity is UNPINNED: what pins this
// file is the integer reference of tests/pairing_ref.py (bilinear, non-degenerate, exact exponent), limb for limb.
//   Fq2  = Fq[u]/(u^2 + 1),  xi = 9 + u
//   Fq6  = Fq2[v]/(v^3 - xi)
//   Fq12 = Fq6[w]/(w^2 - v)
//   G2   = the order-r subgroup of the D-type twist y^2 = x^3 + 3/xi over Fq2; untwist (x, y) -> (x w^2, y w^3)
//   G2 generator: EIP-197's (pairing.hpp).  u = 4965661367192848881.
//   Optimal ate: Miller loop over 6u + 2 (plain binary), then the two Frobenius lines of pi(Q) and -pi^2(Q).
//   e(P, Q) = f^((p^12 - 1)/r), the EXACT exponent: the hard part is the Scott et al. chain for
//   (p^4 - p^2 + 1)/r = l0 + l1 p + l2 p^2 + p^3 with l0 = -36u^3 - 30u^2 - 18u - 2, l1 = -36u^3 - 18u^2 - 12u + 1,
//   l2 = 6u^2 + 1 — no extra power: c = 1. The GT value is therefore canonical: it does not depend on how lines are
//   scaled (factors in proper subfields die in the easy part), on binary against NAF, or on the chain.
//
// In-memory formats are halo2curves': G2Affine {x.c0, x.c1, y.c0, y.c1} and Fq12 as 12 Fq in declaration order
// (c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1), Montgomery R = 2^256. Inside, every Fq is an Fq29 in radix 2^261.
//
// Value discipline, as fp29.cuh: every function states the bound of its result in units of p. ONE invariant carries the
// tower: a STORED coefficient (anything in a register of the slab, between two program words) is normalised and below 2p.
// Products come out below 2p by themselves; sums and differences go through f29_reduce_weak (about 30 instructions,
// below 1.0003p). A host build with FP29_CHECK_BOUNDS (tests/native/pairing_host_check.cpp) runs the whole pairing with
// these bounds as hard failures.
//
// Registers and memory: one Fq12 is 108 VGPRs in this form, so no code here holds one in registers — and none keeps one on
// the stack either: the library ships no kernel with a private segment (tests/test_miscompile_guard.py). The tower is
// therefore split in two. THIS file is the Fq2 layer and an executor: a lane owns a slab of Fq2 "registers" in global
// memory (72 bytes each, contiguous per lane) and runs a flat program of three-address words over it, one Fq2-sized
// piece at a time — 18 VGPRs per operand, a few thousand instructions of code, no calls, no arrays. pairing.hpp writes the
// programs: the Fq6 / Fq12 products and squarings, the sparse line product, Frobenius, cyclotomic squaring, the
// inversion, the Miller loop and the final exponentiation are emitters there, flattened once on the host. The host check
// (tests/native/pairing_host_check.cpp) runs the same programs through the same executor.
#ifndef AMDZK_FQ12_CUH
#define AMDZK_FQ12_CUH
#include "fp29.cuh"

namespace bn254 {

struct Fq2x {
  Fq29 c0, c1;
};
constexpr uint64_t BN_U = 4965661367192848881ull;       // the curve parameter, 63 bits
constexpr uint64_t ATE_LOOP_LOW = 0x9d797039be763ba8ull;  // 6u + 2 = 2^64 + this
constexpr int ate_popcount() {
  int c = 0;
  for (int i = 0; i < 64; i++) c += (int)((ATE_LOOP_LOW >> i) & 1);
  return c;
}
// one line per doubling, one per set bit below the top one, and the two Frobenius lines
constexpr int PAIRING_NUM_LINES = 64 + ate_popcount() + 2;

// ---------------------------------------------------------------------------------- Fq, stored form
ZK_HD Fq29 fqx_zero() {
  Fq29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = 0;
  return r;
}
// a, b below 2p -> below 1.0003p
ZK_HD Fq29 fqx_add(const Fq29& a, const Fq29& b) { return f29_reduce_weak(f29_add_lazy(a, b)); }
// a, b below 2p -> a - b + 3p below 5p -> below 1.0003p
ZK_HD Fq29 fqx_sub(const Fq29& a, const Fq29& b) { return f29_reduce_weak(f29_sub3(a, b)); }
// a below 2p -> 3p - a, at most 3p -> below 1.0003p
ZK_HD Fq29 fqx_neg(const Fq29& a) { return f29_reduce_weak(f29_neg3(a)); }
// 9a + b (minus = false) or 9a - b + 3p (minus = true) for a, b below 2p, normalised, in ONE carry chain: below 21p,
// normalised -> below 1.0003p. (The 3p digits are raised by 2^30, so no term of the chain goes negative.)
ZK_HD Fq29 fqx_9a_pm_b(const Fq29& a, const Fq29& b, bool minus) {
  for (int i = 0; i < 8; i++) F29_REQUIRE(a.l[i] < (1u << 29) && b.l[i] < (1u << 29), "9a_pm_b: operand not normalised");
  F29_REQUIRE(b.l[8] <= Fq29P::c3(8), "9a_pm_b: subtrahend too large");
  Fq29 r;
  uint64_t acc = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    acc += 9ull * a.l[i] + (minus ? (uint64_t)(Fq29P::c3(i) - b.l[i]) : (uint64_t)b.l[i]);
    r.l[i] = i < 8 ? ((uint32_t)acc & F29_MASK) : (uint32_t)acc;
    acc >>= 29;
  }
  return f29_reduce_weak(r);
}
// 1/a for a below 2p (0 for 0): the Fermat chain a^(p-2), about 380 products; below 2p.
ZK_HD Fq29 fqx_inv(const Fq29& a) {
  Fq29 r = f29_one<Fq29P>();
  bool started = false;
#pragma unroll 1
  for (int limb = 7; limb >= 0; limb--) {
    // p - 2: the lowest limb ends in ...47, so only limb 0 changes
    const uint32_t w = limb == 0 ? FqP::p(0) - 2u : (limb == 1 ? FqP::p(1) : limb == 2 ? FqP::p(2) : limb == 3 ? FqP::p(3) : limb == 4 ? FqP::p(4)
                                                   : limb == 5 ? FqP::p(5) : limb == 6 ? FqP::p(6) : FqP::p(7));
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      if (started) r = f29_sqr(r);
      if ((w >> b) & 1) {
        r = f29_mul(r, a);
        started = true;
      }
    }
  }
  return r;
}

// ---------------------------------------------------------------------------------- Fq2 (results: stored form)
ZK_HD Fq2x fq2x_zero() { return Fq2x{fqx_zero(), fqx_zero()}; }
ZK_HD Fq2x fq2x_one() { return Fq2x{f29_one<Fq29P>(), fqx_zero()}; }
ZK_HD Fq2x fq2x_add(const Fq2x& a, const Fq2x& b) { return Fq2x{fqx_add(a.c0, b.c0), fqx_add(a.c1, b.c1)}; }  // < 1.0003
ZK_HD Fq2x fq2x_sub(const Fq2x& a, const Fq2x& b) { return Fq2x{fqx_sub(a.c0, b.c0), fqx_sub(a.c1, b.c1)}; }  // < 1.0003
ZK_HD Fq2x fq2x_dbl(const Fq2x& a) { return fq2x_add(a, a); }
ZK_HD Fq2x fq2x_neg(const Fq2x& a) { return Fq2x{fqx_neg(a.c0), fqx_neg(a.c1)}; }
ZK_HD Fq2x fq2x_conj(const Fq2x& a) { return Fq2x{a.c0, fqx_neg(a.c1)}; }
// (a0 + a1 u)(9 + u) = (9 a0 - a1) + (9 a1 + a0) u; below 1.0003p
ZK_HD Fq2x fq2x_mul_xi(const Fq2x& a) { return Fq2x{fqx_9a_pm_b(a.c0, a.c1, true), fqx_9a_pm_b(a.c1, a.c0, false)}; }
// Each component is a sum of two products under ONE reduction (f29_mul2): a0 b0 + (3p - a1) b1 is below 4 + 6 = 10 p^2
// and a0 b1 + a1 b0 below 8 p^2, inside 169 p^2; below 2p.
ZK_HD Fq2x fq2x_mul(const Fq2x& a, const Fq2x& b) {
  Fq2x r;
  r.c0 = f29_mul2(a.c0, b.c0, f29_neg3(a.c1), b.c1);
  r.c1 = f29_mul2(a.c0, b.c1, a.c1, b.c0);
  return r;
}
// (a0 + a1)(a0 - a1 + 3p): 4p * 5p = 20 p^2;  (2 a0) a1: 8 p^2; below 2p.
ZK_HD Fq2x fq2x_sqr(const Fq2x& a) {
  Fq2x r;
  r.c0 = f29_mul(f29_add(a.c0, a.c1), f29_sub3(a.c0, a.c1));
  r.c1 = f29_mul(f29_add(a.c0, a.c0), a.c1);
  return r;
}
ZK_HD Fq2x fq2x_mul_fq(const Fq2x& a, const Fq29& s) { return Fq2x{f29_mul(a.c0, s), f29_mul(a.c1, s)}; }  // < 2
// ---------------------------------------------------------------------------------- the executor
// One program word: op << 24 | d << 16 | a << 8 | b, over the lane's registers R[0..255] (stored form in, stored form out:
// every result below 2p, normalised). K: the constant table (pairing.hpp: 0, 1, the Frobenius constants).
enum PairOp : uint32_t {
  P_MUL = 0,  // R[d] = R[a] R[b]
  P_SQR,      // R[d] = R[a]^2
  P_ADD,      // R[d] = R[a] + R[b]
  P_SUB,      // R[d] = R[a] - R[b]
  P_NEG,      // R[d] = -R[a]
  P_CONJ,     // R[d] = conj(R[a]) = R[a]^p
  P_MULXI,    // R[d] = xi R[a]
  P_MOV,      // R[d] = R[a]
  P_MOVK,     // R[d] = K[b]
  P_MULK,     // R[d] = R[a] K[b]
  P_MULFQ,    // R[d] = R[a] * (R[b].c0 as an element of Fq)
  P_FQINV,    // R[d] = (1 / R[a].c0, 0)
  P_LINE      // R[d], R[d + 1] = the next prepared line's two Fq2 (packed canonical radix 2^261); advances the line pointer
};
ZK_HD constexpr uint32_t pair_word(uint32_t op, uint32_t d, uint32_t a, uint32_t b) { return op << 24 | d << 16 | a << 8 | b; }

ZK_HD void pairing_exec(const uint32_t* prog, uint32_t n, Fq2x* R, const Fq2x* K, const Fq* lines) {
#pragma unroll 1
  for (uint32_t pc = 0; pc < n; pc++) {
    const uint32_t w = prog[pc], d = (w >> 16) & 255u, a = (w >> 8) & 255u, b = w & 255u;
    switch (w >> 24) {
      case P_MUL:
      case P_MULK: {
        const Fq2x y = (w >> 24) == P_MULK ? K[b] : R[b];
        R[d] = fq2x_mul(R[a], y);
        break;
      }
      case P_SQR: R[d] = fq2x_sqr(R[a]); break;
      case P_ADD: R[d] = fq2x_add(R[a], R[b]); break;
      case P_SUB: R[d] = fq2x_sub(R[a], R[b]); break;
      case P_NEG: R[d] = fq2x_neg(R[a]); break;
      case P_CONJ: R[d] = fq2x_conj(R[a]); break;
      case P_MULXI: R[d] = fq2x_mul_xi(R[a]); break;
      case P_MOV: R[d] = R[a]; break;
      case P_MOVK: R[d] = K[b]; break;
      case P_MULFQ: R[d] = fq2x_mul_fq(R[a], R[b].c0); break;
      case P_FQINV: R[d] = Fq2x{fqx_inv(R[a].c0), fqx_zero()}; break;
      default:  // P_LINE
        R[d] = Fq2x{fq29_unpack(lines[0]), fq29_unpack(lines[1])};
        R[d + 1] = Fq2x{fq29_unpack(lines[2]), fq29_unpack(lines[3])};
        lines += 4;
        break;
    }
  }
}

// Six registers in tower order (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2) -> halo2curves' Fq12: 12 packed canonical Fq,
// Montgomery R = 2^256, declaration order.
ZK_HD void fq12x_to_r256(Fq out[12], const Fq2x* a) {
  for (int i = 0; i < 6; i++) {
    out[2 * i] = fq29_to_r256(a[i].c0);
    out[2 * i + 1] = fq29_to_r256(a[i].c1);
  }
}
ZK_HD bool gt_is_one(const Fq out[12]) {
  bool ok = out[0] == Fq::one();
  for (int i = 1; i < 12; i++) ok = ok && out[i].is_zero();
  return ok;
}

}  // namespace bn254
#endif
