// pairing.hpp — the host half of the pairing unit: Fq2 and G2 arithmetic, s * G2, and g2_prepare, which
// turns ONE G2 point into the line coefficients of every step of the Miller loop (what halo2curves' G2Prepared holds), so
// that the device half (fq12.cuh, pairing.hip) does no G2 arithmetic at all — and the PROGRAMS the device half runs: the
// tower above Fq2 (Fq6 / Fq12 products and squarings, the sparse line product, Frobenius, cyclotomic squaring, inversion),
// the Miller loop and the final exponentiation as emitters of fq12.cuh's three-address words, flattened once per process.
// Plain C++ with no HIP in it, like verifier.hpp: the arithmetic is O(100) Fq2 operations per point — the O(1) glue the
// header of bn254.cuh puts on the host.
// Conventions: the top of fq12.cuh. Values here are bn254.cuh's Fq (canonical, Montgomery R = 2^256); only the prepared
// lines and the Frobenius constants leave in the device half's radix 2^261.
#pragma once
#include <string.h>

#include <vector>

#include "../../include/amdzk.h"
#include "fq12.cuh"
#include "workspace.hpp"

namespace pairing {
using namespace bn254;

struct Fq2 {
  Fq c0, c1;
  bool is_zero() const { return c0.is_zero() && c1.is_zero(); }
  bool operator==(const Fq2& b) const { return c0 == b.c0 && c1 == b.c1; }
};
inline Fq fq_small(uint32_t v) {
  Fq a = Fq::zero();
  a.l[0] = v;
  return to_mont(a);
}
inline Fq2 f2_add(const Fq2& a, const Fq2& b) { return Fq2{add(a.c0, b.c0), add(a.c1, b.c1)}; }
inline Fq2 f2_sub(const Fq2& a, const Fq2& b) { return Fq2{sub(a.c0, b.c0), sub(a.c1, b.c1)}; }
inline Fq2 f2_neg(const Fq2& a) { return Fq2{neg(a.c0), neg(a.c1)}; }
inline Fq2 f2_conj(const Fq2& a) { return Fq2{a.c0, neg(a.c1)}; }
inline Fq2 f2_mul(const Fq2& a, const Fq2& b) { return Fq2{sub(mul(a.c0, b.c0), mul(a.c1, b.c1)), add(mul(a.c0, b.c1), mul(a.c1, b.c0))}; }
inline Fq2 f2_sqr(const Fq2& a) { return f2_mul(a, a); }
inline Fq2 f2_inv(const Fq2& a) {  // 0 for 0
  const Fq d = inv(add(sqr(a.c0), sqr(a.c1)));
  return Fq2{mul(a.c0, d), mul(neg(a.c1), d)};
}
inline Fq2 f2_one() { return Fq2{Fq::one(), Fq::zero()}; }
inline Fq2 f2_xi() { return Fq2{fq_small(9), Fq::one()}; }
inline Fq2 f2_pow(const Fq2& a, const uint32_t e[8]) {
  Fq2 r = f2_one();
  for (int i = 7; i >= 0; i--)
    for (int b = 31; b >= 0; b--) {
      r = f2_sqr(r);
      if ((e[i] >> b) & 1) r = f2_mul(r, a);
    }
  return r;
}

// gamma[k-1][i-1] = xi^(i (p^k - 1)/6): from g = xi^((p-1)/6) alone, since x^p is the conjugate in Fq2:
// xi^((p^2-1)/6) = g conj(g) and xi^((p^3-1)/6) = g conj(g) g.
struct Consts {
  Fq2 gamma[3][5];
  Fq2 twist_b;  // 3 / xi
};
inline Consts make_consts() {
  uint32_t e[8];
  uint64_t rem = 0;
  for (int i = 7; i >= 0; i--) {  // (p - 1)/6: p is odd, so p - 1 only clears bit 0
    const uint64_t cur = (rem << 32) | (FqP::p(i) - (i == 0 ? 1u : 0u));
    e[i] = (uint32_t)(cur / 6), rem = cur % 6;
  }
  Consts c;
  const Fq2 g1 = f2_pow(f2_xi(), e), g2 = f2_mul(g1, f2_conj(g1)), g3 = f2_mul(g2, g1);
  const Fq2 base[3] = {g1, g2, g3};
  for (int k = 0; k < 3; k++) {
    c.gamma[k][0] = base[k];
    for (int i = 1; i < 5; i++) c.gamma[k][i] = f2_mul(c.gamma[k][i - 1], base[k]);
  }
  c.twist_b = f2_mul(Fq2{fq_small(3), Fq::zero()}, f2_inv(f2_xi()));
  return c;
}
inline const Consts& consts() {
  static const Consts c = make_consts();
  return c;
}

// ---- G2 on the twist, affine; all-zero is the identity (halo2curves' G2Affine)
struct G2Affine {
  Fq2 x, y;
  bool is_inf() const { return x.is_zero() && y.is_zero(); }
};
inline G2Affine g2_inf() { return G2Affine{Fq2{Fq::zero(), Fq::zero()}, Fq2{Fq::zero(), Fq::zero()}}; }
inline G2Affine g2_generator() {  // EIP-197's
  static const uint64_t w[4][4] = {{0x46debd5cd992f6edull, 0x674322d4f75edaddull, 0x426a00665e5c4479ull, 0x1800deef121f1e76ull},
                                   {0x97e485b7aef312c2ull, 0xf1aa493335a9e712ull, 0x7260bfb731fb5d25ull, 0x198e9393920d483aull},
                                   {0x4ce6cc0166fa7daaull, 0xe3d1e7690c43d37bull, 0x4aab71808dcb408full, 0x12c85ea5db8c6debull},
                                   {0x55acdadcd122975bull, 0xbc4b313370b38ef3ull, 0xec9e99ad690c3395ull, 0x090689d0585ff075ull}};
  Fq c[4];
  for (int i = 0; i < 4; i++) {
    memcpy(c[i].l, w[i], 32);
    c[i] = to_mont(c[i]);
  }
  return G2Affine{Fq2{c[0], c[1]}, Fq2{c[2], c[3]}};
}
inline bool g2_on_twist(const G2Affine& q) { return f2_sqr(q.y) == f2_add(f2_mul(f2_sqr(q.x), q.x), consts().twist_b); }
inline G2Affine g2_neg(const G2Affine& q) { return G2Affine{q.x, f2_neg(q.y)}; }
// The slope of the line through t and q (the tangent when they are equal). The caller has excluded t = -q.
inline Fq2 g2_slope(const G2Affine& t, const G2Affine& q) {
  if (t.x == q.x) {
    const Fq2 xx = f2_sqr(t.x);
    return f2_mul(f2_add(f2_add(xx, xx), xx), f2_inv(f2_add(t.y, t.y)));
  }
  return f2_mul(f2_sub(q.y, t.y), f2_inv(f2_sub(q.x, t.x)));
}
inline G2Affine g2_add_slope(const G2Affine& t, const G2Affine& q, const Fq2& lam) {
  G2Affine r;
  r.x = f2_sub(f2_sub(f2_sqr(lam), t.x), q.x);
  r.y = f2_sub(f2_mul(lam, f2_sub(t.x, r.x)), t.y);
  return r;
}
inline G2Affine g2_add(const G2Affine& a, const G2Affine& b) {
  if (a.is_inf()) return b;
  if (b.is_inf()) return a;
  if (a.x == b.x && (!(a.y == b.y) || a.y.is_zero())) return g2_inf();
  return g2_add_slope(a, b, g2_slope(a, b));
}
// k * q, k a plain 256-bit integer (4 x u64, little-endian)
inline G2Affine g2_mul(const G2Affine& q, const uint64_t k[4]) {
  G2Affine r = g2_inf();
  for (int i = 255; i >= 0; i--) {
    r = g2_add(r, r);
    if ((k[i >> 6] >> (i & 63)) & 1) r = g2_add(r, q);
  }
  return r;
}
inline G2Affine g2_frobenius(const G2Affine& q) {  // pi on the twist: (conj(x) xi^((p-1)/3), conj(y) xi^((p-1)/2))
  return G2Affine{f2_mul(f2_conj(q.x), consts().gamma[0][1]), f2_mul(f2_conj(q.y), consts().gamma[0][2])};
}

// The prepared form of ONE finite point: per line step of the Miller program (miller_program below) the line through the running point T and
// the addend (T itself for a doubling), as (-lambda, lambda x_T - y_T) — the untwisted line at P = (x_P, y_P) is
// y_P + (-lambda x_P) w + (lambda x_T - y_T) v w. Out: 4 * PAIRING_NUM_LINES packed canonical Fq in radix 2^261.
// A point of the order-r subgroup never meets T = +-Q inside the loop; for a point outside it (membership is not checked)
// a degenerate step divides by zero, which inv() maps to 0: the result is then meaningless but nothing faults.
inline void g2_prepare(const G2Affine& q, Fq* lines) {
  G2Affine t = q;
  Fq* out = lines;
  auto step = [&](const G2Affine& addend) {
    const Fq2 lam = g2_slope(t, addend);
    const Fq2 c0 = f2_neg(lam), c1 = f2_sub(f2_mul(lam, t.x), t.y);
    const Fq v[4] = {c0.c0, c0.c1, c1.c0, c1.c1};
    for (int i = 0; i < 4; i++) *out++ = fq29_pack_canonical(fq29_from_r256(v[i]));
    t = g2_add_slope(t, addend, lam);
  };
  for (int b = 63; b >= 0; b--) {
    step(t);
    if ((ATE_LOOP_LOW >> b) & 1) step(q);
  }
  const G2Affine q1 = g2_frobenius(q);
  step(q1);
  step(g2_neg(g2_frobenius(q1)));
}

inline Fq2x to_fq2x(const Fq2& a) { return Fq2x{fq29_from_r256(a.c0), fq29_from_r256(a.c1)}; }

// ---- the constant table of the executor: 0, 1, then gamma_k[i] at K_GAMMA + 5 (k - 1) + (i - 1)
constexpr int K_ZERO = 0, K_ONE = 1, K_GAMMA = 2, K_COUNT = 17;
inline void device_consts(Fq2x out[K_COUNT]) {
  out[K_ZERO] = fq2x_zero();
  out[K_ONE] = fq2x_one();
  for (int k = 0; k < 3; k++)
    for (int i = 0; i < 5; i++) out[K_GAMMA + 5 * k + i] = to_fq2x(consts().gamma[k][i]);
}

// ---- programs. A register is an index into the lane's slab; an Fq6 is three consecutive registers (c0, c1, c2), an Fq12
// six (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2). Temporaries come from a stack allocator (alloc / release), so `regs` is
// the slab a lane needs. Every emitter may be given a destination that aliases an operand. Bounds: every word of
// fq12.cuh's executor takes stored-form operands and leaves a stored-form result, so a program cannot leave the range.
struct Prog {
  std::vector<uint32_t> w;
  int top = 0, regs = 0;
  int alloc(int n) {
    const int r = top;
    top += n;
    if (top > regs) regs = top;
    return r;
  }
  void release(int mark) { top = mark; }
  void op(uint32_t o, int d, int a = 0, int b = 0) { w.push_back(pair_word(o, (uint32_t)d, (uint32_t)a, (uint32_t)b)); }
  void mul(int d, int a, int b) { op(P_MUL, d, a, b); }
  void sqr(int d, int a) { op(P_SQR, d, a); }
  void add(int d, int a, int b) { op(P_ADD, d, a, b); }
  void sub(int d, int a, int b) { op(P_SUB, d, a, b); }
  void neg(int d, int a) { op(P_NEG, d, a); }
  void conj(int d, int a) { op(P_CONJ, d, a); }
  void mulxi(int d, int a) { op(P_MULXI, d, a); }
  void mov(int d, int a) {
    if (d != a) op(P_MOV, d, a);
  }
};

inline void e6_add(Prog& p, int r, int a, int b) { for (int i = 0; i < 3; i++) p.add(r + i, a + i, b + i); }
inline void e6_sub(Prog& p, int r, int a, int b) { for (int i = 0; i < 3; i++) p.sub(r + i, a + i, b + i); }
inline void e6_neg(Prog& p, int r, int a) { for (int i = 0; i < 3; i++) p.neg(r + i, a + i); }
inline void e6_mov(Prog& p, int r, int a) { for (int i = 0; i < 3; i++) p.mov(r + i, a + i); }
// a v: (a0, a1, a2) -> (xi a2, a0, a1)
inline void e6_mul_v(Prog& p, int r, int a) {
  const int m = p.top, t = p.alloc(1);
  p.mulxi(t, a + 2);
  p.mov(r + 2, a + 1);
  p.mov(r + 1, a);
  p.mov(r, t);
  p.release(m);
}
// Karatsuba over Fq2: six products
inline void e6_mul(Prog& p, int r, int a, int b) {
  const int m = p.top, t0 = p.alloc(1), t1 = p.alloc(1), t2 = p.alloc(1), c0 = p.alloc(1), c1 = p.alloc(1), c2 = p.alloc(1), s = p.alloc(1), u = p.alloc(1);
  p.mul(t0, a, b), p.mul(t1, a + 1, b + 1), p.mul(t2, a + 2, b + 2);
  p.add(s, a + 1, a + 2), p.add(u, b + 1, b + 2), p.mul(c0, s, u), p.sub(c0, c0, t1), p.sub(c0, c0, t2), p.mulxi(c0, c0), p.add(c0, c0, t0);
  p.add(s, a, a + 1), p.add(u, b, b + 1), p.mul(c1, s, u), p.sub(c1, c1, t0), p.sub(c1, c1, t1), p.mulxi(s, t2), p.add(c1, c1, s);
  p.add(s, a, a + 2), p.add(u, b, b + 2), p.mul(c2, s, u), p.sub(c2, c2, t0), p.sub(c2, c2, t2), p.add(c2, c2, t1);
  p.mov(r, c0), p.mov(r + 1, c1), p.mov(r + 2, c2);
  p.release(m);
}
// Chung-Hasan SQR2: three squarings and two products
inline void e6_sqr(Prog& p, int r, int a) {
  const int m = p.top, s0 = p.alloc(1), s1 = p.alloc(1), s2 = p.alloc(1), s3 = p.alloc(1), s4 = p.alloc(1), t = p.alloc(1);
  p.sqr(s0, a), p.mul(s1, a, a + 1), p.add(s1, s1, s1);
  p.sub(s2, a, a + 1), p.add(s2, s2, a + 2), p.sqr(s2, s2);
  p.mul(s3, a + 1, a + 2), p.add(s3, s3, s3), p.sqr(s4, a + 2);
  p.mulxi(t, s3), p.add(r, s0, t);        // c0 = s0 + xi s3
  p.add(s2, s2, s1), p.add(s2, s2, s3), p.sub(s2, s2, s0), p.sub(s2, s2, s4);  // c2 = s1 + s2 + s3 - s0 - s4
  p.mulxi(t, s4), p.add(r + 1, s1, t);    // c1 = s1 + xi s4
  p.mov(r + 2, s2);
  p.release(m);
}
// a (b0 + b1 v): the sparse right operand of a line; six products
inline void e6_mul_01(Prog& p, int r, int a, int b0, int b1) {
  const int m = p.top, c0 = p.alloc(1), c1 = p.alloc(1), c2 = p.alloc(1), t = p.alloc(1);
  p.mul(c0, a, b0), p.mul(t, a + 2, b1), p.mulxi(t, t), p.add(c0, c0, t);
  p.mul(c1, a, b1), p.mul(t, a + 1, b0), p.add(c1, c1, t);
  p.mul(c2, a + 1, b1), p.mul(t, a + 2, b0), p.add(c2, c2, t);
  p.mov(r, c0), p.mov(r + 1, c1), p.mov(r + 2, c2);
  p.release(m);
}
// 1/a: A = a0^2 - xi a1 a2, B = xi a2^2 - a0 a1, C = a1^2 - a0 a2, F = a0 A + xi (a2 B + a1 C); (A, B, C)/F, with
// 1/F = conj(F) / (F conj(F)) and the norm's one Fq inversion
inline void e6_inv(Prog& p, int r, int a) {
  const int m = p.top, A = p.alloc(1), B = p.alloc(1), C = p.alloc(1), f = p.alloc(1), t = p.alloc(1);
  p.sqr(A, a), p.mul(t, a + 1, a + 2), p.mulxi(t, t), p.sub(A, A, t);
  p.sqr(B, a + 2), p.mulxi(B, B), p.mul(t, a, a + 1), p.sub(B, B, t);
  p.sqr(C, a + 1), p.mul(t, a, a + 2), p.sub(C, C, t);
  p.mul(f, a + 2, B), p.mul(t, a + 1, C), p.add(f, f, t), p.mulxi(f, f), p.mul(t, a, A), p.add(f, f, t);
  p.conj(t, f), p.mul(f, f, t);      // the norm, in Fq: (f0^2 + f1^2, 0)
  p.op(P_FQINV, f, f);
  p.op(P_MULFQ, t, t, f);            // 1/F
  p.mul(r, A, t), p.mul(r + 1, B, t), p.mul(r + 2, C, t);
  p.release(m);
}

inline void e12_mov(Prog& p, int r, int a) { for (int i = 0; i < 6; i++) p.mov(r + i, a + i); }
inline void e12_one(Prog& p, int r) {
  for (int i = 0; i < 6; i++) p.op(P_MOVK, r + i, 0, i == 0 ? K_ONE : K_ZERO);
}
inline void e12_conj(Prog& p, int r, int a) {  // a^(p^6): the inverse inside the cyclotomic subgroup
  e6_mov(p, r, a);
  e6_neg(p, r + 3, a + 3);
}
// Karatsuba over Fq6: three Fq6 products
inline void e12_mul(Prog& p, int r, int a, int b) {
  const int m = p.top, t0 = p.alloc(3), t1 = p.alloc(3), t2 = p.alloc(3), s = p.alloc(3);
  e6_mul(p, t0, a, b);
  e6_mul(p, t1, a + 3, b + 3);
  e6_add(p, t2, a, a + 3);
  e6_add(p, s, b, b + 3);
  e6_mul(p, t2, t2, s);
  e6_sub(p, t2, t2, t0);
  e6_sub(p, r + 3, t2, t1);
  e6_mul_v(p, t1, t1);
  e6_add(p, r, t0, t1);
  p.release(m);
}
// Complex squaring: (a0 + a1)(a0 + v a1) - a0 a1 - v a0 a1 and 2 a0 a1: two Fq6 products
inline void e12_sqr(Prog& p, int r, int a) {
  const int m = p.top, ab = p.alloc(3), s = p.alloc(3), t = p.alloc(3);
  e6_mul(p, ab, a, a + 3);
  e6_add(p, s, a, a + 3);
  e6_mul_v(p, t, a + 3);
  e6_add(p, t, a, t);
  e6_mul(p, t, s, t);
  e6_sub(p, t, t, ab);
  e6_add(p, r + 3, ab, ab);
  e6_mul_v(p, ab, ab);
  e6_sub(p, r, t, ab);
  p.release(m);
}
// a (l0 + (l3 + l4 v) w) with l0 in Fq (register l0: (l0, 0)): the untwisted line y_P + (-lambda x_P) w +
// (lambda x_T - y_T) v w. Two sparse Fq6 products and one by an Fq.
inline void e12_mul_034(Prog& p, int r, int a, int l0, int l3, int l4) {
  const int m = p.top, t0 = p.alloc(3), t1 = p.alloc(3), t2 = p.alloc(3), l03 = p.alloc(1);
  for (int i = 0; i < 3; i++) p.op(P_MULFQ, t0 + i, a + i, l0);
  e6_mul_01(p, t1, a + 3, l3, l4);
  e6_add(p, t2, a, a + 3);
  p.add(l03, l3, l0);
  e6_mul_01(p, t2, t2, l03, l4);
  e6_sub(p, t2, t2, t0);
  e6_sub(p, r + 3, t2, t1);
  e6_mul_v(p, t1, t1);
  e6_add(p, r, t0, t1);
  p.release(m);
}
// a^(p^k), k = 1..3: the coefficient of w^e (e = i + 2j for c_i.c_j) is conjugated k times and multiplied by gamma_k[e]
inline void e12_frobenius(Prog& p, int r, int a, int k) {
  static const int reg_of_e[6] = {0, 3, 1, 4, 2, 5};  // e -> register offset
  for (int e = 0; e < 6; e++) {
    const int d = r + reg_of_e[e], x = a + reg_of_e[e];
    if (k & 1) p.conj(d, x);
    else p.mov(d, x);
    if (e) p.op(P_MULK, d, d, K_GAMMA + 5 * (k - 1) + (e - 1));
  }
}
// Granger-Scott squaring inside the cyclotomic subgroup: three squarings in Fq4 = Fq2[s]/(s^2 - xi)
inline void e4_sqr(Prog& p, int c0, int c1, int a0, int a1) {  // c0, c1 fresh registers
  const int m = p.top, t0 = p.alloc(1), t1 = p.alloc(1);
  p.sqr(t0, a0), p.sqr(t1, a1);
  p.add(c1, a0, a1), p.sqr(c1, c1), p.sub(c1, c1, t0), p.sub(c1, c1, t1);
  p.mulxi(c0, t1), p.add(c0, c0, t0);
  p.release(m);
}
inline void e12_cyclotomic_sqr(Prog& p, int r, int a) {
  const int m = p.top, o = p.alloc(6), t3 = p.alloc(1), t4 = p.alloc(1), t5 = p.alloc(1), t6 = p.alloc(1);
  auto fin = [&](int dst, int t, int x, bool minus) {  // dst = 2 (t -+ x) + t
    if (minus) p.sub(dst, t, x);
    else p.add(dst, t, x);
    p.add(dst, dst, dst), p.add(dst, dst, t);
  };
  e4_sqr(p, t3, t4, a + 0, a + 4);  // (c0.c0, c1.c1)
  fin(o + 0, t3, a + 0, true);
  fin(o + 4, t4, a + 4, false);
  e4_sqr(p, t3, t4, a + 3, a + 2);  // (c1.c0, c0.c2)
  e4_sqr(p, t5, t6, a + 1, a + 5);  // (c0.c1, c1.c2)
  fin(o + 1, t3, a + 1, true);
  fin(o + 5, t4, a + 5, false);
  p.mulxi(t3, t6);
  fin(o + 3, t3, a + 3, false);
  fin(o + 2, t5, a + 2, true);
  e12_mov(p, r, o);
  p.release(m);
}
// 1/a = (a0 - a1 w)/(a0^2 - v a1^2): one Fq6 inversion, hence one Fq inversion
inline void e12_inv(Prog& p, int r, int a) {
  const int m = p.top, t0 = p.alloc(3), t1 = p.alloc(3);
  e6_sqr(p, t0, a);
  e6_sqr(p, t1, a + 3);
  e6_mul_v(p, t1, t1);
  e6_sub(p, t0, t0, t1);
  e6_inv(p, t0, t0);
  e6_mul(p, t1, a + 3, t0);
  e6_mul(p, r, a, t0);
  e6_neg(p, r + 3, t1);
  p.release(m);
}
// a^u for a in the cyclotomic subgroup: 62 cyclotomic squarings and a product per set bit of u (r must not alias a)
inline void e12_pow_u(Prog& p, int r, int a) {
  e12_mov(p, r, a);
  for (int b = 61; b >= 0; b--) {
    e12_cyclotomic_sqr(p, r, r);
    if ((BN_U >> b) & 1) e12_mul(p, r, r, a);
  }
}

// The Miller program. Registers: XP = (x_P, 0), YP = (y_P, 0) set by the caller; the value f_{6u+2,Q}(P) times the two
// Frobenius lines in F..F+5. Lines are read in g2_prepare's order (P_LINE).
constexpr int MILLER_XP = 0, MILLER_YP = 1, MILLER_F = 2;
inline Prog miller_program() {
  Prog p;
  p.alloc(8);
  const int l = p.alloc(2);
  e12_one(p, MILLER_F);
  auto line = [&]() {
    p.op(P_LINE, l);
    p.op(P_MULFQ, l, l, MILLER_XP);  // (-lambda) x_P
    e12_mul_034(p, MILLER_F, MILLER_F, MILLER_YP, l, l + 1);
  };
  for (int b = 63; b >= 0; b--) {
    if (b != 63) e12_sqr(p, MILLER_F, MILLER_F);  // the first squaring would square one
    line();
    if ((ATE_LOOP_LOW >> b) & 1) line();
  }
  line();
  line();
  return p;
}
// A = A * B on registers 0..5 and 6..11: how the final kernel multiplies a check's Miller values
constexpr int FINAL_A = 0, FINAL_B = 6;
inline Prog mul_program() {
  Prog p;
  p.alloc(12);
  e12_mul(p, FINAL_A, FINAL_A, FINAL_B);
  return p;
}
// A = A^((p^12 - 1)/r). Easy part A^((p^6 - 1)(p^2 + 1)): one inversion. Hard part: y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36
// with y0 = f^p f^(p^2) f^(p^3), y1 = 1/f, y2 = (f^(u^2))^(p^2), y3 = 1/(f^u)^p, y4 = 1/(f^u (f^(u^2))^p), y5 = 1/f^(u^2),
// y6 = 1/(f^(u^3) (f^(u^3))^p) (inverses are conjugates now).
inline Prog final_exp_program() {
  Prog p;
  p.alloc(6);
  const int A = FINAL_A, f = p.alloc(6), t0 = p.alloc(6), t1 = p.alloc(6), fu = p.alloc(6), fu2 = p.alloc(6), fu3 = p.alloc(6), y = p.alloc(6);
  e12_inv(p, t0, A);
  e12_conj(p, t1, A);
  e12_mul(p, t0, t1, t0);           // f^(p^6 - 1)
  e12_frobenius(p, t1, t0, 2);
  e12_mul(p, f, t1, t0);            // ... ^(p^2 + 1)
  e12_pow_u(p, fu, f);
  e12_pow_u(p, fu2, fu);
  e12_pow_u(p, fu3, fu2);
  e12_frobenius(p, y, fu3, 1), e12_mul(p, y, y, fu3), e12_conj(p, y, y);  // y6
  e12_cyclotomic_sqr(p, t0, y);
  e12_frobenius(p, y, fu2, 1), e12_mul(p, y, y, fu), e12_conj(p, y, y);   // y4
  e12_mul(p, t0, t0, y);
  e12_conj(p, y, fu2);              // y5
  e12_mul(p, t0, t0, y);            // t0 = y6^2 y4 y5
  e12_mul(p, t1, y, t0);
  e12_frobenius(p, y, fu, 1), e12_conj(p, y, y);                          // y3
  e12_mul(p, t1, t1, y);            // t1 = y3 y5 t0
  e12_frobenius(p, y, fu2, 2);      // y2
  e12_mul(p, t0, t0, y);
  e12_cyclotomic_sqr(p, t1, t1);
  e12_mul(p, t1, t1, t0);
  e12_cyclotomic_sqr(p, t1, t1);    // t1 = (t1^2 t0)^2
  e12_conj(p, y, f);                // y1
  e12_mul(p, t0, t1, y);
  e12_frobenius(p, y, f, 1), e12_frobenius(p, fu, f, 2), e12_mul(p, y, y, fu), e12_frobenius(p, fu, f, 3), e12_mul(p, y, y, fu);  // y0
  e12_mul(p, t1, t1, y);
  e12_cyclotomic_sqr(p, t0, t0);
  e12_mul(p, A, t0, t1);            // (t1 y1)^2 (t1 y0)
  return p;
}

// G2Affine <-> the 16 words of the C ABI; coordinates must be canonical (checked by the caller with is_canonical on the
// plain integer: Montgomery words of a residue are themselves below q)
inline G2Affine g2_from_words(const uint64_t w[16]) {
  G2Affine q;
  memcpy(q.x.c0.l, w, 32), memcpy(q.x.c1.l, w + 4, 32), memcpy(q.y.c0.l, w + 8, 32), memcpy(q.y.c1.l, w + 12, 32);
  return q;
}
inline void g2_to_words(const G2Affine& q, uint64_t w[16]) {
  memcpy(w, q.x.c0.l, 32), memcpy(w + 4, q.x.c1.l, 32), memcpy(w + 8, q.y.c0.l, 32), memcpy(w + 12, q.y.c1.l, 32);
}

// ---- byte layouts (a braced list is evaluated left to right). The device image of ONE prepared point (pairing.hip, amdzk_g2):
// the executor's constants Fq2x[K_COUNT] at 0, g2_prepare's Fq[4 * PAIRING_NUM_LINES] at `lines`, then the three programs' words
struct ImageLayout {
  size_t lines, miller, mul, fin, bytes;
};
inline ImageLayout image_layout(size_t n_consts, size_t n_lines, size_t miller_len, size_t mul_len, size_t fin_len) {
  WsLayout w;
  w.take(n_consts * sizeof(Fq2x));
  return ImageLayout{w.take(4 * n_lines * sizeof(Fq)), w.take(miller_len * 4), w.take(mul_len * 4), w.take(fin_len * 4), w.bytes()};
}
// The programs as every handle carries them, flattened once per process
struct Programs {
  Prog miller = miller_program(), mul = mul_program(), fin = final_exp_program();
  ImageLayout at = image_layout(K_COUNT, PAIRING_NUM_LINES, miller.w.size(), mul.w.size(), fin.w.size());
  uint32_t final_regs = (uint32_t)(mul.regs > fin.regs ? mul.regs : fin.regs);  // the slab of a lane of the final kernel: it runs mul and fin
};
inline const Programs& programs() {
  static const Programs P;
  return P;
}
// One amdzk_pairing_products call of n checks over m prepared points (ZK_WS_STARTUP), `chunk` checks per launch
constexpr size_t PAIRING_CHUNK_LANES = 16384;  // Miller lanes per launch: bounds the register slabs (about 2 KB a Miller lane, 5 KB a check)
inline size_t pairing_chunk(size_t n, size_t m) { return PAIRING_CHUNK_LANES / m < n ? PAIRING_CHUNK_LANES / m : n; }  // m <= 16: at least 1024
struct CallLayout {
  // [0, miller_slab) goes up from pinned memory: m pointers to the points' lines at 0 (room for AMDZK_PAIRING_MAX_M), then
  size_t g1;           // G1Affine[n * m], check-major
  size_t miller_slab;  // Fq2x[chunk * m][miller_regs]
  size_t final_slab;   // Fq2x[chunk][final_regs]
  size_t gt;           // Fq[n][12] and, without a gap, ...
  size_t is_one;       // uint8_t[n]: [gt, is_one + n) comes down in one copy
  size_t bytes;
};
inline CallLayout call_layout(size_t n, size_t m, size_t chunk, size_t miller_regs, size_t final_regs) {
  WsLayout w;
  w.take(AMDZK_PAIRING_MAX_M * sizeof(void*));
  return CallLayout{w.take(n * m * sizeof(G1Affine)), w.take(chunk * m * miller_regs * sizeof(Fq2x)), w.take(chunk * final_regs * sizeof(Fq2x)),
                    w.take(n * 12 * sizeof(Fq), 1), w.take(ws_round_up(n, 256), 1), w.bytes()};  // is_one starts at no multiple of 256
}

}  // namespace pairing
