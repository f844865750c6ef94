// fp29_quad.cuh — the XYZZ point formulas of fp29.cuh spread over the four lanes of a quad (device only: DPP moves).
// msm.hip includes it for the latency-mode kernels; tests/native/fp29_device_check.hip runs the functions alone on the
// device against tests/fp29_model.py. The caller passes role = lane & 3 and all four lanes of a quad hold the same points.
#ifndef AMDZK_FP29_QUAD_CUH
#define AMDZK_FP29_QUAD_CUH
#include "fp29.cuh"

namespace bn254 {

// ------------------------------------------------------------------ quad-lane point additions (latency mode)
// One XYZZ addition spread over the FOUR lanes of a quad: every lane of the quad holds the same two points (replicated), takes
// one of the (up to) four independent products of each of the formula's four rounds — its operands picked by its position in
// the quad — and the results go round the quad with DPP quad_perm moves, so that all four lanes end with the same sum. 4
// products + selects + broadcasts per lane (~1,300 VALU) instead of 14 products (~3,100): the bucket reduction's chain of ~30
// dependent additions per commitment batch is what a lone proof waits for (a lone wavefront issues a dependent instruction
// every ~6 cycles whatever it is), and instruction-level parallelism inside ONE lane bought nothing (profiles/r04c_*).
// Costs 4 lanes per addition, so only where the chip is empty anyway: amdzk_ctx::msm_latency_mode. Bounds as x29_add
// (y leaves as the sum of two reduced products, below 4p).
template <int J> __device__ __forceinline__ Fq29 quad_bcast(const Fq29& v) {
  Fq29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.l[i], J * 0x55, 0xf, 0xf, false);  // quad_perm:[J,J,J,J]
  return r;
}
__device__ __forceinline__ Fq29 quad_sel(uint32_t role, const Fq29& a0, const Fq29& a1, const Fq29& a2, const Fq29& a3) {
  Fq29 r;
  const bool hi = (role & 2u) != 0, odd = (role & 1u) != 0;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const uint32_t lo2 = odd ? a1.l[i] : a0.l[i], hi2 = odd ? a3.l[i] : a2.l[i];
    r.l[i] = hi ? hi2 : lo2;
  }
  return r;
}
__device__ __forceinline__ G1X29 x29_dbl_quad(const G1X29& p, uint32_t role) {
  if (p.is_inf()) return p;
  const Fq29 u = f29_add(p.y, p.y);                                                   // < 10
  Fq29 res = f29_mul(quad_sel(role, u, p.x, u, p.x), quad_sel(role, u, p.x, u, p.x));  // u^2 (100 p^2) | x^2 (81)
  const Fq29 v = quad_bcast<0>(res), xx = quad_bcast<1>(res);
  const Fq29 m = f29_add(f29_add_lazy(xx, xx), xx);                                   // < 6
  res = f29_mul(quad_sel(role, u, p.x, m, m), quad_sel(role, v, v, m, m));             // w = u v | s = x v | m^2 (36)
  const Fq29 w = quad_bcast<0>(res), sv = quad_bcast<1>(res), mm = quad_bcast<2>(res);
  G1X29 r;
  r.x = f29_sub5(mm, f29_add(sv, sv));                                                // < 7
  const Fq29 d = f29_sub8(sv, r.x);                                                   // < 10
  res = f29_mul(quad_sel(role, m, f29_neg3(w), v, w), quad_sel(role, d, p.y, p.zz, p.zzz));  // m d (60) | (3p - w) y (15) | v zz | w zzz
  r.y = f29_add(quad_bcast<0>(res), quad_bcast<1>(res));                              // < 4
  r.zz = quad_bcast<2>(res);
  r.zzz = quad_bcast<3>(res);
  return r;
}
__device__ __forceinline__ G1X29 x29_add_quad(const G1X29& a, const G1X29& b, uint32_t role) {
  if (b.is_inf()) return a;  // the four lanes hold the same points: every branch is uniform over the quad
  if (a.is_inf()) return b;
  Fq29 res = f29_mul(quad_sel(role, a.x, b.x, a.y, b.y), quad_sel(role, b.zz, a.zz, b.zzz, a.zzz));  // u1 (18 p^2) | u2 | s1 (10) | s2
  const Fq29 u1 = quad_bcast<0>(res), s1 = quad_bcast<2>(res);
  const Fq29 p = f29_sub3(quad_bcast<1>(res), u1);                                    // < 5
  const Fq29 r = f29_sub3(quad_bcast<3>(res), s1);                                    // < 5
  res = f29_mul(quad_sel(role, p, r, a.zz, a.zzz), quad_sel(role, p, r, b.zz, b.zzz));  // pp (25) | rr | zz1 zz2 | zzz1 zzz2
  const Fq29 pp = quad_bcast<0>(res), rr = quad_bcast<1>(res), zz12 = quad_bcast<2>(res), zzz12 = quad_bcast<3>(res);
  if (f29_is_zero_mod_p(pp)) {
    if (f29_is_zero_mod_p(rr)) return x29_dbl_quad(a, role);
    return G1X29::inf();
  }
  res = f29_mul(quad_sel(role, p, u1, zz12, zz12), pp);                               // ppp (10) | q | zz3
  const Fq29 ppp = quad_bcast<0>(res), q = quad_bcast<1>(res);
  G1X29 o;
  o.zz = quad_bcast<2>(res);
  const Fq29 sq = f29_add(ppp, f29_add_lazy(q, q));                                   // < 6
  o.x = f29_sub7(rr, sq);                                                             // < 9
  const Fq29 t = f29_sub10(q, o.x);                                                   // < 12
  res = f29_mul(quad_sel(role, r, f29_neg3(s1), zzz12, zzz12), quad_sel(role, t, ppp, ppp, ppp));  // r t (60) | (3p - s1) ppp (6) | zzz3
  o.y = f29_add(quad_bcast<0>(res), quad_bcast<1>(res));                              // < 4
  o.zzz = quad_bcast<2>(res);
  return o;
}

}  // namespace bn254
#endif
