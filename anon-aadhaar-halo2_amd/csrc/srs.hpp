// The resident form of a ParamsKZG: what srs.hip builds and owns and msm.hip reads. Internal to these two units —
// everyone else holds an amdzk_srs* and goes through the zk_srs_* functions of common.hpp.
#pragma once
#include "common.hpp"

struct amdzk_srs {
  uint32_t k = 0;
  uint32_t c = 0;        // window bits
  uint32_t W = 0;        // windows = ceil(255 / c)
  size_t n = 0;
  // [basis] -> W x n affine points, window-major: T[w][i] = 2^(c*w) * bases[i]. Coordinates are packed
  // canonical integers in Montgomery radix 2^261 (fp29.cuh) — the form the level-1 accumulation kernel
  // multiplies in; (0, 0) is still the identity.
  bn254::G1Affine* table[AMDZK_NUM_BASES] = {nullptr, nullptr, nullptr};
  // [basis] -> the n bases themselves in halo2curves' radix-2^256 form (ParamsKZG::get_g, write, downsize)
  bn254::G1Affine* base[AMDZK_NUM_BASES] = {nullptr, nullptr, nullptr};
  // Slot AMDZK_BASIS_G_LAGRANGE_PREFIX — S_i = g_lagrange[0] + ... + g_lagrange[i] — is derived, never uploaded or stored:
  // zk_srs_ensure_prefix builds it once, under this guard, when the first proving key with permutation columns is made.
  std::mutex prefix_guard;
  double prefix_build_ms = 0;  // what that one build took (host wall clock, kernels included)
};
// device bytes of one basis slot: the window table and the bases
inline size_t srs_basis_bytes(const amdzk_srs* s) { return ((size_t)s->W + 1) * s->n * sizeof(bn254::G1Affine); }

// msm.hip, for srs.hip alone: the width and the radix of a window table are msm.hip's business.
// window bits of a table over 2^k bases (AMDZK_MSM_C)
uint32_t pick_window_bits(uint32_t k);
// table <- the W window multiples of the n points at base (both on the device), radix 2^261; on ctx's stream
int zk_msm_fill_table(amdzk_ctx* ctx, const bn254::G1Affine* base, bn254::G1Affine* table, size_t n, uint32_t c, uint32_t W);
