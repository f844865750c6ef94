// BN254 G1 multi-scalar multiplication for gfx950.
//
// Replaces halo2_proofs::arithmetic::best_multiexp as reached from
// poly::kzg::commitment::ParamsKZG::{commit, commit_lagrange}
// (halo2_proofs 0.2.0 @ v2023_01_20 [UP], /root/reference/Cargo.lock:469-471; SURVEY.md §8(a) a1,a2).
//
// The CPU original is Pippenger per thread-chunk: c = ceil(ln n) bit windows, 256/c+1 segments,
// 2^c-1 buckets per segment, a running-sum fold per segment and c doublings between segments.
// Same mathematics, different shape here, chosen for this chip:
//
//  * The bases of a ParamsKZG never change, and HBM is 288 GB: at upload time every base is expanded
//    into its W window multiples T[w][i] = 2^(c*w) * g[i] (affine, 64 B). A scalar's W signed digits
//    then all fall into ONE bucket set of 2^(c-1) buckets per column — no per-window bucket sets, no
//    doublings, and the bucket fold runs once per column instead of once per window.
//  * Bucket membership comes from a counting sort of (bucket, point-id) pairs (histogram -> scan ->
//    scatter), so accumulation is gather-only and needs no locks.
//  * Accumulation is cut into equal-sized tasks over the sorted list (not one thread per bucket):
//    skewed witness columns (mostly 0/1/small limbs) and uniform scalars load the chip equally.
//    Level 1 adds affine points into XYZZ accumulators (8M+2S per add), levels 2-3 fold the
//    per-task partial sums.
//  * All of this runs on fp29.cuh's 9 x 29-bit limbs in Montgomery radix 2^261 (in-place 64-bit column
//    accumulation, lazy reduction: 1.7x the 32-bit product on this chip). The window tables store that
//    radix, partial sums cross HBM as raw limbs, and only the one result per column is converted back.
//  * The weighted fold sum_b (b+1)*B_b is done without a serial running sum: with b = r + 64*g,
//    sum = sum_r r*C_r + 64*sum_g g*T_g + sum_g T_g where C_r / T_g are plain column / row sums
//    (lane-per-output serial sums: the prover is bound by instruction issue, and a shuffle tree spends six
//    wave-level additions where a lane loop spends one), then three short reductions per column.
//  * Many columns over the same bases (all advice columns of a phase) go through every kernel in
//    one launch: grid.y = column.
//
// No MFMA: this is 254-bit modular integer work (v_mad_u64_u32), and it is bound by VALU instruction issue, not by HBM.
#include <stdlib.h>

#include "fp29.cuh"
#include "fp29_quad.cuh"
#include "srs.hpp"  // the window tables an MSM reads; srs.hip builds and owns them

using namespace bn254;

namespace {

constexpr int MSM_THREADS = 256;

// ------------------------------------------------------------------ window tables
// next[i] = 2^c * prev[i], affine in, affine out (one Fermat inversion per point; upload-time only).
__global__ void table_next_kernel(const G1Affine* prev, G1Affine* next, size_t n, uint32_t c) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G1Affine p = ld_aff(prev + i);
  G1X x = x_dbl_affine(p);
  for (uint32_t k = 1; k < c; k++) x = x_dbl(x);
  st_aff(next + i, x_to_affine(x));
}

// In place: radix-2^256 Montgomery coordinates -> radix-2^261 (one product per coordinate; 0 stays 0).
__global__ void table_to_r261_kernel(G1Affine* t, size_t count) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  G1Affine p = ld_aff(t + i);
  p.x = fq29_pack_canonical(fq29_from_r256(p.x));
  p.y = fq29_pack_canonical(fq29_from_r256(p.y));
  st_aff(t + i, p);
}

// ------------------------------------------------------------------ digits
// Signed base-2^C digits of the canonical scalar: d_w in [-(2^(C-1)-1), 2^(C-1)], sum d_w 2^(Cw) = s.
// f(w, bucket, negative) is called for every non-zero digit; bucket = |d|-1.
template <int C, class Fn>
__device__ __forceinline__ void for_each_digit(const Fr& canon, Fn f) {
  constexpr int W = (255 + C - 1) / C;
  uint32_t carry = 0;
#pragma unroll
  for (int w = 0; w < W; w++) {
    constexpr uint32_t mask = (1u << C) - 1u;
    const int o = C * w, limb = o >> 5, sh = o & 31;
    uint32_t v = 0;
    if (limb < 8) {
      v = canon.l[limb] >> sh;
      if (sh + C > 32 && limb + 1 < 8) v |= canon.l[limb + 1] << (32 - sh);
    }
    v = (v & mask) + carry;
    carry = v > (1u << (C - 1)) ? 1u : 0u;
    uint32_t mag = carry ? ((1u << C) - v) : v;
    if (mag != 0) f((uint32_t)w, mag - 1, carry);
  }
}

struct DigitArgs {
  union {
    const Fr* scalars;           // column 0 (strided form)
    const Fr* const* col_ptrs;   // PTRS: device array of the columns' addresses (zk_msm_dev_xyzz_cols); same slot, same layout
  };
  size_t col_stride;     // elements (strided form only)
  uint32_t len;
  uint32_t nb;           // buckets per column = 2^(C-1)
  uint32_t chunk;        // scalars per workgroup
  uint32_t nblk;         // workgroups per column
  uint32_t* blk_hist;    // [ncols][nblk][nb]: per-workgroup counts, later per-workgroup start offsets
  const uint32_t* off0;  // [ncols][nb+1] bucket offsets (scatter only)
  uint32_t* entries;     // [ncols][ecap] (scatter only)
  size_t ecap;
  uint32_t table_n;      // row length of the window table (2^k)
};

// One workgroup owns `chunk` consecutive scalars of one column. Counting and cursor bumping happen in
// LDS (ds_add / ds_add_rtn), so global memory sees one coalesced histogram write per workgroup
// instead of one atomic per digit.
// BIG: 1024 threads per workgroup instead of 256 — for the few-columns / long-column case (k >= 19: one 2^22-point
// column is 64 workgroups of 256 threads otherwise, a quarter of the chip's SIMDs with one wavefront each, every thread a
// dependent chain of load -> Montgomery reduction -> 16 LDS atomics -> 16 scattered stores: 1.96 + 0.43 ms of the 9.9 ms
// of a 2^22-point MSM, profiles/r04a_*). The counters of a workgroup fill LDS (2^15 buckets = 128 KiB), so a compute unit
// holds one workgroup whatever its size: sixteen wavefronts hide that chain where four do not.
// PTRS: column `col` starts at a.col_ptrs[col] instead of a.scalars + col * a.col_stride — one wave-uniform pointer load per
// workgroup; the strided instantiations are the code they were before the parameter existed.
template <int C, bool SCATTER, bool BIG, bool PTRS>
__global__ __launch_bounds__(BIG ? 1024 : MSM_THREADS) void msm_digit_kernel(DigitArgs a) {
  extern __shared__ uint32_t lds_cnt[];  // nb counters / cursors
  constexpr uint32_t THREADS = BIG ? 1024 : MSM_THREADS;
  const uint32_t col = blockIdx.y, blk = blockIdx.x, t = threadIdx.x;
  uint32_t* gh = a.blk_hist + ((size_t)col * a.nblk + blk) * a.nb;
  if (!SCATTER) {
    for (uint32_t b = t; b < a.nb; b += THREADS) lds_cnt[b] = 0;
  } else {
    const uint32_t* off = a.off0 + (size_t)col * (a.nb + 1);
    for (uint32_t b = t; b < a.nb; b += THREADS) lds_cnt[b] = off[b] + gh[b];
  }
  __syncthreads();
  const uint32_t lo_i = blk * a.chunk, hi_i = min(lo_i + a.chunk, a.len);
  uint32_t* ent = a.entries + (size_t)col * a.ecap;
  const Fr* colp = nullptr;
  if constexpr (PTRS) colp = a.col_ptrs[col];
  for (uint32_t i = lo_i + t; i < hi_i; i += THREADS) {
    const uint4* sp;
    if constexpr (PTRS) sp = reinterpret_cast<const uint4*>(colp + i);
    else sp = reinterpret_cast<const uint4*>(a.scalars + (size_t)col * a.col_stride + i);
    uint4 lo = sp[0], hi = sp[1];
    if ((lo.x | lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w) == 0) continue;
    Fr s;
    s.l[0] = lo.x; s.l[1] = lo.y; s.l[2] = lo.z; s.l[3] = lo.w;
    s.l[4] = hi.x; s.l[5] = hi.y; s.l[6] = hi.z; s.l[7] = hi.w;
    Fr canon = fr29_from_mont(s);  // = to_repr() of the original
    if (!SCATTER) {
      for_each_digit<C>(canon, [&](uint32_t, uint32_t b, uint32_t) { atomicAdd(&lds_cnt[b], 1u); });
    } else {
      for_each_digit<C>(canon, [&](uint32_t w, uint32_t b, uint32_t negv) {
        uint32_t pos = atomicAdd(&lds_cnt[b], 1u);
        ent[pos] = (w * a.table_n + i) | (negv << 31);
      });
    }
  }
  if (!SCATTER) {
    __syncthreads();
    for (uint32_t b = t; b < a.nb; b += THREADS) gh[b] = lds_cnt[b];
  }
}

// The same counting sort for caller-supplied bases (zk_msm_bases_dev_xyzz): no window table, so every window keeps a
// bucket set of its own. grid.y = column * W + window is one VIRTUAL column: the workgroup walks the signed digits of its
// scalars from window 0 (the carry chain decides the digit) and keeps only its window's, as entry `i | neg << 31` — an
// index into the one copy of the bases. Every scalar is converted W times over the two passes: one product each, against
// the W mixed additions of 14 products it feeds.
// A kernel of its own, on purpose: msm_digit_kernel is on every proof's path, and one body shared by both (tried: a
// __device__ template with a per-digit filter) reordered the instructions of the prover's scatter kernels. Kept apart,
// msm_digit_kernel compiles to the instructions it had before this kernel existed; a change to one body is a change to both.
template <int C, bool SCATTER>
__global__ __launch_bounds__(MSM_THREADS) void msm_digit_win_kernel(DigitArgs a) {
  extern __shared__ uint32_t lds_cnt[];  // nb counters / cursors
  constexpr uint32_t W = (255 + C - 1) / C;
  const uint32_t vcol = blockIdx.y, col = vcol / W, win = vcol % W, blk = blockIdx.x, t = threadIdx.x;
  uint32_t* gh = a.blk_hist + ((size_t)vcol * a.nblk + blk) * a.nb;
  if (!SCATTER) {
    for (uint32_t b = t; b < a.nb; b += MSM_THREADS) lds_cnt[b] = 0;
  } else {
    const uint32_t* off = a.off0 + (size_t)vcol * (a.nb + 1);
    for (uint32_t b = t; b < a.nb; b += MSM_THREADS) lds_cnt[b] = off[b] + gh[b];
  }
  __syncthreads();
  const uint32_t lo_i = blk * a.chunk, hi_i = min(lo_i + a.chunk, a.len);
  uint32_t* ent = a.entries + (size_t)vcol * a.ecap;
  for (uint32_t i = lo_i + t; i < hi_i; i += MSM_THREADS) {
    const uint4* sp = reinterpret_cast<const uint4*>(a.scalars + (size_t)col * a.col_stride + i);
    uint4 lo = sp[0], hi = sp[1];
    if ((lo.x | lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w) == 0) continue;
    Fr s;
    s.l[0] = lo.x; s.l[1] = lo.y; s.l[2] = lo.z; s.l[3] = lo.w;
    s.l[4] = hi.x; s.l[5] = hi.y; s.l[6] = hi.z; s.l[7] = hi.w;
    Fr canon = fr29_from_mont(s);
    for_each_digit<C>(canon, [&](uint32_t w, uint32_t b, uint32_t negv) {
      if (w != win) return;
      if (!SCATTER) {
        atomicAdd(&lds_cnt[b], 1u);
      } else {
        uint32_t pos = atomicAdd(&lds_cnt[b], 1u);
        ent[pos] = i | (negv << 31);
      }
    });
  }
  if (!SCATTER) {
    __syncthreads();
    for (uint32_t b = t; b < a.nb; b += MSM_THREADS) gh[b] = lds_cnt[b];
  }
}

// Per bucket: turn the per-workgroup counts into per-workgroup start offsets (relative to the
// bucket's own start) and emit the bucket total.
__global__ __launch_bounds__(256) void msm_blk_offsets_kernel(uint32_t* blk_hist, uint32_t* cnt, uint32_t nb, uint32_t nblk) {
  const uint32_t col = blockIdx.y, b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb) return;
  uint32_t* h = blk_hist + (size_t)col * nblk * nb + b;
  uint32_t run = 0;
  for (uint32_t k = 0; k < nblk; k++) {
    uint32_t v = h[(size_t)k * nb];
    h[(size_t)k * nb] = run;
    run += v;
  }
  cnt[(size_t)col * nb + b] = run;
}

// ------------------------------------------------------------------ scan
// off_out[b] = exclusive prefix sum over b of v[b]; off_out[nb] = total.
//   mode 1: v[b] = src[b]                       (src has nb entries per column)
//   mode 0: v[b] = ceil((src[b+1]-src[b]) / T)   (src has nb+1 entries per column)
//   mode 2: v[b] = number of T-aligned chunks of the whole list that intersect [src[b], src[b+1])
// The source row is first copied into LDS with coalesced loads (thread t takes words t, t + 1024, ...: all of a thread's
// loads in flight at once) — a thread walking its own `per` consecutive words straight from global memory waits for one
// dependent load after the other: 62 us per launch at 2^15 buckets, 15 us staged (profiles/r04a_*). Rows of up to
// SCAN_LDS_WORDS words (buckets + 1) are staged; longer ones are read in place.
constexpr uint32_t SCAN_LDS_WORDS = 32768 + 1;
__global__ __launch_bounds__(1024) void msm_scan_kernel(const uint32_t* src, uint32_t* off_out,
                                                         uint32_t nb, uint32_t T, int src_is_hist) {
  extern __shared__ uint32_t scan_lds[];  // [16] wavefront totals, then the staged row
  uint32_t* wtot = scan_lds;
  const uint32_t col = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint32_t words = src_is_hist == 1 ? nb : nb + 1;
  const uint32_t* s = src + (size_t)col * words;
  if (words <= SCAN_LDS_WORDS) {
    uint32_t* st = scan_lds + 16;
    for (uint32_t i = t; i < words; i += 1024) st[i] = s[i];
    __syncthreads();
    s = st;
  }
  uint32_t* o = off_out + (size_t)col * (nb + 1);
  const uint32_t per = (nb + 1023) / 1024;
  const uint32_t b0 = t * per, b1 = min(b0 + per, nb);
  auto val = [&](uint32_t b) -> uint32_t {
    if (src_is_hist == 1) return s[b];
    if (src_is_hist == 0) return (s[b + 1] - s[b] + T - 1) / T;
    return s[b + 1] > s[b] ? (s[b + 1] - 1) / T - s[b] / T + 1 : 0u;
  };
  uint32_t sum = 0;
  for (uint32_t b = b0; b < b1; b++) sum += val(b);
  // inclusive scan of the 1024 thread sums: shuffles inside a wavefront, the 16 wavefront totals through LDS (two
  // barriers; the Hillis-Steele scan over LDS this replaces took twenty, and the kernel is pure latency: four or five
  // launches of one workgroup per column on the chain of every commitment batch)
  uint32_t inc = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t v = __shfl_up(inc, d, 64);
    if ((int)lane >= d) inc += v;
  }
  if (lane == 63) wtot[wv] = inc;
  __syncthreads();
  if (wv == 0) {
    uint32_t w = lane < 16 ? wtot[lane] : 0u;
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
      const uint32_t v = __shfl_up(w, d, 64);
      if ((int)lane >= d) w += v;
    }
    if (lane < 16) wtot[lane] = w;  // inclusive totals
  }
  __syncthreads();
  uint32_t run = inc - sum + (wv ? wtot[wv - 1] : 0u);
  for (uint32_t b = b0; b < b1; b++) {  // stores do not wait for each other
    o[b] = run;
    run += val(b);
  }
  if (t == 1023) o[nb] = wtot[15];
}

// ------------------------------------------------------------------ accumulation levels
// From the table gather to the last fold everything runs on fp29.cuh's 9 x 29-bit limbs in Montgomery radix
// 2^261. Partial sums cross HBM as raw G1X29 (36 words, 144 B): limbs normalised, values only lazily
// reduced (x < 9p, y < 5p, zz, zzz < 2p) — no conversion or reduction on the way out or in. Only the one
// result per column is converted to the packed radix-2^256 XYZZ that zk_msm_finish and the callers read.
__device__ __forceinline__ G1X29 ld_x29(const G1X29* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint32_t w[36];
#pragma unroll
  for (int i = 0; i < 9; i++) {
    uint4 v = q[i];
    w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
  }
  G1X29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    r.x.l[i] = w[i];
    r.y.l[i] = w[9 + i];
    r.zz.l[i] = w[18 + i];
    r.zzz.l[i] = w[27 + i];
  }
  return r;
}
__device__ __forceinline__ void st_x29(G1X29* p, const G1X29& v) {
  uint32_t w[36];
#pragma unroll
  for (int i = 0; i < 9; i++) {
    w[i] = v.x.l[i];
    w[9 + i] = v.y.l[i];
    w[18 + i] = v.zz.l[i];
    w[27 + i] = v.zzz.l[i];
  }
  uint4* q = reinterpret_cast<uint4*>(p);
#pragma unroll
  for (int i = 0; i < 9; i++) q[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}

struct AccArgs {
  const uint32_t* off_in;   // [ncols][nb+1] offsets of the input list per bucket
  const uint32_t* off_out;  // [ncols][nb+1] task offsets per bucket (ceil(cnt/T))
  uint32_t nb;
  uint32_t T;
  const uint32_t* entries;  // level 1 input
  size_t ecap;
  const G1Affine* table;
  const G1X29* in_list;     // level >= 2 input
  size_t in_cap;
  G1X29* out_list;
  size_t out_cap;
};

// Balanced accumulation level (FIRST: table points by id; otherwise partial sums of the previous
// level): thread t owns entries [t*T, (t+1)*T) of the column's sorted list, whatever
// buckets they belong to, and emits one partial sum per bucket segment it crosses (slot
// off_out[b] + (t - off_in[b]/T)). Every lane of a wavefront performs the same number of additions,
// so skewed witness columns (thousands of tiny buckets next to a few huge ones) no longer leave most
// lanes idle behind the longest task. FIRST is the hot kernel of the whole prover: a mixed addition (madd-2008-s on
// 29-bit limbs) is 6 products, 2 squares and one two-product reduction (y3 = r (q - x3) - y1 ppp, f29_mul2) — 1,539
// multiply-adds — on a window-table point (packed canonical, radix 2^261).
template <bool FIRST>
__global__ __launch_bounds__(MSM_THREADS) void msm_accum_seg_kernel(AccArgs a) {
  const uint32_t col = blockIdx.y;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t* off_in = a.off_in + (size_t)col * (a.nb + 1);
  const uint32_t* off_out = a.off_out + (size_t)col * (a.nb + 1);
  const uint32_t total = off_in[a.nb];
  const uint32_t start = t * a.T;
  if (start >= total) return;
  const uint32_t end = min(start + a.T, total);
  uint32_t lo = 0, hi = a.nb;  // largest b with off_in[b] <= start: the non-empty bucket holding `start`
  while (hi - lo > 1) {
    uint32_t mid = (lo + hi) >> 1;
    if (off_in[mid] <= start) lo = mid; else hi = mid;
  }
  uint32_t b = lo, b_end = off_in[b + 1];
  const uint32_t* ent = FIRST ? a.entries + (size_t)col * a.ecap : nullptr;
  const G1X29* in = FIRST ? nullptr : a.in_list + (size_t)col * a.in_cap;
  G1X29* out = a.out_list + (size_t)col * a.out_cap;
  G1X29 acc = G1X29::inf();
  for (uint32_t e = start; e < end; e++) {
    if (e >= b_end) {  // crossed into the next non-empty bucket: flush
      st_x29(out + off_out[b] + (t - off_in[b] / a.T), acc);
      acc = G1X29::inf();
      do {
        b++;
        b_end = off_in[b + 1];
      } while (e >= b_end);
    }
    if (FIRST) {
      const uint32_t id = ent[e];
      G1Affine p = ld_aff(a.table + (id & 0x7fffffffu));
      const bool p_inf = p.is_inf();
      if (id >> 31) p.y = neg(p.y);  // negating a canonical value does not depend on the Montgomery radix
      acc = x29_add_affine(acc, fq29_unpack(p.x), fq29_unpack(p.y), p_inf);
    } else {
      acc = x29_add(acc, ld_x29(in + e));
    }
  }
  st_x29(out + off_out[b] + (t - off_in[b] / a.T), acc);
}

// ------------------------------------------------------------------ wavefront reductions
__device__ __forceinline__ G1X29 shfl_xor_x29(const G1X29& v, int m) {
  G1X29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    r.x.l[i] = __shfl_xor(v.x.l[i], m, 64);
    r.y.l[i] = __shfl_xor(v.y.l[i], m, 64);
    r.zz.l[i] = __shfl_xor(v.zz.l[i], m, 64);
    r.zzz.l[i] = __shfl_xor(v.zzz.l[i], m, 64);
  }
  return r;
}
// All 64 lanes end with the sum of the 64 inputs.
__device__ __forceinline__ G1X29 wave_sum29(G1X29 v) {
#pragma unroll 1
  for (int m = 32; m >= 1; m >>= 1) v = x29_add(v, shfl_xor_x29(v, m));
  return v;
}
__device__ __forceinline__ G1X29 shfl_down_x29(const G1X29& v, int d) {
  G1X29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    r.x.l[i] = __shfl_down(v.x.l[i], d, 64);
    r.y.l[i] = __shfl_down(v.y.l[i], d, 64);
    r.zz.l[i] = __shfl_down(v.zz.l[i], d, 64);
    r.zzz.l[i] = __shfl_down(v.zzz.l[i], d, 64);
  }
  return r;
}
// Lane l ends with the sum of the inputs of lanes l .. 63 (six shuffle rounds).
__device__ __forceinline__ G1X29 wave_suffix29(G1X29 v, uint32_t lane) {
#pragma unroll 1
  for (int d = 1; d < 64; d <<= 1) {
    const G1X29 o = shfl_down_x29(v, d);
    v = x29_add(v, lane + d < 64 ? o : G1X29::inf());
  }
  return v;
}
// The same over the first `n` lanes only (n a power of two <= 64; the other lanes must hold the identity).
__device__ __forceinline__ G1X29 wave_sum29_n(G1X29 v, int n) {
#pragma unroll 1
  for (int m = n >> 1; m >= 1; m >>= 1) v = x29_add(v, shfl_xor_x29(v, m));
  return v;
}
__device__ __forceinline__ G1X29 wave_suffix29_n(G1X29 v, uint32_t lane, int n) {
#pragma unroll 1
  for (int d = 1; d < n; d <<= 1) {
    const G1X29 o = shfl_down_x29(v, d);
    v = x29_add(v, (int)lane + d < n ? o : G1X29::inf());
  }
  return v;
}
// Final level: one lane per bucket folds whatever is left and writes the dense bucket array. A bucket
// that still holds more than FINAL_SERIAL partial sums (a witness column where one value dominates)
// is finished by the whole wavefront: lanes take strided shares, then a shuffle-tree sum.
constexpr uint32_t FINAL_SERIAL = 6;
__global__ __launch_bounds__(64) void msm_accum_final_kernel(const uint32_t* off_in_all, uint32_t nb, const G1X29* in_list, size_t in_cap,
                                                             G1X29* dense) {
  const uint32_t col = blockIdx.y, lane = threadIdx.x;
  const uint32_t b = blockIdx.x * 64 + lane;  // nb is a multiple of 64
  const uint32_t* off_in = off_in_all + (size_t)col * (nb + 1);
  const G1X29* in = in_list + (size_t)col * in_cap;
  const uint32_t lo = off_in[b], hi = off_in[b + 1];
  const uint32_t serial_end = min(hi, lo + FINAL_SERIAL);
  G1X29 acc = G1X29::inf();
  for (uint32_t e = lo; e < serial_end; e++) acc = x29_add(acc, ld_x29(in + e));
  unsigned long long heavy = __ballot(hi > serial_end);
  while (heavy) {
    const int src = __ffsll((long long)heavy) - 1;
    heavy &= heavy - 1;
    const uint32_t h_lo = __shfl(serial_end, src, 64), h_hi = __shfl(hi, src, 64);
    G1X29 part = G1X29::inf();
    for (uint32_t e = h_lo + lane; e < h_hi; e += 64) part = x29_add(part, ld_x29(in + e));
    part = wave_sum29(part);
    if ((int)lane == src) acc = x29_add(acc, part);
  }
  st_x29(dense + (size_t)col * nb + b, acc);
}

// rows[col][g] = sum_r dense[col][64g + r],  cols[col][r] = sum_g dense[col][64g + r].
// Lane-parallel serial sums, no shuffles: the prover is bound by instruction issue, and a 64-lane shuffle tree
// spends 6 wave-level point additions to add 64 values that a lane-per-output loop adds in 63 for all 64
// outputs at once. One workgroup of ROWCOL_WAVES wavefronts per "unit": unit 0 computes the 64 column sums (lane = r,
// each wavefront 1 / ROWCOL_WAVES of the g range), unit u >= 1 the row sums of g in [64(u-1), 64u) (lane = g, each
// wavefront 64 / ROWCOL_WAVES of the 64 r); the partial results meet in LDS, pairwise. The kernel is a handful of
// workgroups per column and pure latency — a point addition is ~6.5 us of dependent products — and it sits on the
// transcript's chain at the end of every commitment batch, so what counts is its DEPTH: 8 + 3 additions with eight
// wavefronts (round 3) against 16 + 3 with four.
constexpr uint32_t ROWCOL_WAVES = 8;
// Units [0, U) with U = ceil(G / 64): the column sums over the row groups g in [64 u, 64 u + 64) (lane = r; cols[col][u][r] —
// msm_fold adds the U slices: one slice up to k = 18, eight at k = 22, where ONE unit summing all 512 row groups was a
// chain of 64 + 3 additions, 0.7 ms of a 2^22-point MSM); units [U, 2U): the row sums of g in [64 (unit - U), ...) (lane = g).
__global__ __launch_bounds__(64 * ROWCOL_WAVES) void msm_rowcol_kernel(const G1X29* dense, uint32_t nb, G1X29* rows, G1X29* cols) {
  __shared__ G1X29 part[ROWCOL_WAVES / 2][64];
  const uint32_t col = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t G = nb >> 6, U = (G + 63) >> 6;
  const bool col_unit = blockIdx.x < U;
  const uint32_t unit = col_unit ? blockIdx.x : blockIdx.x - U;
  const G1X29* d = dense + (size_t)col * nb;
  const uint32_t g_row = unit * 64 + lane;  // row units only
  constexpr uint32_t per = 64 / ROWCOL_WAVES;
  G1X29 acc = G1X29::inf();
  if (col_unit) {
    const uint32_t g0 = unit * 64 + per * wv, g1 = min(G, g0 + per);
    for (uint32_t g = g0; g < g1; g++) acc = x29_add(acc, ld_x29(d + 64 * g + lane));
  } else if (g_row < G) {
    for (uint32_t r = per * wv; r < per * wv + per; r++) acc = x29_add(acc, ld_x29(d + 64 * g_row + r));
  }
  for (uint32_t half = ROWCOL_WAVES / 2; half >= 1; half >>= 1) {  // waves [half, 2 half) hand their sums to waves [0, half)
    if (wv >= half && wv < 2 * half) part[wv - half][lane] = acc;
    __syncthreads();
    if (wv < half) acc = x29_add(acc, part[wv][lane]);
    __syncthreads();
  }
  if (wv == 0) {
    if (col_unit) st_x29(cols + ((size_t)col * U + unit) * 64 + lane, acc);
    else if (g_row < G) st_x29(rows + (size_t)col * G + g_row, acc);
  }
}

// The same sums as shuffle trees (latency mode): one wavefront per output GROUP — workgroup (u, j) of 64 lanes loads the 64
// buckets of row group g = 64 u' + j (row units) or, transposed, the 64 row groups' buckets of residue r = j (column
// units), and adds them in six shuffle rounds: depth 6 instead of 8 + 3, at 4.4 x the additions (128 wavefronts x 6 per
// 64 x 64 block instead of 16 x 11). Same slots, same values as group elements.
__global__ __launch_bounds__(64) void msm_rowcol_tree_kernel(const G1X29* dense, uint32_t nb, G1X29* rows, G1X29* cols) {
  const uint32_t col = blockIdx.z, lane = threadIdx.x, j = blockIdx.x;
  const uint32_t G = nb >> 6, U = (G + 63) >> 6;
  const bool col_unit = blockIdx.y < U;
  const uint32_t unit = col_unit ? blockIdx.y : blockIdx.y - U;
  const G1X29* d = dense + (size_t)col * nb;
  G1X29 v = G1X29::inf();
  if (col_unit) {  // residue r = j, row groups 64 unit + lane
    const uint32_t g = unit * 64 + lane;
    if (g < G) v = ld_x29(d + 64 * g + j);
  } else {  // row group g = 64 unit + j, residues r = lane
    const uint32_t g = unit * 64 + j;
    if (g < G) v = ld_x29(d + 64 * g + lane);
  }
  v = wave_sum29(v);
  if (lane == 0) {
    if (col_unit) st_x29(cols + ((size_t)col * U + unit) * 64 + j, v);
    else if (unit * 64 + j < G) st_x29(rows + (size_t)col * G + unit * 64 + j, v);
  }
}

// ------------------------------------------------------------------ quad-lane point additions (latency mode)
// x29_dbl_quad / x29_add_quad: fp29_quad.cuh.
// A point in LDS as 36 consecutive words; all four lanes of a quad read the same words (a broadcast read).
__device__ __forceinline__ G1X29 lds_ld_x29(const uint32_t* p) {
  G1X29 r;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    r.x.l[i] = p[i];
    r.y.l[i] = p[9 + i];
    r.zz.l[i] = p[18 + i];
    r.zzz.l[i] = p[27 + i];
  }
  return r;
}
__device__ __forceinline__ void lds_st_x29(uint32_t* p, const G1X29& v, uint32_t role) {  // each lane of the quad stores one coordinate
  const Fq29 c = quad_sel(role, v.x, v.y, v.zz, v.zzz);
#pragma unroll
  for (int i = 0; i < 9; i++) p[role * 9 + i] = c.l[i];
}

// A folding level (msm_accum_seg_kernel<false>) with quad additions: quad t owns partial sums [t * T, (t + 1) * T) of the column's
// list; the four lanes load the same sums, add them together, and lane 0 of the quad stores. Same slots, same values.
__global__ __launch_bounds__(MSM_THREADS) void msm_accum_fold_quad_kernel(AccArgs a) {
  const uint32_t col = blockIdx.y;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x, t = gtid >> 2, role = gtid & 3u;
  const uint32_t* off_in = a.off_in + (size_t)col * (a.nb + 1);
  const uint32_t* off_out = a.off_out + (size_t)col * (a.nb + 1);
  const uint32_t total = off_in[a.nb];
  const uint32_t start = t * a.T;
  if (start >= total) return;
  const uint32_t end = min(start + a.T, total);
  uint32_t lo = 0, hi = a.nb;
  while (hi - lo > 1) {
    uint32_t mid = (lo + hi) >> 1;
    if (off_in[mid] <= start) lo = mid; else hi = mid;
  }
  uint32_t b = lo, b_end = off_in[b + 1];
  const G1X29* in = a.in_list + (size_t)col * a.in_cap;
  G1X29* out = a.out_list + (size_t)col * a.out_cap;
  G1X29 acc = G1X29::inf();
  for (uint32_t e = start; e < end; e++) {
    if (e >= b_end) {
      if (role == 0) st_x29(out + off_out[b] + (t - off_in[b] / a.T), acc);
      acc = G1X29::inf();
      do {
        b++;
        b_end = off_in[b + 1];
      } while (e >= b_end);
    }
    acc = x29_add_quad(acc, ld_x29(in + e), role);
  }
  if (role == 0) st_x29(out + off_out[b] + (t - off_in[b] / a.T), acc);
}

// Row / column sums with quad additions: one workgroup of 64 quads per OUTPUT (a row group's 64 residues, or a residue's 64 row
// groups): the 64 points meet pairwise through LDS in six rounds. grid = (64 outputs, 2 units, columns); nb <= 4096 (G <= 64).
__global__ __launch_bounds__(256) void msm_rowcol_quad_kernel(const G1X29* dense, uint32_t nb, G1X29* rows, G1X29* cols) {
  __shared__ uint32_t pts[64 * 36];
  const uint32_t col = blockIdx.z, j = blockIdx.x, quad = threadIdx.x >> 2, role = threadIdx.x & 3u;
  const uint32_t G = nb >> 6;
  const bool col_unit = blockIdx.y == 0;
  const G1X29* d = dense + (size_t)col * nb;
  if (!col_unit && j >= G) return;
  // column unit: residue r = j, this quad's row group g = quad; row unit: row group g = j, this quad's residue r = quad
  const uint32_t g = col_unit ? quad : j, r_ = col_unit ? j : quad;
  G1X29 v = g < G ? ld_x29(d + 64 * g + r_) : G1X29::inf();
  for (uint32_t s = 32; s >= 1; s >>= 1) {
    if (quad >= s && quad < 2 * s) lds_st_x29(pts + (quad - s) * 36, v, role);
    __syncthreads();
    if (quad < s) v = x29_add_quad(v, lds_ld_x29(pts + quad * 36), role);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (col_unit) st_x29(cols + (size_t)col * 64 + j, v);
    else st_x29(rows + (size_t)col * G + j, v);
  }
}

// msm_fold for nb <= 4096 with quad additions: quads [0, 64) hold the row sums T_g, quads [64, 128) the column sums C_r; suffix
// sums by six shift-and-add rounds through LDS (two buffers per vector), their sum by six halving rounds, then quad 0:
// out = 64 * sum_g g T_g + sum_g T_g + sum_r r C_r.
__global__ __launch_bounds__(512) void msm_fold_quad_kernel(const G1X29* rows, const G1X29* cols, uint32_t nb, G1X* out) {
  __shared__ uint32_t buf[2][2][64 * 36];  // [vector][ping-pong][point]
  __shared__ uint32_t keep[3 * 36];        // sum_g T_g, sum_g g T_g, sum_r r C_r
  const uint32_t col = blockIdx.x, quad = threadIdx.x >> 2, role = threadIdx.x & 3u, vec = quad >> 6, l = quad & 63u;
  const uint32_t G = nb >> 6;
  G1X29 v = vec == 0 ? (l < G ? ld_x29(rows + (size_t)col * G + l) : G1X29::inf()) : ld_x29(cols + (size_t)col * 64 + l);
  int cur = 0;
  lds_st_x29(buf[vec][cur] + l * 36, v, role);
  __syncthreads();
  for (uint32_t dd = 1; dd < 64; dd <<= 1) {  // v_l <- v_l + v_{l + dd}: after six rounds the suffix sums S_l
    if (l + dd < 64) v = x29_add_quad(v, lds_ld_x29(buf[vec][cur] + (l + dd) * 36), role);
    cur ^= 1;
    lds_st_x29(buf[vec][cur] + l * 36, v, role);
    __syncthreads();
  }
  if (vec == 0 && l == 0) lds_st_x29(keep, v, role);  // S_0 of the rows = sum_g T_g
  if (l == 0) v = G1X29::inf();                        // the weighted sum is S_1 + ... + S_63
  for (uint32_t s = 32; s >= 1; s >>= 1) {
    __syncthreads();
    if (l >= s && l < 2 * s) lds_st_x29(buf[vec][cur] + (l - s) * 36, v, role);
    __syncthreads();
    if (l < s) v = x29_add_quad(v, lds_ld_x29(buf[vec][cur] + l * 36), role);
  }
  if (l == 0) lds_st_x29(keep + (1 + vec) * 36, v, role);
  __syncthreads();
  if (quad == 0) {
    G1X29 acc = lds_ld_x29(keep + 36);
#pragma unroll 1
    for (int i = 0; i < 6; i++) acc = x29_dbl_quad(acc, role);
    acc = x29_add_quad(acc, lds_ld_x29(keep), role);
    acc = x29_add_quad(acc, lds_ld_x29(keep + 72), role);
    if (role == 0) st_x(out + col, x29_to_r256(acc));
  }
}

// out[col] = sum_r r*cols[r] + sum_g (64g+1)*rows[g]
//          = sum_r r*cols[r] + 64 * (sum_g g*rows[g]) + sum_g rows[g].
// A weighted sum sum_l l * v_l over the 64 lanes of a wavefront is the sum of the suffix sums S_1 .. S_63 (S_l = v_l + ... +
// v_63): six shuffle rounds for the suffixes, six for their sum — 12 dependent point additions where the per-lane 6-bit
// double-and-add followed by a shuffle tree took 18 — and S_0, the plain sum, comes with it (round 3). One wavefront per 64
// row sums (W = ceil(G / 64) of them; g = 64 w + l gives sum_g g v_g = sum_w (A_w + 64 w B_w), A_w the wavefront's
// weighted sum and B_w its plain sum) and one for the 64 column sums; lane 0 of the first wavefront combines them by
// Horner (6 doublings per factor 64). The kernel is pure latency, one workgroup per column, at the end of every
// commitment batch. The result leaves in the packed radix-2^256 XYZZ form (x29_to_r256): the only radix conversion of
// the whole MSM.
// MAXW: the most row-sum wavefronts a workgroup may have (1 up to 2^12 buckets, i.e. every proof-sized MSM: two wavefronts,
// the whole register file each; 8 for the window widths of k >= 19).
template <int MAXW>
__global__ __launch_bounds__(64 * (MAXW + 1)) void msm_fold_kernel(const G1X29* rows, const G1X29* cols, uint32_t nb, G1X* out) {
  __shared__ G1X29 partA[8], partB[8], partC;
  const uint32_t col = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint32_t G = nb >> 6, W = (G + 63) >> 6;
  if (wv <= W) {
    G1X29 v;
    if (wv < W) {
      const uint32_t g = wv * 64 + lane;
      v = g < G ? ld_x29(rows + (size_t)col * G + g) : G1X29::inf();
    } else {
      v = ld_x29(cols + (size_t)col * W * 64 + lane);  // the W slices of the column sums (msm_rowcol)
      for (uint32_t u = 1; u < W; u++) v = x29_add(v, ld_x29(cols + ((size_t)col * W + u) * 64 + lane));
    }
    const G1X29 suf = wave_suffix29(v, lane);
    if (lane == 0 && wv < W) partB[wv] = suf;
    const G1X29 wsum = wave_sum29(lane == 0 ? G1X29::inf() : suf);
    if (lane == 0) {
      if (wv < W) partA[wv] = wsum;
      else partC = wsum;
    }
  }
  __syncthreads();
  if (wv == 0) {
    G1X29 acc;
    if (W > 1) {
      // wavefront 0, lanes w < W (<= 8): Y = sum_w w B_w = the sum of the suffix sums of B over w = 1 .. W - 1, sum_w B_w (the
      // suffix sum of lane 0, parked in partB[0]) and sum_w A_w — three shuffle rounds each instead of lane 0 walking the
      // W values three times. One point live at a time beside the running one: the kernel may hold 168 registers.
      G1X29 y;
      {
        const G1X29 sufb = wave_suffix29_n(lane < W ? partB[lane] : G1X29::inf(), lane, 8);
        if (lane == 0) partB[0] = sufb;  // lane 0 alone reads it back below
        y = wave_sum29_n(lane == 0 || lane >= W ? G1X29::inf() : sufb, 8);
      }
#pragma unroll 1
      for (int i = 0; i < 6; i++) y = x29_dbl(y);
      acc = x29_add(wave_sum29_n(lane < W ? partA[lane] : G1X29::inf(), 8), y);
    } else {
      acc = partA[0];
    }
    if (t == 0) {
#pragma unroll 1
      for (int i = 0; i < 6; i++) acc = x29_dbl(acc);
      acc = x29_add(acc, partB[0]);
      st_x(out + col, x29_to_r256(x29_add(acc, partC)));
    }
  }
}

template <bool SCATTER, bool PTRS>
int launch_digits(amdzk_ctx* ctx, uint32_t c, const DigitArgs& a, dim3 grid, bool big) {
  const size_t shmem = (size_t)a.nb * sizeof(uint32_t);
  const char* nm = SCATTER ? "msm_scatter" : "msm_hist";
  switch (c) {
#define ZK_CASE_T(CC, BIG)                                         \
  {                                                                \
    auto kfn = msm_digit_kernel<CC, SCATTER, BIG, PTRS>;           \
    if (shmem > 65536) ZK_HIP(ctx, hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem)); \
    ZK_LAUNCH(ctx, nm, kfn, grid, dim3(BIG ? 1024 : MSM_THREADS), shmem, a); \
  }
#define ZK_CASE(CC) \
  case CC:          \
    ZK_CASE_T(CC, false) break;
#define ZK_CASE2(CC)               \
  case CC:                         \
    if (big) ZK_CASE_T(CC, true)   \
    else ZK_CASE_T(CC, false)      \
    break;
    ZK_CASE(8) ZK_CASE(9) ZK_CASE(10) ZK_CASE(11) ZK_CASE(12) ZK_CASE(13) ZK_CASE2(14) ZK_CASE2(15) ZK_CASE2(16)
#undef ZK_CASE
#undef ZK_CASE2
#undef ZK_CASE_T
    default:
      ZK_FAIL(ctx, AMDZK_E_INVALID, "msm: window bits %u unsupported", c);
  }
  return AMDZK_OK;
}

template <bool SCATTER>
int launch_digits_win(amdzk_ctx* ctx, uint32_t c, const DigitArgs& a, dim3 grid) {
  const size_t shmem = (size_t)a.nb * sizeof(uint32_t);
  const char* nm = SCATTER ? "msm_scatter_win" : "msm_hist_win";
  switch (c) {
#define ZK_CASE(CC)                                                                                                                \
  case CC: {                                                                                                                       \
    auto kfn = msm_digit_win_kernel<CC, SCATTER>;                                                                                  \
    if (shmem > 65536) ZK_HIP(ctx, hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem)); \
    ZK_LAUNCH(ctx, nm, kfn, grid, dim3(MSM_THREADS), shmem, a);                                                                    \
  } break;
    ZK_CASE(8) ZK_CASE(9) ZK_CASE(10) ZK_CASE(11) ZK_CASE(12) ZK_CASE(13) ZK_CASE(14) ZK_CASE(15) ZK_CASE(16)
#undef ZK_CASE
    default:
      ZK_FAIL(ctx, AMDZK_E_INVALID, "msm: window bits %u unsupported", c);
  }
  return AMDZK_OK;
}

// Caller-supplied bases: out[col] = sum_w 2^(c w) win[col][w], Horner from the top window down — c doublings and one
// addition per window, about 255 dependent doublings per column that no layout removes. One QUAD per column
// (x29_dbl_quad / x29_add_quad: a lone wavefront issues a dependent instruction every few cycles whatever it is, and the
// quad forms are 0.4 x the instructions per lane); the kernel is a handful of wavefronts and pure latency. The window
// sums arrive as msm_fold left them (packed radix 2^256) and the result leaves in the same form for zk_msm_finish.
__global__ __launch_bounds__(64) void msm_window_combine_kernel(const G1X* win, uint32_t W, uint32_t c, uint32_t ncols, G1X* out) {
  const uint32_t gtid = blockIdx.x * 64 + threadIdx.x, col = gtid >> 2, role = gtid & 3u;
  if (col >= ncols) return;  // whole quads leave together
  G1X29 acc = G1X29::inf();
#pragma unroll 1
  for (int w = (int)W - 1; w >= 0; w--) {
#pragma unroll 1
    for (uint32_t i = 0; i < c; i++) acc = x29_dbl_quad(acc, role);  // the identity stays the identity
    const G1X s = ld_x(win + (size_t)col * W + w);
    G1X29 v = G1X29::inf();
    if (!s.is_inf()) {
      v.x = fq29_from_r256(s.x);
      v.y = fq29_from_r256(s.y);
      v.zz = fq29_from_r256(s.zz);
      v.zzz = fq29_from_r256(s.zzz);
    }
    acc = x29_add_quad(acc, v, role);
  }
  if (role == 0) st_x(out + col, x29_to_r256(acc));
}

}  // namespace

// ---------------------------------------------------------------------------------- host side
// What srs.hip needs to give a basis slot its window table (srs.hpp): the width, and the table itself.
uint32_t pick_window_bits(uint32_t k) {
  const char* e = getenv("AMDZK_MSM_C");
  if (e) {
    int v = atoi(e);
    if (v >= 8 && v <= 16) return (uint32_t)v;
  }
  if (k <= 10) return 8;
  if (k <= 12) return 10;
  if (k <= 13) return 11;
  if (k <= 14) return 12;
  // k = 17, 18: 13 and 14 prove at the same rate, 13 with a 3.5 ms shorter proof (fewer buckets to fold per column:
  // profiles/r02j_msm_window_sweep.txt)
  if (k <= 18) return 13;
  if (k <= 20) return 15;
  return 16;
}

// table <- the W window multiples of the n points at base (both on the device), radix 2^261; on ctx's stream
int zk_msm_fill_table(amdzk_ctx* ctx, const G1Affine* base, G1Affine* table, size_t n, uint32_t c, uint32_t W) {
  ZK_HIP(ctx, hipMemcpyAsync(table, base, n * sizeof(G1Affine), hipMemcpyDeviceToDevice, ctx->stream));
  dim3 grid((unsigned)((n + 255) / 256)), block(256);
  for (uint32_t w = 1; w < W; w++)
    ZK_LAUNCH(ctx, "msm_table_next", table_next_kernel, grid, block, 0, table + (size_t)(w - 1) * n, table + (size_t)w * n, n, c);
  const size_t count = (size_t)W * n;  // all windows are built: switch the whole table to radix 2^261
  ZK_LAUNCH(ctx, "msm_table_to_r261", table_to_r261_kernel, dim3((unsigned)((count + 255) / 256)), block, 0, table, count);
  return AMDZK_OK;
}

// Geometry of one batch (msm_group): counting sort, level-1 accumulation, folds, bucket reduction.
struct MsmGeom {
  uint32_t c, W, nb, T1, TL, chunk, nblk;
  bool latency;  // latency mode for this batch: amdzk_ctx::msm_latency_mode and a batch of a few columns
  bool big_digits;  // counting sort with 1024-thread workgroups, up to 256 of them per column
  size_t ecap, cap[4], G;
  size_t o_bh, o_cnt, o_off[4], o_ent, o_list[4], o_dense, o_rows, o_cols, bytes;
};
// Accumulation levels in front of the per-bucket final: level 1 + two folding levels. ONE fold (with TL = max(6, partial
// sums per bucket / 4)) was measured in round 4 and is a trap: the AVERAGE bucket of a proof-sized MSM then reaches the
// final kernel with ~5 partial sums, but witness columns are skewed — a few hundred buckets per column hold hundreds — and
// every such bucket takes the whole wavefront of its 64 neighbours through the cooperative path: msm_accum_final
// 0.76 -> 8.9 ms per proof, 79.6 -> 72 proofs/s (profiles/r04d_one_fold_level_ab.txt).
static constexpr int MSM_NLEV = 3;

// per_window = false: the window-table form (amdzk_srs) — a scalar's W digits all land in ONE bucket set per column.
// per_window = true: caller-supplied bases (zk_msm_bases_dev_xyzz) — `ncols` counts VIRTUAL columns (column, window), each
// with one digit per scalar and a bucket set of its own.
static MsmGeom msm_geometry_cw(uint32_t c, uint32_t W, bool per_window, size_t ncols, size_t len, bool latency_mode) {
  MsmGeom g;
  const size_t dps = per_window ? 1 : W;  // digits per scalar and (virtual) column
  // latency mode applies to batches of a few columns only (the h pieces, the multiopen argument's two, the random polynomial:
  // the chip is empty behind them); the bucket reduction of a 141-column batch is 2,000 wavefronts and throughput-bound —
  // spending 4 lanes per addition there made a lone proof 0.4 ms SLOWER (profiles/r04h_*)
  static const size_t latency_cols = getenv("AMDZK_LATENCY_COLS") && atoi(getenv("AMDZK_LATENCY_COLS")) > 0 ? (size_t)atoi(getenv("AMDZK_LATENCY_COLS")) : 8;
  g.latency = latency_mode && ncols <= latency_cols;
  g.c = c;
  g.W = W;
  g.nb = 1u << (g.c - 1);
  g.ecap = ws_round_up(len * dps ? len * dps : 1, 4);
  // task sizes: level 1 adds T1 table points per thread, levels 2.. fold TL partial sums per thread;
  // all levels use the balanced segmented kernel. Every extra folding level costs a latency-bound launch, so two
  // folding levels; T1 = 12 for the large batches (profiles/r02j_msm_task_size.txt: T1 = 8 / 12 / 16 / 32 / 48 take
  // 5.8 / 5.7 / 6.5 / 7.1 / 7.8 ms per proof in level 1 against 2.4 / 2.1 / 1.9 / 1.6 / 1.6 in the folds — a task of 32
  // additions leaves the last of its few thousand wavefronts running alone — and 76.9 against 76.0 proofs/s for
  // 12 against 16 with ten proofs in flight). e_total is a capacity: zero digits never become entries.
  const size_t e_total = g.ecap * ncols;
  g.T1 = 4;
  if (e_total > (size_t)4 * 262144) g.T1 = 8;
  if (e_total > (size_t)8 * 262144) g.T1 = 12;
  // one long column (k >= 19): tens of millions of entries keep the chip full whatever the task size, and every partial
  // sum a task leaves behind is one more addition in the folds (profiles/r04a_*: 2^22 points, T1 = 12 / 24 / 32 / 48 / 64: 7.48 / 7.44 / 7.36 / 7.32 / 7.28 ms)
  const size_t col_digits = ws_round_up(len * W ? len * W : 1, 4);  // of one column over all its windows (= ecap with a window table)
  if (col_digits >= ((size_t)1 << 23)) g.T1 = col_digits >= ((size_t)1 << 25) ? 64 : 32;  // 2^19 points: 1.53 ms with 32, 1.69 with 64; 2^22: 7.33 / 7.14
  if (const char* e = getenv("AMDZK_MSM_T1")) g.T1 = (uint32_t)atoi(e) > 0 ? (uint32_t)atoi(e) : g.T1;
  g.TL = 6;  // 4 / 6 / 8 / 12 / 16 prove at the same rate (76.7-78.0 proofs/s); 6 has the shortest proof (profiles/r02j_msm_task_size.txt)
  {
    // ... unless the FULLEST buckets of a uniform column would then reach the per-bucket final with more than FINAL_SERIAL partial
    // sums. The top window of a 254-bit scalar has few digits — (r >> c (W - 1)) + 1 of them: 97 at c = 13 — so those buckets
    // hold len / 97 entries on top of the average len W / nb, they are neighbours (one wavefront of msm_accum_final), and each
    // takes that wavefront through the cooperative path in turn: at 2^18 points (3,983 entries in each of them) the final
    // kernel was 1.48 ms of a 2.33 ms MSM and 10.4 ms of the k = 18 proof (profiles/r04x_k18_top_window_buckets.txt). Two
    // folds of TL must bring the fullest bucket's T1-sums down to ~4: TL = 7 at 2^17, 9 at 2^18; 6 up to 2^16 and for c >= 15.
    const unsigned top_shift = g.c * (g.W - 1);
    const uint64_t r_top = 0x30644e72e131a029ULL;  // the scalar field's modulus, bits 192..255 (contract.sol:211)
    const double top_digits = top_shift >= 192 && top_shift < 256 ? (double)((r_top >> (top_shift - 192)) + 1) : (double)g.nb;
    const double fullest = (double)len * dps / g.nb + (double)len / std::min<double>(top_digits, (double)g.nb);
    if (top_digits >= 8)  // two or four such buckets (c = 11, 12) cost 40 us each in the final: not worth wider folds
      while (g.TL < 16 && fullest / g.T1 / ((double)g.TL * g.TL) > 4.5) g.TL++;
  }
  if (const char* e = getenv("AMDZK_MSM_TL")) g.TL = (uint32_t)atoi(e) > 1 ? (uint32_t)atoi(e) : g.TL;
  g.cap[0] = g.ecap;
  g.cap[1] = g.ecap / g.T1 + g.nb + 1;
  for (int l = 2; l <= MSM_NLEV; l++) g.cap[l] = g.cap[l - 1] / g.TL + g.nb + 1;
  // counting-sort geometry: one workgroup per `chunk` scalars, at most 64 workgroups per column — 256 workgroups of 1024
  // threads when the batch is a few long columns (msm_digit_kernel<.., BIG>: window widths 14-16 only)
  g.big_digits = g.c >= 14 && len >= ((size_t)1 << 18) && ncols * ((len + 65535) / 65536) < 256;
  if (const char* e = getenv("AMDZK_MSM_BIG_DIGITS")) g.big_digits = g.c >= 14 && atoi(e) != 0;
  if (per_window) g.big_digits = false;  // msm_digit_win_kernel: 256 threads; a batch of W virtual columns is workgroups enough
  const size_t maxblk = g.big_digits ? 256 : 64;
  g.chunk = g.big_digits ? 4096 : 2048;
  while ((len + g.chunk - 1) / g.chunk > maxblk) g.chunk <<= 1;
  g.nblk = len ? (uint32_t)((len + g.chunk - 1) / g.chunk) : 1;
  WsLayout w;
  g.o_bh = w.take(ncols * (size_t)g.nblk * g.nb * 4);
  g.o_cnt = w.take(ncols * g.nb * 4);
  for (int l = 0; l <= MSM_NLEV; l++) g.o_off[l] = w.take(ncols * (g.nb + 1) * 4);
  g.o_ent = w.take(ncols * g.ecap * 4);
  g.o_list[0] = 0;
  for (int l = 1; l <= MSM_NLEV; l++) g.o_list[l] = w.take(ncols * g.cap[l] * sizeof(G1X29));
  g.o_dense = w.take(ncols * g.nb * sizeof(G1X29));
  g.G = g.nb >> 6;
  g.o_rows = w.take(ncols * g.G * sizeof(G1X29));
  g.o_cols = w.take(ncols * ((g.G + 63) / 64) * 64 * sizeof(G1X29));
  g.bytes = w.bytes();
  return g;
}
static MsmGeom msm_geometry(const amdzk_srs* srs, size_t ncols, size_t len, bool latency_mode) {
  return msm_geometry_cw(srs->c, srs->W, false, ncols, len, latency_mode);
}

// Where the scalars of a batch are: column c at base + c * stride, or — ptrs != null, window-table form only — at ptrs[c],
// a device array of device addresses.
struct MsmScalars {
  const Fr* base;
  size_t stride;
  const Fr* const* ptrs;
};

// table: what level 1 gathers from (a window table of rows of table_n points, or — per_window — the converted copy of the
// caller's bases, table_n = 0). per_window: ncols counts virtual columns (column, window) over ncols / g.W scalar columns.
// ctx->msm_l1_evt (made on first use) is recorded when the level-1 kernel ends; a batch that went out whole leaves
// ctx->msm_l1_fresh set (zk_stream_after_l1).
static int msm_group(amdzk_ctx* ctx, const G1Affine* table, uint32_t table_n, bool per_window, const MsmGeom& g, char* ws, const MsmScalars& sc,
                     size_t ncols, size_t len, G1X* outp) {
  if (!ctx->msm_l1_evt) ZK_HIP(ctx, hipEventCreateWithFlags(&ctx->msm_l1_evt, hipEventDisableTiming));
  const uint32_t nb = g.nb;
  uint32_t* blk_hist = (uint32_t*)(ws + g.o_bh);
  uint32_t* cnt = (uint32_t*)(ws + g.o_cnt);
  uint32_t* off[MSM_NLEV + 1];
  G1X29* list[MSM_NLEV + 1];
  for (int l = 0; l <= MSM_NLEV; l++) off[l] = (uint32_t*)(ws + g.o_off[l]), list[l] = (G1X29*)(ws + g.o_list[l]);
  uint32_t* entries = (uint32_t*)(ws + g.o_ent);
  G1X29* dense = (G1X29*)(ws + g.o_dense);
  G1X29 *rows = (G1X29*)(ws + g.o_rows), *cols = (G1X29*)(ws + g.o_cols);

  DigitArgs da;
  da.scalars = sc.base;
  da.col_stride = sc.stride;
  if (sc.ptrs) {
    if (per_window) ZK_FAIL(ctx, AMDZK_E_INVALID, "msm: a column pointer table needs the window-table form");
    da.col_ptrs = sc.ptrs;
    da.col_stride = 0;
  }
  da.len = (uint32_t)len;
  da.nb = nb;
  da.chunk = g.chunk;
  da.nblk = g.nblk;
  da.blk_hist = blk_hist;
  da.off0 = off[0];
  da.entries = entries;
  da.ecap = g.ecap;
  da.table_n = table_n;
  dim3 dgrid(g.nblk, (unsigned)ncols);
  // quad-lane point additions in the folds and the bucket reduction: in latency mode (-1), never (0), always (1: tests)
  static const int tail_quad = getenv("AMDZK_TAIL_QUAD") ? atoi(getenv("AMDZK_TAIL_QUAD")) : -1;
  const bool quad_on = (tail_quad < 0 ? g.latency : tail_quad != 0) && ncols <= 65535;
  const size_t scan_shmem = (16 + (nb + 1 <= SCAN_LDS_WORDS ? (size_t)nb + 1 : 0)) * sizeof(uint32_t);
  if (scan_shmem > 65536)
    ZK_HIP(ctx, hipFuncSetAttribute((const void*)msm_scan_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((16 + SCAN_LDS_WORDS) * sizeof(uint32_t))));
  if (per_window) ZK_TRY(launch_digits_win<false>(ctx, g.c, da, dgrid));
  else if (sc.ptrs) ZK_TRY((launch_digits<false, true>(ctx, g.c, da, dgrid, g.big_digits)));
  else ZK_TRY((launch_digits<false, false>(ctx, g.c, da, dgrid, g.big_digits)));
  ZK_LAUNCH(ctx, "msm_blk_offsets", msm_blk_offsets_kernel, dim3((nb + 255) / 256, (unsigned)ncols), dim3(256), 0, blk_hist, cnt, nb, g.nblk);
  ZK_LAUNCH(ctx, "msm_scan", msm_scan_kernel, dim3((unsigned)ncols), dim3(1024), scan_shmem, cnt, off[0], nb, 1u, 1);
  if (per_window) ZK_TRY(launch_digits_win<true>(ctx, g.c, da, dgrid));
  else if (sc.ptrs) ZK_TRY((launch_digits<true, true>(ctx, g.c, da, dgrid, g.big_digits)));
  else ZK_TRY((launch_digits<true, false>(ctx, g.c, da, dgrid, g.big_digits)));
  for (int l = 1; l <= MSM_NLEV; l++) {
    const uint32_t T = l == 1 ? g.T1 : g.TL;
    ZK_LAUNCH(ctx, "msm_scan", msm_scan_kernel, dim3((unsigned)ncols), dim3(1024), scan_shmem, off[l - 1], off[l], nb, T, 2);
    AccArgs a;
    a.off_in = off[l - 1];
    a.off_out = off[l];
    a.nb = nb;
    a.T = T;
    a.entries = entries;
    a.ecap = g.ecap;
    a.table = table;
    a.in_list = list[l - 1];
    a.in_cap = g.cap[l - 1];
    a.out_list = list[l];
    a.out_cap = g.cap[l];
    const size_t threads = (g.cap[l - 1] + T - 1) / T;
    dim3 grid((unsigned)((threads + MSM_THREADS - 1) / MSM_THREADS), (unsigned)ncols);
    if (l == 1) {
      ZK_LAUNCH(ctx, "msm_accum_l1", msm_accum_seg_kernel<true>, grid, dim3(MSM_THREADS), 0, a);
      ZK_HIP(ctx, hipEventRecord(ctx->msm_l1_evt, ctx->stream));
    } else if (quad_on && !(getenv("AMDZK_FOLD_QUAD") && atoi(getenv("AMDZK_FOLD_QUAD")) == 0)) {
      const dim3 qgrid((unsigned)((4 * threads + MSM_THREADS - 1) / MSM_THREADS), (unsigned)ncols);
      ZK_LAUNCH(ctx, "msm_accum_fold", msm_accum_fold_quad_kernel, qgrid, dim3(MSM_THREADS), 0, a);
    } else {
      ZK_LAUNCH(ctx, "msm_accum_fold", msm_accum_seg_kernel<false>, grid, dim3(MSM_THREADS), 0, a);
    }
  }
  const unsigned fold_w = (unsigned)((g.G + 63) / 64);  // 1, 2, 4 or 8 (c <= 16): at most 9 wavefronts per workgroup (launch bound 576)
  ZK_LAUNCH(ctx, "msm_accum_final", msm_accum_final_kernel, dim3(nb / 64, (unsigned)ncols), dim3(64), 0, off[MSM_NLEV], nb, list[MSM_NLEV],
            g.cap[MSM_NLEV], dense);
  static const int tail_tree = getenv("AMDZK_TAIL_TREE") ? atoi(getenv("AMDZK_TAIL_TREE")) : -1;  // -1: in latency mode; 0 / 1: never / always
  const bool quad = quad_on && fold_w == 1;
  if (quad)
    ZK_LAUNCH(ctx, "msm_rowcol", msm_rowcol_quad_kernel, dim3(64, 2, (unsigned)ncols), dim3(256), 0, dense, nb, rows, cols);
  else if ((tail_tree < 0 ? g.latency : tail_tree != 0) && ncols <= 65535)
    ZK_LAUNCH(ctx, "msm_rowcol", msm_rowcol_tree_kernel, dim3(64, (unsigned)(2 * ((g.G + 63) / 64)), (unsigned)ncols), dim3(64), 0, dense, nb, rows, cols);
  else
    ZK_LAUNCH(ctx, "msm_rowcol", msm_rowcol_kernel, dim3((unsigned)(2 * ((g.G + 63) / 64)), (unsigned)ncols), dim3(64 * ROWCOL_WAVES), 0, dense, nb, rows, cols);
  if (quad) ZK_LAUNCH(ctx, "msm_fold", msm_fold_quad_kernel, dim3((unsigned)ncols), dim3(512), 0, rows, cols, nb, outp);
  else if (fold_w == 1) ZK_LAUNCH(ctx, "msm_fold", msm_fold_kernel<1>, dim3((unsigned)ncols), dim3(128), 0, rows, cols, nb, outp);
  else ZK_LAUNCH(ctx, "msm_fold", msm_fold_kernel<8>, dim3((unsigned)ncols), dim3(64 * (fold_w + 1)), 0, rows, cols, nb, outp);
  ctx->msm_l1_fresh = true;
  return AMDZK_OK;
}

// The refusals the two window-table entry points share, in their order: the basis and the length (msm_check_basis), then
// the entry point's own rule for the column count, then a table whose point ids do not fit 31 bits (msm_check_ids).
static int msm_check_basis(amdzk_ctx* ctx, const amdzk_srs* srs, int basis, size_t len) {
  if (!srs || basis < 0 || basis >= AMDZK_NUM_BASES) ZK_FAIL(ctx, AMDZK_E_INVALID, "msm: no parameters or basis %d unknown", basis);
  if (!srs->table[basis]) {
    if (basis == AMDZK_BASIS_G_LAGRANGE_PREFIX)
      ZK_FAIL(ctx, AMDZK_E_INVALID, "msm: the prefix-sum basis has not been built (it is made with the first proving key that has permutation columns)");
    ZK_FAIL(ctx, AMDZK_E_INVALID, "msm: basis %d not uploaded", basis);
  }
  if (len > srs->n) ZK_FAIL(ctx, AMDZK_E_INVALID, "msm: len %zu > 2^k = %zu", len, srs->n);
  return AMDZK_OK;
}
static int msm_check_ids(amdzk_ctx* ctx, const amdzk_srs* srs) {
  if ((uint64_t)srs->W * srs->n >= (1ull << 31)) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "msm: table too large for 31-bit ids");
  return AMDZK_OK;
}

// ncols MSMs of length len over srs->table[basis]; results (XYZZ) land in d_out[ncols].
int zk_msm_dev_xyzz(amdzk_ctx* ctx, const amdzk_srs* srs, int basis, const Fr* d_scalars, size_t ncols,
                    size_t len, size_t col_stride, G1X** d_out) {
  ZK_TRY(msm_check_basis(ctx, srs, basis, len));
  if (ncols == 0 || ncols > 65535) ZK_FAIL(ctx, AMDZK_E_INVALID, "msm: ncols %zu out of range", ncols);
  ZK_TRY(msm_check_ids(ctx, srs));
  const MsmGeom g = msm_geometry(srs, ncols, len, ctx->msm_latency_mode);
  WsLayout w;
  w.take(g.bytes);
  const size_t o_out = w.take(ncols * sizeof(G1X));
  char* ws = nullptr;
  ZK_TRY(zk_ws_reserve(ctx, ZK_WS_MSM, w.bytes(), (void**)&ws));
  G1X* outp = (G1X*)(ws + o_out);
  ZK_TRY(msm_group(ctx, srs->table[basis], (uint32_t)srs->n, false, g, ws, MsmScalars{d_scalars, col_stride, nullptr}, ncols, len, outp));
  *d_out = outp;
  return AMDZK_OK;
}

// The same MSM with column c read from d_col_ptrs[c] — a DEVICE array of ncols device pointers, `len` scalars behind each —
// instead of d_scalars + c * col_stride: the columns of one commitment step of a batch of proofs live in as many workspaces
// (prover.hip, Gang). Only the counting sort's scalar loads differ (msm_digit_kernel<.., PTRS>); geometry, level 1, folds
// and the bucket reduction are those of zk_msm_dev_xyzz for the same column count. Results (XYZZ) land in d_out[ncols],
// column order. A batch whose geometry would take more than max_ws_bytes of workspace (0: MSM_COLS_WS_BYTES) or more than
// 65535 columns is cut into the fewest equal runs of columns that fit, submitted one behind the other on the stream over
// the same scratch; the results of all runs sit in front of it. One column is never cut: it runs alone whatever it takes.
// The table must stay untouched until the call's kernels have run (stream order).
// 16 GiB: at k = 15 (c = 13, 20 windows) a column's counting-sort entries and bucket lists take about 15 MiB, so ten proofs'
// 1410 advice columns go as two runs of 705 — five times the 141 columns with which one proof already fills the chip, so the
// cut costs no occupancy — and two contexts with full scratch hold a ninth of the 288 GB of HBM beside keys and workspaces.
static constexpr size_t MSM_COLS_WS_BYTES = (size_t)16 << 30;
int zk_msm_dev_xyzz_cols(amdzk_ctx* ctx, const amdzk_srs* srs, int basis, const Fr* const* d_col_ptrs, size_t ncols, size_t len,
                         size_t max_ws_bytes, G1X** d_out) {
  ZK_TRY(msm_check_basis(ctx, srs, basis, len));
  if (!d_col_ptrs || ncols == 0) ZK_FAIL(ctx, AMDZK_E_INVALID, "msm: no column pointer table or ncols == 0");
  ZK_TRY(msm_check_ids(ctx, srs));
  const size_t cap = max_ws_bytes ? max_ws_bytes : MSM_COLS_WS_BYTES;
  // a run's geometry: that of its column count; the last run may be shorter, and fewer columns can mean finer tasks and so
  // more bytes per column — the scratch holds the larger of the two
  size_t runs = (ncols + 65534) / 65535, per = 0, bytes = 0;
  for (;; runs++) {
    per = (ncols + runs - 1) / runs;
    const size_t last = ncols - (ncols - 1) / per * per;
    bytes = std::max(msm_geometry(srs, per, len, ctx->msm_latency_mode).bytes, msm_geometry(srs, last, len, ctx->msm_latency_mode).bytes);
    if (per == 1 || bytes <= cap) break;
  }
  WsLayout w;  // the results of all runs | one run's scratch
  w.take(ncols * sizeof(G1X));
  const size_t o_scratch = w.take(bytes);
  char* ws = nullptr;
  ZK_TRY(zk_ws_reserve(ctx, ZK_WS_MSM, w.bytes(), (void**)&ws));
  G1X* outp = (G1X*)ws;
  for (size_t first = 0; first < ncols; first += per) {
    const size_t cnt = std::min(per, ncols - first);
    const MsmGeom gr = msm_geometry(srs, cnt, len, ctx->msm_latency_mode);
    ZK_TRY(msm_group(ctx, srs->table[basis], (uint32_t)srs->n, false, gr, ws + o_scratch, MsmScalars{nullptr, 0, d_col_ptrs + first}, cnt, len,
                     outp + first));
  }
  *d_out = outp;
  return AMDZK_OK;
}

// ---- caller-supplied bases: arithmetic::best_multiexp(coeffs, bases) without an amdzk_srs.
// No window table: the classical Pippenger shape — one bucket set per window (virtual column = (column, window), the whole
// pipeline above with grid.y = ncols * W over ONE converted copy of the bases), then sum_w 2^(c w) S_w
// (msm_window_combine_kernel). Costs W bucket reductions and ~255 dependent doublings where the table form has one and
// none; saves the table: (W - 1) (c doublings + one inversion) per point and W x 64 bytes.
//
// Window width. By operation count a call costs W (len + a nb) point additions (level 1, plus a ~ 6 per bucket on its
// way through the folds, the per-bucket final and the row / column sums): 8, 10, 13, 15, 16 bits from 2^10 to 2^22 points.
// The sweep (2^10 .. 2^22 points, all nine widths: profiles/msm_foreign_bases.txt) did not follow the count, for two
// reasons it also shows:
//  * up to 2^18 points the call is latency, not work: msm_window_combine's ~255 dependent doublings (0.6 - 0.8 ms at any
//    width) and the bucket reduction's chain; fewer windows are fewer virtual columns in that tail;
//  * from 2^20 the counting sort is W passes over the scalars, each workgroup with 2^(c-1) counters in LDS — one workgroup
//    per compute unit at c = 16 — and grows faster with c than level 1 shrinks (2^22, c = 13 -> 16: level 1 5.86 -> 4.96 ms, the
//    whole call 10.3 -> 11.0; the sort is 2.8 ms at c = 13).
// c = 13 is the fastest width at 2^14 (1.13 ms), 2^16, 2^18, 2^20 (3.36 against 3.51 at c = 15) and 2^22 (10.3 against 10.4
// at c = 15, 11.0 at c = 16); at 2^10 c = 12 is the fastest (1.24 ms against 1.32 at c = 13). The widths whose TOP window is
// poorly filled pay for it as predicted: the top window of a 254-bit scalar has (r >> c (W - 1)) + 1 digits — 97 at c = 13, but 4 at c = 9,
// 12 and 14 and 2 at c = 11 — so its virtual column is two or four buckets of len / 4 entries that msm_accum_final's
// cooperative path takes one after the other: 0.15 - 0.35 ms in msm_accum_final from 2^14 points at c = 9, 12, 14 (1.0 ms at
// c = 9 and 2^22), 0.10 - 0.25 at c = 11 (and 0.2 - 0.5 from 2^18 at c = 10 with its 13 digits), 0.03 - 0.05 at c = 13 at every size (msm_geometry's fold-width rule sees to its 97).
// AMDZK_MSM_BASES_C forces a width 8..16 (sweeps, tests).
static uint32_t pick_window_bits_bases(size_t len) {
  if (const char* e = getenv("AMDZK_MSM_BASES_C")) {
    int v = atoi(e);
    if (v >= 8 && v <= 16) return (uint32_t)v;
  }
  return len < ((size_t)1 << 12) ? 12 : 13;  // measured at 2^10 and 2^14; where between them the cut belongs is not
}

// THE geometry of a table-free MSM: amdzk_msm_g1_bases_plan reports it, zk_msm_bases_dev_xyzz reserves it.
struct MsmBasesPlan {
  MsmGeom g;       // over ncols * W virtual columns
  size_t vcols;
  size_t o_win;    // G1X[vcols]: the window sums
  size_t o_out;    // G1X[ncols]: the results
  size_t o_bases;  // G1Affine[len]: the bases in radix 2^261
  size_t bytes;
};
// Pure host code. Returns AMDZK_OK or the status of the refusal, with its reason in `why`.
static int zk_msm_bases_plan(size_t ncols, size_t len, bool latency_mode, MsmBasesPlan* p, char why[160]) {
  why[0] = 0;
  if (ncols == 0) {
    snprintf(why, 160, "msm_bases: ncols == 0");
    return AMDZK_E_INVALID;
  }
  if (len >= ((size_t)1 << 31)) {
    snprintf(why, 160, "msm_bases: len %zu >= 2^31 (31-bit point ids)", len);
    return AMDZK_E_UNSUPPORTED;
  }
  const uint32_t c = pick_window_bits_bases(len), W = (255 + c - 1) / c;
  if (ncols > 65535 / W) {
    snprintf(why, 160, "msm_bases: ncols %zu x %u windows > 65535 (one launch per batch: split the batch)", ncols, W);
    return AMDZK_E_UNSUPPORTED;
  }
  p->vcols = ncols * W;
  p->g = msm_geometry_cw(c, W, true, p->vcols, len, latency_mode);
  WsLayout w;
  w.take(p->g.bytes);
  p->o_win = w.take(p->vcols * sizeof(G1X)), p->o_out = w.take(ncols * sizeof(G1X)), p->o_bases = w.take((len ? len : 1) * sizeof(G1Affine));
  p->bytes = w.bytes();
  return AMDZK_OK;
}

int zk_msm_bases_plan_host(size_t ncols, size_t len, uint32_t* window_bits, uint32_t* windows, size_t* scratch_bytes, char why[160]) {
  MsmBasesPlan p;
  const int rc = zk_msm_bases_plan(ncols, len, false, &p, why);  // latency mode picks kernels, never sizes
  if (rc != AMDZK_OK) return rc;
  if (window_bits) *window_bits = p.g.c;
  if (windows) *windows = p.g.W;
  if (scratch_bytes) *scratch_bytes = p.bytes;
  return AMDZK_OK;
}

// ncols MSMs of `len` scalars each (column c at d_scalars + c * col_stride) over the `len` affine points at d_bases
// (radix 2^256 as everywhere on the ABI, (0, 0) = identity, not checked to be on the curve; read only). len > 0.
// Results (XYZZ) land in d_out[ncols].
int zk_msm_bases_dev_xyzz(amdzk_ctx* ctx, const Fr* d_scalars, size_t ncols, size_t len, size_t col_stride, const G1Affine* d_bases,
                          G1X** d_out) {
  MsmBasesPlan p;
  char why[160];
  const int rc = zk_msm_bases_plan(ncols, len, ctx->msm_latency_mode, &p, why);
  if (rc != AMDZK_OK) ZK_FAIL(ctx, rc, "%s", why);
  if (!d_scalars || !d_bases || len == 0) ZK_FAIL(ctx, AMDZK_E_INVALID, "msm_bases: null pointer or len == 0");
  if (ncols > 1 && col_stride < len) ZK_FAIL(ctx, AMDZK_E_INVALID, "msm_bases: col_stride %zu < len %zu", col_stride, len);
  char* ws = nullptr;
  ZK_TRY(zk_ws_reserve(ctx, ZK_WS_MSM, p.bytes, (void**)&ws));
  G1X *win = (G1X*)(ws + p.o_win), *outp = (G1X*)(ws + p.o_out);
  G1Affine* bases = (G1Affine*)(ws + p.o_bases);
  ZK_HIP(ctx, hipMemcpyAsync(bases, d_bases, len * sizeof(G1Affine), hipMemcpyDeviceToDevice, ctx->stream));
  ZK_LAUNCH(ctx, "msm_bases_to_r261", table_to_r261_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, bases, len);
  ZK_TRY(msm_group(ctx, bases, 0, true, p.g, ws, MsmScalars{d_scalars, col_stride, nullptr}, p.vcols, len, win));
  ZK_LAUNCH(ctx, "msm_window_combine", msm_window_combine_kernel, dim3((unsigned)((4 * ncols + 63) / 64)), dim3(64), 0, (const G1X*)win, p.g.W,
            p.g.c, (uint32_t)ncols, outp);
  *d_out = outp;
  return AMDZK_OK;
}

// Host finish: XYZZ -> normalised Jacobian (z = 1) with one shared inversion (Montgomery's trick).
int zk_msm_finish(amdzk_ctx* ctx, const G1X* d_res, size_t ncols, uint64_t* out_jac) {
  G1X* h = nullptr;
  ZK_TRY(zk_pinned_reserve(ctx, ncols * sizeof(G1X), (void**)&h));
  ZK_HIP(ctx, hipMemcpyAsync(h, d_res, ncols * sizeof(G1X), hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  std::vector<Fq> pre(ncols);
  Fq acc = Fq::one();
  for (size_t i = 0; i < ncols; i++) {
    pre[i] = acc;
    if (!h[i].is_inf()) acc = mul(acc, h[i].zzz);
  }
  acc = inv(acc);
  for (size_t i = ncols; i-- > 0;) {
    G1Jac* o = reinterpret_cast<G1Jac*>(out_jac + 12 * i);
    if (h[i].is_inf()) {
      o->x = Fq::zero();
      o->y = Fq::one();
      o->z = Fq::zero();
      continue;
    }
    Fq izzz = mul(acc, pre[i]);
    acc = mul(acc, h[i].zzz);
    Fq iz = mul(h[i].zz, izzz);
    Fq izz = sqr(iz);
    o->x = mul(h[i].x, izz);
    o->y = mul(h[i].y, izzz);
    o->z = Fq::one();
  }
  return AMDZK_OK;
}
