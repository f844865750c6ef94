// The pairing unit (include/amdzk.h "pairing"): amdzk_g2_prepare / amdzk_g2_setup (host half, pairing.hpp),
// the SRS file's G2 codec and membership test (amdzk_g2_compress / _decompress / _check: host only, g2codec.hpp)
// and amdzk_pairing_products — n independent products of m pairings over the same m prepared G2 points — as two launches:
// one lane per (check, pair) runs the Miller program over that pair's prepared lines (no G2 arithmetic on the device), one
// lane per check multiplies its m Miller values, runs the final-exponentiation program and compares with one. A lane's
// running values are Fq2 registers in a slab of global memory, contiguous per lane; the programs (pairing.hpp) and the
// executor (fq12.cuh) are the same ones the host check runs. Both kernels are latency-bound chains of about 10^4 dependent
// Fq products per lane, so the blocks are single waves with FEW active lanes (pairing_active_lanes): the lanes spread
// over every SIMD of the chip before any wave gets a second one, as proof_decode_kernel's single-wave blocks do.
#include <string.h>

#include <vector>

#include "common.hpp"
#include "g2codec.hpp"
#include "pairing.hpp"

using namespace bn254;

// ONE prepared point: constants | lines | the three programs (the same in every handle: a handle is self-contained)
struct amdzk_g2 {
  int device = 0;
  char* d = nullptr;
};

namespace {

constexpr uint32_t PAIRING_THREADS = 64;

struct MillerArgs {
  const uint32_t* prog;
  uint32_t prog_len, regs, m, active;
  const Fq2x* K;
  const Fq* const* lines;  // [m]
  const G1Affine* g1;      // [total], this launch's first lane at 0
  Fq2x* slab;              // [total][regs]
  size_t total;
};
// lane t = blockIdx.x * active + threadIdx.x, for threadIdx.x < active
__global__ __launch_bounds__(PAIRING_THREADS) void pairing_miller_kernel(MillerArgs a) {
  if (threadIdx.x >= a.active) return;
  const size_t t = (size_t)blockIdx.x * a.active + threadIdx.x;
  if (t >= a.total) return;
  const G1Affine p = ld_aff(a.g1 + t);
  Fq2x* R = a.slab + t * a.regs;
  if (p.is_inf()) {  // the identity contributes the factor 1
    R[pairing::MILLER_F] = fq2x_one();
    for (int k = 1; k < 6; k++) R[pairing::MILLER_F + k] = fq2x_zero();
    return;
  }
  R[pairing::MILLER_XP] = Fq2x{fq29_from_r256(p.x), fqx_zero()};
  R[pairing::MILLER_YP] = Fq2x{fq29_from_r256(p.y), fqx_zero()};
  pairing_exec(a.prog, a.prog_len, R, a.K, a.lines[t % a.m]);
}

struct FinalArgs {
  const uint32_t *mul_prog, *fin_prog;
  uint32_t mul_len, fin_len, regs, miller_regs, m, active;
  const Fq2x* K;
  const Fq2x* miller_slab;  // [n * m][miller_regs]
  Fq2x* slab;               // [n][regs]
  size_t n;
  Fq* gt_out;        // [n][12]
  uint8_t* is_one;   // [n]
};
__global__ __launch_bounds__(PAIRING_THREADS) void pairing_final_kernel(FinalArgs a) {
  if (threadIdx.x >= a.active) return;
  const size_t i = (size_t)blockIdx.x * a.active + threadIdx.x;
  if (i >= a.n) return;
  Fq2x* R = a.slab + i * a.regs;
  const Fq2x* M = a.miller_slab + i * a.m * a.miller_regs + pairing::MILLER_F;
  for (int k = 0; k < 6; k++) R[pairing::FINAL_A + k] = M[k];
#pragma unroll 1
  for (uint32_t j = 1; j <= a.m; j++) {  // m - 1 products, then the exponentiation: one site of the executor
    const bool last = j == a.m;
    if (!last)
      for (int k = 0; k < 6; k++) R[pairing::FINAL_B + k] = M[(size_t)j * a.miller_regs + k];
    pairing_exec(last ? a.fin_prog : a.mul_prog, last ? a.fin_len : a.mul_len, R, a.K, nullptr);
  }
  Fq out[12];
  fq12x_to_r256(out, R + pairing::FINAL_A);
  for (int k = 0; k < 12; k++) st_fq(a.gt_out + i * 12 + k, out[k]);
  a.is_one[i] = gt_is_one(out) ? 1 : 0;
}

// lanes per single-wave block: one until every SIMD of the chip has a wave, then as many as it takes
uint32_t pairing_active_lanes(const amdzk_ctx* ctx, size_t total) {
  const size_t simds = (size_t)(ctx->num_cu > 0 ? ctx->num_cu : 1) * 4;
  const size_t a = (total + simds - 1) / simds;
  return (uint32_t)(a < 1 ? 1 : a > PAIRING_THREADS ? PAIRING_THREADS : a);
}

}  // namespace

int zk_pairing_products(amdzk_ctx* ctx, const char* who, const amdzk_g2* const* qs, size_t m, const G1Affine* h_g1, size_t n, uint8_t* is_one,
                        uint64_t* gt_out) {
  if (!qs || !h_g1) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: null argument", who);
  if (m == 0 || n == 0) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: m or n is 0", who);
  if (m > AMDZK_PAIRING_MAX_M) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: m = %zu is above AMDZK_PAIRING_MAX_M = %d", who, m, AMDZK_PAIRING_MAX_M);
  if (n > ((size_t)1 << 20)) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: more than 2^20 products in one call", who);
  for (size_t j = 0; j < m; j++) {
    if (!qs[j] || !qs[j]->d) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: null argument (prepared point %zu)", who, j);
    if (qs[j]->device != ctx->device) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: prepared point %zu lives on device %d, the ctx on %d", who, j, qs[j]->device, ctx->device);
  }
  const pairing::Programs& P = pairing::programs();
  const size_t total = n * m, chunk = pairing::pairing_chunk(n, m);  // checks per launch
  const pairing::CallLayout L = pairing::call_layout(n, m, chunk, P.miller.regs, P.final_regs);
  const size_t up = L.miller_slab, down = n * 12 * sizeof(Fq) + n;
  char* ws = nullptr;
  ZK_TRY(zk_ws_reserve(ctx, ZK_WS_STARTUP, L.bytes, (void**)&ws));
  char* pin = nullptr;
  ZK_TRY(zk_pinned_reserve(ctx, up > down ? up : down, (void**)&pin));
  memset(pin, 0, L.g1);
  for (size_t j = 0; j < m; j++) ((const Fq**)pin)[j] = (const Fq*)(qs[j]->d + P.at.lines);
  memcpy(pin + L.g1, h_g1, total * sizeof(G1Affine));
  ZK_HIP(ctx, hipMemcpyAsync(ws, pin, up, hipMemcpyHostToDevice, ctx->stream));
  const char* q0 = qs[0]->d;  // constants and programs: any handle's copy
  for (size_t c0 = 0; c0 < n; c0 += chunk) {
    const size_t nc = c0 + chunk < n ? chunk : n - c0, lanes = nc * m;
    MillerArgs ma;
    ma.prog = (const uint32_t*)(q0 + P.at.miller), ma.prog_len = (uint32_t)P.miller.w.size(), ma.regs = (uint32_t)P.miller.regs, ma.m = (uint32_t)m;
    ma.active = pairing_active_lanes(ctx, lanes), ma.K = (const Fq2x*)q0, ma.lines = (const Fq* const*)ws;
    ma.g1 = (const G1Affine*)(ws + L.g1) + c0 * m, ma.slab = (Fq2x*)(ws + L.miller_slab), ma.total = lanes;
    ZK_LAUNCH(ctx, "pairing_miller", pairing_miller_kernel, dim3((unsigned)((lanes + ma.active - 1) / ma.active)), dim3(PAIRING_THREADS), 0, ma);
    FinalArgs fa;
    fa.mul_prog = (const uint32_t*)(q0 + P.at.mul), fa.fin_prog = (const uint32_t*)(q0 + P.at.fin), fa.mul_len = (uint32_t)P.mul.w.size();
    fa.fin_len = (uint32_t)P.fin.w.size(), fa.regs = P.final_regs, fa.miller_regs = (uint32_t)P.miller.regs, fa.m = (uint32_t)m;
    fa.active = pairing_active_lanes(ctx, nc), fa.K = (const Fq2x*)q0, fa.miller_slab = (const Fq2x*)(ws + L.miller_slab), fa.slab = (Fq2x*)(ws + L.final_slab);
    fa.n = nc, fa.gt_out = (Fq*)(ws + L.gt) + c0 * 12, fa.is_one = (uint8_t*)(ws + L.is_one) + c0;
    ZK_LAUNCH(ctx, "pairing_final", pairing_final_kernel, dim3((unsigned)((nc + fa.active - 1) / fa.active)), dim3(PAIRING_THREADS), 0, fa);
  }
  ZK_HIP(ctx, hipMemcpyAsync(pin, ws + L.gt, down, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  if (gt_out) memcpy(gt_out, pin, n * 12 * sizeof(Fq));
  if (is_one) memcpy(is_one, pin + n * 12 * sizeof(Fq), n);
  return AMDZK_OK;
}

extern "C" int amdzk_g2_prepare(amdzk_ctx* ctx, const uint64_t q[16], amdzk_g2** out) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  if (!q || !out) ZK_FAIL(ctx, AMDZK_E_INVALID, "g2_prepare: null argument");
  *out = nullptr;
  const pairing::G2Affine p = pairing::g2_from_words(q);
  if (!is_canonical(p.x.c0) || !is_canonical(p.x.c1) || !is_canonical(p.y.c0) || !is_canonical(p.y.c1))
    ZK_FAIL(ctx, AMDZK_E_INVALID, "g2_prepare: a coordinate is not below the modulus");
  if (p.is_inf()) ZK_FAIL(ctx, AMDZK_E_INVALID, "g2_prepare: the identity has no prepared form");
  if (!pairing::g2_on_twist(p)) ZK_FAIL(ctx, AMDZK_E_INVALID, "g2_prepare: the point is not on the twist");
  const pairing::Programs& P = pairing::programs();
  std::vector<char> host(P.at.bytes, 0);
  pairing::device_consts((Fq2x*)host.data());
  pairing::g2_prepare(p, (Fq*)(host.data() + P.at.lines));
  memcpy(host.data() + P.at.miller, P.miller.w.data(), P.miller.w.size() * 4);
  memcpy(host.data() + P.at.mul, P.mul.w.data(), P.mul.w.size() * 4);
  memcpy(host.data() + P.at.fin, P.fin.w.data(), P.fin.w.size() * 4);
  amdzk_g2* g = new amdzk_g2();
  g->device = ctx->device;
  hipError_t e = hipMalloc((void**)&g->d, P.at.bytes);
  if (e == hipSuccess) e = hipMemcpyAsync(g->d, host.data(), P.at.bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = zk_host_wait(ctx, ctx->stream);
  if (e != hipSuccess) {
    if (g->d) (void)hipFree(g->d);
    delete g;
    ZK_FAIL(ctx, e == hipErrorOutOfMemory ? AMDZK_E_NOMEM : AMDZK_E_HIP, "g2_prepare: %s", hipGetErrorString(e));
  }
  *out = g;
  return AMDZK_OK;
}

extern "C" void amdzk_g2_free(amdzk_ctx* ctx, amdzk_g2* g) {
  ZK_ENTER(ctx);
  if (!g) return;
  if (g->d) (void)hipFree(g->d);
  delete g;
}

extern "C" int amdzk_g2_setup(amdzk_ctx* ctx, const uint64_t s[4], uint64_t g2_out[16], uint64_t s_g2_out[16]) {
  if (!ctx) return AMDZK_E_INVALID;
  if (!s || !g2_out || !s_g2_out) ZK_FAIL(ctx, AMDZK_E_INVALID, "g2_setup: null argument");
  Fr sm;
  memcpy(sm.l, s, 32);
  if (!is_canonical(sm)) ZK_FAIL(ctx, AMDZK_E_INVALID, "g2_setup: s is not below the modulus");
  const Fr k = from_mont(sm);
  uint64_t kw[4];
  memcpy(kw, k.l, 32);
  const pairing::G2Affine g = pairing::g2_generator();
  pairing::g2_to_words(g, g2_out);
  pairing::g2_to_words(pairing::g2_mul(g, kw), s_g2_out);
  return AMDZK_OK;
}

// ---- the SRS file's G2 fields and membership in G2: g2codec.hpp behind the C ABI. No ctx, no device.
static int g2_codec_result(const char* who, const char* why, char* msg, size_t msg_cap) {
  if (msg && msg_cap) {
    if (why) snprintf(msg, msg_cap, "%s: %s", who, why);
    else msg[0] = 0;
  }
  return why ? AMDZK_E_INVALID : AMDZK_OK;
}
extern "C" int amdzk_g2_compress(const uint64_t q[16], uint8_t out[64], char* msg, size_t msg_cap) {
  if (!q || !out) return g2_codec_result("g2_compress", "null argument", msg, msg_cap);
  return g2_codec_result("g2_compress", g2codec::g2_compress(q, out), msg, msg_cap);
}
extern "C" int amdzk_g2_decompress(const uint8_t in[64], uint64_t q_out[16], char* msg, size_t msg_cap) {
  if (!in || !q_out) return g2_codec_result("g2_decompress", "null argument", msg, msg_cap);
  return g2_codec_result("g2_decompress", g2codec::g2_decompress(in, q_out), msg, msg_cap);
}
extern "C" int amdzk_g2_check(const uint64_t q[16], int* status) {
  if (!q || !status) return AMDZK_E_INVALID;
  *status = g2codec::g2_status(q);
  return AMDZK_OK;
}

extern "C" int amdzk_pairing_products(amdzk_ctx* ctx, const amdzk_g2* const* qs, size_t m, const uint64_t* g1, size_t n, uint8_t* is_one,
                                      uint64_t* gt_out) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  return zk_pairing_products(ctx, "pairing_products", qs, m, (const G1Affine*)g1, n, is_one, gt_out);
}
