// The whole life of an amdzk_srs (srs.hpp): poly::kzg::commitment::ParamsKZG::{new, setup, write, read, downsize, get_g}
// and arithmetic::g_to_lagrange of halo2_proofs 0.2.0 [UP], the prefix-sum basis
// the permutation products are committed over, and the check that an SRS is one (amdzk_srs_check). Start-up work, all of
// it on the device, in the 32-bit radix-2^256 form of bn254.cuh; the window tables behind the bases are msm.hip's
// (zk_msm_fill_table) and so is their radix.
#include <stdlib.h>
#include <string.h>

#include "hostcrypto.hpp"     // ChaCha20Rng, fr_omega
#include "plonk_kernels.hpp"  // zk_batch_invert
#include "srs.hpp"

using namespace bn254;

uint32_t zk_srs_k(const amdzk_srs* srs) { return srs->k; }
// an MSM over this basis can run (multiopen.hip asks before it touches the caller's transcript)
bool zk_srs_has_basis(const amdzk_srs* srs, int basis) { return srs && basis >= 0 && basis < AMDZK_NUM_BASES && srs->table[basis]; }
// the n bases of a slot on the device, radix 2^256 (verify.hip takes G = g[0] from here); null when not resident
const G1Affine* zk_srs_base_dev(const amdzk_srs* srs, int basis) { return srs && basis >= 0 && basis < AMDZK_NUM_BASES ? srs->base[basis] : nullptr; }

// ParamsKZG::get_g() / g_lagrange: the affine bases back on the host.
int zk_srs_get(amdzk_ctx* ctx, const amdzk_srs* srs, int basis, uint64_t* out) {
  if (!srs || !out || basis < 0 || basis > 1) ZK_FAIL(ctx, AMDZK_E_INVALID, "srs_get: bad argument");
  if (!srs->base[basis]) ZK_FAIL(ctx, AMDZK_E_INVALID, "srs_get: basis %d was not uploaded", basis);
  ZK_HIP(ctx, hipMemcpyAsync(out, srs->base[basis], srs->n * sizeof(G1Affine), hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  return AMDZK_OK;
}

// ---------------------------------------------------------------------------------- slots
// Device memory of one basis slot: the window table and the bases. All or nothing — on failure both pointers are null
// and *refused is the request that was turned down.
static hipError_t srs_alloc_slot(const amdzk_srs* s, G1Affine** base, G1Affine** table, size_t* refused) {
  *base = *table = nullptr;
  hipError_t e = hipMalloc((void**)table, *refused = (size_t)s->W * s->n * sizeof(G1Affine));
  if (e == hipSuccess) e = hipMalloc((void**)base, *refused = s->n * sizeof(G1Affine));
  if (e != hipSuccess && *table) {
    hipFree(*table);
    *table = nullptr;
  }
  return e;
}

void zk_srs_free(amdzk_ctx*, amdzk_srs* s) {
  if (!s) return;
  for (int b = 0; b < AMDZK_NUM_BASES; b++) {
    if (s->table[b]) hipFree(s->table[b]);
    if (s->base[b]) hipFree(s->base[b]);
  }
  delete s;
}

// slots G and G_LAGRANGE of s <- the given bases (null: slot stays empty) and their window tables
static int srs_fill_slots(amdzk_ctx* ctx, amdzk_srs* s, const void* g, const void* g_lagrange, bool src_on_device) {
  const void* src[2] = {g, g_lagrange};
  for (int b = 0; b < 2; b++) {
    if (!src[b]) continue;
    size_t refused = 0;
    const hipError_t e = srs_alloc_slot(s, &s->base[b], &s->table[b], &refused);
    if (e != hipSuccess) ZK_FAIL(ctx, AMDZK_E_NOMEM, "srs: hipMalloc(%zu) failed: %s", refused, hipGetErrorString(e));
    ZK_HIP(ctx, hipMemcpyAsync(s->base[b], src[b], s->n * sizeof(G1Affine), src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                               ctx->stream));
    ZK_TRY(zk_msm_fill_table(ctx, s->base[b], s->table[b], s->n, s->c, s->W));
  }
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));  // source buffers may be released by the caller
  return AMDZK_OK;
}

// The one maker of an amdzk_srs. Whatever fails after `new`, the half-built object and its slots go through zk_srs_free.
static int srs_build(amdzk_ctx* ctx, const void* g, const void* g_lagrange, bool src_on_device, uint32_t k, amdzk_srs** out) {
  if (!out || (!g && !g_lagrange)) ZK_FAIL(ctx, AMDZK_E_INVALID, "srs: null argument");
  if (k > 26) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "srs: k %u > 26", k);
  amdzk_srs* s = new amdzk_srs();
  s->k = k;
  s->n = (size_t)1 << k;
  s->c = pick_window_bits(k);
  s->W = (255 + s->c - 1) / s->c;
  const int r = srs_fill_slots(ctx, s, g, g_lagrange, src_on_device);
  if (r != AMDZK_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // nothing in flight may still write what is freed
    zk_srs_free(ctx, s);
    return r;
  }
  *out = s;
  return AMDZK_OK;
}

int zk_srs_upload(amdzk_ctx* ctx, const uint64_t* g, const uint64_t* g_lagrange, uint32_t k, amdzk_srs** out) {
  return srs_build(ctx, g, g_lagrange, false, k, out);
}

// ---- ParamsKZG::setup(k, rng) [UP] with the secret s given explicitly (unsafe by construction, test
// and benchmark use only, exactly like upstream's setup): g[i] = s^i G, g_lagrange[i] = L_i(s) G with
// L_i(s) = omega^i (s^n - 1) / (n (s - omega^i)). Everything on the device.
namespace {
// out[i] = sum over set bits j of the canonical scalar of table[j] (table[j] = 2^j G), affine.
__global__ __launch_bounds__(256) void fixed_base_mul_kernel(const Fr* scalars, const G1Affine* table, G1Affine* out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4* sp = reinterpret_cast<const uint4*>(scalars + i);
  uint4 lo = sp[0], hi = sp[1];
  Fr s;
  s.l[0] = lo.x; s.l[1] = lo.y; s.l[2] = lo.z; s.l[3] = lo.w;
  s.l[4] = hi.x; s.l[5] = hi.y; s.l[6] = hi.z; s.l[7] = hi.w;
  Fr c = from_mont(s);
  G1X acc = G1X::inf();
#pragma unroll 1
  for (int limb = 0; limb < 8; limb++) {
    uint32_t w = c.l[limb];
#pragma unroll 1
    for (int b = 0; b < 32; b++)
      if ((w >> b) & 1) acc = x_add_affine(acc, ld_aff(table + limb * 32 + b));
  }
  st_aff(out + i, x_to_affine(acc));
}
// p[i] = base^i
__global__ void powers_kernel(Fr* p, Fr base, size_t count, uint32_t chunk) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t start = t * chunk;
  if (start >= count) return;
  Fr cur = pow_u64(base, start);
  size_t end = start + chunk < count ? start + chunk : count;
  for (size_t i = start; i < end; i++) {
    uint4* q = reinterpret_cast<uint4*>(p + i);
    q[0] = make_uint4(cur.l[0], cur.l[1], cur.l[2], cur.l[3]);
    q[1] = make_uint4(cur.l[4], cur.l[5], cur.l[6], cur.l[7]);
    cur = mul(cur, base);
  }
}
// den[i] = s - w[i]
__global__ void sub_from_const_kernel(Fr* den, const Fr* w, Fr s, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4* q = reinterpret_cast<const uint4*>(w + i);
  uint4 a = q[0], b = q[1];
  Fr v;
  v.l[0] = a.x; v.l[1] = a.y; v.l[2] = a.z; v.l[3] = a.w;
  v.l[4] = b.x; v.l[5] = b.y; v.l[6] = b.z; v.l[7] = b.w;
  Fr r = sub(s, v);
  uint4* o = reinterpret_cast<uint4*>(den + i);
  o[0] = make_uint4(r.l[0], r.l[1], r.l[2], r.l[3]);
  o[1] = make_uint4(r.l[4], r.l[5], r.l[6], r.l[7]);
}
// a[i] = a[i] * w[i] * c
__global__ void mul2_kernel(Fr* a, const Fr* w, Fr c, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4* q = reinterpret_cast<const uint4*>(w + i);
  uint4 x0 = q[0], x1 = q[1];
  Fr v;
  v.l[0] = x0.x; v.l[1] = x0.y; v.l[2] = x0.z; v.l[3] = x0.w;
  v.l[4] = x1.x; v.l[5] = x1.y; v.l[6] = x1.z; v.l[7] = x1.w;
  const uint4* p = reinterpret_cast<const uint4*>(a + i);
  uint4 y0 = p[0], y1 = p[1];
  Fr u;
  u.l[0] = y0.x; u.l[1] = y0.y; u.l[2] = y0.z; u.l[3] = y0.w;
  u.l[4] = y1.x; u.l[5] = y1.y; u.l[6] = y1.z; u.l[7] = y1.w;
  Fr r = mul(mul(u, v), c);
  uint4* o = reinterpret_cast<uint4*>(a + i);
  o[0] = make_uint4(r.l[0], r.l[1], r.l[2], r.l[3]);
  o[1] = make_uint4(r.l[4], r.l[5], r.l[6], r.l[7]);
}
}  // namespace

int zk_srs_setup(amdzk_ctx* ctx, uint32_t k, const uint64_t s_mont[4], const uint64_t omega_mont[4], amdzk_srs** out,
                 uint64_t* g_out, uint64_t* g_lagrange_out) {
  if (k > 26) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "srs_setup: k %u > 26", k);
  const size_t n = (size_t)1 << k;
  Fr s, omega;
  memcpy(s.l, s_mont, 32);
  memcpy(omega.l, omega_mont, 32);
  // Two trapdoors mean nothing. Words at or above r are no field element. With s^n = 1, s is a point omega^i of the domain:
  // s - omega^i = 0 has no inverse and (s^n - 1) / n = 0, so every L_i would come out 0 (upstream panics in invert().unwrap()).
  if (!is_canonical(s)) ZK_FAIL(ctx, AMDZK_E_INVALID, "srs_setup: s is not below the modulus (s >= r)");
  const Fr sn_minus_1 = sub(pow_u64(s, n), Fr::one());
  if (sn_minus_1.is_zero()) ZK_FAIL(ctx, AMDZK_E_INVALID, "srs_setup: s^n = 1 for n = 2^%u: s is a point of the domain, the Lagrange basis has no value there", k);
  // workspace: gtable[256] | scal[n] | w[n] | scratch[n] | g[n] | gl[n]
  char* ws = nullptr;
  const size_t bytes = 256 * sizeof(G1Affine) + 3 * n * sizeof(Fr) + 2 * n * sizeof(G1Affine);
  ZK_TRY(zk_ws_reserve(ctx, ZK_WS_STARTUP, bytes, (void**)&ws));
  G1Affine* gtab = (G1Affine*)ws;
  Fr* scal = (Fr*)(ws + 256 * sizeof(G1Affine));
  Fr* w = scal + n;
  Fr* scratch = w + n;
  G1Affine* g = (G1Affine*)(scratch + n);
  G1Affine* gl = g + n;
  {  // 2^j G on the host (256 doublings)
    std::vector<G1Affine> t(256);
    G1Affine gen;
    gen.x = Fq::one();
    gen.y = add(Fq::one(), Fq::one());
    t[0] = gen;
    for (int j = 1; j < 256; j++) t[j] = x_to_affine(x_dbl_affine(t[j - 1]));
    ZK_HIP(ctx, hipMemcpyAsync(gtab, t.data(), 256 * sizeof(G1Affine), hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  }
  const uint32_t chunk = 64;
  dim3 pg((unsigned)(((n + chunk - 1) / chunk + 63) / 64)), pb(64);
  dim3 eg((unsigned)((n + 255) / 256)), eb(256);
  ZK_LAUNCH(ctx, "srs_powers", powers_kernel, pg, pb, 0, scal, s, n, chunk);
  ZK_LAUNCH(ctx, "srs_fixed_base_mul", fixed_base_mul_kernel, eg, eb, 0, scal, gtab, g, n);
  // Lagrange scalars
  ZK_LAUNCH(ctx, "srs_powers", powers_kernel, pg, pb, 0, w, omega, n, chunk);
  ZK_LAUNCH(ctx, "srs_sub", sub_from_const_kernel, eg, eb, 0, scal, w, s, n);
  ZK_TRY(zk_batch_invert(ctx, scal, scratch, n));
  Fr two = add(Fr::one(), Fr::one());
  Fr mult = mul(sn_minus_1, inv(pow_u64(two, k)));  // (s^n - 1) / n
  ZK_LAUNCH(ctx, "srs_mul2", mul2_kernel, eg, eb, 0, scal, w, mult, n);
  ZK_LAUNCH(ctx, "srs_fixed_base_mul", fixed_base_mul_kernel, eg, eb, 0, scal, gtab, gl, n);
  if (g_out) ZK_HIP(ctx, hipMemcpyAsync(g_out, g, n * sizeof(G1Affine), hipMemcpyDeviceToHost, ctx->stream));
  if (g_lagrange_out) ZK_HIP(ctx, hipMemcpyAsync(g_lagrange_out, gl, n * sizeof(G1Affine), hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  return srs_build(ctx, g, gl, true, k, out);
}

// ---- ParamsKZG::{write, read} [UP]: k as u32 LE, then the n points of g and
// of g_lagrange in halo2curves' 32-byte compressed form, then g2 and s_g2 (64 bytes each, passed
// through untouched: the prover never uses G2). Compression / decompression (one Fq square root per
// point, q = 3 mod 4) run on the device.
namespace {
__global__ __launch_bounds__(256) void g1_compress_kernel(const G1Affine* pts, uint8_t* out, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G1Affine p = ld_aff(pts + i);
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (!p.is_inf()) {
    Fq x = from_mont(p.x), y = from_mont(p.y);
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = x.l[j];
    w[7] |= (y.l[0] & 1u) << 31;  // byte 31 bit 7 = parity of y
  }
  uint4* o = reinterpret_cast<uint4*>(out + 32 * i);
  o[0] = make_uint4(w[0], w[1], w[2], w[3]);
  o[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

__global__ __launch_bounds__(256) void g1_decompress_kernel(const uint8_t* in, G1Affine* out, size_t n, int* err) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4* q4 = reinterpret_cast<const uint4*>(in + 32 * i);
  uint4 a = q4[0], b = q4[1];
  Fq x;
  x.l[0] = a.x; x.l[1] = a.y; x.l[2] = a.z; x.l[3] = a.w;
  x.l[4] = b.x; x.l[5] = b.y; x.l[6] = b.z; x.l[7] = b.w;
  const uint32_t ysign = x.l[7] >> 31;
  x.l[7] &= 0x7fffffffu;
  G1Affine p;
  p.x = Fq::zero();
  p.y = Fq::zero();
  bool ok = is_canonical(x);  // x must be canonical (< q)
  if (ok && !(x.is_zero() && ysign == 0)) {
    const Fq xm = to_mont(x);
    Fq y;
    ok = g1_y_from_x(xm, ysign, &y);
    if (ok) {
      p.x = xm;
      p.y = y;
    }
  }
  if (!ok) atomicExch(err, 1);
  st_aff(out + i, p);
}

// amdzk_srs_check, CURVE: thread t < n tests g[t], thread n + t tests g_lagrange[t] (a basis that is not resident is null
// and its threads leave): coordinates below q, y^2 = x^3 + 3, not (0, 0). *first, preset to all ones, receives the smallest
// basis << 32 | index of an offending point. Memory-bound: four 16-byte loads and five products a point.
__global__ __launch_bounds__(256) void srs_check_curve_kernel(const G1Affine* g, const G1Affine* g_lagrange, size_t n, unsigned long long* first) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * n) return;
  const unsigned long long basis = t >= n ? 1 : 0, i = t - basis * n;
  const G1Affine* src = basis ? g_lagrange : g;
  if (!src) return;
  const G1Affine p = ld_aff(src + i);
  const bool ok = is_canonical(p.x) && is_canonical(p.y) && !p.is_inf() && sqr(p.y) == g1_curve_rhs(p.x);
  if (!ok) atomicMin(first, basis << 32 | i);
}

// amdzk_srs_check's scalar columns, n each, from E[i] = rho^i: colA = (E[0] ... E[n-2], 0), colB = (0, E[0] ... E[n-2]),
// colC = colE = E (colC then goes through the inverse NTT). A thread takes `chunk` consecutive i, as in powers_kernel.
__device__ __forceinline__ void st_fr(Fr* p, const Fr& v) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}
__global__ void srs_check_columns_kernel(Fr* colA, Fr* colB, Fr* colC, Fr* colE, Fr rho, size_t n, uint32_t chunk) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, start = t * chunk;
  if (start >= n) return;
  const size_t end = start + chunk < n ? start + chunk : n;
  Fr cur = pow_u64(rho, start);
  if (start == 0) st_fr(colB, Fr::zero());
  for (size_t i = start; i < end; i++) {
    st_fr(colC + i, cur);
    st_fr(colE + i, cur);
    if (i + 1 < n) {  // the pairs (g[i], g[i+1]) end at i = n - 2
      st_fr(colA + i, cur);
      st_fr(colB + i + 1, cur);
    } else {
      st_fr(colA + i, Fr::zero());
    }
    cur = mul(cur, rho);
  }
}
}  // namespace

size_t zk_srs_serialized_size(uint32_t k) { return 4 + 2 * ((size_t)32 << k) + 128; }

int zk_srs_write(amdzk_ctx* ctx, const amdzk_srs* s, const uint8_t g2[64], const uint8_t s_g2[64], uint8_t* out, size_t cap) {
  if (!s || !s->base[0] || !s->base[1] || !out) ZK_FAIL(ctx, AMDZK_E_INVALID, "srs_write: both bases must be resident");
  const size_t need = zk_srs_serialized_size(s->k);
  if (cap < need) ZK_FAIL(ctx, AMDZK_E_INVALID, "srs_write: buffer too small (%zu < %zu)", cap, need);
  uint8_t* d = nullptr;
  ZK_TRY(zk_ws_reserve(ctx, ZK_WS_STARTUP, 2 * s->n * 32, (void**)&d));
  dim3 grid((unsigned)((s->n + 255) / 256)), block(256);
  ZK_LAUNCH(ctx, "g1_compress", g1_compress_kernel, grid, block, 0, s->base[0], d, s->n);
  ZK_LAUNCH(ctx, "g1_compress", g1_compress_kernel, grid, block, 0, s->base[1], d + s->n * 32, s->n);
  uint32_t k = s->k;
  memcpy(out, &k, 4);
  ZK_HIP(ctx, hipMemcpyAsync(out + 4, d, 2 * s->n * 32, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  if (g2) memcpy(out + 4 + 2 * s->n * 32, g2, 64); else memset(out + 4 + 2 * s->n * 32, 0, 64);
  if (s_g2) memcpy(out + 4 + 2 * s->n * 32 + 64, s_g2, 64); else memset(out + 4 + 2 * s->n * 32 + 64, 0, 64);
  return AMDZK_OK;
}

int zk_srs_read(amdzk_ctx* ctx, const uint8_t* data, size_t len, amdzk_srs** out, uint8_t g2_out[64], uint8_t s_g2_out[64]) {
  if (!data || !out || len < 4) ZK_FAIL(ctx, AMDZK_E_INVALID, "srs_read: null or truncated input");
  uint32_t k;
  memcpy(&k, data, 4);
  if (k > 26) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "srs_read: k %u > 26", k);
  const size_t n = (size_t)1 << k;
  if (len < zk_srs_serialized_size(k)) ZK_FAIL(ctx, AMDZK_E_INVALID, "srs_read: %zu bytes given, %zu needed for k = %u", len, zk_srs_serialized_size(k), k);
  char* ws = nullptr;
  ZK_TRY(zk_ws_reserve(ctx, ZK_WS_STARTUP, 2 * n * 32 + 2 * n * sizeof(G1Affine) + 256, (void**)&ws));
  uint8_t* d_in = (uint8_t*)ws;
  G1Affine* pts = (G1Affine*)(ws + 2 * n * 32);
  int* d_err = (int*)(ws + 2 * n * 32 + 2 * n * sizeof(G1Affine));
  ZK_HIP(ctx, hipMemcpyAsync(d_in, data + 4, 2 * n * 32, hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(ctx, hipMemsetAsync(d_err, 0, sizeof(int), ctx->stream));
  ZK_LAUNCH(ctx, "g1_decompress", g1_decompress_kernel, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, d_in, pts, 2 * n, d_err);
  int herr = 0;
  ZK_HIP(ctx, hipMemcpyAsync(&herr, d_err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  if (herr) ZK_FAIL(ctx, AMDZK_E_INVALID, "srs_read: invalid point encoding (not on the curve or x >= q)");
  if (g2_out) memcpy(g2_out, data + 4 + 2 * n * 32, 64);
  if (s_g2_out) memcpy(s_g2_out, data + 4 + 2 * n * 32 + 64, 64);
  return srs_build(ctx, pts, pts + n, true, k, out);
}

// ---- amdzk_srs_check (include/amdzk.h states the checks, their order and the soundness bound): the curve test
// above, four scalar columns, the inverse NTT of one of them, the table MSM (A, B, C over g in one submission, E over
// g_lagrange), and one product of two pairings with g2 / s_g2 prepared and freed here.
namespace {
void jac_to_affine_words(const uint64_t jac[12], uint64_t out[8]) {  // zk_msm_finish's normal form: z = 1, or the identity
  const G1Jac* p = reinterpret_cast<const G1Jac*>(jac);
  if (p->z.is_zero()) memset(out, 0, 64);
  else memcpy(out, jac, 64);
}

int srs_check_run(amdzk_ctx* ctx, const amdzk_srs* s, const uint64_t g2[16], const uint64_t s_g2[16], uint32_t checks, const Fr& rho,
                  amdzk_srs_report* rep) {
  const size_t n = s->n;
  const G1Affine *g = s->base[AMDZK_BASIS_G], *gl = s->base[AMDZK_BASIS_G_LAGRANGE];
  {  // G2: host. The statuses are filled either way: POWERS depends on them.
    int st[2] = {0, 0};
    amdzk_g2_check(g2, &st[0]);
    amdzk_g2_check(s_g2, &st[1]);
    rep->g2_status[0] = (uint32_t)st[0], rep->g2_status[1] = (uint32_t)st[1];
    if (checks & AMDZK_SRS_CHECK_G2) {
      rep->ran |= AMDZK_SRS_CHECK_G2;
      if (st[0] || st[1]) rep->failed |= AMDZK_SRS_CHECK_G2;
    }
  }
  char* ws = nullptr;  // first offender (256 bytes) | colA[n] | colB[n] | colC[n] | colE[n]; not ZK_WS_STARTUP: workspace.hpp
  ZK_TRY(zk_ws_reserve(ctx, ZK_WS_STAGING, 256 + 4 * n * sizeof(Fr), (void**)&ws));
  unsigned long long* d_first = (unsigned long long*)ws;
  Fr *colA = (Fr*)(ws + 256), *colB = colA + n, *colC = colB + n, *colE = colC + n;
  if (checks & AMDZK_SRS_CHECK_CURVE) {
    unsigned long long first = ~0ull;
    ZK_HIP(ctx, hipMemsetAsync(d_first, 0xFF, sizeof(first), ctx->stream));
    ZK_LAUNCH(ctx, "srs_check_curve", srs_check_curve_kernel, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, g, gl, n, d_first);
    ZK_HIP(ctx, hipMemcpyAsync(&first, d_first, sizeof(first), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
    rep->ran |= AMDZK_SRS_CHECK_CURVE;
    if (first != ~0ull) {
      rep->failed |= AMDZK_SRS_CHECK_CURVE;
      rep->curve_basis = (uint32_t)(first >> 32);
      rep->curve_index = first & 0xFFFFFFFFull;
      return AMDZK_OK;  // the sums over off-curve points mean nothing
    }
  }
  const bool powers = (checks & AMDZK_SRS_CHECK_POWERS) && g && !rep->g2_status[0] && !rep->g2_status[1];
  if (!powers) return AMDZK_OK;  // and LAGRANGE is sound only given POWERS
  const bool lagrange = (checks & AMDZK_SRS_CHECK_LAGRANGE) && gl;
  const uint32_t chunk = 64;
  ZK_LAUNCH(ctx, "srs_check_columns", srs_check_columns_kernel, dim3((unsigned)(((n + chunk - 1) / chunk + 63) / 64)), dim3(64), 0, colA, colB, colC,
            colE, rho, n, chunk);
  if (lagrange) {
    const Fr omega_inv = inv(zkhost::fr_omega(s->k));
    uint64_t w[4];
    memcpy(w, omega_inv.l, 32);
    ZK_TRY(zk_ntt_dev(ctx, colC, s->k, w, AMDZK_NTT_SCALE_NINV, 1, n));
  }
  alignas(16) uint64_t jac[3 * 12];
  G1X* d_res = nullptr;
  ZK_TRY(zk_msm_dev_xyzz(ctx, s, AMDZK_BASIS_G, colA, lagrange ? 3 : 2, n, n, &d_res));
  ZK_TRY(zk_msm_finish(ctx, d_res, lagrange ? 3 : 2, jac));
  for (int j = 0; j < (lagrange ? 3 : 2); j++) jac_to_affine_words(jac + 12 * j, rep->points + 8 * j);
  G1Affine ab[2];  // A, -B
  memcpy(&ab[0], rep->points, 64);
  memcpy(&ab[1], rep->points + 8, 64);
  ab[1] = a_neg(ab[1]);
  rep->ran |= AMDZK_SRS_CHECK_POWERS;
  if (n > 1) {  // n = 1 has no pair (g[i], g[i+1]): passes vacuously
    bool ok = !ab[0].is_inf() && !ab[1].is_inf();
    if (ok) {
      amdzk_g2* q[2] = {nullptr, nullptr};  // e(A, s_g2) e(-B, g2)
      int r = amdzk_g2_prepare(ctx, s_g2, &q[0]);
      if (r == AMDZK_OK) r = amdzk_g2_prepare(ctx, g2, &q[1]);
      uint8_t one = 0;
      if (r == AMDZK_OK) r = zk_pairing_products(ctx, "srs_check", q, 2, ab, 1, &one, nullptr);
      (void)zk_quiet_if_refused(ctx, r);  // nothing reads the handles any more
      amdzk_g2_free(ctx, q[0]);
      amdzk_g2_free(ctx, q[1]);
      ZK_TRY(r);
      ok = one != 0;
    }
    if (!ok) {
      rep->failed |= AMDZK_SRS_CHECK_POWERS;
      return AMDZK_OK;
    }
  }
  if (!lagrange) return AMDZK_OK;
  ZK_TRY(zk_msm_dev_xyzz(ctx, s, AMDZK_BASIS_G_LAGRANGE, colE, 1, n, n, &d_res));
  ZK_TRY(zk_msm_finish(ctx, d_res, 1, jac));
  jac_to_affine_words(jac, rep->points + 24);
  rep->ran |= AMDZK_SRS_CHECK_LAGRANGE;
  if (memcmp(rep->points + 16, rep->points + 24, 64) != 0) rep->failed |= AMDZK_SRS_CHECK_LAGRANGE;
  return AMDZK_OK;
}
}  // namespace

int zk_srs_check(amdzk_ctx* ctx, const amdzk_srs* s, const uint64_t g2[16], const uint64_t s_g2[16], const amdzk_srs_check_opts* opts,
                 amdzk_srs_report* rep) {
  if (!s || !g2 || !s_g2 || !rep) ZK_FAIL(ctx, AMDZK_E_INVALID, "srs_check: null argument");
  if (opts && opts->size < sizeof(amdzk_srs_check_opts))
    ZK_FAIL(ctx, AMDZK_E_INVALID, "srs_check: amdzk_srs_check_opts.size is %zu, this library needs %zu", opts->size, sizeof(amdzk_srs_check_opts));
  const uint32_t all = AMDZK_SRS_CHECK_G2 | AMDZK_SRS_CHECK_CURVE | AMDZK_SRS_CHECK_POWERS | AMDZK_SRS_CHECK_LAGRANGE;
  const uint32_t checks = opts && opts->checks ? opts->checks : all;
  if (checks & ~all) ZK_FAIL(ctx, AMDZK_E_INVALID, "srs_check: unknown check bits 0x%x", checks & ~all);
  Fr rho;
  if (opts && opts->rho) {
    memcpy(rho.l, opts->rho, 32);
    if (!is_canonical(rho)) ZK_FAIL(ctx, AMDZK_E_INVALID, "srs_check: rho is not below the modulus (rho >= r)");
  } else {
    zkhost::ChaCha20Rng rng(opts ? opts->seed : 0);
    rho = rng.fr();
  }
  memset(rep, 0, sizeof(*rep));
  return zk_quiet_if_refused(ctx, srs_check_run(ctx, s, g2, s_g2, checks, rho, rep));  // whatever was enqueued is finished before the call returns
}

// ---- arithmetic::g_to_lagrange(g, k) and ParamsKZG::downsize(k) [UP]:
// g_lagrange = (1/n) * FFT_{omega^-1}(g) over the group — the same radix-2 network as the scalar NTT with
// every twiddle product a G1 scalar multiplication. Decimation in frequency on XYZZ points in HBM
// (k launches, one butterfly per thread), then one pass that scales by 1/n, normalises to affine and
// undoes the bit reversal. Start-up work only: n/2 * log n + n scalar multiplications.
namespace {
// canon: canonical (non-Montgomery) scalar; MSB-first double-and-add.
__device__ G1X x_scalar_mul(const G1X& p, const Fr& canon) {
  G1X acc = G1X::inf();
  int top = -1;
  for (int limb = 7; limb >= 0 && top < 0; limb--)
    if (canon.l[limb]) top = limb * 32 + 31 - __clz(canon.l[limb]);
#pragma unroll 1
  for (int b = top; b >= 0; b--) {
    acc = x_dbl(acc);
    if ((canon.l[b >> 5] >> (b & 31)) & 1) acc = x_add(acc, p);
  }
  return acc;
}
__global__ __launch_bounds__(256) void ecfft_load_kernel(const G1Affine* g, G1X* a, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) st_x(a + i, x_from_affine(ld_aff(g + i)));
}
// One DIF round: (u, v) at distance half -> (u + v, (u - v) * w^(pos << tw_shift)).
__global__ __launch_bounds__(256) void ecfft_round_kernel(G1X* a, size_t n, uint32_t half_log, const Fr* tw, uint32_t tw_shift) {
  size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n / 2) return;
  const size_t half = (size_t)1 << half_log, pos = j & (half - 1);
  const size_t i0 = ((j >> half_log) << (half_log + 1)) + pos, i1 = i0 + half;
  G1X u = ld_x(a + i0), v = ld_x(a + i1);
  st_x(a + i0, x_add(u, v));
  G1X d = x_add(u, x_neg(v));
  if (pos != 0) {
    const uint4* q = reinterpret_cast<const uint4*>(tw + (pos << tw_shift));
    uint4 lo = q[0], hi = q[1];
    Fr w;
    w.l[0] = lo.x; w.l[1] = lo.y; w.l[2] = lo.z; w.l[3] = lo.w;
    w.l[4] = hi.x; w.l[5] = hi.y; w.l[6] = hi.z; w.l[7] = hi.w;
    d = x_scalar_mul(d, from_mont(w));
  }
  st_x(a + i1, d);
}
__global__ __launch_bounds__(256) void ecfft_finish_kernel(const G1X* a, G1Affine* out, size_t n, uint32_t k, Fr ninv_canon) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  size_t r = k ? (size_t)(__brevll((unsigned long long)i) >> (64 - k)) : 0;
  st_aff(out + r, x_to_affine(x_scalar_mul(ld_x(a + i), ninv_canon)));
}

// d_g, d_out: n affine points on the device (may not alias); d_xyzz: n G1X; d_tw: max(n/2, 1) Fr.
int ecfft_to_lagrange(amdzk_ctx* ctx, const G1Affine* d_g, uint32_t k, const Fr& omega_inv, const Fr& n_inv, G1X* d_xyzz, Fr* d_tw,
                      G1Affine* d_out) {
  const size_t n = (size_t)1 << k;
  dim3 eg((unsigned)((n + 255) / 256)), hg((unsigned)((n / 2 + 255) / 256)), eb(256);
  ZK_LAUNCH(ctx, "ecfft_load", ecfft_load_kernel, eg, eb, 0, d_g, d_xyzz, n);
  if (k > 0) {
    const uint32_t chunk = 64;
    dim3 pg((unsigned)(((n / 2 + chunk - 1) / chunk + 63) / 64)), pb(64);
    ZK_LAUNCH(ctx, "srs_powers", powers_kernel, pg, pb, 0, d_tw, omega_inv, n / 2, chunk);
    for (uint32_t s = 0; s < k; s++)
      ZK_LAUNCH(ctx, "ecfft_round", ecfft_round_kernel, hg, eb, 0, d_xyzz, n, k - 1 - s, (const Fr*)d_tw, s);
  }
  ZK_LAUNCH(ctx, "ecfft_finish", ecfft_finish_kernel, eg, eb, 0, (const G1X*)d_xyzz, d_out, n, k, from_mont(n_inv));
  return AMDZK_OK;
}
}  // namespace

int zk_g_to_lagrange(amdzk_ctx* ctx, const uint64_t* g, uint32_t k, const uint64_t omega_inv[4], const uint64_t n_inv[4], uint64_t* out) {
  if (!g || !out) ZK_FAIL(ctx, AMDZK_E_INVALID, "g_to_lagrange: null argument");
  if (k > 26) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "g_to_lagrange: k %u > 26", k);
  const size_t n = (size_t)1 << k;
  Fr wi, ni;
  memcpy(wi.l, omega_inv, 32);
  memcpy(ni.l, n_inv, 32);
  char* ws = nullptr;  // g[n] | gl[n] | xyzz[n] | tw[n/2]
  ZK_TRY(zk_ws_reserve(ctx, ZK_WS_STARTUP, 2 * n * sizeof(G1Affine) + n * sizeof(G1X) + (n / 2 + 1) * sizeof(Fr), (void**)&ws));
  G1Affine* dg = (G1Affine*)ws;
  G1Affine* dl = dg + n;
  G1X* dx = (G1X*)(dl + n);
  Fr* tw = (Fr*)(dx + n);
  ZK_HIP(ctx, hipMemcpyAsync(dg, g, n * sizeof(G1Affine), hipMemcpyHostToDevice, ctx->stream));
  ZK_TRY(ecfft_to_lagrange(ctx, dg, k, wi, ni, dx, tw, dl));
  ZK_HIP(ctx, hipMemcpyAsync(out, dl, n * sizeof(G1Affine), hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  return AMDZK_OK;
}

int zk_srs_downsize(amdzk_ctx* ctx, const amdzk_srs* srs, uint32_t new_k, const uint64_t omega_inv[4], const uint64_t n_inv[4],
                    amdzk_srs** out) {
  if (!srs || !out) ZK_FAIL(ctx, AMDZK_E_INVALID, "srs_downsize: null argument");
  if (new_k > srs->k) ZK_FAIL(ctx, AMDZK_E_INVALID, "srs_downsize: k %u > params k %u", new_k, srs->k);
  if (!srs->base[0]) ZK_FAIL(ctx, AMDZK_E_INVALID, "srs_downsize: params hold no monomial basis g");
  const size_t n = (size_t)1 << new_k;
  Fr wi, ni;
  memcpy(wi.l, omega_inv, 32);
  memcpy(ni.l, n_inv, 32);
  char* ws = nullptr;  // gl[n] | xyzz[n] | tw[n/2]
  ZK_TRY(zk_ws_reserve(ctx, ZK_WS_STARTUP, n * sizeof(G1Affine) + n * sizeof(G1X) + (n / 2 + 1) * sizeof(Fr), (void**)&ws));
  G1Affine* dl = (G1Affine*)ws;
  G1X* dx = (G1X*)(dl + n);
  Fr* tw = (Fr*)(dx + n);
  ZK_TRY(ecfft_to_lagrange(ctx, srs->base[0], new_k, wi, ni, dx, tw, dl));
  return srs_build(ctx, srs->base[0], dl, true, new_k, out);
}

// ---- the prefix-sum basis S_i = g_lagrange[0] + ... + g_lagrange[i] (AMDZK_BASIS_G_LAGRANGE_PREFIX).
// Abel summation: sum_i z[i] L_i = sum_i d[i] S_i with d[i] = z[i] - z[i+1], d[n-1] = z[n-1] — a column that is constant
// over long runs of rows (a permutation product away from the copy cycles) has as few non-zero d[i] as it has jumps, and
// the counting sort drops zero scalars before they become entries. S depends on the SRS alone.
// An EC prefix scan in chunks of PREFIX_CHUNK: one thread sums a chunk serially (its total), the totals are scanned the same
// way one level up (in place, XYZZ) until one chunk is left, and on the way down every thread redoes its chunk from the
// scanned total in front of it. Two additions per point and one inversion (the affine form the window table is built
// from); start-up work, once per SRS. x_add / x_add_affine are complete (equal points, opposite points, the identity).
namespace {
constexpr uint32_t PREFIX_CHUNK = 16;
__device__ __forceinline__ G1X prefix_step(const G1X& acc, const G1Affine* in, size_t i) { return x_add_affine(acc, ld_aff(in + i)); }
__device__ __forceinline__ G1X prefix_step(const G1X& acc, const G1X* in, size_t i) { return x_add(acc, ld_x(in + i)); }
// totals[t] = in[t * CHUNK] + ... + in[min((t + 1) * CHUNK, m) - 1]
template <class P>
__global__ __launch_bounds__(64) void prefix_chunk_total_kernel(const P* in, size_t m, G1X* totals) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, lo = t * PREFIX_CHUNK;
  if (lo >= m) return;
  const size_t hi = lo + PREFIX_CHUNK < m ? lo + PREFIX_CHUNK : m;
  G1X acc = G1X::inf();
#pragma unroll 1
  for (size_t i = lo; i < hi; i++) acc = prefix_step(acc, in, i);
  st_x(totals + t, acc);
}
// Inclusive scan of chunk t, started from carry[t - 1] (the scanned totals; null: one chunk, nothing in front).
// XYZZ, in place (the upper levels): a[i] <- carry + a[lo] + ... + a[i].
__global__ __launch_bounds__(64) void prefix_apply_x_kernel(G1X* a, size_t m, const G1X* carry) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, lo = t * PREFIX_CHUNK;
  if (lo >= m) return;
  const size_t hi = lo + PREFIX_CHUNK < m ? lo + PREFIX_CHUNK : m;
  G1X acc = (carry && t) ? ld_x(carry + t - 1) : G1X::inf();
#pragma unroll 1
  for (size_t i = lo; i < hi; i++) {
    acc = prefix_step(acc, a, i);
    st_x(a + i, acc);
  }
}
// The bottom level: affine in, affine out (one inversion per point, as ecfft_finish_kernel does).
__global__ __launch_bounds__(64) void prefix_apply_affine_kernel(const G1Affine* in, size_t m, const G1X* carry, G1Affine* out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, lo = t * PREFIX_CHUNK;
  if (lo >= m) return;
  const size_t hi = lo + PREFIX_CHUNK < m ? lo + PREFIX_CHUNK : m;
  G1X acc = (carry && t) ? ld_x(carry + t - 1) : G1X::inf();
#pragma unroll 1
  for (size_t i = lo; i < hi; i++) {
    acc = prefix_step(acc, in, i);
    st_aff(out + i, x_to_affine(acc));
  }
}
inline size_t prefix_chunks(size_t m) { return (m + PREFIX_CHUNK - 1) / PREFIX_CHUNK; }
inline dim3 prefix_grid(size_t m) { return dim3((unsigned)((prefix_chunks(m) + 63) / 64)); }

// d_out[i] = d_in[0] + ... + d_in[i], n affine points each (may not alias), on ctx's stream.
int ec_prefix_sums(amdzk_ctx* ctx, const G1Affine* d_in, size_t n, G1Affine* d_out) {
  // the levels' totals, one behind the other: level l holds prefix_chunks(size of level l - 1) points
  std::vector<size_t> sizes;
  size_t total = 0;
  for (size_t m = n; m > PREFIX_CHUNK;) {
    m = prefix_chunks(m);
    sizes.push_back(m);
    total += m;
  }
  G1X* tot = nullptr;
  if (total) ZK_TRY(zk_ws_reserve(ctx, ZK_WS_STARTUP, total * sizeof(G1X), (void**)&tot));
  std::vector<G1X*> lvl;
  for (size_t l = 0, o = 0; l < sizes.size(); o += sizes[l], l++) lvl.push_back(tot + o);
  const dim3 block(64);
  // up: chunk totals of every level that has more than one chunk
  for (size_t l = 0; l < sizes.size(); l++) {
    if (l == 0) ZK_LAUNCH(ctx, "srs_prefix_total", prefix_chunk_total_kernel<G1Affine>, prefix_grid(n), block, 0, d_in, n, lvl[0]);
    else ZK_LAUNCH(ctx, "srs_prefix_total", prefix_chunk_total_kernel<G1X>, prefix_grid(sizes[l - 1]), block, 0, (const G1X*)lvl[l - 1], sizes[l - 1], lvl[l]);
  }
  // down: the top level is one chunk; every level below starts its chunks from the scanned totals above it
  for (size_t l = sizes.size(); l-- > 0;)
    ZK_LAUNCH(ctx, "srs_prefix_apply", prefix_apply_x_kernel, prefix_grid(sizes[l]), block, 0, lvl[l], sizes[l],
              l + 1 < sizes.size() ? (const G1X*)lvl[l + 1] : (const G1X*)nullptr);
  ZK_LAUNCH(ctx, "srs_prefix_apply", prefix_apply_affine_kernel, prefix_grid(n), block, 0, d_in, n,
            sizes.empty() ? (const G1X*)nullptr : (const G1X*)lvl[0], d_out);
  return AMDZK_OK;
}
}  // namespace

int zk_srs_ensure_prefix(amdzk_ctx* ctx, const amdzk_srs* srs_c) {
  if (!srs_c) ZK_FAIL(ctx, AMDZK_E_INVALID, "srs: null argument");
  amdzk_srs* s = const_cast<amdzk_srs*>(srs_c);  // the derived slot is the one thing a key adds to the parameters it is made on
  const int P = AMDZK_BASIS_G_LAGRANGE_PREFIX;
  std::lock_guard<std::mutex> lock(s->prefix_guard);
  if (s->table[P]) return AMDZK_OK;
  if (!s->base[AMDZK_BASIS_G_LAGRANGE]) ZK_FAIL(ctx, AMDZK_E_INVALID, "srs: the prefix-sum basis needs g_lagrange, which was not uploaded");
  const auto t0 = std::chrono::steady_clock::now();
  G1Affine *base = nullptr, *table = nullptr;
  size_t refused = 0;
  const hipError_t e = srs_alloc_slot(s, &base, &table, &refused);
  if (e != hipSuccess)
    ZK_FAIL(ctx, AMDZK_E_NOMEM, "srs: hipMalloc(%zu) for the prefix-sum basis failed: %s", srs_basis_bytes(s), hipGetErrorString(e));
  int r = ec_prefix_sums(ctx, s->base[AMDZK_BASIS_G_LAGRANGE], s->n, base);
  if (r == AMDZK_OK) r = zk_msm_fill_table(ctx, base, table, s->n, s->c, s->W);
  if (r == AMDZK_OK && zk_host_wait(ctx, ctx->stream) != hipSuccess) {
    ctx->err = "srs: building the prefix-sum basis failed on the device";
    r = AMDZK_E_HIP;
  }
  if (r != AMDZK_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    hipFree(table);
    hipFree(base);
    return r;
  }
  s->base[P] = base;
  s->table[P] = table;  // published last: complete on the device
  s->prefix_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (getenv("AMDZK_TRACE_TIME"))
    fprintf(stderr, "[amdzk-time] srs prefix-sum basis k=%u: %.3f ms, %zu bytes\n", s->k, s->prefix_build_ms, srs_basis_bytes(s));
  return AMDZK_OK;
}
