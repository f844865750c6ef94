// Poseidon over Fr on the device (include/amdzk.h "Poseidon over Fr"): the kernels and the entry points.
// The host half — the validation, the plain statement of the semantics and the lane step the kernels run — is poseidon.hpp.
//
//   pos_permute_kernel — n states permuted in place.
//   pos_sponge_kernel  — n sponges of their own lengths: absorb, permute, ..., digest.
//
// One sponge per group of eight adjacent lanes, state element i in lane i of its group, lanes >= t idle: a wavefront carries
// eight sponges, a block 32. A sponge is a chain of dependent permutations, and what the reference hashes is few long
// sponges: this layout makes a round about four products deep (two squarings and a product for x^5, then the lane's own row
// of M·s as ONE sum of products with one reduction) instead of 3t + t^2 in a lane that holds a whole state.
// The state stays on 29-bit limbs in Montgomery radix 2^261 from entry to exit (pos::lane_enter / lane_exit). The round
// constants lie in LDS (packed, 32 bytes each), copied once per block; a lane's MDS row lies in its registers as limbs.
// Lanes >= t and the groups beyond n take part in every cross-lane operation and every barrier — no lane leaves early — but
// load and store nothing: they carry a copy of a valid element through the same arithmetic, inside the same bounds.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "common.hpp"
#include "poseidon.hpp"

using namespace bn254;

struct amdzk_poseidon {
  pos::Compiled c;
  int device = 0;
  Fr* d_k = nullptr;
  // grow-only: the lengths of a ragged call, and the host form's staged inputs and digests
  uint32_t* d_lens = nullptr;
  size_t lens_cap = 0;
  Fr* d_in = nullptr;
  size_t in_cap = 0;
  Fr* d_out = nullptr;
  size_t out_cap = 0;
};

namespace {

__device__ __forceinline__ Fr pos_ld(const Fr* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 lo = q[0], hi = q[1];
  Fr r;
  r.l[0] = lo.x; r.l[1] = lo.y; r.l[2] = lo.z; r.l[3] = lo.w;
  r.l[4] = hi.x; r.l[5] = hi.y; r.l[6] = hi.z; r.l[7] = hi.w;
  return r;
}
__device__ __forceinline__ void pos_st(Fr* p, const Fr& v) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

struct PosArgs {
  const Fr* k;  // pos::Compiled::k
  uint32_t t, rate, r_f, r_p;
};

// What every thread of a block holds before its first round: the round constants in LDS, its MDS row in registers.
struct PosLane {
  uint32_t lane;              // within the group
  uint32_t el;                // the state element whose constants this lane reads: lane, or t - 1 in the idle lanes
  uint32_t row[pos::MAX_T * 9];
};

__device__ __forceinline__ void pos_setup(const PosArgs& A, Fr* lds_rc, PosLane& L) {
  const uint32_t n_rc = (A.r_f + A.r_p) * A.t;  // <= pos::MAX_RC
  for (uint32_t i = threadIdx.x; i < n_rc; i += pos::BLOCK) pos_st(lds_rc + i, pos_ld(A.k + i));
  L.lane = threadIdx.x & (pos::GROUP - 1);
  L.el = L.lane < A.t ? L.lane : A.t - 1;
#pragma unroll
  for (uint32_t j = 0; j < pos::MAX_T; j++) {
    Fr29 m;
#pragma unroll
    for (int i = 0; i < 9; i++) m.l[i] = 0;
    if (j < A.t) m = fr29_unpack(pos_ld(A.k + n_rc + L.el * A.t + j));
#pragma unroll
    for (int i = 0; i < 9; i++) L.row[9 * j + i] = m.l[i];
  }
  __syncthreads();
}

// One permutation of the group's state; s: this lane's element, below 4p, normalised. Result below 2p, normalised.
__device__ __forceinline__ Fr29 pos_permute_lane(const PosArgs& A, const Fr* lds_rc, const PosLane& L, Fr29 s) {
  const uint32_t rounds = A.r_f + A.r_p, half = A.r_f / 2;
#pragma unroll 1
  for (uint32_t rho = 0; rho < rounds; rho++) {
    const bool full = rho < half || rho >= half + A.r_p;
    const Fr29 y = pos::lane_sbox(L.lane, s, fr29_unpack(lds_rc[rho * A.t + L.el]), full);
    s = pos::lane_mix(A.t, L.row, [&](uint32_t j) {  // element j of the group, limb by limb
      Fr29 v;
#pragma unroll
      for (int i = 0; i < 9; i++) v.l[i] = (uint32_t)__shfl((int)y.l[i], (int)j, (int)pos::GROUP);
      return v;
    });
  }
  return s;
}

__global__ __launch_bounds__(pos::BLOCK) void pos_permute_kernel(PosArgs A, Fr* __restrict__ states, size_t stride, uint32_t n) {
  extern __shared__ uint4 pos_lds[];
  Fr* lds_rc = reinterpret_cast<Fr*>(pos_lds);
  PosLane L;
  pos_setup(A, lds_rc, L);
  const uint32_t group = blockIdx.x * (pos::BLOCK / pos::GROUP) + threadIdx.x / pos::GROUP;
  const bool live = group < n && L.lane < A.t;
  Fr* mine = states + (size_t)group * stride + L.lane;
  Fr29 s = f29_one<Fr29P>();  // idle lanes: any value within the bounds
  if (live) s = pos::lane_enter(pos_ld(mine));
  s = pos_permute_lane(A, lds_rc, L, s);
  if (live) pos_st(mine, pos::lane_exit(s));
}

// lens: n lengths, or nullptr = every sponge has `len` inputs. Lengths below 2^31.
__global__ __launch_bounds__(pos::BLOCK) void pos_sponge_kernel(PosArgs A, const Fr* __restrict__ in, size_t in_stride, const uint32_t* __restrict__ lens,
                                                                uint32_t len, uint32_t n, Fr* __restrict__ out, size_t out_stride) {
  extern __shared__ uint4 pos_lds[];
  Fr* lds_rc = reinterpret_cast<Fr*>(pos_lds);
  PosLane L;
  pos_setup(A, lds_rc, L);
  const uint32_t group = blockIdx.x * (pos::BLOCK / pos::GROUP) + threadIdx.x / pos::GROUP;
  const bool live = group < n && L.lane < A.t;
  const uint32_t my_len = group < n ? (lens ? lens[group] : len) : 0u;
  const uint32_t count = group < n ? my_len / A.rate + 1 : 0u;  // this group's permutations
  uint32_t longest = count;                                     // ... and the wavefront's
#pragma unroll
  for (int m = (int)pos::GROUP; m < 64; m <<= 1) longest = max(longest, (uint32_t)__shfl_xor((int)longest, m));
  const Fr* mine = in + (size_t)group * in_stride;
  Fr29 s = fr29_unpack(pos_ld(A.k + (size_t)(A.r_f + A.r_p) * A.t + A.t * A.t + L.el));  // the initial state: canonical
#pragma unroll 1
  for (uint32_t c = 0; c < longest; c++) {
    if (live && c < count) s = pos::lane_absorb(L.lane, A.rate, s, c, my_len, [&](uint32_t a) { return pos_ld(mine + a); });
    s = pos_permute_lane(A, lds_rc, L, s);
    // a group that is through goes on permuting what it has (within the bounds) beside the longer ones of its wavefront
    if (live && L.lane == 1 && c + 1 == count) pos_st(out + (size_t)group * out_stride, pos::lane_exit(s));
  }
}

uint32_t pos_blocks(size_t n) { return (uint32_t)((n + pos::BLOCK / pos::GROUP - 1) / (pos::BLOCK / pos::GROUP)); }
size_t pos_lds_bytes(const pos::Compiled& c) { return (size_t)c.rounds() * c.t * sizeof(Fr); }
PosArgs pos_args(const amdzk_poseidon* p) { return PosArgs{p->d_k, p->c.t, p->c.rate, p->c.r_f, p->c.r_p}; }

int pos_grow(amdzk_ctx* ctx, void** p, size_t* cap, size_t bytes) {
  if (*cap >= bytes) return AMDZK_OK;
  if (*p) {
    ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
    ZK_HIP(ctx, hipFree(*p));
    *p = nullptr;
    *cap = 0;
  }
  if (hipMalloc(p, bytes) != hipSuccess) {
    *p = nullptr;
    ZK_FAIL(ctx, AMDZK_E_NOMEM, "poseidon: hipMalloc(%zu) failed", bytes);
  }
  *cap = bytes;
  return AMDZK_OK;
}

void pos_release(amdzk_poseidon* p) {
  for (void* q : {(void*)p->d_k, (void*)p->d_lens, (void*)p->d_in, (void*)p->d_out})
    if (q) (void)hipFree(q);
  delete p;
}

// a caller's device pointer: amdzk_ptr_check_affinity's test, refused as a bad argument
int pos_ptr(amdzk_ctx* ctx, const void* p, const char* what) {
  const int r = zk_ptr_on_device(ctx, p, what);
  if (r == AMDZK_OK) return r;
  (void)hipGetLastError();  // a pointer the runtime does not know leaves its error behind
  ctx->err = "poseidon: " + ctx->err;
  return r == AMDZK_E_HIP ? AMDZK_E_INVALID : r;
}

int pos_handle(amdzk_ctx* ctx, const amdzk_poseidon* p) {
  if (!p) ZK_FAIL(ctx, AMDZK_E_INVALID, "poseidon: null argument");
  if (p->device != ctx->device) ZK_FAIL(ctx, AMDZK_E_INVALID, "poseidon: the spec was compiled on device %d, the ctx is on device %d", p->device, ctx->device);
  return AMDZK_OK;
}

// The lengths of a call: n of them at lens, or all `len`. Refuses what the kernel's 32-bit counters do not hold.
int pos_longest(amdzk_ctx* ctx, const size_t* lens, size_t len, size_t n, size_t* longest) {
  if (n == 0) ZK_FAIL(ctx, AMDZK_E_INVALID, "poseidon: n = 0");
  if (n > pos::MAX_N) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "poseidon: %zu sponges in one call (2^31 or more)", n);
  size_t m = lens ? 0 : len;
  for (size_t b = 0; lens && b < n; b++) m = std::max(m, lens[b]);
  if (m > pos::MAX_N) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "poseidon: a length of %zu (2^31 or more)", m);
  *longest = m;
  return AMDZK_OK;
}

// everything the _dev form refuses has been refused by the caller of this
int pos_hash_launch(amdzk_ctx* ctx, amdzk_poseidon* p, const Fr* d_in, size_t in_stride, const size_t* lens, size_t len, size_t n, Fr* d_out,
                    size_t out_stride) {
  const uint32_t* d_lens = nullptr;
  std::vector<uint32_t> l32;
  if (lens) {
    ZK_TRY(pos_grow(ctx, (void**)&p->d_lens, &p->lens_cap, n * sizeof(uint32_t)));
    if (ctx->ws_poison) ZK_TRY(zk_ws_poison_fill(ctx, p->d_lens, n * sizeof(uint32_t)));  // AMDZK_WS_POISON (workspace.hpp)
    l32.assign(lens, lens + n);
    ZK_HIP(ctx, hipMemcpyAsync(p->d_lens, l32.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    d_lens = p->d_lens;
  }
  ZK_LAUNCH(ctx, "pos_sponge", pos_sponge_kernel, dim3(pos_blocks(n)), dim3(pos::BLOCK), pos_lds_bytes(p->c), pos_args(p), d_in, in_stride, d_lens,
            (uint32_t)len, (uint32_t)n, d_out, out_stride);
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));  // l32 is read until here
  return AMDZK_OK;
}

}  // namespace

extern "C" int amdzk_poseidon_check_desc(const amdzk_poseidon_desc* desc, char* msg, size_t msg_cap) {
  pos::Spec s;
  std::string err;
  const int rc = pos::check(desc, s, err);
  if (msg && msg_cap) snprintf(msg, msg_cap, "%s", err.c_str());
  return rc;
}

extern "C" int amdzk_poseidon_compile(amdzk_ctx* ctx, const amdzk_poseidon_desc* desc, amdzk_poseidon** out) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  if (!desc || !out) ZK_FAIL(ctx, AMDZK_E_INVALID, "poseidon: null argument");
  *out = nullptr;
  pos::Spec s;
  std::string err;
  const int rc = pos::check(desc, s, err);
  if (rc != AMDZK_OK) ZK_FAIL(ctx, rc, "%s", err.c_str());
  amdzk_poseidon* p = new amdzk_poseidon();
  p->c = pos::compile(s);
  p->device = ctx->device;
  const size_t bytes = p->c.k.size() * sizeof(Fr);
  if (hipMalloc((void**)&p->d_k, bytes) != hipSuccess) {
    p->d_k = nullptr;
    pos_release(p);
    ZK_FAIL(ctx, AMDZK_E_NOMEM, "poseidon: hipMalloc(%zu) failed", bytes);
  }
  if (hipMemcpy(p->d_k, p->c.k.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
    pos_release(p);
    ZK_FAIL(ctx, AMDZK_E_HIP, "poseidon: the upload of the constants failed");
  }
  *out = p;
  return AMDZK_OK;
}

extern "C" void amdzk_poseidon_free(amdzk_ctx* ctx, amdzk_poseidon* p) {
  ZK_ENTER(ctx);
  if (!p) return;
  if (ctx) (void)zk_host_wait(ctx, ctx->stream);
  pos_release(p);
}

extern "C" int amdzk_poseidon_permute_dev(amdzk_ctx* ctx, amdzk_poseidon* p, void* d_states, size_t n_states, size_t state_stride) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  ZK_TRY(pos_handle(ctx, p));
  if (!d_states) ZK_FAIL(ctx, AMDZK_E_INVALID, "poseidon: null argument");
  if (n_states == 0) ZK_FAIL(ctx, AMDZK_E_INVALID, "poseidon: n_states = 0");
  if (n_states > pos::MAX_N) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "poseidon: %zu states in one call (2^31 or more)", n_states);
  if (state_stride < p->c.t) ZK_FAIL(ctx, AMDZK_E_INVALID, "poseidon: state_stride %zu < t = %u", state_stride, p->c.t);
  if (state_stride > SIZE_MAX / sizeof(Fr) / n_states) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "poseidon: %zu states of stride %zu do not fit size_t", n_states, state_stride);
  ZK_TRY(pos_ptr(ctx, d_states, "d_states"));
  ZK_LAUNCH(ctx, "pos_permute", pos_permute_kernel, dim3(pos_blocks(n_states)), dim3(pos::BLOCK), pos_lds_bytes(p->c), pos_args(p), (Fr*)d_states,
            state_stride, (uint32_t)n_states);
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  return AMDZK_OK;
}

extern "C" int amdzk_poseidon_hash_dev(amdzk_ctx* ctx, amdzk_poseidon* p, const void* d_inputs, size_t input_stride, const size_t* lens, size_t len,
                                       size_t n, void* d_out, size_t out_stride) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  ZK_TRY(pos_handle(ctx, p));
  if (!d_out) ZK_FAIL(ctx, AMDZK_E_INVALID, "poseidon: null argument");
  size_t longest = 0;
  ZK_TRY(pos_longest(ctx, lens, len, n, &longest));
  if (longest && !d_inputs) ZK_FAIL(ctx, AMDZK_E_INVALID, "poseidon: null argument");
  if (input_stride < longest) ZK_FAIL(ctx, AMDZK_E_INVALID, "poseidon: input_stride %zu < the longest length %zu", input_stride, longest);
  if (out_stride == 0) ZK_FAIL(ctx, AMDZK_E_INVALID, "poseidon: out_stride = 0");
  if (input_stride > SIZE_MAX / sizeof(Fr) / n || out_stride > SIZE_MAX / sizeof(Fr) / n)
    ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "poseidon: %zu sponges of strides %zu and %zu do not fit size_t", n, input_stride, out_stride);
  ZK_TRY(pos_ptr(ctx, d_inputs, "d_inputs"));
  ZK_TRY(pos_ptr(ctx, d_out, "d_out"));
  return zk_quiet_if_refused(ctx, pos_hash_launch(ctx, p, (const Fr*)d_inputs, input_stride, lens, len, n, (Fr*)d_out, out_stride));
}

extern "C" int amdzk_poseidon_hash(amdzk_ctx* ctx, amdzk_poseidon* p, const uint64_t* const* inputs, const size_t* lens, size_t n, uint64_t* out) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  ZK_TRY(pos_handle(ctx, p));
  if (!inputs || !lens || !out) ZK_FAIL(ctx, AMDZK_E_INVALID, "poseidon: null argument");
  size_t longest = 0;
  ZK_TRY(pos_longest(ctx, lens, 0, n, &longest));
  for (size_t b = 0; b < n; b++) {
    if (lens[b] && !inputs[b]) ZK_FAIL(ctx, AMDZK_E_INVALID, "poseidon: inputs[%zu] is null", b);
    for (size_t a = 0; a < lens[b]; a++)
      if (!is_canonical(pos::load_fr(inputs[b], a))) ZK_FAIL(ctx, AMDZK_E_INVALID, "poseidon: input %zu of sponge %zu is not below the modulus", a, b);
  }
  const size_t stride = std::max<size_t>(longest, 1);
  if (stride > SIZE_MAX / sizeof(Fr) / n) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "poseidon: %zu sponges of up to %zu inputs do not fit size_t", n, longest);
  ZK_TRY(pos_grow(ctx, (void**)&p->d_in, &p->in_cap, n * stride * sizeof(Fr)));
  ZK_TRY(pos_grow(ctx, (void**)&p->d_out, &p->out_cap, n * sizeof(Fr)));
  if (ctx->ws_poison) {  // AMDZK_WS_POISON (workspace.hpp): the staged inputs keep the last call's values between the sponges' ends and the stride
    ZK_TRY(zk_ws_poison_fill(ctx, p->d_in, n * stride * sizeof(Fr)));
    ZK_TRY(zk_ws_poison_fill(ctx, p->d_out, n * sizeof(Fr)));
  }
  int rc = [&]() -> int {
    for (size_t b = 0; b < n; b++)
      if (lens[b]) ZK_HIP(ctx, hipMemcpyAsync(p->d_in + b * stride, inputs[b], lens[b] * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    ZK_TRY(pos_hash_launch(ctx, p, p->d_in, stride, lens, 0, n, p->d_out, 1));
    ZK_HIP(ctx, hipMemcpyAsync(out, p->d_out, n * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
    return AMDZK_OK;
  }();
  return zk_quiet_if_refused(ctx, rc);
}
