// Device-side unit harness for csrc/fp29.cuh and the device-only branches of csrc/bn254.cuh (tests/test_gpu_field_ops.py).
//
// The asm products of fp29_asm.inc, the 8 x 32-bit CIOS mul and the Fermat inv exist only in the device compile; this
// program runs them in isolation, built with the library's own flags (tests/native/Makefile reads them from
// csrc/Makefile), and includes nothing of the library but the two headers. It computes and judges nothing itself:
//   fp29_device_check <cases.bin> <results.bin>
// reads records {function id, field, aux, words used, data[IN_WORDS]} that tests/fp29_model.py wrote, runs each record
// in REPLICAS lanes of different wavefronts (one wavefront per workgroup; neighbouring lanes hold different records) and
// writes OUT_WORDS result words per record and replica. Python compares them with the model.
//
// Three compile contexts surround the asm block: (i) one product per thread, operands straight from memory (OpMul, OpSqr);
// (ii) dependent chains, eight blocks back to back between two stores (OpMulChain, OpSqrChain, OpMul2Chain); (iii) the
// point formulas (OpDblAffine ... OpAddChain), four live 9-limb values around every block; (iv) the quad formulas, selects and
// DPP moves around every block.
//
// The quad formulas of csrc/fp29_quad.cuh (OpDblQuad, OpAddQuad, OpQuadChain) take one QUAD of lanes per record: lane
// `role` = t & 3 calls the formula with its role, every lane writes the point it ends with, neighbouring quads of a wavefront
// hold different records (different branches), and a record whose aux has bit 0 set sits out: its quad returns before the
// call, so that the DPP moves of the quads beside it run with idle neighbours, as in the rounds of msm_rowcol_quad_kernel.
//
// Exit status: 0 results written; 2 HIP error; 3 not a gfx950 device; 4 malformed case file.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "../../anon-aadhaar-halo2_amd/csrc/fp29.cuh"
#include "../../anon-aadhaar-halo2_amd/csrc/fp29_quad.cuh"
using namespace bn254;

constexpr uint32_t MAGIC = 0x43393246u;  // "F29C"
constexpr uint32_t IN_WORDS = 112, OUT_WORDS = 320, REC_WORDS = 4 + IN_WORDS, REPLICAS = 2, WAVE = 64;
constexpr int CHAIN_STEPS = 64, CHAIN_EVERY = 8;
constexpr uint32_t FIRST_QUAD_FUNC = 29, AUX_SIT_OUT = 1;  // F_DBL_QUAD ... of tests/fp29_model.py: one record per quad
constexpr int QUAD_CHAIN_STEPS = 16, QUAD_CHAIN_EVERY = 4;

#define HIP_OK(call)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      fprintf(stderr, "HIP error %s at %s:%d: %s\n", hipGetErrorName(e_), __FILE__, __LINE__, #call); \
      exit(2);                                                                               \
    }                                                                                        \
  } while (0)

template <class P> __device__ __forceinline__ Fp29<P> ld9(const uint32_t* d) {
  Fp29<P> r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = d[i];
  return r;
}
template <class P> __device__ __forceinline__ void st9(uint32_t* o, const Fp29<P>& v) {
#pragma unroll
  for (int i = 0; i < 9; i++) o[i] = v.l[i];
}
template <class B> __device__ __forceinline__ Fp<B> ld8(const uint32_t* d) {
  Fp<B> r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.l[i] = d[i];
  return r;
}
template <class B> __device__ __forceinline__ void st8(uint32_t* o, const Fp<B>& v) {
#pragma unroll
  for (int i = 0; i < 8; i++) o[i] = v.l[i];
}
__device__ __forceinline__ G1X29 ldpt(const uint32_t* d) {
  G1X29 r;
  r.x = ld9<Fq29P>(d);
  r.y = ld9<Fq29P>(d + 9);
  r.zz = ld9<Fq29P>(d + 18);
  r.zzz = ld9<Fq29P>(d + 27);
  return r;
}
// raw XYZZ (36 words), then the packed radix-2^256 form the callers read (32 words)
__device__ __forceinline__ void stpt(uint32_t* o, const G1X29& r, bool packed) {
  st9(o, r.x);
  st9(o + 9, r.y);
  st9(o + 18, r.zz);
  st9(o + 27, r.zzz);
  if (packed) {
    const G1X g = x29_to_r256(r);
    st8(o + 36, g.x);
    st8(o + 44, g.y);
    st8(o + 52, g.zz);
    st8(o + 60, g.zzz);
  }
}

// ---- the functions under test. P: Fq29P / Fr29P, B: the packed field FqP / FrP that goes with it.
template <class P, class B> struct OpMul {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) { st9(o, f29_mul(ld9<P>(d), ld9<P>(d + 9))); }
};
template <class P, class B> struct OpSqr {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) { st9(o, f29_sqr(ld9<P>(d))); }
};
template <class P, class B> struct OpMul2 {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) { st9(o, f29_mul2(ld9<P>(d), ld9<P>(d + 9), ld9<P>(d + 18), ld9<P>(d + 27))); }
};
template <class P, class B> struct OpMulChain {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) {
    Fp29<P> r = ld9<P>(d);
    const Fp29<P> b = ld9<P>(d + 9);
#pragma unroll 1
    for (int c = 0; c < CHAIN_STEPS / CHAIN_EVERY; c++) {
#pragma unroll
      for (int n = 0; n < CHAIN_EVERY; n++) r = f29_mul(r, b);
      st9(o + 9 * c, r);
    }
  }
};
template <class P, class B> struct OpSqrChain {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) {
    Fp29<P> r = ld9<P>(d);
#pragma unroll 1
    for (int c = 0; c < CHAIN_STEPS / CHAIN_EVERY; c++) {
#pragma unroll
      for (int n = 0; n < CHAIN_EVERY; n++) r = f29_sqr(r);
      st9(o + 9 * c, r);
    }
  }
};
template <class P, class B> struct OpMul2Chain {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) {
    Fp29<P> r = ld9<P>(d);
    const Fp29<P> b = ld9<P>(d + 9), c2 = ld9<P>(d + 18), d2 = ld9<P>(d + 27);
#pragma unroll 1
    for (int c = 0; c < CHAIN_STEPS / CHAIN_EVERY; c++) {
#pragma unroll 1
      for (int n = 0; n < CHAIN_EVERY; n++) r = f29_mul2(r, b, c2, d2);
      st9(o + 9 * c, r);
    }
  }
};
// the wide accumulator as the h(X) interpreter drives it: term j is pair j % 6, a carry pass after every sixth term
template <class P, class B> struct OpWide {
  static __device__ void run(const uint32_t* d, uint32_t nterms, uint32_t* o) {
    if (nterms > 24) return;
    F29Wide w;
    f29_wide_zero(w);
#pragma unroll 1
    for (uint32_t j = 0; j < nterms; j++) {
      const uint32_t* pr = d + 18 * (j % 6);
      const Fp29<P> a = ld9<P>(pr), b = ld9<P>(pr + 9);
      f29_wide_madd(w, a, b.l);
      if (j % 6 == 5) f29_wide_carry(w);
    }
    f29_wide_carry(w);
    st9(o, f29_wide_redc<P>(w));
  }
};
template <class P, class B> struct OpReduceWeak {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) { st9(o, f29_reduce_weak(ld9<P>(d))); }
};
// f29_mul(f29_sub<K>(a, b), c): the point formulas' differences feeding a product
template <class P, class B> struct OpSubMul {
  static __device__ void run(const uint32_t* d, uint32_t K, uint32_t* o) {
    const Fp29<P> a = ld9<P>(d), b = ld9<P>(d + 9), c = ld9<P>(d + 18);
    Fp29<P> t;
    switch (K) {
      case 3: t = f29_sub3(a, b); break;
      case 5: t = f29_sub5(a, b); break;
      case 6: t = f29_sub6(a, b); break;
      case 7: t = f29_sub7(a, b); break;
      case 8: t = f29_sub8(a, b); break;
      case 10: t = f29_sub10(a, b); break;
      default: return;
    }
    st9(o, t);
    st9(o + 9, f29_mul(t, c));
  }
};
// f29_mul2(a, b, f29_neg<K>(c), d) = a*b - c*d
template <class P, class B> struct OpNegMul2 {
  static __device__ void run(const uint32_t* d, uint32_t K, uint32_t* o) {
    const Fp29<P> a = ld9<P>(d), b = ld9<P>(d + 9), c = ld9<P>(d + 18), e = ld9<P>(d + 27);
    Fp29<P> t;
    switch (K) {
      case 3: t = f29_neg3(c); break;
      case 6: t = f29_neg6(c); break;
      case 10: t = f29_neg10(c); break;
      default: return;
    }
    st9(o, t);
    st9(o + 9, f29_mul2(a, b, t, e));
  }
};
// the NTT butterfly's (u - v) * w
template <class P, class B> struct OpLazyMul {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) {
    const Fp29<P> t = f29_sub10_lazy(ld9<P>(d), ld9<P>(d + 9));
    st9(o, t);
    st9(o + 9, f29_mul(t, ld9<P>(d + 18)));
  }
};
// the radix-4 block's ((x0 + x2) - (x1 + x3)) * w on lazy sums
template <class P, class B> struct OpLazy2Mul {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) {
    const Fp29<P> s0 = f29_add_lazy(ld9<P>(d), ld9<P>(d + 9)), s1 = f29_add_lazy(ld9<P>(d + 18), ld9<P>(d + 27));
    const Fp29<P> t = f29_sub10_lazy2(s0, s1);
    st9(o, t);
    st9(o + 9, f29_mul(t, ld9<P>(d + 36)));
  }
};
// the point additions' r * (q - x3) - y1 * ppp with the difference not carried
template <class P, class B> struct OpLazyMul2 {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) {
    const Fp29<P> t = f29_sub10_lazy(ld9<P>(d + 9), ld9<P>(d + 18));
    st9(o, f29_mul2(ld9<P>(d), t, ld9<P>(d + 27), ld9<P>(d + 36)));
  }
};
template <class P, class B> struct OpUnpackPack {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) {
    const Fp29<P> u = f29_unpack<P>(ld8<B>(d));
    st9(o, u);
    st8(o + 9, f29_pack_canonical<B>(u));
  }
};
template <class P, class B> struct OpFromToR256 {  // base field only
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) {
    const Fq29 v = fq29_from_r256(ld8<FqP>(d));
    st9(o, v);
    st8(o + 9, fq29_to_r256(v));
  }
};
template <class P, class B> struct OpToR256 {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) { st8(o, fq29_to_r256(ld9<Fq29P>(d))); }
};
template <class P, class B> struct OpMulConst {  // scalar field only, as the four below
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) { st8(o, fr29_mul_const(ld8<FrP>(d), ld8<FrP>(d + 8))); }
};
template <class P, class B> struct OpMulRR {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) { st8(o, fr29_mul_rr(ld8<FrP>(d), ld8<FrP>(d + 8))); }
};
template <class P, class B> struct OpMulStd {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) { st8(o, fr29_mul_std(ld8<FrP>(d), ld8<FrP>(d + 8))); }
};
template <class P, class B> struct OpFromMont {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) { st8(o, fr29_from_mont(ld8<FrP>(d))); }
};
template <class P, class B> struct OpInv29 {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) { st8(o, fr29_inv(ld8<FrP>(d))); }
};
template <class P, class B> struct OpBnMul {  // bn254.cuh, device branch: 8 x 32-bit CIOS
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) { st8(o, mul(ld8<B>(d), ld8<B>(d + 8))); }
};
template <class P, class B> struct OpBnInv {  // bn254.cuh, device branch: Fermat
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) { st8(o, inv(ld8<B>(d))); }
};
template <class P, class B> struct OpDblAffine {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) { stpt(o, x29_dbl_affine(ld9<Fq29P>(d), ld9<Fq29P>(d + 9)), true); }
};
template <class P, class B> struct OpAddAffine {
  static __device__ void run(const uint32_t* d, uint32_t q_inf, uint32_t* o) {
    stpt(o, x29_add_affine(ldpt(d), ld9<Fq29P>(d + 36), ld9<Fq29P>(d + 45), q_inf != 0), true);
  }
};
template <class P, class B> struct OpDbl {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) { stpt(o, x29_dbl(ldpt(d)), true); }
};
template <class P, class B> struct OpAdd {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) { stpt(o, x29_add(ldpt(d), ldpt(d + 36)), true); }
};
// 64 mixed additions, step j adds the affine point j % 4; the running sum at every eighth step
template <class P, class B> struct OpAddChain {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o) {
    G1X29 acc = G1X29::inf();
#pragma unroll 1
    for (int j = 0; j < CHAIN_STEPS; j++) {
      const uint32_t* q = d + 18 * (j % 4);
      acc = x29_add_affine(acc, ld9<Fq29P>(q), ld9<Fq29P>(q + 9), false);
      if (j % CHAIN_EVERY == CHAIN_EVERY - 1) stpt(o + 36 * (j / CHAIN_EVERY), acc, false);
    }
  }
};

// ---- the quad formulas: o + 36 * role receives this lane's copy of the result, o + 144 lane 0's packed form
__device__ __forceinline__ void st_quad(uint32_t* o, const G1X29& r, uint32_t role) {
  stpt(o + 36 * role, r, false);
  if (role == 0) {
    const G1X g = x29_to_r256(r);
    st8(o + 144, g.x);
    st8(o + 152, g.y);
    st8(o + 160, g.zz);
    st8(o + 168, g.zzz);
  }
}
template <class P, class B> struct OpDblQuad {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o, uint32_t role) { st_quad(o, x29_dbl_quad(ldpt(d), role), role); }
};
template <class P, class B> struct OpAddQuad {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o, uint32_t role) { st_quad(o, x29_add_quad(ldpt(d), ldpt(d + 36), role), role); }
};
// msm_window_combine_kernel's loop: 16 steps of three doublings and one addition of the affine point j % 4 (zz = zzz = 1), from
// the identity. Lane 0 stores the running point after steps 4, 8 and 12, all four lanes after step 16.
template <class P, class B> struct OpQuadChain {
  static __device__ void run(const uint32_t* d, uint32_t, uint32_t* o, uint32_t role) {
    G1X29 acc = G1X29::inf();
#pragma unroll 1
    for (int j = 0; j < QUAD_CHAIN_STEPS; j++) {
#pragma unroll 1
      for (int i = 0; i < 3; i++) acc = x29_dbl_quad(acc, role);
      const uint32_t* q = d + 18 * (j % 4);
      G1X29 v;
      v.x = ld9<Fq29P>(q);
      v.y = ld9<Fq29P>(q + 9);
      v.zz = v.zzz = f29_one<Fq29P>();
      acc = x29_add_quad(acc, v, role);
      if (j % QUAD_CHAIN_EVERY == QUAD_CHAIN_EVERY - 1) {
        if (j == QUAD_CHAIN_STEPS - 1) st_quad(o + 108, acc, role);
        else if (role == 0) stpt(o + 36 * (j / QUAD_CHAIN_EVERY), acc, false);
      }
    }
  }
};

// One launch per run of records with the same (function, field). Thread t: replica t / stride, record t % stride; stride is
// the record count rounded up to whole wavefronts, so the replicas of a record sit in different wavefronts.
template <class Op> __global__ void __launch_bounds__(WAVE) run_kernel(const uint32_t* in, uint32_t* out, uint32_t count, uint32_t stride, uint32_t total) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t rep = t / stride, idx = t % stride;
  if (rep >= REPLICAS || idx >= count) return;
  const uint32_t* rec = in + (size_t)idx * REC_WORDS;
  Op::run(rec + 4, rec[2], out + ((size_t)rep * total + idx) * OUT_WORDS);
}

// The same for the quad functions: quad t / 4 is the record, lane t & 3 its role; stride counts quads and is a whole number of
// wavefronts (16 quads each). A record that sits out leaves here, before the call: whole quads leave together.
template <class Op> __global__ void __launch_bounds__(WAVE) run_kernel_quad(const uint32_t* in, uint32_t* out, uint32_t count, uint32_t stride, uint32_t total) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, quad = t >> 2, role = t & 3u;
  const uint32_t rep = quad / stride, idx = quad % stride;
  if (rep >= REPLICAS || idx >= count) return;
  const uint32_t* rec = in + (size_t)idx * REC_WORDS;
  if (rec[2] & AUX_SIT_OUT) return;
  Op::run(rec + 4, rec[2], out + ((size_t)rep * total + idx) * OUT_WORDS, role);
}

typedef void (*kernel_t)(const uint32_t*, uint32_t*, uint32_t, uint32_t, uint32_t);
#define BOTH(Op) {run_kernel<Op<Fq29P, FqP>>, run_kernel<Op<Fr29P, FrP>>}
#define FQ_ONLY(Op) {run_kernel<Op<Fq29P, FqP>>, nullptr}
#define FR_ONLY(Op) {nullptr, run_kernel<Op<Fr29P, FrP>>}
#define FQ_QUAD(Op) {run_kernel_quad<Op<Fq29P, FqP>>, nullptr}
// index = function id of tests/fp29_model.py (F_MUL = 1 ...)
static const kernel_t KERNELS[][2] = {
    {nullptr, nullptr},    BOTH(OpMul),          BOTH(OpSqr),         BOTH(OpMul2),       BOTH(OpMulChain),     BOTH(OpSqrChain),
    BOTH(OpMul2Chain),     BOTH(OpWide),         BOTH(OpReduceWeak),  BOTH(OpSubMul),     BOTH(OpNegMul2),      BOTH(OpLazyMul),
    BOTH(OpLazy2Mul),      BOTH(OpLazyMul2),     BOTH(OpUnpackPack),  FQ_ONLY(OpFromToR256), FQ_ONLY(OpToR256), FR_ONLY(OpMulConst),
    FR_ONLY(OpMulRR),      FR_ONLY(OpMulStd),    FR_ONLY(OpFromMont), FR_ONLY(OpInv29),   BOTH(OpBnMul),        BOTH(OpBnInv),
    FQ_ONLY(OpDblAffine),  FQ_ONLY(OpAddAffine), FQ_ONLY(OpDbl),      FQ_ONLY(OpAdd),     FQ_ONLY(OpAddChain),
    FQ_QUAD(OpDblQuad),    FQ_QUAD(OpAddQuad),   FQ_QUAD(OpQuadChain)};
static_assert(sizeof(KERNELS) / sizeof(KERNELS[0]) == FIRST_QUAD_FUNC + 3, "the quad functions are the last three of the table");
constexpr uint32_t N_FUNCS = sizeof(KERNELS) / sizeof(KERNELS[0]);

static int bad_file(const char* what) {
  fprintf(stderr, "case file: %s\n", what);
  return 4;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s <cases.bin> <results.bin>\n", argv[0]);
    return 4;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return bad_file("cannot open");
  uint32_t hdr[4];
  if (fread(hdr, 4, 4, f) != 4 || hdr[0] != MAGIC || hdr[2] != IN_WORDS || hdr[3] != OUT_WORDS) return bad_file("bad header");
  const uint32_t n = hdr[1];
  if (n == 0 || n > (1u << 20)) return bad_file("case count out of range");
  std::vector<uint32_t> in((size_t)n * REC_WORDS);
  if (fread(in.data(), 4, in.size(), f) != in.size() || fgetc(f) != EOF) return bad_file("length does not match the header");
  fclose(f);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t* r = &in[(size_t)i * REC_WORDS];
    if (r[0] == 0 || r[0] >= N_FUNCS || r[1] > 1 || !KERNELS[r[0]][r[1]] || r[3] > IN_WORDS) return bad_file("unknown function / field in a record");
  }

  int ndev = 0;
  HIP_OK(hipGetDeviceCount(&ndev));
  if (ndev < 1) return 3;
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, 0));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    fprintf(stderr, "device 0 is %s, not gfx950: refusing to run\n", prop.gcnArchName);
    return 3;
  }
  HIP_OK(hipSetDevice(0));

  const size_t out_words = (size_t)REPLICAS * n * OUT_WORDS;
  uint32_t *d_in = nullptr, *d_out = nullptr;
  HIP_OK(hipMalloc(&d_in, in.size() * 4));
  HIP_OK(hipMalloc(&d_out, out_words * 4));
  HIP_OK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemset(d_out, 0xff, out_words * 4));  // words a function does not write stay 0xffffffff
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t launches = 0;
  for (uint32_t first = 0; first < n;) {
    const uint32_t func = in[(size_t)first * REC_WORDS], field = in[(size_t)first * REC_WORDS + 1];
    uint32_t count = 1;
    while (first + count < n && in[(size_t)(first + count) * REC_WORDS] == func && in[(size_t)(first + count) * REC_WORDS + 1] == field) count++;
    const uint32_t per_wave = func >= FIRST_QUAD_FUNC ? WAVE / 4 : WAVE;  // records of one wavefront
    const uint32_t stride = (count + per_wave - 1) / per_wave * per_wave;
    KERNELS[func][field]<<<dim3(REPLICAS * stride / per_wave), dim3(WAVE)>>>(d_in + (size_t)first * REC_WORDS, d_out + (size_t)first * OUT_WORDS, count, stride, n);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());  // a fault is reported at the launch that caused it
    first += count;
    launches++;
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  std::vector<uint32_t> out(out_words);
  HIP_OK(hipMemcpy(out.data(), d_out, out_words * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipFree(d_in));
  HIP_OK(hipFree(d_out));
  f = fopen(argv[2], "wb");
  if (!f) return bad_file("cannot write the results");
  const uint32_t ohdr[4] = {MAGIC, n, REPLICAS, OUT_WORDS};
  if (fwrite(ohdr, 4, 4, f) != 4 || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f) != 0) return bad_file("short write");
  printf("fp29_device_check: %u cases x %u replicas in %u launches on %s, %.1f ms\n", n, REPLICAS, launches, prop.gcnArchName, ms);
  return 0;
}
