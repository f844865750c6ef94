// Unit harness for the pairing's Fq2 layer, executor and programs (csrc/fq12.cuh, csrc/pairing.hpp), driven by
// tests/fq12_model.py (tests/test_fq12_model.py on the CPU, tests/test_gpu_pairing_words.py on the device).
//
// ONE source, two builds:
//   device  hipcc with the library's own flags (tests/native/Makefile reads them from csrc/Makefile), so that f29_mul,
//           f29_sqr here ARE the asm blocks of fp29_asm.inc in the compile context the library ships them in: operands
//           loaded from a lane's slab in global memory, inside the 13-way switch of pairing_exec's `unroll 1` loop. The
//           kernel has pairing_miller_kernel's shape (__launch_bounds__(64), the lane's slab at slab + t * regs, K and
//           the lines in global memory, one call of pairing_exec) and no arithmetic of its own.
//   host    g++ -x c++: the same case reader, the same slabs and the same call of pairing_exec with no HIP call, and
//           with the documented fp29 bounds compiled in as hard failures (FP29_CHECK_BOUNDS): a case that breaks a
//           stated precondition aborts here, before any GPU run.
// It computes and judges nothing itself:
//   fq12_check <cases.bin> <results.bin>   run every case, write the registers each case asks for
//   fq12_check --emit <requests.txt>       (either build; no device needed) print the constant table K and, per request
//                                          line "id base args...", the words pairing.hpp emits: the Python executor runs
//                                          the words the device runs, and the emitters are not restated in Python
//
// Case file (u32 words): MAGIC, count, then per case
//   kind, regs, n_prog, n_in, n_lines, n_out,
//   n_prog words   kind 0: the program words themselves; kind > 0: an emitter id, the words are "base args..." (below)
//   n_in  x (register, 18 limbs)   raw Fq2x values: non-canonical stored forms can be given
//   n_lines x 32 words             prepared lines, four packed canonical Fq (radix 2^261) each
//   n_out x register               what comes back
// Every register of a slab that is not an input holds PATTERN(register, limb) before the run, so a register nobody should
// touch can be asked for and compared. K is always pairing::device_consts.
// Result file: MAGIC, count, REPLICAS, then per replica and case n_out x 18 limbs.
//
// Cases with the same (kind, regs) that follow each other are one launch. Thread t: replica t / stride, case t % stride,
// stride the case count rounded up to whole wavefronts: the replicas of a case sit in different wavefronts, and
// neighbouring lanes hold different cases (for kind 0: different ops of the switch).
//
// Every register index and constant index of every word (given or emitted) is checked against `regs` / K_COUNT and the
// line count before anything runs. Exit status: 0 results written; 2 HIP error; 3 not a gfx950 device; 4 malformed case file.
#if !defined(__HIPCC__)
#define FP29_CHECK_BOUNDS 1
#endif
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "../../anon-aadhaar-halo2_amd/csrc/pairing.hpp"
using namespace bn254;

constexpr uint32_t MAGIC = 0x43323146u;  // "F12C"
constexpr uint32_t REPLICAS = 2, WAVE = 64, LIMBS = 18;
constexpr uint32_t pattern(uint32_t reg, uint32_t limb) { return 0xA5000000u | (reg << 8) | limb; }

// emitter ids of tests/fq12_model.py
enum Emitter : uint32_t {
  E_RAW = 0, E6_MUL_V, E6_MUL, E6_SQR, E6_MUL_01, E6_INV, E12_CONJ, E12_MUL, E12_SQR, E12_MUL_034, E12_FROBENIUS, E4_SQR,
  E12_CYCLOTOMIC_SQR, E12_INV, E12_POW_U, MILLER_PROGRAM, MUL_PROGRAM, FINAL_EXP_PROGRAM, E_COUNT
};
// how many register arguments follow `base` (E12_FROBENIUS: r, a and k)
static const int EMITTER_ARGS[E_COUNT] = {0, 2, 3, 2, 4, 2, 2, 3, 2, 5, 3, 4, 2, 2, 2, 0, 0, 0};

// The words of emitter `id`. args = base, then the emitter's own arguments; temporaries are allocated from `base` up.
static bool emit(uint32_t id, const std::vector<uint32_t>& args, pairing::Prog& p) {
  if (id == E_RAW || id >= E_COUNT) return false;
  if (id >= MILLER_PROGRAM) {
    if (!args.empty()) return false;
    p = id == MILLER_PROGRAM ? pairing::miller_program() : id == MUL_PROGRAM ? pairing::mul_program() : pairing::final_exp_program();
    return p.regs <= 256;
  }
  if (args.size() != (size_t)EMITTER_ARGS[id] + 1) return false;
  if (args[0] > 256) return false;
  for (size_t i = 1; i < args.size(); i++)
    if (args[i] > 250) return false;  // an operand is at most six registers: every index an emitter forms fits its 8-bit field
  const int* x = (const int*)args.data() + 1;
  p.alloc((int)args[0]);
  switch (id) {
    case E6_MUL_V: pairing::e6_mul_v(p, x[0], x[1]); break;
    case E6_MUL: pairing::e6_mul(p, x[0], x[1], x[2]); break;
    case E6_SQR: pairing::e6_sqr(p, x[0], x[1]); break;
    case E6_MUL_01: pairing::e6_mul_01(p, x[0], x[1], x[2], x[3]); break;
    case E6_INV: pairing::e6_inv(p, x[0], x[1]); break;
    case E12_CONJ: pairing::e12_conj(p, x[0], x[1]); break;
    case E12_MUL: pairing::e12_mul(p, x[0], x[1], x[2]); break;
    case E12_SQR: pairing::e12_sqr(p, x[0], x[1]); break;
    case E12_MUL_034: pairing::e12_mul_034(p, x[0], x[1], x[2], x[3], x[4]); break;
    case E12_FROBENIUS:
      if (x[2] < 1 || x[2] > 3) return false;
      pairing::e12_frobenius(p, x[0], x[1], x[2]);
      break;
    case E4_SQR: pairing::e4_sqr(p, x[0], x[1], x[2], x[3]); break;
    case E12_CYCLOTOMIC_SQR: pairing::e12_cyclotomic_sqr(p, x[0], x[1]); break;
    case E12_INV: pairing::e12_inv(p, x[0], x[1]); break;
    default: pairing::e12_pow_u(p, x[0], x[1]); break;
  }
  return p.regs <= 256;
}

struct Case {
  uint32_t kind = 0, regs = 0;
  std::vector<uint32_t> prog, in, lines, out;  // in: n x (register, 18 limbs); lines: n x 32 words
};

// every index a word can form stays inside the slab, the constant table and the case's lines
static bool words_in_range(const std::vector<uint32_t>& w, uint32_t regs, size_t n_lines) {
  size_t lines_used = 0;
  for (uint32_t x : w) {
    const uint32_t op = x >> 24, d = (x >> 16) & 255u, a = (x >> 8) & 255u, b = x & 255u;
    if (op > P_LINE || d >= regs) return false;
    if (op == P_LINE) {
      if (d + 1 >= regs || ++lines_used > n_lines) return false;
      continue;
    }
    if (op != P_MOVK && a >= regs) return false;
    if ((op == P_MUL || op == P_ADD || op == P_SUB || op == P_MULFQ) && b >= regs) return false;
    if ((op == P_MULK || op == P_MOVK) && b >= (uint32_t)pairing::K_COUNT) return false;
  }
  return true;
}

static int bad_file(const char* what) {
  fprintf(stderr, "case file: %s\n", what);
  return 4;
}

static int emit_mode(const char* path) {
  Fq2x K[pairing::K_COUNT];
  pairing::device_consts(K);
  for (int i = 0; i < pairing::K_COUNT; i++) {
    printf("K %d", i);
    for (int j = 0; j < 9; j++) printf(" %x", K[i].c0.l[j]);
    for (int j = 0; j < 9; j++) printf(" %x", K[i].c1.l[j]);
    printf("\n");
  }
  FILE* f = fopen(path, "r");
  if (!f) return bad_file("cannot open the requests");
  char line[256];
  while (fgets(line, sizeof(line), f)) {
    std::vector<uint32_t> v;
    char* s = line;
    for (;;) {
      char* e;
      const unsigned long x = strtoul(s, &e, 10);
      if (e == s) break;
      v.push_back((uint32_t)x);
      s = e;
    }
    if (v.empty()) continue;
    pairing::Prog p;
    if (!emit(v[0], std::vector<uint32_t>(v.begin() + 1, v.end()), p)) return bad_file("unknown emitter or bad arguments in a request");
    printf("prog %d %zu", p.regs, p.w.size());
    for (uint32_t w : p.w) printf(" %x", w);
    printf("\n");
  }
  fclose(f);
  return 0;
}

struct Lane {
  uint32_t prog_off, prog_len, lines_off;
};
struct Args {
  const uint32_t* prog;
  const Lane* lane;
  const Fq2x* K;
  const Fq* lines;
  Fq2x* slab;  // [total][regs]
  uint32_t regs, total;
};

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HIP_OK(call)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      fprintf(stderr, "HIP error %s at %s:%d: %s\n", hipGetErrorName(e_), __FILE__, __LINE__, #call); \
      exit(2);                                                                               \
    }                                                                                        \
  } while (0)

__global__ __launch_bounds__(WAVE) void fq12_check_kernel(Args a) {
  const size_t t = (size_t)blockIdx.x * WAVE + threadIdx.x;
  if (t >= a.total) return;
  const Lane d = a.lane[t];
  pairing_exec(a.prog + d.prog_off, d.prog_len, a.slab + t * a.regs, a.K, a.lines + d.lines_off);
}

template <class T> static T* upload(const void* h, size_t bytes) {
  void* d = nullptr;
  HIP_OK(hipMalloc(&d, bytes ? bytes : 4));
  if (bytes) HIP_OK(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
  return (T*)d;
}
// one launch: the slab comes back in place
static void run_lanes(const std::vector<uint32_t>& prog, const std::vector<Lane>& lane, const Fq2x* K, const std::vector<Fq>& lines,
                      std::vector<Fq2x>& slab, uint32_t regs) {
  Args a;
  uint32_t* d_prog = upload<uint32_t>(prog.data(), prog.size() * 4);
  Lane* d_lane = upload<Lane>(lane.data(), lane.size() * sizeof(Lane));
  Fq2x* d_K = upload<Fq2x>(K, pairing::K_COUNT * sizeof(Fq2x));
  Fq* d_lines = upload<Fq>(lines.data(), lines.size() * sizeof(Fq));
  Fq2x* d_slab = upload<Fq2x>(slab.data(), slab.size() * sizeof(Fq2x));
  a.prog = d_prog, a.lane = d_lane, a.K = d_K, a.lines = d_lines, a.slab = d_slab, a.regs = regs, a.total = (uint32_t)lane.size();
  fq12_check_kernel<<<dim3((unsigned)(lane.size() / WAVE)), dim3(WAVE)>>>(a);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());  // a fault is reported at the launch that caused it
  HIP_OK(hipMemcpy(slab.data(), d_slab, slab.size() * sizeof(Fq2x), hipMemcpyDeviceToHost));
  HIP_OK(hipFree(d_prog));
  HIP_OK(hipFree(d_lane));
  HIP_OK(hipFree(d_K));
  HIP_OK(hipFree(d_lines));
  HIP_OK(hipFree(d_slab));
}
#else
static void run_lanes(const std::vector<uint32_t>& prog, const std::vector<Lane>& lane, const Fq2x* K, const std::vector<Fq>& lines,
                      std::vector<Fq2x>& slab, uint32_t regs) {
  for (size_t t = 0; t < lane.size(); t++)
    pairing_exec(prog.data() + lane[t].prog_off, lane[t].prog_len, slab.data() + t * regs, K, lines.data() + lane[t].lines_off);
}
#endif

int main(int argc, char** argv) {
  static_assert(sizeof(Fq2x) == LIMBS * 4 && sizeof(Fq) == 32, "a register is 18 words, a packed Fq eight");
  if (argc == 3 && strcmp(argv[1], "--emit") == 0) return emit_mode(argv[2]);
  if (argc != 3) {
    fprintf(stderr, "usage: %s <cases.bin> <results.bin> | --emit <requests.txt>\n", argv[0]);
    return 4;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return bad_file("cannot open");
  std::vector<uint32_t> raw;
  {
    uint32_t buf[4096];
    size_t got;
    while ((got = fread(buf, 4, 4096, f)) > 0) raw.insert(raw.end(), buf, buf + got);
    fclose(f);
  }
  if (raw.size() < 2 || raw[0] != MAGIC) return bad_file("bad header");
  const uint32_t n = raw[1];
  if (n == 0 || n > (1u << 20)) return bad_file("case count out of range");
  std::vector<Case> cases(n);
  size_t pos = 2;
  for (uint32_t i = 0; i < n; i++) {
    if (pos + 6 > raw.size()) return bad_file("truncated record");
    Case& c = cases[i];
    const uint32_t* h = &raw[pos];
    const size_t n_prog = h[2], n_in = h[3], n_lines = h[4], n_out = h[5];
    c.kind = h[0], c.regs = h[1];
    pos += 6;
    if (c.regs == 0 || c.regs > 256 || n_prog > (1u << 20) || n_in > 256 || n_lines > 1024 || n_out > 256) return bad_file("record header out of range");
    if (pos + n_prog + n_in * (1 + LIMBS) + n_lines * 32 + n_out > raw.size()) return bad_file("truncated record");
    std::vector<uint32_t> given(raw.begin() + pos, raw.begin() + pos + n_prog);
    pos += n_prog;
    c.in.assign(raw.begin() + pos, raw.begin() + pos + n_in * (1 + LIMBS));
    pos += n_in * (1 + LIMBS);
    c.lines.assign(raw.begin() + pos, raw.begin() + pos + n_lines * 32);
    pos += n_lines * 32;
    c.out.assign(raw.begin() + pos, raw.begin() + pos + n_out);
    pos += n_out;
    if (c.kind == E_RAW) {
      c.prog = given;
    } else {
      pairing::Prog p;
      if (!emit(c.kind, given, p) || (uint32_t)p.regs > c.regs) return bad_file("unknown emitter, bad arguments, or more registers than the record gives");
      c.prog = p.w;
    }
    if (!words_in_range(c.prog, c.regs, n_lines)) return bad_file("a program word leaves the slab, the constant table or the lines");
    for (size_t k = 0; k < n_in; k++)
      if (c.in[k * (1 + LIMBS)] >= c.regs) return bad_file("input register outside the slab");
    for (uint32_t r : c.out)
      if (r >= c.regs) return bad_file("output register outside the slab");
  }
  if (pos != raw.size()) return bad_file("length does not match the header");

  const char* where = "the host";
#if defined(__HIPCC__)
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
  where = prop.gcnArchName;
#endif

  Fq2x K[pairing::K_COUNT];
  pairing::device_consts(K);
  std::vector<std::vector<uint32_t>> results(REPLICAS);
  const auto t0 = std::chrono::steady_clock::now();
  uint32_t launches = 0;
  for (uint32_t first = 0; first < n;) {
    uint32_t count = 1;
    while (first + count < n && cases[first + count].kind == cases[first].kind && cases[first + count].regs == cases[first].regs) count++;
    const uint32_t regs = cases[first].regs, stride = (count + WAVE - 1) / WAVE * WAVE;
    std::vector<uint32_t> prog;
    std::vector<Fq> lines(1);  // never an empty allocation
    std::vector<Lane> lane((size_t)REPLICAS * stride, Lane{0, 0, 0});
    std::vector<Fq2x> slab((size_t)REPLICAS * stride * regs);
    for (size_t t = 0; t < lane.size(); t++)
      for (uint32_t r = 0; r < regs; r++) {
        uint32_t* limb = (uint32_t*)&slab[t * regs + r];
        for (uint32_t j = 0; j < LIMBS; j++) limb[j] = pattern(r, j);
      }
    for (uint32_t i = 0; i < count; i++) {
      const Case& c = cases[first + i];
      const Lane d{(uint32_t)prog.size(), (uint32_t)c.prog.size(), (uint32_t)lines.size()};
      prog.insert(prog.end(), c.prog.begin(), c.prog.end());
      for (size_t k = 0; k < c.lines.size(); k += 8) {
        Fq v;
        memcpy(v.l, &c.lines[k], 32);
        lines.push_back(v);
      }
      for (uint32_t rep = 0; rep < REPLICAS; rep++) {
        const size_t t = (size_t)rep * stride + i;
        lane[t] = d;
        for (size_t k = 0; k < c.in.size(); k += 1 + LIMBS) memcpy(&slab[t * regs + c.in[k]], &c.in[k + 1], LIMBS * 4);
      }
    }
    run_lanes(prog, lane, K, lines, slab, regs);
    for (uint32_t rep = 0; rep < REPLICAS; rep++)
      for (uint32_t i = 0; i < count; i++)
        for (uint32_t r : cases[first + i].out) {
          const uint32_t* limb = (const uint32_t*)&slab[((size_t)rep * stride + i) * regs + r];
          results[rep].insert(results[rep].end(), limb, limb + LIMBS);
        }
    first += count;
    launches++;
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  f = fopen(argv[2], "wb");
  if (!f) return bad_file("cannot write the results");
  const uint32_t ohdr[3] = {MAGIC, n, REPLICAS};
  bool ok = fwrite(ohdr, 4, 3, f) == 3;
  for (uint32_t rep = 0; rep < REPLICAS; rep++) ok = ok && fwrite(results[rep].data(), 4, results[rep].size(), f) == results[rep].size();
  if (fclose(f) != 0 || !ok) return bad_file("short write");
  printf("fq12_check: %u cases x %u replicas in %u launches on %s, %.1f ms\n", n, REPLICAS, launches, where, ms);
  return 0;
}
