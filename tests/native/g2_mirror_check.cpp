// The C++ mirror's side of the SRS file's G2 points (include/amdzk_halo2.hpp): G2Affine::{to_bytes, from_bytes,
// is_on_curve_and_in_subgroup}, ParamsVerifierKZG from the two 64-byte fields, ParamsKZG::check. Driven by
// tests/test_g2_mirror.py.
//   g2_mirror_check codec       no device: round trips of the generator, the refusals, membership; prints "codec ok"
//   g2_mirror_check check K     on the GPU: setup(K) and the G2 half with one trapdoor, write, read, ParamsVerifierKZG from the
//                               file's fields, ParamsKZG::check; then the same parameters against another trapdoor's s_g2.
//                               Prints "honest RAN FAILED" and "mixed RAN FAILED".
#include <cstdio>
#include <cstring>
#include <string>

#include "amdzk_halo2.hpp"

using namespace amdzk::halo2;

static int fails = 0;
#define CHECK(cond)                                            \
  do {                                                         \
    if (!(cond)) {                                             \
      printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond);  \
      fails++;                                                 \
    }                                                          \
  } while (0)

template <class F>
static std::string refusal(F f) {
  try {
    f();
  } catch (const Error& e) {
    return e.code == AMDZK_E_INVALID ? e.what() : "wrong code";
  }
  return "";
}

static Fr trapdoor(uint64_t v) {  // distinct trapdoors are all this needs: the words are the Montgomery representative itself
  Fr s;
  s.l[0] = v, s.l[1] = 0x1234, s.l[2] = 0, s.l[3] = 0;
  return s;
}

static int codec() {
  // EIP-197's generator: its x as plain integers, little-endian, is its encoding (y.c0 is even: no flag)
  static const uint64_t gx[8] = {0x46debd5cd992f6edull, 0x674322d4f75edaddull, 0x426a00665e5c4479ull, 0x1800deef121f1e76ull,
                                 0x97e485b7aef312c2ull, 0xf1aa493335a9e712ull, 0x7260bfb731fb5d25ull, 0x198e9393920d483aull};
  uint8_t enc[64];
  memcpy(enc, gx, 64);
  const G2Affine g = G2Affine::from_bytes(enc);
  CHECK(g.is_on_curve_and_in_subgroup() && g.check() == 0);
  const auto back = g.to_bytes();
  CHECK(memcmp(back.data(), enc, 64) == 0);
  uint8_t neg[64];
  memcpy(neg, enc, 64);
  neg[63] ^= 0x80;
  const G2Affine ng = G2Affine::from_bytes(neg);
  CHECK(memcmp(ng.w, g.w, 64) == 0 && memcmp(ng.w + 8, g.w + 8, 64) != 0 && ng.is_on_curve_and_in_subgroup());
  CHECK(memcmp(ng.to_bytes().data(), neg, 64) == 0);
  uint8_t zero[64] = {0};
  const G2Affine id = G2Affine::from_bytes(zero);
  CHECK(id.check() == 3 && !id.is_on_curve_and_in_subgroup());
  CHECK(memcmp(id.to_bytes().data(), zero, 64) == 0);
  uint8_t bad[64];
  memcpy(bad, enc, 64), bad[63] |= 0x40;
  CHECK(refusal([&] { G2Affine::from_bytes(bad); }).rfind("g2_decompress:", 0) == 0);
  memset(bad, 0, 64), bad[63] = 0x80;
  CHECK(refusal([&] { G2Affine::from_bytes(bad); }).rfind("g2_decompress:", 0) == 0);
  G2Affine off = g;
  off.w[8] ^= 1;
  CHECK(off.check() == 2);
  CHECK(refusal([&] { off.to_bytes(); }).rfind("g2_compress:", 0) == 0);
  CHECK(refusal([&] { ParamsVerifierKZG::member(zero, "g2"); }).find("g2 is the identity") != std::string::npos);
  CHECK(memcmp(ParamsVerifierKZG::member(enc, "g2").w, g.w, 128) == 0);
  if (fails) return 1;
  printf("codec ok\n");
  return 0;
}

static int check(uint32_t k) {
  Context ctx(0);
  const Fr s = trapdoor(77), other = trapdoor(78);
  G2Affine g2, s_g2, g2b, other_s_g2;
  ctx.check(amdzk_g2_setup(ctx.get(), s.l, g2.w, s_g2.w));
  ctx.check(amdzk_g2_setup(ctx.get(), other.l, g2b.w, other_s_g2.w));
  std::vector<uint8_t> file;
  {
    ParamsKZG made = ParamsKZG::setup(ctx, k, s);
    file = made.write(g2.to_bytes().data(), s_g2.to_bytes().data());
  }
  uint8_t f_g2[64], f_s_g2[64];
  ParamsKZG params = ParamsKZG::read(ctx, file, f_g2, f_s_g2);
  ParamsVerifierKZG vparams(ctx, f_g2, f_s_g2);
  CHECK(vparams.g2.handle() && vparams.s_g2.handle());
  const G2Affine r_g2 = G2Affine::from_bytes(f_g2), r_s_g2 = G2Affine::from_bytes(f_s_g2);
  CHECK(memcmp(r_g2.w, g2.w, 128) == 0 && memcmp(r_s_g2.w, s_g2.w, 128) == 0);
  const amdzk_srs_report honest = params.check(r_g2, r_s_g2);
  const uint64_t seed = 5;
  const amdzk_srs_report mixed = params.check(r_g2, other_s_g2, &seed);
  if (fails) return 1;
  printf("honest %u %u\nmixed %u %u\n", honest.ran, honest.failed, mixed.ran, mixed.failed);
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc == 2 && std::string(argv[1]) == "codec") return codec();
    if (argc == 3 && std::string(argv[1]) == "check") return check((uint32_t)atoi(argv[2]));
  } catch (const std::exception& e) {
    printf("exception: %s\n", e.what());
    return 3;
  }
  printf("usage: g2_mirror_check codec | check K\n");
  return 2;
}
