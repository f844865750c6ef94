// Host build of the G2 codec — csrc/g2codec.hpp and nothing else of the library, with the host compiler alone — driven by
// tests/test_g2_codec_host.py against tests/pairing_ref.py, once plain and once under ASan + UBSan. Self-checks run first:
// round trips over multiples of the generator, and every refusal. Then commands on stdin, one per line, numbers in hex:
//   enc X0 X1 Y0 Y1   (plain integers below the modulus; all zero = the identity)  -> "bytes <128 hex digits>" | "refused <why>"
//   dec <128 hex digits>                                                           -> "pt X0 X1 Y0 Y1" | "refused <why>"
//   chk X0 X1 Y0 Y1                                                                -> "status N"
// The last line is "ok".
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../../anon-aadhaar-halo2_amd/csrc/g2codec.hpp"

using namespace bn254;

static int fails = 0;
#define CHECK(cond)                                            \
  do {                                                         \
    if (!(cond)) {                                             \
      printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond);  \
      fails++;                                                 \
    }                                                          \
  } while (0)

static bool parse_fq(const std::string& s, Fq* out) {
  if (s.empty() || s.size() > 64) return false;
  uint64_t w[4] = {0, 0, 0, 0};
  for (char ch : s) {
    const int d = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1;
    if (d < 0) return false;
    for (int i = 3; i > 0; i--) w[i] = (w[i] << 4) | (w[i - 1] >> 60);
    w[0] = (w[0] << 4) | (uint64_t)d;
  }
  Fq a;
  memcpy(a.l, w, 32);
  if (!is_canonical(a)) return false;
  *out = to_mont(a);
  return true;
}
static std::string hex_fq(const Fq& m) {
  const Fq a = from_mont(m);
  char buf[65];
  for (int i = 0; i < 8; i++) snprintf(buf + 8 * i, 9, "%08x", a.l[7 - i]);
  return buf;
}
static bool read_point(std::istringstream& in, uint64_t w[16]) {
  pairing::G2Affine q;
  Fq* c[4] = {&q.x.c0, &q.x.c1, &q.y.c0, &q.y.c1};
  for (int i = 0; i < 4; i++) {
    std::string s;
    if (!(in >> s) || !parse_fq(s, c[i])) return false;
  }
  pairing::g2_to_words(q, w);
  return true;
}

static void selfcheck() {
  const pairing::G2Affine gen = pairing::g2_generator();
  uint64_t w[16], back[16];
  uint8_t b[64], zero[64] = {0};
  // round trips, both signs, and membership
  const uint64_t ks[5][4] = {{1, 0, 0, 0}, {2, 0, 0, 0}, {0x9E3779B97F4A7C15ull, 0xF39CC0605CEDC834ull, 0, 0}, {7, 7, 7, 7}, {0xFFFFFFFFFFFFFFFFull, 0, 0, 1}};
  for (const auto& k : ks) {
    const pairing::G2Affine p = pairing::g2_mul(gen, k);
    for (int sign = 0; sign < 2; sign++) {
      pairing::g2_to_words(sign ? pairing::g2_neg(p) : p, w);
      CHECK(g2codec::g2_compress(w, b) == nullptr);
      CHECK((b[63] & 0x40) == 0);
      CHECK(g2codec::g2_decompress(b, back) == nullptr && memcmp(w, back, sizeof(w)) == 0);
      CHECK(g2codec::g2_status(w) == g2codec::G2_IN_GROUP);
      b[63] ^= 0x80;  // the other root
      uint64_t negw[16];
      pairing::g2_to_words(sign ? p : pairing::g2_neg(p), negw);
      CHECK(g2codec::g2_decompress(b, back) == nullptr && memcmp(negw, back, sizeof(negw)) == 0);
    }
  }
  // the identity
  memset(w, 0, sizeof(w));
  memset(b, 0xAA, 64);
  CHECK(g2codec::g2_compress(w, b) == nullptr && memcmp(b, zero, 64) == 0);
  memset(back, 0xFF, sizeof(back));
  CHECK(g2codec::g2_decompress(zero, back) == nullptr && memcmp(back, w, sizeof(w)) == 0);
  CHECK(g2codec::g2_status(w) == g2codec::G2_IDENTITY);
  // x = 0 with the sign bit
  memset(b, 0, 64);
  b[63] = 0x80;
  CHECK(g2codec::g2_decompress(b, back) != nullptr);
  // x.c0 = q, x.c1 = q, bit 6
  pairing::g2_to_words(gen, w);
  CHECK(g2codec::g2_compress(w, b) == nullptr);
  uint8_t qb[32];
  for (int i = 0; i < 8; i++)
    for (int j = 0; j < 4; j++) qb[4 * i + j] = (uint8_t)(FqP::p(i) >> (8 * j));
  uint8_t t[64];
  memcpy(t, b, 64), memcpy(t, qb, 32);
  CHECK(g2codec::g2_decompress(t, back) != nullptr);
  memcpy(t, b, 64), memcpy(t + 32, qb, 32);
  CHECK(g2codec::g2_decompress(t, back) != nullptr);
  memcpy(t, b, 64), t[63] |= 0x40;
  CHECK(g2codec::g2_decompress(t, back) != nullptr);
  memset(t, 0xFF, 64);
  CHECK(g2codec::g2_decompress(t, back) != nullptr);
  // words that are no residues: every coordinate in turn = q (Montgomery words of a residue are below q)
  for (int c = 0; c < 4; c++) {
    uint64_t bad[16];
    pairing::g2_to_words(gen, bad);
    for (int i = 0; i < 4; i++) bad[4 * c + i] = (uint64_t)FqP::p(2 * i) | ((uint64_t)FqP::p(2 * i + 1) << 32);
    CHECK(g2codec::g2_compress(bad, t) != nullptr);
    CHECK(g2codec::g2_status(bad) == g2codec::G2_COORD_TOO_LARGE);
  }
  memset(w, 0xFF, sizeof(w));
  CHECK(g2codec::g2_compress(w, t) != nullptr && g2codec::g2_status(w) == g2codec::G2_COORD_TOO_LARGE);
  // off the twist
  pairing::G2Affine off = gen;
  off.y.c0 = add(off.y.c0, Fq::one());
  pairing::g2_to_words(off, w);
  CHECK(g2codec::g2_compress(w, t) != nullptr && g2codec::g2_status(w) == g2codec::G2_OFF_TWIST);
  // small x: a non-residue is refused under both signs; a residue gives a point of the twist with that x which [r] does not
  // kill (the cofactor is about 2^254) and which round-trips
  int residues = 0, non_residues = 0;
  for (uint32_t a = 1; a < 24; a++) {
    memset(t, 0, 64);
    t[0] = (uint8_t)a;
    const char* why = g2codec::g2_decompress(t, back);
    if (why) {
      non_residues++;
      t[63] = 0x80;
      CHECK(g2codec::g2_decompress(t, back) != nullptr);
      continue;
    }
    residues++;
    const pairing::G2Affine p = pairing::g2_from_words(back);
    CHECK(pairing::g2_on_twist(p) && p.x.c1.is_zero() && from_mont(p.x.c0).l[0] == a);
    CHECK((from_mont(p.y.c0).l[0] & 1u) == 0);
    CHECK(g2codec::g2_status(back) == g2codec::G2_OUTSIDE_SUBGROUP);
    uint8_t again[64];
    CHECK(g2codec::g2_compress(back, again) == nullptr && memcmp(again, t, 64) == 0);
  }
  CHECK(residues >= 4 && non_residues >= 4);
  // f2_sqrt on squares, zero included
  for (uint32_t a = 0; a < 8; a++) {
    const pairing::Fq2 v{pairing::fq_small(a), pairing::fq_small(3 * a + 1)}, sq = pairing::f2_sqr(v);
    pairing::Fq2 r;
    CHECK(g2codec::f2_sqrt(sq, &r) && (r == v || r == pairing::f2_neg(v)));
  }
  pairing::Fq2 r;
  const pairing::Fq2 z{Fq::zero(), Fq::zero()};
  CHECK(g2codec::f2_sqrt(z, &r) && r.is_zero());
}

int main() {
  selfcheck();
  if (fails) return 1;
  printf("selfcheck ok\n");
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    uint64_t w[16];
    if (cmd == "enc" || cmd == "chk") {
      if (!read_point(in, w)) {
        printf("bad input\n");
        return 2;
      }
      if (cmd == "chk") {
        printf("status %d\n", g2codec::g2_status(w));
        continue;
      }
      uint8_t b[64];
      const char* why = g2codec::g2_compress(w, b);
      if (why) {
        printf("refused %s\n", why);
        continue;
      }
      printf("bytes ");
      for (int i = 0; i < 64; i++) printf("%02x", b[i]);
      printf("\n");
    } else if (cmd == "dec") {
      std::string h;
      if (!(in >> h) || h.size() != 128) {
        printf("bad input\n");
        return 2;
      }
      uint8_t b[64];
      for (int i = 0; i < 64; i++) b[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
      const char* why = g2codec::g2_decompress(b, w);
      if (why) {
        printf("refused %s\n", why);
        continue;
      }
      const pairing::G2Affine q = pairing::g2_from_words(w);
      printf("pt %s %s %s %s\n", hex_fq(q.x.c0).c_str(), hex_fq(q.x.c1).c_str(), hex_fq(q.y.c0).c_str(), hex_fq(q.y.c1).c_str());
    } else {
      printf("bad command\n");
      return 2;
    }
  }
  printf("ok\n");
  return 0;
}
