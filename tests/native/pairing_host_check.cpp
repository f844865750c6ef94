// Host build of the pairing unit — the host half with its programs (csrc/pairing.hpp) and the ZK_HD device half, the Fq2
// layer and the executor (csrc/fq12.cuh), exactly as pairing.hip's kernels run them: the same program words through the
// same executor — with the documented fp29 bounds compiled in as hard failures (FP29_CHECK_BOUNDS), driven
// by tests/test_pairing_host.py against tests/pairing_ref.py. Commands on stdin, one per line, numbers in hex (plain
// integers below the modulus):
//   setup S                       -> "g2 x0 x1 y0 y1" (the generator) and "sg2 x0 x1 y0 y1" (S * generator)
//   prod M  then M lines "px py qx0 qx1 qy0 qy1" ((0, 0) = the G1 identity)
//                                 -> "gt" and the 12 Fq of prod e(P_j, Q_j) in halo2curves' declaration order
// Self-checks of the tower run first. The last line is "ok".
#define FP29_CHECK_BOUNDS 1
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../anon-aadhaar-halo2_amd/csrc/pairing.hpp"

using namespace bn254;

static bool parse_hex(const std::string& s, uint64_t w[4]) {
  w[0] = w[1] = w[2] = w[3] = 0;
  if (s.empty() || s.size() > 64) return false;
  for (char ch : s) {
    int d = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1;
    if (d < 0) return false;
    for (int i = 3; i > 0; i--) w[i] = (w[i] << 4) | (w[i - 1] >> 60);
    w[0] = (w[0] << 4) | (uint64_t)d;
  }
  return true;
}
static bool parse_fq(const std::string& s, Fq* out) {
  uint64_t w[4];
  if (!parse_hex(s, w)) return false;
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
static void print_g2(const char* tag, const pairing::G2Affine& q) {
  printf("%s %s %s %s %s\n", tag, hex_fq(q.x.c0).c_str(), hex_fq(q.x.c1).c_str(), hex_fq(q.y.c0).c_str(), hex_fq(q.y.c1).c_str());
}
struct Machine {  // what a lane of pairing.hip has: the constants and a slab of registers
  Fq2x K[pairing::K_COUNT];
  std::vector<Fq2x> R;
  Machine() : R(256) { pairing::device_consts(K); }
  void run(const pairing::Prog& p, const Fq* lines = nullptr) { pairing_exec(p.w.data(), (uint32_t)p.w.size(), R.data(), K, lines); }
};
static bool eq12(const Fq2x* a, const Fq2x* b) {
  Fq x[12], y[12];
  fq12x_to_r256(x, a);
  fq12x_to_r256(y, b);
  return memcmp(x, y, sizeof(x)) == 0;
}

// the Miller value of (p, q) into R[MILLER_F..], as pairing_miller_kernel does
static void miller_of(Machine& M, const pairing::Prog& miller, const G1Affine& p, const pairing::G2Affine& q) {
  if (p.is_inf()) {
    M.R[pairing::MILLER_F] = fq2x_one();
    for (int k = 1; k < 6; k++) M.R[pairing::MILLER_F + k] = fq2x_zero();
    return;
  }
  std::vector<Fq> lines(4 * PAIRING_NUM_LINES);
  pairing::g2_prepare(q, lines.data());
  M.R[pairing::MILLER_XP] = Fq2x{fq29_from_r256(p.x), fqx_zero()};
  M.R[pairing::MILLER_YP] = Fq2x{fq29_from_r256(p.y), fqx_zero()};
  M.run(miller, lines.data());
}

// The emitters on a generic element (a Miller value) and on an element of the cyclotomic subgroup: X = 0..5 holds the
// input, every check computes two six-register values and compares them.
static int self_checks(const pairing::Prog& miller, const pairing::Prog& fin) {
  int fails = 0;
  const pairing::G2Affine g2 = pairing::g2_generator();
  if (!pairing::g2_on_twist(g2)) fails++, printf("generator not on the twist\n");
  G1Affine g1;
  g1.x = Fq::one();
  g1.y = add(Fq::one(), Fq::one());
  Machine M;
  miller_of(M, miller, g1, g2);
  std::vector<Fq2x> f(M.R.begin() + pairing::MILLER_F, M.R.begin() + pairing::MILLER_F + 6);
  const int X = 0, U = 6, V = 12, base = 18;
  auto check = [&](const char* what, const std::vector<Fq2x>& in, void (*emit)(pairing::Prog&, int, int, int), bool want_equal = true) {
    pairing::Prog p;
    p.alloc(base);
    emit(p, X, U, V);
    Machine T;
    for (int k = 0; k < 6; k++) T.R[X + k] = in[k];
    T.run(p);
    if (eq12(&T.R[U], &T.R[V]) != want_equal) fails++, printf("%s\n", what);
  };
  check("inv", f, [](pairing::Prog& p, int x, int u, int v) { pairing::e12_inv(p, u, x), pairing::e12_mul(p, u, u, x), pairing::e12_one(p, v); });
  check("sqr", f, [](pairing::Prog& p, int x, int u, int v) { pairing::e12_sqr(p, u, x), pairing::e12_mul(p, v, x, x); });
  check("sqr in place", f, [](pairing::Prog& p, int x, int u, int v) { pairing::e12_mul(p, v, x, x), pairing::e12_mov(p, u, x), pairing::e12_sqr(p, u, u); });
  check("frobenius 2", f, [](pairing::Prog& p, int x, int u, int v) { pairing::e12_frobenius(p, u, x, 1), pairing::e12_frobenius(p, u, u, 1), pairing::e12_frobenius(p, v, x, 2); });
  check("frobenius 3", f, [](pairing::Prog& p, int x, int u, int v) {
    pairing::e12_frobenius(p, u, x, 2), pairing::e12_frobenius(p, u, u, 1), pairing::e12_frobenius(p, v, x, 3);
  });
  Machine E;  // into the cyclotomic subgroup
  for (int k = 0; k < 6; k++) E.R[pairing::FINAL_A + k] = f[k];
  E.run(fin);
  std::vector<Fq2x> e(E.R.begin() + pairing::FINAL_A, E.R.begin() + pairing::FINAL_A + 6);
  check("cyclotomic sqr", e, [](pairing::Prog& p, int x, int u, int v) { pairing::e12_cyclotomic_sqr(p, u, x), pairing::e12_sqr(p, v, x); });
  check("conj", e, [](pairing::Prog& p, int x, int u, int v) { pairing::e12_conj(p, u, x), pairing::e12_mul(p, u, u, x), pairing::e12_one(p, v); });
  check("degenerate", e, [](pairing::Prog& p, int x, int u, int v) { pairing::e12_mov(p, u, x), pairing::e12_one(p, v); }, false);
  return fails;
}

int main() {
  const pairing::Prog miller = pairing::miller_program(), mulp = pairing::mul_program(), fin = pairing::final_exp_program();
  if (miller.regs > 256 || fin.regs > 256 || mulp.regs > 256) return 1;  // a register index is 8 bits
  if (self_checks(miller, fin)) return 1;
  printf("selfcheck ok\n");
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "setup") {
      std::string s;
      uint64_t k[4];
      if (!(in >> s) || !parse_hex(s, k)) return 2;
      const pairing::G2Affine g2 = pairing::g2_generator();
      print_g2("g2", g2);
      print_g2("sg2", pairing::g2_mul(g2, k));
    } else if (cmd == "prod") {
      size_t m = 0;
      if (!(in >> m) || m == 0 || m > 16) return 2;
      Machine A;  // the final kernel's lane: A = the first Miller value, then A = A * B for every further one
      for (size_t j = 0; j < m; j++) {
        if (!std::getline(std::cin, line)) return 2;
        std::istringstream pin(line);
        std::string t[6];
        Fq v[6];
        for (int i = 0; i < 6; i++)
          if (!(pin >> t[i]) || !parse_fq(t[i], &v[i])) return 2;
        G1Affine p;
        p.x = v[0], p.y = v[1];
        const pairing::G2Affine q{pairing::Fq2{v[2], v[3]}, pairing::Fq2{v[4], v[5]}};
        if (!pairing::g2_on_twist(q)) return 3;
        Machine L;
        miller_of(L, miller, p, q);
        for (int k = 0; k < 6; k++) A.R[(j ? pairing::FINAL_B : pairing::FINAL_A) + k] = L.R[pairing::MILLER_F + k];
        if (j) A.run(mulp);
      }
      A.run(fin);
      Fq out[12];
      fq12x_to_r256(out, &A.R[pairing::FINAL_A]);
      printf("gt");
      for (int i = 0; i < 12; i++) printf(" %s", hex_fq(out[i]).c_str());
      printf(" %d\n", gt_is_one(out) ? 1 : 0);
    } else {
      return 2;
    }
  }
  printf("ok\n");
  return 0;
}
