// Driver for tests/test_phased_cpp_mirror.py: the challenge-phase part of include/amdzk_halo2.hpp.
//   describe <rlc|rlc3> <k>     print the flattened C-ABI arrays and the phase table (no GPU call)
//   errors                      print what advice_column_in / challenge_usable_after refuse (no GPU call)
//   prove <rlc|rlc3> <k> <witness> <seed> <tau hex> <transcript_repr hex>
//                               keygen + create_proof with a synthesize functor on the GPU: the proof as hex and the
//                               challenges handed to the functor; then the same proof through a TranscriptWrite object
// The circuit mirrors tests/phased_circuits.py rlc_circuit statement for statement.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "amdzk_halo2.hpp"

using namespace amdzk::halo2;

struct Rlc {
  Column a, b, r, s, q, t0, t1;
  Challenge ch, ch2;
  bool three;
};

static Rlc configure(ConstraintSystem& cs, const std::string& name) {
  Rlc c{};
  c.three = name == "rlc3";
  if (name != "rlc" && !c.three) throw Error(AMDZK_E_INVALID, "unknown circuit " + name);
  c.a = cs.advice_column();
  c.b = cs.advice_column();
  c.r = cs.advice_column_in(1);
  c.ch = cs.challenge_usable_after(0);
  if (c.three) {
    c.s = cs.advice_column_in(2);
    c.ch2 = cs.challenge_usable_after(1);
  }
  c.q = cs.selector();
  c.t0 = cs.fixed_column();
  c.t1 = cs.fixed_column();
  cs.enable_equality(c.a);
  cs.enable_equality(c.r);
  // queries are numbered in first-use order: named locals fix the order the Python fixture queries in
  cs.create_gate("rlc", [&](VirtualCells& m) {
    Expression a = m.query_advice(c.a, Rotation::cur());
    Expression b = m.query_advice(c.b, Rotation::cur());
    Expression rlc = a + Expression::challenge(c.ch) * b;
    Expression q = m.query_selector(c.q);
    Expression r = m.query_advice(c.r, Rotation::cur());
    std::vector<Expression> out = {q * (r - rlc)};
    if (c.three) {
      Expression q2 = m.query_selector(c.q);
      Expression s = m.query_advice(c.s, Rotation::cur());
      Expression r2 = m.query_advice(c.r, Rotation::cur());
      Expression a1 = m.query_advice(c.a, Rotation::next());
      out.push_back(q2 * (s - (r2 * Expression::challenge(c.ch2) + Expression::challenge(c.ch) * a1)));
    }
    return out;
  });
  cs.lookup("rlc table", [&](VirtualCells& m) {
    Expression a = m.query_advice(c.a, Rotation::cur());
    Expression b = m.query_advice(c.b, Rotation::cur());
    Expression t0 = m.query_fixed(c.t0, Rotation::cur());
    Expression t1 = m.query_fixed(c.t1, Rotation::cur());
    return std::vector<std::pair<Expression, Expression>>{{a + Expression::challenge(c.ch) * b, t0 + Expression::challenge(c.ch) * t1}};
  });
  return c;
}

template <class T>
static void dump(const char* tag, const std::vector<T>& v) {
  std::cout << tag;
  for (auto& x : v) std::cout << ' ' << (long long)x;
  std::cout << '\n';
}

static int describe(const std::string& name, uint32_t k) {
  ConstraintSystem cs;
  configure(cs, name);
  CircuitData cd(cs, k);
  std::cout << "shape " << cd.c.k << ' ' << cd.c.num_fixed << ' ' << cd.c.num_advice << ' ' << cd.c.num_instance << ' ' << cd.c.blinding_factors << ' '
            << cd.c.cs_degree << ' ' << cd.c.num_gates << ' ' << cd.c.num_lookups << ' ' << cd.c.num_exprs << ' ' << cs.minimum_rows() << '\n';
  dump("aq", cd.aq);
  dump("fq", cd.fq);
  dump("iq", cd.iq);
  dump("lookup_shape", cd.lookup_shape);
  dump("expr_offsets", cd.expr_offsets);
  dump("expr_words", cd.expr_words);
  std::cout << "constants";
  for (uint64_t w : cd.constants) std::printf(" %016llx", (unsigned long long)w);
  std::cout << '\n';
  dump("perm", cd.perm_columns);
  std::cout << "phased " << (cd.phased ? 1 : 0) << ' ' << cd.phases.num_challenges << '\n';
  dump("advice_phase", std::vector<int>(cd.phases.advice_phase, cd.phases.advice_phase + cd.c.num_advice));
  dump("challenge_phase", std::vector<int>(cd.phases.challenge_phase, cd.phases.challenge_phase + cd.phases.num_challenges));
  return 0;
}

template <class F>
static void refused(const char* what, F&& f) {
  try {
    f();
    std::cout << what << ": accepted\n";
  } catch (const Error& e) {
    std::cout << what << ": " << e.code << ' ' << e.what() << '\n';
  }
}

static int errors() {
  ConstraintSystem cs;
  refused("advice_column_in(1) first", [&] { cs.advice_column_in(1); });
  refused("challenge_usable_after(0) first", [&] { cs.challenge_usable_after(0); });
  cs.advice_column();
  refused("advice_column_in(2) without phase 1", [&] { cs.advice_column_in(2); });
  refused("advice_column_in(3)", [&] { cs.advice_column_in(3); });
  refused("challenge_usable_after(1) without phase 1", [&] { cs.challenge_usable_after(1); });
  refused("challenge_usable_after(0)", [&] { cs.challenge_usable_after(0); });
  refused("advice_column_in(1)", [&] { cs.advice_column_in(1); });
  std::cout << "degree of a challenge " << Expression::challenge(Challenge{0, 0}).degree() << '\n';
  std::cout << "phased " << (cs.phased() ? 1 : 0) << '\n';
  return 0;
}

// a TranscriptWrite that owns nothing but a log: challenges are a counter, so the proof it drives is reproducible
struct CountingTranscript : TranscriptWrite {
  size_t points = 0, scalars = 0, squeezes = 0;
  void common_point(const G1Affine&) override { points++; }
  void common_scalar(const Fr&) override { scalars++; }
  void write_point(const G1Affine&) override { points++; }
  void write_scalar(const Fr&) override { scalars++; }
  Fr squeeze_challenge() override { return Fr::from_u64(1000 + squeezes++); }
};

static int prove(char** argv) {
  const std::string name = argv[2];
  const uint32_t k = (uint32_t)std::atoi(argv[3]);
  const size_t n = (size_t)1 << k;
  ConstraintSystem cs;
  const Rlc c = configure(cs, name);
  const size_t usable = n - (cs.blinding_factors() + 1);
  std::vector<std::vector<Fr>> fixed(cs.num_fixed, std::vector<Fr>(n, Fr::zero())), advice(cs.num_advice, std::vector<Fr>(n, Fr::zero()));
  Assembly assembly(n, cs.permutation_columns.size());
  std::ifstream f(argv[4]);
  if (!f) throw Error(AMDZK_E_INVALID, "cannot open witness file");
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    std::string tag;
    ss >> tag;
    if (tag == "F" || tag == "A") {
      size_t col, row;
      std::string hex;
      ss >> col >> row >> hex;
      (tag == "F" ? fixed : advice).at(col).at(row) = Fr::from_hex(hex);
    } else if (tag == "C") {
      size_t lc, lr, rc, rr;
      ss >> lc >> lr >> rc >> rr;
      assembly.copy(lc, lr, rc, rr);
    }
  }
  const uint64_t seed = std::strtoull(argv[5], nullptr, 10);
  Context ctx(0);
  ParamsKZG params = ParamsKZG::setup(ctx, k, Fr::from_hex(argv[6]));
  ProvingKey pk(ctx, params, cs, fixed, assembly, Fr::from_hex(argv[7]), 0);
  std::vector<Fr> flat(advice.size() * n, Fr::zero());
  for (size_t col = 0; col < 2; col++) std::copy(advice[col].begin(), advice[col].end(), flat.begin() + col * n);  // phase 0 only
  void* d = nullptr;
  ctx.check(amdzk_dev_alloc(ctx.get(), flat.size() * sizeof(Fr), &d));
  std::vector<std::vector<Fr>> seen;
  Synthesize synthesize = [&](uint32_t phase, const std::vector<Fr>& ch, void*) {
    seen.push_back(ch);
    std::vector<Fr>& out = advice[phase == 1 ? c.r.index : c.s.index];
    for (size_t row = 0; row < usable; row++)
      out[row] = phase == 1 ? advice[c.a.index][row] + ch[c.ch.index] * advice[c.b.index][row]
                            : advice[c.r.index][row] * ch[c.ch2.index] + ch[c.ch.index] * advice[c.a.index][(row + 1) % n];
    const size_t col = phase == 1 ? c.r.index : c.s.index;
    ctx.check(amdzk_dev_upload(ctx.get(), (char*)d + col * n * sizeof(Fr), out.data(), n * sizeof(Fr)));
  };
  for (int pass = 0; pass < 2; pass++) {
    for (size_t col = 2; col < advice.size(); col++) std::fill(advice[col].begin(), advice[col].end(), Fr::zero());
    ctx.check(amdzk_dev_upload(ctx.get(), d, flat.data(), flat.size() * sizeof(Fr)));
    seen.clear();
    CountingTranscript ct;
    std::vector<uint8_t> proof = create_proof(ctx, {&pk}, {{}}, {d}, n, seed, synthesize, pass ? &ct : nullptr);
    if (pass == 0) {
      std::cout << "proof ";
      for (uint8_t b : proof) std::printf("%02x", b);
      std::cout << '\n';
    } else {
      std::cout << "object " << proof.size() << ' ' << ct.points << ' ' << ct.scalars << ' ' << ct.squeezes << '\n';
    }
    for (auto& ch : seen) {
      std::cout << (pass ? "object_callback" : "callback");
      for (auto& v : ch) {
        uint64_t raw[4];
        v.to_repr(raw);
        std::printf(" %016llx%016llx%016llx%016llx", (unsigned long long)raw[3], (unsigned long long)raw[2], (unsigned long long)raw[1],
                    (unsigned long long)raw[0]);
      }
      std::cout << '\n';
    }
  }
  // a functor that throws: the exception comes back out of create_proof, and the key proves again afterwards
  try {
    create_proof(ctx, {&pk}, {{}}, {d}, n, seed, [](uint32_t, const std::vector<Fr>&, void*) { throw std::runtime_error("synthesize failed"); });
    std::cout << "throwing: accepted\n";
  } catch (const std::runtime_error& e) {
    std::cout << "throwing: " << e.what() << '\n';
  }
  for (size_t col = 2; col < advice.size(); col++) std::fill(advice[col].begin(), advice[col].end(), Fr::zero());
  ctx.check(amdzk_dev_upload(ctx.get(), d, flat.data(), flat.size() * sizeof(Fr)));
  std::cout << "again ";
  for (uint8_t b : create_proof(ctx, {&pk}, {{}}, {d}, n, seed, synthesize)) std::printf("%02x", b);
  std::cout << '\n';
  amdzk_dev_free(ctx.get(), d);
  return 0;
}

int main(int argc, char** argv) {
  try {
    if (argc == 4 && std::string(argv[1]) == "describe") return describe(argv[2], (uint32_t)std::atoi(argv[3]));
    if (argc == 2 && std::string(argv[1]) == "errors") return errors();
    if (argc == 8 && std::string(argv[1]) == "prove") return prove(argv);
    std::fprintf(stderr, "usage: %s describe <rlc|rlc3> <k> | errors | prove <rlc|rlc3> <k> <witness> <seed> <tau hex> <transcript_repr hex>\n", argv[0]);
    return 2;
  } catch (const Error& e) {
    std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
    return 1;
  }
}
