// Driver for tests/test_multiopen_cpp_mirror.py: ProverSHPLONK / ProverGWC of include/amdzk_halo2.hpp over three
// polynomials at two points.
//   multiopen_mirror_check <k> <tau hex>
// Polynomial i has coefficient j = 1 + 7 i + 13 j + i j; the points are 3 and 5; polynomial 0 is opened at both,
// polynomial 1 at 3 (twice), polynomial 2 at 5. The transcript's challenges are a counter (1000, 1001, ..), so the test
// can drive the oracle with the same ones. Prints per scheme the written points (Montgomery words, hex) twice — as
// create_proof returned them and as the transcript received them — then the same with the evaluations supplied, and what
// a throwing transcript gives.
#include <cstdio>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "amdzk_halo2.hpp"

using namespace amdzk::halo2;

struct CountingTranscript : TranscriptWrite {
  std::vector<G1Affine> written;
  size_t squeezes = 0, others = 0;
  bool throwing = false;
  void common_point(const G1Affine&) override { others++; }
  void common_scalar(const Fr&) override { others++; }
  void write_point(const G1Affine& p) override {
    if (throwing) throw std::runtime_error("write_point failed");
    written.push_back(p);
  }
  void write_scalar(const Fr&) override { others++; }
  Fr squeeze_challenge() override { return Fr::from_u64(1000 + squeezes++); }
};

static void print_points(const char* tag, const std::vector<G1Affine>& pts) {
  for (const G1Affine& p : pts) {
    std::printf("%s", tag);
    for (int i = 0; i < 4; i++) std::printf(" %016llx", (unsigned long long)p.x[i]);
    for (int i = 0; i < 4; i++) std::printf(" %016llx", (unsigned long long)p.y[i]);
    std::printf("\n");
  }
}

template <class Prover>
static void run(const char* name, const Prover& prover, const std::vector<ProverQuery>& queries) {
  for (int with_evals = 0; with_evals < 2; with_evals++) {
    CountingTranscript t;
    const std::vector<G1Affine> pts = prover.create_proof(t, queries, with_evals != 0);
    const std::string tag = std::string(name) + (with_evals ? "_evals" : "");
    print_points((tag + "_returned").c_str(), pts);
    print_points((tag + "_written").c_str(), t.written);
    std::printf("%s_calls %zu %zu\n", tag.c_str(), t.squeezes, t.others);
  }
  CountingTranscript t;
  t.throwing = true;
  try {
    prover.create_proof(t, queries);
    std::printf("%s_throwing: accepted\n", name);
  } catch (const std::runtime_error& e) {
    std::printf("%s_throwing: %s\n", name, e.what());
  }
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s <k> <tau hex>\n", argv[0]);
    return 2;
  }
  try {
    const uint32_t k = (uint32_t)std::atoi(argv[1]);
    const size_t n = (size_t)1 << k;
    Context ctx(0);
    ParamsKZG params = ParamsKZG::setup(ctx, k, Fr::from_hex(argv[2]));
    std::vector<Fr> flat(3 * n);
    for (size_t i = 0; i < 3; i++)
      for (size_t j = 0; j < n; j++) flat[i * n + j] = Fr::from_u64(1 + 7 * i + 13 * j + i * j);
    void* d = nullptr;
    ctx.check(amdzk_dev_alloc(ctx.get(), flat.size() * sizeof(Fr), &d));
    ctx.check(amdzk_dev_upload(ctx.get(), d, flat.data(), flat.size() * sizeof(Fr)));
    auto poly = [&](size_t i) { return (const void*)((const char*)d + i * n * sizeof(Fr)); };
    auto eval = [&](size_t i, const Fr& x) {  // Horner on the host
      Fr acc = Fr::zero();
      for (size_t j = n; j-- > 0;) acc = acc * x + flat[i * n + j];
      return acc;
    };
    const Fr a = Fr::from_u64(3), b = Fr::from_u64(5);
    const std::vector<ProverQuery> queries = {{poly(0), a, eval(0, a)}, {poly(1), a, eval(1, a)}, {poly(0), b, eval(0, b)},
                                              {poly(2), b, eval(2, b)}, {poly(1), a, eval(1, a)}};
    run("shplonk", ProverSHPLONK(ctx, params), queries);
    run("gwc", ProverGWC(ctx, params), queries);
    amdzk_dev_free(ctx.get(), d);
    return 0;
  } catch (const Error& e) {
    std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
    return 1;
  }
}
