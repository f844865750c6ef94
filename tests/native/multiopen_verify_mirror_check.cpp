// Driver for tests/test_multiopen_verify_cpp_mirror.py: VerifierSHPLONK / VerifierGWC of include/amdzk_halo2.hpp behind
// ProverSHPLONK / ProverGWC, over the polynomials, points and counter challenges of tests/native/multiopen_mirror_check.cpp.
//   multiopen_verify_mirror_check <k> <tau hex>
// Per scheme: the prover writes its points to a counting transcript; the verifier reads them back from a transcript with
// the same counter challenges (1000, 1001, ..) over commitments made with ParamsKZG::commit. Prints
// "<scheme>_commitment <x> <y>" per polynomial, "<scheme>_point <x> <y>" per written point, "<scheme>_guard <lhs> <rhs>",
// "<scheme>_calls <reads> <squeezes> <others>", "<scheme>_verdict <honest> <wrong evaluation> <wrong commitment>" and what
// a throwing transcript gives. Coordinates are Montgomery words, least significant first.
#include <cstdio>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "amdzk_halo2.hpp"

using namespace amdzk::halo2;

struct Writing : TranscriptWrite {
  std::vector<G1Affine> written;
  size_t squeezes = 0;
  void common_point(const G1Affine&) override {}
  void common_scalar(const Fr&) override {}
  void write_point(const G1Affine& p) override { written.push_back(p); }
  void write_scalar(const Fr&) override {}
  Fr squeeze_challenge() override { return Fr::from_u64(1000 + squeezes++); }
};

struct Reading : TranscriptRead {
  const std::vector<G1Affine>& points;
  size_t reads = 0, squeezes = 0, others = 0;
  bool throwing = false;
  explicit Reading(const std::vector<G1Affine>& p) : points(p) {}
  void common_point(const G1Affine&) override { others++; }
  void common_scalar(const Fr&) override { others++; }
  G1Affine read_point() override {
    if (throwing || reads >= points.size()) throw std::runtime_error("read_point failed");
    return points[reads++];
  }
  Fr read_scalar() override {
    others++;
    return Fr::zero();
  }
  Fr squeeze_challenge() override { return Fr::from_u64(1000 + squeezes++); }
};

static void print_point(const char* tag, const G1Affine& p) {
  std::printf("%s", tag);
  for (int i = 0; i < 4; i++) std::printf(" %016llx", (unsigned long long)p.x[i]);
  for (int i = 0; i < 4; i++) std::printf(" %016llx", (unsigned long long)p.y[i]);
  std::printf("\n");
}

template <class Prover, class Verifier>
static void run(const std::string& name, const Prover& prover, const Verifier& verifier, const ParamsVerifierKZG& vparams,
                const std::vector<ProverQuery>& pq, std::vector<VerifierQuery> vq) {
  Writing w;
  prover.create_proof(w, pq);
  for (const G1Affine& p : w.written) print_point((name + "_point").c_str(), p);
  Reading r(w.written);
  const OpeningGuard g = verifier.verify_proof(r, vq);
  std::printf("%s_guard", name.c_str());
  for (const G1Affine* p : {&g.lhs, &g.rhs}) {
    for (int i = 0; i < 4; i++) std::printf(" %016llx", (unsigned long long)p->x[i]);
    for (int i = 0; i < 4; i++) std::printf(" %016llx", (unsigned long long)p->y[i]);
  }
  std::printf("\n%s_calls %zu %zu %zu\n", name.c_str(), r.reads, r.squeezes, r.others);
  Reading a(w.written), b(w.written), c(w.written), t(w.written);
  const bool honest = verifier.decide(a, vq, vparams);
  std::vector<VerifierQuery> wrong_eval = vq, wrong_com = vq;
  wrong_eval[0].eval = wrong_eval[0].eval + Fr::from_u64(1);
  for (VerifierQuery& q : wrong_com)
    if (std::memcmp(&q.commitment, &vq[0].commitment, 64) == 0) q.commitment = vq[1].commitment;
  std::printf("%s_verdict %d %d %d\n", name.c_str(), (int)honest, (int)verifier.decide(b, wrong_eval, vparams), (int)verifier.decide(c, wrong_com, vparams));
  t.throwing = true;
  try {
    verifier.verify_proof(t, vq);
    std::printf("%s_throwing: accepted\n", name.c_str());
  } catch (const std::runtime_error& e) {
    std::printf("%s_throwing: %s\n", name.c_str(), e.what());
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
    const Fr tau = Fr::from_hex(argv[2]);
    Context ctx(0);
    ParamsKZG params = ParamsKZG::setup(ctx, k, tau);
    ParamsVerifierKZG vparams = ParamsVerifierKZG::setup(ctx, tau);
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
    std::vector<G1Affine> com(3);
    for (size_t i = 0; i < 3; i++) {
      const G1 c = params.commit(std::vector<Fr>(flat.begin() + i * n, flat.begin() + (i + 1) * n));
      std::memcpy(com[i].x, c.x, 32);
      std::memcpy(com[i].y, c.y, 32);
      print_point("commitment", com[i]);
    }
    const Fr a = Fr::from_u64(3), b = Fr::from_u64(5);
    const size_t which[5] = {0, 1, 0, 2, 1};
    const Fr at[5] = {a, a, b, b, a};
    std::vector<ProverQuery> pq;
    std::vector<VerifierQuery> vq;
    for (int i = 0; i < 5; i++) {
      pq.push_back({poly(which[i]), at[i], eval(which[i], at[i])});
      vq.push_back({com[which[i]], at[i], eval(which[i], at[i])});
    }
    const G1Affine g = params.get_g()[0];
    run("shplonk", ProverSHPLONK(ctx, params), VerifierSHPLONK(ctx, g), vparams, pq, vq);
    run("gwc", ProverGWC(ctx, params), VerifierGWC(ctx, g), vparams, pq, vq);
    amdzk_dev_free(ctx.get(), d);
    return 0;
  } catch (const Error& e) {
    std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
    return 1;
  }
}
