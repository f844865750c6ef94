// Driver for tests/test_verify_mixed_cpp_mirror.py: verify_proofs / decide_proofs of include/amdzk_halo2.hpp over a list of
// VerifyItem — proofs of different circuits under different keys in one call.
//   verify_mixed_mirror_check <tau hex> <k A> <key file A> <proof file A> <k B> <key file B> <proof file B> <foreign vk file>
// Key A is read over the setup downsized to k A (k A <= k B), key B over the setup at k B and turned into a verifying key; the
// public inputs come from "<key file>.inst" (as tests/native/verify_mirror_check.cpp). Blake2b, SHPLONK.
// Prints "single <status> <offset> <pair>" (verify_proofs, key A, [A, A], seed 7), "same <...>" (the same batch as items:
// equal words), "mixed <status A> <status B> <status A'> <pair>" (items [A under pk, B under vk, A with a flipped byte] with
// weights 2, 3, 5), "decide <verdicts> <n_valid>" per proof and "combined <verdicts> <n_valid>" for that batch, and
// "refused: <message>" for an item list whose second key — the verifying-key file of circuit A made over a setup with another
// G — breaks the one rule, and "after <verdict> <n_valid>": the ctx decides item B afterwards.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "amdzk_halo2.hpp"

using namespace amdzk::halo2;

static std::vector<uint8_t> slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw Error(AMDZK_E_INVALID, std::string("cannot open ") + path);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static std::vector<std::vector<Fr>> instances_of(const char* key_file) {
  std::vector<std::vector<Fr>> instances;
  std::ifstream f(std::string(key_file) + ".inst");
  if (!f) throw Error(AMDZK_E_INVALID, "cannot open the instance file");
  std::string line, hex;
  while (std::getline(f, line)) {
    instances.emplace_back();
    std::istringstream is(line);
    while (is >> hex) instances.back().push_back(Fr::from_hex(hex));
  }
  return instances;
}
static void print_words(const uint64_t w[4]) {
  std::printf(" %016llx%016llx%016llx%016llx", (unsigned long long)w[3], (unsigned long long)w[2], (unsigned long long)w[1], (unsigned long long)w[0]);
}
static void print_guard(const char* tag, const Guard& g) {
  std::printf("%s", tag);
  for (const ProofStatus& s : g.statuses) std::printf(" %u %u", (unsigned)s.status, s.offset);
  print_words(g.lhs.x), print_words(g.lhs.y), print_words(g.rhs.x), print_words(g.rhs.y);
  std::printf("\n");
}
static void print_decision(const char* tag, const Decision& d) {
  std::printf("%s", tag);
  for (bool v : d.verdicts) std::printf(" %d", (int)v);
  std::printf(" %zu\n", d.n_valid);
}

int main(int argc, char** argv) {
  if (argc != 9) {
    std::fprintf(stderr, "usage: %s <tau hex> <k A> <key file A> <proof file A> <k B> <key file B> <proof file B> <foreign vk file>\n", argv[0]);
    return 2;
  }
  try {
    const Fr tau = Fr::from_hex(argv[1]);
    const uint32_t ka = (uint32_t)std::atoi(argv[2]), kb = (uint32_t)std::atoi(argv[5]);
    const std::vector<std::vector<std::vector<Fr>>> inst_a{instances_of(argv[3])}, inst_b{instances_of(argv[6])};
    const std::vector<uint8_t> proof_a = slurp(argv[4]), proof_b = slurp(argv[7]);
    std::vector<uint8_t> bad_a = proof_a;
    bad_a[bad_a.size() - 1] ^= 0x40;  // the last point's x: still a proof of the right length
    Context ctx(0);
    ParamsKZG params_b = ParamsKZG::setup(ctx, kb, tau), params_a = ParamsKZG::setup(ctx, kb, tau);
    params_a.downsize(ka);
    ParamsVerifierKZG vparams = ParamsVerifierKZG::setup(ctx, tau);
    std::unique_ptr<ProvingKey> pk_a = ProvingKey::read(ctx, params_a, slurp(argv[3]));
    std::unique_ptr<VerifyingKey> vk_b;
    {
      std::unique_ptr<ProvingKey> pk_b = ProvingKey::read(ctx, params_b, slurp(argv[6]));
      vk_b = pk_b->get_vk();
    }
    print_guard("single", verify_proofs(ctx, *pk_a, {inst_a, inst_a}, {proof_a, proof_a}, Transcript::Blake2b, Multiopen::Shplonk, 7));
    print_guard("same", verify_proofs(ctx, {VerifyItem(*pk_a, inst_a, proof_a), VerifyItem(*pk_a, inst_a, proof_a)}, 7));
    const std::vector<VerifyItem> items{VerifyItem(*pk_a, inst_a, proof_a), VerifyItem(*vk_b, inst_b, proof_b, Transcript::Blake2b, Multiopen::Shplonk),
                                        VerifyItem(*pk_a, inst_a, bad_a)};
    print_guard("mixed", verify_proofs(ctx, items, 0, {Fr::from_u64(2), Fr::from_u64(3), Fr::from_u64(5)}));
    print_decision("decide", decide_proofs(ctx, vparams, items));
    print_decision("combined", decide_proofs(ctx, vparams, items, true, 99));
    std::unique_ptr<VerifyingKey> foreign = VerifyingKey::read(ctx, slurp(argv[8]));
    try {
      verify_proofs(ctx, {VerifyItem(*pk_a, inst_a, proof_a), VerifyItem(*foreign, inst_a, proof_a)});
      std::printf("refused: no\n");
    } catch (const Error& e) {
      std::printf("refused: %s\n", e.what());
    }
    print_decision("after", decide_proofs(ctx, vparams, {items[1]}));
    return 0;
  } catch (const Error& e) {
    std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
    return 1;
  }
}
