// Driver for tests/test_verify_read_cpp_mirror.py: verify_proof / verify_proofs / decide_proof of include/amdzk_halo2.hpp
// through a TranscriptRead of the caller's.
//   verify_read_mirror_check <k> <tau hex> <key file> <transcript: 0 | 1> <multiopen: 0 | 1> <proof file> <replay file>
// The key comes from a key file, the public inputs from "<key file>.inst" (as tests/native/verify_mirror_check.cpp). The
// replay file is what a reader of the proof's bytes hands back, call after call: lines "p <8 words>", "s <4 words>",
// "c <4 words>" (hex u64, Montgomery, least significant word first) — the driver's transcript replays it and throws when
// the library asks out of order.
// Prints "bytes <status> <offset> <pair>" (the bytes route), "read <status> <offset> <pair>" (the transcript, proving key),
// "read_vk ..." (verifying key), "decide <bytes> <read>", "calls <commons> <reads> <squeezes> <left over>",
// "throwing: <message>" (verify_proof with a transcript that throws at its 4th read), then "status <status> <offset>" per
// proof of verify_proofs over [the transcript, the throwing one].
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "amdzk_halo2.hpp"

using namespace amdzk::halo2;

static std::vector<uint8_t> slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw Error(AMDZK_E_INVALID, std::string("cannot open ") + path);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static void print_words(const uint64_t w[4]) {
  std::printf(" %016llx%016llx%016llx%016llx", (unsigned long long)w[3], (unsigned long long)w[2], (unsigned long long)w[1], (unsigned long long)w[0]);
}
static void print_guard(const char* tag, const Guard& g) {
  std::printf("%s %u %u", tag, (unsigned)g.statuses[0].status, g.statuses[0].offset);
  print_words(g.lhs.x), print_words(g.lhs.y), print_words(g.rhs.x), print_words(g.rhs.y);
  std::printf("\n");
}

struct Entry {
  char kind;
  uint64_t w[8];
};

struct Replay : TranscriptRead {
  const std::vector<Entry>& log;
  size_t next = 0, commons = 0, reads = 0, squeezes = 0;
  size_t throw_at_read = (size_t)-1;
  explicit Replay(const std::vector<Entry>& l) : log(l) {}
  const Entry& take(char kind) {
    if (next >= log.size() || log[next].kind != kind) throw std::runtime_error("the library asked out of order");
    return log[next++];
  }
  void common_point(const G1Affine&) override { throw std::runtime_error("common_point is not the verifier's to call"); }
  void common_scalar(const Fr&) override { commons++; }
  G1Affine read_point() override {
    if (reads == throw_at_read) throw std::runtime_error("read failed");
    G1Affine p;
    std::memcpy(&p, take('p').w, 64);
    reads++;
    return p;
  }
  Fr read_scalar() override {
    if (reads == throw_at_read) throw std::runtime_error("read failed");
    Fr v;
    std::memcpy(v.l, take('s').w, 32);
    reads++;
    return v;
  }
  Fr squeeze_challenge() override {
    Fr v;
    std::memcpy(v.l, take('c').w, 32);
    squeezes++;
    return v;
  }
};

int main(int argc, char** argv) {
  if (argc != 8) {
    std::fprintf(stderr, "usage: %s <k> <tau hex> <key file> <transcript> <multiopen> <proof file> <replay file>\n", argv[0]);
    return 2;
  }
  try {
    const uint32_t k = (uint32_t)std::atoi(argv[1]);
    const Fr tau = Fr::from_hex(argv[2]);
    const Transcript tr = std::atoi(argv[4]) ? Transcript::Keccak256Evm : Transcript::Blake2b;
    const Multiopen mo = std::atoi(argv[5]) ? Multiopen::Gwc : Multiopen::Shplonk;
    std::vector<std::vector<Fr>> instances;
    {
      std::ifstream f(std::string(argv[3]) + ".inst");
      if (!f) throw Error(AMDZK_E_INVALID, "cannot open the instance file");
      std::string line, hex;
      while (std::getline(f, line)) {
        instances.emplace_back();
        std::istringstream is(line);
        while (is >> hex) instances.back().push_back(Fr::from_hex(hex));
      }
    }
    std::vector<Entry> log;
    {
      std::ifstream f(argv[7]);
      if (!f) throw Error(AMDZK_E_INVALID, "cannot open the replay file");
      std::string line, tok;
      while (std::getline(f, line)) {
        std::istringstream is(line);
        Entry e{};
        is >> tok;
        e.kind = tok.empty() ? '?' : tok[0];
        for (int i = 0; i < (e.kind == 'p' ? 8 : 4); i++) {
          is >> tok;
          e.w[i] = std::strtoull(tok.c_str(), nullptr, 16);
        }
        log.push_back(e);
      }
    }
    const std::vector<uint8_t> proof = slurp(argv[6]);
    Context ctx(0);
    ParamsKZG params = ParamsKZG::setup(ctx, k, tau);
    ParamsVerifierKZG vparams = ParamsVerifierKZG::setup(ctx, tau);
    std::unique_ptr<ProvingKey> pk = ProvingKey::read(ctx, params, slurp(argv[3]));
    std::unique_ptr<VerifyingKey> vk = pk->get_vk();
    print_guard("bytes", verify_proof(ctx, *pk, instances, proof, tr, mo));
    Replay a(log), b(log), c(log), d(log), e(log), t(log);
    print_guard("read", verify_proof(ctx, *pk, instances, a, mo));
    print_guard("read_vk", verify_proof(ctx, *vk, instances, b, mo));
    std::printf("decide %d %d\n", (int)decide_proof(ctx, *pk, vparams, instances, proof, tr, mo), (int)decide_proof(ctx, *vk, vparams, instances, c, mo));
    std::printf("calls %zu %zu %zu %zu\n", a.commons, a.reads, a.squeezes, log.size() - a.next);
    t.throw_at_read = 3;
    try {
      verify_proof(ctx, *pk, instances, t, mo);
      std::printf("throwing: accepted\n");
    } catch (const std::runtime_error& err) {
      std::printf("throwing: %s\n", err.what());
    }
    e.throw_at_read = 3;
    const Guard g = verify_proofs(ctx, *pk, std::vector<std::vector<std::vector<std::vector<Fr>>>>(2, {instances}), std::vector<TranscriptRead*>{&d, &e}, mo, 7);
    for (const ProofStatus& s : g.statuses) std::printf("status %u %u\n", (unsigned)s.status, s.offset);
    return 0;
  } catch (const Error& e) {
    std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
    return 1;
  }
}
