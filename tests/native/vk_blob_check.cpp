// The host-only parser of the verifying-key file (csrc/vkblob.hpp) on its own, for a build under ASan + UBSan
// (tests/test_vk_blob.py). The first file must parse; it then gets the exhaustive mutations of the Python test —
//   one flipped bit at every byte position, every truncation length 0 .. len - 1, one byte appended —
// and every one must be refused. Each further pair is a file the test has mutated (digest recomputed) and the reason the
// parser must give for refusing it: alternatives separated by '|', one of which must occur in the message.
// Usage: vk_blob_check <key file> [<mutated file> <reason>]...
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../anon-aadhaar-halo2_amd/csrc/vkblob.hpp"

static std::vector<uint8_t> slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static int parse(const std::vector<uint8_t>& b, size_t len, pkblob::Desc* out = nullptr, vkblob::Layout* lay = nullptr, std::string* why = nullptr) {
  // an exact-size copy: a read one byte past `len` is a heap overflow the sanitizer reports
  std::vector<uint8_t> exact(b.begin(), b.begin() + len);
  pkblob::Desc d;
  vkblob::Layout l;
  std::string err;
  const int rc = vkblob::parse(exact.empty() ? (const uint8_t*)"" : exact.data(), len, out ? out : &d, lay ? lay : &l, &err);
  if (rc != AMDZK_OK && err.compare(0, 8, "vk_read:") != 0) {
    std::printf("FAILED: a refusal without a vk_read: message (%s)\n", err.c_str());
    std::exit(1);
  }
  if (why) *why = err;
  return rc;
}

int main(int argc, char** argv) {
  if (argc < 2 || argc % 2 != 0) {
    std::fprintf(stderr, "usage: %s <key file> [<mutated file> <reason>]...\n", argv[0]);
    return 2;
  }
  const std::vector<uint8_t> blob = slurp(argv[1]);
  pkblob::Desc d;
  vkblob::Layout L;
  if (parse(blob, blob.size(), &d, &L) != AMDZK_OK) {
    std::printf("FAILED: the unmodified file is refused\n");
    return 1;
  }
  if (vkblob::serialized_size(d, L.with_g2) != blob.size() || L.total != blob.size()) {
    std::printf("FAILED: serialized_size %zu, file %zu\n", vkblob::serialized_size(d, L.with_g2), blob.size());
    return 1;
  }
  {  // the writer's frame gives the file's own bytes back: magic .. phase table and the has-g2 byte
    std::vector<uint8_t> w = blob;
    std::fill(w.begin(), w.begin() + L.transcript_repr, 0xEE);
    w[L.has_g2] = 0xEE;
    vkblob::write_frame(d, L, w.data());
    vkblob::seal(L, w.data());
    if (w != blob) {
      std::printf("FAILED: write_frame and seal differ from the file\n");
      return 1;
    }
  }
  std::printf("parsed k %u fixed %u advice %u perm %u challenges %u g2 %d\n", d.k, d.num_fixed, d.num_advice, d.num_perm_columns(), d.num_challenges,
              L.with_g2 ? 1 : 0);
  size_t flips = 0, cuts = 0, named = 0;
  for (size_t i = 0; i < blob.size(); i++) {
    std::vector<uint8_t> m = blob;
    m[i] ^= (uint8_t)(1u << (i % 8));
    if (parse(m, m.size()) == AMDZK_OK) {
      std::printf("FAILED: a flipped bit at byte %zu is accepted\n", i);
      return 1;
    }
    flips++;
  }
  for (size_t len = 0; len < blob.size(); len++) {
    if (parse(blob, len) == AMDZK_OK) {
      std::printf("FAILED: a file cut to %zu bytes is accepted\n", len);
      return 1;
    }
    cuts++;
  }
  {
    std::vector<uint8_t> m = blob;
    m.push_back(0);
    if (parse(m, m.size()) == AMDZK_OK) {
      std::printf("FAILED: a file with a byte appended is accepted\n");
      return 1;
    }
  }
  for (int a = 2; a + 1 < argc; a += 2) {
    const std::vector<uint8_t> m = slurp(argv[a]);
    const std::string want = argv[a + 1];
    std::string why;
    if (parse(m, m.size(), nullptr, nullptr, &why) == AMDZK_OK) {
      std::printf("FAILED: %s is accepted\n", argv[a]);
      return 1;
    }
    bool found = false;
    for (size_t lo = 0; lo <= want.size() && !found;) {
      const size_t hi = std::min(want.find('|', lo), want.size());
      found = hi > lo && why.find(want.substr(lo, hi - lo)) != std::string::npos;
      lo = hi + 1;
    }
    if (!found) {
      std::printf("FAILED: %s is refused with \"%s\", not with \"%s\"\n", argv[a], why.c_str(), want.c_str());
      return 1;
    }
    named++;
  }
  std::printf("flips %zu refused\ntruncations %zu refused\nnamed %zu refused\nvk_blob_check ok\n", flips, cuts, named);
  return 0;
}
