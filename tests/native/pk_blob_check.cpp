// The host-only parser of the proving-key file (csrc/pkblob.hpp) on its own, for a build under ASan + UBSan
// (tests/test_pk_blob.py): reads a key file that must parse, then applies the mutations of the Python test and expects
// every one to be refused —
//   one flipped bit at every byte position, every truncation length 0 .. len - 1, one byte appended,
//   every count field of the header enlarged to 2^31 with the digest recomputed (refused before anything is sized by it),
//   a description with 65537 permutation columns (the file that would carry it is too large to make).
// Usage: pk_blob_check <key file>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../anon-aadhaar-halo2_amd/csrc/pkblob.hpp"

static int parse(const std::vector<uint8_t>& b, size_t len, pkblob::Desc* out = nullptr) {
  // an exact-size copy: a read one byte past `len` is a heap overflow the sanitizer reports
  std::vector<uint8_t> exact(b.begin(), b.begin() + len);
  pkblob::Desc d;
  pkblob::Layout lay;
  std::string err;
  const int rc = pkblob::parse(exact.empty() ? (const uint8_t*)"" : exact.data(), len, out ? out : &d, &lay, &err);
  if (rc != AMDZK_OK && err.compare(0, 8, "pk_read:") != 0) {
    std::printf("FAILED: a refusal without a pk_read: message (%s)\n", err.c_str());
    std::exit(1);
  }
  return rc;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <key file>\n", argv[0]);
    return 2;
  }
  std::ifstream f(argv[1], std::ios::binary);
  std::vector<uint8_t> blob((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  pkblob::Desc d;
  if (parse(blob, blob.size(), &d) != AMDZK_OK) {
    std::printf("FAILED: the unmodified file is refused\n");
    return 1;
  }
  if (d.serialized_size() != blob.size()) {
    std::printf("FAILED: serialized_size %zu, file %zu\n", d.serialized_size(), blob.size());
    return 1;
  }
  {  // the header's writer gives the file's own first bytes back
    std::vector<uint8_t> h(d.header_bytes());
    d.write_header(h.data());
    if (!std::equal(h.begin(), h.end(), blob.begin())) {
      std::printf("FAILED: write_header differs from the file\n");
      return 1;
    }
  }
  std::printf("parsed k %u fixed %u advice %u perm %u challenges %u\n", d.k, d.num_fixed, d.num_advice, d.num_perm_columns(), d.num_challenges);
  size_t flips = 0, cuts = 0, counts = 0;
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
  // the count fields: walk the header the way the format lays it out
  std::vector<size_t> at = {16, 20, 24};  // num_fixed, num_advice, num_instance
  size_t pos = 12 + 24;
  for (const auto* q : {&d.advice_queries, &d.fixed_queries, &d.instance_queries}) {
    at.push_back(pos);
    pos += 4 + 4 * q->size();
  }
  at.insert(at.end(), {pos, pos + 4, pos + 8});  // num_gates, num_lookups, num_exprs
  pos += 12 + 4 * d.lookup_shape.size();
  at.push_back(pos + 4 * d.expr_offsets.size() - 4);  // expr_offsets[num_exprs] = the number of words
  pos += 4 * (d.expr_offsets.size() + d.expr_words.size());
  at.push_back(pos);  // num_constants
  pos += 4 + 8 * d.constants.size();
  at.push_back(pos);  // num_perm_columns
  pos += 4 + 4 * d.perm_columns.size();
  if (d.has_phases) at.push_back(pos + 1);  // num_challenges
  for (size_t off : at) {
    std::vector<uint8_t> m = blob;
    const uint32_t big = 1u << 31;
    memcpy(m.data() + off, &big, 4);
    pkblob::digest(m.data(), m.size() - pkblob::DIGEST_BYTES, m.data() + m.size() - pkblob::DIGEST_BYTES);
    if (parse(m, m.size()) == AMDZK_OK) {
      std::printf("FAILED: the count at byte %zu enlarged to 2^31 is accepted\n", off);
      return 1;
    }
    counts++;
  }
  {  // 65536 columns of a kind, the permutation's included: the bound that keeps the size arithmetic from wrapping
    pkblob::Desc many = d;
    std::string err;
    if (d.perm_columns.empty() || pkblob::validate(many, &err) != AMDZK_OK) {
      std::printf("FAILED: the file's own description does not validate (%s)\n", err.c_str());
      return 1;
    }
    many.perm_columns.clear();  // the file's first permutation column, over and over
    for (uint32_t i = 0; i < pkblob::MAX_COLUMNS + 1; i++) many.perm_columns.insert(many.perm_columns.end(), {d.perm_columns[0], d.perm_columns[1]});
    if (pkblob::validate(many, &err) == AMDZK_OK || err.find("65536") == std::string::npos) {
      std::printf("FAILED: 65537 permutation columns are accepted (%s)\n", err.c_str());
      return 1;
    }
    many.perm_columns.resize(2 * (size_t)pkblob::MAX_COLUMNS);
    if (pkblob::validate(many, &err) != AMDZK_OK) {
      std::printf("FAILED: 65536 permutation columns are refused (%s)\n", err.c_str());
      return 1;
    }
  }
  std::printf("flips %zu refused\ntruncations %zu refused\ncounts %zu refused\npk_blob_check ok\n", flips, cuts, counts);
  return 0;
}
