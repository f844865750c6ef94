// The verifying-key file (amdzk_vk_write / amdzk_vk_read / amdzk_vk_blob_info, include/amdzk.h): layout,
// writer, and the parser with every check the file gets — none of them needs a device. Host-only: no HIP include, compiles
// with g++ (tests/native/vk_blob_check.cpp runs it under ASan + UBSan).
//
// All integers little-endian, no padding, in this order:
//   magic "AMDZKVK\0" (8) | format version u32 = 1
//   the proving-key file's sections from amdzk_circuit through the phase table, byte for byte (pkblob.hpp:
//     Desc::write_circuit writes them, detail::read_circuit and validate read and check them)
//   transcript_repr 4 x u64
//   fixed commitments num_fixed x 64 B | permutation commitments num_perm_columns x 64 B      (amdzk_vk_commitments)
//   G = g[0] of the SRS the key was made on, 64 B                                              (G1Affine, Montgomery)
//   has_g2 u8 (0 / 1); if 1: g2 128 B | s_g2 128 B                          (G2Affine as include/amdzk.h lays it out)
//   BLAKE2b-512 of every byte before it, personalisation "amdzk_vk_blob_v1"                     64 B
// The file is self-delimiting: its length must be exactly what the header implies. A parse allocates at most the header's
// own size. Points are checked as far as an in-memory point is anywhere in this library: coordinates below q, on the curve
// (a commitment may also be (0, 0), the identity: an all-zero column commits to it), G and the G2 points finite; subgroup
// membership of the G2 points is NOT checked.
#pragma once
#include "pairing.hpp"
#include "pkblob.hpp"

namespace vkblob {

constexpr size_t MAGIC_BYTES = 8, DIGEST_BYTES = 64, G1_BYTES = 64, G2_BYTES = 128;
inline const char* magic() { return "AMDZKVK"; }  // 7 characters and the terminating NUL: 8 bytes
constexpr uint32_t FORMAT_VERSION = 1;

inline void digest(const uint8_t* data, size_t len, uint8_t out[DIGEST_BYTES]) {
  zkhost::Blake2b h("amdzk_vk_blob_v1");
  h.update(data, len);
  h.digest(out);
}

// Byte offsets of the sections; g2 = s_g2 = 0 in a file without the pair.
struct Layout {
  size_t circuit = 0, transcript_repr = 0, fixed_commitments = 0, perm_commitments = 0, g = 0, has_g2 = 0, g2 = 0, s_g2 = 0, digest = 0, total = 0;
  bool with_g2 = false;
};

inline Layout layout(const pkblob::Desc& d, bool with_g2) {
  Layout L;
  L.circuit = MAGIC_BYTES + 4;
  L.transcript_repr = L.circuit + d.circuit_bytes();
  L.fixed_commitments = L.transcript_repr + 32;
  L.perm_commitments = L.fixed_commitments + (size_t)d.num_fixed * G1_BYTES;
  L.g = L.perm_commitments + (size_t)d.num_perm_columns() * G1_BYTES;
  L.has_g2 = L.g + G1_BYTES;
  L.with_g2 = with_g2;
  L.digest = L.has_g2 + 1;
  if (with_g2) L.g2 = L.digest, L.s_g2 = L.g2 + G2_BYTES, L.digest = L.s_g2 + G2_BYTES;
  L.total = L.digest + DIGEST_BYTES;
  return L;
}
inline size_t serialized_size(const pkblob::Desc& d, bool with_g2) { return layout(d, with_g2).total; }

// magic .. has_g2 and the digest; the caller fills the sections in between (Layout says where) before it calls seal()
inline void write_frame(const pkblob::Desc& d, const Layout& L, uint8_t* out) {
  memcpy(out, magic(), MAGIC_BYTES);
  const uint32_t version = FORMAT_VERSION;
  memcpy(out + MAGIC_BYTES, &version, 4);
  d.write_circuit(out + L.circuit);
  out[L.has_g2] = L.with_g2 ? 1 : 0;
}
inline void seal(const Layout& L, uint8_t* out) { digest(out, L.digest, out + L.digest); }

namespace detail {
inline int fail(std::string* err, const char* fmt, unsigned long long a = 0, unsigned long long b = 0) {
  if (err) {
    char buf[256];
    snprintf(buf, sizeof(buf), fmt, a, b);
    *err = std::string("vk_read: ") + buf;
  }
  return AMDZK_E_INVALID;
}
// a refusal of pkblob's reader or validate(), under this file's prefix
inline int as_vk(int rc, std::string* err) {
  const std::string pk = "pk_read: ";
  if (rc != AMDZK_OK && err && err->compare(0, pk.size(), pk) == 0) *err = "vk_read: " + err->substr(pk.size());
  return rc;
}
inline bn254::Fq fq_at(const uint8_t* p) {
  bn254::Fq v;
  memcpy(v.l, p, 32);
  return v;
}
// 0: fine; 1: a coordinate >= q; 2: not on the curve; 3: the identity
inline int g1_status(const uint8_t* p) {
  const bn254::Fq x = fq_at(p), y = fq_at(p + 32);
  if (!bn254::is_canonical(x) || !bn254::is_canonical(y)) return 1;
  if (x.is_zero() && y.is_zero()) return 3;
  return bn254::sqr(y) == bn254::g1_curve_rhs(x) ? 0 : 2;
}
// amdzk_g2_prepare's checks
inline int g2_status(const uint8_t* p) {
  uint64_t w[16];
  memcpy(w, p, G2_BYTES);
  const pairing::G2Affine q = pairing::g2_from_words(w);
  if (!bn254::is_canonical(q.x.c0) || !bn254::is_canonical(q.x.c1) || !bn254::is_canonical(q.y.c0) || !bn254::is_canonical(q.y.c1)) return 1;
  if (q.is_inf()) return 3;
  return pairing::g2_on_twist(q) ? 0 : 2;
}
}  // namespace detail

// Everything amdzk_vk_read checks. On success *d owns the circuit's arrays and *lay says where the sections are.
inline int parse(const uint8_t* data, size_t len, pkblob::Desc* d, Layout* lay, std::string* err) {
  using detail::as_vk;
  using detail::fail;
  if (!data) return fail(err, "null data");
  if (len < MAGIC_BYTES + 4 + DIGEST_BYTES) return fail(err, "%llu bytes are too few for a verifying-key file", len);
  if (memcmp(data, magic(), MAGIC_BYTES) != 0) return fail(err, "bad magic: not a verifying-key file");
  pkblob::detail::Reader r{data, len, MAGIC_BYTES};
  uint32_t version = 0;
  r.u32(&version);
  if (version != FORMAT_VERSION) return fail(err, "format version %llu, this library reads version %llu", version, FORMAT_VERSION);
  if (int rc = as_vk(pkblob::detail::read_circuit(r, d, err), err)) return rc;
  if (d->k < 1 || d->k > pkblob::MAX_K) return fail(err, "k = %llu out of range (1 .. 28)", d->k);
  if (d->num_fixed > pkblob::MAX_COLUMNS || d->num_perm_columns() > pkblob::MAX_COLUMNS) return fail(err, "more than 65536 columns of one kind");
  // at most 2^17 commitments of 64 bytes behind the header: no sum below can wrap
  Layout L = layout(*d, false);
  if (r.pos != L.transcript_repr) return fail(err, "internal: the header's length is %llu, its writer's %llu", r.pos, L.transcript_repr);
  if ((uint64_t)len < (uint64_t)L.has_g2 + 1 + DIGEST_BYTES)
    return fail(err, "length mismatch: the header implies at least %llu bytes, %llu given", L.total, len);
  const uint8_t has_g2 = data[L.has_g2];
  if (has_g2 > 1) return fail(err, "has-g2 byte is %llu", has_g2);
  L = layout(*d, has_g2 == 1);
  if ((uint64_t)L.total != (uint64_t)len) return fail(err, "length mismatch: the header implies %llu bytes, %llu given", L.total, len);
  uint8_t dg[DIGEST_BYTES];
  digest(data, L.digest, dg);
  if (memcmp(dg, data + L.digest, DIGEST_BYTES) != 0) return fail(err, "digest mismatch: the file is damaged");
  if (int rc = as_vk(pkblob::validate(*d, err), err)) return rc;
  for (size_t i = 0; i < d->columns(); i++) {
    const int st = detail::g1_status(data + L.fixed_commitments + i * G1_BYTES);
    if (st == 1) return fail(err, "commitment %llu has a coordinate that is not below the modulus", i);
    if (st == 2) return fail(err, "commitment %llu is not on the curve", i);
  }
  switch (detail::g1_status(data + L.g)) {
    case 1: return fail(err, "G has a coordinate that is not below the modulus");
    case 2: return fail(err, "G is not on the curve");
    case 3: return fail(err, "G is the identity");
  }
  for (int i = 0; has_g2 && i < 2; i++) {
    const int st = detail::g2_status(data + (i ? L.s_g2 : L.g2));
    const char* which = i ? "s_g2" : "g2";
    if (st == 1) return fail(err, (std::string(which) + " has a coordinate that is not below the modulus").c_str());
    if (st == 2) return fail(err, (std::string(which) + " is not on the twist").c_str());
    if (st == 3) return fail(err, (std::string(which) + " is the identity").c_str());
  }
  if (lay) *lay = L;
  return AMDZK_OK;
}

}  // namespace vkblob
