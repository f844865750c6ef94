// The proving-key file (amdzk_pk_write / amdzk_pk_read / amdzk_pk_blob_info, include/amdzk.h): layout,
// writer of the header, and the parser with every check that needs no device. Host-only: no HIP include, compiles with
// g++ (tests/native/pk_blob_check.cpp runs it under ASan + UBSan).
//
// All integers little-endian, no padding, in this order:
//   magic "AMDZKPK\0" (8) | format version u32 = 1
//   amdzk_circuit in declaration order, as the caller of keygen passed it:
//     k, num_fixed, num_advice, num_instance, blinding_factors, cs_degree                       6 x u32
//     num_advice_queries u32   | advice_queries   2 x num x i32      (the same for fixed_queries, instance_queries)
//     num_gates, num_lookups, num_exprs                                                         3 x u32
//     lookup_shape 2 x num_lookups x u32 | expr_offsets (num_exprs + 1) x u32 | expr_words expr_offsets[num_exprs] x u32
//     num_constants u32 | constants num x 4 x u64 | num_perm_columns u32 | perm_columns 2 x num x u32
//   has_phases u8 (0 / 1); if 1: num_challenges u32 | advice_phase num_advice x u8 | challenge_phase num_challenges x u8
//   transcript_repr 4 x u64
//   fixed commitments num_fixed x 64 B | permutation commitments num_perm_columns x 64 B      (amdzk_pk_commitments)
//   fixed columns num_fixed x 2^k x 32 B | sigma columns num_perm_columns x 2^k x 32 B         (Lagrange, Montgomery)
//   BLAKE2b-512 of every byte before it, personalisation "amdzk_pk_blob_v1"                     64 B
// Every count is checked against the bytes that are left before anything is sized by it, so a parse allocates at most
// the header's own size; the columns are never copied on the host. The file is self-delimiting: its length must be
// exactly what the header implies. Hosts are little-endian (as the whole C ABI assumes for Fr limbs).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "hostcrypto.hpp"

namespace pkblob {

constexpr size_t MAGIC_BYTES = 8, DIGEST_BYTES = 64;
inline const char* magic() { return "AMDZKPK"; }  // 7 characters and the terminating NUL: 8 bytes
constexpr uint32_t FORMAT_VERSION = 1;
constexpr uint32_t MAX_K = 28;             // Fr's two-adicity: no larger domain exists
constexpr uint32_t MAX_COLUMNS = 1u << 16;  // an expression word addresses a column with 16 bits

inline void digest(const uint8_t* data, size_t len, uint8_t out[DIGEST_BYTES]) {
  zkhost::Blake2b h("amdzk_pk_blob_v1");
  h.update(data, len);
  h.digest(out);
}

// What keygen took, owned: the flattened amdzk_circuit arrays and the phase table.
struct Desc {
  uint32_t k = 0, num_fixed = 0, num_advice = 0, num_instance = 0, blinding_factors = 0, cs_degree = 0;
  std::vector<int32_t> advice_queries, fixed_queries, instance_queries;  // (column, rotation) pairs
  uint32_t num_gates = 0, num_lookups = 0, num_exprs = 0;
  std::vector<uint32_t> lookup_shape, expr_offsets, expr_words;
  std::vector<uint64_t> constants;     // 4 words each
  std::vector<uint32_t> perm_columns;  // (kind, index) pairs
  bool has_phases = false;
  uint32_t num_challenges = 0;
  std::vector<uint8_t> advice_phase, challenge_phase;

  uint32_t num_perm_columns() const { return (uint32_t)(perm_columns.size() / 2); }

  void assign(const amdzk_circuit& c, const amdzk_phases* ph) {
    k = c.k, num_fixed = c.num_fixed, num_advice = c.num_advice, num_instance = c.num_instance;
    blinding_factors = c.blinding_factors, cs_degree = c.cs_degree;
    auto take = [](auto& v, const auto* p, size_t n) {
      v.clear();
      if (p && n) v.assign(p, p + n);
    };
    take(advice_queries, c.advice_queries, 2 * (size_t)c.num_advice_queries);
    take(fixed_queries, c.fixed_queries, 2 * (size_t)c.num_fixed_queries);
    take(instance_queries, c.instance_queries, 2 * (size_t)c.num_instance_queries);
    num_gates = c.num_gates, num_lookups = c.num_lookups, num_exprs = c.num_exprs;
    take(lookup_shape, c.lookup_shape, 2 * (size_t)c.num_lookups);
    expr_offsets.assign((size_t)c.num_exprs + 1, 0);
    if (c.expr_offsets) expr_offsets.assign(c.expr_offsets, c.expr_offsets + (size_t)c.num_exprs + 1);
    take(expr_words, c.expr_words, expr_offsets.back());
    take(constants, c.constants, 4 * (size_t)c.num_constants);
    take(perm_columns, c.perm_columns, 2 * (size_t)c.num_perm_columns);
    has_phases = ph != nullptr;
    num_challenges = ph ? ph->num_challenges : 0;
    advice_phase.clear(), challenge_phase.clear();
    if (ph) {
      take(advice_phase, ph->advice_phase, c.num_advice);
      take(challenge_phase, ph->challenge_phase, ph->num_challenges);
    }
  }
  // amdzk_circuit / amdzk_phases over this object's arrays (valid while it lives and is not modified)
  void view(amdzk_circuit* c, amdzk_phases* ph) const {
    memset(c, 0, sizeof(*c));
    c->k = k, c->num_fixed = num_fixed, c->num_advice = num_advice, c->num_instance = num_instance;
    c->blinding_factors = blinding_factors, c->cs_degree = cs_degree;
    c->num_advice_queries = (uint32_t)(advice_queries.size() / 2), c->advice_queries = advice_queries.data();
    c->num_fixed_queries = (uint32_t)(fixed_queries.size() / 2), c->fixed_queries = fixed_queries.data();
    c->num_instance_queries = (uint32_t)(instance_queries.size() / 2), c->instance_queries = instance_queries.data();
    c->num_gates = num_gates, c->num_lookups = num_lookups, c->num_exprs = num_exprs;
    c->lookup_shape = lookup_shape.data(), c->expr_offsets = expr_offsets.data(), c->expr_words = expr_words.data();
    c->num_constants = (uint32_t)(constants.size() / 4), c->constants = constants.data();
    c->num_perm_columns = num_perm_columns(), c->perm_columns = perm_columns.data();
    ph->num_challenges = num_challenges, ph->advice_phase = advice_phase.data(), ph->challenge_phase = challenge_phase.data();
  }
  // amdzk_circuit .. phase table: the sections the verifying-key file (vkblob.hpp) shares with this one, byte for byte
  size_t circuit_bytes() const {
    size_t b = 6 * 4;
    b += 3 * 4 + 4 * (advice_queries.size() + fixed_queries.size() + instance_queries.size());
    b += 3 * 4 + 4 * (lookup_shape.size() + expr_offsets.size() + expr_words.size());
    b += 4 + 8 * constants.size() + 4 + 4 * perm_columns.size();
    b += 1 + (has_phases ? 4 + advice_phase.size() + challenge_phase.size() : 0);
    return b;
  }
  size_t header_bytes() const { return MAGIC_BYTES + 4 + circuit_bytes(); }  // magic .. phase table
  size_t columns() const { return (size_t)num_fixed + num_perm_columns(); }
  // bytes of the whole file, for a description that passed validate(): at most 2^17 columns of 2^28 rows, below 2^51
  size_t serialized_size() const { return header_bytes() + 32 + columns() * 64 + (columns() << k) * 32 + DIGEST_BYTES; }
  // writes header_bytes() bytes
  void write_header(uint8_t* out) const {
    memcpy(out, magic(), MAGIC_BYTES);
    const uint32_t version = FORMAT_VERSION;
    memcpy(out + MAGIC_BYTES, &version, 4);
    write_circuit(out + MAGIC_BYTES + 4);
  }
  // writes circuit_bytes() bytes
  void write_circuit(uint8_t* out) const {
    uint8_t* p = out;
    auto put = [&](const void* s, size_t n) {
      if (n) memcpy(p, s, n);
      p += n;
    };
    auto u32 = [&](uint32_t v) { put(&v, 4); };
    auto arr = [&](const auto& v) { put(v.data(), v.size() * sizeof(v[0])); };
    u32(k), u32(num_fixed), u32(num_advice), u32(num_instance), u32(blinding_factors), u32(cs_degree);
    u32((uint32_t)(advice_queries.size() / 2)), arr(advice_queries);
    u32((uint32_t)(fixed_queries.size() / 2)), arr(fixed_queries);
    u32((uint32_t)(instance_queries.size() / 2)), arr(instance_queries);
    u32(num_gates), u32(num_lookups), u32(num_exprs);
    arr(lookup_shape), arr(expr_offsets), arr(expr_words);
    u32((uint32_t)(constants.size() / 4)), arr(constants);
    u32(num_perm_columns()), arr(perm_columns);
    const uint8_t hp = has_phases ? 1 : 0;
    put(&hp, 1);
    if (has_phases) u32(num_challenges), arr(advice_phase), arr(challenge_phase);
  }
};

// Byte offsets of the sections behind the header.
struct Layout {
  size_t transcript_repr = 0, fixed_commitments = 0, perm_commitments = 0, fixed_values = 0, sigma_values = 0, digest = 0, total = 0;
};

namespace detail {
struct Reader {
  const uint8_t* p;
  size_t len, pos;
  size_t left() const { return len - pos; }
  bool u32(uint32_t* v) {
    if (left() < 4) return false;
    memcpy(v, p + pos, 4);
    pos += 4;
    return true;
  }
  // `count` elements: refused unless the bytes that are left hold them (the division cannot overflow)
  template <class T>
  bool arr(std::vector<T>& out, uint64_t count) {
    if (count > left() / sizeof(T)) return false;
    out.resize((size_t)count);
    if (count) memcpy(out.data(), p + pos, (size_t)count * sizeof(T));
    pos += (size_t)count * sizeof(T);
    return true;
  }
};
inline int fail(std::string* err, const char* fmt, unsigned long long a = 0, unsigned long long b = 0) {
  if (err) {
    char buf[256];
    snprintf(buf, sizeof(buf), fmt, a, b);
    *err = std::string("pk_read: ") + buf;
  }
  return AMDZK_E_INVALID;
}
// amdzk_circuit .. phase table at r.pos into *d (the sections Desc::write_circuit writes): every count is checked against the
// bytes that are left before anything is sized by it. Shared with the verifying-key file's parser (vkblob.hpp).
inline int read_circuit(Reader& r, Desc* d, std::string* err) {
  const size_t len = r.len;
  uint32_t cnt = 0;
#define PKB_GET(x) \
  if (!(x)) return fail(err, "truncated: the header runs past the %llu bytes given", len)
  PKB_GET(r.u32(&d->k) && r.u32(&d->num_fixed) && r.u32(&d->num_advice) && r.u32(&d->num_instance) && r.u32(&d->blinding_factors) &&
          r.u32(&d->cs_degree));
  PKB_GET(r.u32(&cnt) && r.arr(d->advice_queries, 2 * (uint64_t)cnt));
  PKB_GET(r.u32(&cnt) && r.arr(d->fixed_queries, 2 * (uint64_t)cnt));
  PKB_GET(r.u32(&cnt) && r.arr(d->instance_queries, 2 * (uint64_t)cnt));
  PKB_GET(r.u32(&d->num_gates) && r.u32(&d->num_lookups) && r.u32(&d->num_exprs));
  PKB_GET(r.arr(d->lookup_shape, 2 * (uint64_t)d->num_lookups));
  PKB_GET(r.arr(d->expr_offsets, (uint64_t)d->num_exprs + 1));
  PKB_GET(r.arr(d->expr_words, d->expr_offsets.back()));
  PKB_GET(r.u32(&cnt) && r.arr(d->constants, 4 * (uint64_t)cnt));
  PKB_GET(r.u32(&cnt) && r.arr(d->perm_columns, 2 * (uint64_t)cnt));
  std::vector<uint8_t> hp;
  PKB_GET(r.arr(hp, 1));
  if (hp[0] > 1) return fail(err, "has-phases byte is %llu", hp[0]);
  d->has_phases = hp[0] == 1;
  d->num_challenges = 0;
  d->advice_phase.clear(), d->challenge_phase.clear();
  if (d->has_phases) PKB_GET(r.u32(&d->num_challenges) && r.arr(d->advice_phase, d->num_advice) && r.arr(d->challenge_phase, d->num_challenges));
#undef PKB_GET
  return AMDZK_OK;
}
}  // namespace detail

// The checks keygen makes on a circuit and its phase table (and the index checks its expression compiler makes), plus the
// bounds that keep every later index inside its array. No allocation beyond a small stack of depths.
inline int validate(const Desc& d, std::string* err) {
  using detail::fail;
  if (d.k < 1 || d.k > MAX_K) return fail(err, "k = %llu out of range (1 .. 28)", d.k);
  const uint64_t n = (uint64_t)1 << d.k;
  if (d.num_fixed > MAX_COLUMNS || d.num_advice > MAX_COLUMNS || d.num_instance > MAX_COLUMNS || d.num_perm_columns() > MAX_COLUMNS)
    return fail(err, "more than 65536 columns of one kind");
  if (d.cs_degree < 3) return fail(err, "cs_degree %llu < 3", d.cs_degree);
  if (((uint64_t)(d.cs_degree - 1) << d.k) > ((uint64_t)1 << MAX_K))  // extended_k = ceil(log2(n (cs_degree - 1)))
    return fail(err, "cs_degree %llu needs an extended domain above 2^28 at k = %llu", d.cs_degree, d.k);
  if (n < (uint64_t)d.blinding_factors + 3) return fail(err, "not enough rows (n = %llu, blinding factors = %llu)", n, d.blinding_factors);
  const std::vector<int32_t>* qs[3] = {&d.advice_queries, &d.fixed_queries, &d.instance_queries};
  const uint32_t qlim[3] = {d.num_advice, d.num_fixed, d.num_instance};
  for (int t = 0; t < 3; t++)
    for (size_t i = 0; i < qs[t]->size(); i += 2) {
      const int32_t col = (*qs[t])[i], rot = (*qs[t])[i + 1];
      if (col < 0 || (uint32_t)col >= qlim[t]) return fail(err, "query %llu names a column out of range", i / 2);
      if (rot < -128 || rot > 127) return fail(err, "query %llu has a rotation out of range", i / 2);
    }
  uint64_t nexpr = d.num_gates;
  for (size_t l = 0; l < d.lookup_shape.size(); l++) nexpr += d.lookup_shape[l];
  if (nexpr != d.num_exprs) return fail(err, "expression count mismatch (%llu vs %llu)", nexpr, d.num_exprs);
  if (d.expr_offsets.size() != (size_t)d.num_exprs + 1 || d.expr_offsets[0] != 0) return fail(err, "expression offsets do not start at 0");
  for (size_t e = 0; e < d.num_exprs; e++)
    if (d.expr_offsets[e + 1] < d.expr_offsets[e]) return fail(err, "expression offsets decrease at expression %llu", e);
  if (d.expr_offsets.back() != d.expr_words.size()) return fail(err, "expression offsets and words disagree");
  for (size_t i = 0; i < d.perm_columns.size(); i += 2) {
    const uint32_t kind = d.perm_columns[i], idx = d.perm_columns[i + 1];
    if (kind > 2 || idx >= (kind == 0 ? d.num_advice : kind == 1 ? d.num_fixed : d.num_instance))
      return fail(err, "permutation column %llu out of range", i / 2);
  }
  if (d.has_phases) {
    if (d.advice_phase.size() != d.num_advice || d.challenge_phase.size() != d.num_challenges) return fail(err, "phase table size mismatch");
    bool has[3] = {false, false, false};
    for (size_t a = 0; a < d.advice_phase.size(); a++) {
      if (d.advice_phase[a] > 2) return fail(err, "advice column %llu is in phase %llu (phases are 0, 1, 2)", a, d.advice_phase[a]);
      has[d.advice_phase[a]] = true;
    }
    for (int p = 1; p < 3; p++)
      if (has[p] && !has[p - 1]) return fail(err, "phase %llu has advice columns but phase %llu has none", p, p - 1);
    for (size_t i = 0; i < d.challenge_phase.size(); i++)
      if (d.challenge_phase[i] > 2 || !has[d.challenge_phase[i]])
        return fail(err, "challenge %llu is usable after phase %llu, which has no advice column", i, d.challenge_phase[i]);
  }
  const uint32_t nconst = (uint32_t)(d.constants.size() / 4);
  for (size_t e = 0; e < d.num_exprs; e++) {
    uint64_t depth = 0;
    for (size_t i = d.expr_offsets[e]; i < d.expr_offsets[e + 1]; i++) {
      const uint32_t w = d.expr_words[i], op = w >> 24, pl = w & 0xffffffu;
      bool ok = true;
      switch (op) {
        case 1: ok = pl < nconst, depth++; break;
        case 2: ok = (pl >> 8) < d.num_fixed, depth++; break;
        case 3: ok = (pl >> 8) < d.num_advice, depth++; break;
        case 4: ok = (pl >> 8) < d.num_instance, depth++; break;
        case 9: ok = d.has_phases && pl < d.num_challenges, depth++; break;
        case 5: ok = depth >= 1; break;
        case 8: ok = depth >= 1 && pl < nconst; break;
        case 6: case 7: ok = depth >= 2, depth--; break;
        default: ok = false;
      }
      if (!ok) return fail(err, "bad expression word %08llx in expression %llu", w, e);
    }
    if (depth != 1) return fail(err, "malformed expression %llu", e);
  }
  return AMDZK_OK;
}

// Everything amdzk_pk_read checks before it touches the device. On success *d owns the header's arrays and *lay says
// where the sections are; `data` is not referenced afterwards.
inline int parse(const uint8_t* data, size_t len, Desc* d, Layout* lay, std::string* err) {
  using detail::fail;
  if (!data) return fail(err, "null data");
  detail::Reader r{data, len, 0};
  if (len < MAGIC_BYTES + 4 + DIGEST_BYTES) return fail(err, "%llu bytes are too few for a key file", len);
  if (memcmp(data, magic(), MAGIC_BYTES) != 0) return fail(err, "bad magic: not a proving-key file");
  r.pos = MAGIC_BYTES;
  uint32_t version = 0;
  r.u32(&version);
  if (version != FORMAT_VERSION) return fail(err, "format version %llu, this library reads version %llu", version, FORMAT_VERSION);
  if (int rc = detail::read_circuit(r, d, err)) return rc;
  if (d->k < 1 || d->k > MAX_K) return fail(err, "k = %llu out of range (1 .. 28)", d->k);
  // sections behind the header: with both counts bounded, F + S <= 2^17 columns of 2^k <= 2^28 rows of 32 bytes are at
  // most 2^50 bytes, so `want` cannot wrap (unbounded, 2^33 columns would reach 2^66)
  if (d->num_fixed > MAX_COLUMNS || d->num_perm_columns() > MAX_COLUMNS) return fail(err, "more than 65536 columns of one kind");
  const uint64_t cols = (uint64_t)d->num_fixed + d->num_perm_columns();
  const uint64_t want = (uint64_t)r.pos + 32 + cols * 64 + (cols << d->k) * 32 + DIGEST_BYTES;
  if (want != (uint64_t)len) return fail(err, "length mismatch: the header implies %llu bytes, %llu given", want, len);
  Layout L;
  L.transcript_repr = r.pos;
  L.fixed_commitments = L.transcript_repr + 32;
  L.perm_commitments = L.fixed_commitments + (size_t)d->num_fixed * 64;
  L.fixed_values = L.perm_commitments + (size_t)d->num_perm_columns() * 64;
  L.sigma_values = L.fixed_values + ((size_t)d->num_fixed << d->k) * 32;
  L.digest = len - DIGEST_BYTES;
  L.total = len;
  uint8_t dg[DIGEST_BYTES];
  digest(data, L.digest, dg);
  if (memcmp(dg, data + L.digest, DIGEST_BYTES) != 0) return fail(err, "digest mismatch: the file is damaged");
  if (int rc = validate(*d, err)) return rc;
  if (lay) *lay = L;
  return AMDZK_OK;
}

}  // namespace pkblob
