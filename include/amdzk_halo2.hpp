// amdzk_halo2.hpp — host-side mirror, in C++, of the halo2_proofs interface the reference's circuits are
// written against and its prover is called through (halo2_proofs 0.2.0 @ v2023_01_20 [UP],
// /root/reference/Cargo.lock:469-471):
//
//   plonk::{Column, Expression, VirtualCells, ConstraintSystem}   <- Circuit::configure(meta)
//        /root/reference/src/lib.rs:295-326, src/signal.rs:27-49, src/conditional_secrets.rs:81-187,
//        src/timestamp.rs:58-138
//   plonk::permutation::keygen::Assembly                           <- region.constrain_equal / copy_advice
//   poly::kzg::commitment::ParamsKZG {setup, read, write, downsize, commit, commit_lagrange, get_g}
//   plonk::{keygen_pk -> ProvingKey, create_proof}
//   plonk::{Challenge, ConstraintSystem::advice_column_in / challenge_usable_after, Expression::Challenge} and
//   transcript::TranscriptWrite — challenge phases and a caller-owned transcript (amdzk_keygen_phased,
//   amdzk_create_proof_opts); create_proof_batch: many independent proofs in lock-step (amdzk_create_proof_batch; with
//   per-proof transcripts, a batch synthesize and different circuits: amdzk_create_proof_batch_opts)
//
// Header-only over the C ABI of include/amdzk.h (link libamdzk.so); the same names, argument meaning and
// derived quantities (query order, degree(), blinding_factors()) as upstream. Everything O(n) runs on
// the MI355X; this file only describes circuits and moves bytes. The Python package
// (anon-aadhaar-halo2_amd/halo2/*.py) is the same mirror for the test-suite;
// tests/test_cpp_mirror.py checks that both flatten a circuit to identical C-ABI arrays and that a
// proof made through this header equals the oracle prover's bytes.
#ifndef AMDZK_HALO2_HPP
#define AMDZK_HALO2_HPP

#include <array>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <map>
#include <random>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "amdzk.h"

namespace amdzk {
namespace halo2 {

// ------------------------------------------------------------------------------------------ errors
struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

class Context {
 public:
  explicit Context(int device = 0) {
    int rc = amdzk_init(device, &h_);
    if (rc != AMDZK_OK) throw Error(rc, "amdzk_init failed");
  }
  ~Context() {
    if (h_) amdzk_destroy(h_);
  }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  amdzk_ctx* get() const { return h_; }
  void check(int rc) const {
    if (rc != AMDZK_OK) throw Error(rc, amdzk_last_error(h_));
  }
  // amdzk_set_host_wait: true = this context's calls POLL a completion event while they wait for the device (20 us of
  // yielding, then 50-us sleeps: every wait ends up to ~50 us late, 8-10 waits per proof; for hosts with more proofs in
  // flight than cores to spare), false = they spin in hipStreamSynchronize (the default: lowest latency)
  void set_blocking_waits(bool block) const { check(amdzk_set_host_wait(h_, block ? AMDZK_WAIT_BLOCK : AMDZK_WAIT_SPIN)); }

 private:
  amdzk_ctx* h_ = nullptr;
};

// ------------------------------------------------------------------------------------------ Fr
// halo2curves::bn256::Fr: 4 x u64 little-endian limbs, Montgomery form with R = 2^256. Host arithmetic is
// only used for circuit constants and test witnesses.
struct Fr {
  uint64_t l[4];

  static constexpr uint64_t MOD[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};
  static constexpr uint64_t INV = 0xc2e1f593efffffffULL;  // -r^-1 mod 2^64
  static constexpr uint64_t R2[4] = {0x1bb8e645ae216da7ULL, 0x53fe3ab1e35c59e3ULL, 0x8c49833d53bb8085ULL, 0x0216d0b17f4e44a5ULL};

  static Fr zero() { return Fr{{0, 0, 0, 0}}; }
  static Fr one() { return from_u64(1); }
  // Fr::from_raw: canonical little-endian limbs (< r) -> Montgomery.
  static Fr from_raw(const uint64_t v[4]) {
    Fr a{{v[0], v[1], v[2], v[3]}}, r2{{R2[0], R2[1], R2[2], R2[3]}};
    return mont_mul(a, r2);
  }
  static Fr from_u64(uint64_t v) {
    uint64_t raw[4] = {v, 0, 0, 0};
    return from_raw(raw);
  }
  // Big-endian hex digits of the canonical value (no 0x prefix), as halo2's Debug prints them.
  static Fr from_hex(const std::string& hex) {
    uint64_t raw[4] = {0, 0, 0, 0};
    int bit = 0;
    for (size_t i = hex.size(); i-- > 0;) {
      char c = hex[i];
      uint64_t d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : 16;
      if (d > 15 || bit >= 256) throw Error(AMDZK_E_INVALID, "Fr::from_hex: bad digit or too long");
      raw[bit >> 6] |= d << (bit & 63);
      bit += 4;
    }
    return from_raw(raw);
  }
  // Fr::to_repr: canonical limbs.
  void to_repr(uint64_t out[4]) const {
    Fr o{{1, 0, 0, 0}};
    Fr c = mont_mul(*this, o);
    std::memcpy(out, c.l, 32);
  }
  bool is_zero() const { return (l[0] | l[1] | l[2] | l[3]) == 0; }
  bool operator==(const Fr& o) const { return std::memcmp(l, o.l, 32) == 0; }
  bool operator<(const Fr& o) const {  // ordering for std::map keys only
    for (int i = 3; i >= 0; i--)
      if (l[i] != o.l[i]) return l[i] < o.l[i];
    return false;
  }
  Fr operator+(const Fr& o) const {
    Fr r;
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; i++) {
      c += (unsigned __int128)l[i] + o.l[i];
      r.l[i] = (uint64_t)c;
      c >>= 64;
    }
    return (c || geq_mod(r)) ? sub_mod(r) : r;
  }
  Fr operator-() const {
    if (is_zero()) return *this;
    Fr m{{MOD[0], MOD[1], MOD[2], MOD[3]}}, r;
    unsigned __int128 b = 0;
    for (int i = 0; i < 4; i++) {
      unsigned __int128 d = (unsigned __int128)m.l[i] - l[i] - (uint64_t)b;
      r.l[i] = (uint64_t)d;
      b = (d >> 64) & 1;
    }
    return r;
  }
  Fr operator-(const Fr& o) const { return *this + (-o); }
  Fr operator*(const Fr& o) const { return mont_mul(*this, o); }

 private:
  static bool geq_mod(const Fr& a) {
    for (int i = 3; i >= 0; i--)
      if (a.l[i] != MOD[i]) return a.l[i] > MOD[i];
    return true;
  }
  static Fr sub_mod(const Fr& a) {
    Fr r;
    unsigned __int128 b = 0;
    for (int i = 0; i < 4; i++) {
      unsigned __int128 d = (unsigned __int128)a.l[i] - MOD[i] - (uint64_t)b;
      r.l[i] = (uint64_t)d;
      b = (d >> 64) & 1;
    }
    return r;
  }
  static Fr mont_mul(const Fr& a, const Fr& b) {  // CIOS, 4 x 64
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
      unsigned __int128 c = 0;
      for (int j = 0; j < 4; j++) {
        c += (unsigned __int128)a.l[j] * b.l[i] + t[j];
        t[j] = (uint64_t)c;
        c >>= 64;
      }
      c += t[4];
      t[4] = (uint64_t)c;
      t[5] = (uint64_t)(c >> 64);
      uint64_t m = t[0] * INV;
      c = (unsigned __int128)m * MOD[0] + t[0];
      c >>= 64;
      for (int j = 1; j < 4; j++) {
        c += (unsigned __int128)m * MOD[j] + t[j];
        t[j - 1] = (uint64_t)c;
        c >>= 64;
      }
      c += t[4];
      t[3] = (uint64_t)c;
      t[4] = t[5] + (uint64_t)(c >> 64);
    }
    Fr r{{t[0], t[1], t[2], t[3]}};
    return (t[4] || geq_mod(r)) ? sub_mod(r) : r;
  }
};

// ------------------------------------------------------------------------------------------ columns
enum class Any : uint32_t { Advice = 0, Fixed = 1, Instance = 2 };  // upstream's ordering of `Any`

struct Column {
  Any kind;
  uint32_t index;
  bool operator==(const Column& o) const { return kind == o.kind && index == o.index; }
};
struct Rotation {
  int32_t v;
  static Rotation cur() { return {0}; }
  static Rotation next() { return {1}; }
  static Rotation prev() { return {-1}; }
};

// ------------------------------------------------------------------------------------------ Expression
// plonk::Challenge: squeezed once the advice columns of `phase` (and of the phases before it) are committed.
struct Challenge {
  uint32_t index;
  uint8_t phase;
};

// plonk::Expression: Constant | Fixed | Advice | Instance | Challenge | Negated | Sum | Product | Scaled.
class Expression {
 public:
  enum Op : uint32_t { Constant = 1, Fixed = 2, Advice = 3, Instance = 4, Negated = 5, Sum = 6, Product = 7, Scaled = 8, ChallengeOp = 9 };
  struct Node {
    Op op;
    Fr c;               // Constant / Scaled
    uint32_t column;    // queries; the index of a challenge
    int32_t rotation;
    std::shared_ptr<const Node> a, b;
  };

  Expression() = default;
  static Expression constant(const Fr& v) { return Expression(mk(Constant, v, 0, 0, nullptr, nullptr)); }
  static Expression query(Any kind, uint32_t column, int32_t rot) {
    Op op = kind == Any::Advice ? Advice : kind == Any::Fixed ? Fixed : Instance;
    return Expression(mk(op, Fr::zero(), column, rot, nullptr, nullptr));
  }
  static Expression challenge(Challenge ch) { return Expression(mk(ChallengeOp, Fr::zero(), ch.index, 0, nullptr, nullptr)); }
  Expression operator-() const { return Expression(mk(Negated, Fr::zero(), 0, 0, n_, nullptr)); }
  Expression operator+(const Expression& o) const { return Expression(mk(Sum, Fr::zero(), 0, 0, n_, o.n_)); }
  Expression operator-(const Expression& o) const { return *this + (-o); }  // upstream: Sum(a, Negated(b))
  Expression operator*(const Expression& o) const { return Expression(mk(Product, Fr::zero(), 0, 0, n_, o.n_)); }
  Expression operator*(const Fr& s) const { return Expression(mk(Scaled, s, 0, 0, n_, nullptr)); }

  uint32_t degree() const { return degree(n_.get()); }
  const Node* node() const { return n_.get(); }

 private:
  explicit Expression(std::shared_ptr<const Node> n) : n_(std::move(n)) {}
  static std::shared_ptr<const Node> mk(Op op, const Fr& c, uint32_t col, int32_t rot, std::shared_ptr<const Node> a,
                                        std::shared_ptr<const Node> b) {
    auto n = std::make_shared<Node>();
    n->op = op;
    n->c = c;
    n->column = col;
    n->rotation = rot;
    n->a = std::move(a);
    n->b = std::move(b);
    return n;
  }
  static uint32_t degree(const Node* n) {
    switch (n->op) {
      case Constant: case ChallengeOp: return 0;
      case Fixed: case Advice: case Instance: return 1;
      case Negated: case Scaled: return degree(n->a.get());
      case Sum: return std::max(degree(n->a.get()), degree(n->b.get()));
      case Product: return degree(n->a.get()) + degree(n->b.get());
    }
    return 0;
  }
  std::shared_ptr<const Node> n_;
};

class ConstraintSystem;

// What the closures of create_gate / lookup receive (`meta.query_advice(col, Rotation::cur())`).
class VirtualCells {
 public:
  explicit VirtualCells(ConstraintSystem& cs) : cs_(cs) {}
  Expression query_advice(Column c, Rotation r);
  Expression query_fixed(Column c, Rotation r = Rotation::cur());
  Expression query_instance(Column c, Rotation r);
  Expression query_selector(Column s) { return query_fixed(s, Rotation::cur()); }

 private:
  ConstraintSystem& cs_;
};

// plonk::ConstraintSystem as it stands after Circuit::configure and selector compression (selectors
// are fixed columns here, one each).
class ConstraintSystem {
 public:
  using Query = std::pair<Column, int32_t>;
  struct Lookup {
    std::vector<Expression> inputs, tables;
  };

  uint32_t num_fixed = 0, num_advice = 0, num_instance = 0;
  std::vector<Query> advice_queries, fixed_queries, instance_queries;  // first-use order
  std::vector<uint32_t> num_advice_queries;                            // per advice column
  std::vector<Expression> gates;                                       // one entry per polynomial, in order
  std::vector<Lookup> lookups;
  std::vector<Column> permutation_columns;
  uint32_t minimum_degree = 0;
  std::vector<uint8_t> advice_column_phase, challenge_phase;  // per advice column / per challenge

  Column advice_column() { return advice_column_in(0); }
  // ConstraintSystem::advice_column_in: phases are 0, 1, 2; a phase above 0 needs a column in the phase before it.
  Column advice_column_in(uint32_t phase) {
    if (phase > 2) throw Error(AMDZK_E_INVALID, "advice_column_in: phase " + std::to_string(phase) + " (phases are 0, 1, 2)");
    if (phase > 0 && !phase_has_advice(phase - 1))
      throw Error(AMDZK_E_INVALID, "advice_column_in: no advice column in phase " + std::to_string(phase - 1) + ", the one before phase " +
                                       std::to_string(phase));
    num_advice_queries.push_back(0);
    advice_column_phase.push_back((uint8_t)phase);
    return {Any::Advice, num_advice++};
  }
  // ConstraintSystem::challenge_usable_after: the phase must already have an advice column.
  Challenge challenge_usable_after(uint32_t phase) {
    if (phase > 2 || !phase_has_advice(phase)) throw Error(AMDZK_E_INVALID, "challenge_usable_after: no advice column in phase " + std::to_string(phase));
    challenge_phase.push_back((uint8_t)phase);
    return {(uint32_t)challenge_phase.size() - 1, (uint8_t)phase};
  }
  bool phase_has_advice(uint32_t phase) const {
    for (uint8_t p : advice_column_phase)
      if (p == phase) return true;
    return false;
  }
  // later phases or challenges: the key goes through amdzk_keygen_phased, the proof needs a synthesize callback
  bool phased() const {
    for (uint8_t p : advice_column_phase)
      if (p) return true;
    return !challenge_phase.empty();
  }
  Column fixed_column() { return {Any::Fixed, num_fixed++}; }
  Column selector() { return fixed_column(); }
  Column instance_column() { return {Any::Instance, num_instance++}; }

  // ConstraintSystem::enable_equality: query at Rotation::cur() and add to the permutation argument.
  void enable_equality(Column c) {
    VirtualCells m(*this);
    if (c.kind == Any::Advice) m.query_advice(c, Rotation::cur());
    else if (c.kind == Any::Fixed) m.query_fixed(c, Rotation::cur());
    else m.query_instance(c, Rotation::cur());
    for (const Column& p : permutation_columns)
      if (p == c) return;
    permutation_columns.push_back(c);
  }
  void create_gate(const char* /*name*/, const std::function<std::vector<Expression>(VirtualCells&)>& f) {
    VirtualCells m(*this);
    std::vector<Expression> polys = f(m);
    if (polys.empty()) throw Error(AMDZK_E_INVALID, "create_gate: gates must contain at least one constraint");
    for (auto& p : polys) gates.push_back(p);
  }
  size_t lookup(const char* /*name*/, const std::function<std::vector<std::pair<Expression, Expression>>(VirtualCells&)>& f) {
    VirtualCells m(*this);
    Lookup lk;
    for (auto& pr : f(m)) {
      lk.inputs.push_back(pr.first);
      lk.tables.push_back(pr.second);
    }
    lookups.push_back(std::move(lk));
    return lookups.size() - 1;
  }

  // Upstream formulas.
  uint32_t degree() const {
    uint32_t d = 3;  // permutation::Argument::required_degree()
    for (const Lookup& lk : lookups) {
      uint32_t di = 1, dt = 1;
      for (auto& e : lk.inputs) di = std::max(di, e.degree());
      for (auto& e : lk.tables) dt = std::max(dt, e.degree());
      d = std::max(d, std::max(4u, 2 + di + dt));
    }
    for (auto& g : gates) d = std::max(d, g.degree());
    return std::max(d, std::max(minimum_degree, 1u));
  }
  uint32_t blinding_factors() const {
    uint32_t f = num_advice_queries.empty() ? 1 : 0;
    for (uint32_t q : num_advice_queries) f = std::max(f, q);
    return std::max(3u, f) + 2;
  }
  uint32_t minimum_rows() const { return blinding_factors() + 3; }
  size_t permutation_index(Column c) const {
    for (size_t i = 0; i < permutation_columns.size(); i++)
      if (permutation_columns[i] == c) return i;
    throw Error(AMDZK_E_INVALID, "column is not equality-enabled");
  }

  bool note_query(std::vector<Query>& lst, Column c, int32_t rot) {
    for (auto& q : lst)
      if (q.first == c && q.second == rot) return false;
    lst.push_back({c, rot});
    return true;
  }
};

inline Expression VirtualCells::query_advice(Column c, Rotation r) {
  if (c.kind != Any::Advice) throw Error(AMDZK_E_INVALID, "query_advice: not an advice column");
  if (cs_.note_query(cs_.advice_queries, c, r.v)) cs_.num_advice_queries[c.index]++;
  return Expression::query(Any::Advice, c.index, r.v);
}
inline Expression VirtualCells::query_fixed(Column c, Rotation r) {
  if (c.kind != Any::Fixed) throw Error(AMDZK_E_INVALID, "query_fixed: not a fixed column");
  cs_.note_query(cs_.fixed_queries, c, r.v);
  return Expression::query(Any::Fixed, c.index, r.v);
}
inline Expression VirtualCells::query_instance(Column c, Rotation r) {
  if (c.kind != Any::Instance) throw Error(AMDZK_E_INVALID, "query_instance: not an instance column");
  cs_.note_query(cs_.instance_queries, c, r.v);
  return Expression::query(Any::Instance, c.index, r.v);
}

// ------------------------------------------------------------------------------------------ flattening
// The plain-data form of a ConstraintSystem that amdzk_keygen takes (include/amdzk.h: amdzk_circuit).
struct CircuitData {
  std::vector<int32_t> aq, fq, iq;
  std::vector<uint32_t> lookup_shape, expr_offsets, expr_words, perm_columns;
  std::vector<uint64_t> constants;  // 4 limbs each, Montgomery
  amdzk_circuit c;
  std::vector<uint8_t> advice_phase, challenge_phase;
  amdzk_phases phases;  // amdzk_keygen_phased's table (use it when `phased`)
  bool phased;

  CircuitData(const ConstraintSystem& cs, uint32_t k) : advice_phase(cs.advice_column_phase), challenge_phase(cs.challenge_phase), phased(cs.phased()) {
    phases.num_challenges = (uint32_t)challenge_phase.size();
    phases.advice_phase = advice_phase.data();
    phases.challenge_phase = challenge_phase.data();
    auto put = [](std::vector<int32_t>& dst, const std::vector<ConstraintSystem::Query>& qs) {
      for (auto& q : qs) {
        dst.push_back((int32_t)q.first.index);
        dst.push_back(q.second);
      }
    };
    put(aq, cs.advice_queries);
    put(fq, cs.fixed_queries);
    put(iq, cs.instance_queries);
    expr_offsets.push_back(0);
    auto add = [&](const Expression& e) {
      emit(e.node());
      expr_offsets.push_back((uint32_t)expr_words.size());
    };
    for (auto& g : cs.gates) add(g);
    for (auto& lk : cs.lookups) {
      lookup_shape.push_back((uint32_t)lk.inputs.size());
      lookup_shape.push_back((uint32_t)lk.tables.size());
      for (auto& e : lk.inputs) add(e);
      for (auto& e : lk.tables) add(e);
    }
    for (auto& p : cs.permutation_columns) {
      perm_columns.push_back((uint32_t)p.kind);
      perm_columns.push_back(p.index);
    }
    std::memset(&c, 0, sizeof(c));
    c.k = k;
    c.num_fixed = cs.num_fixed;
    c.num_advice = cs.num_advice;
    c.num_instance = cs.num_instance;
    c.blinding_factors = cs.blinding_factors();
    c.cs_degree = cs.degree();
    c.num_advice_queries = (uint32_t)cs.advice_queries.size();
    c.advice_queries = aq.data();
    c.num_fixed_queries = (uint32_t)cs.fixed_queries.size();
    c.fixed_queries = fq.data();
    c.num_instance_queries = (uint32_t)cs.instance_queries.size();
    c.instance_queries = iq.data();
    c.num_gates = (uint32_t)cs.gates.size();
    c.num_lookups = (uint32_t)cs.lookups.size();
    c.num_exprs = (uint32_t)expr_offsets.size() - 1;
    c.lookup_shape = lookup_shape.data();
    c.expr_offsets = expr_offsets.data();
    c.expr_words = expr_words.data();
    c.num_constants = (uint32_t)(constants.size() / 4);
    c.constants = constants.data();
    c.num_perm_columns = (uint32_t)cs.permutation_columns.size();
    c.perm_columns = perm_columns.data();
  }
  CircuitData(const CircuitData&) = delete;
  CircuitData& operator=(const CircuitData&) = delete;

 private:
  std::map<Fr, uint32_t> cidx_;
  uint32_t constant_index(const Fr& v) {
    auto it = cidx_.find(v);
    if (it != cidx_.end()) return it->second;
    uint32_t i = (uint32_t)cidx_.size();
    cidx_[v] = i;
    constants.insert(constants.end(), v.l, v.l + 4);
    return i;
  }
  void emit(const Expression::Node* n) {
    switch (n->op) {
      case Expression::Constant:
        expr_words.push_back((1u << 24) | constant_index(n->c));
        break;
      case Expression::Fixed: case Expression::Advice: case Expression::Instance:
        if (n->rotation < -128 || n->rotation > 127 || n->column >= (1u << 16)) throw Error(AMDZK_E_UNSUPPORTED, "query out of encodable range");
        expr_words.push_back(((uint32_t)n->op << 24) | (n->column << 8) | (uint32_t)(n->rotation + 128));
        break;
      case Expression::ChallengeOp:
        expr_words.push_back((9u << 24) | n->column);
        break;
      case Expression::Negated:
        emit(n->a.get());
        expr_words.push_back(5u << 24);
        break;
      case Expression::Sum: case Expression::Product:
        emit(n->a.get());
        emit(n->b.get());
        expr_words.push_back((uint32_t)n->op << 24);
        break;
      case Expression::Scaled:
        emit(n->a.get());
        expr_words.push_back((8u << 24) | constant_index(n->c));
        break;
    }
  }
};

// ------------------------------------------------------------------------------------------ Assembly
// plonk::permutation::keygen::Assembly: copy-constraint cycles over the permutation columns.
class Assembly {
 public:
  Assembly(size_t n, size_t ncols) : n_(n), ncols_(ncols), mapping_(2 * n * ncols), aux_(2 * n * ncols), sizes_(n * ncols, 1) {
    for (size_t c = 0; c < ncols; c++)
      for (size_t r = 0; r < n; r++) {
        size_t i = c * n + r;
        mapping_[2 * i] = aux_[2 * i] = (uint32_t)c;
        mapping_[2 * i + 1] = aux_[2 * i + 1] = (uint32_t)r;
      }
  }
  // Assembly::copy: merge the cycles of (left column, row) and (right column, row), union by size.
  void copy(size_t lc, size_t lr, size_t rc, size_t rr) {
    if (lc >= ncols_ || rc >= ncols_ || lr >= n_ || rr >= n_) throw Error(AMDZK_E_INVALID, "Assembly::copy: out of bounds");
    size_t l = lc * n_ + lr, r = rc * n_ + rr;
    size_t lcy = (size_t)aux_[2 * l] * n_ + aux_[2 * l + 1], rcy = (size_t)aux_[2 * r] * n_ + aux_[2 * r + 1];
    if (lcy == rcy) return;
    if (sizes_[lcy] < sizes_[rcy]) std::swap(lcy, rcy);
    sizes_[lcy] += sizes_[rcy];
    size_t i = rcy;
    do {
      aux_[2 * i] = (uint32_t)(lcy / n_);
      aux_[2 * i + 1] = (uint32_t)(lcy % n_);
      i = (size_t)mapping_[2 * i] * n_ + mapping_[2 * i + 1];
    } while (i != rcy);
    std::swap(mapping_[2 * l], mapping_[2 * r]);
    std::swap(mapping_[2 * l + 1], mapping_[2 * r + 1]);
  }
  const uint32_t* mapping() const { return mapping_.data(); }  // amdzk_keygen's perm_mapping layout
  size_t n() const { return n_; }
  size_t num_columns() const { return ncols_; }

 private:
  size_t n_, ncols_;
  std::vector<uint32_t> mapping_, aux_;
  std::vector<uint64_t> sizes_;
};

// ------------------------------------------------------------------------------------------ ParamsKZG
struct G1Affine {
  uint64_t x[4], y[4];  // Montgomery Fq; (0, 0) = identity
};
struct G1 {
  uint64_t x[4], y[4], z[4];  // Jacobian, z = 0 identity; results come back with z = 1
};

struct G2Affine;  // below, beside the pairing

class ParamsKZG {
 public:
  ParamsKZG(const Context& ctx, uint32_t k, const G1Affine* g, const G1Affine* g_lagrange) : ctx_(ctx), k_(k) {
    ctx_.check(amdzk_srs_upload(ctx_.get(), (const uint64_t*)g, (const uint64_t*)g_lagrange, k, &h_));
  }
  // ParamsKZG::setup(k, rng) with the trapdoor given explicitly (tests / benchmarks, as unsafe as upstream's).
  // Throws for s >= r and for s^n = 1 (amdzk_srs_setup).
  static ParamsKZG setup(const Context& ctx, uint32_t k, const Fr& s) {
    amdzk_srs* h = nullptr;
    ctx.check(amdzk_srs_setup(ctx.get(), k, s.l, &h, nullptr, nullptr));
    return ParamsKZG(ctx, k, h);
  }
  static ParamsKZG read(const Context& ctx, const std::vector<uint8_t>& data, uint8_t g2[64] = nullptr, uint8_t s_g2[64] = nullptr) {
    if (data.size() < 4) throw Error(AMDZK_E_INVALID, "ParamsKZG::read: truncated");
    uint32_t k;
    std::memcpy(&k, data.data(), 4);
    amdzk_srs* h = nullptr;
    ctx.check(amdzk_srs_read(ctx.get(), data.data(), data.size(), &h, g2, s_g2));
    return ParamsKZG(ctx, k, h);
  }
  std::vector<uint8_t> write(const uint8_t g2[64], const uint8_t s_g2[64]) const {
    std::vector<uint8_t> out(amdzk_srs_serialized_size(k_));
    ctx_.check(amdzk_srs_write(ctx_.get(), h_, g2, s_g2, out.data(), out.size()));
    return out;
  }
  void downsize(uint32_t k) {
    amdzk_srs* h = nullptr;
    ctx_.check(amdzk_srs_downsize(ctx_.get(), h_, k, &h));
    amdzk_srs_free(ctx_.get(), h_);
    h_ = h;
    k_ = k;
  }
  // amdzk_srs_check: is this SRS an SRS? g2 / s_g2 e.g. G2Affine::from_bytes of the file's two fields. rho (< r) wins over
  // seed; with neither, 64 bits from std::random_device. checks: AMDZK_SRS_CHECK_* bits, 0 = all. Consistent iff
  // report.failed == 0 and report.ran covers what was asked.
  amdzk_srs_report check(const G2Affine& g2, const G2Affine& s_g2, const uint64_t* seed = nullptr, const Fr* rho = nullptr,
                         uint32_t checks = 0) const;
  std::vector<G1Affine> get_g() const { return get(0); }
  std::vector<G1Affine> get_g_lagrange() const { return get(1); }
  G1 commit(const std::vector<Fr>& poly) const { return msm(0, poly); }            // blind ignored for KZG
  G1 commit_lagrange(const std::vector<Fr>& poly) const { return msm(1, poly); }
  uint32_t k() const { return k_; }
  uint64_t n() const { return (uint64_t)1 << k_; }
  const amdzk_srs* handle() const { return h_; }

  ~ParamsKZG() {
    if (h_) amdzk_srs_free(ctx_.get(), h_);
  }
  ParamsKZG(ParamsKZG&& o) noexcept : ctx_(o.ctx_), k_(o.k_), h_(o.h_) { o.h_ = nullptr; }
  ParamsKZG(const ParamsKZG&) = delete;
  ParamsKZG& operator=(const ParamsKZG&) = delete;

 private:
  ParamsKZG(const Context& ctx, uint32_t k, amdzk_srs* h) : ctx_(ctx), k_(k), h_(h) {}
  std::vector<G1Affine> get(int basis) const {
    std::vector<G1Affine> out((size_t)1 << k_);
    ctx_.check(amdzk_srs_get(ctx_.get(), h_, basis, (uint64_t*)out.data()));
    return out;
  }
  G1 msm(int basis, const std::vector<Fr>& poly) const {
    G1 out;
    ctx_.check(amdzk_msm_g1(ctx_.get(), h_, basis, (const uint64_t*)poly.data(), poly.size(), (uint64_t*)&out));
    return out;
  }
  const Context& ctx_;
  uint32_t k_;
  amdzk_srs* h_ = nullptr;
};

// arithmetic::best_multiexp(coeffs, bases) over the caller's own points — no ParamsKZG, no window table, any length
// (amdzk_msm_g1_bases). For bases that serve a few MSMs; a ParamsKZG pays for its table after the number of commitments
// INTEGRATION.md gives. The result is normalised (z = 1, or the identity (0, 1, 0)).
inline G1 best_multiexp(const Context& ctx, const std::vector<Fr>& coeffs, const std::vector<G1Affine>& bases) {
  if (coeffs.size() != bases.size()) throw Error(AMDZK_E_INVALID, "best_multiexp: coeffs.len() != bases.len()");
  G1 out;
  ctx.check(amdzk_msm_g1_bases(ctx.get(), (const uint64_t*)coeffs.data(), (const uint64_t*)bases.data(), coeffs.size(), (uint64_t*)&out));
  return out;
}

// ------------------------------------------------------------------------------------------ keys and proofs
// What ProvingKey::check_witness found (amdzk_check_witness: MockProver::verify's constraint checks on the device): one
// entry per failing constraint — a gate polynomial, a lookup, a column of the permutation — with the number of failing
// rows and the smallest of them, ordered by kind, then index. ok() iff there is none.
struct CheckFailure {
  enum Kind : uint32_t { Gate = AMDZK_CHECK_GATE, Lookup = AMDZK_CHECK_LOOKUP, Copy = AMDZK_CHECK_COPY };
  Kind kind;
  uint32_t index, first_row;
  uint64_t count;
};
struct WitnessReport {
  std::vector<CheckFailure> failures;
  bool ok() const { return failures.empty(); }
};

class VerifyingKey;  // below, beside the verifier

// plonk::keygen_vk + keygen_pk: fixed[c] = the 2^k Lagrange values of fixed column c (selectors included).
class ProvingKey {
 public:
  // flags: AMDZK_KEYGEN_* of include/amdzk.h or'ed together; kEnvDefaults = amdzk_keygen (the modes from the environment)
  static constexpr uint32_t kEnvDefaults = 0xffffffffu;
  ProvingKey(const Context& ctx, const ParamsKZG& params, const ConstraintSystem& cs, const std::vector<std::vector<Fr>>& fixed,
             const Assembly& assembly, const Fr& transcript_repr, uint32_t flags = kEnvDefaults)
      : ctx_(ctx), num_fixed_(cs.num_fixed), num_perm_(cs.permutation_columns.size()), num_advice_(cs.num_advice), k_(params.k()) {
    const size_t n = (size_t)1 << k_;
    if (fixed.size() != cs.num_fixed) throw Error(AMDZK_E_INVALID, "keygen: fixed column count");
    if (assembly.n() != n || assembly.num_columns() != num_perm_) throw Error(AMDZK_E_INVALID, "keygen: assembly shape");
    std::vector<Fr> flat(fixed.size() * n, Fr::zero());
    for (size_t c = 0; c < fixed.size(); c++) {
      if (fixed[c].size() > n) throw Error(AMDZK_E_INVALID, "keygen: fixed column longer than 2^k");
      std::copy(fixed[c].begin(), fixed[c].end(), flat.begin() + c * n);
    }
    CircuitData cd(cs, k_);
    const uint64_t* fx = flat.empty() ? nullptr : (const uint64_t*)flat.data();
    const uint32_t* mp = num_perm_ ? assembly.mapping() : nullptr;
    if (cd.phased) {
      ctx_.check(amdzk_keygen_phased(ctx_.get(), params.handle(), &cd.c, &cd.phases, fx, mp, transcript_repr.l, resolve(flags), &h_));
    } else if (flags == kEnvDefaults) ctx_.check(amdzk_keygen(ctx_.get(), params.handle(), &cd.c, fx, mp, transcript_repr.l, &h_));
    else ctx_.check(amdzk_keygen_ex(ctx_.get(), params.handle(), &cd.c, fx, mp, transcript_repr.l, flags, &h_));
  }
  ~ProvingKey() {
    if (h_) amdzk_pk_free(ctx_.get(), h_);
  }
  ProvingKey(const ProvingKey&) = delete;
  ProvingKey& operator=(const ProvingKey&) = delete;
  // ProvingKey::read for a fork that parsed upstream's own file: the key from the sigma columns it holds
  // (pk.permutation.permutations, Lagrange form, one vector of 2^k per permutation column) instead of the Assembly
  // (amdzk_keygen_sigma). The same key as the constructor's.
  static std::unique_ptr<ProvingKey> from_sigma(const Context& ctx, const ParamsKZG& params, const ConstraintSystem& cs,
                                                const std::vector<std::vector<Fr>>& fixed, const std::vector<std::vector<Fr>>& sigma,
                                                const Fr& transcript_repr, uint32_t flags = kEnvDefaults) {
    std::unique_ptr<ProvingKey> pk(new ProvingKey(ctx, cs.num_fixed, cs.permutation_columns.size(), cs.num_advice, params.k()));
    const size_t n = (size_t)1 << pk->k_;
    if (fixed.size() != pk->num_fixed_ || sigma.size() != pk->num_perm_) throw Error(AMDZK_E_INVALID, "keygen: column count");
    auto flatten = [n](const std::vector<std::vector<Fr>>& cols) {
      std::vector<Fr> flat(cols.size() * n, Fr::zero());
      for (size_t c = 0; c < cols.size(); c++) {
        if (cols[c].size() > n) throw Error(AMDZK_E_INVALID, "keygen: column longer than 2^k");
        std::copy(cols[c].begin(), cols[c].end(), flat.begin() + c * n);
      }
      return flat;
    };
    const std::vector<Fr> fx = flatten(fixed), sg = flatten(sigma);
    CircuitData cd(cs, pk->k_);
    ctx.check(amdzk_keygen_sigma(ctx.get(), params.handle(), &cd.c, cd.phased ? &cd.phases : nullptr, fx.empty() ? nullptr : (const uint64_t*)fx.data(),
                                 sg.empty() ? nullptr : (const uint64_t*)sg.data(), transcript_repr.l, resolve(flags), &pk->h_));
    return pk;
  }
  // The key of a file write() made (amdzk_pk_read), under the parameters the key was made with: a file paired with another
  // SRS, a damaged or truncated one is refused with a message that starts "pk_read:".
  static std::unique_ptr<ProvingKey> read(const Context& ctx, const ParamsKZG& params, const std::vector<uint8_t>& data,
                                          uint32_t flags = kEnvDefaults) {
    std::unique_ptr<ProvingKey> pk(new ProvingKey(ctx, 0, 0, 0, params.k()));  // amdzk_pk_read refuses a file of another k
    ctx.check(amdzk_pk_read(ctx.get(), params.handle(), data.data(), data.size(), resolve(flags), &pk->h_));
    // The shape from the key that was read, not from amdzk_pk_blob_info: that would hash the whole file a second time.
    const size_t n = (size_t)1 << pk->k_;
    size_t count = 0;
    ctx.check(amdzk_pk_export(ctx.get(), pk->h_, 0, nullptr, 0, &count));
    pk->num_fixed_ = count / n;
    ctx.check(amdzk_pk_export(ctx.get(), pk->h_, 1, nullptr, 0, &count));
    pk->num_perm_ = count / n;
    uint32_t na = 0;
    std::memcpy(&na, data.data() + 20, 4);  // magic (8), format version, k, num_fixed, then num_advice: the file was accepted
    pk->num_advice_ = na;
    return pk;
  }
  // The key file (include/amdzk.h has the layout): everything keygen took except the SRS and the mode flags.
  std::vector<uint8_t> write() const {
    std::vector<uint8_t> out(amdzk_pk_serialized_size(h_));
    size_t written = 0;
    ctx_.check(amdzk_pk_write(ctx_.get(), h_, out.data(), out.size(), &written));
    out.resize(written);
    return out;
  }
  // amdzk_pk_export: what = 0 the fixed columns (Lagrange), 1 the sigma columns (Lagrange), 2 / 3 the same as coefficients;
  // column c is [c * 2^k, (c + 1) * 2^k) — what a fork's ProvingKey::write stores of a key made on the device.
  std::vector<Fr> export_columns(int what) const {
    size_t count = 0;
    ctx_.check(amdzk_pk_export(ctx_.get(), h_, what, nullptr, 0, &count));
    std::vector<Fr> out(count, Fr::zero());
    ctx_.check(amdzk_pk_export(ctx_.get(), h_, what, count ? (uint64_t*)out.data() : nullptr, count, &count));
    return out;
  }
  // amdzk_pk_clone_workspace: a key sharing this key's material that owns one more circuit instance's per-proof
  // workspace (the second, third, ... instance of a multi-circuit create_proof, or one more proof in flight). It and
  // this key are freed in any order: the last handle frees the key material.
  std::unique_ptr<ProvingKey> clone_workspace() const {
    std::unique_ptr<ProvingKey> c(new ProvingKey(ctx_, num_fixed_, num_perm_, num_advice_, k_));
    ctx_.check(amdzk_pk_clone_workspace(ctx_.get(), h_, &c->h_));
    return c;
  }
  // VerifyingKey::{fixed_commitments, permutation.commitments}
  void commitments(std::vector<G1Affine>& fixed, std::vector<G1Affine>& permutation) const {
    fixed.assign(num_fixed_, G1Affine{});
    permutation.assign(num_perm_, G1Affine{});
    ctx_.check(amdzk_pk_commitments(h_, num_fixed_ ? (uint64_t*)fixed.data() : nullptr, num_perm_ ? (uint64_t*)permutation.data() : nullptr));
  }
  // dev::MockProver::run(k, &circuit, instances) followed by verify(), for a witness that is already resident: does it
  // satisfy the circuit, and if not, which gates, lookups and copy constraints fail and where (include/amdzk.h has the
  // semantics). d_advice: the witness columns on the GPU (column c at d_advice + c * advice_stride Fr), read unblinded.
  // theta_seed seeds the theta that compresses multi-expression lookups; challenges: the values of a phased key's
  // challenges. Overwrites the key's per-proof workspace (one call at a time per key, as for create_proof).
  WitnessReport check_witness(const std::vector<std::vector<Fr>>& instances, const void* d_advice, size_t advice_stride, uint64_t theta_seed = 0,
                              const std::vector<Fr>& challenges = {}) const {
    std::vector<const uint64_t*> ptrs(std::max<size_t>(1, instances.size()), nullptr);
    std::vector<size_t> lens(std::max<size_t>(1, instances.size()), 0);
    for (size_t i = 0; i < instances.size(); i++) {
      ptrs[i] = instances[i].empty() ? nullptr : (const uint64_t*)instances[i].data();
      lens[i] = instances[i].size();
    }
    amdzk_check_opts opts = {};
    opts.size = sizeof(opts);
    opts.theta_seed = theta_seed;
    opts.challenges = challenges.empty() ? nullptr : (const uint64_t*)challenges.data();
    opts.num_challenges = (uint32_t)challenges.size();
    // one call in the common cases (a satisfying witness, or up to kFirst failing constraints); a longer report is fetched
    // by a second call with room for all of it
    constexpr size_t kFirst = 64;
    std::vector<amdzk_check_failure> raw(kFirst);
    size_t total = 0;
    ctx_.check(amdzk_check_witness(ctx_.get(), h_, ptrs.data(), lens.data(), d_advice, advice_stride, &opts, raw.data(), raw.size(), &total));
    if (total > raw.size()) {
      raw.resize(total);
      ctx_.check(amdzk_check_witness(ctx_.get(), h_, ptrs.data(), lens.data(), d_advice, advice_stride, &opts, raw.data(), raw.size(), &total));
    }
    raw.resize(std::min(total, raw.size()));
    WitnessReport rep;
    for (const amdzk_check_failure& f : raw) rep.failures.push_back(CheckFailure{(CheckFailure::Kind)f.kind, f.index, f.first_row, f.count});
    return rep;
  }
  // ProvingKey::get_vk (amdzk_vk_from_pk): the key's VerifyingKey, which may outlive this key and its params
  std::unique_ptr<VerifyingKey> get_vk() const;
  amdzk_pk* handle() const { return h_; }
  uint32_t k() const { return k_; }
  size_t num_advice() const { return num_advice_; }

 private:
  ProvingKey(const Context& ctx, size_t nf, size_t np, size_t na, uint32_t k) : ctx_(ctx), num_fixed_(nf), num_perm_(np), num_advice_(na), k_(k) {}
  static uint32_t resolve(uint32_t flags) {  // kEnvDefaults: the modes as amdzk_keygen reads them from the environment
    if (flags != kEnvDefaults) return flags;
    const char *fc = std::getenv("AMDZK_FULL_COSETS"), *se = std::getenv("AMDZK_SERIAL");
    return (fc && (std::atoi(fc) != 0 || !*fc) ? AMDZK_KEYGEN_FULL_COSETS : 0u) | (se && std::atoi(se) != 0 ? AMDZK_KEYGEN_SERIAL : 0u);
  }
  const Context& ctx_;
  size_t num_fixed_, num_perm_, num_advice_;
  uint32_t k_;
  amdzk_pk* h_ = nullptr;
};

enum class Transcript : int { Blake2b = AMDZK_TRANSCRIPT_BLAKE2B, Keccak256Evm = AMDZK_TRANSCRIPT_KECCAK256_EVM };
// The `P: Prover` type parameter of create_proof: poly::kzg::multiopen::{ProverSHPLONK, ProverGWC}.
enum class Multiopen : int { Shplonk = 0, Gwc = AMDZK_MULTIOPEN_GWC };

// plonk::create_proof(params, pk, &[circuit], &[instances], ChaCha20Rng::seed_from_u64(seed), transcript) for
// one circuit. `d_advice`: the witness columns resident on the GPU (column c at d_advice + c*stride Fr).
inline std::vector<uint8_t> create_proof(const Context& ctx, const ProvingKey& pk, const std::vector<std::vector<Fr>>& instances,
                                         const void* d_advice, size_t advice_stride, uint64_t rng_seed,
                                         Transcript transcript = Transcript::Blake2b, Multiopen multiopen = Multiopen::Shplonk) {
  const int format = (int)transcript | (int)multiopen;
  std::vector<const uint64_t*> ptrs(std::max<size_t>(1, instances.size()), nullptr);
  std::vector<size_t> lens(std::max<size_t>(1, instances.size()), 0);
  for (size_t i = 0; i < instances.size(); i++) {
    ptrs[i] = instances[i].empty() ? nullptr : (const uint64_t*)instances[i].data();
    lens[i] = instances[i].size();
  }
  size_t need = 0;
  std::vector<uint8_t> proof(amdzk_proof_size(pk.handle(), format));
  ctx.check(amdzk_create_proof_ex(ctx.get(), pk.handle(), ptrs.data(), lens.data(), d_advice, advice_stride, rng_seed, format,
                                  proof.data(), proof.size(), &need));
  proof.resize(need);
  return proof;
}

namespace detail {
// instances[c][col] as the tables the C entry points read — pp[c][col]: column col of circuit (or proof) c, null if it is
// empty; lp[c][col]: its length; a circuit without instance columns still has one (null, 0) entry — and, with keys, pks[c]:
// their handles. The containers it was built from must outlive it.
struct InstanceTables {
  std::vector<std::vector<const uint64_t*>> ptrs;
  std::vector<std::vector<size_t>> lens;
  std::vector<const uint64_t* const*> pp;
  std::vector<const size_t*> lp;
  std::vector<amdzk_pk*> pks;
  InstanceTables() = default;
  InstanceTables(const std::vector<std::vector<std::vector<Fr>>>& instances, const std::vector<const ProvingKey*>& keys) {
    for (const ProvingKey* k : keys) pks.push_back(k->handle());
    for (const auto& cols : instances) add(cols);
    finish();
  }
  void add(const std::vector<std::vector<Fr>>& cols) {
    ptrs.emplace_back(std::max<size_t>(1, cols.size()), nullptr);
    lens.emplace_back(std::max<size_t>(1, cols.size()), 0);
    for (size_t i = 0; i < cols.size(); i++) {
      ptrs.back()[i] = cols[i].empty() ? nullptr : (const uint64_t*)cols[i].data();
      lens.back()[i] = cols[i].size();
    }
  }
  void finish() {  // after the last add
    pp.assign(std::max<size_t>(1, ptrs.size()), nullptr);
    lp.assign(std::max<size_t>(1, ptrs.size()), nullptr);
    for (size_t i = 0; i < ptrs.size(); i++) pp[i] = ptrs[i].data(), lp[i] = lens[i].data();
  }
};
}  // namespace detail

// plonk::create_proof(params, pk, &[circuit; N], &[instances; N], rng, transcript): N instances of the key's circuit in
// ONE proof (upstream's slices). keys[c]: instance c's workspace — the key itself and ProvingKey::clone_workspace() handles,
// pairwise different; instances[c], d_advice[c] as for one circuit.
inline std::vector<uint8_t> create_proof(const Context& ctx, const std::vector<const ProvingKey*>& keys,
                                         const std::vector<std::vector<std::vector<Fr>>>& instances, const std::vector<const void*>& d_advice,
                                         size_t advice_stride, uint64_t rng_seed, Transcript transcript = Transcript::Blake2b,
                                         Multiopen multiopen = Multiopen::Shplonk) {
  const size_t N = keys.size();
  if (N == 0 || instances.size() != N || d_advice.size() != N) throw Error(AMDZK_E_INVALID, "create_proof: one key, instance set and witness per circuit");
  const int format = (int)transcript | (int)multiopen;
  const detail::InstanceTables in(instances, keys);
  size_t need = 0;
  std::vector<uint8_t> proof(amdzk_proof_size_multi(in.pks[0], N, format));
  ctx.check(amdzk_create_proof_multi(ctx.get(), in.pks.data(), N, in.pp.data(), in.lp.data(), d_advice.data(), advice_stride, rng_seed, format, proof.data(),
                                     proof.size(), &need));
  proof.resize(need);
  return proof;
}

// amdzk_create_proof_batch: keys.size() INDEPENDENT proofs of one circuit (own transcript, RNG stream and challenges each)
// from one host thread, advanced in lock-step on the context's stream — every step's commitments of all proofs in one MSM,
// one host wait per step. keys[b]: proof b's workspace — the key itself and ProvingKey::clone_workspace() handles, pairwise
// different; instances[b], d_advice[b], rng_seeds[b] as for one proof, and proof b's bytes are create_proof's for the same
// arguments. A proof whose witness fails (a lookup input not in its table, ...) comes back with its status and no bytes while
// the others finish; `error` is set for the first failing proof (the library keeps one message). A refused call throws.
struct BatchProof {
  int status = AMDZK_OK;
  std::vector<uint8_t> proof;
  std::string error;
};
namespace detail {
// What a batch call left — rc, the proofs' bytes at `stride`, their lengths and statuses — as one BatchProof each. A call
// that was refused as a whole (or ended for all by the device) throws: its message is not one proof's ("proof <b>: ...").
inline std::vector<BatchProof> batch_proofs(const Context& ctx, int rc, const std::vector<uint8_t>& bytes, size_t stride,
                                            const std::vector<size_t>& got, const std::vector<int>& st) {
  if (rc != AMDZK_OK && std::string(amdzk_last_error(ctx.get())).rfind("proof ", 0) != 0) ctx.check(rc);
  std::vector<BatchProof> out(st.size());
  bool first = true;
  for (size_t b = 0; b < st.size(); b++) {
    out[b].status = st[b];
    if (st[b] == AMDZK_OK) out[b].proof.assign(bytes.begin() + b * stride, bytes.begin() + b * stride + got[b]);
    else if (first) out[b].error = amdzk_last_error(ctx.get()), first = false;
  }
  return out;
}
}  // namespace detail
inline std::vector<BatchProof> create_proof_batch(const Context& ctx, const std::vector<const ProvingKey*>& keys,
                                                  const std::vector<std::vector<std::vector<Fr>>>& instances,
                                                  const std::vector<const void*>& d_advice, size_t advice_stride,
                                                  const std::vector<uint64_t>& rng_seeds, Transcript transcript = Transcript::Blake2b,
                                                  Multiopen multiopen = Multiopen::Shplonk) {
  const size_t N = keys.size();
  if (N == 0 || instances.size() != N || d_advice.size() != N || rng_seeds.size() != N)
    throw Error(AMDZK_E_INVALID, "create_proof_batch: one key, instance set, witness and seed per proof");
  const int format = (int)transcript | (int)multiopen;
  const detail::InstanceTables in(instances, keys);
  amdzk_batch_opts opts = {};
  opts.size = sizeof(opts);
  opts.transcript_kind = format;
  opts.rng_seeds = rng_seeds.data();
  const size_t stride = amdzk_proof_size(in.pks[0], format);
  std::vector<uint8_t> bytes(stride * N);
  std::vector<size_t> got(N, 0);
  std::vector<int> st(N, AMDZK_OK);
  const int rc = amdzk_create_proof_batch(ctx.get(), in.pks.data(), N, in.pp.data(), in.lp.data(), d_advice.data(), advice_stride, &opts, bytes.data(),
                                          stride, got.data(), st.data());
  return detail::batch_proofs(ctx, rc, bytes, stride, got, st);
}

// transcript::TranscriptWrite as far as create_proof uses it: implement it to own the transcript (`&mut T:
// TranscriptWrite` upstream). Values are Montgomery; a point is never the identity. Throwing from a member ends the
// proof: the exception is rethrown by create_proof once the library has returned.
class TranscriptWrite {
 public:
  virtual ~TranscriptWrite() {}
  virtual void common_point(const G1Affine& p) = 0;
  virtual void common_scalar(const Fr& s) = 0;
  virtual void write_point(const G1Affine& p) = 0;
  virtual void write_scalar(const Fr& s) = 0;
  virtual Fr squeeze_challenge() = 0;
};

// What `synthesize` of a circuit with challenge phases is here: called once per phase >= 1 with the challenges known so
// far (index order; those of unfinished phases are zero), it fills that phase's advice columns of every instance on the
// device — work on `hip_stream` is ordered before the library's read, anything else must be complete on return.
using Synthesize = std::function<void(uint32_t phase, const std::vector<Fr>& challenges, void* hip_stream)>;

namespace detail {
// what the C callbacks of amdzk_create_proof_opts get as `user`: nothing may unwind through the library, so the first
// exception is kept and rethrown by create_proof
struct Trampoline {
  const Synthesize* syn;
  TranscriptWrite* t;
  std::exception_ptr err;
  template <class F>
  int guard(F&& f) {
    try {
      f();
      return 0;
    } catch (...) {
      if (!err) err = std::current_exception();
      return 1;
    }
  }
};
// the amdzk_transcript that forwards to tr->t
inline amdzk_transcript c_transcript(Trampoline* tr) {
  amdzk_transcript ct;
  ct.user = tr;
  ct.common_point = [](void* u, const uint64_t* xy) { auto* t = (Trampoline*)u; return t->guard([&] { G1Affine p; std::memcpy(&p, xy, 64); t->t->common_point(p); }); };
  ct.common_scalar = [](void* u, const uint64_t* s) { auto* t = (Trampoline*)u; return t->guard([&] { Fr v; std::memcpy(v.l, s, 32); t->t->common_scalar(v); }); };
  ct.write_point = [](void* u, const uint64_t* xy) { auto* t = (Trampoline*)u; return t->guard([&] { G1Affine p; std::memcpy(&p, xy, 64); t->t->write_point(p); }); };
  ct.write_scalar = [](void* u, const uint64_t* s) { auto* t = (Trampoline*)u; return t->guard([&] { Fr v; std::memcpy(v.l, s, 32); t->t->write_scalar(v); }); };
  ct.squeeze_challenge = [](void* u, uint64_t* out) { auto* t = (Trampoline*)u; return t->guard([&] { Fr v = t->t->squeeze_challenge(); std::memcpy(out, v.l, 32); }); };
  return ct;
}
}  // namespace detail

// plonk::create_proof for circuits with challenge phases and / or the caller's own transcript (amdzk_create_proof_opts).
// keys / instances / d_advice as for the multi-circuit overload (one entry each for one circuit). With `transcript_obj`
// the bytes are the caller's and the result is empty; `transcript` then only selects nothing and `multiopen` still counts.
inline std::vector<uint8_t> create_proof(const Context& ctx, const std::vector<const ProvingKey*>& keys,
                                         const std::vector<std::vector<std::vector<Fr>>>& instances, const std::vector<const void*>& d_advice,
                                         size_t advice_stride, uint64_t rng_seed, const Synthesize& synthesize,
                                         TranscriptWrite* transcript_obj = nullptr, Transcript transcript = Transcript::Blake2b,
                                         Multiopen multiopen = Multiopen::Shplonk) {
  const size_t N = keys.size();
  if (N == 0 || instances.size() != N || d_advice.size() != N) throw Error(AMDZK_E_INVALID, "create_proof: one key, instance set and witness per circuit");
  detail::Trampoline tr{&synthesize, transcript_obj, nullptr};
  amdzk_transcript ct = detail::c_transcript(&tr);
  amdzk_proof_opts opts;
  std::memset(&opts, 0, sizeof(opts));
  opts.size = sizeof(opts);
  opts.transcript_kind = (int)transcript | (int)multiopen;
  opts.transcript = transcript_obj ? &ct : nullptr;
  opts.phase_user = &tr;
  if (synthesize)
    opts.phase_fn = [](void* u, uint32_t phase, const uint64_t* ch, uint32_t nch, void* stream) {
      auto* t = (detail::Trampoline*)u;
      return t->guard([&] {
        std::vector<Fr> v(nch);
        if (nch) std::memcpy((void*)v.data(), ch, (size_t)nch * 32);
        (*t->syn)(phase, v, stream);
      });
    };
  opts.rng_seed = rng_seed;
  const detail::InstanceTables in(instances, keys);
  size_t need = 0;
  std::vector<uint8_t> proof(transcript_obj ? 0 : amdzk_proof_size_multi(in.pks[0], N, opts.transcript_kind));
  const int rc = amdzk_create_proof_opts(ctx.get(), in.pks.data(), N, in.pp.data(), in.lp.data(), d_advice.data(), advice_stride, &opts, proof.data(),
                                         proof.size(), &need);
  if (rc != AMDZK_OK && tr.err) std::rethrow_exception(tr.err);
  ctx.check(rc);
  proof.resize(need);
  return proof;
}

// What `synthesize` of the later phases is for a BATCH (amdzk_batch_phase_fn): called once per phase >= 1 for all proofs
// together. wanted[b] != 0: proof b is live and its circuit has advice columns in `phase`; challenges[b]: its challenges
// known so far (those of unfinished phases, and all of a proof that is not wanted, are zero; every row has the largest
// challenge count of the batch). It fills that phase's columns of every wanted proof on the device — a witness program
// (WitnessProgram below) computes them for the whole batch in one run — and returns per-proof codes: empty or all zero for
// success, a non-zero entry drops that proof alone. Throwing drops every wanted proof; the exception is rethrown.
using BatchSynthesize = std::function<std::vector<int>(uint32_t phase, const std::vector<uint8_t>& wanted,
                                                        const std::vector<std::vector<Fr>>& challenges, void* hip_stream)>;

// amdzk_create_proof_batch_opts: create_proof_batch for circuits with challenge phases, proofs with the caller's transcript
// and DIFFERENT circuits — keys[b] any key or workspace clone made on one ParamsKZG, pairwise different. transcripts: empty,
// or one entry per proof (nullptr = the built-in `transcript`); a proof with its own transcript comes back with status 0 and
// no bytes. Proof b's bytes, and the calls its transcript receives, are those of the opts overload of create_proof on
// keys[b] alone. Failures as for create_proof_batch.
inline std::vector<BatchProof> create_proof_batch(const Context& ctx, const std::vector<const ProvingKey*>& keys,
                                                  const std::vector<std::vector<std::vector<Fr>>>& instances,
                                                  const std::vector<const void*>& d_advice, size_t advice_stride,
                                                  const std::vector<uint64_t>& rng_seeds, const std::vector<TranscriptWrite*>& transcripts,
                                                  const BatchSynthesize& synthesize, Transcript transcript = Transcript::Blake2b,
                                                  Multiopen multiopen = Multiopen::Shplonk) {
  const size_t N = keys.size();
  if (N == 0 || instances.size() != N || d_advice.size() != N || rng_seeds.size() != N || (!transcripts.empty() && transcripts.size() != N))
    throw Error(AMDZK_E_INVALID, "create_proof_batch: one key, instance set, witness, seed and transcript entry per proof");
  const int format = (int)transcript | (int)multiopen;
  struct Shared {
    const BatchSynthesize* syn;
    std::exception_ptr err;
  } shared{&synthesize, nullptr};
  std::vector<detail::Trampoline> trs(N, detail::Trampoline{nullptr, nullptr, nullptr});
  std::vector<amdzk_transcript> cts(N);
  std::vector<const amdzk_transcript*> ctp(N, nullptr);
  for (size_t b = 0; b < N && !transcripts.empty(); b++) {
    if (!transcripts[b]) continue;
    trs[b].t = transcripts[b];
    cts[b] = detail::c_transcript(&trs[b]);
    ctp[b] = &cts[b];
  }
  amdzk_batch_proof_opts opts;
  std::memset(&opts, 0, sizeof(opts));
  opts.size = sizeof(opts);
  opts.transcript_kind = format;
  opts.rng_seeds = rng_seeds.data();
  opts.transcripts = transcripts.empty() ? nullptr : ctp.data();
  opts.phase_user = &shared;
  if (synthesize)
    opts.phase_fn = [](void* u, uint32_t phase, size_t n_proofs, const uint8_t* wanted, const uint64_t* ch, size_t stride, int* proof_rc, void* stream) {
      auto* s = (Shared*)u;
      try {
        std::vector<uint8_t> w(wanted, wanted + n_proofs);
        std::vector<std::vector<Fr>> c(n_proofs, std::vector<Fr>(stride));
        for (size_t b = 0; b < n_proofs && stride; b++) std::memcpy((void*)c[b].data(), ch + 4 * b * stride, stride * 32);
        const std::vector<int> rc = (*s->syn)(phase, w, c, stream);
        for (size_t b = 0; b < n_proofs && b < rc.size(); b++) proof_rc[b] = rc[b];
        return 0;
      } catch (...) {
        if (!s->err) s->err = std::current_exception();
        return 1;
      }
    };
  const detail::InstanceTables in(instances, keys);
  size_t stride = 0;
  for (size_t b = 0; b < N; b++)
    if (!ctp[b]) stride = std::max(stride, amdzk_proof_size(in.pks[b], format));
  std::vector<uint8_t> bytes(std::max<size_t>(1, stride * N));
  std::vector<size_t> got(N, 0);
  std::vector<int> st(N, AMDZK_OK);
  const int rc = amdzk_create_proof_batch_opts(ctx.get(), in.pks.data(), N, in.pp.data(), in.lp.data(), d_advice.data(), advice_stride, &opts, bytes.data(),
                                               stride, got.data(), st.data());
  if (shared.err) std::rethrow_exception(shared.err);
  for (auto& t : trs)
    if (t.err) std::rethrow_exception(t.err);
  return detail::batch_proofs(ctx, rc, bytes, stride, got, st);
}

// Convenience for host-resident witnesses (what a WitnessCollection holds after synthesis): uploads the
// advice columns (padded with zeros to 2^k rows), proves, frees.
inline std::vector<uint8_t> create_proof(const Context& ctx, const ProvingKey& pk, const std::vector<std::vector<Fr>>& instances,
                                         const std::vector<std::vector<Fr>>& advice, uint64_t rng_seed,
                                         Transcript transcript = Transcript::Blake2b, Multiopen multiopen = Multiopen::Shplonk) {
  const size_t n = (size_t)1 << pk.k();
  if (advice.size() != pk.num_advice()) throw Error(AMDZK_E_INVALID, "create_proof: advice column count");
  std::vector<Fr> flat(std::max<size_t>(1, advice.size()) * n, Fr::zero());
  for (size_t c = 0; c < advice.size(); c++) {
    if (advice[c].size() > n) throw Error(AMDZK_E_INVALID, "create_proof: advice column longer than 2^k");
    std::copy(advice[c].begin(), advice[c].end(), flat.begin() + c * n);
  }
  void* d = nullptr;
  ctx.check(amdzk_dev_alloc(ctx.get(), flat.size() * sizeof(Fr), &d));
  std::vector<uint8_t> proof;
  try {
    ctx.check(amdzk_dev_upload(ctx.get(), d, flat.data(), flat.size() * sizeof(Fr)));
    proof = create_proof(ctx, pk, instances, d, n, rng_seed, transcript, multiopen);
  } catch (...) {
    amdzk_dev_free(ctx.get(), d);
    throw;
  }
  amdzk_dev_free(ctx.get(), d);
  return proof;
}

// ------------------------------------------------------------------------------------------ multiopen on its own
// poly::kzg::multiopen::{ProverSHPLONK, ProverGWC} over the caller's polynomials (amdzk_multiopen_dev): for a fork that
// keeps upstream's create_proof and swaps the opening argument, and for KZG outside PLONK (commit, then open).
// poly::query::ProverQuery: `poly` = 2^k coefficients on the device (Montgomery); its identity is its address, as
// upstream's PolynomialPointer compares. `point` is any field element; equal values are one point. `eval` is only read
// by create_proof(.., use_evals = true) and is then TRUSTED, NOT CHECKED, as upstream trusts it.
struct ProverQuery {
  const void* poly;
  Fr point;
  Fr eval;
};

namespace detail {
// Prover::create_proof(params, rng, transcript, queries) of poly::commitment; returns the points it wrote
inline std::vector<G1Affine> multiopen(const Context& ctx, const ParamsKZG& params, Multiopen scheme, TranscriptWrite& transcript,
                                       const std::vector<ProverQuery>& queries, bool use_evals) {
  std::vector<const void*> polys;
  std::vector<Fr> points;
  std::map<const void*, uint32_t> poly_of;
  std::map<std::array<uint64_t, 4>, uint32_t> point_of;
  std::vector<amdzk_open_query> q(queries.size());
  std::vector<Fr> evals(queries.size());
  for (size_t i = 0; i < queries.size(); i++) {
    auto pi = poly_of.find(queries[i].poly);
    if (pi == poly_of.end()) {
      pi = poly_of.emplace(queries[i].poly, (uint32_t)polys.size()).first;
      polys.push_back(queries[i].poly);
    }
    const std::array<uint64_t, 4> key{{queries[i].point.l[0], queries[i].point.l[1], queries[i].point.l[2], queries[i].point.l[3]}};
    auto zi = point_of.find(key);
    if (zi == point_of.end()) {
      zi = point_of.emplace(key, (uint32_t)points.size()).first;
      points.push_back(queries[i].point);
    }
    q[i].poly = pi->second;
    q[i].point = zi->second;
    evals[i] = queries[i].eval;
  }
  Trampoline tr{nullptr, &transcript, nullptr};
  const amdzk_transcript ct = c_transcript(&tr);
  amdzk_multiopen_opts opts;
  std::memset(&opts, 0, sizeof(opts));
  opts.size = sizeof(opts);
  opts.scheme = (int)scheme;
  opts.transcript = &ct;
  opts.evals = use_evals ? (const uint64_t*)evals.data() : nullptr;
  std::vector<G1Affine> out(scheme == Multiopen::Shplonk ? 2 : std::max<size_t>(1, points.size()));
  size_t n_out = 0;
  const int rc = amdzk_multiopen_dev(ctx.get(), params.handle(), polys.data(), polys.size(), (const uint64_t*)points.data(), points.size(), q.data(),
                                     q.size(), &opts, (uint64_t*)out.data(), out.size(), &n_out);
  if (rc != AMDZK_OK && tr.err) std::rethrow_exception(tr.err);
  ctx.check(rc);
  out.resize(n_out);
  return out;
}
}  // namespace detail

class ProverSHPLONK {
 public:
  ProverSHPLONK(const Context& ctx, const ParamsKZG& params) : ctx_(ctx), params_(params) {}
  std::vector<G1Affine> create_proof(TranscriptWrite& transcript, const std::vector<ProverQuery>& queries, bool use_evals = false) const {
    return detail::multiopen(ctx_, params_, Multiopen::Shplonk, transcript, queries, use_evals);
  }

 private:
  const Context& ctx_;
  const ParamsKZG& params_;
};

class ProverGWC {
 public:
  ProverGWC(const Context& ctx, const ParamsKZG& params) : ctx_(ctx), params_(params) {}
  std::vector<G1Affine> create_proof(TranscriptWrite& transcript, const std::vector<ProverQuery>& queries, bool use_evals = false) const {
    return detail::multiopen(ctx_, params_, Multiopen::Gwc, transcript, queries, use_evals);
  }

 private:
  const Context& ctx_;
  const ParamsKZG& params_;
};

// One witness per proof from the host (what a caller does after Circuit::synthesize, /root/reference/src/lib.rs:328-397):
// the advice columns are synthesized into pinned memory, and the upload of proof i+1's witness runs on the ctx's copy
// stream while proof i is proved (amdzk_dev_upload_async / amdzk_upload_fence; double-buffered device staging).
class WitnessStream {
 public:
  WitnessStream(const Context& ctx, const ProvingKey& pk) : ctx_(ctx), pk_(pk), n_((size_t)1 << pk.k()) {
    bytes_ = std::max<size_t>(1, pk.num_advice()) * n_ * sizeof(Fr);
    for (int i = 0; i < 2; i++) {
      ctx_.check(amdzk_dev_alloc(ctx_.get(), bytes_, &dev_[i]));
      ctx_.check(amdzk_host_alloc(ctx_.get(), bytes_, &pin_[i]));
    }
  }
  ~WitnessStream() {
    for (int i = 0; i < 2; i++) {
      if (dev_[i]) amdzk_dev_free(ctx_.get(), dev_[i]);
      if (pin_[i]) amdzk_host_free(ctx_.get(), pin_[i]);
    }
  }
  WitnessStream(const WitnessStream&) = delete;
  WitnessStream& operator=(const WitnessStream&) = delete;

  // create_proof for every (advice, instances, seed) of the batch, in order.
  struct Item {
    const std::vector<std::vector<Fr>>* advice;
    const std::vector<std::vector<Fr>>* instances;
    uint64_t rng_seed;
  };
  std::vector<std::vector<uint8_t>> prove(const std::vector<Item>& items, Transcript transcript = Transcript::Blake2b,
                                          Multiopen multiopen = Multiopen::Shplonk) {
    std::vector<std::vector<uint8_t>> out;
    if (items.empty()) return out;
    stage(0, *items[0].advice);
    for (size_t j = 0; j < items.size(); j++) {
      const int cur = (int)(j & 1);
      ctx_.check(amdzk_upload_fence(ctx_.get()));                    // proof j's witness is (being) uploaded: order the proof behind it
      if (j + 1 < items.size()) stage(cur ^ 1, *items[j + 1].advice);  // proof j-1, the last reader of that buffer, has returned
      out.push_back(create_proof(ctx_, pk_, *items[j].instances, dev_[cur], n_, items[j].rng_seed, transcript, multiopen));
    }
    return out;
  }

 private:
  void stage(int slot, const std::vector<std::vector<Fr>>& advice) {
    if (advice.size() != pk_.num_advice()) throw Error(AMDZK_E_INVALID, "WitnessStream: advice column count");
    Fr* h = (Fr*)pin_[slot];
    for (size_t c = 0; c < advice.size(); c++) {
      if (advice[c].size() > n_) throw Error(AMDZK_E_INVALID, "WitnessStream: advice column longer than 2^k");
      std::copy(advice[c].begin(), advice[c].end(), h + c * n_);
      std::fill(h + c * n_ + advice[c].size(), h + (c + 1) * n_, Fr::zero());
    }
    ctx_.check(amdzk_dev_upload_async(ctx_.get(), dev_[slot], pin_[slot], bytes_));
  }
  const Context& ctx_;
  const ProvingKey& pk_;
  size_t n_, bytes_ = 0;
  void* dev_[2] = {nullptr, nullptr};
  void* pin_[2] = {nullptr, nullptr};
};

// ------------------------------------------------------------------------------------------ witness programs
// The advice cells of a batch computed on the device (amdzk.h "witness programs"): what Circuit::synthesize does for a
// halo2-base style circuit — a fixed straight-line computation over a few per-proof inputs — recorded once as nodes, then
// run for a whole batch straight into the buffers create_proof_batch reads. Every method returns the new node's index; what
// is not field arithmetic the host computes per proof and passes as an input.
class WitnessProgram {
 public:
  using Node = uint32_t;
  WitnessProgram(uint32_t k, uint32_t num_advice) : k_(k), num_advice_(num_advice) {}

  Node input() { return node(AMDZK_W_INPUT, n_inputs_++); }  // inputs are numbered in the order of these calls
  Node constant(const Fr& v) {
    auto it = const_idx_.find(v);
    if (it == const_idx_.end()) {
      it = const_idx_.emplace(v, (uint32_t)constants_.size()).first;
      constants_.push_back(v);
    }
    return node(AMDZK_W_CONST, it->second);
  }
  Node add(Node a, Node b) { return node(AMDZK_W_ADD, a, b); }
  Node sub(Node a, Node b) { return node(AMDZK_W_SUB, a, b); }
  Node mul(Node a, Node b) { return node(AMDZK_W_MUL, a, b); }
  Node neg(Node a) { return node(AMDZK_W_NEG, a); }
  Node inv(Node a) { return node(AMDZK_W_INV, a); }
  Node select(Node cond, Node then, Node otherwise) { return node(AMDZK_W_SELECT, cond, then, otherwise); }
  Node is_zero(Node a) { return node(AMDZK_W_IS_ZERO, a); }
  Node eq(Node a, Node b) { return node(AMDZK_W_EQ, a, b); }
  Node lt(Node a, Node b) { return node(AMDZK_W_LT, a, b); }
  Node bits(Node a, uint32_t lo, uint32_t len) { return node(AMDZK_W_BITS, a, lo, len); }  // (canon(a) >> lo) mod 2^len
  Node and_(Node a, Node b) { return node(AMDZK_W_AND, a, b); }
  Node xor_(Node a, Node b) { return node(AMDZK_W_XOR, a, b); }
  // the value of `n` goes to advice cell (column, row) of every proof
  Node assign(Node n, uint32_t column, uint32_t row) {
    cells_.push_back(amdzk_wcell{n, column, row});
    return n;
  }
  // `n` is returned to the host per proof (an instance value); its position among the publics
  uint32_t expose(Node n) {
    publics_.push_back(n);
    return (uint32_t)publics_.size() - 1;
  }

  // valid while the program is alive and unchanged
  amdzk_witness_desc desc() const {
    amdzk_witness_desc d;
    std::memset(&d, 0, sizeof(d));
    d.size = sizeof(d);
    d.k = k_;
    d.num_advice = num_advice_;
    d.n_inputs = n_inputs_;
    d.n_constants = (uint32_t)constants_.size();
    d.constants = constants_.empty() ? nullptr : constants_[0].l;
    d.n_nodes = (uint32_t)nodes_.size();
    d.nodes = nodes_.data();
    d.n_cells = (uint32_t)cells_.size();
    d.cells = cells_.data();
    d.n_publics = (uint32_t)publics_.size();
    d.publics = publics_.data();
    return d;
  }
  struct Plan {
    uint32_t levels, launches, fused_width;
    size_t scratch_bytes;
  };
  Plan plan(size_t n_proofs) const {  // amdzk_witness_plan: no device needed
    const amdzk_witness_desc d = desc();
    Plan p{};
    char msg[256] = "";
    const int rc = amdzk_witness_plan(&d, n_proofs, &p.levels, &p.launches, &p.fused_width, &p.scratch_bytes, msg, sizeof(msg));
    if (rc != AMDZK_OK) throw Error(rc, msg);
    return p;
  }
  uint32_t k() const { return k_; }
  uint32_t num_inputs() const { return n_inputs_; }
  uint32_t num_publics() const { return (uint32_t)publics_.size(); }

 private:
  Node node(uint32_t op, uint32_t a = 0, uint32_t b = 0, uint32_t c = 0) {
    nodes_.push_back(amdzk_wnode{op, a, b, c});
    return (Node)nodes_.size() - 1;
  }
  uint32_t k_, num_advice_, n_inputs_ = 0;
  std::vector<Fr> constants_;
  std::map<Fr, uint32_t> const_idx_;
  std::vector<amdzk_wnode> nodes_;
  std::vector<amdzk_wcell> cells_;
  std::vector<uint32_t> publics_;
};

// amdzk_witness: a program resident on the context's device. One run at a time.
class CompiledWitness {
 public:
  CompiledWitness(const Context& ctx, const WitnessProgram& prog) : ctx_(ctx), k_(prog.k()), n_inputs_(prog.num_inputs()), n_publics_(prog.num_publics()) {
    const amdzk_witness_desc d = prog.desc();
    ctx_.check(amdzk_witness_compile(ctx_.get(), &d, &h_));
  }
  ~CompiledWitness() {
    if (h_) amdzk_witness_free(ctx_.get(), h_);
  }
  CompiledWitness(const CompiledWitness&) = delete;
  CompiledWitness& operator=(const CompiledWitness&) = delete;

  // inputs[b]: the n_inputs values of proof b; d_advice[b]: its buffer (as for create_proof_batch; advice_stride 0 = 2^k).
  // Returns the publics, one vector per proof.
  std::vector<std::vector<Fr>> run(const std::vector<std::vector<Fr>>& inputs, const std::vector<void*>& d_advice, size_t advice_stride = 0,
                                   uint32_t flags = 0, size_t max_scratch_bytes = 0) const {
    if (inputs.size() != d_advice.size()) throw Error(AMDZK_E_INVALID, "witness: one input row and one buffer per proof");
    std::vector<const uint64_t*> in(inputs.size());
    for (size_t b = 0; b < inputs.size(); b++) {
      if (inputs[b].size() != n_inputs_) throw Error(AMDZK_E_INVALID, "witness: input count");
      in[b] = inputs[b].empty() ? nullptr : inputs[b][0].l;
    }
    std::vector<Fr> flat(inputs.size() * n_publics_);
    ctx_.check(amdzk_witness_run(ctx_.get(), h_, inputs.size(), n_inputs_ ? in.data() : nullptr, d_advice.data(),
                                 advice_stride ? advice_stride : (size_t)1 << k_, flags, max_scratch_bytes, flat.empty() ? nullptr : flat[0].l));
    return split(flat, inputs.size());
  }
  // the inputs resident: proof b at d_inputs + b * input_stride Fr
  std::vector<std::vector<Fr>> run_dev(const void* d_inputs, size_t input_stride, const std::vector<void*>& d_advice, size_t advice_stride = 0,
                                       uint32_t flags = 0, size_t max_scratch_bytes = 0) const {
    std::vector<Fr> flat(d_advice.size() * n_publics_);
    ctx_.check(amdzk_witness_run_dev(ctx_.get(), h_, d_advice.size(), d_inputs, input_stride, d_advice.data(),
                                     advice_stride ? advice_stride : (size_t)1 << k_, flags, max_scratch_bytes, flat.empty() ? nullptr : flat[0].l));
    return split(flat, d_advice.size());
  }
  amdzk_witness* get() const { return h_; }

 private:
  std::vector<std::vector<Fr>> split(const std::vector<Fr>& flat, size_t n) const {
    std::vector<std::vector<Fr>> out(n);
    for (size_t b = 0; b < n; b++) out[b].assign(flat.begin() + b * n_publics_, flat.begin() + (b + 1) * n_publics_);
    return out;
  }
  const Context& ctx_;
  uint32_t k_, n_inputs_, n_publics_;
  amdzk_witness* h_ = nullptr;
};

// ------------------------------------------------------------------------------------------ Poseidon
// The `poseidon` crate's Poseidon<Fr, T, RATE> on the device (amdzk.h "Poseidon over Fr"; parity unpinned): new / update /
// squeeze for one sponge, hash_many and permute for batches. The spec is DATA: the textbook round constants ((r_f + r_p)
// rows of t) and the full t x t MDS matrix — the crate's Spec stores the optimised form, so a caller carries its own copy of
// the generator. initial_state empty = the crate's (2^64, 0, ..., 0).
struct PoseidonSpec {
  uint32_t t = 0, rate = 0, r_f = 0, r_p = 0;
  std::vector<Fr> round_constants, mds, initial_state;
  amdzk_poseidon_desc desc() const {
    if (round_constants.size() != (size_t)(r_f + r_p) * t || mds.size() != (size_t)t * t || (!initial_state.empty() && initial_state.size() != t))
      throw Error(AMDZK_E_INVALID, "poseidon: the spec's arrays do not have (r_f + r_p) * t, t * t and t (or no) elements");
    amdzk_poseidon_desc d;
    std::memset(&d, 0, sizeof(d));
    d.size = sizeof(d);
    d.t = t;
    d.rate = rate;
    d.r_f = r_f;
    d.r_p = r_p;
    d.round_constants = round_constants.empty() ? nullptr : round_constants[0].l;
    d.mds = mds.empty() ? nullptr : mds[0].l;
    d.initial_state = initial_state.empty() ? nullptr : initial_state[0].l;
    return d;
  }
  // amdzk_poseidon_check_desc: every validation, without a device
  void check() const {
    const amdzk_poseidon_desc d = desc();
    char msg[256] = "";
    const int rc = amdzk_poseidon_check_desc(&d, msg, sizeof(msg));
    if (rc != AMDZK_OK) throw Error(rc, msg);
  }
};

class Poseidon {
 public:
  Poseidon(const Context& ctx, const PoseidonSpec& spec) : ctx_(ctx), t_(spec.t) {
    const amdzk_poseidon_desc d = spec.desc();
    ctx_.check(amdzk_poseidon_compile(ctx_.get(), &d, &h_));
  }
  ~Poseidon() {
    if (h_) amdzk_poseidon_free(ctx_.get(), h_);
  }
  Poseidon(const Poseidon&) = delete;
  Poseidon& operator=(const Poseidon&) = delete;

  void update(const std::vector<Fr>& elements) { buf_.insert(buf_.end(), elements.begin(), elements.end()); }
  // the digest of everything updated so far; the sponge starts afresh
  Fr squeeze() {
    const Fr out = hash_many({buf_})[0];
    buf_.clear();
    return out;
  }
  std::vector<Fr> hash_many(const std::vector<std::vector<Fr>>& inputs) const {
    std::vector<const uint64_t*> in(inputs.size());
    std::vector<size_t> lens(inputs.size());
    for (size_t b = 0; b < inputs.size(); b++) {
      in[b] = inputs[b].empty() ? nullptr : inputs[b][0].l;
      lens[b] = inputs[b].size();
    }
    std::vector<Fr> out(inputs.size());
    ctx_.check(amdzk_poseidon_hash(ctx_.get(), h_, in.data(), lens.data(), inputs.size(), out.empty() ? nullptr : out[0].l));
    return out;
  }
  // the inputs resident (amdzk_poseidon_hash_dev): lens empty = every sponge has `len` inputs
  void hash_many_dev(const void* d_inputs, size_t input_stride, const std::vector<size_t>& lens, size_t len, size_t n, void* d_out, size_t out_stride = 1) const {
    if (!lens.empty() && lens.size() != n) throw Error(AMDZK_E_INVALID, "poseidon: one length per sponge");
    ctx_.check(amdzk_poseidon_hash_dev(ctx_.get(), h_, d_inputs, input_stride, lens.empty() ? nullptr : lens.data(), len, n, d_out, out_stride));
  }
  // n_states resident states of t elements permuted in place (state_stride 0 = t)
  void permute_dev(void* d_states, size_t n_states, size_t state_stride = 0) const {
    ctx_.check(amdzk_poseidon_permute_dev(ctx_.get(), h_, d_states, n_states, state_stride ? state_stride : t_));
  }
  amdzk_poseidon* get() const { return h_; }

 private:
  const Context& ctx_;
  uint32_t t_;
  std::vector<Fr> buf_;
  amdzk_poseidon* h_ = nullptr;
};

// ------------------------------------------------------------------------------------------ verify_proof up to the pairing
// plonk::verify_proof [UP] without its last step (amdzk_verify_proofs): what upstream's verifier hands to its strategy as a
// GuardKZG. Every well-formed proof that went in is valid iff e(lhs, [s]_2) = e(rhs, [1]_2) — ONE pairing check, which stays
// with the caller (params.s_g2() and halo2curves' pairing on the Rust side). (0, 0) is the identity.
struct ProofStatus {
  enum Status : uint32_t {
    WellFormed = AMDZK_PROOF_WELL_FORMED, BadLength = AMDZK_PROOF_BAD_LENGTH, BadPoint = AMDZK_PROOF_BAD_POINT,
    BadScalar = AMDZK_PROOF_BAD_SCALAR, BadInstance = AMDZK_PROOF_BAD_INSTANCE, BadTranscript = AMDZK_PROOF_BAD_TRANSCRIPT
  };
  Status status;
  // byte offset of the first offending element (BadPoint, BadScalar; its index in read order for a proof read through a
  // TranscriptRead), the column (BadInstance), the read_* calls completed (BadTranscript), else 0
  uint32_t offset;
};
struct Guard {
  G1Affine lhs, rhs;
  std::vector<ProofStatus> statuses;  // one per proof; malformed proofs are in neither sum
  bool well_formed() const {
    for (const ProofStatus& s : statuses)
      if (s.status != ProofStatus::WellFormed) return false;
    return true;
  }
};

// The arguments amdzk_verify_proofs and amdzk_verify_proofs_decide share, built from the mirrors' containers (which must
// outlive it).
struct VerifyArgs {
  size_t B = 0, N = 1;
  detail::InstanceTables inst;  // one entry per (proof, circuit instance), proof after proof
  std::vector<const uint8_t*> pp;
  std::vector<size_t> pl;
  amdzk_verify_opts opts = {};
  std::vector<amdzk_proof_status> raw;
  VerifyArgs(const char* who, const std::vector<std::vector<std::vector<std::vector<Fr>>>>& instances, const std::vector<std::vector<uint8_t>>& proofs,
             Transcript transcript, Multiopen multiopen, uint64_t combine_seed, const std::vector<Fr>& combine_scalars) {
    const std::string w(who);
    B = proofs.size();
    if (instances.size() != B) throw Error(AMDZK_E_INVALID, w + ": one instance list per proof");
    if (!combine_scalars.empty() && combine_scalars.size() != B) throw Error(AMDZK_E_INVALID, w + ": one weight per proof");
    N = B ? instances[0].size() : 1;
    for (size_t b = 0; b < B; b++) {
      if (instances[b].size() != N || N == 0) throw Error(AMDZK_E_INVALID, w + ": every proof has the same number of circuit instances");
      for (size_t c = 0; c < N; c++) inst.add(instances[b][c]);
    }
    inst.finish();
    static const uint8_t none = 0;
    pp.assign(std::max<size_t>(1, B), nullptr);
    pl.assign(std::max<size_t>(1, B), 0);
    for (size_t b = 0; b < B; b++) pp[b] = proofs[b].empty() ? &none : proofs[b].data(), pl[b] = proofs[b].size();
    opts.size = sizeof(opts);
    opts.transcript_kind = (int)transcript | (int)multiopen;
    opts.n_circuits = (uint32_t)N;
    opts.combine_seed = combine_seed;
    opts.combine_scalars = combine_scalars.empty() ? nullptr : (const uint64_t*)combine_scalars.data();
    raw.resize(std::max<size_t>(1, B));
  }
  std::vector<ProofStatus> statuses() const {
    std::vector<ProofStatus> out;
    for (size_t b = 0; b < B; b++) out.push_back(ProofStatus{(ProofStatus::Status)raw[b].status, raw[b].offset});
    return out;
  }
};

// AccumulatorStrategy / BatchVerifier: one call per batch. instances[b][c][col]: the public inputs of circuit instance c of
// proof b (n_circuits instances per proof, as create_proof_multi wrote them). combine_scalars: one weight per proof, or
// empty to draw them from combine_seed — which must then be unpredictable to whoever made the proofs (seed it from the OS).
// After a failed pairing, call again on subsets to find the culprit.
// Every function below takes the key as a ProvingKey or as a VerifyingKey (further down): the C entry points differ in the
// key's type alone.
namespace detail {
inline int c_verify(amdzk_ctx* c, const amdzk_pk* key, VerifyArgs& a, uint64_t pair[16]) {
  return amdzk_verify_proofs(c, key, a.B, a.inst.pp.data(), a.inst.lp.data(), a.pp.data(), a.pl.data(), &a.opts, a.raw.data(), pair);
}
inline int c_verify(amdzk_ctx* c, const amdzk_vk* key, VerifyArgs& a, uint64_t pair[16]) {
  return amdzk_verify_proofs_vk(c, key, a.B, a.inst.pp.data(), a.inst.lp.data(), a.pp.data(), a.pl.data(), &a.opts, a.raw.data(), pair);
}
template <class Key>
Guard verify_proofs(const Context& ctx, const Key& key, const std::vector<std::vector<std::vector<std::vector<Fr>>>>& instances,
                    const std::vector<std::vector<uint8_t>>& proofs, Transcript transcript, Multiopen multiopen, uint64_t combine_seed,
                    const std::vector<Fr>& combine_scalars) {
  VerifyArgs a("verify_proofs", instances, proofs, transcript, multiopen, combine_seed, combine_scalars);
  uint64_t pair[16];
  ctx.check(c_verify(ctx.get(), key.handle(), a, pair));
  Guard g;
  std::memcpy(&g.lhs, pair, sizeof(G1Affine));
  std::memcpy(&g.rhs, pair + 8, sizeof(G1Affine));
  g.statuses = a.statuses();
  return g;
}
template <class Key>
Guard verify_proof(const Context& ctx, const Key& key, const std::vector<std::vector<Fr>>& instances, const std::vector<uint8_t>& proof,
                   Transcript transcript, Multiopen multiopen) {
  Guard g = detail::verify_proofs(ctx, key, {{instances}}, {proof}, transcript, multiopen, 0, {});
  if (!g.well_formed())
    throw Error(AMDZK_E_INVALID, "verify_proof: malformed proof, status " + std::to_string((unsigned)g.statuses[0].status) + ", offset " +
                                     std::to_string(g.statuses[0].offset));
  return g;
}
}  // namespace detail
inline Guard verify_proofs(const Context& ctx, const ProvingKey& pk, const std::vector<std::vector<std::vector<std::vector<Fr>>>>& instances,
                           const std::vector<std::vector<uint8_t>>& proofs, Transcript transcript = Transcript::Blake2b,
                           Multiopen multiopen = Multiopen::Shplonk, uint64_t combine_seed = 0, const std::vector<Fr>& combine_scalars = {}) {
  return detail::verify_proofs(ctx, pk, instances, proofs, transcript, multiopen, combine_seed, combine_scalars);
}

// SingleStrategy: one proof (weight 1), one call, one pairing. A malformed proof throws, naming status and offset.
inline Guard verify_proof(const Context& ctx, const ProvingKey& pk, const std::vector<std::vector<Fr>>& instances, const std::vector<uint8_t>& proof,
                          Transcript transcript = Transcript::Blake2b, Multiopen multiopen = Multiopen::Shplonk) {
  return detail::verify_proof(ctx, pk, instances, proof, transcript, multiopen);
}

// ------------------------------------------------------------------------------------------ verify_proof WITH the pairing
// The G2 side (include/amdzk.h "pairing"; conventions: csrc/fq12.cuh). G2Affine is halo2curves' {x.c0, x.c1, y.c0, y.c1},
// Montgomery; all zero is the identity.
struct G2Affine {
  uint64_t w[16];
  // halo2curves' G2Compressed, the g2 / s_g2 fields of the ParamsKZG file (amdzk_g2_compress / amdzk_g2_decompress): host only
  std::array<uint8_t, 64> to_bytes() const {
    std::array<uint8_t, 64> out;
    char msg[256];
    const int rc = amdzk_g2_compress(w, out.data(), msg, sizeof(msg));
    if (rc != AMDZK_OK) throw Error(rc, msg);
    return out;
  }
  static G2Affine from_bytes(const uint8_t bytes[64]) {
    G2Affine q;
    char msg[256];
    const int rc = amdzk_g2_decompress(bytes, q.w, msg, sizeof(msg));
    if (rc != AMDZK_OK) throw Error(rc, msg);
    return q;
  }
  // amdzk_g2_check: 0 in G2 | 1 a coordinate >= q | 2 not on the twist | 3 the identity | 4 outside the order-r subgroup
  int check() const {
    int status = -1;
    if (amdzk_g2_check(w, &status) != AMDZK_OK) throw Error(AMDZK_E_INVALID, "g2_check: null argument");
    return status;
  }
  bool is_on_curve_and_in_subgroup() const { return check() == 0; }
};
inline amdzk_srs_report ParamsKZG::check(const G2Affine& g2, const G2Affine& s_g2, const uint64_t* seed, const Fr* rho, uint32_t checks) const {
  amdzk_srs_check_opts opts;
  opts.size = sizeof(opts);
  opts.checks = checks;
  opts.rho = rho ? rho->l : nullptr;
  if (seed) {
    opts.seed = *seed;
  } else {
    std::random_device rd;
    opts.seed = ((uint64_t)rd() << 32) | (uint64_t)(uint32_t)rd();
  }
  amdzk_srs_report rep;
  ctx_.check(amdzk_srs_check(ctx_.get(), h_, g2.w, s_g2.w, &opts, &rep));
  return rep;
}
// halo2curves' G2Prepared: one finite point's line coefficients, resident on the device. Subgroup membership is not checked.
class G2Prepared {
 public:
  G2Prepared(const Context& ctx, const G2Affine& q) : ctx_(ctx) { ctx_.check(amdzk_g2_prepare(ctx_.get(), q.w, &h_)); }
  ~G2Prepared() {
    if (h_) amdzk_g2_free(ctx_.get(), h_);
  }
  G2Prepared(G2Prepared&& o) noexcept : ctx_(o.ctx_), h_(o.h_) { o.h_ = nullptr; }
  G2Prepared(const G2Prepared&) = delete;
  G2Prepared& operator=(const G2Prepared&) = delete;
  const amdzk_g2* handle() const { return h_; }

 private:
  const Context& ctx_;
  amdzk_g2* h_ = nullptr;
};
// The verifier's part of ParamsKZG: the prepared [1]_2 and [s]_2.
struct ParamsVerifierKZG {
  G2Prepared g2, s_g2;
  ParamsVerifierKZG(const Context& ctx, const G2Affine& g2_, const G2Affine& s_g2_) : g2(ctx, g2_), s_g2(ctx, s_g2_) {}
  // from the two 64-byte fields of a ParamsKZG file (ParamsKZG::read): both decompressed, and both must be in G2 — the zero
  // fields of a file written without G2 points are refused as the identity
  ParamsVerifierKZG(const Context& ctx, const uint8_t g2_bytes[64], const uint8_t s_g2_bytes[64])
      : ParamsVerifierKZG(ctx, member(g2_bytes, "g2"), member(s_g2_bytes, "s_g2")) {}
  static G2Affine member(const uint8_t bytes[64], const char* name) {
    static const char* const why[5] = {"in G2", "a coordinate is not below the modulus", "not on the twist", "the identity",
                                       "on the twist, outside the order-r subgroup"};
    const G2Affine q = G2Affine::from_bytes(bytes);
    const int st = q.check();
    if (st != 0) throw Error(AMDZK_E_INVALID, std::string("ParamsVerifierKZG: ") + name + " is " + why[st >= 0 && st < 5 ? st : 1]);
    return q;
  }
  // the G2 half of ParamsKZG::setup with the trapdoor given explicitly (tests / benchmarks, as unsafe as ParamsKZG::setup)
  static ParamsVerifierKZG setup(const Context& ctx, const Fr& s) {
    G2Affine g, sg;
    ctx.check(amdzk_g2_setup(ctx.get(), s.l, g.w, sg.w));
    return ParamsVerifierKZG(ctx, g, sg);
  }
};
struct Decision {
  std::vector<bool> verdicts;         // one per proof; a malformed proof is false
  std::vector<ProofStatus> statuses;  // as verify_proofs'
  size_t n_valid = 0;
};
// amdzk_verify_proofs_decide. combined = false: every proof by itself (SingleStrategy; deterministic, the weights are not
// read). combined = true: upstream's BatchVerifier — ONE check with the weights of combine_seed / combine_scalars, which must
// be unpredictable to whoever made the proofs; every well-formed proof gets that check's result.
namespace detail {
inline int c_decide(amdzk_ctx* c, const amdzk_pk* key, const ParamsVerifierKZG& vp, uint32_t flags, VerifyArgs& a, uint8_t* v, size_t* n_valid) {
  return amdzk_verify_proofs_decide(c, key, vp.s_g2.handle(), vp.g2.handle(), flags, a.B, a.inst.pp.data(), a.inst.lp.data(), a.pp.data(), a.pl.data(),
                                    &a.opts, a.raw.data(), v, n_valid);
}
inline int c_decide(amdzk_ctx* c, const amdzk_vk* key, const ParamsVerifierKZG& vp, uint32_t flags, VerifyArgs& a, uint8_t* v, size_t* n_valid) {
  return amdzk_verify_proofs_decide_vk(c, key, vp.s_g2.handle(), vp.g2.handle(), flags, a.B, a.inst.pp.data(), a.inst.lp.data(), a.pp.data(),
                                       a.pl.data(), &a.opts, a.raw.data(), v, n_valid);
}
template <class Key>
Decision decide_proofs(const Context& ctx, const Key& key, const ParamsVerifierKZG& vparams,
                       const std::vector<std::vector<std::vector<std::vector<Fr>>>>& instances, const std::vector<std::vector<uint8_t>>& proofs,
                       Transcript transcript, Multiopen multiopen, bool combined, uint64_t combine_seed, const std::vector<Fr>& combine_scalars) {
  VerifyArgs a("decide_proofs", instances, proofs, transcript, multiopen, combine_seed, combine_scalars);
  std::vector<uint8_t> v(std::max<size_t>(1, a.B), 0);
  Decision d;
  ctx.check(c_decide(ctx.get(), key.handle(), vparams, combined ? AMDZK_DECIDE_COMBINED : 0u, a, v.data(), &d.n_valid));
  for (size_t b = 0; b < a.B; b++) d.verdicts.push_back(v[b] != 0);
  d.statuses = a.statuses();
  return d;
}
template <class Key>
bool decide_proof(const Context& ctx, const Key& key, const ParamsVerifierKZG& vparams, const std::vector<std::vector<Fr>>& instances,
                  const std::vector<uint8_t>& proof, Transcript transcript, Multiopen multiopen) {
  const Decision d = detail::decide_proofs(ctx, key, vparams, {{instances}}, {proof}, transcript, multiopen, false, 0, {});
  if (d.statuses[0].status != ProofStatus::WellFormed)
    throw Error(AMDZK_E_INVALID, "decide_proof: malformed proof, status " + std::to_string((unsigned)d.statuses[0].status) + ", offset " +
                                     std::to_string(d.statuses[0].offset));
  return d.verdicts[0];
}
}  // namespace detail
inline Decision decide_proofs(const Context& ctx, const ProvingKey& pk, const ParamsVerifierKZG& vparams,
                              const std::vector<std::vector<std::vector<std::vector<Fr>>>>& instances, const std::vector<std::vector<uint8_t>>& proofs,
                              Transcript transcript = Transcript::Blake2b, Multiopen multiopen = Multiopen::Shplonk, bool combined = false,
                              uint64_t combine_seed = 0, const std::vector<Fr>& combine_scalars = {}) {
  return detail::decide_proofs(ctx, pk, vparams, instances, proofs, transcript, multiopen, combined, combine_seed, combine_scalars);
}
// plonk::verify_proof(params, vk, SingleStrategy, ...).is_ok(). A malformed proof throws, naming status and offset.
inline bool decide_proof(const Context& ctx, const ProvingKey& pk, const ParamsVerifierKZG& vparams, const std::vector<std::vector<Fr>>& instances,
                         const std::vector<uint8_t>& proof, Transcript transcript = Transcript::Blake2b, Multiopen multiopen = Multiopen::Shplonk) {
  return detail::decide_proof(ctx, pk, vparams, instances, proof, transcript, multiopen);
}

// ------------------------------------------------------------------------------------------ the verifying key
// plonk::VerifyingKey with the G of its params (amdzk_vk): all the verifier reads of a key. Host data only; it refers to no
// ParamsKZG and no ProvingKey, so a verifier process holds a Context, this and a ParamsVerifierKZG — which read() can give it.
class VerifyingKey {
 public:
  // plonk::keygen_vk (amdzk_keygen_vk): the key alone, without making a proving key — the fixed columns and the Assembly
  // as for ProvingKey; the device holds the F + S Lagrange columns while the call runs and nothing afterwards.
  static std::unique_ptr<VerifyingKey> keygen_vk(const Context& ctx, const ParamsKZG& params, const ConstraintSystem& cs,
                                                 const std::vector<std::vector<Fr>>& fixed, const Assembly& assembly, const Fr& transcript_repr) {
    const size_t n = (size_t)1 << params.k(), np = cs.permutation_columns.size();
    if (fixed.size() != cs.num_fixed) throw Error(AMDZK_E_INVALID, "keygen_vk: fixed column count");
    if (assembly.n() != n || assembly.num_columns() != np) throw Error(AMDZK_E_INVALID, "keygen_vk: assembly shape");
    std::vector<Fr> flat(fixed.size() * n, Fr::zero());
    for (size_t c = 0; c < fixed.size(); c++) {
      if (fixed[c].size() > n) throw Error(AMDZK_E_INVALID, "keygen_vk: fixed column longer than 2^k");
      std::copy(fixed[c].begin(), fixed[c].end(), flat.begin() + c * n);
    }
    CircuitData cd(cs, params.k());
    std::unique_ptr<VerifyingKey> vk(new VerifyingKey(ctx, cs.num_fixed, np));
    ctx.check(amdzk_keygen_vk(ctx.get(), params.handle(), &cd.c, cd.phased ? &cd.phases : nullptr, flat.empty() ? nullptr : (const uint64_t*)flat.data(),
                              np ? assembly.mapping() : nullptr, nullptr, transcript_repr.l, &vk->h_));
    return vk;
  }
  // ... from the sigma columns (one vector of 2^k per permutation column), as ProvingKey::from_sigma
  static std::unique_ptr<VerifyingKey> keygen_vk_sigma(const Context& ctx, const ParamsKZG& params, const ConstraintSystem& cs,
                                                       const std::vector<std::vector<Fr>>& fixed, const std::vector<std::vector<Fr>>& sigma,
                                                       const Fr& transcript_repr) {
    const size_t n = (size_t)1 << params.k();
    if (fixed.size() != cs.num_fixed || sigma.size() != cs.permutation_columns.size()) throw Error(AMDZK_E_INVALID, "keygen_vk: column count");
    auto flatten = [n](const std::vector<std::vector<Fr>>& cols) {
      std::vector<Fr> flat(cols.size() * n, Fr::zero());
      for (size_t c = 0; c < cols.size(); c++) {
        if (cols[c].size() > n) throw Error(AMDZK_E_INVALID, "keygen_vk: column longer than 2^k");
        std::copy(cols[c].begin(), cols[c].end(), flat.begin() + c * n);
      }
      return flat;
    };
    const std::vector<Fr> fx = flatten(fixed), sg = flatten(sigma);
    CircuitData cd(cs, params.k());
    std::unique_ptr<VerifyingKey> vk(new VerifyingKey(ctx, fixed.size(), sigma.size()));
    ctx.check(amdzk_keygen_vk(ctx.get(), params.handle(), &cd.c, cd.phased ? &cd.phases : nullptr, fx.empty() ? nullptr : (const uint64_t*)fx.data(), nullptr,
                              sg.empty() ? nullptr : (const uint64_t*)sg.data(), transcript_repr.l, &vk->h_));
    return vk;
  }
  // The key file (include/amdzk.h has the layout). With g2 and s_g2 (both or neither) the file carries the SRS's [1]_2 and
  // [s]_2 too and is all a verifier needs.
  std::vector<uint8_t> write(const G2Affine* g2 = nullptr, const G2Affine* s_g2 = nullptr) const {
    std::vector<uint8_t> out(amdzk_vk_serialized_size(h_, g2 ? 1 : 0));
    size_t written = 0;
    ctx_.check(amdzk_vk_write(ctx_.get(), h_, g2 ? g2->w : nullptr, s_g2 ? s_g2->w : nullptr, out.data(), out.size(), &written));
    out.resize(written);
    return out;
  }
  // The key of a file write() made (amdzk_vk_read); needs no ParamsKZG. A damaged, truncated or inconsistent file is refused
  // with a message that starts "vk_read:". *has_g2 (may be null) says whether g2 / s_g2 (may be null) were in the file.
  static std::unique_ptr<VerifyingKey> read(const Context& ctx, const std::vector<uint8_t>& data, G2Affine* g2 = nullptr, G2Affine* s_g2 = nullptr,
                                            bool* has_g2 = nullptr) {
    std::unique_ptr<VerifyingKey> vk(new VerifyingKey(ctx, 0, 0));
    int has = 0;
    ctx.check(amdzk_vk_read(ctx.get(), data.data(), data.size(), &vk->h_, g2 ? g2->w : nullptr, s_g2 ? s_g2->w : nullptr, &has));
    uint32_t nf = 0, np = 0;
    ctx.check(amdzk_vk_blob_info(data.data(), data.size(), nullptr, &nf, nullptr, &np, nullptr, nullptr));
    vk->num_fixed_ = nf, vk->num_perm_ = np;
    if (has_g2) *has_g2 = has != 0;
    return vk;
  }
  ~VerifyingKey() {
    if (h_) amdzk_vk_free(ctx_.get(), h_);
  }
  VerifyingKey(const VerifyingKey&) = delete;
  VerifyingKey& operator=(const VerifyingKey&) = delete;
  // VerifyingKey::{fixed_commitments, permutation.commitments}
  void commitments(std::vector<G1Affine>& fixed, std::vector<G1Affine>& permutation) const {
    fixed.assign(num_fixed_, G1Affine{});
    permutation.assign(num_perm_, G1Affine{});
    ctx_.check(amdzk_vk_commitments(h_, num_fixed_ ? (uint64_t*)fixed.data() : nullptr, num_perm_ ? (uint64_t*)permutation.data() : nullptr));
  }
  size_t proof_size(size_t n_circuits = 1, Transcript transcript = Transcript::Blake2b, Multiopen multiopen = Multiopen::Shplonk) const {
    return amdzk_vk_proof_size_multi(h_, n_circuits, (int)transcript | (int)multiopen);
  }
  const amdzk_vk* handle() const { return h_; }

 private:
  friend class ProvingKey;
  VerifyingKey(const Context& ctx, size_t nf, size_t np) : ctx_(ctx), num_fixed_(nf), num_perm_(np) {}
  const Context& ctx_;
  size_t num_fixed_, num_perm_;
  amdzk_vk* h_ = nullptr;
};
inline std::unique_ptr<VerifyingKey> ProvingKey::get_vk() const {
  std::unique_ptr<VerifyingKey> vk(new VerifyingKey(ctx_, num_fixed_, num_perm_));
  ctx_.check(amdzk_vk_from_pk(ctx_.get(), h_, &vk->h_));
  return vk;
}
inline std::unique_ptr<VerifyingKey> keygen_vk(const Context& ctx, const ParamsKZG& params, const ConstraintSystem& cs,
                                               const std::vector<std::vector<Fr>>& fixed, const Assembly& assembly, const Fr& transcript_repr) {
  return VerifyingKey::keygen_vk(ctx, params, cs, fixed, assembly, transcript_repr);
}
// The verifier's calls over a VerifyingKey: the contracts above, word for word.
inline Guard verify_proofs(const Context& ctx, const VerifyingKey& vk, const std::vector<std::vector<std::vector<std::vector<Fr>>>>& instances,
                           const std::vector<std::vector<uint8_t>>& proofs, Transcript transcript = Transcript::Blake2b,
                           Multiopen multiopen = Multiopen::Shplonk, uint64_t combine_seed = 0, const std::vector<Fr>& combine_scalars = {}) {
  return detail::verify_proofs(ctx, vk, instances, proofs, transcript, multiopen, combine_seed, combine_scalars);
}
inline Guard verify_proof(const Context& ctx, const VerifyingKey& vk, const std::vector<std::vector<Fr>>& instances, const std::vector<uint8_t>& proof,
                          Transcript transcript = Transcript::Blake2b, Multiopen multiopen = Multiopen::Shplonk) {
  return detail::verify_proof(ctx, vk, instances, proof, transcript, multiopen);
}
inline Decision decide_proofs(const Context& ctx, const VerifyingKey& vk, const ParamsVerifierKZG& vparams,
                              const std::vector<std::vector<std::vector<std::vector<Fr>>>>& instances, const std::vector<std::vector<uint8_t>>& proofs,
                              Transcript transcript = Transcript::Blake2b, Multiopen multiopen = Multiopen::Shplonk, bool combined = false,
                              uint64_t combine_seed = 0, const std::vector<Fr>& combine_scalars = {}) {
  return detail::decide_proofs(ctx, vk, vparams, instances, proofs, transcript, multiopen, combined, combine_seed, combine_scalars);
}
inline bool decide_proof(const Context& ctx, const VerifyingKey& vk, const ParamsVerifierKZG& vparams, const std::vector<std::vector<Fr>>& instances,
                         const std::vector<uint8_t>& proof, Transcript transcript = Transcript::Blake2b, Multiopen multiopen = Multiopen::Shplonk) {
  return detail::decide_proof(ctx, vk, vparams, instances, proof, transcript, multiopen);
}

// ------------------------------------------------------------------------------------------ the caller's read transcript
// transcript::TranscriptRead as far as verify_proof uses it: implement it to own the transcript (`&mut T: TranscriptRead`
// upstream; amdzk_transcript_read). Values are Montgomery. The library keeps no hash of its own for such a proof and uses the
// challenges squeeze_challenge returns; what read_point / read_scalar return is checked on the device like a proof's bytes.
// A member that throws makes its proof ProofStatus::BadTranscript; the single-proof calls rethrow the exception.
class TranscriptRead {
 public:
  virtual ~TranscriptRead() {}
  virtual void common_point(const G1Affine& p) = 0;
  virtual void common_scalar(const Fr& s) = 0;
  virtual G1Affine read_point() = 0;
  virtual Fr read_scalar() = 0;
  virtual Fr squeeze_challenge() = 0;
};

namespace detail {
struct ReadTrampoline {
  TranscriptRead* t;
  std::exception_ptr err;
  template <class F>
  int guard(F&& f) {
    try {
      f();
      return 0;
    } catch (...) {
      if (!err) err = std::current_exception();
      return 1;
    }
  }
};
inline amdzk_transcript_read c_transcript_read(ReadTrampoline* tr) {
  amdzk_transcript_read ct;
  ct.user = tr;
  ct.common_point = [](void* u, const uint64_t* xy) { auto* t = (ReadTrampoline*)u; return t->guard([&] { G1Affine p; std::memcpy(&p, xy, 64); t->t->common_point(p); }); };
  ct.common_scalar = [](void* u, const uint64_t* s) { auto* t = (ReadTrampoline*)u; return t->guard([&] { Fr v; std::memcpy(v.l, s, 32); t->t->common_scalar(v); }); };
  ct.read_point = [](void* u, uint64_t* out) { auto* t = (ReadTrampoline*)u; return t->guard([&] { const G1Affine p = t->t->read_point(); std::memcpy(out, &p, 64); }); };
  ct.read_scalar = [](void* u, uint64_t* out) { auto* t = (ReadTrampoline*)u; return t->guard([&] { const Fr v = t->t->read_scalar(); std::memcpy(out, v.l, 32); }); };
  ct.squeeze_challenge = [](void* u, uint64_t* out) { auto* t = (ReadTrampoline*)u; return t->guard([&] { const Fr v = t->t->squeeze_challenge(); std::memcpy(out, v.l, 32); }); };
  return ct;
}
// the C side of a batch of read transcripts; must outlive the call
struct ReadBatch {
  std::vector<ReadTrampoline> tramp;
  std::vector<amdzk_transcript_read> c;
  std::vector<const amdzk_transcript_read*> ptrs;
  explicit ReadBatch(const std::vector<TranscriptRead*>& ts) : tramp(ts.size()), c(ts.size()), ptrs(std::max<size_t>(1, ts.size()), nullptr) {
    for (size_t b = 0; b < ts.size(); b++) {
      if (!ts[b]) throw Error(AMDZK_E_INVALID, "verify_proofs: null transcript");
      tramp[b] = ReadTrampoline{ts[b], nullptr};
      c[b] = c_transcript_read(&tramp[b]);
      ptrs[b] = &c[b];
    }
  }
  void rethrow_first() const {
    for (const ReadTrampoline& t : tramp)
      if (t.err) std::rethrow_exception(t.err);
  }
};
template <class Key>
Guard verify_proofs_read(const Context& ctx, const Key& key, const std::vector<std::vector<std::vector<std::vector<Fr>>>>& instances,
                         const std::vector<TranscriptRead*>& transcripts, Multiopen multiopen, uint64_t combine_seed,
                         const std::vector<Fr>& combine_scalars, bool rethrow) {
  ReadBatch rb(transcripts);
  VerifyArgs a("verify_proofs", instances, std::vector<std::vector<uint8_t>>(transcripts.size()), Transcript::Blake2b, multiopen, combine_seed, combine_scalars);
  a.opts.transcripts = rb.ptrs.data();
  uint64_t pair[16];
  const int rc = c_verify(ctx.get(), key.handle(), a, pair);
  if (rethrow) rb.rethrow_first();
  ctx.check(rc);
  Guard g;
  std::memcpy(&g.lhs, pair, sizeof(G1Affine));
  std::memcpy(&g.rhs, pair + 8, sizeof(G1Affine));
  g.statuses = a.statuses();
  return g;
}
template <class Key>
Decision decide_proofs_read(const Context& ctx, const Key& key, const ParamsVerifierKZG& vparams,
                            const std::vector<std::vector<std::vector<std::vector<Fr>>>>& instances, const std::vector<TranscriptRead*>& transcripts,
                            Multiopen multiopen, bool combined, uint64_t combine_seed, const std::vector<Fr>& combine_scalars, bool rethrow) {
  ReadBatch rb(transcripts);
  VerifyArgs a("decide_proofs", instances, std::vector<std::vector<uint8_t>>(transcripts.size()), Transcript::Blake2b, multiopen, combine_seed, combine_scalars);
  a.opts.transcripts = rb.ptrs.data();
  std::vector<uint8_t> v(std::max<size_t>(1, a.B), 0);
  Decision d;
  const int rc = c_decide(ctx.get(), key.handle(), vparams, combined ? AMDZK_DECIDE_COMBINED : 0u, a, v.data(), &d.n_valid);
  if (rethrow) rb.rethrow_first();
  ctx.check(rc);
  for (size_t b = 0; b < a.B; b++) d.verdicts.push_back(v[b] != 0);
  d.statuses = a.statuses();
  return d;
}
inline void throw_malformed(const char* who, const ProofStatus& s) {
  if (s.status != ProofStatus::WellFormed)
    throw Error(AMDZK_E_INVALID, std::string(who) + ": malformed proof, status " + std::to_string((unsigned)s.status) + ", offset " + std::to_string(s.offset));
}
}  // namespace detail

// verify_proofs / verify_proof / decide_proofs / decide_proof generic over `T: TranscriptRead`: one transcript per proof in
// the place of the bytes (Key = ProvingKey or VerifyingKey). Of the built-in kinds only `multiopen` remains to be named.
template <class Key>
Guard verify_proofs(const Context& ctx, const Key& key, const std::vector<std::vector<std::vector<std::vector<Fr>>>>& instances,
                    const std::vector<TranscriptRead*>& transcripts, Multiopen multiopen = Multiopen::Shplonk, uint64_t combine_seed = 0,
                    const std::vector<Fr>& combine_scalars = {}) {
  return detail::verify_proofs_read(ctx, key, instances, transcripts, multiopen, combine_seed, combine_scalars, false);
}
template <class Key>
Guard verify_proof(const Context& ctx, const Key& key, const std::vector<std::vector<Fr>>& instances, TranscriptRead& transcript,
                   Multiopen multiopen = Multiopen::Shplonk) {
  Guard g = detail::verify_proofs_read(ctx, key, {{instances}}, {&transcript}, multiopen, 0, {}, true);
  detail::throw_malformed("verify_proof", g.statuses[0]);
  return g;
}
template <class Key>
Decision decide_proofs(const Context& ctx, const Key& key, const ParamsVerifierKZG& vparams,
                       const std::vector<std::vector<std::vector<std::vector<Fr>>>>& instances, const std::vector<TranscriptRead*>& transcripts,
                       Multiopen multiopen = Multiopen::Shplonk, bool combined = false, uint64_t combine_seed = 0,
                       const std::vector<Fr>& combine_scalars = {}) {
  return detail::decide_proofs_read(ctx, key, vparams, instances, transcripts, multiopen, combined, combine_seed, combine_scalars, false);
}
template <class Key>
bool decide_proof(const Context& ctx, const Key& key, const ParamsVerifierKZG& vparams, const std::vector<std::vector<Fr>>& instances,
                  TranscriptRead& transcript, Multiopen multiopen = Multiopen::Shplonk) {
  const Decision d = detail::decide_proofs_read(ctx, key, vparams, {{instances}}, {&transcript}, multiopen, false, 0, {}, true);
  detail::throw_malformed("decide_proof", d.statuses[0]);
  return d.verdicts[0];
}

// ------------------------------------------------------------------------------------------ proofs of different circuits
// One member of a batch over DIFFERENT keys (amdzk_verify_item): the key — a ProvingKey or a VerifyingKey —, the proof's
// public inputs instances[c][col] (as many circuit instances as the proof was made with), the proof's bytes and their kinds;
// or `reader`, the caller's TranscriptRead, in the bytes' place (of the kinds only `multiopen` then counts). All keys of a
// batch were made over the same G: one setup, any k (ParamsKZG::downsize), keys from files included. Everything an item
// points to must outlive the call.
struct VerifyItem {
  const ProvingKey* pk = nullptr;
  const VerifyingKey* vk = nullptr;
  const std::vector<std::vector<std::vector<Fr>>>* instances = nullptr;
  const std::vector<uint8_t>* proof = nullptr;
  Transcript transcript = Transcript::Blake2b;
  Multiopen multiopen = Multiopen::Shplonk;
  TranscriptRead* reader = nullptr;
  VerifyItem(const ProvingKey& key, const std::vector<std::vector<std::vector<Fr>>>& inst, const std::vector<uint8_t>& bytes,
             Transcript t = Transcript::Blake2b, Multiopen m = Multiopen::Shplonk)
      : pk(&key), instances(&inst), proof(&bytes), transcript(t), multiopen(m) {}
  VerifyItem(const VerifyingKey& key, const std::vector<std::vector<std::vector<Fr>>>& inst, const std::vector<uint8_t>& bytes,
             Transcript t = Transcript::Blake2b, Multiopen m = Multiopen::Shplonk)
      : vk(&key), instances(&inst), proof(&bytes), transcript(t), multiopen(m) {}
  VerifyItem(const ProvingKey& key, const std::vector<std::vector<std::vector<Fr>>>& inst, TranscriptRead& t, Multiopen m = Multiopen::Shplonk)
      : pk(&key), instances(&inst), multiopen(m), reader(&t) {}
  VerifyItem(const VerifyingKey& key, const std::vector<std::vector<std::vector<Fr>>>& inst, TranscriptRead& t, Multiopen m = Multiopen::Shplonk)
      : vk(&key), instances(&inst), multiopen(m), reader(&t) {}
};

namespace detail {
// the C side of a mixed batch; must outlive the call
struct MixedArgs {
  std::vector<std::vector<const uint64_t*>> ptrs;
  std::vector<std::vector<size_t>> lens;
  std::vector<std::vector<const uint64_t* const*>> inst_pp;
  std::vector<std::vector<const size_t*>> lens_pp;
  std::vector<ReadTrampoline> tramp;
  std::vector<amdzk_transcript_read> tr;
  std::vector<amdzk_verify_item> items;
  amdzk_verify_mixed_opts opts = {};
  std::vector<amdzk_proof_status> raw;
  MixedArgs(const char* who, const std::vector<VerifyItem>& in, uint64_t combine_seed, const std::vector<Fr>& combine_scalars)
      : inst_pp(in.size()), lens_pp(in.size()), tramp(in.size()), tr(in.size()), items(std::max<size_t>(1, in.size())), raw(std::max<size_t>(1, in.size())) {
    const std::string w(who);
    if (!combine_scalars.empty() && combine_scalars.size() != in.size()) throw Error(AMDZK_E_INVALID, w + ": one weight per item");
    static const uint8_t none = 0;
    size_t total = 0;
    for (const VerifyItem& it : in) total += it.instances ? it.instances->size() : 0;
    ptrs.reserve(total), lens.reserve(total);
    for (size_t b = 0; b < in.size(); b++) {
      const VerifyItem& it = in[b];
      if (!it.instances || it.instances->empty() || (!it.proof && !it.reader)) throw Error(AMDZK_E_INVALID, w + ": item " + std::to_string(b) + " is incomplete");
      for (const auto& cols : *it.instances) {
        ptrs.emplace_back(std::max<size_t>(1, cols.size()), nullptr);
        lens.emplace_back(std::max<size_t>(1, cols.size()), 0);
        for (size_t i = 0; i < cols.size(); i++) {
          ptrs.back()[i] = cols[i].empty() ? nullptr : (const uint64_t*)cols[i].data();
          lens.back()[i] = cols[i].size();
        }
        inst_pp[b].push_back(ptrs.back().data());
        lens_pp[b].push_back(lens.back().data());
      }
      amdzk_verify_item& c = items[b];
      c.pk = it.pk ? it.pk->handle() : nullptr;
      c.vk = it.vk ? it.vk->handle() : nullptr;
      c.transcript_kind = (int)it.transcript | (int)it.multiopen;
      c.n_circuits = (uint32_t)it.instances->size();
      c.instances = inst_pp[b].data();
      c.instance_lens = lens_pp[b].data();
      c.proof = it.proof && !it.proof->empty() ? it.proof->data() : &none;
      c.proof_len = it.proof ? it.proof->size() : 0;
      c.transcript = nullptr;
      if (it.reader) {
        tramp[b] = ReadTrampoline{it.reader, nullptr};
        tr[b] = c_transcript_read(&tramp[b]);
        c.transcript = &tr[b];
      }
    }
    opts.size = sizeof(opts);
    opts.combine_seed = combine_seed;
    opts.combine_scalars = combine_scalars.empty() ? nullptr : (const uint64_t*)combine_scalars.data();
  }
  std::vector<ProofStatus> statuses(size_t B) const {
    std::vector<ProofStatus> out;
    for (size_t b = 0; b < B; b++) out.push_back(ProofStatus{(ProofStatus::Status)raw[b].status, raw[b].offset});
    return out;
  }
};
}  // namespace detail

// verify_proofs over items that each bring their own key (amdzk_verify_proofs_mixed): guard = sum_b rho_b (L_b, R_b), and
// statuses[b] is what verify_proofs gives item b under its key. One decode launch and one MSM for the whole batch.
inline Guard verify_proofs(const Context& ctx, const std::vector<VerifyItem>& items, uint64_t combine_seed = 0, const std::vector<Fr>& combine_scalars = {}) {
  detail::MixedArgs a("verify_proofs", items, combine_seed, combine_scalars);
  uint64_t pair[16];
  ctx.check(amdzk_verify_proofs_mixed(ctx.get(), a.items.data(), items.size(), &a.opts, a.raw.data(), pair));
  Guard g;
  std::memcpy(&g.lhs, pair, sizeof(G1Affine));
  std::memcpy(&g.rhs, pair + 8, sizeof(G1Affine));
  g.statuses = a.statuses(items.size());
  return g;
}
// ... and decided (amdzk_verify_proofs_decide_mixed): one pairing launch for all items, per proof or (combined) one check.
inline Decision decide_proofs(const Context& ctx, const ParamsVerifierKZG& vparams, const std::vector<VerifyItem>& items, bool combined = false,
                              uint64_t combine_seed = 0, const std::vector<Fr>& combine_scalars = {}) {
  detail::MixedArgs a("decide_proofs", items, combine_seed, combine_scalars);
  std::vector<uint8_t> v(std::max<size_t>(1, items.size()), 0);
  Decision d;
  ctx.check(amdzk_verify_proofs_decide_mixed(ctx.get(), vparams.s_g2.handle(), vparams.g2.handle(), combined ? AMDZK_DECIDE_COMBINED : 0u, a.items.data(),
                                             items.size(), &a.opts, a.raw.data(), v.data(), &d.n_valid));
  for (size_t b = 0; b < items.size(); b++) d.verdicts.push_back(v[b] != 0);
  d.statuses = a.statuses(items.size());
  return d;
}

// ------------------------------------------------------------------------------------------ multiopen verified on its own
// poly::kzg::multiopen::{VerifierSHPLONK, VerifierGWC} over the caller's commitments (amdzk_multiopen_verify / _decide).
// poly::query::VerifierQuery with a plain commitment (upstream's CommitmentReference::MSM is not built): a commitment's
// identity is its words, equal point values are one point, `eval` is the evaluation the query claims.
struct VerifierQuery {
  G1Affine commitment;
  Fr point;
  Fr eval;
};
struct OpeningGuard {
  G1Affine lhs, rhs;  // valid iff e(lhs, [s]_2) = e(rhs, [1]_2); (0, 0) is the identity
};

namespace detail {
// verify_proof of poly::commitment::Verifier; vparams == nullptr: up to the pairing
inline bool multiopen_verify(const Context& ctx, const G1Affine& g, Multiopen scheme, TranscriptRead& transcript, const std::vector<VerifierQuery>& queries,
                             const ParamsVerifierKZG* vparams, OpeningGuard* guard) {
  std::vector<G1Affine> coms;
  std::vector<Fr> points, evals(queries.size());
  std::map<std::array<uint64_t, 8>, uint32_t> com_of;
  std::map<std::array<uint64_t, 4>, uint32_t> point_of;
  std::vector<amdzk_open_query> q(queries.size());
  for (size_t i = 0; i < queries.size(); i++) {
    std::array<uint64_t, 8> ck;
    std::memcpy(ck.data(), &queries[i].commitment, 64);
    auto ci = com_of.find(ck);
    if (ci == com_of.end()) {
      ci = com_of.emplace(ck, (uint32_t)coms.size()).first;
      coms.push_back(queries[i].commitment);
    }
    const std::array<uint64_t, 4> key{{queries[i].point.l[0], queries[i].point.l[1], queries[i].point.l[2], queries[i].point.l[3]}};
    auto zi = point_of.find(key);
    if (zi == point_of.end()) {
      zi = point_of.emplace(key, (uint32_t)points.size()).first;
      points.push_back(queries[i].point);
    }
    q[i].poly = ci->second;
    q[i].point = zi->second;
    evals[i] = queries[i].eval;
  }
  ReadTrampoline tr{&transcript, nullptr};
  const amdzk_transcript_read ct = c_transcript_read(&tr);
  amdzk_multiopen_verify_opts opts;
  std::memset(&opts, 0, sizeof(opts));
  opts.size = sizeof(opts);
  opts.scheme = (int)scheme;
  opts.transcript = &ct;
  uint64_t pair[16];
  uint8_t verdict = 0;
  const int rc = vparams ? amdzk_multiopen_decide(ctx.get(), (const uint64_t*)&g, (const uint64_t*)coms.data(), coms.size(), (const uint64_t*)points.data(),
                                                  points.size(), q.data(), (const uint64_t*)evals.data(), q.size(), &opts, vparams->s_g2.handle(),
                                                  vparams->g2.handle(), &verdict)
                         : amdzk_multiopen_verify(ctx.get(), (const uint64_t*)&g, (const uint64_t*)coms.data(), coms.size(), (const uint64_t*)points.data(),
                                                  points.size(), q.data(), (const uint64_t*)evals.data(), q.size(), &opts, pair);
  if (rc != AMDZK_OK && tr.err) std::rethrow_exception(tr.err);
  ctx.check(rc);
  if (guard && !vparams) {
    std::memcpy(&guard->lhs, pair, sizeof(G1Affine));
    std::memcpy(&guard->rhs, pair + 8, sizeof(G1Affine));
  }
  return verdict != 0;
}
}  // namespace detail

// g: the SRS's g[0] (ParamsKZG::get_g()[0], or a verifying key's). verify_proof leaves the pairing to the caller; decide
// makes it on the device.
class VerifierSHPLONK {
 public:
  VerifierSHPLONK(const Context& ctx, const G1Affine& g) : ctx_(ctx), g_(g) {}
  OpeningGuard verify_proof(TranscriptRead& transcript, const std::vector<VerifierQuery>& queries) const {
    OpeningGuard out;
    detail::multiopen_verify(ctx_, g_, Multiopen::Shplonk, transcript, queries, nullptr, &out);
    return out;
  }
  bool decide(TranscriptRead& transcript, const std::vector<VerifierQuery>& queries, const ParamsVerifierKZG& vparams) const {
    return detail::multiopen_verify(ctx_, g_, Multiopen::Shplonk, transcript, queries, &vparams, nullptr);
  }

 private:
  const Context& ctx_;
  G1Affine g_;
};

class VerifierGWC {
 public:
  VerifierGWC(const Context& ctx, const G1Affine& g) : ctx_(ctx), g_(g) {}
  OpeningGuard verify_proof(TranscriptRead& transcript, const std::vector<VerifierQuery>& queries) const {
    OpeningGuard out;
    detail::multiopen_verify(ctx_, g_, Multiopen::Gwc, transcript, queries, nullptr, &out);
    return out;
  }
  bool decide(TranscriptRead& transcript, const std::vector<VerifierQuery>& queries, const ParamsVerifierKZG& vparams) const {
    return detail::multiopen_verify(ctx_, g_, Multiopen::Gwc, transcript, queries, &vparams, nullptr);
  }

 private:
  const Context& ctx_;
  G1Affine g_;
};

}  // namespace halo2
}  // namespace amdzk
#endif /* AMDZK_HALO2_HPP */
