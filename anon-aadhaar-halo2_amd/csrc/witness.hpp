// Witness programs (include/amdzk.h "witness programs") — the host half: validation, levelization, the
// launch plan, and wit::eval_node, the ONE function that computes a node from its operands. It is ZK_HD over bn254.cuh's
// field, so that the kernels of witness.hip and a host loop (wit::host_run, tests/native/witness_check.cpp) run the same
// code. Nothing here touches the device: a plain host compiler builds this file.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/amdzk.h"
#include "bn254.cuh"

namespace wit {

using bn254::Fr;

constexpr uint32_t OP_COUNT = AMDZK_W_XOR + 1;
// A stretch of levels of at most FUSED_WIDTH (node, proof) items each runs in one launch of ONE workgroup of FUSED_WIDTH
// threads with a workgroup barrier between levels: 1024 is the largest workgroup, 16 waves = 4 per SIMD of the one compute
// unit it runs on, so a level is a single pass (one item per thread); a level that needed a second pass on one compute unit
// is better served by the whole chip, one kernel boundary away (measured, DESIGN.md §3.10: 1.4 us per fused level, for all the
// proofs of a run together). Wide levels: LEVEL_BLOCK = 256 threads, one wave per SIMD, as many blocks as the level needs.
constexpr uint32_t FUSED_WIDTH = 1024;
constexpr uint32_t LEVEL_BLOCK = 256;
constexpr size_t DEFAULT_SCRATCH = (size_t)16 << 30;
constexpr size_t SCRATCH_FIXED = 256;        // the status word, with room to keep what follows aligned
constexpr uint64_t MAX_ITEMS = 0x7fffffffu;  // (node, proof) items of one launch

// node operands that name nodes (the rest of a, b, c are immediates or unused)
ZK_HD uint32_t arity(uint32_t op) {
  switch (op) {
    case AMDZK_W_INPUT:
    case AMDZK_W_CONST: return 0;
    case AMDZK_W_NEG:
    case AMDZK_W_INV:
    case AMDZK_W_IS_ZERO:
    case AMDZK_W_BITS: return 1;
    case AMDZK_W_SELECT: return 3;
    default: return 2;
  }
}

// ---- integer ops on the 8 x 32-bit words of a canonical value
ZK_HD bool words_lt(const Fr& a, const Fr& b) {  // a < b as integers
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t t = (uint64_t)a.l[i] - b.l[i] - borrow;
    borrow = (uint32_t)(t >> 63);
  }
  return borrow == 1;
}
// (a >> lo) mod 2^len, lo + len <= 256, len >= 1: a barrel shifter over the words (no indexing by a run-time value, so the
// words stay in registers on the device), then the bits, then the mask.
ZK_HD Fr words_bits(const Fr& a, uint32_t lo, uint32_t len) {
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = a.l[i];
  const uint32_t ws = lo >> 5, bs = lo & 31;
#pragma unroll
  for (int s = 4; s >= 1; s >>= 1) {
    const bool on = (ws & s) != 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint32_t from = i + s < 8 ? w[i + s < 8 ? i + s : 7] : 0u;
      w[i] = on ? from : w[i];
    }
  }
  Fr r;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint32_t hi = i + 1 < 8 ? w[i + 1 < 8 ? i + 1 : 7] : 0u;
    const uint32_t v = bs ? (w[i] >> bs) | (hi << (32 - bs)) : w[i];
    const int rem = (int)len - 32 * i;  // bits of this word that are kept
    const uint32_t mask = rem <= 0 ? 0u : rem >= 32 ? 0xffffffffu : (1u << rem) - 1u;
    r.l[i] = v & mask;
  }
  return r;
}

// The value of a node. a, b, c: the values of the operand nodes (those beyond arity(op) are not read); for INPUT and CONST
// `a` is the input / the constant itself; imm_b, imm_c: the node's b and c fields (BITS: lo and len).
ZK_HD Fr eval_node(uint32_t op, uint32_t imm_b, uint32_t imm_c, const Fr& a, const Fr& b, const Fr& c) {
  using namespace bn254;
  switch (op) {
    case AMDZK_W_INPUT:
    case AMDZK_W_CONST: return a;
    case AMDZK_W_ADD: return add(a, b);
    case AMDZK_W_SUB: return sub(a, b);
    case AMDZK_W_MUL: return mul(a, b);
    case AMDZK_W_NEG: return neg(a);
    case AMDZK_W_INV: return inv(a);
    case AMDZK_W_SELECT: return a.is_zero() ? c : b;
    case AMDZK_W_IS_ZERO: return a.is_zero() ? Fr::one() : Fr::zero();
    case AMDZK_W_EQ: return a == b ? Fr::one() : Fr::zero();
    default: break;
  }
  // the integer ops: canonical words in, canonical words out
  const Fr ca = from_mont(a);
  Fr r;
  if (op == AMDZK_W_BITS) {
    r = words_bits(ca, imm_b, imm_c);  // <= canon(a) < r
  } else {
    const Fr cb = from_mont(b);
    if (op == AMDZK_W_LT) return words_lt(ca, cb) ? Fr::one() : Fr::zero();
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = op == AMDZK_W_AND ? (ca.l[i] & cb.l[i]) : (ca.l[i] ^ cb.l[i]);
    r = reduce_once(r);  // a ^ b < 2^254 < 2r
  }
  return to_mont(r);
}

// ---- the compiled program: nodes in level order ("slots"), every node reference rewritten to a slot
struct Node {
  uint32_t op, a, b, c;
};
struct Cell {
  uint32_t slot, column, row;
};
struct Program {
  uint32_t k = 0, num_advice = 0, n_inputs = 0;
  std::vector<Fr> consts;
  std::vector<Node> nodes;          // by slot
  std::vector<uint32_t> level_off;  // levels + 1 entries: level l is the slots [level_off[l], level_off[l + 1])
  std::vector<Cell> cells;          // sorted by (column, row)
  std::vector<uint32_t> publics;    // slots
  std::vector<uint32_t> slot_of;    // the caller's node index -> slot
  uint32_t levels() const { return level_off.empty() ? 0 : (uint32_t)level_off.size() - 1; }
  uint32_t widest() const {
    uint32_t w = 0;
    for (uint32_t l = 0; l < levels(); l++) w = std::max(w, level_off[l + 1] - level_off[l]);
    return w;
  }
};

inline int refuse(std::string& err, int code, const char* fmt, uint64_t x = 0, uint64_t y = 0, uint64_t z = 0) {
  char b[256];
  snprintf(b, sizeof(b), fmt, (unsigned long long)x, (unsigned long long)y, (unsigned long long)z);
  err = std::string("witness: ") + b;
  return code;
}

inline int build(const amdzk_witness_desc* d, Program& p, std::string& err) {
  if (!d) return refuse(err, AMDZK_E_INVALID, "null description");
  if (d->size < sizeof(amdzk_witness_desc)) return refuse(err, AMDZK_E_INVALID, "desc->size %llu is too small (%llu)", d->size, sizeof(amdzk_witness_desc));
  if ((d->n_constants && !d->constants) || (d->n_nodes && !d->nodes) || (d->n_cells && !d->cells) || (d->n_publics && !d->publics))
    return refuse(err, AMDZK_E_INVALID, "null array with a non-zero count");
  if (d->k > 31) return refuse(err, AMDZK_E_INVALID, "k = %llu > 31", d->k);
  p = Program();
  p.k = d->k;
  p.num_advice = d->num_advice;
  p.n_inputs = d->n_inputs;
  p.consts.resize(d->n_constants);
  for (uint32_t i = 0; i < d->n_constants; i++) {
    memcpy(p.consts[i].l, d->constants + 4 * (size_t)i, 32);
    if (!bn254::is_canonical(p.consts[i])) return refuse(err, AMDZK_E_INVALID, "constant %llu is not below the modulus", i);
  }
  const uint32_t n = d->n_nodes;
  std::vector<uint32_t> level(n);
  uint32_t depth = 0;  // number of levels
  for (uint32_t i = 0; i < n; i++) {
    const amdzk_wnode& nd = d->nodes[i];
    if (nd.op >= OP_COUNT) return refuse(err, AMDZK_E_INVALID, "node %llu: unknown op %llu", i, nd.op);
    const uint32_t ops[3] = {nd.a, nd.b, nd.c};
    const uint32_t ar = arity(nd.op);
    uint32_t lv = 0;
    for (uint32_t j = 0; j < ar; j++) {
      if (ops[j] >= i) return refuse(err, AMDZK_E_INVALID, "node %llu: operand %llu names node %llu, not an earlier node", i, j, ops[j]);
      lv = std::max(lv, level[ops[j]] + 1);
    }
    if (nd.op == AMDZK_W_INPUT && nd.a >= d->n_inputs) return refuse(err, AMDZK_E_INVALID, "node %llu: input %llu out of range (%llu)", i, nd.a, d->n_inputs);
    if (nd.op == AMDZK_W_CONST && nd.a >= d->n_constants)
      return refuse(err, AMDZK_E_INVALID, "node %llu: constant %llu out of range (%llu)", i, nd.a, d->n_constants);
    if (nd.op == AMDZK_W_BITS && (nd.c == 0 || nd.b > 256 || nd.c > 256 || nd.b + nd.c > 256))
      return refuse(err, AMDZK_E_INVALID, "node %llu: BITS lo = %llu, len = %llu (len >= 1 and lo + len <= 256)", i, nd.b, nd.c);
    level[i] = lv;
    depth = std::max(depth, lv + 1);
  }
  // order by level, the caller's order kept inside a level
  p.level_off.assign(n ? depth + 1 : 0, 0);
  for (uint32_t i = 0; i < n; i++) p.level_off[level[i] + 1]++;
  for (uint32_t l = 0; l < depth && n; l++) p.level_off[l + 1] += p.level_off[l];
  p.slot_of.resize(n);
  {
    std::vector<uint32_t> next(p.level_off.begin(), p.level_off.end());
    for (uint32_t i = 0; i < n; i++) p.slot_of[i] = next[level[i]]++;
  }
  p.nodes.resize(n);
  for (uint32_t i = 0; i < n; i++) {
    const amdzk_wnode& nd = d->nodes[i];
    Node o{nd.op, nd.a, nd.b, nd.c};
    const uint32_t ar = arity(nd.op);
    if (ar >= 1) o.a = p.slot_of[nd.a];
    if (ar >= 2) o.b = p.slot_of[nd.b];
    if (ar >= 3) o.c = p.slot_of[nd.c];
    if (ar < 3 && nd.op != AMDZK_W_BITS) o.c = 0;  // unused fields: never followed, kept at 0
    if (ar < 2 && nd.op != AMDZK_W_BITS) o.b = 0;
    p.nodes[p.slot_of[i]] = o;
  }
  p.cells.resize(d->n_cells);
  for (uint32_t j = 0; j < d->n_cells; j++) {
    const amdzk_wcell& c = d->cells[j];
    if (c.node >= n) return refuse(err, AMDZK_E_INVALID, "cell %llu names node %llu of %llu", j, c.node, n);
    if (c.column >= d->num_advice) return refuse(err, AMDZK_E_INVALID, "cell %llu: column %llu >= num_advice %llu", j, c.column, d->num_advice);
    if (c.row >= ((uint64_t)1 << d->k)) return refuse(err, AMDZK_E_INVALID, "cell %llu: row %llu >= 2^%llu", j, c.row, d->k);
    p.cells[j] = Cell{p.slot_of[c.node], c.column, c.row};
  }
  std::sort(p.cells.begin(), p.cells.end(), [](const Cell& x, const Cell& y) { return x.column != y.column ? x.column < y.column : x.row < y.row; });
  for (size_t j = 1; j < p.cells.size(); j++)
    if (p.cells[j].column == p.cells[j - 1].column && p.cells[j].row == p.cells[j - 1].row)
      return refuse(err, AMDZK_E_INVALID, "the cell (column %llu, row %llu) is named twice", p.cells[j].column, p.cells[j].row);
  p.publics.resize(d->n_publics);
  for (uint32_t j = 0; j < d->n_publics; j++) {
    if (d->publics[j] >= n) return refuse(err, AMDZK_E_INVALID, "public %llu names node %llu of %llu", j, d->publics[j], n);
    p.publics[j] = p.slot_of[d->publics[j]];
  }
  return AMDZK_OK;
}

// ---- the launch plan of one call
struct Plan {
  size_t runs = 0, per_run = 0;  // R runs of P proofs (the last one shorter)
  size_t scratch_bytes = 0;      // (n_nodes + n_publics) * P * 32 + SCRATCH_FIXED
  uint32_t launches = 0;         // over all runs: level launches, the scatter, the gather
};

// the launches of the levels for a run of P proofs: fn(first level, one past the last level, fused)
template <class F>
inline void for_each_launch(const Program& p, size_t P, F&& fn) {
  const uint32_t L = p.levels();
  uint32_t l = 0;
  while (l < L) {
    const uint64_t items = (uint64_t)(p.level_off[l + 1] - p.level_off[l]) * P;
    if (items > FUSED_WIDTH) {
      fn(l, l + 1, false);
      l++;
      continue;
    }
    uint32_t e = l + 1;
    while (e < L && (uint64_t)(p.level_off[e + 1] - p.level_off[e]) * P <= FUSED_WIDTH) e++;
    fn(l, e, true);
    l = e;
  }
}

inline int plan(const Program& p, size_t n_proofs, size_t max_scratch_bytes, Plan& out, std::string& err) {
  if (n_proofs == 0) return refuse(err, AMDZK_E_INVALID, "n_proofs = 0");
  const bool dflt = max_scratch_bytes == 0;
  const size_t cap = dflt ? DEFAULT_SCRATCH : max_scratch_bytes;
  const uint64_t per_proof = ((uint64_t)p.nodes.size() + p.publics.size()) * 32;  // < 2^38
  // everything below is computed in size_t: refuse what would not fit it
  const uint64_t widest = std::max<uint64_t>({1, p.widest(), p.cells.size(), p.publics.size(), p.n_inputs});
  if (n_proofs > (SIZE_MAX - SCRATCH_FIXED) / std::max<uint64_t>(per_proof, 32) || n_proofs > SIZE_MAX / 32 / widest)
    return refuse(err, AMDZK_E_UNSUPPORTED, "the workspace of %llu proofs does not fit size_t", n_proofs);
  if (per_proof + SCRATCH_FIXED > cap)
    return refuse(err, dflt ? AMDZK_E_UNSUPPORTED : AMDZK_E_INVALID, "one proof needs %llu bytes of workspace, the bound is %llu", per_proof + SCRATCH_FIXED,
                  cap);
  size_t fit = per_proof ? (size_t)((cap - SCRATCH_FIXED) / per_proof) : n_proofs;  // proofs of one run, by bytes
  fit = (size_t)std::min<uint64_t>(fit, MAX_ITEMS / widest);                      // ... and by items of one launch
  if (fit == 0) return refuse(err, AMDZK_E_UNSUPPORTED, "a level of %llu nodes is too wide", widest);
  out.runs = (n_proofs + fit - 1) / fit;
  out.per_run = (n_proofs + out.runs - 1) / out.runs;
  out.scratch_bytes = (size_t)per_proof * out.per_run + SCRATCH_FIXED;
  uint64_t launches = 0;
  for (size_t r = 0, done = 0; r < out.runs; r++) {
    const size_t P = std::min(out.per_run, n_proofs - done);
    for_each_launch(p, P, [&](uint32_t, uint32_t, bool) { launches++; });
    launches += (p.cells.empty() ? 0 : 1) + (p.publics.empty() ? 0 : 1);
    done += P;
  }
  if (launches > 0xffffffffu) return refuse(err, AMDZK_E_UNSUPPORTED, "%llu launches", launches);
  out.launches = (uint32_t)launches;
  return AMDZK_OK;
}

// One proof on the host through eval_node: values[slot] for every slot. inputs: n_inputs Fr (Montgomery).
inline void host_run(const Program& p, const Fr* inputs, Fr* values) {
  for (size_t s = 0; s < p.nodes.size(); s++) {
    const Node& nd = p.nodes[s];
    const uint32_t ar = arity(nd.op);
    const Fr z = Fr::zero();
    const Fr a = nd.op == AMDZK_W_INPUT ? inputs[nd.a] : nd.op == AMDZK_W_CONST ? p.consts[nd.a] : values[nd.a];
    const Fr b = ar >= 2 ? values[nd.b] : z;
    const Fr c = ar >= 3 ? values[nd.c] : z;
    values[s] = eval_node(nd.op, nd.b, nd.c, a, b, c);
  }
}

}  // namespace wit
