// The expression compiler and program runner of the PLONK layer: circuit expressions (include/amdzk.h's postfix words)
// to the stack programs of plonk_kernels.hip's interpreters, the pass that readies a quotient-domain program for the
// limb-resident interpreter, and the upload / launch of a key's programs. Host code only. No kernel lives here.
#include <string.h>

#include <algorithm>

#include "pk.hpp"

using namespace bn254;

namespace {

// Translate a host-format postfix expression into device ops. The postfix words are first rebuilt
// into a tree so that a binary operation with a leaf operand (a column or a constant) becomes ONE
// fused instruction on the top of stack (MUL_COL / ADD_COL / SUB_COL / MUL_CONST / ADD_CONST) instead
// of push + pop through the LDS stack. Field addition and multiplication are exact and commutative,
// so the value is the one upstream's Expression::evaluate produces. Lagrange and extended programs
// share slot numbers for fixed/advice/instance columns.
struct ENode {
  uint32_t op, payload;
  int l, r;
};

int emit_tree(amdzk_ctx* ctx, const KeyMaterial& K, RotTable* grow, ProgramText& pr, const std::vector<ENode>& t, int i) {
  const ENode& n = t[i];
  auto is_col = [&](int j) { return t[j].op == XOP_FIXED || t[j].op == XOP_ADVICE || t[j].op == XOP_INSTANCE; };
  // the fused or pushing instruction `op` on column node j
  auto col_op = [&](uint32_t op, int j) -> int {
    const ENode& c = t[j];
    uint32_t col = c.payload >> 8;
    int32_t rot = (int32_t)(c.payload & 0xff) - 128;
    uint32_t slot = c.op == XOP_FIXED ? K.sl_fixed(col) : c.op == XOP_ADVICE ? K.sl_adv(col) : K.sl_inst(col);
    const int r = grow ? (int)grow->index(rot) : K.rots.find(rot);
    // (the one caller on a frozen key is the witness check; cannot happen for a key keygen made: the h(X) program queried the gates' rotations)
    if (r < 0) ZK_FAIL(ctx, AMDZK_E_INVALID, "check_witness: a gate polynomial queries a rotation the key's programs do not");
    pr.op(op, (slot << 8) | (uint32_t)r);
    return AMDZK_OK;
  };
  switch (n.op) {
    case XOP_CONST:
      pr.op(OP_PUSH_CONST, n.payload);
      pr.push();
      return AMDZK_OK;
    case XOP_FIXED:
    case XOP_ADVICE:
    case XOP_INSTANCE:
      ZK_TRY(col_op(OP_PUSH_COL, i));
      pr.push();
      return AMDZK_OK;
    case XOP_NEG:
      ZK_TRY(emit_tree(ctx, K, grow, pr, t, n.l));
      pr.op(OP_NEG);
      return AMDZK_OK;
    case XOP_SCALE:
      ZK_TRY(emit_tree(ctx, K, grow, pr, t, n.l));
      pr.op(OP_MUL_CONST, n.payload);
      return AMDZK_OK;
    case XOP_ADD: {
      int a = n.l, b = n.r;
      if (t[b].op == XOP_NEG && is_col(t[b].l)) {  // a + (-col) -> a - col
        ZK_TRY(emit_tree(ctx, K, grow, pr, t, a));
        ZK_TRY(col_op(OP_SUB_COL, t[b].l));
        return AMDZK_OK;
      }
      if (!is_col(b) && t[b].op != XOP_CONST && (is_col(a) || t[a].op == XOP_CONST)) std::swap(a, b);
      if (is_col(b)) {
        ZK_TRY(emit_tree(ctx, K, grow, pr, t, a));
        ZK_TRY(col_op(OP_ADD_COL, b));
        return AMDZK_OK;
      }
      if (t[b].op == XOP_CONST) {
        ZK_TRY(emit_tree(ctx, K, grow, pr, t, a));
        pr.op(OP_ADD_CONST, t[b].payload);
        return AMDZK_OK;
      }
      ZK_TRY(emit_tree(ctx, K, grow, pr, t, a));
      ZK_TRY(emit_tree(ctx, K, grow, pr, t, b));
      pr.op(OP_ADD);
      pr.pop();
      return AMDZK_OK;
    }
    case XOP_MUL: {
      int a = n.l, b = n.r;
      if (!is_col(b) && t[b].op != XOP_CONST && (is_col(a) || t[a].op == XOP_CONST)) std::swap(a, b);
      if (is_col(b)) {
        ZK_TRY(emit_tree(ctx, K, grow, pr, t, a));
        ZK_TRY(col_op(OP_MUL_COL, b));
        return AMDZK_OK;
      }
      if (t[b].op == XOP_CONST) {
        ZK_TRY(emit_tree(ctx, K, grow, pr, t, a));
        pr.op(OP_MUL_CONST, t[b].payload);
        return AMDZK_OK;
      }
      ZK_TRY(emit_tree(ctx, K, grow, pr, t, a));
      ZK_TRY(emit_tree(ctx, K, grow, pr, t, b));
      pr.op(OP_MUL);
      pr.pop();
      return AMDZK_OK;
    }
    default:
      ZK_FAIL(ctx, AMDZK_E_INVALID, "circuit: bad expression node %u", n.op);
  }
}

}  // namespace

int emit_expr(amdzk_ctx* ctx, const KeyMaterial& K, RotTable* grow, ProgramText& pr, const std::vector<uint32_t>& words) {
  std::vector<ENode> t;
  std::vector<int> st;
  for (uint32_t w : words) {
    uint32_t op = w >> 24, pl = w & 0xffffffu;
    switch (op) {
      case XOP_CONST:
        if (pl >= K.c_one) ZK_FAIL(ctx, AMDZK_E_INVALID, "circuit: constant index %u out of range", pl);
        t.push_back(ENode{op, pl, -1, -1});
        st.push_back((int)t.size() - 1);
        break;
      case XOP_FIXED:
      case XOP_ADVICE:
      case XOP_INSTANCE: {
        uint32_t col = pl >> 8;
        uint32_t lim = op == XOP_FIXED ? K.F : op == XOP_ADVICE ? K.A : K.I;
        if (col >= lim) ZK_FAIL(ctx, AMDZK_E_INVALID, "circuit: column %u out of range", col);
        t.push_back(ENode{op, pl, -1, -1});
        st.push_back((int)t.size() - 1);
      } break;
      case XOP_CHALLENGE:  // one more constant operand: its slot is written per proof, so nothing here may read its value
        if (pl >= K.num_challenges) ZK_FAIL(ctx, AMDZK_E_INVALID, "circuit: bad expression word %08x", w);
        t.push_back(ENode{XOP_CONST, K.c_chal0 + pl, -1, -1});
        st.push_back((int)t.size() - 1);
        break;
      case XOP_NEG:
      case XOP_SCALE:
        if (st.empty()) ZK_FAIL(ctx, AMDZK_E_INVALID, "circuit: malformed expression");
        if (op == XOP_SCALE && pl >= K.c_one) ZK_FAIL(ctx, AMDZK_E_INVALID, "circuit: constant index %u out of range", pl);
        t.push_back(ENode{op, pl, st.back(), -1});
        st.back() = (int)t.size() - 1;
        break;
      case XOP_ADD:
      case XOP_MUL: {
        if (st.size() < 2) ZK_FAIL(ctx, AMDZK_E_INVALID, "circuit: malformed expression");
        int r = st.back();
        st.pop_back();
        int l = st.back();
        t.push_back(ENode{op, 0, l, r});
        st.back() = (int)t.size() - 1;
      } break;
      default:
        ZK_FAIL(ctx, AMDZK_E_INVALID, "circuit: bad expression word %08x", w);
    }
  }
  if (st.size() != 1) ZK_FAIL(ctx, AMDZK_E_INVALID, "circuit: malformed expression");
  return emit_tree(ctx, K, grow, pr, t, st[0]);
}

// fold(acc * theta + expr) over a lookup's expressions (first term: 0*theta + e0 = e0)
int emit_compressed(amdzk_ctx* ctx, KeyMaterial& K, ProgramText& pr, uint32_t first, uint32_t count) {
  for (uint32_t i = 0; i < count; i++) {
    if (i > 0) pr.op(OP_MUL_CONST, K.c_theta);
    ZK_TRY(emit_expr(ctx, K, &K.rots, pr, K.exprs[first + i]));
    if (i > 0) {
      pr.op(OP_ADD);
      pr.pop();
    }
  }
  return AMDZK_OK;
}

// Quotient-domain programs run on the limb-resident interpreter (plonk_kernels.hip expr_eval_limbs_kernel): values are
// 9 x 29-bit limbs, lazily reduced. This pass walks the (straight-line, wave-uniform) program once with the bound of
// every stack entry in units of p and
//   * inserts OP_REDUCE where a product would leave f29_mul's range (a*b < 169 p^2), where a subtrahend is too large
//     for the K*p constants (below 2p: K = 3, below 9p: K = 10), before a value sinks into the LDS stack with a bound
//     above 8, and before OP_STORE (packing needs a value below 2p);
//   * picks OP_SUB / OP_SUB_BIG and OP_NEG / OP_NEG_BIG by the subtrahend's bound;
//   * replaces the Horner fold h = h*y + term (OP_ACC) by a sum of products with one reduction per group: the program
//     is cut into its terms (the stack is empty at every OP_ACC), a term that ends in `* hot[k]` loses that factor
//     and joins group k, the others group 4; term j of the original order adds term_j * y^(K-1-j) to the wide
//     accumulator (OP_WACC j; every sixth term of a group also moves the columns' carries up), and each group ends
//     with OP_WFLUSH k: h (+)= reduce(wide) * hot[k], h canonical in its output row. A group is split when its sum of
//     bounds would leave the reduction's range.
// Bounds: a column, constant or hot value is below 1 (canonical); a product is below 2; a sum adds the bounds; a
// difference a - b adds K to a's; the weak reduction gives 1.0002; a flushed group sum(bounds) / 169.3 + 1.
// nparts > 1 cuts the finalised program into that many independent pieces of about equal length (ProgramText::piece_starts):
// a piece is a run of terms of the group order, closed by its own flush, and its first flush overwrites ITS h (bit 4) —
// the interpreter runs piece p on the workgroups with blockIdx.y = p into h + p * rows, and the pieces' sums are added
// afterwards (h is linear in the terms). One proof alone fills the chip's wavefront slots only that way.
// Returns the number of terms (= the powers of y of amdzk_pk::d_ypow that the OP_WACC instructions point at).
uint32_t finalize_limb_program(ProgramText& pr, uint32_t nparts) {
  const double LIM = 160.0, RED = 1.01, GROUP_LIM = 169.0 * 30.0;  // a flushed group stays below ~31 p (+ h, canonical)
  struct Term {
    std::vector<uint32_t> words;
    double bound = 0;
    uint32_t index = 0, group = 4;
  };
  std::vector<Term> terms;
  std::vector<uint32_t> tail;  // programs without OP_ACC (OP_STORE only) keep their order
  std::vector<uint32_t> out;
  std::vector<double> st;  // bounds, st.back() = top of stack
  auto emit = [&](uint32_t op, uint32_t arg = 0) { out.push_back((op << 24) | (arg & 0xffffffu)); };
  auto reduce_tos = [&]() {
    emit(OP_REDUCE);
    st.back() = RED;
  };
  uint32_t depth = 0, nterms = 0;
  for (size_t wi = 0; wi < pr.words.size(); wi++) {
    const uint32_t w = pr.words[wi], op = w >> 24, arg = w & 0xffffffu;
    switch (op) {
      case OP_PUSH_COL:
      case OP_PUSH_CONST:
      case OP_PUSH_HOT:
        if (!st.empty() && st.back() > 8.0) reduce_tos();
        emit(op, arg);
        st.push_back(1.0);
        break;
      case OP_MUL_HOT:
        // the closing `* hot[k]` of a term is factored out of its group instead of being multiplied in
        if (st.size() == 1 && wi + 1 < pr.words.size() && (pr.words[wi + 1] >> 24) == OP_ACC) {
          Term t;
          t.group = arg;
          t.bound = st.back();
          t.index = nterms++;
          t.words.swap(out);
          terms.push_back(std::move(t));
          st.clear();
          wi++;  // the OP_ACC is consumed
          break;
        }
        [[fallthrough]];
      case OP_MUL_COL:
      case OP_MUL_CONST:
        if (st.back() >= LIM) reduce_tos();
        emit(op, arg);
        st.back() = 2.0;
        break;
      case OP_ADD_COL:
      case OP_ADD_CONST:
        if (st.back() + 1.0 > 40.0) reduce_tos();
        emit(op, arg);
        st.back() += 1.0;
        break;
      case OP_SUB_COL:
        if (st.back() + 3.0 > 40.0) reduce_tos();
        emit(op, arg);
        st.back() += 3.0;
        break;
      case OP_ADD: {
        if (st[st.size() - 2] + st.back() > 40.0) reduce_tos();
        const double b = st.back();
        st.pop_back();
        emit(op);
        st.back() += b;
      } break;
      case OP_SUB: {
        if (st.back() >= 9.0) reduce_tos();
        const double b = st.back();
        st.pop_back();
        emit(b < 2.0 ? OP_SUB : OP_SUB_BIG);
        st.back() += b < 2.0 ? 3.0 : 10.0;
      } break;
      case OP_MUL: {
        if (st[st.size() - 2] * st.back() >= LIM) reduce_tos();
        st.pop_back();
        emit(op);
        st.back() = 2.0;
      } break;
      case OP_NEG:
        if (st.back() >= 9.0) reduce_tos();
        emit(st.back() < 2.0 ? OP_NEG : OP_NEG_BIG);
        st.back() = st.back() < 2.0 ? 3.0 : 10.0;
        break;
      case OP_SQR:
        if (st.back() * st.back() >= LIM) reduce_tos();
        emit(op);
        st.back() = 2.0;
        break;
      case OP_ACC: {  // end of a term without a hot factor
        Term t;
        t.group = 4;
        t.bound = st.back();
        t.index = nterms++;
        t.words.swap(out);
        terms.push_back(std::move(t));
        st.clear();
      } break;
      case OP_STORE:
        if (st.back() >= 2.0) reduce_tos();
        emit(op, arg);
        st.pop_back();
        tail.insert(tail.end(), out.begin(), out.end());
        out.clear();
        break;
      case OP_PICK:  // a copy of the entry `arg` below the top; the top sinks into the LDS stack
        if (st.back() > 8.0) reduce_tos();
        emit(op, arg);
        st.push_back(st[st.size() - 1 - arg]);
        break;
      case OP_NIP:
        emit(op, arg);
        st.erase(st.end() - 1 - arg, st.end() - 1);
        break;
      default:
        emit(op, arg);
        break;
    }
    if (st.size() > depth) depth = (uint32_t)st.size();
  }
  tail.insert(tail.end(), out.begin(), out.end());
  std::vector<uint32_t> fin;
  bool first = true;
  auto flush = [&](uint32_t g) {
    fin.push_back((OP_WFLUSH << 24) | g | (first ? 16u : 0u));
    first = false;
  };
  size_t term_words = 0;
  for (const Term& t : terms) term_words += t.words.size() + 1;
  if (terms.empty() || !tail.empty()) nparts = 1;  // (programs that store columns are not cut)
  pr.piece_starts.clear();
  uint32_t part = 0;
  size_t part_begin = 0;
  if (nparts > 1) pr.piece_starts.push_back(0);
  for (uint32_t g = 0; g <= 4; g++) {
    double sum = 0;
    uint32_t since_carry = 0;
    bool open = false;
    for (const Term& t : terms) {
      if (t.group != g) continue;
      if (open && sum + t.bound > GROUP_LIM) {
        flush(g);
        sum = 0;
        since_carry = 0;
        open = false;
      }
      // the next piece starts where this one has its share of the instructions
      if (part + 1 < nparts && fin.size() - part_begin >= (term_words + nparts - 1) / nparts) {
        if (open) flush(g);
        sum = 0;
        since_carry = 0;
        open = false;
        part++;
        part_begin = fin.size();
        pr.piece_starts.push_back((uint32_t)fin.size());
        first = true;
      }
      fin.insert(fin.end(), t.words.begin(), t.words.end());
      const bool carry = ++since_carry == 6;  // a column holds six un-carried terms
      if (carry) since_carry = 0;
      fin.push_back((OP_WACC << 24) | (carry ? 1u << 23 : 0u) | t.index);
      sum += t.bound;
      open = true;
    }
    if (open) flush(g);
  }
  fin.insert(fin.end(), tail.begin(), tail.end());
  pr.words.swap(fin);
  pr.depth = depth + 1;
  return nterms;
}

// d_consts261[i] = 32 * consts[i] in the ordinary form, i.e. consts[i] in radix 2^261 (a few hundred values).
int upload_consts261(amdzk_ctx* ctx, amdzk_pk* pk) {
  Fr k32 = Fr::one();
  for (int i = 0; i < 5; i++) k32 = add(k32, k32);
  std::vector<Fr> c(pk->consts.size());
  for (size_t i = 0; i < c.size(); i++) c[i] = mul(pk->consts[i], k32);
  ZK_TRY(h2d_staged(ctx, pk, pk->d_consts261, c.data(), c.size() * 32));
  // without the pinned staging area the copy above reads `c` asynchronously: finish it before `c` goes away
  if (!pk->pin || c.size() * 32 > pk->pin_cap) ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  return AMDZK_OK;
}

// d_ypow[j] = y^(K-1-j) for the K terms of the h(X) program, radix 2^261 (upstream folds the constraint values with
// Horner, h = h*y + value, in the same order: term j carries y^(K-1-j)).
int upload_ypow(amdzk_ctx* ctx, amdzk_pk* pk) {
  const KeyMaterial& K = *pk->key;
  const uint32_t nt = K.h_terms;
  if (!nt) return AMDZK_OK;
  Fr k32 = Fr::one();
  for (int i = 0; i < 5; i++) k32 = add(k32, k32);
  std::vector<Fr> pw(nt);
  Fr cur = k32;
  const Fr y = pk->consts[K.c_y], beta = pk->consts[K.c_beta];
  std::vector<Fr> bpow = {Fr::one()};  // beta^m for the terms whose factor beta^m was taken out (the permutation products)
  for (uint32_t j = nt; j-- > 0;) {
    const uint32_t m = j < K.h_term_beta_pow.size() ? K.h_term_beta_pow[j] : 0;
    while (bpow.size() <= m) bpow.push_back(mul(bpow.back(), beta));
    pw[j] = m ? mul(cur, bpow[m]) : cur;
    cur = mul(cur, y);
  }
  ZK_TRY(h2d_staged(ctx, pk, pk->d_ypow, pw.data(), pw.size() * 32));
  if (!pk->pin || pw.size() * 32 > pk->pin_cap) ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  return AMDZK_OK;
}

// Resolve slots / rotation indices / constant indices into addresses and row offsets for one domain
// and upload the 16-byte instructions.
int upload_program(amdzk_ctx* ctx, amdzk_pk* pk, Program& pr, bool extended) {
  const KeyMaterial& K = *pk->key;
  const std::vector<uint32_t>& words = pr.text->words;
  const std::vector<const Fr*>& cols = extended ? pk->h_cols_ext : pk->h_cols_lag;
  // The interpreters fetch every instruction's operand, and the instruction two ahead, unconditionally: an
  // instruction without an operand names the first constant, and two END instructions close the program.
  const Fr* dummy = extended ? pk->d_consts261 : pk->d_consts;
  std::vector<ExprInstr> ins(words.size() + 2);
  for (size_t i = 0; i < ins.size(); i++) {
    const uint32_t w = i < words.size() ? words[i] : (uint32_t)OP_END << 24, op = w >> 24, arg = w & 0xffffffu;
    ins[i].op_arg = w;
    ins[i].rot = 0;
    ins[i].ptr = dummy;
    if (op == OP_PUSH_COL || op == OP_MUL_COL || op == OP_ADD_COL || op == OP_SUB_COL) {
      if ((arg >> 8) >= cols.size() || (arg & 0xff) >= K.rots.rots.size()) ZK_FAIL(ctx, AMDZK_E_INVALID, "program: bad column operand");
      ins[i].ptr = cols[arg >> 8];
      ins[i].rot = K.rots.rots[arg & 0xff];  // rows of one coset are consecutive: a rotation is a row offset in both domains
    } else if (op == OP_PUSH_CONST || op == OP_MUL_CONST || op == OP_ADD_CONST) {
      if (arg >= pk->consts.size()) ZK_FAIL(ctx, AMDZK_E_INVALID, "program: bad constant operand");
      ins[i].ptr = (extended ? pk->d_consts261 : pk->d_consts) + arg;
    } else if (op == OP_WACC) {
      if (!extended || (arg & 0x7fffffu) >= K.h_terms) ZK_FAIL(ctx, AMDZK_E_INVALID, "program: bad power of y");
      ins[i].ptr = pk->d_ypow + (arg & 0x7fffffu);
    }
  }
  ZK_TRY(dalloc(ctx, pk, &pr.d_instr, ins.size()));
  ZK_TRY(h2d(ctx, pr.d_instr, ins.data(), ins.size() * sizeof(ExprInstr)));
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));  // `ins` is a host temporary
  return AMDZK_OK;
}

// the launch arguments of a program of this key: its pieces, its column table, where it stores
int program_args(amdzk_ctx* ctx, const amdzk_pk* pk, const Program& bound, bool extended, Fr* const* d_outs, Fr* h_out, ExprArgs& a) {
  const KeyMaterial& K = *pk->key;
  const ProgramText& pr = *bound.text;
  a.prog = bound.d_instr;
  a.prog_len = (uint32_t)pr.words.size();
  a.cols = extended ? pk->d_cols_ext : pk->d_cols_lag;
  a.outs = d_outs;
  a.h_out = h_out;
  a.nrows = extended ? K.ext : K.n;
  a.mask = K.n - 1;
  // Quotient-domain programs (h(X), l_active) run in radix 2^261: their columns come from
  // zk_coeff_to_cosets_r261, their constants from d_consts261, and the result goes back through
  // zk_cosets_to_pieces. Lagrange-domain programs read the caller's radix-2^256 witness as is.
  a.radix261 = extended ? 1u : 0u;
  a.nparts = 0;
  if (!extended && pr.piece_starts.size() > 1) {  // balanced by instruction count, cut at piece boundaries only
    const uint32_t total = (uint32_t)pr.words.size(), want = std::min<uint32_t>(EXPR_MAX_PARTS, (uint32_t)pr.piece_starts.size());
    uint32_t begin = 0;
    for (size_t i = 1; i <= pr.piece_starts.size() && a.nparts < want; i++) {
      const uint32_t end = i < pr.piece_starts.size() ? pr.piece_starts[i] : total;
      const bool last_part = a.nparts + 1 == want;
      if ((!last_part && end >= (uint64_t)total * (a.nparts + 1) / want) || (last_part && end == total)) {
        a.part_start[a.nparts] = begin;
        a.part_len[a.nparts] = end - begin;
        a.nparts++;
        begin = end;
      }
    }
    if (begin != total) a.nparts = 0;  // (cannot happen: the last part runs to the end) — fall back to one part
  }
  if (extended && pr.piece_starts.size() > 1) {  // the pieces finalize_limb_program cut: one per blockIdx.y, h_out + p * rows each
    if (pr.piece_starts.size() > (size_t)EXPR_MAX_PARTS) ZK_FAIL(ctx, AMDZK_E_INVALID, "program: too many pieces");
    for (size_t i = 0; i < pr.piece_starts.size(); i++) {
      a.part_start[i] = pr.piece_starts[i];
      a.part_len[i] = (i + 1 < pr.piece_starts.size() ? pr.piece_starts[i + 1] : (uint32_t)pr.words.size()) - pr.piece_starts[i];
    }
    a.nparts = (uint32_t)pr.piece_starts.size();
  }
  for (int i = 0; i < EXPR_HOT; i++) a.hot[i] = EXPR_NO_SLOT;
  if (extended && pr.uses_hot) {
    a.hot[0] = K.se_l0();
    a.hot[1] = K.se_llast();
    a.hot[2] = K.se_lactive();
    a.hot[3] = K.se_x();
  }
  return AMDZK_OK;
}

int run_program(amdzk_ctx* ctx, const amdzk_pk* pk, const Program& bound, bool extended, Fr* const* d_outs, Fr* h_out, const char* name) {
  const ProgramText& pr = *bound.text;
  ExprArgs a;
  ZK_TRY(program_args(ctx, pk, bound, extended, d_outs, h_out, a));
  return extended ? zk_expr_eval_limbs(ctx, a, limb_stack_slots(pr), name) : zk_expr_eval(ctx, a, lagrange_stack_slots(pr), name);
}

// A right-nested expression, (a*b) + ((c*d) + (...)), adds a stack entry per level (emit_tree keeps the operands' order),
// and nothing else bounds a program's depth: a key whose program does not fit would fail at proof time, in the launch.
int check_program_fits(amdzk_ctx* ctx, const ProgramText& pr, bool extended, const char* name) {
  int limit = 0;
  if (hipDeviceGetAttribute(&limit, hipDeviceAttributeSharedMemPerBlockOptin, ctx->device) != hipSuccess || limit <= 0) {
    (void)hipGetLastError();
    ZK_HIP(ctx, hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
  }
  const uint32_t slots = extended ? limb_stack_slots(pr) : lagrange_stack_slots(pr);
  auto bytes = [&](uint32_t s) { return extended ? expr_limbs_lds_bytes(s) : expr_lds_bytes(s); };
  if (bytes(slots) <= (size_t)limit) return AMDZK_OK;
  uint32_t fit = 0;  // the largest recorded depth whose launch fits
  for (uint32_t s = 1; bytes(s) <= (size_t)limit; s++) fit = extended ? s + 1 : s - 1;
  ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "keygen: the %s program has stack depth %u (%zu bytes of LDS); depth %u fits this device (%d bytes per workgroup)",
          name, pr.depth, bytes(slots), fit, limit);
}

extern "C" {

// Test hooks for the host pass that prepares quotient-domain programs for the limb-resident interpreter
// (finalize_limb_program): (a) the pass on caller-supplied program words — pure host code, no device — and (b) the
// finalised h(X) program of a key. Words are `op << 24 | arg` with the opcodes of csrc/plonk_kernels.hpp.
int amdzk_debug_limb_program(const uint32_t* words, size_t n, uint32_t* out, size_t cap, size_t* out_n, uint32_t* depth) {
  if ((!words && n) || !out_n) return AMDZK_E_INVALID;
  ProgramText pr;
  pr.words.assign(words, words + n);
  (void)finalize_limb_program(pr);
  *out_n = pr.words.size();
  if (depth) *depth = pr.depth;
  if (out) {
    if (cap < pr.words.size()) return AMDZK_E_INVALID;
    memcpy(out, pr.words.data(), pr.words.size() * sizeof(uint32_t));
  }
  return AMDZK_OK;
}
int amdzk_pk_h_program(const amdzk_pk* pk, uint32_t* out, size_t cap, size_t* out_n) {
  if (!pk || !out_n) return AMDZK_E_INVALID;
  const std::vector<uint32_t>& words = pk->key->prog_h.words;
  *out_n = words.size();
  if (out) {
    if (cap < words.size()) return AMDZK_E_INVALID;
    memcpy(out, words.data(), words.size() * sizeof(uint32_t));
  }
  return AMDZK_OK;
}

}  // extern "C"
