// amdzk_check_witness (MockProver::verify's constraint checks [UP], without its region bookkeeping): its device kernels,
// their launch wrappers and, behind them, its host side.
//
//   expr_check_kernel    — the gate polynomials as one Lagrange-domain stack program (the interpreter of
//                          plonk_kernels.hip's expr_eval_kernel, one row per lane, operand stack in LDS) whose values are
//                          TESTED instead of stored: OP_CHECK pops a value and counts the row when it is non-zero.
//   lookup_member_kernel — every theta-compressed input row, binary-searched in its sorted table.
//   sigma_decode_kernel  — sigma_i(omega^j) = delta^i' omega^j' back to (i', j') by arithmetic alone, once per key.
//   copy_check_kernel    — the two cells of every copy constraint, gathered and compared.
//
// A satisfying witness is the common case and pays nothing for the bookkeeping: a wavefront without a failing lane
// issues no atomic. Where lanes fail, the lowest failing lane of the wavefront adds the wavefront's count and its own
// row — rows grow with the lane, so it is the wavefront's smallest — with two vector atomics.
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "fp29.cuh"
#include "hostcrypto.hpp"
#include "pk.hpp"

using namespace bn254;
using zkhost::ChaCha20Rng;

// One more instruction of Lagrange-domain programs, executed by expr_check_kernel only: pop the top of stack; where it is
// a non-zero residue on a row < usable, constraint `arg` has one more failing row. (Beside plonk_kernels.hpp's ExprOp,
// whose interpreters ignore it.)
constexpr uint32_t OP_CHECK = 24;

// What a check leaves per constraint: count[c] failing rows, the smallest of them in first[c] (UINT32_MAX: none). The
// caller clears both before the kernels run (count to 0, first to 0xFF bytes).
struct CheckCounters {
  unsigned long long* count;
  uint32_t* first;
};

namespace {

__device__ __forceinline__ Fr ck_ld_fr(const Fr* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint4 a = q[0], b = q[1];
  Fr r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  return r;
}

// `fail` lanes of this wavefront each have one failing row of constraint c, lane order = row order
__device__ __forceinline__ void ck_record(bool fail, uint32_t c, uint32_t row, const CheckCounters& out) {
  const unsigned long long m = __ballot(fail);
  if (fail && (m & ((1ull << (threadIdx.x & 63u)) - 1ull)) == 0) {
    atomicAdd(out.count + c, (unsigned long long)__popcll(m));
    atomicMin(out.first + c, row);
  }
}

// ------------------------------------------------------------------------------ gates
typedef const ExprInstr __attribute__((address_space(4))) * CkProgPtr;
struct CkWord {  // one instruction in scalar registers
  uint32_t op_arg;
  int32_t rot;
  const Fr* ptr;
};
__device__ __forceinline__ CkWord ck_word(CkProgPtr prog, uint32_t i) {
  CkWord w;
  w.op_arg = prog[i].op_arg;
  w.rot = prog[i].rot;
  w.ptr = prog[i].ptr;
  return w;
}
__device__ __forceinline__ Fr ck_fetch(const CkWord& in, size_t row, size_t mask) {
  const uint32_t op = in.op_arg >> 24;
  const size_t sel = (op == OP_PUSH_COL || op == OP_MUL_COL || op == OP_ADD_COL || op == OP_SUB_COL) ? ~(size_t)0 : 0;
  return ck_ld_fr(in.ptr + (((row + (size_t)(int64_t)in.rot) & mask) & sel));
}

// The shape of expr_eval_kernel: instructions through the constant address space two ahead, the next operand always in
// flight, the top of stack in registers. Values are canonical throughout — columns and constants arrive below r, and
// add, sub, neg and fr29_mul_std all return the canonical residue (reduce_once / the conditional add of r /
// f29_pack_canonical) — so "all eight words zero" is the test of the residue.
__global__ __launch_bounds__(EXPR_THREADS) void expr_check_kernel(ExprArgs a, uint32_t usable, CheckCounters out) {
  extern __shared__ uint4 lds_raw[];
  Fr* stack = reinterpret_cast<Fr*>(lds_raw);  // [depth][EXPR_THREADS]
  const uint32_t tid = threadIdx.x;
  const size_t row = (size_t)blockIdx.x * EXPR_THREADS + tid;
  if (row >= a.nrows) return;  // no barriers below
  Fr tos = Fr::zero();
  uint32_t sp = 0;
  const uint32_t first = a.nparts ? a.part_start[blockIdx.y] : 0u, prog_len = a.nparts ? a.part_len[blockIdx.y] : a.prog_len;
  const CkProgPtr prog = (CkProgPtr)a.prog + first;
  CkWord cur = ck_word(prog, 0), nxt = ck_word(prog, 1);
  Fr pre = ck_fetch(cur, row, a.mask);
  for (uint32_t pc = 0; pc < prog_len; pc++) {
    const uint32_t op = cur.op_arg >> 24, arg = cur.op_arg & 0xffffffu;
    const Fr v = pre;
    const CkWord nn = ck_word(prog, pc + 2);
    pre = ck_fetch(nxt, row, a.mask);
    switch (op) {
      case OP_PUSH_COL:
      case OP_PUSH_CONST:
        if (sp > 0) stack[(sp - 1) * EXPR_THREADS + tid] = tos;
        tos = v;
        sp++;
        break;
      case OP_MUL_COL:
      case OP_MUL_CONST:
        tos = fr29_mul_std(tos, v);
        break;
      case OP_ADD_COL:
      case OP_ADD_CONST:
        tos = add(tos, v);
        break;
      case OP_SUB_COL:
        tos = sub(tos, v);
        break;
      case OP_ADD:
        tos = add(stack[(sp - 2) * EXPR_THREADS + tid], tos);
        sp--;
        break;
      case OP_SUB:
        tos = sub(stack[(sp - 2) * EXPR_THREADS + tid], tos);
        sp--;
        break;
      case OP_MUL:
        tos = fr29_mul_std(stack[(sp - 2) * EXPR_THREADS + tid], tos);
        sp--;
        break;
      case OP_NEG:
        tos = neg(tos);
        break;
      case OP_SQR:
        tos = fr29_mul_std(tos, tos);
        break;
      case OP_CHECK:
        ck_record(row < usable && !tos.is_zero(), arg, (uint32_t)row, out);
        sp--;
        if (sp > 0) tos = stack[(sp - 1) * EXPR_THREADS + tid];
        break;
      default:
        break;
    }
    cur = nxt;
    nxt = nn;
  }
}

// ------------------------------------------------------------------------------ lookups
__device__ __forceinline__ bool ck_key_less(const Fr& a, const Fr& b) {
#pragma unroll
  for (int i = 7; i >= 0; i--) {
    if (a.l[i] != b.l[i]) return a.l[i] < b.l[i];
  }
  return false;
}

// grid (rows, lookups): lower bound of the input's key among the table's first u keys (the padding sorts behind them)
__global__ __launch_bounds__(256) void lookup_member_kernel(const Fr* inputs, const Fr* tables, uint32_t n, uint32_t u, uint32_t c0,
                                                            CheckCounters out) {
  const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
  if (row >= u) return;
  const Fr key = ck_ld_fr(inputs + (size_t)l * n + row);
  const Fr* T = tables + (size_t)l * n;
  uint32_t lo = 0, hi = u;  // first position in [0, u] whose key is not below `key`
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (ck_key_less(ck_ld_fr(T + mid), key)) lo = mid + 1;
    else hi = mid;
  }
  const bool hit = lo < u && ck_ld_fr(T + lo) == key;
  ck_record(!hit, c0 + l, row, out);
}

// ------------------------------------------------------------------------------ copy constraints
// s = delta^i' omega^j' with omega of order 2^k and delta of odd order:
//   s^(2^k) = delta^(i' 2^k) names i' among the S constants tab[0..S) — k squarings and a search;
//   t = s delta^(-i') (tab[S + i']) lies in <omega>, and its exponent's bits fall out lowest first (Pohlig-Hellman):
//   (t omega^(-e))^(2^(k-1-b)) is 1 or -1 for e = the bits below b — k (k - 1) / 2 squarings, tab[2S + b] = omega^(-(2^b)).
// s^(2^k) matching a constant already puts t in the subgroup of order 2^k, which is <omega>: the search is the whole test.
__global__ __launch_bounds__(256) void sigma_decode_kernel(const Fr* sigma, uint32_t S, uint32_t k, uint32_t n, const Fr* tab, uint2* cells,
                                                           unsigned long long* bad) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  if (j >= n) return;
  const Fr s = ck_ld_fr(sigma + (size_t)c * n + j);
  Fr p = s;
  for (uint32_t i = 0; i < k; i++) p = fr29_mul_std(p, p);
  uint32_t col = S;
  for (uint32_t i = 0; i < S; i++)
    if (col == S && ck_ld_fr(tab + i) == p) col = i;
  if (col == S) {
    atomicMin(bad, (((unsigned long long)c << 32) | j) + 1ull);
    cells[(size_t)c * n + j] = make_uint2(0u, 0u);
    return;
  }
  Fr t = fr29_mul_std(s, ck_ld_fr(tab + S + col));
  const Fr one = Fr::one();
  uint32_t e = 0;
  for (uint32_t b = 0; b < k; b++) {
    Fr x = t;
    for (uint32_t i = b + 1; i < k; i++) x = fr29_mul_std(x, x);
    if (x != one) {
      e |= 1u << b;
      t = fr29_mul_std(t, ck_ld_fr(tab + 2 * S + b));
    }
  }
  cells[(size_t)c * n + j] = make_uint2(col, e);
}

// grid (rows, permutation columns)
__global__ __launch_bounds__(256) void copy_check_kernel(const Fr* const* cols, const uint2* cells, uint32_t n, uint32_t c0, CheckCounters out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
  if (j >= n) return;
  const uint2 to = cells[(size_t)c * n + j];
  const Fr v = ck_ld_fr(cols[c] + j), w = ck_ld_fr(cols[to.x] + to.y);
  ck_record(v != w, c0 + c, j, out);
}

}  // namespace

// ------------------------------------------------------------------------------ launch wrappers
// A Lagrange-domain program (ExprArgs as for zk_expr_eval, radix 2^256) whose values end in OP_CHECK instead of OP_STORE.
int zk_check_expr(amdzk_ctx* ctx, const ExprArgs& a, uint32_t depth, uint32_t usable, CheckCounters out, const char* name) {
  const size_t shmem = expr_lds_bytes(depth);
  const dim3 grid((unsigned)((a.nrows + EXPR_THREADS - 1) / EXPR_THREADS), a.nparts ? a.nparts : 1u), block(EXPR_THREADS);
  if (a.radix261) ZK_FAIL(ctx, AMDZK_E_INVALID, "check_expr: a Lagrange-domain program is needed");
  if (a.nparts > (uint32_t)EXPR_MAX_PARTS) ZK_FAIL(ctx, AMDZK_E_INVALID, "check_expr: too many program parts");
  if (usable > a.nrows || a.nrows > 0xffffffffull) ZK_FAIL(ctx, AMDZK_E_INVALID, "check_expr: bad row counts");
  if (shmem > 65536) ZK_HIP(ctx, hipFuncSetAttribute((const void*)expr_check_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  ZK_LAUNCH(ctx, name, expr_check_kernel, grid, block, shmem, a, usable, out);
  return AMDZK_OK;
}

// inputs / tables: [L][n] canonical keys (Fr::to_repr), every table sorted ascending with its rows >= usable padded by
// all-ones keys (zk_sort_keys' convention): input row r < usable of lookup l fails constraint first_constraint + l when
// its key is none of the table's first `usable` keys.
int zk_check_lookups(amdzk_ctx* ctx, const Fr* d_inputs, const Fr* d_tables, size_t L, uint32_t n, uint32_t usable, uint32_t first_constraint,
                     CheckCounters out) {
  if (!L || !usable) return AMDZK_OK;
  if (usable > n || L > 65535) ZK_FAIL(ctx, AMDZK_E_INVALID, "check_lookups: bad shape");
  ZK_LAUNCH(ctx, "check_lookup_member", lookup_member_kernel, dim3((usable + 255) / 256, (unsigned)L), dim3(256), 0, d_inputs, d_tables, n, usable,
            first_constraint, out);
  return AMDZK_OK;
}

// sigma: [S][n] Montgomery values delta^i' omega^j' -> cells[c * n + j] = (i', j'). d_tab: S values delta^(i * 2^k), S values
// delta^(-i), k values omega^(-(2^b)). A value that is no delta^i omega^j with i < S leaves (c << 32 | j) + 1 of the smallest
// such cell in *d_bad (the caller sets it to all ones: none).
int zk_sigma_decode(amdzk_ctx* ctx, const Fr* d_sigma, uint32_t S, uint32_t k, const Fr* d_tab, uint2* d_cells, unsigned long long* d_bad) {
  if (!S) return AMDZK_OK;
  if (S > 65535 || k > 31) ZK_FAIL(ctx, AMDZK_E_INVALID, "sigma_decode: bad shape");
  const uint32_t n = 1u << k;
  ZK_LAUNCH(ctx, "check_sigma_decode", sigma_decode_kernel, dim3((n + 255) / 256, S), dim3(256), 0, d_sigma, S, k, n, d_tab, d_cells, d_bad);
  return AMDZK_OK;
}

// cell (c, j) of the permutation fails constraint first_constraint + c when its value differs from the value of the cell
// d_cells names for it; d_cols[c]: the Lagrange values of permutation column c (n rows).
int zk_check_copies(amdzk_ctx* ctx, const Fr* const* d_cols, const uint2* d_cells, uint32_t S, uint32_t n, uint32_t first_constraint,
                    CheckCounters out) {
  if (!S) return AMDZK_OK;
  if (S > 65535) ZK_FAIL(ctx, AMDZK_E_INVALID, "check_copies: bad shape");
  ZK_LAUNCH(ctx, "check_copies", copy_check_kernel, dim3((n + 255) / 256, S), dim3(256), 0, d_cols, d_cells, n, first_constraint, out);
  return AMDZK_OK;
}

// ------------------------------------------------------------------------------ host side
// ---- amdzk_check_witness: MockProver::verify's constraint checks on the device (include/amdzk.h has the semantics).
// What this handle needs beyond what a proof uses, made by its first check: the gate program, the permutation columns'
// addresses in this workspace, the counters.
// The gate polynomials as one Lagrange-domain program, gate g ending in OP_CHECK g. The gates' rotations are all in the
// key's table already (the h(X) program queried them): emit_expr refuses any other.
int emit_check_gates(amdzk_ctx* ctx, const KeyMaterial& K, ProgramText& pr) {
  for (uint32_t g = 0; g < K.num_gates; g++) {
    pr.piece();
    ZK_TRY(emit_expr(ctx, K, nullptr, pr, K.exprs[g]));
    pr.op(OP_CHECK, g);
    pr.pop();
  }
  return AMDZK_OK;
}

static int check_build(amdzk_ctx* ctx, amdzk_pk* pk) {
  const KeyMaterial& K = *pk->key;
  amdzk_pk::Check& ck = pk->chk;
  if (ck.built) return AMDZK_OK;
  const uint32_t ncon = K.num_gates + K.L + K.S;
  if (!ck.prog_gates.d_instr) {
    ProgramText pr;
    ZK_TRY(emit_check_gates(ctx, K, pr));
    ck.gates = std::move(pr);
    ck.prog_gates.text = &ck.gates;
    ZK_TRY(upload_program(ctx, pk, ck.prog_gates, false));
  }
  if (!ck.d_count) {
    ZK_TRY(dalloc(ctx, pk, &ck.d_count, (size_t)ncon + ((size_t)ncon + 1) / 2 + 1));  // u64 counts, then u32 first rows
    ck.d_first = reinterpret_cast<uint32_t*>(ck.d_count + ncon);
  }
  ck.built = true;
  return AMDZK_OK;
}

// The key's sigma columns back to (column, row), once: S * n * 8 bytes that every handle of the key reads.
static int check_decode_sigma(amdzk_ctx* ctx, const KeyMaterial& K) {
  KeyMaterial::CheckShared& sh = *K.chk_shared;
  std::lock_guard<std::mutex> lock(sh.guard);
  if (sh.decoded || !K.S) return AMDZK_OK;
  const uint32_t S = K.S, k = K.k;
  const size_t n = K.n;
  if (!sh.d_cells) {
    void* q = nullptr;
    if (hipMalloc(&q, (size_t)S * n * sizeof(uint2)) != hipSuccess) ZK_FAIL(ctx, AMDZK_E_NOMEM, "check_witness: hipMalloc of the decoded permutation failed");
    sh.d_cells = (uint2*)q;
  }
  // delta^(i 2^k), delta^(-i) for i < S, omega^(-(2^b)) for b < k
  std::vector<Fr> tab(2 * (size_t)S + k);
  const Fr delta = fr_delta(), delta_inv = inv(delta);
  Fr d2k = delta;
  for (uint32_t i = 0; i < k; i++) d2k = mul(d2k, d2k);
  Fr a = Fr::one(), b = Fr::one();
  for (uint32_t i = 0; i < S; i++) {
    tab[i] = a;
    tab[S + i] = b;
    a = mul(a, d2k);
    b = mul(b, delta_inv);
  }
  Fr w = K.omega_inv;
  for (uint32_t i = 0; i < k; i++) {
    tab[2 * (size_t)S + i] = w;
    w = mul(w, w);
  }
  void* d_tab = nullptr;
  if (hipMalloc(&d_tab, tab.size() * 32 + 8) != hipSuccess) ZK_FAIL(ctx, AMDZK_E_NOMEM, "check_witness: hipMalloc failed");
  unsigned long long* d_bad = reinterpret_cast<unsigned long long*>((Fr*)d_tab + tab.size());
  unsigned long long bad = 0;
  int r = h2d(ctx, d_tab, tab.data(), tab.size() * 32);
  if (r == AMDZK_OK && hipMemsetAsync(d_bad, 0xFF, 8, ctx->stream) != hipSuccess) r = AMDZK_E_HIP;
  if (r == AMDZK_OK) r = zk_sigma_decode(ctx, K.sigma_lag, S, k, (const Fr*)d_tab, sh.d_cells, d_bad);
  if (r == AMDZK_OK) r = d2h(ctx, &bad, d_bad, 8);
  else (void)zk_host_wait(ctx, ctx->stream);  // `tab` is a host temporary
  hipFree(d_tab);
  ZK_TRY(r);
  if (bad != ~0ull) {
    const unsigned long long cell = bad - 1;
    ZK_FAIL(ctx, AMDZK_E_INVALID, "check_witness: sigma column %u row %u is not delta^i omega^j for a column i < %u of this circuit",
            (uint32_t)(cell >> 32), (uint32_t)cell, S);
  }
  sh.decoded = true;
  return AMDZK_OK;
}

static int check_witness_run(amdzk_ctx* ctx, amdzk_pk* pk, const uint64_t* const* instances, const size_t* instance_lens, const void* d_advice,
                             size_t advice_stride, const amdzk_check_opts* opts, amdzk_check_failure* out, size_t cap, size_t* n_failures) {
  if (!pk || !n_failures || (pk->key->A && !d_advice)) ZK_FAIL(ctx, AMDZK_E_INVALID, "check_witness: null argument");
  const KeyMaterial& K = *pk->key;
  if (opts && opts->size < sizeof(amdzk_check_opts))
    ZK_FAIL(ctx, AMDZK_E_INVALID, "check_witness: amdzk_check_opts.size is %zu, this library needs %zu", opts->size, sizeof(amdzk_check_opts));
  const size_t n = K.n, usable = n - (K.bf + 1);
  const uint32_t A = K.A, I = K.I, L = K.L, S = K.S, G = K.num_gates, ncon = G + L + S;
  if (K.A && advice_stride < n) ZK_FAIL(ctx, AMDZK_E_INVALID, "check_witness: advice stride < n");
  const uint32_t given = opts && opts->challenges ? opts->num_challenges : 0;
  if (K.num_challenges && !given) ZK_FAIL(ctx, AMDZK_E_INVALID, "check_witness: the key has %u challenges and none were given", K.num_challenges);
  if ((opts ? opts->num_challenges : 0) != K.num_challenges)
    ZK_FAIL(ctx, AMDZK_E_INVALID, "check_witness: %u challenges given, the key has %u", opts ? opts->num_challenges : 0, K.num_challenges);
  for (uint32_t c = 0; c < I; c++) {
    const size_t len = instance_lens ? instance_lens[c] : 0;
    if (len > usable) ZK_FAIL(ctx, AMDZK_E_INVALID, "check_witness: instance column %u too long (InstanceTooLarge)", c);
    if (len && (!instances || !instances[c])) ZK_FAIL(ctx, AMDZK_E_INVALID, "check_witness: null argument (instance column %u)", c);
  }
  ZK_TRY(check_build(ctx, pk));
  ZK_TRY(check_decode_sigma(ctx, K));
  const amdzk_pk::Check& ck = pk->chk;
  const CheckCounters counters = {ck.d_count, ck.d_first};
  *n_failures = 0;
  if (!ncon) return AMDZK_OK;
  ZK_TRY(zk_pk_poison(ctx, pk));
  ZK_HIP(ctx, hipMemsetAsync(ck.d_count, 0, (size_t)ncon * 8, ctx->stream));
  ZK_HIP(ctx, hipMemsetAsync(ck.d_first, 0xFF, (size_t)ncon * 4, ctx->stream));
  // the witness into the workspace as create_proof copies it, unblinded: instance columns zero behind the caller's values
  if (I) {
    ZK_HIP(ctx, hipMemsetAsync(pk->inst(), 0, (size_t)I * n * 32, ctx->stream));
    for (uint32_t c = 0; c < I; c++) {
      const size_t len = instance_lens ? instance_lens[c] : 0;
      if (!len) continue;
      ZK_TRY(h2d_staged(ctx, pk, pk->inst() + (size_t)c * n, instances[c], len * 32));
    }
  }
  if (A) ZK_HIP(ctx, hipMemcpy2DAsync(pk->adv(), n * 32, d_advice, advice_stride * 32, n * 32, A, hipMemcpyDeviceToDevice, ctx->stream));
  {  // theta and the phase challenges into their slots of the constant table
    ChaCha20Rng rng(opts ? opts->theta_seed : 0);
    pk->consts[K.c_theta] = rng.fr();
    ZK_TRY(h2d_staged(ctx, pk, pk->d_consts + K.c_theta, &pk->consts[K.c_theta], 32));
    if (K.num_challenges) {
      memcpy(pk->consts[K.c_chal0].l, opts->challenges, (size_t)K.num_challenges * 32);
      ZK_TRY(h2d_staged(ctx, pk, pk->d_consts + K.c_chal0, &pk->consts[K.c_chal0], (size_t)K.num_challenges * 32));
    }
  }
  if (G) {
    ExprArgs a;
    ZK_TRY(program_args(ctx, pk, pk->chk.prog_gates, false, nullptr, nullptr, a));
    ZK_TRY(zk_check_expr(ctx, a, lagrange_stack_slots(ck.gates), (uint32_t)usable, counters, "expr_check_gates"));
  }
  if (L) {  // compressed inputs and tables as canonical keys, the tables sorted (constant ones were sorted at keygen)
    ZK_TRY(run_program(ctx, pk, pk->prog_compress, false, pk->d_outs_compress, nullptr, "expr_lookup_compress"));
    ZK_TRY(d2d(ctx, pk->la(), pk->ci, (size_t)L * n * 32));
    ZK_TRY(amdzk_fr_to_repr_dev(ctx, pk->la(), (size_t)L * n));
    const uint32_t pre = K.lk_const, rest = L - pre;
    if (pre) ZK_TRY(d2d(ctx, pk->lk_ts, K.lk_ts_const, (size_t)pre * n * 32));
    if (rest) {
      Fr* Tr = pk->lk_ts + (size_t)pre * n;
      ZK_TRY(d2d(ctx, Tr, pk->ct + (size_t)pre * n, (size_t)rest * n * 32));
      ZK_TRY(amdzk_fr_to_repr_dev(ctx, Tr, (size_t)rest * n));
      ZK_HIP(ctx, hipMemset2DAsync(Tr + usable, n * 32, 0xFF, (n - usable) * 32, rest, ctx->stream));
      ZK_TRY(zk_sort_keys(ctx, Tr, rest, (uint32_t)n, n));
    }
    ZK_TRY(zk_check_lookups(ctx, pk->la(), pk->lk_ts, L, (uint32_t)n, (uint32_t)usable, G, counters));
  }
  if (S) ZK_TRY(zk_check_copies(ctx, pk->d_perm_cols, K.chk_shared->d_cells, S, (uint32_t)n, G + L, counters));
  std::vector<unsigned long long> host((size_t)ncon + ((size_t)ncon + 1) / 2);
  ZK_TRY(d2h(ctx, host.data(), ck.d_count, (size_t)ncon * 12));
  const uint32_t* first = reinterpret_cast<const uint32_t*>(host.data() + ncon);
  size_t nf = 0;
  for (uint32_t c = 0; c < ncon; c++) {
    if (!host[c]) continue;
    if (out && nf < cap) {
      amdzk_check_failure& f = out[nf];
      f.kind = c < G ? AMDZK_CHECK_GATE : c < G + L ? AMDZK_CHECK_LOOKUP : AMDZK_CHECK_COPY;
      f.index = c < G ? c : c < G + L ? c - G : c - G - L;
      f.first_row = first[c];
      f.reserved = 0;
      f.count = host[c];
    }
    nf++;
  }
  *n_failures = nf;
  return AMDZK_OK;
}

extern "C" int amdzk_check_witness(amdzk_ctx* ctx, amdzk_pk* pk, const uint64_t* const* instances, const size_t* instance_lens, const void* d_advice,
                        size_t advice_stride, const amdzk_check_opts* opts, amdzk_check_failure* out, size_t cap, size_t* n_failures) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  // whatever was enqueued (copies from the caller's memory among it) is finished before a refused call returns
  return zk_quiet_if_refused(ctx, check_witness_run(ctx, pk, instances, instance_lens, d_advice, advice_stride, opts, out, cap, n_failures));
}
