// Device kernels of amdzk_check_witness (MockProver::verify's constraint checks [UP], without its region bookkeeping):
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
#include "check_kernels.hpp"
#include "fp29.cuh"

using namespace bn254;

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
int zk_check_expr(amdzk_ctx* ctx, const ExprArgs& a, uint32_t depth, uint32_t usable, CheckCounters out, const char* name) {
  const size_t shmem = (size_t)(depth ? depth : 1) * EXPR_THREADS * sizeof(Fr);
  const dim3 grid((unsigned)((a.nrows + EXPR_THREADS - 1) / EXPR_THREADS), a.nparts ? a.nparts : 1u), block(EXPR_THREADS);
  if (a.radix261) ZK_FAIL(ctx, AMDZK_E_INVALID, "check_expr: a Lagrange-domain program is needed");
  if (a.nparts > (uint32_t)EXPR_MAX_PARTS) ZK_FAIL(ctx, AMDZK_E_INVALID, "check_expr: too many program parts");
  if (usable > a.nrows || a.nrows > 0xffffffffull) ZK_FAIL(ctx, AMDZK_E_INVALID, "check_expr: bad row counts");
  if (shmem > 65536) ZK_HIP(ctx, hipFuncSetAttribute((const void*)expr_check_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
  ZK_LAUNCH(ctx, name, expr_check_kernel, grid, block, shmem, a, usable, out);
  return AMDZK_OK;
}

int zk_check_lookups(amdzk_ctx* ctx, const Fr* d_inputs, const Fr* d_tables, size_t L, uint32_t n, uint32_t usable, uint32_t first_constraint,
                     CheckCounters out) {
  if (!L || !usable) return AMDZK_OK;
  if (usable > n || L > 65535) ZK_FAIL(ctx, AMDZK_E_INVALID, "check_lookups: bad shape");
  ZK_LAUNCH(ctx, "check_lookup_member", lookup_member_kernel, dim3((usable + 255) / 256, (unsigned)L), dim3(256), 0, d_inputs, d_tables, n, usable,
            first_constraint, out);
  return AMDZK_OK;
}

int zk_sigma_decode(amdzk_ctx* ctx, const Fr* d_sigma, uint32_t S, uint32_t k, const Fr* d_tab, uint2* d_cells, unsigned long long* d_bad) {
  if (!S) return AMDZK_OK;
  if (S > 65535 || k > 31) ZK_FAIL(ctx, AMDZK_E_INVALID, "sigma_decode: bad shape");
  const uint32_t n = 1u << k;
  ZK_LAUNCH(ctx, "check_sigma_decode", sigma_decode_kernel, dim3((n + 255) / 256, S), dim3(256), 0, d_sigma, S, k, n, d_tab, d_cells, d_bad);
  return AMDZK_OK;
}

int zk_check_copies(amdzk_ctx* ctx, const Fr* const* d_cols, const uint2* d_cells, uint32_t S, uint32_t n, uint32_t first_constraint,
                    CheckCounters out) {
  if (!S) return AMDZK_OK;
  if (S > 65535) ZK_FAIL(ctx, AMDZK_E_INVALID, "check_copies: bad shape");
  ZK_LAUNCH(ctx, "check_copies", copy_check_kernel, dim3((n + 255) / 256, S), dim3(256), 0, d_cols, d_cells, n, first_constraint, out);
  return AMDZK_OK;
}
