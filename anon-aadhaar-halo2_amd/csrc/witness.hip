// Witness programs on the device (include/amdzk.h "witness programs"): the kernels and the entry points.
// The host half — validation, levelization, the launch plan and wit::eval_node, which computes a node — is witness.hpp.
//
//   wit_level_kernel    — one level: one work item per (node of the level, proof). The values of a node for the proofs of a
//                         run are adjacent in the slab, so a wavefront's operand loads and its store coalesce over the batch.
//   wit_fused_kernel    — a stretch of consecutive levels of at most wit::FUSED_WIDTH items each, in ONE workgroup with a
//                         workgroup barrier between levels: a deep narrow chain costs barriers, not kernel boundaries.
//   wit_scatter_kernel  — slab -> the named advice cells of every proof; wit_gather_kernel — slab -> the publics' staging.
//   wit_inputs_check_kernel — resident inputs < r, the first offender in a status word; wit_zero_kernel — ZERO_FILL.
//
// Every index a kernel follows was bounded by wit::build (operand slots below the node's own, input and constant indices,
// columns and rows) or is a loop bound of the launch (proofs of the run): nothing is indexed by a computed value.
// Between launches the order is stream order alone; no grid-wide barrier, no spinning on memory.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "common.hpp"
#include "witness.hpp"

using namespace bn254;

struct amdzk_witness {
  wit::Program prog;
  int device = 0;
  wit::Node* d_nodes = nullptr;
  uint32_t* d_level_off = nullptr;
  Fr* d_consts = nullptr;
  wit::Cell* d_cells = nullptr;
  uint32_t* d_publics = nullptr;
  // grow-only: [status word | slab | publics staging], the d_advice pointer table, and the host form's staged inputs
  void* d_ws = nullptr;
  size_t ws_cap = 0;
  void** d_ptrs = nullptr;
  size_t ptrs_cap = 0;
  Fr* d_inputs = nullptr;
  size_t inputs_cap = 0;
};

namespace {

__device__ __forceinline__ Fr wit_ld(const Fr* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 lo = q[0], hi = q[1];
  Fr r;
  r.l[0] = lo.x; r.l[1] = lo.y; r.l[2] = lo.z; r.l[3] = lo.w;
  r.l[4] = hi.x; r.l[5] = hi.y; r.l[6] = hi.z; r.l[7] = hi.w;
  return r;
}
__device__ __forceinline__ void wit_st(Fr* p, const Fr& v) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

struct WitArgs {
  const wit::Node* nodes;
  const Fr* consts;
  const Fr* inputs;     // of the run's first proof
  size_t input_stride;  // Fr per proof
  Fr* slab;             // slot s, proof p of the run at slab[s * P + p]
  uint32_t P;           // proofs of the run
};

// item `it` of the slots [s0, s0 + cnt): slot s0 + it / P, proof it % P. it < cnt * P (the caller checks).
__device__ __forceinline__ void wit_item(const WitArgs& A, uint32_t s0, uint32_t it) {
  const uint32_t s = s0 + it / A.P, p = it % A.P;
  const wit::Node nd = A.nodes[s];
  const uint32_t ar = wit::arity(nd.op);
  Fr a, b = Fr::zero(), c = Fr::zero();
  if (nd.op == AMDZK_W_INPUT) a = wit_ld(A.inputs + (size_t)p * A.input_stride + nd.a);
  else if (nd.op == AMDZK_W_CONST) a = wit_ld(A.consts + nd.a);
  else a = wit_ld(A.slab + (size_t)nd.a * A.P + p);
  if (ar >= 2) b = wit_ld(A.slab + (size_t)nd.b * A.P + p);
  if (ar >= 3) c = wit_ld(A.slab + (size_t)nd.c * A.P + p);
  wit_st(A.slab + (size_t)s * A.P + p, wit::eval_node(nd.op, nd.b, nd.c, a, b, c));
}

__global__ __launch_bounds__(wit::LEVEL_BLOCK) void wit_level_kernel(WitArgs A, uint32_t s0, uint32_t items) {
  const uint32_t it = blockIdx.x * wit::LEVEL_BLOCK + threadIdx.x;
  if (it < items) wit_item(A, s0, it);
}

// levels [l0, l1), each of at most FUSED_WIDTH items: one workgroup, one item per thread and level. The barrier orders the
// level's stores to the slab before the next level's loads (all of them by waves of this one workgroup).
// (Measured and not kept: loading the next level's bounds and node ahead of the barrier, so that only the operand loads and
// the store sit between two barriers — the 10^4-level chain of tools/bench_witness.py took 19.9 ms instead of 14.0.)
__global__ __launch_bounds__(wit::FUSED_WIDTH) void wit_fused_kernel(WitArgs A, const uint32_t* __restrict__ level_off, uint32_t l0, uint32_t l1) {
  uint32_t s0 = level_off[l0];
  for (uint32_t l = l0; l < l1; l++) {
    const uint32_t s1 = level_off[l + 1];
    if (threadIdx.x < (s1 - s0) * A.P) wit_item(A, s0, threadIdx.x);
    s0 = s1;
    __syncthreads();
  }
}

// cell j of proof p: thread p * n_cells + j, so that a wavefront writes neighbouring rows of one column
__global__ __launch_bounds__(wit::LEVEL_BLOCK) void wit_scatter_kernel(const wit::Cell* __restrict__ cells, uint32_t n_cells, const Fr* __restrict__ slab, uint32_t P,
                                                                       void* const* __restrict__ advice, size_t advice_stride) {
  const uint32_t it = blockIdx.x * wit::LEVEL_BLOCK + threadIdx.x;
  if (it >= n_cells * P) return;
  const uint32_t p = it / n_cells;
  const wit::Cell c = cells[it % n_cells];
  wit_st(reinterpret_cast<Fr*>(advice[p]) + (size_t)c.column * advice_stride + c.row, wit_ld(slab + (size_t)c.slot * P + p));
}

__global__ __launch_bounds__(wit::LEVEL_BLOCK) void wit_gather_kernel(const uint32_t* __restrict__ publics, uint32_t n_publics, const Fr* __restrict__ slab, uint32_t P,
                                                                      Fr* __restrict__ out) {
  const uint32_t it = blockIdx.x * wit::LEVEL_BLOCK + threadIdx.x;
  if (it >= n_publics * P) return;
  const uint32_t p = it / n_publics;
  wit_st(out + it, wit_ld(slab + (size_t)publics[it % n_publics] * P + p));
}

// value (b, a) at in[b * stride + a], b < n_proofs, a < n_inputs: *status = the smallest b * n_inputs + a that is >= r
__global__ __launch_bounds__(wit::LEVEL_BLOCK) void wit_inputs_check_kernel(const Fr* __restrict__ in, size_t stride, uint32_t n_inputs, size_t total,
                                                                            unsigned long long* status) {
  for (size_t i = (size_t)blockIdx.x * wit::LEVEL_BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * wit::LEVEL_BLOCK) {
    const Fr v = wit_ld(in + (i / n_inputs) * stride + i % n_inputs);
    if (!is_canonical(v)) atomicMin(status, (unsigned long long)i);
  }
}

// proofs [0, P) x columns [0, ncol) x rows [0, 2^k): the cells and nothing between the columns
__global__ __launch_bounds__(wit::LEVEL_BLOCK) void wit_zero_kernel(void* const* __restrict__ advice, size_t advice_stride, uint32_t k, uint32_t ncol, size_t total) {
  for (size_t i = (size_t)blockIdx.x * wit::LEVEL_BLOCK + threadIdx.x; i < total; i += (size_t)gridDim.x * wit::LEVEL_BLOCK) {
    const size_t row = i & (((size_t)1 << k) - 1), cp = i >> k;
    wit_st(reinterpret_cast<Fr*>(advice[cp / ncol]) + (cp % ncol) * advice_stride + row, Fr::zero());
  }
}

uint32_t wit_blocks(uint64_t items) { return (uint32_t)((items + wit::LEVEL_BLOCK - 1) / wit::LEVEL_BLOCK); }
// grid-stride kernels: enough blocks to fill the chip several times over, never more than the items need
uint32_t wit_stride_blocks(const amdzk_ctx* ctx, uint64_t items) { return (uint32_t)std::min<uint64_t>(wit_blocks(items), (uint64_t)ctx->num_cu * 64); }

template <class T>
int wit_upload(amdzk_ctx* ctx, T** d, const std::vector<T>& h) {
  if (h.empty()) return AMDZK_OK;
  if (hipMalloc((void**)d, h.size() * sizeof(T)) != hipSuccess) ZK_FAIL(ctx, AMDZK_E_NOMEM, "witness: hipMalloc(%zu) failed", h.size() * sizeof(T));
  ZK_HIP(ctx, hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return AMDZK_OK;
}

int wit_grow(amdzk_ctx* ctx, void** p, size_t* cap, size_t bytes) {
  if (*cap >= bytes) return AMDZK_OK;
  if (*p) {
    ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
    ZK_HIP(ctx, hipFree(*p));
    *p = nullptr;
    *cap = 0;
  }
  if (hipMalloc(p, bytes) != hipSuccess) {
    *p = nullptr;
    ZK_FAIL(ctx, AMDZK_E_NOMEM, "witness: hipMalloc(%zu) of the workspace failed", bytes);
  }
  *cap = bytes;
  return AMDZK_OK;
}

void wit_release(amdzk_witness* w) {
  for (void* p : {(void*)w->d_nodes, (void*)w->d_level_off, (void*)w->d_consts, (void*)w->d_cells, (void*)w->d_publics, w->d_ws, (void*)w->d_ptrs, (void*)w->d_inputs})
    if (p) (void)hipFree(p);
  delete w;
}

// d_inputs: resident, proof b at + b * input_stride. checked: the values are known to be < r (the host form looked).
int wit_run(amdzk_ctx* ctx, amdzk_witness* w, size_t n_proofs, const Fr* d_inputs, size_t input_stride, bool checked, void* const* d_advice,
            size_t advice_stride, uint32_t flags, size_t max_scratch_bytes, uint64_t* publics_out) {
  const wit::Program& pr = w->prog;
  if (w->device != ctx->device) ZK_FAIL(ctx, AMDZK_E_INVALID, "witness: the program was compiled on device %d, the ctx is on device %d", w->device, ctx->device);
  if (!d_advice || (pr.n_inputs && !d_inputs)) ZK_FAIL(ctx, AMDZK_E_INVALID, "witness: null argument");
  if (flags & ~AMDZK_WITNESS_ZERO_FILL) ZK_FAIL(ctx, AMDZK_E_INVALID, "witness: unknown flags 0x%x", flags);
  wit::Plan pl;
  std::string err;
  const int rc = wit::plan(pr, n_proofs, max_scratch_bytes, pl, err);
  if (rc != AMDZK_OK) ZK_FAIL(ctx, rc, "%s", err.c_str());
  const size_t n = (size_t)1 << pr.k;
  if (advice_stride < n) ZK_FAIL(ctx, AMDZK_E_INVALID, "witness: advice_stride %zu < 2^k = %zu", advice_stride, n);
  if (input_stride < pr.n_inputs) ZK_FAIL(ctx, AMDZK_E_INVALID, "witness: input_stride %zu < n_inputs = %u", input_stride, pr.n_inputs);
  {
    std::vector<const void*> sorted(d_advice, d_advice + n_proofs);
    std::sort(sorted.begin(), sorted.end());
    if (!sorted[0]) ZK_FAIL(ctx, AMDZK_E_INVALID, "witness: a d_advice pointer is null");
    for (size_t b = 1; b < n_proofs; b++)
      if (sorted[b] == sorted[b - 1]) ZK_FAIL(ctx, AMDZK_E_INVALID, "witness: two proofs share one d_advice buffer");
    for (size_t b = 0; b < n_proofs; b++) {
      const int r = zk_ptr_on_device(ctx, d_advice[b], "d_advice");
      if (r != AMDZK_OK) {
        ctx->err = "witness: " + ctx->err;
        return r == AMDZK_E_HIP ? AMDZK_E_INVALID : r;  // not a pointer the runtime knows
      }
    }
  }
  ZK_TRY(wit_grow(ctx, &w->d_ws, &w->ws_cap, pl.scratch_bytes));
  ZK_TRY(wit_grow(ctx, (void**)&w->d_ptrs, &w->ptrs_cap, n_proofs * sizeof(void*)));
  unsigned long long* d_status = reinterpret_cast<unsigned long long*>(w->d_ws);
  Fr* slab = reinterpret_cast<Fr*>((char*)w->d_ws + wit::SCRATCH_FIXED);
  Fr* d_pub = slab + pr.nodes.size() * pl.per_run;
  hipStream_t st = ctx->stream;
  // AMDZK_WS_POISON (workspace.hpp): the handle's workspace in front of the call, and the slab and the publics in front of every
  // run below (a bounded workspace serves runs of different sizes from one slab). d_ptrs holds addresses: never.
  if (ctx->ws_poison) ZK_TRY(zk_ws_poison_fill(ctx, w->d_ws, pl.scratch_bytes));

  if (!checked && pr.n_inputs) {  // before anything is written anywhere else
    const size_t total = n_proofs * pr.n_inputs;
    ZK_HIP(ctx, hipMemsetAsync(d_status, 0xff, sizeof(unsigned long long), st));
    ZK_LAUNCH(ctx, "wit_inputs_check", wit_inputs_check_kernel, dim3(wit_stride_blocks(ctx, total)), dim3(wit::LEVEL_BLOCK), 0, d_inputs, input_stride,
              pr.n_inputs, total, d_status);
    unsigned long long status = 0;
    ZK_HIP(ctx, hipMemcpyAsync(&status, d_status, sizeof(status), hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, zk_host_wait(ctx, st));
    if (status != ~0ull)
      ZK_FAIL(ctx, AMDZK_E_INVALID, "witness: input %llu of proof %llu is not below the modulus", status % pr.n_inputs, status / pr.n_inputs);
  }
  // the caller's pointer array is read before the call returns: every path below waits for the stream
  ZK_HIP(ctx, hipMemcpyAsync(w->d_ptrs, d_advice, n_proofs * sizeof(void*), hipMemcpyHostToDevice, st));
  if (flags & AMDZK_WITNESS_ZERO_FILL) {
    const size_t total = n_proofs * pr.num_advice * n;
    if (total / n / std::max<size_t>(pr.num_advice, 1) != n_proofs) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "witness: the cells of %zu proofs do not fit size_t", n_proofs);
    if (total)
      ZK_LAUNCH(ctx, "wit_zero", wit_zero_kernel, dim3(wit_stride_blocks(ctx, total)), dim3(wit::LEVEL_BLOCK), 0, w->d_ptrs, advice_stride, pr.k,
                pr.num_advice, total);
  }
  for (size_t done = 0; done < n_proofs;) {
    const uint32_t P = (uint32_t)std::min(pl.per_run, n_proofs - done);
    WitArgs A{w->d_nodes, w->d_consts, d_inputs + done * input_stride, input_stride, slab, P};
    if (ctx->ws_poison && done) ZK_TRY(zk_ws_poison_fill(ctx, slab, pl.scratch_bytes - wit::SCRATCH_FIXED));
    int lrc = AMDZK_OK;
    wit::for_each_launch(pr, P, [&](uint32_t l0, uint32_t l1, bool fused) {
      if (lrc != AMDZK_OK) return;
      lrc = [&]() -> int {
        if (fused) {
          ZK_LAUNCH(ctx, "wit_fused", wit_fused_kernel, dim3(1), dim3(wit::FUSED_WIDTH), 0, A, w->d_level_off, l0, l1);
        } else {
          const uint32_t s0 = pr.level_off[l0], items = (pr.level_off[l1] - s0) * P;  // < 2^31: wit::plan
          ZK_LAUNCH(ctx, "wit_level", wit_level_kernel, dim3(wit_blocks(items)), dim3(wit::LEVEL_BLOCK), 0, A, s0, items);
        }
        return AMDZK_OK;
      }();
    });
    ZK_TRY(lrc);
    if (!pr.cells.empty())
      ZK_LAUNCH(ctx, "wit_scatter", wit_scatter_kernel, dim3(wit_blocks((uint64_t)pr.cells.size() * P)), dim3(wit::LEVEL_BLOCK), 0, w->d_cells,
                (uint32_t)pr.cells.size(), slab, P, w->d_ptrs + done, advice_stride);
    if (!pr.publics.empty()) {
      ZK_LAUNCH(ctx, "wit_gather", wit_gather_kernel, dim3(wit_blocks((uint64_t)pr.publics.size() * P)), dim3(wit::LEVEL_BLOCK), 0, w->d_publics,
                (uint32_t)pr.publics.size(), slab, P, d_pub);
      if (publics_out)
        ZK_HIP(ctx, hipMemcpyAsync(publics_out + done * pr.publics.size() * 4, d_pub, (size_t)P * pr.publics.size() * sizeof(Fr), hipMemcpyDeviceToHost, st));
    }
    done += P;
  }
  ZK_HIP(ctx, zk_host_wait(ctx, st));
  return AMDZK_OK;
}

}  // namespace

extern "C" int amdzk_witness_plan(const amdzk_witness_desc* desc, size_t n_proofs, uint32_t* levels, uint32_t* launches, uint32_t* fused_width,
                                  size_t* scratch_bytes, char* msg, size_t msg_cap) {
  wit::Program pr;
  wit::Plan pl;
  std::string err;
  int rc = wit::build(desc, pr, err);
  if (rc == AMDZK_OK) rc = wit::plan(pr, n_proofs, 0, pl, err);
  if (msg && msg_cap) snprintf(msg, msg_cap, "%s", err.c_str());
  if (rc != AMDZK_OK) return rc;
  if (levels) *levels = pr.levels();
  if (launches) *launches = pl.launches;
  if (fused_width) *fused_width = wit::FUSED_WIDTH;
  if (scratch_bytes) *scratch_bytes = pl.scratch_bytes;
  return AMDZK_OK;
}

extern "C" int amdzk_witness_compile(amdzk_ctx* ctx, const amdzk_witness_desc* desc, amdzk_witness** out) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  if (!desc || !out) ZK_FAIL(ctx, AMDZK_E_INVALID, "witness: null argument");
  *out = nullptr;
  amdzk_witness* w = new amdzk_witness();
  std::string err;
  int rc = wit::build(desc, w->prog, err);
  if (rc != AMDZK_OK) {
    delete w;
    ZK_FAIL(ctx, rc, "%s", err.c_str());
  }
  w->device = ctx->device;
  rc = wit_upload(ctx, &w->d_nodes, w->prog.nodes);
  if (rc == AMDZK_OK) rc = wit_upload(ctx, &w->d_level_off, w->prog.level_off);
  if (rc == AMDZK_OK) rc = wit_upload(ctx, &w->d_consts, w->prog.consts);
  if (rc == AMDZK_OK) rc = wit_upload(ctx, &w->d_cells, w->prog.cells);
  if (rc == AMDZK_OK) rc = wit_upload(ctx, &w->d_publics, w->prog.publics);
  if (rc != AMDZK_OK) {
    wit_release(w);
    return rc;
  }
  *out = w;
  return AMDZK_OK;
}

extern "C" void amdzk_witness_free(amdzk_ctx* ctx, amdzk_witness* w) {
  ZK_ENTER(ctx);
  if (!w) return;
  if (ctx) (void)zk_host_wait(ctx, ctx->stream);
  wit_release(w);
}

extern "C" int amdzk_witness_run_dev(amdzk_ctx* ctx, amdzk_witness* w, size_t n_proofs, const void* d_inputs, size_t input_stride, void* const* d_advice,
                                     size_t advice_stride, uint32_t flags, size_t max_scratch_bytes, uint64_t* publics_out) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  if (!w) ZK_FAIL(ctx, AMDZK_E_INVALID, "witness: null argument");
  return zk_quiet_if_refused(ctx, wit_run(ctx, w, n_proofs, (const Fr*)d_inputs, input_stride, false, d_advice, advice_stride, flags, max_scratch_bytes, publics_out));
}

extern "C" int amdzk_witness_run(amdzk_ctx* ctx, amdzk_witness* w, size_t n_proofs, const uint64_t* const* inputs, void* const* d_advice,
                                 size_t advice_stride, uint32_t flags, size_t max_scratch_bytes, uint64_t* publics_out) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  if (!w || !d_advice || (w->prog.n_inputs && !inputs)) ZK_FAIL(ctx, AMDZK_E_INVALID, "witness: null argument");
  if (n_proofs == 0) ZK_FAIL(ctx, AMDZK_E_INVALID, "witness: n_proofs = 0");
  const uint32_t ni = w->prog.n_inputs;
  if (ni && n_proofs > SIZE_MAX / 32 / ni) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "witness: the inputs of %zu proofs do not fit size_t", n_proofs);
  for (size_t b = 0; b < n_proofs && ni; b++) {
    if (!inputs[b]) ZK_FAIL(ctx, AMDZK_E_INVALID, "witness: inputs[%zu] is null", b);
    for (uint32_t a = 0; a < ni; a++) {
      Fr v;
      memcpy(v.l, inputs[b] + 4 * (size_t)a, 32);
      if (!is_canonical(v)) ZK_FAIL(ctx, AMDZK_E_INVALID, "witness: input %u of proof %zu is not below the modulus", a, b);
    }
  }
  if (ni) {
    ZK_TRY(wit_grow(ctx, (void**)&w->d_inputs, &w->inputs_cap, n_proofs * ni * sizeof(Fr)));
    if (ctx->ws_poison) ZK_TRY(zk_ws_poison_fill(ctx, w->d_inputs, n_proofs * ni * sizeof(Fr)));
    for (size_t b = 0; b < n_proofs; b++)
      ZK_HIP(ctx, hipMemcpyAsync(w->d_inputs + b * ni, inputs[b], (size_t)ni * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
  }
  return zk_quiet_if_refused(ctx, wit_run(ctx, w, n_proofs, w->d_inputs, ni, true, d_advice, advice_stride, flags, max_scratch_bytes, publics_out));
}
