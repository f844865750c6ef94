// A proving key's life: keygen (plonk::keygen::{keygen_vk, keygen_pk} [UP]) from a circuit description and its fixed
// columns with either the copy-constraint mapping or the sigma columns, workspace clones, the key file (pkblob.hpp has its
// layout), inspection and export, and the release of all of it. The circuit arrives as a plain-data description of its
// ConstraintSystem (amdzk_circuit). Control flow and the O(columns) bookkeeping are host code; every O(n) step is a kernel
// of another unit on resident columns. No kernel lives here.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <string>

#include "pk.hpp"

using namespace bn254;

int h2d(amdzk_ctx* ctx, void* d, const void* h, size_t bytes) {
  if (bytes) ZK_HIP(ctx, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ctx->stream));
  return AMDZK_OK;
}
// host -> device through the key's pinned staging area: the source may be a temporary, and the copy
// is truly asynchronous (no pageable-memory staging inside the runtime).
// AMDZK_WS_POISON: the staging ring where its bump pointer goes back to 0 — host memory, filled at once (workspace.hpp): a copy
// still reading the ring would now read the pattern. Counted like every fill.
static void pin_poison(amdzk_ctx* ctx, amdzk_pk* pk) {
  for (size_t i = 0; i < pk->pin_cap / 4; i++) ((uint32_t*)pk->pin)[i] = ZK_WS_POISON_WORD;
  if (ctx->prof) ctx->prof_map["ws_poison"].launches++;
}
int h2d_staged(amdzk_ctx* ctx, amdzk_pk* pk, void* d, const void* h, size_t bytes) {
  if (!bytes) return AMDZK_OK;
  if (!pk->pin || bytes > pk->pin_cap) return h2d(ctx, d, h, bytes);
  size_t off = (pk->pin_off + 63) & ~(size_t)63;
  if (off + bytes > pk->pin_cap) {  // wrap: every stream that may still be reading the staging area must be done with it
    ZK_TRY(zk_sync_all(ctx));
    off = 0;
    if (ctx->ws_poison) pin_poison(ctx, pk);
  }
  memcpy(pk->pin + off, h, bytes);
  pk->pin_off = off + bytes;
  ZK_HIP(ctx, hipMemcpyAsync(d, pk->pin + off, bytes, hipMemcpyHostToDevice, ctx->stream));
  return AMDZK_OK;
}
int d2h(amdzk_ctx* ctx, void* h, const void* d, size_t bytes) {
  if (bytes) {
    ZK_HIP(ctx, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  }
  return AMDZK_OK;
}
int d2d(amdzk_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (bytes) ZK_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return AMDZK_OK;
}

namespace {

// Owns a key from `new amdzk_pk` until it is handed to the caller: an early return in between frees what the key holds by
// then. (ZK_FAIL has set ctx->err before the return runs this; amdzk_pk_free leaves ctx->err alone.)
struct PkFree {
  amdzk_ctx* ctx;
  void operator()(amdzk_pk* pk) const { amdzk_pk_free(ctx, pk); }
};
using PkOwner = std::unique_ptr<amdzk_pk, PkFree>;

}  // namespace

// The per-proof workspace of ONE circuit instance (arenas, lookup / product scratch, multiopen buffers, small staging):
// what a handle allocates, keygen's and a clone's alike.
static int alloc_proof_workspace(amdzk_ctx* ctx, amdzk_pk* pk) {
  const KeyMaterial& K = *pk->key;
  const size_t n = K.n, ext = K.ext;
  const uint32_t L = K.L, ns = K.nsets;
  // a device buffer of the workspace whose content no kernel takes for an address: allocated, and listed for zk_pk_poison
  auto arena = [&](auto** p, size_t count) {
    ZK_TRY(dalloc(ctx, pk, p, count));
    pk->arenas.push_back({(void*)*p, (count ? count : 1) * sizeof(**p)});
    return (int)AMDZK_OK;
  };
  ZK_TRY(arena(&pk->P, K.NP * n));
  ZK_TRY(arena(&pk->PQ, K.NP * n));
  ZK_TRY(arena(&pk->PC, K.NP * ext));
  ZK_TRY(arena(&pk->ci, (size_t)L * n));
  ZK_TRY(arena(&pk->ct, (size_t)L * n));
  ZK_TRY(arena(&pk->lk_ts, (size_t)L * n));
  ZK_TRY(arena(&pk->lk_left, (size_t)L * n));
  ZK_TRY(arena(&pk->lk_flags, (size_t)4 * L * (n + 8)));
  ZK_TRY(arena(&pk->d_err, 1));
  ZK_TRY(arena(&pk->rnd, n));
  ZK_TRY(arena(&pk->hq, (size_t)H_PARTS_MAX * ext));  // one h per piece of the cut h(X) program (finalize_limb_program)
  ZK_TRY(arena(&pk->hpieces, (size_t)K.qdeg * n));
  ZK_TRY(arena(&pk->hpoly, n));
  const size_t nfrac = std::max<size_t>(std::max<size_t>(ns, L), 1);
  ZK_TRY(arena(&pk->frac, nfrac * n));
  ZK_TRY(arena(&pk->scratch, std::max(nfrac * n, ext)));
  ZK_TRY(arena(&pk->scan_tmp, zk_scan_totals_elems(n, nfrac) + 2 * nfrac + 8));
  ZK_TRY(arena(&pk->frac2, std::max<size_t>(L, 1) * n));
  ZK_TRY(arena(&pk->scratch2, std::max<size_t>(L, 1) * n));
  ZK_TRY(arena(&pk->scan_tmp2, zk_scan_totals_elems(n, std::max<size_t>(L, 1)) + 2 * std::max<size_t>(L, 1) + 8));
  const size_t max_rsets = K.max_sets;
  ZK_TRY(arena(&pk->sets_L, max_rsets * n));
  ZK_TRY(arena(&pk->sets_N, max_rsets * n));
  ZK_TRY(arena(&pk->hx, n));
  pk->small_cap = std::max<size_t>((size_t)K.NP * (K.bf + 2) + 4096, 8192);
  for (int l = 0; l < 3; l++) ZK_TRY(arena(&pk->small_l[l], pk->small_cap));
  pk->small = pk->small_l[0];
  pk->pin_cap = std::max<size_t>((size_t)8 << 20, 2 * n * 32);
  if (hipHostMalloc((void**)&pk->pin, pk->pin_cap + 64, hipHostMallocDefault) != hipSuccess) {
    pk->pin = nullptr;
    pk->pin_cap = 0;
    ZK_FAIL(ctx, AMDZK_E_NOMEM, "prover: hipHostMalloc of the pinned staging area failed");
  }
  pk->h_err = (int*)(pk->pin + pk->pin_cap);  // behind the staging ring
  pk->ptrs_cap = 8192;
  for (int l = 0; l < 3; l++) {
    void** pp = nullptr;
    ZK_TRY(dalloc(ctx, pk, &pp, pk->ptrs_cap));
    pk->ptrs_l[l] = pp;
  }
  pk->ptrs = pk->ptrs_l[0];

  return AMDZK_OK;
}

// AMDZK_WS_POISON: every arena of the handle's per-proof workspace filled with the pattern, at the start of a call that
// uses it (create_proof*, the lock-step batch, amdzk_check_witness). Not the pointer-table slices ptrs_l, which kernels
// dereference, nor what a handle keeps from call to call (constant table, column tables, programs, the check's counters) —
// among it the first lk_const columns of ct: the compressed constant lookup tables, written once by build_constant_tables or
// copied by a clone, which the per-proof compression program skips.
// A proof's lanes write the arenas from their own streams: the last call's lanes are waited for in front of the fill and
// the fill is waited for behind it, so that the pattern is in place before any lane starts and over nothing still in use.
int zk_pk_poison(amdzk_ctx* ctx, amdzk_pk* pk) {
  if (!ctx->ws_poison) return AMDZK_OK;
  ZK_TRY(zk_sync_all(ctx));
  if (pk->pin) {  // every stream is idle: the staging ring starts over (pk.hpp), and is filled where it does
    pk->pin_off = 0;
    pin_poison(ctx, pk);
  }
  for (auto& a : pk->arenas) {
    const size_t keep = a.first == (void*)pk->ct ? (size_t)pk->key->lk_const * pk->key->n * sizeof(Fr) : 0;
    if (a.second > keep) ZK_TRY(zk_ws_poison_fill(ctx, (char*)a.first + keep, a.second - keep));
  }
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  return AMDZK_OK;
}

// The slot -> column pointer tables the interpreters read (Lagrange and quotient domain): key columns and this
// workspace's arenas.
static int build_column_tables(amdzk_ctx* ctx, amdzk_pk* pk) {
  const KeyMaterial& K = *pk->key;
  const size_t n = K.n, ext = K.ext;
  const uint32_t F = K.F, A = K.A, I = K.I, S = K.S, L = K.L, ns = K.nsets;
  // ---- column pointer tables
  {
    std::vector<const Fr*> lag(K.nslots_lag()), ex(K.nslots_ext());
    for (uint32_t i = 0; i < F; i++) lag[K.sl_fixed(i)] = K.fixed_lag + (size_t)i * n, ex[i] = K.fixed_coset + (size_t)i * ext;
    for (uint32_t i = 0; i < A; i++) lag[K.sl_adv(i)] = pk->adv() + (size_t)i * n, ex[K.sl_adv(i)] = pk->PC + (size_t)i * ext;
    for (uint32_t i = 0; i < I; i++) lag[K.sl_inst(i)] = pk->inst() + (size_t)i * n, ex[K.sl_inst(i)] = pk->PC + (size_t)(A + i) * ext;
    for (uint32_t i = 0; i < S; i++) lag[K.sl_sigma(i)] = K.sigma_lag + (size_t)i * n, ex[K.se_sigma(i)] = K.sigma_coset + (size_t)i * ext;
    for (uint32_t i = 0; i < S; i++) lag[K.sl_dxw(i)] = K.dxw_lag + (size_t)i * n, ex[K.se_dx(i)] = K.dx_coset + (size_t)i * ext;
    for (uint32_t l = 0; l < L; l++) {
      lag[K.sl_ci(l)] = pk->ci + (size_t)l * n;
      lag[K.sl_ct(l)] = pk->ct + (size_t)l * n;
      lag[K.sl_la(l)] = pk->la() + (size_t)l * n;
      lag[K.sl_ls(l)] = pk->ls() + (size_t)l * n;
      ex[K.se_la(l)] = pk->PC + (size_t)(A + I + l) * ext;
      ex[K.se_ls(l)] = pk->PC + (size_t)(A + I + L + l) * ext;
      ex[K.se_zl(l)] = pk->PC + (size_t)(A + I + 2 * L + ns + l) * ext;
    }
    for (uint32_t s = 0; s < ns; s++) ex[K.se_zp(s)] = pk->PC + (size_t)(A + I + 2 * L + s) * ext;
    lag[K.sl_omega()] = K.omega_pow;
    ex[K.se_l0()] = K.l0_c;
    ex[K.se_llast()] = K.llast_c;
    ex[K.se_lactive()] = K.lactive_c;
    ex[K.se_x()] = K.x_coset;
    pk->h_cols_lag = lag;
    pk->h_cols_ext = ex;
    ZK_TRY(dalloc(ctx, pk, &pk->d_cols_lag, lag.size()));
    ZK_TRY(dalloc(ctx, pk, &pk->d_cols_ext, ex.size()));
    ZK_TRY(h2d(ctx, pk->d_cols_lag, lag.data(), lag.size() * sizeof(Fr*)));
    ZK_TRY(h2d(ctx, pk->d_cols_ext, ex.data(), ex.size() * sizeof(Fr*)));
    // the permutation columns' values, in the permutation's order (the sparse products and the copy check read them by row)
    std::vector<const Fr*> pv(S);
    for (uint32_t i = 0; i < S; i++) {
      const std::pair<int, int>& kc = K.perm_cols[i];
      pv[i] = lag[kc.first == 0 ? K.sl_adv(kc.second) : kc.first == 1 ? K.sl_fixed(kc.second) : K.sl_inst(kc.second)];
    }
    ZK_TRY(dalloc(ctx, pk, &pk->d_perm_cols, pv.size()));
    ZK_TRY(h2d(ctx, pk->d_perm_cols, pv.data(), pv.size() * sizeof(Fr*)));
    ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  }

  return AMDZK_OK;
}

// Where the Lagrange-domain programs store: compressed lookup inputs / tables, permutation fractions, lookup fractions.
static int build_output_tables(amdzk_ctx* ctx, amdzk_pk* pk) {
  const KeyMaterial& K = *pk->key;
  const size_t n = K.n;
  const uint32_t L = K.L, ns = K.nsets;
  {
    std::vector<Fr*> outs(2 * L);
    for (uint32_t l = 0; l < L; l++) outs[2 * l] = pk->ci + (size_t)l * n, outs[2 * l + 1] = pk->ct + (size_t)l * n;
    ZK_TRY(dalloc(ctx, pk, &pk->d_outs_compress, outs.size()));
    ZK_TRY(h2d(ctx, pk->d_outs_compress, outs.data(), outs.size() * sizeof(Fr*)));
    ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  }
  {
    std::vector<Fr*> outs(2 * ns);
    for (uint32_t s = 0; s < ns; s++) outs[2 * s] = pk->frac + (size_t)s * n, outs[2 * s + 1] = pk->zp() + (size_t)s * n;
    ZK_TRY(dalloc(ctx, pk, &pk->d_outs_pfrac, outs.size()));
    ZK_TRY(h2d(ctx, pk->d_outs_pfrac, outs.data(), outs.size() * sizeof(Fr*)));
    ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  }
  {
    std::vector<Fr*> outs(2 * L);
    for (uint32_t l = 0; l < L; l++) outs[2 * l] = pk->frac2 + (size_t)l * n, outs[2 * l + 1] = pk->zl() + (size_t)l * n;  // frac2: beside the permutation products
    ZK_TRY(dalloc(ctx, pk, &pk->d_outs_lfrac, outs.size()));
    ZK_TRY(h2d(ctx, pk->d_outs_lfrac, outs.data(), outs.size() * sizeof(Fr*)));
    ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  }
  return AMDZK_OK;
}

// What a key handle holds for ITS workspace besides the arenas: the pointer tables, the constant tables, the powers of
// y, and the four programs resolved to this workspace's addresses. Keygen and amdzk_pk_clone_workspace both go through it.
static int bind_workspace(amdzk_ctx* ctx, amdzk_pk* pk) {
  const KeyMaterial& K = *pk->key;
  pk->consts = K.consts;
  pk->prog_compress.text = &K.prog_compress, pk->prog_pfrac.text = &K.prog_pfrac, pk->prog_lfrac.text = &K.prog_lfrac, pk->prog_h.text = &K.prog_h;
  ZK_TRY(build_column_tables(ctx, pk));
  ZK_TRY(build_output_tables(ctx, pk));
  ZK_TRY(dalloc(ctx, pk, &pk->d_consts, pk->consts.size()));
  ZK_TRY(h2d(ctx, pk->d_consts, pk->consts.data(), pk->consts.size() * 32));
  ZK_TRY(dalloc(ctx, pk, &pk->d_consts261, pk->consts.size()));
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  ZK_TRY(upload_program(ctx, pk, pk->prog_compress, false));
  ZK_TRY(upload_program(ctx, pk, pk->prog_pfrac, false));
  ZK_TRY(upload_program(ctx, pk, pk->prog_lfrac, false));
  ZK_TRY(dalloc(ctx, pk, &pk->d_ypow, (size_t)std::max<uint32_t>(K.h_terms, 1)));
  ZK_TRY(upload_program(ctx, pk, pk->prog_h, true));
  return upload_consts261(ctx, pk);
}

// ---- keygen, step by step (keygen_common below runs them in this order; amdzk_keygen_vk, vk.hip, runs the ones pk.hpp
// declares). K: the material under construction; pk: the handle keygen will return, where a step works in its workspace.

// The phase table the way ConstraintSystem::{advice_column_in, challenge_usable_after} assert [UP], the flags and the null
// arguments: pure checks, before anything is allocated. *nphases: the number of phases the table uses (1 without one).
int check_keygen_args(amdzk_ctx* ctx, const amdzk_srs* srs, const amdzk_circuit* c, const amdzk_phases* ph, const uint64_t transcript_repr[4],
                      uint32_t flags, const void* out, uint32_t* nphases) {
  *nphases = 1;
  if (ph && c) {
    if ((c->num_advice && !ph->advice_phase) || (ph->num_challenges && !ph->challenge_phase))
      ZK_FAIL(ctx, AMDZK_E_INVALID, "keygen: phase table has a null array");
    bool has[3] = {false, false, false};
    for (uint32_t a = 0; a < c->num_advice; a++) {
      if (ph->advice_phase[a] > 2) ZK_FAIL(ctx, AMDZK_E_INVALID, "keygen: advice column %u is in phase %u (phases are 0, 1, 2)", a, ph->advice_phase[a]);
      has[ph->advice_phase[a]] = true;
    }
    for (uint32_t p = 1; p < 3; p++)
      if (has[p]) {
        if (!has[p - 1]) ZK_FAIL(ctx, AMDZK_E_INVALID, "keygen: phase %u has advice columns but phase %u has none", p, p - 1);
        *nphases = p + 1;
      }
    for (uint32_t i = 0; i < ph->num_challenges; i++) {
      const uint32_t p = ph->challenge_phase[i];
      if (p > 2) ZK_FAIL(ctx, AMDZK_E_INVALID, "keygen: challenge %u is usable after phase %u (phases are 0, 1, 2)", i, p);
      if (!has[p]) ZK_FAIL(ctx, AMDZK_E_INVALID, "keygen: challenge %u is usable after phase %u, which has no advice column", i, p);
    }
    if (c->expr_offsets && c->expr_words)
      for (uint32_t i = 0; i < c->expr_offsets[c->num_exprs]; i++)
        if ((c->expr_words[i] >> 24) == XOP_CHALLENGE && (c->expr_words[i] & 0xffffffu) >= ph->num_challenges)
          ZK_FAIL(ctx, AMDZK_E_INVALID, "keygen: challenge index %u out of range (num_challenges = %u)", c->expr_words[i] & 0xffffffu,
                  ph->num_challenges);
  }
  if (flags & ~(uint32_t)(AMDZK_KEYGEN_FULL_COSETS | AMDZK_KEYGEN_SERIAL)) ZK_FAIL(ctx, AMDZK_E_INVALID, "keygen: unknown flags %#x", flags);
  if (!srs || !c || !out || !transcript_repr) ZK_FAIL(ctx, AMDZK_E_INVALID, "keygen: null argument");
  if (c->cs_degree < 3) ZK_FAIL(ctx, AMDZK_E_INVALID, "keygen: cs_degree %u < 3", c->cs_degree);
  return AMDZK_OK;
}

// The circuit description into the key — shape, domain, queries, expressions, the key file's header — and the layout of
// the constant table. vk_only (amdzk_keygen_vk, vk.hip): the key will only commit to its fixed and permutation columns —
// no prefix basis, no quotient plan, no extended domain (ext stays 0).
int describe_circuit(amdzk_ctx* ctx, KeyMaterial& K, const amdzk_srs* srs, const amdzk_circuit* c, const amdzk_phases* ph, uint32_t nphases,
                     const uint64_t transcript_repr[4], uint32_t flags, bool vk_only) {
  K.srs = srs;
  K.k = c->k;
  K.n = (size_t)1 << c->k;
  K.bf = c->blinding_factors;
  K.degree = c->cs_degree;
  K.F = c->num_fixed;
  K.A = c->num_advice;
  K.I = c->num_instance;
  K.S = c->num_perm_columns;
  K.L = c->num_lookups;
  K.chunk = K.degree - 2;
  K.nsets = (K.S + K.chunk - 1) / K.chunk;
  K.qdeg = K.degree - 1;
  K.NP = (size_t)K.A + K.I + 2 * K.L + K.nsets + K.L;
  if (K.S && !vk_only) ZK_TRY(zk_srs_ensure_prefix(ctx, srs));  // the permutation products are committed over it (Prover::perm_commit)
  if (ph) {
    K.nphases = nphases;
    K.num_challenges = ph->num_challenges;
    K.advice_phase.assign(ph->advice_phase, ph->advice_phase + (c->num_advice ? c->num_advice : 0));
    K.challenge_phase.assign(ph->challenge_phase, ph->challenge_phase + ph->num_challenges);
  }
  if (K.n < K.bf + 3) ZK_FAIL(ctx, AMDZK_E_INVALID, "keygen: not enough rows (n = %zu, blinding factors = %u)", K.n, K.bf);
  memcpy(K.transcript_repr.l, transcript_repr, 32);
  ZK_TRY(amdzk_domain_new(ctx, K.degree, K.k, &K.dom));
  K.ek = amdzk_domain_extended_k(K.dom);
  // h(X) has qdeg = degree - 1 pieces: that many cosets pin it down (AMDZK_FULL_COSETS=1: all 2^(ek-k), upstream's own
  // computation — identical output for satisfying witnesses, and the way to reproduce upstream's bytes for others)
  K.nc = (flags & AMDZK_KEYGEN_FULL_COSETS) ? (1u << (K.ek - K.k)) : K.qdeg;
  K.use_lanes = !(flags & AMDZK_KEYGEN_SERIAL);
  if (!vk_only) {
    ZK_TRY(zk_quotient_plan(ctx, K.dom, K.nc));
    K.ext = (size_t)K.nc * K.n;
  }
  amdzk_domain_constant(K.dom, 0, (uint64_t*)K.omega.l);
  amdzk_domain_constant(K.dom, 1, (uint64_t*)K.omega_inv.l);
  for (uint32_t i = 0; i < c->num_advice_queries; i++) K.advice_queries.push_back({c->advice_queries[2 * i], c->advice_queries[2 * i + 1]});
  for (uint32_t i = 0; i < c->num_fixed_queries; i++) K.fixed_queries.push_back({c->fixed_queries[2 * i], c->fixed_queries[2 * i + 1]});
  for (uint32_t i = 0; i < c->num_instance_queries; i++)
    K.instance_queries.push_back({c->instance_queries[2 * i], c->instance_queries[2 * i + 1]});
  for (uint32_t i = 0; i < K.S; i++) K.perm_cols.push_back({(int)c->perm_columns[2 * i], (int)c->perm_columns[2 * i + 1]});
  K.num_gates = c->num_gates;
  uint32_t nexpr = c->num_gates;
  for (uint32_t l = 0; l < K.L; l++) {
    K.lookup_shape.push_back({c->lookup_shape[2 * l], c->lookup_shape[2 * l + 1]});
    nexpr += c->lookup_shape[2 * l] + c->lookup_shape[2 * l + 1];
  }
  if (nexpr != c->num_exprs) ZK_FAIL(ctx, AMDZK_E_INVALID, "keygen: expression count mismatch (%u vs %u)", nexpr, c->num_exprs);
  for (uint32_t e = 0; e < c->num_exprs; e++)
    K.exprs.emplace_back(c->expr_words + c->expr_offsets[e], c->expr_words + c->expr_offsets[e + 1]);
  {
    auto desc = std::make_shared<pkblob::Desc>();
    desc->assign(*c, ph);
    K.src_desc = desc;
  }
  // constants: circuit | one theta beta gamma y 1/beta
  K.consts.resize(c->num_constants);
  if (c->num_constants) memcpy(K.consts.data(), c->constants, (size_t)c->num_constants * 32);
  K.c_one = c->num_constants;
  K.c_theta = K.c_one + 1;
  K.c_beta = K.c_one + 2;
  K.c_gamma = K.c_one + 3;
  K.c_y = K.c_one + 4;
  K.c_betainv = K.c_one + 5;
  K.c_chal0 = K.c_betainv + 1;
  K.consts.resize((size_t)K.c_chal0 + K.num_challenges, Fr::zero());
  K.consts[K.c_one] = Fr::one();
  return AMDZK_OK;
}

// The key material's device buffers — fixed and permutation columns in their three forms, the domain columns — and the
// per-proof workspace of keygen's handle, which the steps below borrow.
static int alloc_key_material(amdzk_ctx* ctx, KeyMaterial& K, amdzk_pk* pk) {
  const size_t n = K.n, ext = K.ext;
  const uint32_t F = K.F, S = K.S;
  ZK_TRY(dalloc(ctx, &K, &K.fixed_lag, (size_t)F * n));
  ZK_TRY(dalloc(ctx, &K, &K.fixed_poly, (size_t)F * n));
  ZK_TRY(dalloc(ctx, &K, &K.fixed_coset, (size_t)F * ext));
  ZK_TRY(dalloc(ctx, &K, &K.sigma_lag, (size_t)S * n));
  ZK_TRY(dalloc(ctx, &K, &K.sigma_poly, (size_t)S * n));
  ZK_TRY(dalloc(ctx, &K, &K.sigma_coset, (size_t)S * ext));
  ZK_TRY(dalloc(ctx, &K, &K.l0_c, ext));
  ZK_TRY(dalloc(ctx, &K, &K.llast_c, ext));
  ZK_TRY(dalloc(ctx, &K, &K.lactive_c, ext));
  ZK_TRY(dalloc(ctx, &K, &K.x_coset, ext));
  ZK_TRY(dalloc(ctx, &K, &K.omega_pow, n));
  ZK_TRY(dalloc(ctx, &K, &K.dxw_lag, (size_t)S * n));
  ZK_TRY(dalloc(ctx, &K, &K.dx_coset, (size_t)S * ext));
  return alloc_proof_workspace(ctx, pk);
}

// The columns that depend on the domain alone: omega powers; l_0, l_last and l_blind on the cosets (l_blind in lactive_c,
// until finish_l_active); the cosets' points; the identity permutation.
static int build_domain_columns(amdzk_ctx* ctx, KeyMaterial& K, amdzk_pk* pk) {
  const size_t n = K.n, ext = K.ext;
  std::vector<Fr> op(n), l0(n, Fr::zero()), ll(n, Fr::zero()), lb(n, Fr::zero()), xc(ext);
  // the copies below read these vectors asynchronously: a step that fails between a copy and its wait still leaves the
  // stream idle before they go away
  struct IdleOnExit {
    amdzk_ctx* ctx;
    ~IdleOnExit() { (void)zk_host_wait(ctx, ctx->stream); }
  } idle{ctx};
  Fr cur = Fr::one();
  for (size_t i = 0; i < n; i++) {
    op[i] = cur;
    cur = mul(cur, K.omega);
  }
  ZK_TRY(h2d(ctx, K.omega_pow, op.data(), n * 32));
  l0[0] = Fr::one();
  ll[n - K.bf - 1] = Fr::one();
  for (size_t i = n - K.bf; i < n; i++) lb[i] = Fr::one();
  // to cosets via the same device path as every other polynomial, one column at a time through pk->scratch
  Fr* tmp = pk->scratch;
  Fr* dst[3] = {K.l0_c, K.llast_c, K.lactive_c};
  std::vector<Fr>* src[3] = {&l0, &ll, &lb};
  for (int t = 0; t < 3; t++) {
    ZK_TRY(h2d(ctx, tmp, src[t]->data(), n * 32));
    ZK_TRY(amdzk_lagrange_to_coeff_dev(ctx, K.dom, tmp, 1, n));
    ZK_TRY(zk_coeff_to_cosets_r261(ctx, K.dom, tmp, n, dst[t], ext, 1));
    ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  }
  for (uint32_t c = 0; c < K.nc; c++) {
    cur = zk_quotient_coset_g(K.dom, c);
    for (int i = 0; i < 5; i++) cur = add(cur, cur);  // 32 * g_c * omega^i: the points of coset c in radix 2^261
    for (size_t i = 0; i < n; i++) {
      xc[(size_t)c * n + i] = cur;
      cur = mul(cur, K.omega);
    }
  }
  ZK_TRY(h2d(ctx, K.x_coset, xc.data(), ext * 32));
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  // the identity permutation: delta^j * omega^i (Lagrange) and delta^j * X on the cosets (same radix as x_coset)
  Fr dj = Fr::one();
  const Fr delta = fr_delta();
  for (uint32_t j = 0; j < K.S; j++) {
    ZK_TRY(d2d(ctx, K.dxw_lag + (size_t)j * n, K.omega_pow, n * 32));
    ZK_TRY(d2d(ctx, K.dx_coset + (size_t)j * ext, K.x_coset, ext * 32));
    if (j) {
      ZK_TRY(zk_scale(ctx, K.dxw_lag + (size_t)j * n, n, dj));
      ZK_TRY(zk_scale(ctx, K.dx_coset + (size_t)j * ext, ext, dj));
    }
    dj = mul(dj, delta);
  }
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  return AMDZK_OK;
}

// The fixed columns: Lagrange values as given, coefficients and cosets where the material has them (a verifying key's
// has the Lagrange values alone), commitments.
int load_fixed_columns(amdzk_ctx* ctx, KeyMaterial& K, const void* fixed_values) {
  const size_t n = K.n;
  const uint32_t F = K.F;
  if (!F) return AMDZK_OK;
  if (!fixed_values) ZK_FAIL(ctx, AMDZK_E_INVALID, "keygen: fixed_values is null");
  ZK_TRY(h2d(ctx, K.fixed_lag, fixed_values, (size_t)F * n * 32));
  if (K.fixed_poly) {
    ZK_TRY(d2d(ctx, K.fixed_poly, K.fixed_lag, (size_t)F * n * 32));
    ZK_TRY(amdzk_lagrange_to_coeff_dev(ctx, K.dom, K.fixed_poly, F, n));
    ZK_TRY(zk_coeff_to_cosets_r261(ctx, K.dom, K.fixed_poly, n, K.fixed_coset, K.ext, F));
  }
  return commit_cols(ctx, K, AMDZK_BASIS_G_LAGRANGE, K.fixed_lag, F, K.fixed_commitments);
}

// The permutation columns: their Lagrange values from the mapping or as given, then what both routes share, as for the
// fixed columns.
int load_sigma_columns(amdzk_ctx* ctx, KeyMaterial& K, const uint32_t* perm_mapping, const void* sigma_values, bool from_sigma) {
  const size_t n = K.n;
  const uint32_t S = K.S;
  if (!S) return AMDZK_OK;
  if (from_sigma) {
    if (!sigma_values) ZK_FAIL(ctx, AMDZK_E_INVALID, "keygen: sigma_values is null");
    ZK_TRY(h2d(ctx, K.sigma_lag, sigma_values, (size_t)S * n * 32));
    ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  } else {
    if (!perm_mapping) ZK_FAIL(ctx, AMDZK_E_INVALID, "keygen: perm_mapping is null");
    // sigma_i(omega^j) = delta^(i') * omega^(j'), (i', j') = mapping[i][j]
    std::vector<Fr> dpow(S), op(n), sig((size_t)S * n);
    Fr delta = fr_delta(), cur = Fr::one();
    for (uint32_t i = 0; i < S; i++) {
      dpow[i] = cur;
      cur = mul(cur, delta);
    }
    cur = Fr::one();
    for (size_t i = 0; i < n; i++) {
      op[i] = cur;
      cur = mul(cur, K.omega);
    }
    for (uint32_t i = 0; i < S; i++)
      for (size_t j = 0; j < n; j++) {
        uint32_t pi = perm_mapping[2 * ((size_t)i * n + j)], pj = perm_mapping[2 * ((size_t)i * n + j) + 1];
        if (pi >= S || pj >= n) ZK_FAIL(ctx, AMDZK_E_INVALID, "keygen: permutation mapping out of range");
        sig[(size_t)i * n + j] = mul(dpow[pi], op[pj]);
      }
    ZK_TRY(h2d(ctx, K.sigma_lag, sig.data(), (size_t)S * n * 32));
    ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  }
  if (K.sigma_poly) {
    ZK_TRY(d2d(ctx, K.sigma_poly, K.sigma_lag, (size_t)S * n * 32));
    ZK_TRY(amdzk_lagrange_to_coeff_dev(ctx, K.dom, K.sigma_poly, S, n));
    ZK_TRY(zk_coeff_to_cosets_r261(ctx, K.dom, K.sigma_poly, n, K.sigma_coset, K.ext, S));
  }
  return commit_cols(ctx, K, AMDZK_BASIS_G_LAGRANGE, K.sigma_lag, S, K.perm_commitments);
}

// The cells that can change a permutation product (KeyMaterial::perm_rank / perm_off / perm_list), from the sigma columns
// against the identity permutation's, on the device: flags, one scan per set, the sets' totals to the host for the
// offsets, compaction. Every maker of a key comes through here, so a key read from a file or built from sigma has them too.
static int build_perm_lists(amdzk_ctx* ctx, KeyMaterial& K) {
  const uint32_t S = K.S, ns = K.nsets, u = (uint32_t)(K.n - K.bf - 1);
  if (!S) return AMDZK_OK;
  const size_t cells = (size_t)ns * (u + 1);
  uint32_t* flags = nullptr;  // only needed here
  if (hipMalloc((void**)&flags, cells * sizeof(uint32_t)) != hipSuccess) ZK_FAIL(ctx, AMDZK_E_NOMEM, "keygen: hipMalloc of the permutation flags failed");
  struct FreeOnExit {
    amdzk_ctx* ctx;
    void* p;
    ~FreeOnExit() {
      (void)zk_host_wait(ctx, ctx->stream);
      hipFree(p);
    }
  } guard{ctx, flags};
  ZK_TRY(dalloc(ctx, &K, &K.perm_rank, cells));
  ZK_TRY(dalloc(ctx, &K, &K.perm_off, (size_t)ns + 1));
  ZK_TRY(zk_perm_rank(ctx, K.sigma_lag, K.dxw_lag, K.n, u, S, K.chunk, ns, flags, K.perm_rank));
  std::vector<uint32_t> off((size_t)ns + 1, 0);  // the sets' totals (rank[s][u]), then their running sum
  ZK_HIP(ctx, hipMemcpy2DAsync(off.data() + 1, sizeof(uint32_t), K.perm_rank + u, ((size_t)u + 1) * sizeof(uint32_t), sizeof(uint32_t), ns,
                               hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  for (uint32_t s = 0; s < ns; s++) off[s + 1] += off[s];
  K.perm_m = off[ns];
  // Per listed cell the sparse route costs about what the dense one costs per row: it runs up to half the cells. Its
  // arrays (m + 1 numerators and as many denominators) live in the dense route's fraction columns, ns * n elements.
  K.perm_sparse = 2 * K.perm_m <= (size_t)ns * u && 2 * (K.perm_m + 1) <= (size_t)ns * K.n;
  ZK_TRY(h2d(ctx, K.perm_off, off.data(), off.size() * sizeof(uint32_t)));
  if (K.perm_sparse) {
    ZK_TRY(dalloc(ctx, &K, &K.perm_list, K.perm_m));
    ZK_TRY(zk_perm_compact(ctx, flags, K.perm_rank, K.perm_off, u, ns, K.perm_list));
  }
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));  // `off` is a host temporary
  return AMDZK_OK;
}

// ---- the four programs of a key. A column operand is slot << 8 | index into the key's rotation table; fixed, advice and
// instance columns have the same slot in the Lagrange and in the extended table.
static uint32_t COL(uint32_t slot, uint32_t r) { return (slot << 8) | r; }
static uint32_t perm_col_slot(const KeyMaterial& K, uint32_t j) {
  const std::pair<int, int> kc = K.perm_cols[j];
  return kc.first == 0 ? K.sl_adv(kc.second) : kc.first == 1 ? K.sl_fixed(kc.second) : K.sl_inst(kc.second);
}
// w_j = (v_j + gamma) / beta of the permutation columns lo <= j < hi, one after the other onto the stack
static void emit_perm_w(KeyMaterial& K, ProgramText& pr, uint32_t lo, uint32_t hi) {
  for (uint32_t j = lo; j < hi; j++) {
    pr.op(OP_PUSH_COL, COL(perm_col_slot(K, j), K.rots.index(0)));
    pr.push();
    pr.op(OP_ADD_CONST, K.c_gamma);
    pr.op(OP_MUL_CONST, K.c_betainv);
  }
}

// (1) lookup compression: ci[l], ct[l]. Leading lookups whose table is one expression over fixed columns and constants
// (KeyMaterial::lk_const) get ct[l] once, in build_constant_tables.
static int emit_compress_program(amdzk_ctx* ctx, KeyMaterial& K) {
  ProgramText& pr = K.prog_compress;
  const uint32_t L = K.L;
  uint32_t e = K.num_gates;
  for (uint32_t l = 0; l < L && !getenv("AMDZK_NO_TABLE_CACHE"); l++) {
    const uint32_t ni = K.lookup_shape[l].first, nt = K.lookup_shape[l].second;
    bool constant = nt == 1;
    if (constant)
      for (uint32_t w : K.exprs[e + ni]) constant = constant && (w >> 24) != XOP_ADVICE && (w >> 24) != XOP_INSTANCE && (w >> 24) != XOP_CHALLENGE;
    if (!constant) break;
    K.lk_const++;
    e += ni + nt;
  }
  e = K.num_gates;
  for (uint32_t l = 0; l < L; l++) {
    pr.piece();
    ZK_TRY(emit_compressed(ctx, K, pr, e, K.lookup_shape[l].first));
    pr.op(OP_STORE, 2 * l);
    pr.pop();
    e += K.lookup_shape[l].first;
    if (l >= K.lk_const) {
      ZK_TRY(emit_compressed(ctx, K, pr, e, K.lookup_shape[l].second));
      pr.op(OP_STORE, 2 * l + 1);
      pr.pop();
    }
    e += K.lookup_shape[l].second;
  }
  return AMDZK_OK;
}

// (2) permutation fractions: den[s] -> frac column s (inverted later), num[s] -> zp column s. Per set: the columns'
// w_j = (v_j + gamma) / beta stay on the stack and serve both products, prod_j (sigma_j + w_j) and
// prod_j (delta^j omega^row + w_j); the common factor beta^m of numerator and denominator cancels in num / den.
static void emit_pfrac_program(KeyMaterial& K) {
  ProgramText& pr = K.prog_pfrac;
  const uint32_t r0 = K.rots.index(0);
  for (uint32_t s = 0; s < K.nsets; s++) {
    const uint32_t lo = s * K.chunk, hi = std::min(K.S, lo + K.chunk), m = hi - lo;
    pr.piece();
    emit_perm_w(K, pr, lo, hi);
    for (int side = 0; side < 2; side++) {  // 0: denominator (sigma columns), 1: numerator (identity-permutation columns)
      for (uint32_t j = lo; j < hi; j++) {
        // the stack holds the m values w, then (from the second factor on) the running product
        pr.op(OP_PICK, j == lo ? m - 1 : m - (j - lo));
        pr.push();
        pr.op(OP_ADD_COL, COL(side == 0 ? K.sl_sigma(j) : K.sl_dxw(j), r0));
        if (j > lo) {
          pr.op(OP_MUL);
          pr.pop();
        }
      }
      if (side == 1) {
        pr.op(OP_NIP, m);
        pr.cur -= m;
      }
      pr.op(OP_STORE, 2 * s + side);
      pr.pop();
    }
  }
}

// (3) lookup fractions: den = (a'+beta)(s'+gamma) -> frac2[l]; num = (ci+beta)(ct+gamma) -> zl[l]
static void emit_lfrac_program(KeyMaterial& K) {
  ProgramText& pr = K.prog_lfrac;
  const uint32_t r0 = K.rots.index(0);
  for (uint32_t l = 0; l < K.L; l++) {
    pr.piece();
    pr.op(OP_PUSH_COL, COL(K.sl_la(l), r0));
    pr.push();
    pr.op(OP_ADD_CONST, K.c_beta);
    pr.op(OP_PUSH_COL, COL(K.sl_ls(l), r0));
    pr.push();
    pr.op(OP_ADD_CONST, K.c_gamma);
    pr.op(OP_MUL);
    pr.pop();
    pr.op(OP_STORE, 2 * l);
    pr.pop();
    pr.op(OP_PUSH_COL, COL(K.sl_ci(l), r0));
    pr.push();
    pr.op(OP_ADD_CONST, K.c_beta);
    pr.op(OP_PUSH_COL, COL(K.sl_ct(l), r0));
    pr.push();
    pr.op(OP_ADD_CONST, K.c_gamma);
    pr.op(OP_MUL);
    pr.pop();
    pr.op(OP_STORE, 2 * l + 1);
    pr.pop();
  }
}

// (4) the h(X) numerator: gates, permutation, lookups — evaluation.rs evaluate_h order — then the pass that readies it
// for the limb-resident interpreter and cuts it into pieces.
static int emit_h_program(amdzk_ctx* ctx, KeyMaterial& K) {
  ProgramText& pr = K.prog_h;
  const uint32_t S = K.S, L = K.L, ns = K.nsets;
  const uint32_t r0 = K.rots.index(0), r1 = K.rots.index(1), rm1 = K.rots.index(-1), rlast = K.rots.index(-(int32_t)(K.bf + 1));
  pr.uses_hot = true;
  for (uint32_t g = 0; g < K.num_gates; g++) {
    ZK_TRY(emit_expr(ctx, K, &K.rots, pr, K.exprs[g]));
    pr.op(OP_ACC);
    pr.pop();
  }
  if (ns > 0) {
    // l_0 * (1 - z_0)
    pr.op(OP_PUSH_CONST, K.c_one); pr.push();
    pr.op(OP_SUB_COL, COL(K.se_zp(0), r0));
    pr.op(OP_MUL_HOT, 0);
    pr.op(OP_ACC); pr.pop();
    // l_last * (z_l^2 - z_l)
    pr.op(OP_PUSH_COL, COL(K.se_zp(ns - 1), r0)); pr.push();
    pr.op(OP_SQR);
    pr.op(OP_SUB_COL, COL(K.se_zp(ns - 1), r0));
    pr.op(OP_MUL_HOT, 1);
    pr.op(OP_ACC); pr.pop();
    // l_0 * (z_i - z_{i-1}(omega^last X))
    for (uint32_t s = 1; s < ns; s++) {
      pr.op(OP_PUSH_COL, COL(K.se_zp(s), r0)); pr.push();
      pr.op(OP_SUB_COL, COL(K.se_zp(s - 1), rlast));
      pr.op(OP_MUL_HOT, 0);
      pr.op(OP_ACC); pr.pop();
    }
    // l_active * (z_i(omega X) prod(v + beta sigma + gamma) - z_i(X) prod(v + beta delta^j X + gamma))
    //   = beta^m * l_active * (z_i(omega X) prod(sigma_j + w_j) - z_i(X) prod(delta^j X + w_j)),  w_j = (v_j + gamma) / beta:
    // the w_j stay on the stack for both products (one product per column instead of two), delta^j X is a key column,
    // and beta^m goes into the term's power of y (h_term_beta_pow, upload_ypow)
    for (uint32_t s = 0; s < ns; s++) {
      const uint32_t lo = s * K.chunk, hi = std::min(S, lo + K.chunk), m = hi - lo;
      emit_perm_w(K, pr, lo, hi);
      pr.op(OP_PUSH_COL, COL(K.se_zp(s), r1)); pr.push();
      for (uint32_t j = lo; j < hi; j++) {
        pr.op(OP_PICK, m - (j - lo)); pr.push();
        pr.op(OP_ADD_COL, COL(K.se_sigma(j), r0));
        pr.op(OP_MUL); pr.pop();
      }
      pr.op(OP_PUSH_COL, COL(K.se_zp(s), r0)); pr.push();
      for (uint32_t j = lo; j < hi; j++) {
        pr.op(OP_PICK, 1 + m - (j - lo)); pr.push();
        pr.op(OP_ADD_COL, COL(K.se_dx(j), r0));
        pr.op(OP_MUL); pr.pop();
      }
      pr.op(OP_SUB); pr.pop();
      pr.op(OP_NIP, m); pr.cur -= m;
      pr.op(OP_MUL_HOT, 2);
      pr.next_beta = m;
      pr.op(OP_ACC); pr.pop();
    }
  }
  uint32_t e = K.num_gates;
  for (uint32_t l = 0; l < L; l++) {
    const uint32_t ni = K.lookup_shape[l].first, nt = K.lookup_shape[l].second;
    // l_0 * (1 - z)
    pr.op(OP_PUSH_CONST, K.c_one); pr.push();
    pr.op(OP_SUB_COL, COL(K.se_zl(l), r0));
    pr.op(OP_MUL_HOT, 0);
    pr.op(OP_ACC); pr.pop();
    // l_last * (z^2 - z)
    pr.op(OP_PUSH_COL, COL(K.se_zl(l), r0)); pr.push();
    pr.op(OP_SQR);
    pr.op(OP_SUB_COL, COL(K.se_zl(l), r0));
    pr.op(OP_MUL_HOT, 1);
    pr.op(OP_ACC); pr.pop();
    // l_active * (z(wX)(a'+beta)(s'+gamma) - z(X)(ci+beta)(ct+gamma))
    pr.op(OP_PUSH_COL, COL(K.se_zl(l), r1)); pr.push();
    pr.op(OP_PUSH_COL, COL(K.se_la(l), r0)); pr.push();
    pr.op(OP_ADD_CONST, K.c_beta);
    pr.op(OP_MUL); pr.pop();
    pr.op(OP_PUSH_COL, COL(K.se_ls(l), r0)); pr.push();
    pr.op(OP_ADD_CONST, K.c_gamma);
    pr.op(OP_MUL); pr.pop();
    pr.op(OP_PUSH_COL, COL(K.se_zl(l), r0)); pr.push();
    ZK_TRY(emit_compressed(ctx, K, pr, e, ni));
    pr.op(OP_ADD_CONST, K.c_beta);
    pr.op(OP_MUL); pr.pop();
    ZK_TRY(emit_compressed(ctx, K, pr, e + ni, nt));
    pr.op(OP_ADD_CONST, K.c_gamma);
    pr.op(OP_MUL); pr.pop();
    pr.op(OP_SUB); pr.pop();
    pr.op(OP_MUL_HOT, 2);
    pr.op(OP_ACC); pr.pop();
    // l_0 * (a' - s')
    pr.op(OP_PUSH_COL, COL(K.se_la(l), r0)); pr.push();
    pr.op(OP_SUB_COL, COL(K.se_ls(l), r0));
    pr.op(OP_MUL_HOT, 0);
    pr.op(OP_ACC); pr.pop();
    // l_active * (a' - s')(a' - a'(w^-1 X))
    pr.op(OP_PUSH_COL, COL(K.se_la(l), r0)); pr.push();
    pr.op(OP_SUB_COL, COL(K.se_ls(l), r0));
    pr.op(OP_PUSH_COL, COL(K.se_la(l), r0)); pr.push();
    pr.op(OP_SUB_COL, COL(K.se_la(l), rm1));
    pr.op(OP_MUL); pr.pop();
    pr.op(OP_MUL_HOT, 2);
    pr.op(OP_ACC); pr.pop();
    e += ni + nt;
  }
  // pieces of the h(X) program: 6 by default. One piece is 1.5 wavefronts per SIMD at k = 15 (3 cosets x 2^15 rows) and
  // the interpreter alone took 2.30 ms of a lone proof's critical path; 8 pieces 1.70 ms. Latency of one proof, median
  // of 15, two runs each on one box: 1 piece 18.34 / 18.39 ms, 4: 17.71 / 17.86, 6: 17.61 / 17.78, 8: 17.63 / 17.46;
  // 10 proofs in flight: 78.0 / 76.7, 77.8 / 78.3, 78.2 / 78.5, 78.0 / 77.6 proofs/s (no difference).
  // AMDZK_H_PARTS=1..8 for experiments.
  const char* env = getenv("AMDZK_H_PARTS");
  uint32_t parts = env ? (uint32_t)atoi(env) : 6u;
  parts = parts < 1 ? 1 : parts > H_PARTS_MAX ? H_PARTS_MAX : parts;
  K.h_terms = finalize_limb_program(pr, parts);
  K.h_term_beta_pow = pr.term_beta;
  return AMDZK_OK;
}

// Every program of the key must fit the LDS of the interpreter that runs it (program.hip check_program_fits): the h(X)
// program, the Lagrange-domain programs, the constant tables' one-off program (build_constant_tables), and the witness
// check's gates, which a handle compiles at its first check — compiled here once for their depth alone.
static int check_program_depths(amdzk_ctx* ctx, const KeyMaterial& K) {
  ZK_TRY(check_program_fits(ctx, K.prog_h, true, "h(X)"));
  ZK_TRY(check_program_fits(ctx, K.prog_compress, false, "lookup compression"));
  ZK_TRY(check_program_fits(ctx, K.prog_pfrac, false, "permutation fraction"));
  ZK_TRY(check_program_fits(ctx, K.prog_lfrac, false, "lookup fraction"));
  ProgramText tables;
  uint32_t e = K.num_gates;
  for (uint32_t l = 0; l < K.lk_const; l++) {
    RotTable rots = K.rots;  // (emit_compress_program has queried these rotations: the copy does not grow)
    ZK_TRY(emit_expr(ctx, K, &rots, tables, K.exprs[e + K.lookup_shape[l].first]));
    tables.pop();
    e += K.lookup_shape[l].first + 1;
  }
  ZK_TRY(check_program_fits(ctx, tables, false, "constant lookup table"));
  ProgramText gates;
  ZK_TRY(emit_check_gates(ctx, K, gates));
  ZK_TRY(check_program_fits(ctx, gates, false, "witness-check gate"));
  return AMDZK_OK;
}

// AMDZK_DUMP_PROG, a debugging aid: what the compiled h(X) program is made of
static void dump_h_program(const KeyMaterial& K) {
  static const char* names[] = {"END", "PUSH_COL", "PUSH_CONST", "ADD", "SUB", "MUL", "NEG", "MUL_CONST", "ADD_CONST", "MUL_COL",
                                "ADD_COL", "SUB_COL", "ACC", "STORE", "SQR", "PUSH_HOT", "MUL_HOT", "REDUCE", "SUB_BIG", "NEG_BIG",
                                "WACC", "WFLUSH"};
  std::map<uint32_t, size_t> hist;
  std::map<std::pair<uint32_t, uint32_t>, size_t> pairs;
  const auto& w = K.prog_h.words;
  for (size_t i = 0; i < w.size(); i++) {
    hist[w[i] >> 24]++;
    if (i + 1 < w.size()) pairs[{w[i] >> 24, w[i + 1] >> 24}]++;
  }
  fprintf(stderr, "[amdzk] prog_h: %zu instructions, stack depth %u\n", w.size(), K.prog_h.depth);
  for (auto& kv : hist) fprintf(stderr, "[amdzk]   %-10s %zu\n", kv.first < 22 ? names[kv.first] : "?", kv.second);
  auto is_mul = [](uint32_t o) { return o == OP_MUL || o == OP_MUL_CONST || o == OP_MUL_COL || o == OP_MUL_HOT || o == OP_SQR || o == OP_WACC; };
  size_t mm = 0;
  for (auto& kv : pairs)
    if (is_mul(kv.first.first) && is_mul(kv.first.second)) {
      mm += kv.second;
      fprintf(stderr, "[amdzk]   product -> product: %s -> %s x %zu\n", names[kv.first.first], names[kv.first.second], kv.second);
    }
  fprintf(stderr, "[amdzk]   products directly followed by a product: %zu\n", mm);
}

// Constant tables (KeyMaterial::lk_const): ct[l] evaluated here, once, in the handle's workspace, and its canonical, padded,
// sorted form kept
static int build_constant_tables(amdzk_ctx* ctx, KeyMaterial& K, amdzk_pk* pk) {
  if (!K.lk_const) return AMDZK_OK;
  const size_t n = K.n;
  const uint32_t cnt = K.lk_const, usable = (uint32_t)n - (K.bf + 1);
  ZK_TRY(dalloc(ctx, &K, &K.lk_ts_const, (size_t)cnt * n));
  ProgramText tx;
  uint32_t e = K.num_gates;
  for (uint32_t l = 0; l < cnt; l++) {
    tx.piece();
    ZK_TRY(emit_expr(ctx, K, &K.rots, tx, K.exprs[e + K.lookup_shape[l].first]));
    tx.op(OP_STORE, 2 * l + 1);
    tx.pop();
    e += K.lookup_shape[l].first + 1;
  }
  Program pr{&tx};
  ZK_TRY(upload_program(ctx, pk, pr, false));
  ZK_TRY(run_program(ctx, pk, pr, false, pk->d_outs_compress, nullptr, "expr_const_tables"));
  ZK_TRY(d2d(ctx, K.lk_ts_const, pk->ct, (size_t)cnt * n * 32));
  ZK_TRY(amdzk_fr_to_repr_dev(ctx, K.lk_ts_const, (size_t)cnt * n));
  ZK_HIP(ctx, hipMemset2DAsync(K.lk_ts_const + usable, (size_t)n * 32, 0xFF, (size_t)(n - usable) * 32, cnt, ctx->stream));
  ZK_TRY(zk_sort_keys(ctx, K.lk_ts_const, cnt, n, n));
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  return AMDZK_OK;
}

// l_active = 1 - (l_last + l_blind) on the cosets: lactive_c holds l_blind's coset (build_domain_columns); a tiny one-off
// program over the extended table, whose constants bind_workspace has uploaded
static int finish_l_active(amdzk_ctx* ctx, KeyMaterial& K, amdzk_pk* pk) {
  const uint32_t r0 = K.rots.index(0);
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  ProgramText tx;
  tx.op(OP_PUSH_CONST, K.c_one); tx.push();
  tx.op(OP_SUB_COL, COL(K.se_llast(), r0));
  tx.op(OP_SUB_COL, COL(K.se_lactive(), r0));
  tx.op(OP_STORE, 0); tx.pop();
  (void)finalize_limb_program(tx);
  Program pr{&tx};
  ZK_TRY(upload_program(ctx, pk, pr, true));
  Fr** d_out = nullptr;
  ZK_TRY(dalloc(ctx, pk, &d_out, 1));
  Fr* tgt = K.lactive_c;
  ZK_TRY(h2d(ctx, d_out, &tgt, sizeof(Fr*)));
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  ZK_TRY(run_program(ctx, pk, pr, true, d_out, nullptr, "expr_l_active"));
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  return AMDZK_OK;
}

// keygen with ConstraintSystem::{advice_column_in, challenge_usable_after}'s phase table (NULL: every column in phase 0,
// no challenges). One of perm_mapping (Assembly::mapping: the sigma values are computed here) and sigma_values (the
// Lagrange values themselves, amdzk_keygen_sigma / amdzk_pk_read) feeds the permutation columns; everything behind their
// upload is shared. fixed_values / sigma_values are only copied to the device: any alignment (amdzk_pk_read passes
// pointers into the file). The key belongs to `owner` until it is handed to *out: every refusal and every failed call
// on the way frees it.
static int keygen_common(amdzk_ctx* ctx, const amdzk_srs* srs, const amdzk_circuit* c, const amdzk_phases* ph, const void* fixed_values,
                         const uint32_t* perm_mapping, const void* sigma_values, bool from_sigma, const uint64_t transcript_repr[4],
                         uint32_t flags, amdzk_pk** out) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  uint32_t nphases = 1;
  ZK_TRY(check_keygen_args(ctx, srs, c, ph, transcript_repr, flags, out, &nphases));
  PkOwner owner(new amdzk_pk(), PkFree{ctx});
  amdzk_pk* pk = owner.get();
  // The material under construction: the handle is its one owner from the start (so that a failed step frees both), and
  // K is the only way to write it. It ends with this function: from here on the material is frozen.
  KeyMaterial& K = *new KeyMaterial();
  pk->key.reset(&K);
  ZK_TRY(describe_circuit(ctx, K, srs, c, ph, nphases, transcript_repr, flags, false));
  ZK_TRY(alloc_key_material(ctx, K, pk));
  ZK_TRY(build_domain_columns(ctx, K, pk));
  ZK_TRY(load_fixed_columns(ctx, K, fixed_values));
  ZK_TRY(load_sigma_columns(ctx, K, perm_mapping, sigma_values, from_sigma));
  ZK_TRY(build_perm_lists(ctx, K));
  // rotations 0, 1, -1 and -(bf + 1) open the rotation table of every key, ahead of what its expressions query
  for (int32_t r : {0, 1, -1, -(int32_t)(K.bf + 1)}) K.rots.index(r);
  ZK_TRY(emit_compress_program(ctx, K));
  emit_pfrac_program(K);
  emit_lfrac_program(K);
  ZK_TRY(emit_h_program(ctx, K));
  if (K.rots.rots.size() > 255) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "keygen: more than 255 distinct rotations");
  ZK_TRY(check_program_depths(ctx, K));
  ZK_TRY(bind_workspace(ctx, pk));
  if (getenv("AMDZK_DUMP_PROG")) dump_h_program(K);
  ZK_TRY(build_constant_tables(ctx, K, pk));
  ZK_TRY(finish_l_active(ctx, K, pk));
  *out = owner.release();
  return AMDZK_OK;
}

// The one release of key material: whoever drops the last pointer to it runs this. The domain's free takes a ctx — the
// one of the call that lets go (amdzk_pk_free, KeyFree), which leaves it here for its own thread.
static thread_local amdzk_ctx* t_release_ctx = nullptr;
KeyMaterial::~KeyMaterial() {
  for (void* p : allocs) hipFree(p);
  if (chk_shared->d_cells) hipFree(chk_shared->d_cells);
  if (dom) amdzk_domain_free(t_release_ctx, dom);
}
void KeyFree::operator()(KeyMaterial* K) const {
  if (ctx) zk_host_wait(ctx, ctx->stream);
  t_release_ctx = ctx;
  delete K;
  t_release_ctx = nullptr;
}

extern "C" {

// The handle's workspace, and the key material if this was its last handle.
void amdzk_pk_free(amdzk_ctx* ctx, amdzk_pk* pk) {
  ZK_ENTER(ctx);
  if (!pk) return;
  if (ctx) zk_host_wait(ctx, ctx->stream);
  for (void* p : pk->allocs) hipFree(p);
  if (pk->pin) hipHostFree(pk->pin);
  t_release_ctx = ctx;
  delete pk;
  t_release_ctx = nullptr;
}

// Every device allocation of the handle (per-proof workspace) and of its key (columns, cosets) must live on ctx's device.
int amdzk_pk_check_affinity(amdzk_ctx* ctx, const amdzk_pk* pk) {
  ZK_ENTER(ctx);
  if (!ctx || !pk) return AMDZK_E_INVALID;
  for (void* p : pk->key->allocs) ZK_TRY(zk_ptr_on_device(ctx, p, "proving-key buffer"));
  for (void* p : pk->allocs) ZK_TRY(zk_ptr_on_device(ctx, p, "proving-key buffer"));
  return AMDZK_OK;
}

// keygen with the environment's defaults for the key's modes (AMDZK_FULL_COSETS, AMDZK_SERIAL); amdzk_keygen_ex takes
// them as explicit flags, so that two keys of one process can differ.
int amdzk_keygen(amdzk_ctx* ctx, const amdzk_srs* srs, const amdzk_circuit* c, const uint64_t* fixed_values, const uint32_t* perm_mapping,
                 const uint64_t transcript_repr[4], amdzk_pk** out) {
  uint32_t flags = 0;
  if (const char* e = getenv("AMDZK_FULL_COSETS")) flags |= atoi(e) != 0 || !*e ? AMDZK_KEYGEN_FULL_COSETS : 0u;
  if (const char* e = getenv("AMDZK_SERIAL")) flags |= atoi(e) != 0 ? AMDZK_KEYGEN_SERIAL : 0u;
  return amdzk_keygen_ex(ctx, srs, c, fixed_values, perm_mapping, transcript_repr, flags, out);
}

int amdzk_keygen_ex(amdzk_ctx* ctx, const amdzk_srs* srs, const amdzk_circuit* c, const uint64_t* fixed_values, const uint32_t* perm_mapping,
                    const uint64_t transcript_repr[4], uint32_t flags, amdzk_pk** out) {
  return amdzk_keygen_phased(ctx, srs, c, nullptr, fixed_values, perm_mapping, transcript_repr, flags, out);
}

int amdzk_keygen_phased(amdzk_ctx* ctx, const amdzk_srs* srs, const amdzk_circuit* c, const amdzk_phases* ph, const uint64_t* fixed_values,
                        const uint32_t* perm_mapping, const uint64_t transcript_repr[4], uint32_t flags, amdzk_pk** out) {
  return keygen_common(ctx, srs, c, ph, fixed_values, perm_mapping, nullptr, false, transcript_repr, flags, out);
}

// keygen from the sigma columns (permutation::ProvingKey::permutations, Lagrange form) instead of the mapping: what a
// process that has read a cached key holds. The values are taken as they are (upstream's read does not check them either).
int amdzk_keygen_sigma(amdzk_ctx* ctx, const amdzk_srs* srs, const amdzk_circuit* c, const amdzk_phases* ph, const uint64_t* fixed_values,
                       const uint64_t* sigma_values, const uint64_t transcript_repr[4], uint32_t flags, amdzk_pk** out) {
  return keygen_common(ctx, srs, c, ph, fixed_values, nullptr, sigma_values, true, transcript_repr, flags, out);
}

// VK material a verifier needs: commitments of the fixed columns and of the permutation polynomials.
int amdzk_pk_commitments(const amdzk_pk* pk, uint64_t* fixed_out /* F x 8 */, uint64_t* perm_out /* S x 8 */) {
  if (!pk) return AMDZK_E_INVALID;
  const KeyMaterial& K = *pk->key;
  if (fixed_out && K.F) memcpy(fixed_out, K.fixed_commitments.data(), (size_t)K.F * 64);
  if (perm_out && K.S) memcpy(perm_out, K.perm_commitments.data(), (size_t)K.S * 64);
  return AMDZK_OK;
}

// One more circuit instance's workspace for `src`'s circuit: a key handle that holds src's key material (fixed and
// permutation columns in all three forms, the domain, the compiled programs' text, constant lookup tables — const behind
// every handle) and owns its own per-proof workspace, pointer tables and uploaded programs (their instructions carry
// absolute column addresses). What amdzk_create_proof_multi takes for its second, third, ... instance — and, since a
// clone is a complete key for create_proof, the cheap way to keep several proofs of one circuit in flight: a
// clone costs the workspace (the arenas), not the key (354 + 354 MiB of permutation cosets at the metric's shape).
// Free it with amdzk_pk_free; handles of one key are freed in any order, and the last one frees the key material.
int amdzk_pk_clone_workspace(amdzk_ctx* ctx, const amdzk_pk* src, amdzk_pk** out) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  if (!src || !out) ZK_FAIL(ctx, AMDZK_E_INVALID, "pk_clone_workspace: null argument");
  PkOwner owner(new amdzk_pk(), PkFree{ctx});
  amdzk_pk* pk = owner.get();
  pk->key = src->key;
  const KeyMaterial& K = *pk->key;
  ZK_TRY(alloc_proof_workspace(ctx, pk));
  ZK_TRY(bind_workspace(ctx, pk));
  // the compressed constant tables (KeyMaterial::lk_const) are written once, at keygen, into the workspace's ct columns —
  // the per-proof compression program skips them — so a new workspace starts with a copy
  if (K.lk_const) ZK_TRY(d2d(ctx, pk->ct, src->ct, (size_t)K.lk_const * K.n * 32));
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));
  *out = owner.release();
  return AMDZK_OK;
}

// What the last create_proof on this key left in its workspace, for tests that check one stage at a time against the
// oracle: what = 0 the NP committed polynomials in coefficient form ([NP][n], arena order as above); 1 the
// challenges theta, beta, gamma, y; 2 the pieces of h(X) ([cs_degree - 1][n]); 3 the phase challenges. `out` holds cap Fr elements;
// *count = elements available.
int amdzk_pk_inspect(amdzk_ctx* ctx, const amdzk_pk* pk, int what, uint64_t* out, size_t cap, size_t* count) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  if (!pk || !count) ZK_FAIL(ctx, AMDZK_E_INVALID, "pk_inspect: null argument");
  const KeyMaterial& K = *pk->key;
  const Fr* src = nullptr;
  size_t cnt = 0;
  Fr ch[4];
  if (what == 0) {
    src = pk->PQ;
    cnt = K.NP * K.n;
  } else if (what == 2) {
    src = pk->hpieces;
    cnt = (size_t)K.qdeg * K.n;
  } else if (what == 1) {
    ch[0] = pk->consts[K.c_theta];
    ch[1] = pk->consts[K.c_beta];
    ch[2] = pk->consts[K.c_gamma];
    ch[3] = pk->consts[K.c_y];
    cnt = 4;
  } else if (what == 3) {
    cnt = K.num_challenges;
  } else {
    ZK_FAIL(ctx, AMDZK_E_INVALID, "pk_inspect: unknown selector %d", what);
  }
  *count = cnt;
  if (!out) return AMDZK_OK;
  if (cap < cnt) ZK_FAIL(ctx, AMDZK_E_INVALID, "pk_inspect: buffer holds %zu elements, %zu needed", cap, cnt);
  if (what == 1) memcpy(out, ch, sizeof(ch));
  else if (what == 3) memcpy(out, pk->consts.data() + K.c_chal0, cnt * 32);
  else ZK_TRY(d2h(ctx, out, src, cnt * 32));
  return AMDZK_OK;
}

// The key's own columns, for a fork whose ProvingKey::write stores a key that was made on the device: what = 0 the fixed
// columns (Lagrange), 1 the sigma columns (Lagrange), 2 / 3 the same as coefficients: key material, the same through
// every handle of the key.
int amdzk_pk_export(amdzk_ctx* ctx, const amdzk_pk* pk, int what, uint64_t* out, size_t cap, size_t* count) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  if (!pk || !count) ZK_FAIL(ctx, AMDZK_E_INVALID, "pk_export: null argument");
  const KeyMaterial& K = *pk->key;
  if (what < 0 || what > 3) ZK_FAIL(ctx, AMDZK_E_INVALID, "pk_export: unknown selector %d", what);
  const Fr* src[4] = {K.fixed_lag, K.sigma_lag, K.fixed_poly, K.sigma_poly};
  const size_t cnt = (size_t)((what & 1) ? K.S : K.F) * K.n;
  *count = cnt;
  if (!out) return AMDZK_OK;
  if (cap < cnt) ZK_FAIL(ctx, AMDZK_E_INVALID, "pk_export: buffer holds %zu elements, %zu needed", cap, cnt);
  return d2h(ctx, out, src[what], cnt * 32);
}

// ---- the key file (csrc/pkblob.hpp has the layout, the header's writer and the host-only parser)
// keygen takes a circuit on trust where pkblob::validate() does not (a query that no expression uses may name any column,
// for one): such a key proves, but its file would be refused by amdzk_pk_read, so it is not written at all.
size_t amdzk_pk_serialized_size(const amdzk_pk* pk) {
  return pk && pk->key->src_desc && pkblob::validate(*pk->key->src_desc, nullptr) == AMDZK_OK ? pk->key->src_desc->serialized_size() : 0;
}

int amdzk_pk_write(amdzk_ctx* ctx, const amdzk_pk* pk, uint8_t* out, size_t cap, size_t* written) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  if (!pk || !pk->key->src_desc || (!out && !written)) ZK_FAIL(ctx, AMDZK_E_INVALID, "pk_write: null argument");
  const KeyMaterial& K = *pk->key;
  const pkblob::Desc& d = *K.src_desc;
  std::string why;
  if (pkblob::validate(d, &why) != AMDZK_OK)
    ZK_FAIL(ctx, AMDZK_E_INVALID, "pk_write: amdzk_pk_read would refuse this key's circuit (%s)", why.c_str());
  const size_t need = d.serialized_size();
  if (written) *written = need;
  if (!out) return AMDZK_OK;
  if (cap < need) ZK_FAIL(ctx, AMDZK_E_INVALID, "pk_write: buffer holds %zu bytes, %zu needed", cap, need);
  d.write_header(out);
  uint8_t* p = out + d.header_bytes();
  memcpy(p, K.transcript_repr.l, 32);
  p += 32;
  if (K.F) memcpy(p, K.fixed_commitments.data(), (size_t)K.F * 64);
  p += (size_t)K.F * 64;
  if (K.S) memcpy(p, K.perm_commitments.data(), (size_t)K.S * 64);
  p += (size_t)K.S * 64;
  ZK_TRY(d2h(ctx, p, K.fixed_lag, (size_t)K.F * K.n * 32));
  p += (size_t)K.F * K.n * 32;
  ZK_TRY(d2h(ctx, p, K.sigma_lag, (size_t)K.S * K.n * 32));
  p += (size_t)K.S * K.n * 32;
  pkblob::digest(out, (size_t)(p - out), p);
  return AMDZK_OK;
}

// Pure host code: every check amdzk_pk_read makes before it touches the device.
int amdzk_pk_blob_info(const uint8_t* data, size_t len, uint32_t* k, uint32_t* num_fixed, uint32_t* num_advice, uint32_t* num_perm_columns,
                       uint32_t* num_challenges) {
  pkblob::Desc d;
  if (int rc = pkblob::parse(data, len, &d, nullptr, nullptr)) return rc;
  if (k) *k = d.k;
  if (num_fixed) *num_fixed = d.num_fixed;
  if (num_advice) *num_advice = d.num_advice;
  if (num_perm_columns) *num_perm_columns = d.num_perm_columns();
  if (num_challenges) *num_challenges = d.num_challenges;
  return AMDZK_OK;
}

// amdzk_pk_blob_info's verdict with its reason: the message amdzk_pk_read would leave in the ctx ("pk_read: digest mismatch
// ..."), for a host without a device. msg (may be NULL) receives at most msg_cap bytes, NUL-terminated; "" for a good file.
int amdzk_pk_blob_check(const uint8_t* data, size_t len, char* msg, size_t msg_cap) {
  pkblob::Desc d;
  std::string err;
  const int rc = pkblob::parse(data, len, &d, nullptr, &err);
  if (msg && msg_cap) snprintf(msg, msg_cap, "%s", err.c_str());
  return rc;
}

// The file's header and columns through the tail keygen shares (keygen_common), then the commitments it computed against
// the stored ones: they differ exactly when the parameters are not the ones the key was made under.
int amdzk_pk_read(amdzk_ctx* ctx, const amdzk_srs* srs, const uint8_t* data, size_t len, uint32_t flags, amdzk_pk** out) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  if (!srs || !data || !out) ZK_FAIL(ctx, AMDZK_E_INVALID, "pk_read: null argument");
  pkblob::Desc d;
  pkblob::Layout lay;
  std::string err;
  if (int rc = pkblob::parse(data, len, &d, &lay, &err)) {
    ctx->err = err;
    return rc;
  }
  if (d.k != zk_srs_k(srs)) ZK_FAIL(ctx, AMDZK_E_INVALID, "pk_read: the key is for k = %u, the parameters are for k = %u", d.k, zk_srs_k(srs));
  amdzk_circuit c;
  amdzk_phases ph;
  d.view(&c, &ph);
  uint64_t repr[4];
  memcpy(repr, data + lay.transcript_repr, 32);
  amdzk_pk* pk = nullptr;
  const int rc = keygen_common(ctx, srs, &c, d.has_phases ? &ph : nullptr, data + lay.fixed_values, nullptr, data + lay.sigma_values, true, repr,
                               flags, &pk);
  if (rc != AMDZK_OK) {
    if (rc == AMDZK_E_INVALID) ctx->err = "pk_read: " + ctx->err;
    return rc;
  }
  const KeyMaterial& K = *pk->key;
  const bool same = (!K.F || memcmp(K.fixed_commitments.data(), data + lay.fixed_commitments, (size_t)K.F * 64) == 0) &&
                    (!K.S || memcmp(K.perm_commitments.data(), data + lay.perm_commitments, (size_t)K.S * 64) == 0);
  if (!same) {
    amdzk_pk_free(ctx, pk);
    ZK_FAIL(ctx, AMDZK_E_INVALID,
            "pk_read: the commitments in the file are not those of its columns under these parameters: the key was made under other "
            "parameters (another SRS)");
  }
  *out = pk;
  return AMDZK_OK;
}

}  // extern "C"
