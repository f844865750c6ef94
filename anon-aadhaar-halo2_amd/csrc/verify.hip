// amdzk_verify_proofs (include/amdzk.h): plonk::verify_proof [UP] for one proof or a batch, up to the two G1
// sums of the final pairing check. The device decodes every element of every proof in one launch (decompression with its
// curve check, range checks, Montgomery conversion) and runs the one two-column MSM; the transcript, the vanishing
// identity and the per-base scalars are the host half's (verifier.hpp). Two host waits per call. Nothing here touches the
// key's per-proof workspace. The key is read through a view (vk.hpp) that a proving key or a verifying key fills:
// amdzk_verify_proofs_vk and amdzk_verify_proofs_decide_vk are the same code over the same operands.
// amdzk_verify_proofs_mixed and amdzk_verify_proofs_decide_mixed take a key PER ITEM. All of them are ONE verify_core over
// a Call: items in GROUPS that share a key, an instance count and a transcript kind, hence a plan, an element table and a
// block of commitments. An adapter per family of entry points checks its own arguments and fills the Call; a single-key
// call is a Call of one group. One decode launch (proof_decode_kernel) and one MSM per call, however many keys it names.
#include <stddef.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include "common.hpp"
#include "pk.hpp"
#include "verifier.hpp"
#include "vk.hpp"

using namespace bn254;

namespace {

constexpr uint32_t DECODE_THREADS = 64;
constexpr uint32_t STATUS_CLEAN = 0xffffffffu;

// 32 bytes at a 32-byte-aligned address as a 256-bit integer, little- or big-endian
template <class F>
__device__ __forceinline__ F load_u256(const uint8_t* p, bool big_endian) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  F r;
#pragma unroll
  for (int j = 0; j < 8; j++) r.l[j] = big_endian ? __builtin_bswap32(w[7 - j]) : w[j];
  return r;
}
__device__ __forceinline__ void store_fq(Fq* p, const Fq& v) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

// One element in the form a caller's read transcript handed it back: Montgomery words at src, 64 bytes for a point, 32 for a
// scalar. Checked, not converted; a bad element is stored as zero. y: is_point << 31 | index among the proof's points /
// scalars, which start at points / scalars. Returns whether the element is good, *cls its class if not.
__device__ __forceinline__ bool decode_raw_element(const uint8_t* src, uint32_t y, uint32_t inf_below, G1Affine* points, Fr* scalars, uint32_t* cls) {
  const uint32_t index = y & 0x7fffffffu;
  bool ok;
  if (y >> 31) {  // both coordinates canonical, on the curve (which (0, 0) is not) or, where allowed, the identity
    *cls = AMDZK_PROOF_BAD_POINT;
    G1Affine p;
    p.x = load_u256<Fq>(src, false);
    p.y = load_u256<Fq>(src + 32, false);
    ok = is_canonical(p.x) && is_canonical(p.y);
    if (ok) ok = (index < inf_below && p.x.is_zero() && p.y.is_zero()) || sqr(p.y) == g1_curve_rhs(p.x);
    if (!ok) p.x = Fq::zero(), p.y = Fq::zero();
    G1Affine* o = points + index;
    store_fq(&o->x, p.x);
    store_fq(&o->y, p.y);
  } else {
    *cls = AMDZK_PROOF_BAD_SCALAR;
    Fr s = load_u256<Fr>(src, false);
    ok = is_canonical(s);
    if (!ok) s = Fr::zero();
    uint4* o = reinterpret_cast<uint4*>(scalars + index);
    o[0] = make_uint4(s.l[0], s.l[1], s.l[2], s.l[3]);
    o[1] = make_uint4(s.l[4], s.l[5], s.l[6], s.l[7]);
  }
  return ok;
}
// ... and in the bytes of a built-in transcript: compressed (Blake2b) or x | y big-endian (EVM).
__device__ __forceinline__ bool decode_byte_element(const uint8_t* src, uint32_t y, int evm, G1Affine* points, Fr* scalars, uint32_t* cls) {
  const uint32_t index = y & 0x7fffffffu;
  bool ok;
  if (y >> 31) {
    *cls = AMDZK_PROOF_BAD_POINT;
    G1Affine p;
    p.x = Fq::zero();
    p.y = Fq::zero();
    if (evm) {  // x | y, big-endian: both canonical, on the curve (which the identity's encoding (0, 0) is not)
      const Fq x = load_u256<Fq>(src, true), y = load_u256<Fq>(src + 32, true);
      ok = is_canonical(x) && is_canonical(y);
      if (ok) {
        const Fq xm = to_mont(x), ym = to_mont(y);
        ok = sqr(ym) == g1_curve_rhs(xm);
        if (ok) p.x = xm, p.y = ym;
      }
    } else {  // x little-endian, bit 7 of byte 31 = parity of y; all zero is the identity, which the transcripts refuse
      Fq x = load_u256<Fq>(src, false);
      const uint32_t ysign = x.l[7] >> 31;
      x.l[7] &= 0x7fffffffu;
      ok = is_canonical(x) && !(x.is_zero() && ysign == 0);
      if (ok) {
        const Fq xm = to_mont(x);
        Fq y;
        ok = g1_y_from_x(xm, ysign, &y);
        if (ok) p.x = xm, p.y = y;
      }
    }
    G1Affine* o = points + index;
    store_fq(&o->x, p.x);
    store_fq(&o->y, p.y);
  } else {
    *cls = AMDZK_PROOF_BAD_SCALAR;
    const Fr s = load_u256<Fr>(src, evm != 0);
    ok = is_canonical(s);
    const Fr m = ok ? to_mont(s) : Fr::zero();
    uint4* o = reinterpret_cast<uint4*>(scalars + index);
    o[0] = make_uint4(m.l[0], m.l[1], m.l[2], m.l[3]);
    o[1] = make_uint4(m.l[4], m.l[5], m.l[6], m.l[7]);
  }
  return ok;
}

// Every element of every proof of a call (verifier.hpp, MixedLayout), one thread each, the element's form chosen per item.
// A point costs one Fq square-root chain (254 dependent squarings, Blake2b form) or a curve check (EVM and raw forms), a
// scalar one product: the launch is latency-bound, so the blocks are single waves that the dispatcher spreads over the CUs,
// and a wave that holds only scalars retires at once. A block decodes up to 64 elements of ONE item, named by its block
// record, so the item's and its group's records are read wave-uniformly and nothing divides.
struct DecodeArgs {
  const uint8_t* staging;
  const verifier::MixedItemRec* items;
  const verifier::MixedGroupRec* groups;
  const verifier::MixedBlockRec* blocks;
  const uint2 *elems, *elems_raw;  // every group's tables, one behind the other
  G1Affine* points;
  Fr* scalars;
  // per item: min over its bad elements of offset << 2 | class (the raw form: element index in read order << 2 | class),
  // STATUS_CLEAN when there is none
  uint32_t* status;
};
static_assert(DECODE_THREADS == verifier::MIXED_BLOCK, "one block record per launched block");
__global__ __launch_bounds__(DECODE_THREADS) void proof_decode_kernel(DecodeArgs a) {
  const verifier::MixedBlockRec blk = a.blocks[blockIdx.x];
  const verifier::MixedItemRec it = a.items[blk.item];
  const verifier::MixedGroupRec g = a.groups[it.group];
  const uint32_t e = blk.first + threadIdx.x;
  if (e >= g.E) return;
  const uint2 el = (it.raw ? a.elems_raw : a.elems)[g.elems + e];
  const uint8_t* src = a.staging + it.staging + el.x;
  uint32_t cls;
  const bool ok = it.raw ? decode_raw_element(src, el.y, 0, a.points + it.points, a.scalars + it.scalars, &cls)
                         : decode_byte_element(src, el.y, (int)g.evm, a.points + it.points, a.scalars + it.scalars, &cls);
  if (!ok) atomicMin(a.status + blk.item, ((it.raw ? e : el.x) << 2) | cls);
}

// zk_points_check_dev: n raw-form points checked in place; those below inf_below may be the identity. *status: the first
// bad point's index << 2 | class.
__global__ __launch_bounds__(DECODE_THREADS) void points_check_kernel(G1Affine* pts, uint32_t n, uint32_t inf_below, uint32_t* status) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  uint32_t cls;
  if (!decode_raw_element(reinterpret_cast<const uint8_t*>(pts + t), 0x80000000u | t, inf_below, pts, nullptr, &cls)) atomicMin(status, (t << 2) | cls);
}

// The view of a proving key: G stays where the key's SRS keeps it. A key without a description or an SRS gives a view
// without a description, which verify_core refuses.
zk_key_view view_of(const amdzk_pk* pk) {
  const KeyMaterial& K = *pk->key;
  zk_key_view v;
  if (K.src_desc && K.srs) v.desc = K.src_desc.get();
  v.transcript_repr = &K.transcript_repr, v.omega = &K.omega;
  v.fixed_commitments = K.fixed_commitments.data(), v.perm_commitments = K.perm_commitments.data();
  v.d_g = zk_srs_base_dev(K.srs, AMDZK_BASIS_G);
  v.sized_by = pk;
  return v;
}
// ... and of a verifying key, which holds G itself
zk_key_view view_of(const amdzk_vk* vk) {
  zk_key_view v;
  v.desc = vk->desc.get();
  v.transcript_repr = &vk->transcript_repr, v.omega = &vk->omega;
  v.fixed_commitments = vk->fixed_commitments.data(), v.perm_commitments = vk->perm_commitments.data();
  v.h_g = &vk->g;
  return v;
}

// The pairing behind a verify call and the verdicts: pairs holds (L_b, R_b) per proof, or (combined) the batch's one pair.
// Per proof (flags = 0) one launch of n_live checks with m = 2, P = (L_b, -R_b) over (s_g2, g2); combined, one check.
int decide_pairs(amdzk_ctx* ctx, const char* who, const amdzk_g2* s_g2, const amdzk_g2* g2, bool combined, const std::vector<G1Affine>& pairs, size_t n_proofs,
                 const amdzk_proof_status* statuses, uint8_t* verdicts, size_t* n_valid) {
  // the checks worth a pairing: both points finite (a pair of identities must not read as valid; one identity cannot pass)
  std::vector<G1Affine> g1;
  std::vector<size_t> at;
  for (size_t c = 0; c < pairs.size() / 2; c++) {
    if (pairs[2 * c].is_inf() || pairs[2 * c + 1].is_inf()) continue;
    g1.push_back(pairs[2 * c]);
    g1.push_back(a_neg(pairs[2 * c + 1]));
    at.push_back(c);
  }
  std::vector<uint8_t> one(at.size(), 0), holds(pairs.size() / 2, 0);
  if (!at.empty()) {
    const amdzk_g2* qs[2] = {s_g2, g2};
    ZK_TRY(zk_pairing_products(ctx, who, qs, 2, g1.data(), at.size(), one.data(), nullptr));
  }
  for (size_t c = 0; c < at.size(); c++) holds[at[c]] = one[c];
  size_t valid = 0;
  for (size_t b = 0; b < n_proofs; b++) {
    verdicts[b] = statuses[b].status == AMDZK_PROOF_WELL_FORMED && holds[combined ? 0 : b] ? 1 : 0;
    valid += verdicts[b];
  }
  if (n_valid) *n_valid = valid;
  return AMDZK_OK;
}

// ---- a verify call as verify_core sees it, whichever entry point it came through. Items that share a key handle, an
// instance count and a transcript kind form a GROUP (verifier.hpp, group_items / mixed_layout): one plan, one pair of element
// tables, one block of commitments.
struct Item {
  const uint64_t* const* const* instances;  // the item's N circuit instances x num_instance columns; read only where the circuit has any
  const size_t* const* instance_lens;
  const uint8_t* proof;  // not read for an item with a transcript
  size_t proof_len;
  const amdzk_transcript_read* transcript;  // the caller's read transcript, or nullptr
};
struct Group {
  // the adapter's
  zk_key_view key;
  const void* handle;  // the key the caller named: one G per distinct handle
  uint32_t n_circuits;
  int kind;      // the transcript kind that counts, masked by the adapter where only the opening scheme's bit does
  size_t first;  // the group's first item, which its refusals name
  // verify_core's
  verifier::Plan plan;
  std::vector<uint32_t> raw_off;  // filled when the batch has a read transcript
  size_t raw_size = 0, nvk = 0;
  size_t key_index = 0;  // among the distinct key handles, first seen first
};
struct Call {
  bool labelled = false;  // refusals about one item begin "item %zu: " (the mixed calls)
  std::vector<Item> items;
  std::vector<uint32_t> group_of;  // per item
  std::vector<Group> groups;       // first seen first
  const uint64_t* combine_scalars = nullptr;
  uint64_t combine_seed = 0;
};
// An adapter checks the arguments of its entry points, with their wording, and fills the Call.
using Adapter = std::function<int(Call*)>;

// Everything up to the G1 sums. `who` prefixes the refusals.
// pairs == nullptr: the batch's ONE pair, sum_b rho_b (L_b, R_b), in pair_out — amdzk_verify_proofs as documented.
// pairs != nullptr: every proof by itself with weight 1 — (L_b, R_b) in (*pairs)[2b], [2b + 1], identities for a malformed
// proof; the call's combine_* are not read and pair_out is not written. The MSMs run over AMDZK_DECIDE_RUN proofs at a time.
int verify_core(amdzk_ctx* ctx, const char* who, const Adapter& fill, amdzk_proof_status* statuses, uint64_t* pair_out, std::vector<G1Affine>* pairs) {
  const bool per_proof = pairs != nullptr;
  if (!statuses || (!per_proof && !pair_out)) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: null argument", who);
  Call call;
  ZK_TRY(fill(&call));
  const std::vector<Item>& items = call.items;
  const std::vector<uint32_t>& group_of = call.group_of;
  std::vector<Group>& groups = call.groups;
  const size_t n_items = items.size(), G = groups.size();
  auto label = [&](size_t b) { return call.labelled ? "item " + std::to_string(b) + ": " : std::string(); };
  // ---- every group planned and every item validated before anything is uploaded
  size_t n_tr = 0;
  for (const Item& it : items) n_tr += it.transcript != nullptr;
  std::vector<const void*> key_handles;  // distinct, first seen first
  std::vector<size_t> key_first;         // ... and the first item of each
  for (Group& gr : groups) {
    const size_t b = gr.first;
    if (!gr.key.desc) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: %sthe key has no circuit description", who, label(b).c_str());
    std::string why;
    if (verifier::make_plan(*gr.key.desc, gr.n_circuits, gr.kind, &gr.plan, &why) != AMDZK_OK) {
      const std::string own = "verify_proofs: ";  // verifier.hpp's prefix
      ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: %s%s", who, label(b).c_str(), why.compare(0, own.size(), own) == 0 ? why.c_str() + own.size() : why.c_str());
    }
    if ((gr.key.sized_by && gr.plan.proof_bytes != amdzk_proof_size_multi(gr.key.sized_by, gr.plan.N, gr.kind)) || gr.plan.proof_bytes >= ((size_t)1 << 30))
      ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "%s: %sproof layout of %zu bytes disagrees with amdzk_proof_size_multi or is too large", who, label(b).c_str(),
              gr.plan.proof_bytes);
    if (!gr.key.d_g && !gr.key.h_g) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: %sthe key's SRS has no monomial basis", who, label(b).c_str());
    if (n_tr) gr.raw_size = verifier::raw_offsets(gr.plan, &gr.raw_off);
    if (gr.raw_size >= ((size_t)1 << 30)) ZK_FAIL(ctx, AMDZK_E_UNSUPPORTED, "%s: %sproof layout of %zu bytes is too large", who, label(b).c_str(), gr.raw_size);
    gr.nvk = (size_t)gr.plan.F + gr.plan.S;
    size_t ki = 0;
    while (ki < key_handles.size() && key_handles[ki] != gr.handle) ki++;
    if (ki == key_handles.size()) key_handles.push_back(gr.handle), key_first.push_back(b);
    gr.key_index = ki;
  }
  for (size_t b = 0; b < n_items; b++) {
    const verifier::Plan& plan = groups[group_of[b]].plan;
    if (!plan.I) continue;
    if (!items[b].instances || !items[b].instance_lens) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: %snull argument (instances)", who, label(b).c_str());
    for (uint32_t c = 0; c < plan.N; c++) {
      if (items[b].instances[c] && items[b].instance_lens[c]) continue;
      if (call.labelled) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: item %zu: null argument (instances of circuit %u)", who, b, c);
      ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: null argument (instances of circuit %zu)", who, b * plan.N + c);  // one flat array per call
    }
  }
  std::vector<Fr> rho(n_items, Fr::one());
  if (per_proof) {
    // weight 1 for every proof: nothing of the call's combine_* is read
  } else if (call.combine_scalars) {
    for (size_t b = 0; b < n_items; b++) {
      if (!verifier::fr_canonical_words(call.combine_scalars + 4 * b)) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: combine_scalars[%zu] is not below the modulus", who, b);
      memcpy(rho[b].l, call.combine_scalars + 4 * b, 32);
    }
  } else if (n_items > 1) {
    zkhost::ChaCha20Rng rng(call.combine_seed);
    for (size_t b = 0; b < n_items; b++) rho[b] = rng.fr();
  }
  // ---- what the host can see: lengths and public inputs, each against the item's own layout
  size_t live = 0;
  for (size_t b = 0; b < n_items; b++) {
    const verifier::Plan& plan = groups[group_of[b]].plan;
    statuses[b].status = AMDZK_PROOF_WELL_FORMED, statuses[b].offset = 0;
    uint32_t col = 0;
    if (!items[b].transcript && items[b].proof_len != plan.proof_bytes) statuses[b].status = AMDZK_PROOF_BAD_LENGTH;
    else if (plan.I && !verifier::instances_ok(plan, items[b].instances, items[b].instance_lens, &col))
      statuses[b].status = AMDZK_PROOF_BAD_INSTANCE, statuses[b].offset = col;
    else live++;
  }
  G1Affine g1_inf;
  g1_inf.x = g1_inf.y = Fq::zero();
  if (per_proof) pairs->assign(2 * n_items, g1_inf);
  else memset(pair_out, 0, 16 * sizeof(uint64_t));
  if (live == 0) return AMDZK_OK;
  // ---- one reservation (verifier::MixedLayout) and its mirror in pinned memory
  std::vector<verifier::MixedGroupShape> shapes(G);
  for (size_t g = 0; g < G; g++) {
    const verifier::Plan& p = groups[g].plan;
    shapes[g] = {p.elems.size(), p.NP, p.NS, groups[g].nvk, p.proof_bytes, groups[g].raw_size};
  }
  std::vector<uint8_t> is_raw(n_tr ? n_items : 0);
  for (size_t b = 0; n_tr && b < n_items; b++) is_raw[b] = items[b].transcript != nullptr;
  const verifier::MixedLayout L = verifier::mixed_layout(shapes.data(), G, group_of.data(), n_tr ? is_raw.data() : nullptr, n_items, key_handles.size(), per_proof);
  if (L.n_blocks > 0x7fffffffu || L.n_elems > 0x7fffffffu) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: batch too large", who);
  const size_t nbases = L.nvk + 1 + L.n_points, up_bytes = L.up_bytes, down_bytes = L.down_bytes;
  char* ws = nullptr;
  ZK_TRY(zk_ws_reserve(ctx, ZK_WS_STARTUP, L.bytes, (void**)&ws));
  char* pin = nullptr;
  ZK_TRY(zk_pinned_reserve(ctx, up_bytes + down_bytes, (void**)&pin));
  char* h_down = pin + up_bytes;
  memset(pin, 0, up_bytes);
  // a transcript item is read here, through the caller's callbacks, in ascending b: its elements go to the staging area in
  // the raw form and its challenges are kept for the host half
  std::vector<verifier::Challenges> read_ch(n_tr ? n_items : 0);
  auto* h_items = (verifier::MixedItemRec*)(pin + L.items);
  auto* h_blocks = (verifier::MixedBlockRec*)(pin + L.blocks);
  size_t blk = 0;
  for (size_t b = 0; b < n_items; b++) {
    const Group& gr = groups[group_of[b]];
    const verifier::Plan& plan = gr.plan;
    const Item& it = items[b];
    ((uint32_t*)(pin + L.status))[b] = STATUS_CLEAN;
    h_items[b] = {(uint64_t)L.item_staging[b], (uint64_t)L.item_points[b], (uint64_t)L.item_scalars[b], group_of[b], it.transcript ? 1u : 0u};
    for (size_t e = 0; e < plan.elems.size(); e += verifier::MIXED_BLOCK) h_blocks[blk++] = {(uint32_t)b, (uint32_t)e};
    if (statuses[b].status != AMDZK_PROOF_WELL_FORMED) continue;
    char* stage = pin + L.staging + L.item_staging[b];
    if (!it.transcript) {
      memcpy(stage, it.proof, plan.proof_bytes);
      continue;
    }
    verifier::CallbackSource src(it.transcript, (uint8_t*)stage, gr.raw_off.data());
    if (!src.usable() || !verifier::run_transcript(plan, src, *gr.key.transcript_repr, plan.I ? it.instances : nullptr, plan.I ? it.instance_lens : nullptr, &read_ch[b])) {
      statuses[b].status = AMDZK_PROOF_BAD_TRANSCRIPT, statuses[b].offset = src.reads;
      memset(stage, 0, L.item_stride[b]);
      live--;
    }
  }
  if (live == 0) return AMDZK_OK;
  for (size_t g = 0; g < G; g++) {
    const Group& gr = groups[g];
    const verifier::Plan& plan = gr.plan;
    ((verifier::MixedGroupRec*)(pin + L.groups))[g] = {(uint32_t)L.group_elems[g], (uint32_t)plan.elems.size(), plan.evm ? 1u : 0u, 0u};
    for (size_t e = 0; e < plan.elems.size(); e++) {
      const uint32_t y = (plan.elems[e].is_point << 31) | plan.elems[e].index;
      ((uint2*)(pin + L.elems))[L.group_elems[g] + e] = make_uint2(plan.elems[e].offset, y);
      if (n_tr) ((uint2*)(pin + L.elems_raw))[L.group_elems[g] + e] = make_uint2(gr.raw_off[e], y);
    }
    G1Affine* h_vk = (G1Affine*)(pin + L.vk) + L.group_vk[g];
    if (plan.F) memcpy(h_vk, gr.key.fixed_commitments, (size_t)plan.F * sizeof(G1Affine));
    if (plan.S) memcpy(h_vk + plan.F, gr.key.perm_commitments, (size_t)plan.S * sizeof(G1Affine));
    if (gr.key.h_g) memcpy(pin + L.key_g + gr.key_index * sizeof(G1Affine), gr.key.h_g, sizeof(G1Affine));
  }
  ZK_HIP(ctx, hipMemcpyAsync(ws, pin, up_bytes, hipMemcpyHostToDevice, ctx->stream));
  for (size_t g = 0; g < G; g++)  // a proving key's G is on the device: one small copy per distinct key (repeated for a key's further groups)
    if (groups[g].key.d_g)
      ZK_HIP(ctx, hipMemcpyAsync(ws + L.key_g + groups[g].key_index * sizeof(G1Affine), groups[g].key.d_g, sizeof(G1Affine), hipMemcpyDeviceToDevice, ctx->stream));
  ZK_HIP(ctx, hipMemcpyAsync(ws + L.g, ws + L.key_g, sizeof(G1Affine), hipMemcpyDeviceToDevice, ctx->stream));
  DecodeArgs da;
  da.staging = (const uint8_t*)(ws + L.staging), da.items = (const verifier::MixedItemRec*)(ws + L.items);
  da.groups = (const verifier::MixedGroupRec*)(ws + L.groups), da.blocks = (const verifier::MixedBlockRec*)(ws + L.blocks);
  da.elems = (const uint2*)(ws + L.elems), da.elems_raw = (const uint2*)(ws + L.elems_raw);
  da.points = (G1Affine*)(ws + L.points), da.scalars = (Fr*)(ws + L.scalars), da.status = (uint32_t*)(ws + L.status);
  ZK_LAUNCH(ctx, "proof_decode", proof_decode_kernel, dim3((unsigned)L.n_blocks), dim3(DECODE_THREADS), 0, da);
  ZK_HIP(ctx, hipMemcpyAsync(h_down, ws + L.status, down_bytes, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(ctx, zk_host_wait(ctx, ctx->stream));  // wait 1 of 2
  // ---- the one rule, on what came down: every key's G is item 0's
  const G1Affine* h_key_g = (const G1Affine*)(h_down + (L.key_g - L.status));
  for (size_t ki = 1; ki < key_handles.size(); ki++)
    if (memcmp(&h_key_g[ki], &h_key_g[0], sizeof(G1Affine)) != 0)
      ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: item %zu: its key was made over another G than item 0's", who, key_first[ki]);
  // ---- the host half: per item one scalar per base for L and for R
  const uint32_t* h_status = (const uint32_t*)h_down;
  const G1Affine* h_points = (const G1Affine*)(h_down + (L.points - L.status));
  const Fr* h_scalars = (const Fr*)(h_down + (L.scalars - L.status));
  std::vector<Fr> msm(per_proof ? 0 : 2 * nbases, Fr::zero()), Lb, Rb;
  std::vector<Fr> own;         // per proof: the live items' (Lb | Rb), in batch order ...
  std::vector<size_t> own_at;  // ... where each starts ...
  std::vector<size_t> who_b;   // ... and their positions
  live = 0;
  for (size_t b = 0; b < n_items; b++) {
    if (statuses[b].status != AMDZK_PROOF_WELL_FORMED) continue;
    if (h_status[b] != STATUS_CLEAN) {
      statuses[b].status = h_status[b] & 3u, statuses[b].offset = h_status[b] >> 2;
      continue;
    }
    live++;
    const Group& gr = groups[group_of[b]];
    const verifier::Plan& plan = gr.plan;
    const Item& it = items[b];
    const uint64_t* const* const* inst_b = plan.I ? it.instances : nullptr;
    const size_t* const* lens_b = plan.I ? it.instance_lens : nullptr;
    const G1Affine* pts = h_points + L.item_points[b];
    const Fr* scs = h_scalars + L.item_scalars[b];
    Lb.resize(plan.n_bases), Rb.resize(plan.n_bases);
    if (it.transcript) verifier::fold_challenges(plan, *gr.key.omega, inst_b, lens_b, scs, rho[b], read_ch[b], Lb.data(), Rb.data());
    else verifier::fold_proof(plan, *gr.key.transcript_repr, *gr.key.omega, inst_b, lens_b, pts, scs, rho[b], Lb.data(), Rb.data());
    if (per_proof) {
      own_at.push_back(own.size());
      own.insert(own.end(), Lb.begin(), Lb.end());
      own.insert(own.end(), Rb.begin(), Rb.end());
      who_b.push_back(b);
      continue;
    }
    const size_t vk0 = L.group_vk[group_of[b]];
    for (uint32_t i = 0; i < plan.n_bases; i++) {
      // the item's own points | its group's fixed and permutation commitments | G
      const size_t at = i < plan.NP ? L.nvk + 1 + L.item_points[b] + i : i == plan.base_g ? L.nvk : vk0 + (i - plan.NP);
      msm[at] = add(msm[at], Lb[i]);
      msm[nbases + at] = add(msm[nbases + at], Rb[i]);
    }
  }
  if (live == 0) return AMDZK_OK;
  if (per_proof) {
    // ---- (L_b, R_b) for every live item: per run of AMDZK_DECIDE_RUN positions one MSM of 2 columns per live item over the
    // commitments of the groups present in the run, G and the run's decoded points. One host wait per run.
    std::vector<uint64_t> jac(24 * L.run);
    std::vector<size_t> vk_at(G);  // where a present group's commitments sit in the run's base list
    std::vector<uint8_t> present(G);
    for (size_t lo = 0, b0 = 0; b0 < n_items; b0 += L.run) {
      const size_t b1 = b0 + L.run < n_items ? b0 + L.run : n_items;
      size_t hi = lo;
      while (hi < who_b.size() && who_b[hi] < b1) hi++;
      const size_t nl = hi - lo;
      if (nl == 0) continue;
      present.assign(G, 0);
      size_t nv = 0;
      for (size_t b = b0; b < b1; b++) {
        const uint32_t g = group_of[b];
        if (present[g]) continue;
        present[g] = 1, vk_at[g] = nv;
        if (groups[g].nvk)
          ZK_HIP(ctx, hipMemcpyAsync(ws + L.run_bases + nv * sizeof(G1Affine), ws + L.vk + L.group_vk[g] * sizeof(G1Affine), groups[g].nvk * sizeof(G1Affine),
                                     hipMemcpyDeviceToDevice, ctx->stream));
        nv += groups[g].nvk;
      }
      const size_t p0 = L.item_points[b0], np = (b1 < n_items ? L.item_points[b1] : L.n_points) - p0, len = nv + 1 + np;
      ZK_HIP(ctx, hipMemcpyAsync(ws + L.run_bases + nv * sizeof(G1Affine), ws + L.g, sizeof(G1Affine), hipMemcpyDeviceToDevice, ctx->stream));
      if (np)
        ZK_HIP(ctx, hipMemcpyAsync(ws + L.run_bases + (nv + 1) * sizeof(G1Affine), ws + L.points + p0 * sizeof(G1Affine), np * sizeof(G1Affine),
                                   hipMemcpyDeviceToDevice, ctx->stream));
      msm.assign(2 * nl * len, Fr::zero());
      for (size_t q = 0; q < nl; q++) {
        const size_t b = who_b[lo + q];
        const verifier::Plan& plan = groups[group_of[b]].plan;
        for (int side = 0; side < 2; side++) {
          const Fr* src = own.data() + own_at[lo + q] + (size_t)side * plan.n_bases;
          Fr* col = msm.data() + (2 * q + side) * len;
          for (uint32_t i = 0; i < plan.n_bases; i++)
            col[i < plan.NP ? nv + 1 + (L.item_points[b] - p0) + i : i == plan.base_g ? nv : vk_at[group_of[b]] + (i - plan.NP)] = src[i];
        }
      }
      ZK_HIP(ctx, hipMemcpyAsync(ws + L.msm, msm.data(), msm.size() * 32, hipMemcpyHostToDevice, ctx->stream));
      G1X* d_res = nullptr;
      ZK_TRY(zk_msm_bases_dev_xyzz(ctx, (const Fr*)(ws + L.msm), 2 * nl, len, len, (const G1Affine*)(ws + L.run_bases), &d_res));
      ZK_TRY(zk_msm_finish(ctx, d_res, 2 * nl, jac.data()));
      for (size_t q = 0; q < 2 * nl; q++) {
        const G1Jac* j = reinterpret_cast<const G1Jac*>(jac.data() + 12 * q);
        if (j->z.is_zero()) continue;  // the identity stays (0, 0)
        G1Affine& o = (*pairs)[2 * who_b[lo + q / 2] + (q & 1)];
        o.x = j->x, o.y = j->y;
      }
      lo = hi;
    }
    return AMDZK_OK;
  }
  // ---- L and R: one MSM of two columns over every group's commitments, G and every item's decoded points
  ZK_HIP(ctx, hipMemcpyAsync(ws + L.msm, msm.data(), 2 * nbases * 32, hipMemcpyHostToDevice, ctx->stream));
  G1X* d_res = nullptr;
  ZK_TRY(zk_msm_bases_dev_xyzz(ctx, (const Fr*)(ws + L.msm), 2, nbases, nbases, (const G1Affine*)(ws + L.vk), &d_res));
  uint64_t jac[24];
  ZK_TRY(zk_msm_finish(ctx, d_res, 2, jac));  // wait 2 of 2
  for (int c = 0; c < 2; c++) {
    const G1Jac* j = reinterpret_cast<const G1Jac*>(jac + 12 * c);
    if (j->z.is_zero()) continue;  // the identity stays (0, 0)
    memcpy(pair_out + 8 * c, &j->x, 32);
    memcpy(pair_out + 8 * c + 4, &j->y, 32);
  }
  return AMDZK_OK;
}

// amdzk_verify_proofs_decide and its kin: verify_core and the pairing(s) behind it, over n proofs.
int decide_core(amdzk_ctx* ctx, const char* who, const Adapter& fill, size_t n, const amdzk_g2* s_g2, const amdzk_g2* g2, uint32_t flags,
                amdzk_proof_status* statuses, uint8_t* verdicts, size_t* n_valid) {
  if (!s_g2 || !g2 || !verdicts) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: null argument", who);
  if (flags & ~AMDZK_DECIDE_COMBINED) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: unknown flags 0x%x", who, flags);
  const bool combined = (flags & AMDZK_DECIDE_COMBINED) != 0;
  std::vector<G1Affine> pairs;
  uint64_t pair[16];
  ZK_TRY(verify_core(ctx, who, fill, statuses, pair, combined ? nullptr : &pairs));
  if (combined) {
    pairs.resize(2);
    memcpy(&pairs[0], pair, 64);
    memcpy(&pairs[1], pair + 8, 64);
  }
  return decide_pairs(ctx, who, s_g2, g2, combined, pairs, n, statuses, verdicts, n_valid);
}

// The adapter of the calls over ONE key, through a view of it (key == nullptr: the caller passed no key): one group and one
// transcript kind for the whole call, its low byte masked only when every proof has a read transcript.
int single_key_call(amdzk_ctx* ctx, const char* who, const zk_key_view* key, size_t n_proofs, const uint64_t* const* const* instances,
                    const size_t* const* instance_lens, const uint8_t* const* proofs, const size_t* proof_lens, const amdzk_verify_opts* opts, Call* call) {
  if (!key) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: null argument", who);
  if (n_proofs == 0) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: n_proofs is 0", who);
  if (n_proofs > (1u << 20)) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: more than 2^20 proofs in one call", who);
  // the struct as it was before `transcripts` is still a caller's right: exactly that size, or this library's
  constexpr size_t LEGACY_OPTS = offsetof(amdzk_verify_opts, transcripts);
  if (opts && opts->size != LEGACY_OPTS && opts->size < sizeof(amdzk_verify_opts))
    ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: amdzk_verify_opts.size is %zu, this library needs %zu", who, opts->size, sizeof(amdzk_verify_opts));
  const amdzk_transcript_read* const* trs = opts && opts->size >= sizeof(amdzk_verify_opts) ? opts->transcripts : nullptr;
  size_t n_tr = 0;
  for (size_t b = 0; trs && b < n_proofs; b++) n_tr += trs[b] != nullptr;
  if (n_tr < n_proofs && (!proofs || !proof_lens)) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: null argument", who);
  for (size_t b = 0; b < n_proofs; b++)
    if (!(trs && trs[b]) && !proofs[b]) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: null argument (proof %zu)", who, b);
  Group gr;
  gr.key = *key, gr.handle = key, gr.first = 0;
  gr.n_circuits = opts && opts->n_circuits ? opts->n_circuits : 1;
  gr.kind = (opts ? opts->transcript_kind : 0) & (n_tr == n_proofs ? ~0xff : ~0);
  // proof b's instances are N entries of the call's flat arrays; an N that make_plan will refuse shapes no pointer
  const size_t N = gr.n_circuits <= (1u << 16) ? gr.n_circuits : 0;
  call->groups.push_back(std::move(gr));
  call->group_of.assign(n_proofs, 0);
  call->items.resize(n_proofs);
  for (size_t b = 0; b < n_proofs; b++)
    call->items[b] = {instances ? instances + b * N : nullptr, instance_lens ? instance_lens + b * N : nullptr, proofs ? proofs[b] : nullptr,
                      proof_lens ? proof_lens[b] : 0, trs ? trs[b] : nullptr};
  call->combine_scalars = opts ? opts->combine_scalars : nullptr, call->combine_seed = opts ? opts->combine_seed : 0;
  return AMDZK_OK;
}

// The adapter of the calls over a key PER ITEM: the items grouped (verifier.hpp, group_items), a read-transcript item's kind
// masked by itself, every refusal about an item labelled with it.
int mixed_call(amdzk_ctx* ctx, const char* who, const amdzk_verify_item* items, size_t n_items, const amdzk_verify_mixed_opts* opts, Call* call) {
  if (!items) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: null argument", who);
  if (n_items == 0) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: n_items is 0", who);
  if (n_items > (1u << 20)) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: more than 2^20 items in one call", who);
  if (opts && opts->size < sizeof(amdzk_verify_mixed_opts))
    ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: amdzk_verify_mixed_opts.size is %zu, this library needs %zu", who, opts->size, sizeof(amdzk_verify_mixed_opts));
  std::vector<verifier::MixedKey> mk(n_items);
  call->labelled = true;
  call->items.resize(n_items);
  for (size_t b = 0; b < n_items; b++) {
    const amdzk_verify_item& it = items[b];
    if ((it.pk != nullptr) == (it.vk != nullptr)) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: item %zu: exactly one of pk and vk must be set", who, b);
    if (!it.transcript && !it.proof) ZK_FAIL(ctx, AMDZK_E_INVALID, "%s: item %zu: null argument (proof)", who, b);
    // a read-transcript item: only the opening scheme's bit counts
    mk[b] = {it.pk ? (const void*)it.pk : (const void*)it.vk, it.n_circuits ? it.n_circuits : 1, it.transcript ? it.transcript_kind & ~0xff : it.transcript_kind};
    call->items[b] = {it.instances, it.instance_lens, it.proof, it.proof_len, it.transcript};
  }
  std::vector<size_t> firsts;
  call->group_of = verifier::group_items(mk.data(), n_items, &firsts);
  call->groups.resize(firsts.size());
  for (size_t g = 0; g < firsts.size(); g++) {
    const size_t b = firsts[g];
    Group& gr = call->groups[g];
    gr.key = items[b].pk ? view_of(items[b].pk) : view_of(items[b].vk);
    gr.handle = mk[b].key, gr.n_circuits = mk[b].n_circuits, gr.kind = mk[b].kind, gr.first = b;
  }
  call->combine_scalars = opts ? opts->combine_scalars : nullptr, call->combine_seed = opts ? opts->combine_seed : 0;
  return AMDZK_OK;
}

}  // namespace

int zk_points_check_dev(amdzk_ctx* ctx, G1Affine* d_pts, size_t n, size_t inf_below, uint32_t* d_status) {
  if (n == 0 || n >= ((size_t)1 << 30)) ZK_FAIL(ctx, AMDZK_E_INVALID, "points_check: %zu points", n);
  ZK_HIP(ctx, hipMemsetAsync(d_status, 0xff, sizeof(uint32_t), ctx->stream));
  ZK_LAUNCH(ctx, "points_check", points_check_kernel, dim3((unsigned)((n + DECODE_THREADS - 1) / DECODE_THREADS)), dim3(DECODE_THREADS), 0, d_pts, (uint32_t)n,
            (uint32_t)(inf_below < n ? inf_below : n), d_status);
  return AMDZK_OK;
}

// The entry points over either key: the view (no key: no view, which the adapter refuses), the body, and — a refused call may
// have copies in flight out of vectors that die with it — the stream idle before a refusal returns.
template <class Key>
static int verify_entry(amdzk_ctx* ctx, const Key* k, size_t n_proofs, const uint64_t* const* const* instances, const size_t* const* instance_lens,
                        const uint8_t* const* proofs, const size_t* proof_lens, const amdzk_verify_opts* opts, amdzk_proof_status* statuses,
                        uint64_t* pair_out) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  const char* who = "verify_proofs";
  zk_key_view key;
  if (k) key = view_of(k);
  const Adapter fill = [&](Call* c) { return single_key_call(ctx, who, k ? &key : nullptr, n_proofs, instances, instance_lens, proofs, proof_lens, opts, c); };
  return zk_quiet_if_refused(ctx, verify_core(ctx, who, fill, statuses, pair_out, nullptr));
}
template <class Key>
static int decide_entry(amdzk_ctx* ctx, const Key* k, const amdzk_g2* s_g2, const amdzk_g2* g2, uint32_t flags, size_t n_proofs,
                        const uint64_t* const* const* instances, const size_t* const* instance_lens, const uint8_t* const* proofs,
                        const size_t* proof_lens, const amdzk_verify_opts* opts, amdzk_proof_status* statuses, uint8_t* verdicts, size_t* n_valid) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  const char* who = "verify_proofs_decide";
  zk_key_view key;
  if (k) key = view_of(k);
  const Adapter fill = [&](Call* c) { return single_key_call(ctx, who, k ? &key : nullptr, n_proofs, instances, instance_lens, proofs, proof_lens, opts, c); };
  return zk_quiet_if_refused(ctx, decide_core(ctx, who, fill, n_proofs, s_g2, g2, flags, statuses, verdicts, n_valid));
}

extern "C" int amdzk_verify_proofs(amdzk_ctx* ctx, const amdzk_pk* pk, size_t n_proofs, const uint64_t* const* const* instances,
                                   const size_t* const* instance_lens, const uint8_t* const* proofs, const size_t* proof_lens,
                                   const amdzk_verify_opts* opts, amdzk_proof_status* statuses, uint64_t pair_out[16]) {
  return verify_entry(ctx, pk, n_proofs, instances, instance_lens, proofs, proof_lens, opts, statuses, pair_out);
}
extern "C" int amdzk_verify_proofs_vk(amdzk_ctx* ctx, const amdzk_vk* vk, size_t n_proofs, const uint64_t* const* const* instances,
                                      const size_t* const* instance_lens, const uint8_t* const* proofs, const size_t* proof_lens,
                                      const amdzk_verify_opts* opts, amdzk_proof_status* statuses, uint64_t pair_out[16]) {
  return verify_entry(ctx, vk, n_proofs, instances, instance_lens, proofs, proof_lens, opts, statuses, pair_out);
}
extern "C" int amdzk_verify_proofs_decide(amdzk_ctx* ctx, const amdzk_pk* pk, const amdzk_g2* s_g2, const amdzk_g2* g2, uint32_t flags,
                                          size_t n_proofs, const uint64_t* const* const* instances, const size_t* const* instance_lens,
                                          const uint8_t* const* proofs, const size_t* proof_lens, const amdzk_verify_opts* opts,
                                          amdzk_proof_status* statuses, uint8_t* verdicts, size_t* n_valid) {
  return decide_entry(ctx, pk, s_g2, g2, flags, n_proofs, instances, instance_lens, proofs, proof_lens, opts, statuses, verdicts, n_valid);
}
extern "C" int amdzk_verify_proofs_decide_vk(amdzk_ctx* ctx, const amdzk_vk* vk, const amdzk_g2* s_g2, const amdzk_g2* g2, uint32_t flags,
                                             size_t n_proofs, const uint64_t* const* const* instances, const size_t* const* instance_lens,
                                             const uint8_t* const* proofs, const size_t* proof_lens, const amdzk_verify_opts* opts,
                                             amdzk_proof_status* statuses, uint8_t* verdicts, size_t* n_valid) {
  return decide_entry(ctx, vk, s_g2, g2, flags, n_proofs, instances, instance_lens, proofs, proof_lens, opts, statuses, verdicts, n_valid);
}

// ... and over a batch of different keys: one prefix for both calls.
extern "C" int amdzk_verify_proofs_mixed(amdzk_ctx* ctx, const amdzk_verify_item* items, size_t n_items, const amdzk_verify_mixed_opts* opts,
                                         amdzk_proof_status* statuses, uint64_t pair_out[16]) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  const char* who = "verify_proofs_mixed";
  const Adapter fill = [&](Call* c) { return mixed_call(ctx, who, items, n_items, opts, c); };
  return zk_quiet_if_refused(ctx, verify_core(ctx, who, fill, statuses, pair_out, nullptr));
}
extern "C" int amdzk_verify_proofs_decide_mixed(amdzk_ctx* ctx, const amdzk_g2* s_g2, const amdzk_g2* g2, uint32_t flags, const amdzk_verify_item* items,
                                                size_t n_items, const amdzk_verify_mixed_opts* opts, amdzk_proof_status* statuses, uint8_t* verdicts,
                                                size_t* n_valid) {
  ZK_ENTER(ctx);
  if (!ctx) return AMDZK_E_INVALID;
  const char* who = "verify_proofs_mixed";
  const Adapter fill = [&](Call* c) { return mixed_call(ctx, who, items, n_items, opts, c); };
  return zk_quiet_if_refused(ctx, decide_core(ctx, who, fill, n_items, s_g2, g2, flags, statuses, verdicts, n_valid));
}
