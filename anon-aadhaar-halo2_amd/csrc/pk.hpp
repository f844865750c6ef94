// The proving key as every host unit of the PLONK layer sees it (keygen.hip makes and frees it, program.hip compiles and
// runs its programs, prover.hip proves with it, check.hip checks a witness against it), in two types:
//
//   KeyMaterial  what is the same for every handle of a key: the circuit's shape and description, the domain, the fixed
//                and permutation columns, the permutation lists, the constant lookup tables, the programs' text and the
//                rotation table they index, the commitments. Keygen fills it and nothing writes it afterwards: handles
//                hold it as shared_ptr<const KeyMaterial>, so a proof, a check or a verification that tried to would not
//                compile. The last handle that lets go frees it.
//   amdzk_pk     a handle: the pointer to the material and ONE circuit instance's per-proof workspace — the arenas and
//                scratch buffers, the constant table with this proof's challenges in it, the slot -> pointer tables and the
//                programs resolved to this workspace's addresses, the cached multiopen lists, the witness check's program
//                and counters, the pinned staging ring. Keygen returns one; amdzk_pk_clone_workspace makes another of the
//                same material. Handles of one key are equals: they are freed in any order.
//
// A new field goes into KeyMaterial if keygen can compute it from the circuit, the columns and the SRS alone and every
// proof reads the same value; into amdzk_pk if it holds an address of the arenas, a value of one proof (a challenge, an
// error word), or a buffer that two proofs in flight must not share. What is derived from the material after keygen (the
// decoded permutation of the witness check) lives behind a pointer the material holds, with a guard of its own.
#pragma once
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "opening.hpp"
#include "pkblob.hpp"
#include "plonk_kernels.hpp"

using namespace bn254;  // (every unit that includes this header says so itself)

// host-format expression words (include/amdzk.h)
enum : uint32_t { XOP_CONST = 1, XOP_FIXED = 2, XOP_ADVICE = 3, XOP_INSTANCE = 4, XOP_NEG = 5, XOP_ADD = 6, XOP_MUL = 7, XOP_SCALE = 8, XOP_CHALLENGE = 9 };

using zkhost::fr_delta;  // Fr::DELTA (hostcrypto.hpp)

// A program's text: slots, rotation indices and constant indices, the same for every workspace of a key.
struct ProgramText {
  std::vector<uint32_t> words;
  uint32_t depth = 0, cur = 0;
  bool uses_hot = false;
  // Lagrange-domain programs: instruction indices at which an independent piece starts (the stack is empty there):
  // run_program cuts the program there into up to EXPR_MAX_PARTS parts that run side by side (ExprArgs::nparts)
  std::vector<uint32_t> piece_starts;
  void piece() { piece_starts.push_back((uint32_t)words.size()); }
  // h(X) programs: term j (closed by the j-th OP_ACC) carries the factor beta^term_beta[j] in its power of y
  std::vector<uint32_t> term_beta;
  uint32_t next_beta = 0;
  void op(uint32_t o, uint32_t arg = 0) {
    words.push_back((o << 24) | (arg & 0xffffffu));
    if (o == OP_ACC) {
      term_beta.push_back(next_beta);
      next_beta = 0;
    }
  }
  void push() {
    cur++;
    if (cur > depth) depth = cur;
  }
  void pop() { cur--; }
};
// ... and the program as one workspace runs it: the text resolved to that workspace's addresses (upload_program)
struct Program {
  const ProgramText* text = nullptr;
  ExprInstr* d_instr = nullptr;  // resolved instructions (device)
};

struct RotTable {
  std::vector<int32_t> rots;
  int find(int32_t r) const {  // -1: not in the table
    for (size_t i = 0; i < rots.size(); i++)
      if (rots[i] == r) return (int)i;
    return -1;
  }
  uint32_t index(int32_t r) {  // ... added to it (keygen)
    if (find(r) < 0) rots.push_back(r);
    return (uint32_t)find(r);
  }
};

struct KeyMaterial {
  uint32_t k = 0, ek = 0, bf = 0, degree = 0, F = 0, A = 0, I = 0, S = 0, L = 0, nsets = 0, chunk = 0, qdeg = 0;
  uint32_t nc = 0;       // cosets of the quotient domain (poly.hip zk_quotient_plan): qdeg of the 2^(ek-k) upstream uses
  size_t n = 0, ext = 0;  // ext = nc * n rows: every "extended" column holds [coset][row]
  size_t NP = 0;          // columns of a workspace's arenas: adv | inst | la | ls | zp | zl
  std::vector<std::pair<int, int>> advice_queries, fixed_queries, instance_queries;
  std::vector<std::pair<int, int>> perm_cols;  // (kind, index)
  std::vector<std::vector<uint32_t>> exprs;
  uint32_t num_gates = 0;
  std::vector<std::pair<uint32_t, uint32_t>> lookup_shape;  // (#inputs, #tables); expressions follow the gates in order
  // The constant table as a new workspace starts with it: circuit constants, one, then the slots a proof fills
  // (theta ... 1/beta and the phase challenges), zero here.
  std::vector<Fr> consts;
  uint32_t c_one = 0, c_theta = 0, c_beta = 0, c_gamma = 0, c_y = 0, c_betainv = 0;
  // Challenge phases (amdzk_keygen_phased): challenge i lives in slot c_chal0 + i of the constant table, refreshed per
  // proof like theta ... y; nothing made at keygen reads those slots. nphases = 1 and no challenges: a phase-0 key.
  uint32_t num_challenges = 0, c_chal0 = 0, nphases = 1;
  std::vector<uint8_t> advice_phase, challenge_phase;
  bool phased() const { return nphases > 1 || num_challenges > 0; }
  amdzk_domain* dom = nullptr;
  const amdzk_srs* srs = nullptr;
  Fr transcript_repr, omega, omega_inv;
  std::vector<G1Affine> fixed_commitments, perm_commitments;
  // What keygen was given, as the caller passed it (the flattened amdzk_circuit arrays and the phase table): the header of
  // the key file (amdzk_pk_write), and what a verifying key made from this one shares.
  std::shared_ptr<const pkblob::Desc> src_desc;

  // device columns
  Fr *fixed_lag = nullptr, *fixed_poly = nullptr, *fixed_coset = nullptr;
  Fr *sigma_lag = nullptr, *sigma_poly = nullptr, *sigma_coset = nullptr;
  Fr *l0_c = nullptr, *llast_c = nullptr, *lactive_c = nullptr, *x_coset = nullptr, *omega_pow = nullptr;
  // delta^j * omega^i ([S][n], Lagrange) and delta^j * X on the quotient cosets ([S][ext], radix 2^261): the identity
  // permutation's columns. With them v + beta delta^j X + gamma = beta (delta^j X + w), w = (v + gamma) / beta — the SAME w
  // that serves v + beta sigma + gamma = beta (sigma + w): three products per permutation column instead of four, in
  // the Lagrange-domain fractions and in h(X) (the beta^m of a set cancels in a fraction and rides on the term's power of y).
  Fr *dxw_lag = nullptr, *dx_coset = nullptr;
  // The cells of the permutation products that can change them (keygen.hip build_perm_lists): per column set s the usable
  // rows i < u where some column c of the set has sigma_c(omega^i) != delta^c omega^i, ascending — on every other row the
  // set's fraction is 1 whatever the witness. perm_rank[s][i], i <= u (stride u + 1): the set's listed rows below i;
  // perm_off[s]: the listed cells of the sets before s (perm_off[nsets] = perm_m, all of them); perm_list: the cells as
  // (set, row), set after set. Derived from the sigma columns, so never in the key file. perm_sparse:
  // Prover::perm_products walks the list instead of the columns (perm_m <= nsets * u / 2); the list is kept only then.
  uint32_t *perm_rank = nullptr, *perm_off = nullptr;
  uint2* perm_list = nullptr;
  size_t perm_m = 0;
  bool perm_sparse = false;
  // The first lk_const lookups have ONE table expression over fixed columns and constants only: their compressed table
  // does not depend on theta or on the witness, so its sorted canonical form is made once at keygen ([lk_const][n]).
  uint32_t lk_const = 0;
  Fr* lk_ts_const = nullptr;
  // (Permuting the lookups among them that also have ONE input expression before theta exists, on lane C beside the advice
  // commitment, was measured and dropped: a proof alone took 19.1-19.3 ms with it against 18.7-19.0 without, 21
  // proofs x 3 alternating runs, profiles/r03q_constant_tables_and_early_lookups.txt — the small sort kernels stretch the
  // chip-filling commitment by more than they save behind theta; started behind its level-1 kernel instead they stretch
  // its bucket reduction and lane B's transforms: 18.0-18.2 ms against 17.6-17.95.)
  // programs: text, and the rotation table their column operands index
  ProgramText prog_compress, prog_pfrac, prog_lfrac, prog_h;
  RotTable rots;
  uint32_t h_terms = 0;                   // terms of the h(X) program = powers of y its OP_WACC ops index
  std::vector<uint32_t> h_term_beta_pow;  // per term of the h(X) program: the power of beta its power of y is multiplied by
  // Lanes (common.hpp): 0 = the caller's ctx, 1 and 2 = its auxiliary streams. AMDZK_KEYGEN_SERIAL / AMDZK_SERIAL=1
  // keeps everything on the caller's stream (one proof's kernels strictly one after another, as in rounds 1-2).
  bool use_lanes = true;
  uint32_t max_sets = 16, max_set_points = 0;
  std::vector<void*> allocs;  // the device buffers above
  // The one thing derived after keygen: the sigma columns decoded to (column, row), 2 x u32 per cell ([S][n]), by the
  // first amdzk_check_witness on any handle of the key — under the guard, as zk_srs_ensure_prefix derives its basis.
  // Behind a pointer, so that a const material can still fill it. Never in the key file.
  struct CheckShared {
    std::mutex guard;
    bool decoded = false;
    uint2* d_cells = nullptr;
  };
  std::unique_ptr<CheckShared> chk_shared{new CheckShared};

  ~KeyMaterial();  // keygen.hip: the device buffers, the decoded permutation, the domain

  // slots, Lagrange table
  uint32_t sl_fixed(uint32_t c) const { return c; }
  uint32_t sl_adv(uint32_t c) const { return F + c; }
  uint32_t sl_inst(uint32_t c) const { return F + A + c; }
  uint32_t sl_sigma(uint32_t c) const { return F + A + I + c; }
  uint32_t sl_ci(uint32_t l) const { return F + A + I + S + l; }
  uint32_t sl_ct(uint32_t l) const { return F + A + I + S + L + l; }
  uint32_t sl_la(uint32_t l) const { return F + A + I + S + 2 * L + l; }
  uint32_t sl_ls(uint32_t l) const { return F + A + I + S + 3 * L + l; }
  uint32_t sl_omega() const { return F + A + I + S + 4 * L; }
  uint32_t sl_dxw(uint32_t c) const { return F + A + I + S + 4 * L + 1 + c; }
  uint32_t nslots_lag() const { return F + A + I + 2 * S + 4 * L + 1; }
  // slots, extended table
  uint32_t se_sigma(uint32_t c) const { return F + A + I + c; }
  uint32_t se_zp(uint32_t s) const { return F + A + I + S + s; }
  uint32_t se_zl(uint32_t l) const { return F + A + I + S + nsets + l; }
  uint32_t se_la(uint32_t l) const { return F + A + I + S + nsets + L + l; }
  uint32_t se_ls(uint32_t l) const { return F + A + I + S + nsets + 2 * L + l; }
  uint32_t se_l0() const { return F + A + I + S + nsets + 3 * L; }
  uint32_t se_llast() const { return se_l0() + 1; }
  uint32_t se_lactive() const { return se_l0() + 2; }
  uint32_t se_x() const { return se_l0() + 3; }
  uint32_t se_dx(uint32_t c) const { return se_l0() + 4 + c; }
  uint32_t nslots_ext() const { return se_l0() + 4 + S; }
};

struct amdzk_pk {
  std::shared_ptr<const KeyMaterial> key;
  amdzk_pk() = default;
  amdzk_pk(const amdzk_pk&) = delete;  // (programs and tables below hold this workspace's addresses)
  amdzk_pk& operator=(const amdzk_pk&) = delete;
  // P: the committed columns' Lagrange values [NP][n] (what commit_lagrange and the Lagrange-domain programs read);
  // PQ: their coefficients [NP][n] (evaluations, multiopen); PC: their values on the quotient domain [NP][ext].
  // Out of place, so that a phase's transforms run on a lane while its commitments and the next phase's programs
  // still read the Lagrange values. Arena order: adv | inst | la | ls | zp | zl.
  Fr *P = nullptr, *PQ = nullptr, *PC = nullptr;
  Fr *ci = nullptr, *ct = nullptr;  // [L][n] compressed lookup input / table
  Fr *rnd = nullptr, *hq = nullptr, *hpieces = nullptr, *hpoly = nullptr, *frac = nullptr, *scratch = nullptr, *scan_tmp = nullptr;
  Fr *frac2 = nullptr, *scratch2 = nullptr, *scan_tmp2 = nullptr;  // the lookup products' own scratch: they run beside the permutation products
  Fr *sets_L = nullptr, *sets_N = nullptr, *sets_Q = nullptr, *hx = nullptr;  // SHPLONK buffers
  size_t sets_Q_pairs = 0;  // (set, point) pairs sets_Q holds n coefficients for
  // What the multiopen argument derives from the key alone, built by the first proof (the polynomials live at fixed
  // addresses in this workspace): the evaluation list, the query list and its grouping (opening.hpp) in terms of
  // rotations. Only the ORDER of a set's points (upstream keeps them in a BTreeSet of field elements) depends on x.
  struct Multiopen {
    bool built = false;
    std::vector<std::pair<const Fr*, int>> ev;      // (polynomial, rotation) in the order the evaluations are written
    size_t n_written = 0;                           // ... of which the first n_written go to the transcript
    std::vector<int> rots;                          // distinct rotations, first seen first
    std::vector<uint32_t> ev_rot;                   // per evaluation: index into rots
    std::vector<const Fr*> com_poly;                // the queried polynomials, first seen first: grp's commitment ids
    std::vector<opening::Query> q;                  // the queries, upstream order: (index into com_poly, index into rots)
    std::vector<uint32_t> q_ev;                     // per query: index into ev
    opening::Grouping grp;                          // SHPLONK's rotation sets and GWC's point sets over q
  } mo;
  // create_proof over several circuit instances (amdzk_create_proof_multi): the evaluation / query lists over all of
  // them, built by the first such proof on this handle for a given list of instance handles
  Multiopen mo_multi;
  std::vector<const amdzk_pk*> mo_multi_keys;
  Fr *lk_ts = nullptr, *lk_left = nullptr;  // lookup permutation: sorted tables, leftovers [L][n]
  uint32_t* lk_flags = nullptr;              // [4][L][n+8]
  int* d_err = nullptr;
  int* h_err = nullptr;                      // pinned: where create_proof reads d_err (the first word of `pin`'s tail block)
  // misc small device buffers (blinding uploads, points, evals, coefs) and pointer-table scratch, one slice per lane:
  // a slice is reused in stream order by the lane that owns it
  Fr* small_l[3] = {nullptr, nullptr, nullptr};
  void* ptrs_l[3] = {nullptr, nullptr, nullptr};
  Fr* small = nullptr;   // = small_l[0]
  void* ptrs = nullptr;  // = ptrs_l[0]
  size_t small_cap = 0, ptrs_cap = 0;
  // the constant table with this proof's challenges in it (host copy, device copy, the same times 32 = radix 2^261: the
  // constants of programs run on the extended domain), and y^(h_terms-1-j) in radix 2^261, refreshed per proof
  std::vector<Fr> consts;
  Fr *d_consts = nullptr, *d_consts261 = nullptr, *d_ypow = nullptr;
  // slot -> column tables (key columns and this workspace's arenas), their host copies (program resolution), where the
  // Lagrange-domain programs store, and the key's four programs resolved to this workspace
  const Fr** d_cols_lag = nullptr;
  const Fr** d_cols_ext = nullptr;
  const Fr** d_perm_cols = nullptr;  // [S]: the permutation columns' values (advice, fixed or instance) in this workspace
  Fr** d_outs_compress = nullptr;
  Fr** d_outs_pfrac = nullptr;
  Fr** d_outs_lfrac = nullptr;
  std::vector<const Fr*> h_cols_lag, h_cols_ext;
  Program prog_compress, prog_pfrac, prog_lfrac, prog_h;
  // amdzk_check_witness, made by the handle's first check (the instructions carry this workspace's column addresses):
  // the gate polynomials as one Lagrange-domain program, gate g ending in OP_CHECK g; the counters, count[ncon] (u64)
  // followed by first[ncon] (u32), constraints in report order (gates, lookups, permutation columns).
  // (The copy check reads the permutation columns through d_perm_cols above.)
  struct Check {
    bool built = false;
    ProgramText gates;
    Program prog_gates;
    unsigned long long* d_count = nullptr;
    uint32_t* d_first = nullptr;
  } chk;
  // pinned host staging (bump allocator, reset whenever the stream is known to be idle)
  char* pin = nullptr;
  size_t pin_cap = 0, pin_off = 0;
  std::vector<void*> allocs;  // what this handle allocated on the device
  // ... of which the per-proof arenas (address, bytes): what zk_pk_poison fills (alloc_proof_workspace lists them; ptrs_l,
  // which holds device addresses, is not among them)
  std::vector<std::pair<void*, size_t>> arenas;

  Fr* adv() const { return P; }
  Fr* inst() const { return P + (size_t)key->A * key->n; }
  Fr* la() const { return P + (size_t)(key->A + key->I) * key->n; }
  Fr* ls() const { return P + (size_t)(key->A + key->I + key->L) * key->n; }
  Fr* zp() const { return P + (size_t)(key->A + key->I + 2 * key->L) * key->n; }
  Fr* zl() const { return P + (size_t)(key->A + key->I + 2 * key->L + key->nsets) * key->n; }
  Fr* q_adv() const { return PQ; }
  Fr* q_la() const { return PQ + (size_t)(key->A + key->I) * key->n; }
  Fr* q_ls() const { return PQ + (size_t)(key->A + key->I + key->L) * key->n; }
  Fr* q_zp() const { return PQ + (size_t)(key->A + key->I + 2 * key->L) * key->n; }
  Fr* q_zl() const { return PQ + (size_t)(key->A + key->I + 2 * key->L + key->nsets) * key->n; }
};

// a device buffer of the material under construction or of a handle, freed with its owner
template <class Owner, class T>
int dalloc(amdzk_ctx* ctx, Owner* pk, T** p, size_t count) {
  void* q = nullptr;
  hipError_t e = hipMalloc(&q, (count ? count : 1) * sizeof(T));
  if (e != hipSuccess) ZK_FAIL(ctx, AMDZK_E_NOMEM, "prover: hipMalloc(%zu) failed: %s", count * sizeof(T), hipGetErrorString(e));
  pk->allocs.push_back(q);
  *p = (T*)q;
  return AMDZK_OK;
}

// stream-ordered copies on ctx's stream (keygen.hip); d2h also waits for it
int h2d(amdzk_ctx* ctx, void* d, const void* h, size_t bytes);
// host -> device through the key's pinned staging area: the source may be a temporary, and the copy
// is truly asynchronous (no pageable-memory staging inside the runtime).
int h2d_staged(amdzk_ctx* ctx, amdzk_pk* pk, void* d, const void* h, size_t bytes);
int d2h(amdzk_ctx* ctx, void* h, const void* d, size_t bytes);
int d2d(amdzk_ctx* ctx, void* dst, const void* src, size_t bytes);
// AMDZK_WS_POISON (workspace.hpp): the handle's arenas filled with the pattern; a branch on ctx->ws_poison otherwise (keygen.hip)
int zk_pk_poison(amdzk_ctx* ctx, amdzk_pk* pk);
// MSM of ncols resident columns of the key's n rows -> affine points on the host (prover.hip)
int commit_cols(amdzk_ctx* ctx, const KeyMaterial& K, int basis, const Fr* d_cols, size_t ncols, std::vector<G1Affine>& out);

// ---- keygen's steps that amdzk_keygen_vk (vk.hip) runs too (keygen.hip has them in keygen's order), on material alone.
// A verifying key's material holds the description and the F + S Lagrange columns, and nothing sized by the extended
// domain (describe_circuit's vk_only); the load steps make the coefficient and coset forms where the material has them.
int check_keygen_args(amdzk_ctx* ctx, const amdzk_srs* srs, const amdzk_circuit* c, const amdzk_phases* ph, const uint64_t transcript_repr[4],
                      uint32_t flags, const void* out, uint32_t* nphases);
int describe_circuit(amdzk_ctx* ctx, KeyMaterial& K, const amdzk_srs* srs, const amdzk_circuit* c, const amdzk_phases* ph, uint32_t nphases,
                     const uint64_t transcript_repr[4], uint32_t flags, bool vk_only);
int load_fixed_columns(amdzk_ctx* ctx, KeyMaterial& K, const void* fixed_values);
int load_sigma_columns(amdzk_ctx* ctx, KeyMaterial& K, const uint32_t* perm_mapping, const void* sigma_values, bool from_sigma);
// Owns material that no handle holds (amdzk_keygen_vk's): waits for ctx's stream, then frees it.
struct KeyFree {
  amdzk_ctx* ctx;
  void operator()(KeyMaterial* K) const;
};

// ---- programs (program.hip)
constexpr uint32_t H_PARTS_MAX = 8;  // pieces finalize_limb_program cuts an h(X) program into, at most: one h each (amdzk_pk::hq)
// grow: the rotation table of the material under construction (&K.rots, keygen), which takes the rotations the expression
// queries; null on a frozen key, where a rotation that is not in the table is refused
int emit_expr(amdzk_ctx* ctx, const KeyMaterial& K, RotTable* grow, ProgramText& pr, const std::vector<uint32_t>& words);
int emit_compressed(amdzk_ctx* ctx, KeyMaterial& K, ProgramText& pr, uint32_t first, uint32_t count);
uint32_t finalize_limb_program(ProgramText& pr, uint32_t nparts = 1);
int upload_consts261(amdzk_ctx* ctx, amdzk_pk* pk);
int upload_ypow(amdzk_ctx* ctx, amdzk_pk* pk);
int upload_program(amdzk_ctx* ctx, amdzk_pk* pk, Program& pr, bool extended);
int program_args(amdzk_ctx* ctx, const amdzk_pk* pk, const Program& pr, bool extended, Fr* const* d_outs, Fr* h_out, ExprArgs& a);
int run_program(amdzk_ctx* ctx, const amdzk_pk* pk, const Program& pr, bool extended, Fr* const* d_outs, Fr* h_out, const char* name);
// The LDS stack slots a program is launched with. The limb interpreter keeps the top of the stack in registers, so a
// program whose stack holds at most pr.depth - 1 values (finalize_limb_program) needs pr.depth - 2 slots: pr.depth - 1
// leaves one spare. The Lagrange-domain interpreters (zk_expr_eval, zk_check_expr) get one slot above the recorded depth.
inline uint32_t limb_stack_slots(const ProgramText& pr) { return pr.depth > 1 ? pr.depth - 1 : 1; }
inline uint32_t lagrange_stack_slots(const ProgramText& pr) { return pr.depth + 1; }
// Keygen's refusal of a program whose stack does not fit the device's LDS (AMDZK_E_UNSUPPORTED, naming the program, its
// depth and the depth that fits): the bytes are those the launch wrappers ask for, the limit is the device's opt-in
// maximum of shared memory per block.
int check_program_fits(amdzk_ctx* ctx, const ProgramText& pr, bool extended, const char* name);
// The witness check's gate program (check.hip builds it on a handle's first check; keygen compiles it once for its depth).
int emit_check_gates(amdzk_ctx* ctx, const KeyMaterial& K, ProgramText& pr);
