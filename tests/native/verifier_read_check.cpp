// The host half of amdzk_verify_proofs (csrc/verifier.hpp) driven through the CALLER's read transcript, without a device: the
// callback adapter (verifier::CallbackSource) over a C implementation of amdzk_transcript_read that hands back one proof's
// recorded elements and hashes them with the library's own host transcript. The per-base scalars must be those of the
// built-in route (verifier::fold_proof) bit for bit; then every callback of the walk is made to fail in turn (a non-zero
// return, a challenge that is not below r), and a NULL member is tried: the walk must end there with the number of
// completed reads. tests/test_verifier_read_host.py runs it plain and under ASan + UBSan. Plain g++, no HIP.
//   verifier_read_check <key file> <case file>          (the files of tests/native/verifier_check.cpp)
// Output: "plan <NP> <NS> <proof bytes> <bases>", one line "<base> <L> <R>" per base with a non-zero scalar (the callback
// route's, canonical, hex), "calls <commons> <reads> <squeezes>", "failures <tried>", "ok". Exit status 2 on a malformed input,
// 1 with a message when a check fails.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../anon-aadhaar-halo2_amd/csrc/verifier.hpp"

static std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> out;
  FILE* f = fopen(path, "rb");
  if (!f) return out;
  uint8_t buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + got);
  fclose(f);
  return out;
}

struct Cursor {
  const std::vector<uint8_t>& d;
  size_t pos = 0;
  bool ok = true;
  explicit Cursor(const std::vector<uint8_t>& v) : d(v) {}
  void get(void* out, size_t n) {
    if (!ok || d.size() - pos < n) {
      ok = false;
      memset(out, 0, n);
      return;
    }
    memcpy(out, d.data() + pos, n);
    pos += n;
  }
  uint32_t u32() {
    uint32_t v = 0;
    get(&v, 4);
    return v;
  }
};

static void print_fr(const bn254::Fr& a) {
  const bn254::Fr c = bn254::from_mont(a);
  for (int i = 7; i >= 0; i--) printf("%08x", c.l[i]);
}

// The caller's side: one proof's elements in read order, a hash of the caller's choosing (here the library's host
// transcripts, so that the challenges can be compared with the built-in route's), and the failure to inject.
struct Recorded {
  const verifier::Plan* plan;
  const bn254::G1Affine* pts;
  const bn254::Fr* scs;
  zkhost::TranscriptWrite* hash;
  size_t next = 0;                           // element to hand back
  size_t calls = 0, commons = 0, reads = 0, squeezes = 0;
  size_t fail_at = (size_t)-1;               // this call (counted over all members) returns non-zero ...
  size_t big_at = (size_t)-1;                // ... or, being a squeeze, hands back the modulus
  bool step() { return calls++ == fail_at; }
};

static int cb_common_point(void*, const uint64_t*) { return 7; }  // the verifier never calls it
static int cb_common_scalar(void* u, const uint64_t* s) {
  Recorded& r = *(Recorded*)u;
  if (r.step()) return 1;
  bn254::Fr v;
  memcpy(v.l, s, 32);
  r.hash->common_scalar(v);
  r.commons++;
  return 0;
}
static int cb_read_point(void* u, uint64_t* out) {
  Recorded& r = *(Recorded*)u;
  if (r.step()) return 2;
  if (r.next >= r.plan->elems.size() || !r.plan->elems[r.next].is_point) return 3;  // out of order: a failure of the walk
  const bn254::G1Affine& p = r.pts[r.plan->elems[r.next++].index];
  r.hash->common_point(p);
  memcpy(out, &p, 64);
  r.reads++;
  return 0;
}
static int cb_read_scalar(void* u, uint64_t* out) {
  Recorded& r = *(Recorded*)u;
  if (r.step()) return 2;
  if (r.next >= r.plan->elems.size() || r.plan->elems[r.next].is_point) return 3;
  const bn254::Fr& s = r.scs[r.plan->elems[r.next++].index];
  r.hash->common_scalar(s);
  memcpy(out, s.l, 32);
  r.reads++;
  return 0;
}
static int cb_squeeze(void* u, uint64_t* out) {
  Recorded& r = *(Recorded*)u;
  const bool big = r.calls == r.big_at;
  if (r.step()) return 4;
  const bn254::Fr c = r.hash->squeeze_challenge();
  memcpy(out, c.l, 32);
  if (big)
    for (int i = 0; i < 4; i++) out[i] = ~(uint64_t)0;  // far above r
  r.squeezes++;
  return 0;
}

#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      fprintf(stderr, "FAILED: " __VA_ARGS__); \
      fprintf(stderr, "\n");                  \
      return 1;                               \
    }                                         \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: verifier_read_check <key file> <case file>\n"), 2;
  const std::vector<uint8_t> key = slurp(argv[1]), cs = slurp(argv[2]);
  pkblob::Desc desc;
  pkblob::Layout lay;
  std::string err;
  if (pkblob::parse(key.data(), key.size(), &desc, &lay, &err) != AMDZK_OK) return fprintf(stderr, "%s\n", err.c_str()), 2;
  bn254::Fr repr, omega, rho;
  memcpy(repr.l, key.data() + lay.transcript_repr, 32);
  Cursor c(cs);
  const uint32_t N = c.u32(), kind = c.u32();
  c.get(omega.l, 32);
  c.get(rho.l, 32);
  verifier::Plan plan;
  if (verifier::make_plan(desc, N, (int)kind, &plan, &err) != AMDZK_OK) return fprintf(stderr, "%s\n", err.c_str()), 2;
  std::vector<std::vector<uint64_t>> cols((size_t)N * desc.num_instance);
  std::vector<std::vector<const uint64_t*>> col_ptrs(N);
  std::vector<std::vector<size_t>> col_lens(N);
  for (uint32_t ci = 0; ci < N; ci++)
    for (uint32_t i = 0; i < desc.num_instance; i++) {
      const uint32_t len = c.u32();
      if (!c.ok || len > (cs.size() - c.pos) / 32) return fprintf(stderr, "truncated case file (instances)\n"), 2;
      auto& v = cols[(size_t)ci * desc.num_instance + i];
      v.resize(4 * (size_t)len + 4);
      c.get(v.data(), 32 * (size_t)len);
      col_lens[ci].push_back(len);
    }
  for (uint32_t ci = 0; ci < N; ci++)
    for (uint32_t i = 0; i < desc.num_instance; i++) col_ptrs[ci].push_back(cols[(size_t)ci * desc.num_instance + i].data());
  std::vector<const uint64_t* const*> inst(N);
  std::vector<const size_t*> lens(N);
  for (uint32_t ci = 0; ci < N; ci++) inst[ci] = col_ptrs[ci].data(), lens[ci] = col_lens[ci].data();
  const uint32_t np = c.u32();
  if (!c.ok || np != plan.NP) return fprintf(stderr, "case file has %u points, the plan %u\n", np, plan.NP), 2;
  std::vector<bn254::G1Affine> pts(np);
  c.get(pts.data(), (size_t)np * sizeof(bn254::G1Affine));
  const uint32_t ns = c.u32();
  if (!c.ok || ns != plan.NS) return fprintf(stderr, "case file has %u scalars, the plan %u\n", ns, plan.NS), 2;
  std::vector<bn254::Fr> scs(ns);
  c.get(scs.data(), (size_t)ns * sizeof(bn254::Fr));
  if (!c.ok || c.pos != cs.size()) return fprintf(stderr, "case file: truncated or trailing bytes\n"), 2;

  // ---- the built-in route
  std::vector<bn254::Fr> L0(plan.n_bases), R0(plan.n_bases), L1(plan.n_bases), R1(plan.n_bases);
  verifier::fold_proof(plan, repr, omega, inst.data(), lens.data(), pts.data(), scs.data(), rho, L0.data(), R0.data());

  // ---- the callback route over the recorded elements
  std::vector<uint32_t> raw_off;
  const size_t raw_size = verifier::raw_offsets(plan, &raw_off);
  CHECK(raw_size == (size_t)plan.NP * 64 + (size_t)plan.NS * 32 && raw_off.size() == plan.elems.size(), "raw layout");
  std::vector<uint8_t> raw(raw_size, 0xee);
  amdzk_transcript_read t;
  t.common_point = cb_common_point, t.common_scalar = cb_common_scalar, t.read_point = cb_read_point, t.read_scalar = cb_read_scalar;
  t.squeeze_challenge = cb_squeeze;
  size_t total_calls = 0, total_reads = 0;
  std::vector<uint8_t> call_kind;  // per call of the honest walk: 0 common, 1 read, 2 squeeze
  {
    zkhost::Blake2bWrite hb;
    zkhost::Keccak256Write hk;
    Recorded rec{&plan, pts.data(), scs.data(), plan.evm ? (zkhost::TranscriptWrite*)&hk : (zkhost::TranscriptWrite*)&hb};
    t.user = &rec;
    verifier::CallbackSource src(&t, raw.data(), raw_off.data());
    CHECK(src.usable(), "usable");
    verifier::Challenges ch;
    CHECK(verifier::run_transcript(plan, src, repr, inst.data(), lens.data(), &ch), "the honest walk failed");
    CHECK(rec.next == plan.elems.size() && src.reads == plan.elems.size() && rec.reads == src.reads, "not every element was read once");
    // what the device would decode: the raw image back into points and scalars
    std::vector<bn254::G1Affine> p2(np);
    std::vector<bn254::Fr> s2(ns);
    for (size_t e = 0; e < plan.elems.size(); e++) {
      const verifier::Plan::Elem& el = plan.elems[e];
      if (el.is_point) memcpy((void*)&p2[el.index], raw.data() + raw_off[e], 64);
      else memcpy(s2[el.index].l, raw.data() + raw_off[e], 32);
    }
    CHECK(memcmp((const void*)p2.data(), (const void*)pts.data(), (size_t)np * 64) == 0 && memcmp(s2.data(), scs.data(), (size_t)ns * 32) == 0, "raw image");
    verifier::fold_challenges(plan, omega, inst.data(), lens.data(), s2.data(), rho, ch, L1.data(), R1.data());
    CHECK(memcmp(L0.data(), L1.data(), plan.n_bases * 32) == 0 && memcmp(R0.data(), R1.data(), plan.n_bases * 32) == 0,
          "the callback route's scalars differ from the built-in route's");
    total_calls = rec.calls, total_reads = rec.reads;
    printf("plan %u %u %zu %u\n", plan.NP, plan.NS, plan.proof_bytes, plan.n_bases);
    for (uint32_t i = 0; i < plan.n_bases; i++) {
      if (L1[i].is_zero() && R1[i].is_zero()) continue;
      printf("%u ", i);
      print_fr(L1[i]);
      printf(" ");
      print_fr(R1[i]);
      printf("\n");
    }
    printf("calls %zu %zu %zu\n", rec.commons, rec.reads, rec.squeezes);
    CHECK(rec.commons + rec.reads + rec.squeezes == rec.calls, "call count");
  }
  // ---- every failure point: call i returns non-zero; a squeeze hands back a value >= r
  size_t tried = 0;
  for (int mode = 0; mode < 2; mode++)
    for (size_t i = 0; i < total_calls; i++) {
      zkhost::Blake2bWrite hb;
      zkhost::Keccak256Write hk;
      Recorded rec{&plan, pts.data(), scs.data(), plan.evm ? (zkhost::TranscriptWrite*)&hk : (zkhost::TranscriptWrite*)&hb};
      if (mode == 0) rec.fail_at = i;
      else rec.big_at = i;
      t.user = &rec;
      verifier::CallbackSource src(&t, raw.data(), raw_off.data());
      verifier::Challenges ch;
      const bool ok = verifier::run_transcript(plan, src, repr, inst.data(), lens.data(), &ch);
      if (mode == 1 && ok) {  // call i was no squeeze: nothing was injected
        CHECK(rec.calls == total_calls, "an untouched walk must finish");
        continue;
      }
      CHECK(!ok, "call %zu failed and the walk went on", i);
      CHECK(rec.calls == i + 1, "a member was called after call %zu failed (%zu calls)", i, rec.calls);
      CHECK(src.reads == rec.reads && src.reads <= total_reads, "reads after a failure at call %zu: %u, the caller counted %zu", i,
            src.reads, rec.reads);
      tried++;
    }
  CHECK(tried > total_calls, "no challenge was ever replaced");
  // ---- a NULL member: unusable, nothing may be called
  for (int m = 0; m < 5; m++) {
    amdzk_transcript_read n = t;
    if (m == 0) n.common_point = nullptr;
    if (m == 1) n.common_scalar = nullptr;
    if (m == 2) n.read_point = nullptr;
    if (m == 3) n.read_scalar = nullptr;
    if (m == 4) n.squeeze_challenge = nullptr;
    verifier::CallbackSource src(&n, raw.data(), raw_off.data());
    CHECK(!src.usable(), "a NULL member %d passed for usable", m);
  }
  verifier::CallbackSource none(nullptr, raw.data(), raw_off.data());
  CHECK(!none.usable(), "a NULL transcript passed for usable");
  printf("failures %zu\n", tried);
  printf("ok\n");
  return 0;
}
