// The host half of amdzk_verify_proofs (csrc/verifier.hpp) alone, without a device: reads a proving-key file (pkblob::parse)
// and one proof's decoded elements, prints the table of (base, L scalar, R scalar) that the library would hand to its MSM.
// tests/test_verifier_host.py folds the table with the oracle's G1 arithmetic and compares the pair with the reference's;
// it also builds this file with -fsanitize=address,undefined. Plain g++, no HIP.
//   verifier_check <key file> <case file>
// case file, little-endian: N u32 | transcript_kind u32 | omega, rho 4 x u64 (Montgomery) | per circuit and instance column:
// len u32, values 4 x u64 | NP u32, points 8 x u64 | NS u32, scalars 4 x u64.
// Output: "plan <NP> <NS> <proof bytes> <bases>", then one line "<base> <L> <R>" per base with a non-zero scalar (canonical,
// hex), then "ok". Exit status 2 with a message on a malformed input.
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

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: verifier_check <key file> <case file>\n"), 2;
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
      v.resize(4 * (size_t)len + 4);  // never empty: data() is a valid address
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
  uint32_t bad_col = 0;
  if (desc.num_instance && !verifier::instances_ok(plan, inst.data(), lens.data(), &bad_col)) return fprintf(stderr, "bad instance column %u\n", bad_col), 2;
  std::vector<bn254::Fr> L(plan.n_bases), Rr(plan.n_bases);
  verifier::fold_proof(plan, repr, omega, inst.data(), lens.data(), pts.data(), scs.data(), rho, L.data(), Rr.data());
  printf("plan %u %u %zu %u\n", plan.NP, plan.NS, plan.proof_bytes, plan.n_bases);
  for (uint32_t i = 0; i < plan.n_bases; i++) {
    if (L[i].is_zero() && Rr[i].is_zero()) continue;
    printf("%u ", i);
    print_fr(L[i]);
    printf(" ");
    print_fr(Rr[i]);
    printf("\n");
  }
  printf("ok\n");
  return 0;
}
