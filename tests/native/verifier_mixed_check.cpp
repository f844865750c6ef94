// The two pure host functions behind amdzk_verify_proofs_mixed (csrc/verifier.hpp): group_items and mixed_layout, alone, in a
// plain g++ program (tests/test_verifier_mixed_host.py builds it plainly and with ASan + UBSan and restates both in Python).
// stdin, whitespace separated:
//   groups <n>  then n x (key n_circuits kind)                         -> "of ..." and "firsts ..."
//   layout <n_groups> <n_items> <n_keys> <per_proof>  then n_groups x (E NP NS nvk proof_bytes raw_bytes), n_items x (group raw)
//                                                                      -> the regions, the totals and the per-group / per-item tables
#include <stdio.h>

#include <iostream>
#include <string>
#include <vector>

#include "../../anon-aadhaar-halo2_amd/csrc/verifier.hpp"

static void row(const char* name, const std::vector<size_t>& v) {
  std::string out(name);
  for (size_t x : v) out += " " + std::to_string(x);
  puts(out.c_str());
}

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "groups") {
      size_t n;
      std::cin >> n;
      std::vector<verifier::MixedKey> keys(n);
      for (auto& k : keys) {
        size_t key;
        std::cin >> key >> k.n_circuits >> k.kind;
        k.key = (const void*)key;
      }
      std::vector<size_t> firsts;
      const std::vector<uint32_t> of = verifier::group_items(keys.data(), n, &firsts);
      row("of", std::vector<size_t>(of.begin(), of.end()));
      row("firsts", firsts);
    } else if (cmd == "layout") {
      size_t G, n, n_keys, per_proof;
      std::cin >> G >> n >> n_keys >> per_proof;
      std::vector<verifier::MixedGroupShape> shapes(G);
      for (auto& s : shapes) std::cin >> s.E >> s.NP >> s.NS >> s.nvk >> s.proof_bytes >> s.raw_bytes;
      std::vector<uint32_t> group(n);
      std::vector<uint8_t> raw(n);
      bool any_raw = false;
      for (size_t b = 0; b < n; b++) {
        unsigned r;
        std::cin >> group[b] >> r;
        raw[b] = (uint8_t)r, any_raw |= r != 0;
        if (group[b] >= G) return fprintf(stderr, "item %zu names group %u of %zu\n", b, group[b], G), 2;
      }
      if (!std::cin) return fprintf(stderr, "short input\n"), 2;
      const verifier::MixedLayout L = verifier::mixed_layout(shapes.data(), G, group.data(), any_raw ? raw.data() : nullptr, n, n_keys, per_proof != 0);
      row("regions", {L.staging, L.items, L.groups, L.blocks, L.elems, L.elems_raw, L.status, L.key_g, L.vk, L.g, L.points, L.scalars, L.msm, L.run_bases});
      row("totals", {L.bytes, L.up_bytes, L.down_bytes, L.n_blocks, L.n_elems, L.n_points, L.n_scalars, L.nvk, L.staging_bytes, L.run, L.run_len});
      row("group_elems", L.group_elems);
      row("group_vk", L.group_vk);
      row("item_staging", L.item_staging);
      row("item_stride", L.item_stride);
      row("item_points", L.item_points);
      row("item_scalars", L.item_scalars);
    } else {
      return fprintf(stderr, "unknown command %s\n", cmd.c_str()), 2;
    }
  }
  puts("ok");
  return 0;
}
