// Stand-alone driver of csrc/workspace.hpp and of the byte layouts built on it (verifier::mixed_layout, pairing::image_layout
// and pairing::call_layout): prints offsets for tests/test_workspace_layout.py, which holds the formulas they must match.
// Plain g++, no HIP. Commands on stdin, one per line:
//   take <pad> <bytes> ...                                one WsLayout: "<offset> <bytes() after it>" per take; a token p<k> switches to pad k
//   round <a> <v> ...                                     ws_round_up(v, a) per v
//   verify <n> <stride> <E> <NP> <NS> <nvk> <tr> <pp>      a verify call of ONE group, n proofs of <stride> bytes in either form (tr: all
//                                                         through a read transcript): every field of verifier::MixedLayout, in
//                                                         declaration order, the per-item and per-group vectors last
//   consts                                                what the pairing's layouts are functions of, read off the headers
//   image                                                 pairing::programs().at
//   call <n> <m>                                          pairing_chunk and every field of pairing::CallLayout
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../anon-aadhaar-halo2_amd/csrc/pairing.hpp"
#include "../../anon-aadhaar-halo2_amd/csrc/verifier.hpp"
#include "../../anon-aadhaar-halo2_amd/csrc/workspace.hpp"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, tok;
    in >> cmd;
    if (cmd == "take") {
      WsLayout w;
      size_t pad = 256;
      in >> pad;
      while (in >> tok) {
        if (tok[0] == 'p') {
          pad = std::stoull(tok.substr(1));
          continue;
        }
        const size_t at = w.take(std::stoull(tok), pad);
        printf("%zu %zu ", at, w.bytes());
      }
      printf("\n");
    } else if (cmd == "round") {
      size_t a = 1, v;
      in >> a;
      while (in >> v) printf("%zu ", ws_round_up(v, a));
      printf("\n");
    } else if (cmd == "verify") {
      size_t n, stride, E, NP, NS, nvk;
      int tr, pp;
      in >> n >> stride >> E >> NP >> NS >> nvk >> tr >> pp;
      const verifier::MixedGroupShape shape = {E, NP, NS, nvk, stride, stride};
      const std::vector<uint32_t> group(n, 0);
      const std::vector<uint8_t> raw(n, 1);
      const verifier::MixedLayout L = verifier::mixed_layout(&shape, 1, group.data(), tr ? raw.data() : nullptr, n, 1, pp != 0);
      printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu ", L.staging, L.items, L.groups, L.blocks, L.elems, L.elems_raw, L.status, L.key_g, L.vk,
             L.g, L.points, L.scalars, L.msm, L.run_bases);
      printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", L.bytes, L.up_bytes, L.down_bytes, L.n_blocks, L.n_elems, L.n_points, L.n_scalars, L.nvk,
             L.staging_bytes, L.run, L.run_len);
      for (const std::vector<size_t>* v : {&L.item_staging, &L.item_stride, &L.item_points, &L.item_scalars, &L.group_elems, &L.group_vk})
        for (size_t x : *v) printf(" %zu", x);
      printf("\n");
    } else if (cmd == "consts") {
      const pairing::Programs& P = pairing::programs();
      printf("%zu %d %d %zu %zu %zu %d %u %zu %d\n", (size_t)pairing::PAIRING_CHUNK_LANES, pairing::K_COUNT, bn254::PAIRING_NUM_LINES, P.miller.w.size(),
             P.mul.w.size(), P.fin.w.size(), P.miller.regs, P.final_regs, sizeof(bn254::Fq2x), AMDZK_PAIRING_MAX_M);
      printf("%d %d\n", P.mul.regs, P.fin.regs);
    } else if (cmd == "image") {
      const pairing::ImageLayout& L = pairing::programs().at;
      printf("%zu %zu %zu %zu %zu\n", L.lines, L.miller, L.mul, L.fin, L.bytes);
    } else if (cmd == "call") {
      size_t n, m;
      in >> n >> m;
      const pairing::Programs& P = pairing::programs();
      const size_t chunk = pairing::pairing_chunk(n, m);
      const pairing::CallLayout L = pairing::call_layout(n, m, chunk, P.miller.regs, P.final_regs);
      printf("%zu %zu %zu %zu %zu %zu %zu\n", chunk, L.g1, L.miller_slab, L.final_slab, L.gt, L.is_one, L.bytes);
    } else if (!cmd.empty()) {
      fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  printf("ok\n");
  return 0;
}
