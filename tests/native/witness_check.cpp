// Host check of csrc/witness.hpp (tests/test_witness_host.py): whole witness programs through wit::build and, node by
// node, wit::eval_node — the function the kernels of witness.hip call — on the host. Plain g++; no device, no library.
//   witness_check <file>
// file: u32 n_proofs, then the description as WitnessProgram.desc_bytes() lays it out (u32 k, num_advice, n_inputs,
// n_constants, n_nodes, n_cells, n_publics; constants 4 x u64 each; nodes 4 x u32; cells 3 x u32; publics u32), then
// n_proofs x n_inputs x 4 u64 of inputs. Output: "levels <n>", then per proof one line per node IN THE CALLER'S ORDER with
// the 4 Montgomery words of its value in hex, then "ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../anon-aadhaar-halo2_amd/csrc/witness.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> buf;
  uint8_t tmp[65536];
  size_t got;
  while ((got = fread(tmp, 1, sizeof(tmp), f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
  fclose(f);
  size_t off = 0;
  auto take = [&](void* dst, size_t n) {
    if (off + n > buf.size()) {
      fprintf(stderr, "short file\n");
      exit(2);
    }
    if (n) memcpy(dst, buf.data() + off, n);
    off += n;
  };
  uint32_t h[8];
  take(h, sizeof(h));
  const uint32_t n_proofs = h[0];
  std::vector<uint64_t> consts((size_t)h[4] * 4);
  std::vector<amdzk_wnode> nodes(h[5]);
  std::vector<amdzk_wcell> cells(h[6]);
  std::vector<uint32_t> publics(h[7]);
  take(consts.data(), consts.size() * 8);
  take(nodes.data(), nodes.size() * sizeof(amdzk_wnode));
  take(cells.data(), cells.size() * sizeof(amdzk_wcell));
  take(publics.data(), publics.size() * 4);
  amdzk_witness_desc d;
  memset(&d, 0, sizeof(d));
  d.size = sizeof(d);
  d.k = h[1];
  d.num_advice = h[2];
  d.n_inputs = h[3];
  d.n_constants = h[4];
  d.constants = consts.data();
  d.n_nodes = h[5];
  d.nodes = nodes.data();
  d.n_cells = h[6];
  d.cells = cells.data();
  d.n_publics = h[7];
  d.publics = publics.data();
  wit::Program p;
  std::string err;
  if (wit::build(&d, p, err) != AMDZK_OK) {
    printf("refused %s\n", err.c_str());
    return 1;
  }
  printf("levels %u\n", p.levels());
  std::vector<bn254::Fr> in(d.n_inputs), val(p.nodes.size());
  for (uint32_t b = 0; b < n_proofs; b++) {
    take(in.data(), (size_t)d.n_inputs * 32);
    wit::host_run(p, in.data(), val.data());
    for (uint32_t i = 0; i < d.n_nodes; i++) {
      const bn254::Fr& v = val[p.slot_of[i]];
      printf("%08x%08x %08x%08x %08x%08x %08x%08x\n", v.l[1], v.l[0], v.l[3], v.l[2], v.l[5], v.l[4], v.l[7], v.l[6]);
    }
  }
  if (off != buf.size()) return 3;
  printf("ok\n");
  return 0;
}
