// The header-only builder of witness programs (include/amdzk_halo2.hpp WitnessProgram) against the Python one
// (tests/test_witness_cpp_mirror.py): one program that uses every method, printed as the description's bytes in the
// layout of WitnessProgram.desc_bytes() — u32 k, num_advice, n_inputs, n_constants, n_nodes, n_cells, n_publics, then the
// constants, nodes, cells and publics as they lie in memory — in hex, then the plan for 3 proofs. No device is needed.
#include <cstdio>
#include <vector>

#include "amdzk_halo2.hpp"

using namespace amdzk::halo2;

static void hex(const void* p, size_t n) {
  for (size_t i = 0; i < n; i++) printf("%02x", ((const unsigned char*)p)[i]);
}

int main() {
  WitnessProgram w(6, 4);
  auto x = w.input(), y = w.input();
  auto c7 = w.constant(Fr::from_u64(7)), cm1 = w.constant(-Fr::one()), c7b = w.constant(Fr::from_u64(7));
  auto s = w.add(x, y), d = w.sub(s, c7), m = w.mul(d, cm1), n = w.neg(m), i = w.inv(n);
  auto z = w.is_zero(i), e = w.eq(c7, c7b), l = w.lt(x, y), sel = w.select(l, s, d);
  auto b = w.bits(sel, 31, 2), a = w.and_(x, cm1), xo = w.xor_(a, b);
  w.assign(s, 0, 0);
  w.assign(xo, 3, 63);
  w.assign(z, 1, 17);
  w.expose(e);
  w.expose(xo);
  const amdzk_witness_desc t = w.desc();
  const uint32_t head[7] = {t.k, t.num_advice, t.n_inputs, t.n_constants, t.n_nodes, t.n_cells, t.n_publics};
  hex(head, sizeof(head));
  hex(t.constants, (size_t)t.n_constants * 32);
  hex(t.nodes, (size_t)t.n_nodes * sizeof(amdzk_wnode));
  hex(t.cells, (size_t)t.n_cells * sizeof(amdzk_wcell));
  hex(t.publics, (size_t)t.n_publics * 4);
  const WitnessProgram::Plan p = w.plan(3);
  printf("\n%u %u %u %zu %zu\n", p.levels, p.launches, p.fused_width, p.scratch_bytes, t.size);
  return 0;
}
