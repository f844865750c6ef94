// Driver for tests/test_check_witness_cpp_mirror.py: ProvingKey::check_witness of include/amdzk_halo2.hpp.
//   check_witness_mirror <k> <witness file> <tau hex>
// The circuit is tests/circuits.py lookup_circuit, configured here in C++; the witness file is the one
// tests/test_cpp_mirror.py writes (F / A cells, I instance columns, C copies) with further lines "B <col> <row> <hex>":
// advice cells of a second, corrupted witness. Prints "good <failures>" for the first witness and one line
// "failure <kind> <index> <first_row> <count>" per entry of the second one's report.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "amdzk_halo2.hpp"

using namespace amdzk::halo2;
using Exprs = std::vector<Expression>;
using Pairs = std::vector<std::pair<Expression, Expression>>;

static void configure_lookup(ConstraintSystem& cs) {
  Column a = cs.advice_column(), b = cs.advice_column(), c = cs.advice_column();
  Column q_mul = cs.selector(), q_add = cs.selector(), q_rng = cs.selector(), q_pair = cs.selector();
  Column t_rng = cs.fixed_column(), t_x = cs.fixed_column(), t_y = cs.fixed_column(), konst = cs.fixed_column();
  Column inst = cs.instance_column();
  for (Column col : {a, b, c, konst, inst}) cs.enable_equality(col);
  cs.create_gate("mul/add", [&](VirtualCells& m) {  // one query per statement: the order of first use numbers the queries
    Expression s0 = m.query_selector(q_mul);
    Expression a0 = m.query_advice(a, Rotation::cur());
    Expression b0 = m.query_advice(b, Rotation::cur());
    Expression c0 = m.query_advice(c, Rotation::cur());
    Expression s1 = m.query_selector(q_add);
    Expression a1 = m.query_advice(a, Rotation::cur());
    Expression b1 = m.query_advice(b, Rotation::next());
    Expression c1 = m.query_advice(c, Rotation::cur());
    return Exprs{s0 * (a0 * b0 - c0), s1 * (a1 + b1 - c1)};
  });
  cs.lookup("range", [&](VirtualCells& m) {
    Expression s = m.query_selector(q_rng);
    Expression v = m.query_advice(a, Rotation::cur());
    Expression t = m.query_fixed(t_rng);
    return Pairs{{s * v, t}};
  });
  cs.lookup("pair", [&](VirtualCells& m) {
    Expression s0 = m.query_selector(q_pair);
    Expression v0 = m.query_advice(b, Rotation::cur());
    Expression t0 = m.query_fixed(t_x);
    Expression s1 = m.query_selector(q_pair);
    Expression v1 = m.query_advice(c, Rotation::cur());
    Expression t1 = m.query_fixed(t_y);
    return Pairs{{s0 * v0, t0}, {s1 * v1, t1}};
  });
}

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s <k> <witness file> <tau hex>\n", argv[0]);
    return 2;
  }
  try {
    const uint32_t k = (uint32_t)std::atoi(argv[1]);
    const size_t n = (size_t)1 << k;
    ConstraintSystem cs;
    configure_lookup(cs);
    std::vector<std::vector<Fr>> fixed(cs.num_fixed, std::vector<Fr>(n, Fr::zero())), instances(cs.num_instance);
    std::vector<Fr> good(cs.num_advice * n, Fr::zero());
    struct Cell {
      size_t col, row;
      Fr v;
    };
    std::vector<Cell> bad_cells;
    Assembly assembly(n, cs.permutation_columns.size());
    std::ifstream f(argv[2]);
    if (!f) throw Error(AMDZK_E_INVALID, "cannot open witness file");
    std::string line;
    while (std::getline(f, line)) {
      std::istringstream is(line);
      char tag;
      is >> tag;
      if (tag == 'F' || tag == 'A' || tag == 'B') {
        size_t col, row;
        std::string hex;
        is >> col >> row >> hex;
        if (row >= n || col >= (tag == 'F' ? cs.num_fixed : cs.num_advice)) throw Error(AMDZK_E_INVALID, "witness file: cell out of range");
        if (tag == 'F') fixed[col][row] = Fr::from_hex(hex);
        else if (tag == 'A') good[col * n + row] = Fr::from_hex(hex);
        else bad_cells.push_back({col, row, Fr::from_hex(hex)});
      } else if (tag == 'I') {
        size_t col;
        std::string hex;
        is >> col;
        while (is >> hex) instances.at(col).push_back(Fr::from_hex(hex));
      } else if (tag == 'C') {
        size_t c1, r1, c2, r2;
        is >> c1 >> r1 >> c2 >> r2;
        assembly.copy(c1, r1, c2, r2);
      }
    }
    Context ctx(0);
    ParamsKZG params = ParamsKZG::setup(ctx, k, Fr::from_hex(argv[3]));
    ProvingKey pk(ctx, params, cs, fixed, assembly, Fr::from_u64(77));
    void* d = nullptr;
    ctx.check(amdzk_dev_alloc(ctx.get(), good.size() * sizeof(Fr), &d));
    ctx.check(amdzk_dev_upload(ctx.get(), d, good.data(), good.size() * sizeof(Fr)));
    const WitnessReport ok = pk.check_witness(instances, d, n);
    std::printf("good %zu %d\n", ok.failures.size(), ok.ok() ? 1 : 0);
    std::vector<Fr> bad = good;
    for (const Cell& c : bad_cells) bad[c.col * n + c.row] = c.v;
    ctx.check(amdzk_dev_upload(ctx.get(), d, bad.data(), bad.size() * sizeof(Fr)));
    const WitnessReport rep = pk.check_witness(instances, d, n, 5);
    std::printf("bad %zu %d\n", rep.failures.size(), rep.ok() ? 1 : 0);
    for (const CheckFailure& e : rep.failures)
      std::printf("failure %u %u %u %llu\n", (unsigned)e.kind, e.index, e.first_row, (unsigned long long)e.count);
    amdzk_dev_free(ctx.get(), d);
    return 0;
  } catch (const Error& e) {
    std::fprintf(stderr, "error %d: %s\n", e.code, e.what());
    return 1;
  }
}
