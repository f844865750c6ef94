// The multiopen argument's host arithmetic (csrc/opening.hpp) alone: reads cases, prints the grouping and every scalar of
// SHPLONK's two halves. tests/test_opening_host.py compares them, as field elements, with the protocol oracle; it also builds
// this file with -fsanitize=address,undefined. Plain g++, no HIP.
//   opening_check <case file>
// case file, text, one case after another: "<n_coms> <n_pts> <n_queries>", then per query "<com> <pt>", then the n_pts point
// values, then one claimed evaluation per query, then y, v, u — field elements canonical, 64 hex digits.
// Output per case: "case", the grouping in decimal ("coms", "com <c> | pts | first queries", "set <i> | pts | coms", "gw <pt> |
// queries", "shape <set_points> <maxm>"), then per set "order", "pts", "c", "E", "low", "w" (the Lagrange weights at u) and "z",
// per division row "row <set> <root> <v^i c_it> <padded R_i>", then "zt", "z0", "z0_zero", "cf", "cterm". "ok" at the end.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../anon-aadhaar-halo2_amd/csrc/opening.hpp"

using bn254::Fr;

static bool read_fr(FILE* f, Fr* out) {
  char hex[80];
  if (fscanf(f, "%79s", hex) != 1 || strlen(hex) != 64) return false;
  Fr a = Fr::zero();
  for (int i = 0; i < 64; i++) {
    const char ch = hex[i];
    const int d = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1;
    if (d < 0) return false;
    a.l[7 - i / 8] |= (uint32_t)d << (28 - 4 * (i % 8));
  }
  *out = bn254::to_mont(a);
  return true;
}
static void put(const Fr& a) {
  const Fr c = bn254::from_mont(a);
  printf(" ");
  for (int i = 7; i >= 0; i--) printf("%08x", c.l[i]);
}
static void line(const char* label, size_t i, const std::vector<Fr>& v) {
  printf("%s %zu", label, i);
  for (const Fr& a : v) put(a);
  printf("\n");
}
static void ints(const std::vector<uint32_t>& v) {
  printf(" |");
  for (uint32_t a : v) printf(" %u", a);
}

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: opening_check <case file>\n"), 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return fprintf(stderr, "cannot read %s\n", argv[1]), 2;
  size_t n_coms, n_pts, nq;
  while (fscanf(f, "%zu %zu %zu", &n_coms, &n_pts, &nq) == 3) {
    if (n_coms > (1u << 20) || n_pts > (1u << 20) || nq > (1u << 20)) return fprintf(stderr, "case too large\n"), 2;
    std::vector<opening::Query> q(nq);
    for (auto& e : q)
      if (fscanf(f, "%u %u", &e.com, &e.pt) != 2 || e.com >= n_coms || e.pt >= n_pts) return fprintf(stderr, "bad query\n"), 2;
    std::vector<Fr> pt(n_pts), ev(nq);
    Fr y, v, u;
    bool ok = true;
    for (Fr& a : pt) ok = ok && read_fr(f, &a);
    for (Fr& a : ev) ok = ok && read_fr(f, &a);
    if (!ok || !read_fr(f, &y) || !read_fr(f, &v) || !read_fr(f, &u)) return fprintf(stderr, "bad field element\n"), 2;
    const opening::Grouping g = opening::group(q.data(), nq, n_coms, n_pts);
    printf("case\ncoms"), ints(g.coms), printf("\n");
    for (size_t c = 0; c < g.coms.size(); c++) printf("com %zu", c), ints(g.com_pts[c]), ints(g.com_q[c]), printf("\n");
    for (size_t i = 0; i < g.sets.size(); i++) printf("set %zu", i), ints(g.sets[i].pts), ints(g.sets[i].coms), printf("\n");
    for (size_t i = 0; i < g.gw.size(); i++) printf("gw %zu", i), ints(g.gw[i]), printf("\n");
    printf("shape %zu %zu\n", g.set_points, g.maxm);
    const opening::Shplonk sh = opening::shplonk_sets(g, pt.data(), [&](uint32_t i) { return ev[i]; }, y, v);
    const opening::AtU at = opening::at_u(g, pt.data(), u);
    for (size_t i = 0; i < g.sets.size(); i++) {
      printf("order %zu", i), ints(sh.order[i]), printf("\n");
      line("pts", i, sh.pts[i]), line("c", i, sh.c[i]), line("E", i, sh.E[i]), line("low", i, sh.low[i]);
      line("w", i, opening::weights_at(sh, i, u)), line("z", i, {at.z[i]});
    }
    for (size_t r = 0; r < sh.root.size(); r++) {
      std::vector<Fr> row = {sh.root[r], sh.coef[r]};
      row.insert(row.end(), sh.row_low.begin() + r * g.maxm, sh.row_low.begin() + (r + 1) * g.maxm);
      line("row", sh.row_set[r], row);
    }
    const opening::Final fin = opening::shplonk_final(g, sh, pt.data(), v, u);
    line("zt", 0, {at.zt}), line("z0", 0, {at.z0});
    printf("z0_zero %d\n", (int)fin.z0_zero);
    line("cf", 0, fin.cf), line("cterm", 0, {fin.cterm});
  }
  const bool all = feof(f);
  fclose(f);
  if (!all) return fprintf(stderr, "trailing text in the case file\n"), 2;
  printf("ok\n");
  return 0;
}
