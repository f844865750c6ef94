// The header-only Poseidon of include/amdzk_halo2.hpp against the ctypes route (tests/test_poseidon_cpp_mirror.py).
//   poseidon_mirror_check <file>       (no argument: usage, exit 2 — the CPU test only builds this)
// file: the layout of tests/native/poseidon_check.cpp. Output: "check ok" (PoseidonSpec::check, no device), per state one
// line "state" + t x 4 words (permute_dev), per sponge one line "digest" + 4 words (hash_many), one line "squeeze" + 4 words
// (update in two pieces + squeeze of the first sponge), one line "dev" + 4 words per sponge (hash_many_dev, ragged), "ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "amdzk_halo2.hpp"

using namespace amdzk::halo2;

static void print(const char* tag, const Fr* v, size_t n) {
  printf("%s", tag);
  for (size_t i = 0; i < n; i++) printf(" %016llx %016llx %016llx %016llx", (unsigned long long)v[i].l[0], (unsigned long long)v[i].l[1],
                                        (unsigned long long)v[i].l[2], (unsigned long long)v[i].l[3]);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: poseidon_mirror_check <file>\n");
    return 2;
  }
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
  if (h[0] > 64 || h[2] > 4096 || h[3] > 4096) return 2;
  PoseidonSpec spec;
  spec.t = h[0];
  spec.rate = h[1];
  spec.r_f = h[2];
  spec.r_p = h[3];
  spec.round_constants.resize((size_t)(h[2] + h[3]) * h[0]);
  spec.mds.resize((size_t)h[0] * h[0]);
  take(spec.round_constants.data(), spec.round_constants.size() * 32);
  take(spec.mds.data(), spec.mds.size() * 32);
  if (h[4]) {
    spec.initial_state.resize(h[0]);
    take(spec.initial_state.data(), (size_t)h[0] * 32);
  }
  std::vector<Fr> states((size_t)h[5] * h[0]);
  take(states.data(), states.size() * 32);
  std::vector<std::vector<Fr>> sponges(h[6]);
  for (auto& s : sponges) {
    uint32_t len[2];
    take(len, sizeof(len));
    s.resize(len[0]);
    take(s.data(), (size_t)len[0] * 32);
  }
  if (off != buf.size()) return 3;
  try {
    spec.check();
    printf("check ok\n");
    Context ctx(0);
    Poseidon pos(ctx, spec);
    size_t stride = 1;
    for (const auto& s : sponges) stride = s.size() > stride ? s.size() : stride;
    void* d = nullptr;
    ctx.check(amdzk_dev_alloc(ctx.get(), (states.size() + sponges.size() * (stride + 1) + 1) * 32, &d));
    if (!states.empty()) {
      ctx.check(amdzk_dev_upload(ctx.get(), d, states.data(), states.size() * 32));
      pos.permute_dev(d, h[5]);
      ctx.check(amdzk_dev_download(ctx.get(), states.data(), d, states.size() * 32));
      for (uint32_t b = 0; b < h[5]; b++) print("state", &states[(size_t)b * h[0]], h[0]);
    }
    if (!sponges.empty()) {
      const std::vector<Fr> digests = pos.hash_many(sponges);
      for (const Fr& v : digests) print("digest", &v, 1);
      const size_t cut = sponges[0].size() / 2;
      pos.update(std::vector<Fr>(sponges[0].begin(), sponges[0].begin() + cut));
      pos.update(std::vector<Fr>(sponges[0].begin() + cut, sponges[0].end()));
      const Fr sq = pos.squeeze();
      print("squeeze", &sq, 1);
      std::vector<size_t> lens;
      char* d_in = (char*)d;
      char* d_out = d_in + sponges.size() * stride * 32;
      for (size_t b = 0; b < sponges.size(); b++) {
        lens.push_back(sponges[b].size());
        if (!sponges[b].empty()) ctx.check(amdzk_dev_upload(ctx.get(), d_in + b * stride * 32, sponges[b].data(), sponges[b].size() * 32));
      }
      pos.hash_many_dev(d_in, stride, lens, 0, sponges.size(), d_out);
      std::vector<Fr> out(sponges.size());
      ctx.check(amdzk_dev_download(ctx.get(), out.data(), d_out, out.size() * 32));
      for (const Fr& v : out) print("dev", &v, 1);
    }
    ctx.check(amdzk_dev_free(ctx.get(), d));
  } catch (const Error& e) {
    printf("error %d %s\n", e.code, e.what());
    return 1;
  }
  printf("ok\n");
  return 0;
}
