// Single-core time of pos::sponge (csrc/poseidon.hpp: this library's own 8 x 32-bit host field code, NOT the Rust crate) for
// the shapes of tools/bench_poseidon.py, which builds and runs this. Constants are arbitrary values below r: the time does
// not depend on them.
//   poseidon_host_time <t> <rate> <r_f> <r_p> <len> <sponges per sample>     ->  "<microseconds per sponge, median of 7 samples>"
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../anon-aadhaar-halo2_amd/csrc/poseidon.hpp"

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const uint32_t t = atoi(argv[1]), rate = atoi(argv[2]), r_f = atoi(argv[3]), r_p = atoi(argv[4]);
  const size_t len = atol(argv[5]), per = atol(argv[6]);
  uint64_t x = 0x9E3779B97F4A7C15ull;
  auto fill = [&](std::vector<uint64_t>& v) {
    for (size_t i = 0; i < v.size(); i++) {
      x = x * 6364136223846793005ull + 1442695040888963407ull;
      v[i] = (i & 3) == 3 ? x >> 4 : x;  // top word below 2^60: the value is below r
    }
  };
  std::vector<uint64_t> rc((size_t)(r_f + r_p) * t * 4), mds((size_t)t * t * 4), in(len * 4);
  fill(rc);
  fill(mds);
  fill(in);
  amdzk_poseidon_desc d = {sizeof(amdzk_poseidon_desc), t, rate, r_f, r_p, rc.data(), mds.data(), nullptr};
  pos::Spec sp;
  std::string err;
  if (pos::check(&d, sp, err) != AMDZK_OK) {
    fprintf(stderr, "%s\n", err.c_str());
    return 1;
  }
  std::vector<bn254::Fr> inputs(len);
  for (size_t i = 0; i < len; i++) inputs[i] = pos::load_fr(in.data(), i);
  std::vector<double> us;
  uint32_t sink = 0;
  for (int s = 0; s < 8; s++) {  // the first sample warms up
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t i = 0; i < per; i++) {
      if (len) inputs[0].l[0] ^= (uint32_t)i & 1;
      sink ^= pos::sponge(sp, inputs.data(), len).l[0];
    }
    const double dt = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (s) us.push_back(dt / per);
  }
  std::sort(us.begin(), us.end());
  printf("%.3f %u\n", us[us.size() / 2], sink & 1);
  return 0;
}
