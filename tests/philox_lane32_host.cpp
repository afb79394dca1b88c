// Host check of ebm_common.h's PhiloxLane32 (the lean Langevin loop's 32-bit-counter Philox) against philox4x32_10, the
// 64-bit definition: random (group, step, key) triples plus the edge words of both counters.  Built and run by
// tests/test_philox_lane32.py; prints "ok <n>" or the first mismatch and exits non-zero.
#include <cstdio>
#include <cstdlib>

#include "../torchebm_amd/csrc/ebm_common.h"

using ebm::PhiloxLane32;
using ebm::RngKey;
using ebm::U4;

static uint64_t splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static bool same(uint32_t group, uint32_t step, RngKey key) {
  const U4 a = PhiloxLane32(group, key).at(step);
  const U4 b = ebm::philox4x32_10(group, 0, step, 0, key.k0, key.k1);
  if (a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w) return true;
  printf("mismatch group %u step %u key %08x %08x: %08x %08x %08x %08x != %08x %08x %08x %08x\n", group, step, key.k0, key.k1,
         a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w);
  return false;
}

int main(int argc, char** argv) {
  const long n_random = argc > 1 ? atol(argv[1]) : 1000000;
  uint64_t s = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
  long n = 0;
  // Random123 known answer with zero counter high words: counter 0, key 0
  const U4 kat = PhiloxLane32(0, RngKey{0, 0}).at(0);
  if (!(kat.x == 0x6627E8D5u && kat.y == 0xE169C58Du && kat.z == 0xBC57AC4Cu && kat.w == 0x9B00DBD8u)) {
    printf("known answer: %08x %08x %08x %08x\n", kat.x, kat.y, kat.z, kat.w);
    return 1;
  }
  ++n;
  const uint32_t edges[] = {0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
  for (uint32_t g : edges)
    for (uint32_t t : edges)
      for (int r = 0; r < 4; ++r) {
        const uint64_t k = r == 0 ? 0 : (r == 1 ? ~0ull : splitmix64(s));
        if (!same(g, t, RngKey{(uint32_t)k, (uint32_t)(k >> 32)})) return 1;
        ++n;
      }
  for (long i = 0; i < n_random; ++i) {
    const uint64_t gs = splitmix64(s), k = splitmix64(s);
    if (!same((uint32_t)gs, (uint32_t)(gs >> 32), RngKey{(uint32_t)k, (uint32_t)(k >> 32)})) return 1;
    ++n;
  }
  printf("ok %ld\n", n);
  return 0;
}
