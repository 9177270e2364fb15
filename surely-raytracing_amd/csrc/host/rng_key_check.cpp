// rng_key_check — host check of the split stream key (rt_rng.h): rng_key_mix(rng_key_pixel,
// rng_key_sample) and the incremental rng_key_next must give the state of rng_seed for every
// (seed, pixel, sample). Prints "rng_key_check ok: N triples" and exits 0, or the first mismatch
// and exits 1. Built by the Makefile (build/rng_key_check), run by tests/test_rng_key.py.
#include <cstdint>
#include <cstdio>

#include "../rt_rng.h"

namespace {
using rtd::Rng;
unsigned long long g_n = 0;

bool same(uint32_t lo, uint32_t hi, uint32_t pixel, uint32_t sample, Rng b) {
  const Rng a = rtd::rng_seed(lo, hi, pixel, sample);
  ++g_n;
  if (a.s0 == b.s0 && a.s1 == b.s1 && (a.s0 | a.s1) != 0u) return true;
  std::printf("mismatch: seed %08x:%08x pixel %u sample %u: rng_seed %08x %08x, split %08x %08x\n",
              hi, lo, pixel, sample, a.s0, a.s1, b.s0, b.s1);
  return false;
}
// one item: `count` consecutive samples of one pixel, the sample term advanced by one add each
bool item(uint32_t lo, uint32_t hi, uint32_t pixel, uint32_t sample0, uint32_t count) {
  const uint32_t v0 = rtd::rng_key_pixel(lo, pixel);
  uint32_t v1 = rtd::rng_key_sample(lo, hi, sample0);
  for (uint32_t k = 0; k < count; ++k) {
    if (!same(lo, hi, pixel, sample0 + k, rtd::rng_key_mix(v0, v1))) return false;
    v1 = rtd::rng_key_next(v1);
  }
  return true;
}
uint64_t splitmix(uint64_t& x) {
  uint64_t z = (x += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// pcg2d's rounds are bijections of (v0, v1): walk them backwards from the all-zero output to the
// first-round terms that hash to it (1664525 is odd, x ^= x >> 16 is an involution)
void zero_preimage(uint32_t& v0, uint32_t& v1) {
  v0 = 0u, v1 = 0u;
  for (int round = 0; round < 2; ++round) {
    v1 ^= v1 >> 16;
    v0 ^= v0 >> 16;
    v1 -= v0 * 1664525u;
    v0 -= v1 * 1664525u;
  }
}
uint32_t inv_mul(uint32_t a) {  // inverse of an odd a modulo 2^32 (Newton)
  uint32_t x = a;
  for (int k = 0; k < 5; ++k) x *= 2u - a * x;
  return x;
}
}  // namespace

int main() {
  // fixed seeds, corner pixels and samples, runs of consecutive samples across the 32-bit wrap
  const uint32_t seeds[][2] = {{0u, 0u}, {1u, 0u}, {0u, 1u}, {0xffffffffu, 0xffffffffu},
                               {0x12345678u, 0x9abcdef0u}};
  const uint32_t corners[] = {0u, 1u, 2u, 639999u, 0x7fffffffu, 0x80000000u, 0xfffffffeu,
                              0xffffffffu};
  for (const auto& s : seeds)
    for (uint32_t p : corners)
      for (uint32_t q : corners)
        if (!item(s[0], s[1], p, q - 16u, 40u)) return 1;
  // the pool items of a frame: every pixel of a small image, whole rows of samples
  for (uint32_t pixel = 0; pixel < 96u * 64u; ++pixel)
    if (!item(1u, 0u, pixel, (pixel % 31u) * 31u, 31u)) return 1;
  // random triples with random run lengths
  uint64_t st = 0x243F6A8885A308D3ull;
  while (g_n < 1200000ull) {
    const uint64_t a = splitmix(st), b = splitmix(st), c = splitmix(st);
    if (!item((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32),
              1u + (uint32_t)(c % 64u)))
      return 1;
  }
  // the all-zero state rng_seed replaces: for several seeds, the (pixel, sample) that hash to it,
  // reached directly and by stepping from 40 samples before
  uint32_t z0, z1;
  zero_preimage(z0, z1);
  const uint32_t inv = inv_mul(1664525u);
  for (const auto& s : seeds) {
    const uint32_t pixel = (z0 - rtd::rng_key_pixel(s[0], 0u)) * inv;
    const uint32_t sample = (z1 - rtd::rng_key_sample(s[0], s[1], 0u)) * inv;
    const Rng r = rtd::rng_seed(s[0], s[1], pixel, sample);
    if (r.s0 != 0x9E3779B9u || r.s1 != 0u) {
      std::printf("zero state not reached: seed %08x:%08x -> %08x %08x\n", s[1], s[0], r.s0, r.s1);
      return 1;
    }
    if (!item(s[0], s[1], pixel, sample - 40u, 80u)) return 1;
  }
  std::printf("rng_key_check ok: %llu triples\n", g_n);
  return 0;
}
