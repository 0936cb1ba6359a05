// The counter-based generator of the library: splitmix64 (Steele, Lea, Flood 2014), one call per draw.  Shared by the
// dropout masks (decoder.hip) and the sampled beam step (beam_step.hip).
#pragma once
#include <stdint.h>

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
