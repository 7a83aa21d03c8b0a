// scan_noise.h -- the lidar noise draws (include/neupan_amd.h, "npa_world_scan_noisy"): ONE definition that the host export
// (npa_scan_noise_draws) and the noisy instantiation of world_scan_kernel both compile.  The integer part -- the splitmix64
// finaliser of npa_world_behave, chained over seed + scene, beam, draw, k -- is exact; the Box-Muller transform on top of it
// is float64 with every statement one rounded operation, so host and device differ only where libm and the device math
// library do (ln, sqrt is exact, cos).  Per lane and straight-line: no loop, no table, nothing indexed at run time.
// The device takes cospi(2 u): its argument reduction is exact and short, where cos(2 pi u) would inline a second
// large-argument reduction beside the one the scan kernel already carries (the product library has a size limit).
#ifndef NPA_SCAN_NOISE_H
#define NPA_SCAN_NOISE_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define NPA_NOISE_HD __host__ __device__ __forceinline__

namespace npa_noise {

NPA_NOISE_HD uint64_t mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// what the four uniforms of a (scene, beam, draw) share: mix(mix(mix(seed + scene) + beam) + draw)
NPA_NOISE_HD uint64_t key(uint64_t seed, int scene, int beam, int draw) {
  uint64_t z = mix(seed + (uint64_t)(int64_t)scene);
  z = mix(z + (uint64_t)(int64_t)beam);
  return mix(z + (uint64_t)(int64_t)draw);
}

// U(seed, scene, beam, draw, k) in [0, 1) from the key
NPA_NOISE_HD double uniform(uint64_t key3, unsigned k) { return (double)(mix(key3 + k) >> 11) * 0x1.0p-53; }

// g(k0) = sqrt(-2 ln(1 - U(k0))) cos(2 pi U(k0 + 1)); 1 - U is in (0, 1], so |g| <= sqrt(106 ln 2) < 8.6
NPA_NOISE_HD double gauss(uint64_t key3, unsigned k0) {
#pragma clang fp contract(off)
  const double u0 = uniform(key3, k0), u1 = uniform(key3, k0 + 1u);
  const double l = log(1.0 - u0);
  const double r = sqrt(-2.0 * l);
#if defined(__HIP_DEVICE_COMPILE__)
  const double c = cospi(2.0 * u1);
#else
  const double c = cos(6.283185307179586 * u1);
#endif
  return r * c;
}

// (g_a, g_r) of a beam: the bearing draw is g(0), the range draw g(2)
NPA_NOISE_HD void draws(uint64_t seed, int scene, int beam, int draw, double& g_a, double& g_r) {
  const uint64_t k3 = key(seed, scene, beam, draw);
  g_a = gauss(k3, 0u);
  g_r = gauss(k3, 2u);
}

}  // namespace npa_noise

#endif
