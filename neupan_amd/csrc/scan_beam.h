// scan_beam.h -- where a lidar beam starts and where it points (include/neupan_amd.h, "npa_world_scan"): ONE definition that
// world_scan_kernel (libneupan_amd.so) and grid_scan_kernel (libneupan_amd_grid.so, include/neupan_amd_grid.h) both compile,
// so that a beam of the occupancy-grid scan is the beam of the primitive scan bit for bit.  float64, every statement in the
// operation order scan_kernel composes a point in; no FMA contraction.
#ifndef NPA_SCAN_BEAM_H
#define NPA_SCAN_BEAM_H

#include <hip/hip_runtime.h>

#include "../../include/neupan_amd.h"

namespace npa_beam {

// the sensor pose = state o offset of a scene: its position and the two rotations a beam's direction goes through
struct Sensor {
  double sc, ss;    // cos, sin of the offset's heading
  double rc, rsn;   // cos, sin of the robot's heading
  double ox, oy;    // the sensor's world position
};

__device__ __forceinline__ Sensor sensor(const npa_scan_params& P) {
#pragma clang fp contract(off)
  Sensor S;
  S.sc = cos(P.offset[2]); S.ss = sin(P.offset[2]);
  S.rc = cos(P.state[2]); S.rsn = sin(P.state[2]);
  S.ox = (S.rc * P.offset[0] + (-S.rsn) * P.offset[1]) + P.state[0];
  S.oy = (S.rsn * P.offset[0] + S.rc * P.offset[1]) + P.state[1];
  return S;
}

// numpy.linspace(angle_min, angle_max, n)[ii] for 0 <= ii < n
__device__ __forceinline__ double angle(const npa_scan_params& P, int n, int ii) {
#pragma clang fp contract(off)
  const double step = n > 1 ? (P.angle_max - P.angle_min) / (double)(n - 1) : 0.0;
  return (n > 1 && ii == n - 1) ? P.angle_max : (double)ii * step + P.angle_min;
}

// the world direction of the beam at the sensor-frame angle `ang`
__device__ __forceinline__ void direction(const Sensor& S, double ang, double& dx, double& dy) {
#pragma clang fp contract(off)
  const double lx = cos(ang), ly = sin(ang);
  const double tx = S.sc * lx + (-S.ss) * ly, ty = S.ss * lx + S.sc * ly;
  dx = S.rc * tx + (-S.rsn) * ty;
  dy = S.rsn * tx + S.rc * ty;
}

}  // namespace npa_beam

#endif
