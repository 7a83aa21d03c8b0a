// Exact clearance of a plan against the whole moving cloud (gfx950 only): one launch behind the plan, on the plan's stream.
//   clearance_kernel   stands beside the reference's only safety signal: min_distance, the NETWORK's distance at horizon step 0
//                      over the DECIMATED cloud (dune.py:98; the decimation: pan.py:171-174), which check_stop compares with
//                      collision_threshold (neupan.py:169-170); info["collision"] is declared (neupan.py:86) and never set.
//                      Here: the closed-form distance of the robot polygon to EVERY point of the cloud (point flow pan.py:182,
//                      robot frame pan.py:205-210), for every step of the trajectory given, signed (minus the penetration
//                      depth inside), with the index of the nearest point and a per-scene summary.
// One workgroup per scene; its waves stride over the horizon steps, each wave running its step over the whole cloud (lane =
// consecutive n, 16-byte loads where the rows allow them) and reducing (distance, index) as ONE ordered 64-bit key -- the
// ordered-float transform of the distance in the high word, n in the low word -- so that ties resolve to the lowest index and
// the result does not depend on the order of the reduction.  The summary is a reduction of the T + 1 step values through LDS in
// the same launch.  No workspace, no atomics, nothing read at or beyond column n_points[b].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "launch.h"

namespace {

constexpr int CLR_WAVES = 8;                 // waves of a scene's workgroup: T + 1 = 11 steps take two rounds, 21 three
constexpr int CLR_THREADS = 64 * CLR_WAVES;
constexpr int CLR_STEPS = NPA_MAX_T + 1;     // horizon steps of the longest trajectory the ABI accepts

// What the kernel needs of a handle, by value: the polygon as vertices, edge vectors and 1 / |edge| (edge e runs from vertex e
// to vertex e + 1, counter-clockwise; filled on the host from DevParams' pv* / pd*), the box of the axis-aligned fast path, the
// horizon and the step time.  The polygon lives in scalar registers; 1 / |edge|^2 is il * il in the kernel, not a sixth array:
// with it the 8-edge instantiation does not fit the scalar registers of a wave and spills.
struct ClearanceParams {
  int T, rect;
  double dt;
  float rcx, rcy, rhx, rhy;
  float vx[NPA_MAX_E], vy[NPA_MAX_E], dx[NPA_MAX_E], dy[NPA_MAX_E], il[NPA_MAX_E];
};

struct StepFrame {
  float c, s, tx, ty, tdt;    // rotation and translation of the robot at step t; t * dt
};

// monotone float -> uint map (dune_device.h: ordered_key; NaN sorts last) and its inverse
__device__ __forceinline__ unsigned ordered_key(float d) {
  if (d != d) return 0xFFFFFFFEu;
  const unsigned b = __float_as_uint(d);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) {
  if (k == 0xFFFFFFFEu) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_u64(unsigned long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xF, 0xF, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xF, 0xF, false);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long umin64(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int l) {
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, l), hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}
// full-wave minimum of a 64-bit key, every lane active: DPP inside each row of 16 lanes (quad permutes, then the two row
// mirrors), then one readlane per row; the result is the same in every lane
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
  v = umin64(v, dpp_u64<0xB1>(v));
  v = umin64(v, dpp_u64<0x4E>(v));
  v = umin64(v, dpp_u64<0x141>(v));
  v = umin64(v, dpp_u64<0x140>(v));
  return umin64(umin64(readlane_u64(v, 0), readlane_u64(v, 16)), umin64(readlane_u64(v, 32), readlane_u64(v, 48)));
}

// signed distance of the robot-frame point (x, y) to the polygon: outside, the smallest point-segment distance; inside (on
// the inner side of every edge line), the largest signed distance to an edge line, <= 0
template <int E>
__device__ __forceinline__ float signed_dist(const ClearanceParams& K, float x, float y) {
  if (E == 4 && K.rect) {                      // wave-uniform: an axis-aligned box
    const float ax = fabsf(x - K.rcx) - K.rhx, ay = fabsf(y - K.rcy) - K.rhy;
    const float ox = fmaxf(ax, 0.f), oy = fmaxf(ay, 0.f);
    const float in = fminf(fmaxf(ax, ay), 0.f);
    return (__builtin_sqrtf(fmaf(ox, ox, oy * oy)) + in) + 0.f;       // (one of the two terms is 0; + 0: no negative zero)
  }
  float best = 3.0e38f, deep = -3.0e38f;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const float rx = x - K.vx[e], ry = y - K.vy[e];
    deep = fmaxf(deep, fmaf(K.dy[e], rx, -(K.dx[e] * ry)) * K.il[e]);  // outward normal (dy, -dx) / |edge|
    float u = (fmaf(rx, K.dx[e], ry * K.dy[e]) * K.il[e]) * K.il[e];
    u = fminf(fmaxf(u, 0.f), 1.f);
    const float qx = fmaf(-u, K.dx[e], rx), qy = fmaf(-u, K.dy[e], ry);
    best = fminf(best, fmaf(qx, qx, qy * qy));
  }
  return (deep <= 0.f ? deep : __builtin_sqrtf(best)) + 0.f;
}

template <int E>
__device__ __forceinline__ void visit(const ClearanceParams& K, const StepFrame& F, float px, float py, float vx, float vy, int n,
                                      unsigned long long& best) {
  const float gx = fmaf(F.tdt, vx, px) - F.tx, gy = fmaf(F.tdt, vy, py) - F.ty;    // pan.py:182, then pan.py:210
  const float x = fmaf(F.c, gx, F.s * gy), y = fmaf(F.c, gy, -(F.s * gx));
  // (a point that is not a finite number is not near anything: fminf / fmaxf would otherwise drop its NaN)
  const float sd = signed_dist<E>(K, x, y), mag = fabsf(x) + fabsf(y);
  const float d = mag < INFINITY ? sd : mag;
  best = umin64(best, ((unsigned long long)ordered_key(d) << 32) | (unsigned)n);
}

template <int E>
__global__ __launch_bounds__(CLR_THREADS) void clearance_kernel(
    ClearanceParams K, int n_stride, const float* __restrict__ traj, const float* __restrict__ points,
    const float* __restrict__ vel, const int* __restrict__ n_points, float threshold, float* __restrict__ clearance,
    int* __restrict__ nearest, float* __restrict__ min_clearance, int* __restrict__ first_violation) {
  __shared__ StepFrame frame[CLR_STEPS];
  __shared__ float step_clr[CLR_STEPS];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = K.T;
  int n = n_points ? n_points[b] : n_stride;
  n = n < 0 ? 0 : (n > n_stride ? n_stride : n);              // the selection's clamp
  if (tid <= T) {
    const float* s = traj + (size_t)b * 3 * (T + 1);
    StepFrame F;
    npa_trig(s[2 * (T + 1) + tid], F.c, F.s);
    F.tx = s[tid];
    F.ty = s[(T + 1) + tid];
    F.tdt = (float)((double)tid * K.dt);
    frame[tid] = F;
  }
  __syncthreads();
  const float* __restrict__ px = points + (size_t)b * 2 * n_stride;
  const float* __restrict__ py = px + n_stride;
  const float* __restrict__ vx = vel ? vel + (size_t)b * 2 * n_stride : nullptr;
  const float* __restrict__ vy = vel ? vx + n_stride : nullptr;
  // 16-byte loads where every row of the scene starts on a 16-byte boundary (the same in every lane)
  const bool wide = ((((uintptr_t)px | (uintptr_t)py | (uintptr_t)vx | (uintptr_t)vy) & 15) == 0);
  for (int t = wave; t <= T; t += CLR_WAVES) {
    const StepFrame F = frame[t];
    unsigned long long best = ~0ull;
    int i = lane;
    if (wide) {
      const int n4 = n >> 2;
      for (int q = lane; q < n4; q += 64) {
        const float4 X = reinterpret_cast<const float4*>(px)[q], Y = reinterpret_cast<const float4*>(py)[q];
        float4 U = make_float4(0.f, 0.f, 0.f, 0.f), V = U;
        if (vx) {
          U = reinterpret_cast<const float4*>(vx)[q];
          V = reinterpret_cast<const float4*>(vy)[q];
        }
        visit<E>(K, F, X.x, Y.x, U.x, V.x, 4 * q, best);
        visit<E>(K, F, X.y, Y.y, U.y, V.y, 4 * q + 1, best);
        visit<E>(K, F, X.z, Y.z, U.z, V.z, 4 * q + 2, best);
        visit<E>(K, F, X.w, Y.w, U.w, V.w, 4 * q + 3, best);
      }
      i = (n4 << 2) + lane;
    }
    for (; i < n; i += 64) visit<E>(K, F, px[i], py[i], vx ? vx[i] : 0.f, vy ? vy[i] : 0.f, i, best);
    best = wave_min_u64(best);                                 // (every lane is back here: the loops only mask lanes off inside)
    const float d = n > 0 ? key_value((unsigned)(best >> 32)) : INFINITY;
    if (lane == 0) {
      clearance[(size_t)b * (T + 1) + t] = d;
      nearest[(size_t)b * (T + 1) + t] = n > 0 ? (int)(unsigned)best : -1;
      step_clr[t] = d;
    }
  }
  __syncthreads();
  if (wave == 0) {                                             // the scene's summary: lane t holds step t
    const bool have = lane <= T;
    const float d = have ? step_clr[lane] : INFINITY;
    const unsigned long long viol = __ballot(have && d < threshold);
    const unsigned long long m = wave_min_u64(((unsigned long long)ordered_key(d) << 32) | (unsigned)lane);
    if (lane == 0) {
      if (min_clearance) min_clearance[b] = key_value((unsigned)(m >> 32));
      if (first_violation) first_violation[b] = viol ? __ffsll((long long)viol) - 1 : -1;
    }
  }
}

}  // namespace

hipError_t npa_launch_clearance(const DevParams& P, int batch, int n_stride, const float* traj, const float* points,
                                           const float* velocities, const int* n_points, float threshold, float* clearance,
                                           int* nearest, float* min_clearance, int* first_violation, hipStream_t stream) {
  if (P.E < 3 || P.E > NPA_MAX_E || P.T + 1 > CLR_STEPS) return hipErrorInvalidValue;
  ClearanceParams K = {};
  K.T = P.T;
  K.rect = P.geo_rect;
  K.dt = P.dt;
  K.rcx = P.rcx; K.rcy = P.rcy; K.rhx = P.rhx; K.rhy = P.rhy;
  for (int e = 0; e < P.E; ++e) {
    K.vx[e] = P.pvx[e]; K.vy[e] = P.pvy[e]; K.dx[e] = P.pdx[e]; K.dy[e] = P.pdy[e];
    K.il[e] = (float)(1.0 / std::sqrt((double)P.pdx[e] * P.pdx[e] + (double)P.pdy[e] * P.pdy[e]));
  }
#define LAUNCH(EE)                                                                                                          \
  case EE:                                                                                                                  \
    hipLaunchKernelGGL(clearance_kernel<EE>, dim3(batch), dim3(CLR_THREADS), 0, stream, K, n_stride, traj, points, velocities, \
                       n_points, threshold, clearance, nearest, min_clearance, first_violation);                            \
    break
  switch (P.E) {
    LAUNCH(3); LAUNCH(4); LAUNCH(5); LAUNCH(6); LAUNCH(7); LAUNCH(8);
  }
#undef LAUNCH
  return hipGetLastError();
}
