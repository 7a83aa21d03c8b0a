// A lidar world on the device (gfx950 only): what the reference gets from its simulator in example/run_exp.py --
// env.get_lidar_scan() and env.step(action) -- for B robots at once, handle-free and stream-ordered like frontend.hip.
//   world_scan_kernel       ray-casts every beam of every robot against the circles and segments of its world; the outputs are
//                           the ranges / beam velocities npa_scan_to_points takes (neupan.py:173-281 is the consumer);
//                           <true>: with Gaussian bearing and range noise (scan_noise.h), npa_world_scan_noisy
//   world_move_kernel       plant step (motion_predict_model, initial_path.py:388-444, in the float32 / float64 mix nominal_kernel
//                           uses), translation of the moving primitives, the robots' own edges written as moving segments
//   world_clearance_kernel  exact signed distance of every robot's polygon to the nearest primitive of its world
// All arithmetic is float64 in a fixed operation order: no FMA contraction in this file (the beam angle must be the value
// scan_kernel computes, bit for bit, and a (beam, primitive) pair must give the same t whichever chunk or call it is met in).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "handle.h"
#include "scan_beam.h"
#include "scan_noise.h"

namespace {

constexpr int WS_THREADS = 256;            // beams of a workgroup's tile; also the primitives culled per chunk
constexpr int WS_CAP = WS_THREADS;         // capacity of the LDS list: a chunk of WS_CAP primitives cannot overflow it
constexpr double WS_CULL_SLACK = 1.0 + 1e-9;   // on squared distances: rounding of the cull test must not drop a hit below range_max

// ordered compaction of a chunk's survivors: the slot of this thread's survivor and the chunk's total (scan_kernel's scheme)
__device__ __forceinline__ int compact_slot(bool keep, int lane, int wv, int* wave_tot, int& total) {
  const unsigned long long m = __ballot(keep);
  const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
  if (lane == 0) wave_tot[wv] = __popcll(m);
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < WS_THREADS / 64; ++k) {
    const int c = wave_tot[k];
    off += k < wv ? c : 0;
    tot += c;
  }
  total = __builtin_amdgcn_readfirstlane(tot);
  return off + before;
}

// the noisy scan's by-value scalars: the levels, and what selects the draws (scene = scene_base + blockIdx.y)
struct ScanNoise {
  double std, angle_std;
  unsigned long long seed;
  int scene_base, draw;
};

// One workgroup per (scene, tile of WS_THREADS beams).  Per chunk of WS_CAP primitives: phase 1, thread = primitive, culls
// against the sensor's reach and compacts the survivors, in index order and already reduced to what a beam needs of them,
// into LDS; phase 2, thread = beam, every lane walks the same list (broadcast reads).  Circles first, then segments: the walk
// is in primitive-index order and a lane's best changes only on t < best, so ties stay with the lowest index.  Every loop is
// wave-uniform; what depends on the lane is a select.
// NOISE (npa_world_scan_noisy): the beam is cast along ang + angle_std g_a and a hit's range becomes t + std g_r, clamped to
// [0, range_max]; the draws are per lane and straight-line (scan_noise.h).  The plain instantiation compiles none of it.
template <bool NOISE>
__global__ __launch_bounds__(WS_THREADS) void world_scan_kernel(
    int n_worlds, int c_stride, int s_stride, const double* __restrict__ circles, const double* __restrict__ segments,
    const int* __restrict__ n_circles, const int* __restrict__ n_segments, const npa_scan_params* __restrict__ params,
    const int* __restrict__ n_beams, int beam_stride, const int* __restrict__ skip, double* __restrict__ ranges,
    double* __restrict__ beam_vel, int* __restrict__ hit, ScanNoise Z) {
  __shared__ double l0[WS_CAP], l1[WS_CAP], l2[WS_CAP], l3[WS_CAP], l4[WS_CAP];
  __shared__ int lidx[WS_CAP];
  __shared__ int wave_tot[WS_THREADS / 64];
  const int b = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int n = n_beams ? n_beams[b] : beam_stride;
  n = n < 0 ? 0 : (n > beam_stride ? beam_stride : n);
  if ((int)blockIdx.x * WS_THREADS >= n) return;              // (the same in every thread of the workgroup)
  const npa_scan_params P = params[b];
  const int w = n_worlds == 1 ? 0 : b;
  int nC = c_stride > 0 ? n_circles[w] : 0, nS = s_stride > 0 ? n_segments[w] : 0;
  nC = nC < 0 ? 0 : (nC > c_stride ? c_stride : nC);
  nS = nS < 0 ? 0 : (nS > s_stride ? s_stride : nS);
  const int skip0 = skip ? skip[2 * b] : 0, skip1 = skip ? skip[2 * b + 1] : 0;
  const double* cw = circles + (size_t)w * c_stride * 6;
  const double* sw = segments + (size_t)w * s_stride * 6;

  // sensor pose = state o offset, and the beam's direction, composed as scan_kernel composes a point
  // (scan_beam.h: the occupancy-grid scan of libneupan_amd_grid.so starts and points its beams with the same code)
  const npa_beam::Sensor S = npa_beam::sensor(P);
  const double ox = S.ox, oy = S.oy;
  const int i = (int)blockIdx.x * WS_THREADS + tid;
  const bool live = i < n;
  const int ii = live ? i : n - 1;
  double ang = npa_beam::angle(P, n, ii);
  double g_r = 0.0;
  if constexpr (NOISE) {
    double g_a;
    npa_noise::draws(Z.seed, Z.scene_base + b, ii, Z.draw, g_a, g_r);
    const double turn = Z.angle_std * g_a;
    ang = Z.angle_std != 0.0 ? ang + turn : ang;               // (angle_std == 0: the angle's own bits, a zero's sign included)
  }
  double dx, dy;
  npa_beam::direction(S, ang, dx, dy);
  const double rmax = P.range_max;
  const double reach2 = (rmax * rmax) * WS_CULL_SLACK;

  double best = rmax;
  int bi = -1;

  // ---- circles: list entry = (centre - sensor, |centre - sensor|^2 - r^2)
  for (int c0 = 0; c0 < nC; c0 += WS_CAP) {
    const int p = c0 + tid;
    const bool have = p < nC;
    const double* q = cw + (size_t)(have ? p : 0) * 6;
    const double ocx = q[0] - ox, ocy = q[1] - oy, r = q[2];
    const double d2 = ocx * ocx + ocy * ocy;
    const double rr = rmax + r;
    const bool keep = have && d2 <= (rr * rr) * WS_CULL_SLACK;
    int cnt;
    const int slot = compact_slot(keep, lane, wv, wave_tot, cnt);
    if (keep) {
      l0[slot] = ocx; l1[slot] = ocy; l2[slot] = d2 - r * r; lidx[slot] = p;
    }
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
      const double cx = l0[k], cy = l1[k], c2 = l2[k];
      const int idx = lidx[k];
      const double bq = cx * dx + cy * dy;
      const double disc = bq * bq - c2;
      const bool inside = c2 <= 0.0;
      const bool hitc = inside || (disc >= 0.0 && bq > 0.0);
      if (__ballot(hitc) != 0ull) {                            // (wave-uniform)
        const double sq = sqrt(disc > 0.0 ? disc : 0.0);
        const double den = hitc && !inside ? bq + sq : 1.0;
        const double t = inside ? 0.0 : c2 / den;              // the near root b - sqrt(disc), without its cancellation
        const bool upd = hitc && t < best;
        best = upd ? t : best;
        bi = upd ? idx : bi;
      }
    }
    __syncthreads();
  }

  // ---- segments: list entry = (a - sensor, b - a, (a - sensor) x (b - a)); t = that cross product / (d x (b - a))
  for (int s0 = 0; s0 < nS; s0 += WS_CAP) {
    const int p = s0 + tid;
    const bool have = p < nS;
    const double* q = sw + (size_t)(have ? p : 0) * 6;
    const double wx = q[0] - ox, wy = q[1] - oy, ex = q[2] - q[0], ey = q[3] - q[1];
    const double e2 = ex * ex + ey * ey;
    double u = e2 > 0.0 ? -(wx * ex + wy * ey) / e2 : 0.0;    // the sensor's foot point on the segment
    u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
    const double fx = wx + u * ex, fy = wy + u * ey;
    const bool keep = have && !(p >= skip0 && p < skip1) && fx * fx + fy * fy <= reach2;
    int cnt;
    const int slot = compact_slot(keep, lane, wv, wave_tot, cnt);
    if (keep) {
      l0[slot] = wx; l1[slot] = wy; l2[slot] = ex; l3[slot] = ey; l4[slot] = wx * ey - wy * ex; lidx[slot] = nC + p;
    }
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
      const double wxk = l0[k], wyk = l1[k], exk = l2[k], eyk = l3[k], wxe = l4[k];
      const int idx = lidx[k];
      const double det = dx * eyk - dy * exk;
      const double un = wxk * dy - wyk * dx;
      const bool neg = det < 0.0;
      const double ad = neg ? -det : det, tn = neg ? -wxe : wxe, us = neg ? -un : un;
      const bool valid = ad > 0.0 && tn >= 0.0 && us >= 0.0 && us <= ad;      // t >= 0 and 0 <= u <= 1 without a division
      // t < best cross-multiplied, with room for the roundings of the product and of the quotient: it never rejects a t
      // that the exact test below would accept, so the result is the minimum of the divided values whatever came before
      const bool cand = valid && tn <= (best * ad) * (1.0 + 1e-12);
      if (__ballot(cand) != 0ull) {                            // (wave-uniform)
        const double t = tn / (cand ? ad : 1.0) + 0.0;         // (+ 0: no negative zero)
        const bool upd = cand && t < best;
        best = upd ? t : best;
        bi = upd ? idx : bi;
      }
    }
    __syncthreads();
  }

  if constexpr (NOISE) {                                       // a miss stays range_max: no phantom point
    const double v = best + Z.std * g_r;
    const double p = (v > 0.0 ? v : 0.0) + 0.0;                // (+ 0: no negative zero)
    best = bi >= 0 ? (p < rmax ? p : rmax) : rmax;
  }
  if (live) {
    ranges[(size_t)b * beam_stride + i] = best;
    if (hit) hit[(size_t)b * beam_stride + i] = bi;
    if (beam_vel) {
      double vx = 0.0, vy = 0.0;
      if (bi >= 0) {
        const double* q = bi < nC ? cw + (size_t)bi * 6 + 3 : sw + (size_t)(bi - nC) * 6 + 4;
        vx = q[0]; vy = q[1];
      }
      beam_vel[(size_t)b * 2 * beam_stride + i] = vx;
      beam_vel[(size_t)b * 2 * beam_stride + beam_stride + i] = vy;
    }
  }
}

// What the two step kernels need by value.  The robot polygon in the robot frame: edge e runs from (ax, ay)[e] to (bx, by)[e],
// counter-clockwise; (dx, dy) = b - a and il = 1 / |b - a|.  Entries at or beyond E are not read.
struct WorldStepParams {
  int batch, n_worlds, c_stride, s_stride, kin, E, peer_base, has_bounds;
  double dt, L;
  double bounds[4];
  double ax[NPA_MAX_E], ay[NPA_MAX_E], bx[NPA_MAX_E], by[NPA_MAX_E], dx[NPA_MAX_E], dy[NPA_MAX_E], il[NPA_MAX_E];
};

constexpr int WM_THREADS = 256;

// thread g: robot g (plant, then its edges into the segment tail), or circle, or segment of a world.  The tail
// [peer_base, peer_base + batch * E) belongs to the robot threads: the segment threads leave it alone.
__global__ __launch_bounds__(WM_THREADS) void world_move_kernel(
    WorldStepParams K, double* __restrict__ circles, double* __restrict__ segments, const int* __restrict__ n_circles,
    const int* __restrict__ n_segments, double* __restrict__ state, const float* __restrict__ action,
    const int* __restrict__ frozen) {
  const long long g = (long long)blockIdx.x * WM_THREADS + threadIdx.x;
  const long long nc = (long long)K.n_worlds * K.c_stride, ns = (long long)K.n_worlds * K.s_stride;
  const double dt = K.dt;
  if (g < K.batch) {
    const int b = (int)g;
    const double x0 = state[b * 3 + 0], y0 = state[b * 3 + 1], th0 = state[b * 3 + 2];
    double px = x0, py = y0, pth = th0;
    if (!(frozen && frozen[b] != 0)) {
      const float v = action[b * 2 + 0], w = action[b * 2 + 1];
      if (K.kin == NPA_KIN_OMNI) {               // the action is (vx, vy) already (neupan.py:158-164)
        px = px + dt * (double)v;
        py = py + dt * (double)w;
      } else {                                   // motion_predict_model :398-432, as nominal_kernel steps it
        const float dt32 = (float)dt, L32 = (float)K.L;
        const float c32 = (float)cos(pth), s32 = (float)sin(pth);
        const float d0 = (v * c32) * dt32, d1 = (v * s32) * dt32;
        float d2;
        if (K.kin == NPA_KIN_ACKER) d2 = ((v * (float)tan((double)w)) / L32) * dt32;
        else d2 = w * dt32;
        px = px + (double)d0; py = py + (double)d1; pth = pth + (double)d2;
      }
      state[b * 3 + 0] = px; state[b * 3 + 1] = py; state[b * 3 + 2] = pth;
    }
    if (K.peer_base >= 0) {
      const double c = cos(pth), s = sin(pth);
      const double vx = dt > 0.0 ? (px - x0) / dt : 0.0, vy = dt > 0.0 ? (py - y0) / dt : 0.0;
      double* out = segments + ((size_t)K.peer_base + (size_t)b * K.E) * 6;
#pragma unroll
      for (int e = 0; e < NPA_MAX_E; ++e) {
        if (e < K.E) {
          out[e * 6 + 0] = (c * K.ax[e] + (-s) * K.ay[e]) + px;
          out[e * 6 + 1] = (s * K.ax[e] + c * K.ay[e]) + py;
          out[e * 6 + 2] = (c * K.bx[e] + (-s) * K.by[e]) + px;
          out[e * 6 + 3] = (s * K.bx[e] + c * K.by[e]) + py;
          out[e * 6 + 4] = vx;
          out[e * 6 + 5] = vy;
        }
      }
    }
  } else if (g < K.batch + nc) {
    const long long k = g - K.batch;
    const int w = (int)(k / K.c_stride), p = (int)(k % K.c_stride);
    if (p < n_circles[w]) {
      double* q = circles + (size_t)k * 6;
      double vx = q[3], vy = q[4];
      if (vx != 0.0 || vy != 0.0) {
        const double cx = q[0] + vx * dt, cy = q[1] + vy * dt;
        q[0] = cx; q[1] = cy;
        if (K.has_bounds) {                      // outside the box: the offending component points back inside
          if (cx < K.bounds[0]) vx = fabs(vx);
          if (cx > K.bounds[2]) vx = -fabs(vx);
          if (cy < K.bounds[1]) vy = fabs(vy);
          if (cy > K.bounds[3]) vy = -fabs(vy);
          q[3] = vx; q[4] = vy;
        }
      }
    }
  } else if (g < K.batch + nc + ns) {
    const long long k = g - K.batch - nc;
    const int w = (int)(k / K.s_stride), p = (int)(k % K.s_stride);
    const bool tail = K.peer_base >= 0 && p >= K.peer_base && p < K.peer_base + K.batch * K.E;
    if (p < n_segments[w] && !tail) {
      double* q = segments + (size_t)k * 6;
      const double vx = q[4], vy = q[5];
      if (vx != 0.0 || vy != 0.0) {
        q[0] = q[0] + vx * dt; q[1] = q[1] + vy * dt;
        q[2] = q[2] + vx * dt; q[3] = q[3] + vy * dt;
      }
    }
  }
}

// the robot polygon in LDS: the clearance kernel's edge loops read it by broadcast (by value in scalar registers it does not
// fit: 5 x NPA_MAX_E doubles beside the kernel's own state spill)
struct Polygon {
  double ax[NPA_MAX_E], ay[NPA_MAX_E], dx[NPA_MAX_E], dy[NPA_MAX_E], il[NPA_MAX_E];
};

// signed distance of the robot-frame point (x, y) to the polygon (clearance.hip: signed_dist, in float64)
__device__ __forceinline__ double poly_dist(const Polygon& G, int E, double x, double y) {
  double best = __builtin_inf(), deep = -__builtin_inf();
  for (int e = 0; e < E; ++e) {
    const double rx = x - G.ax[e], ry = y - G.ay[e];
    deep = fmax(deep, (G.dy[e] * rx - G.dx[e] * ry) * G.il[e]);              // outward normal (dy, -dx) / |edge|
    double u = ((rx * G.dx[e] + ry * G.dy[e]) * G.il[e]) * G.il[e];
    u = fmin(fmax(u, 0.0), 1.0);
    const double qx = rx - u * G.dx[e], qy = ry - u * G.dy[e];
    best = fmin(best, qx * qx + qy * qy);
  }
  return deep <= 0.0 ? deep : sqrt(best);
}

// squared distance of the point (x, y) to the segment p + u d, u in [0, 1]
__device__ __forceinline__ double point_seg2(double x, double y, double px, double py, double dx, double dy) {
  const double rx = x - px, ry = y - py, d2 = dx * dx + dy * dy;
  double u = d2 > 0.0 ? (rx * dx + ry * dy) / d2 : 0.0;
  u = fmin(fmax(u, 0.0), 1.0);
  const double qx = rx - u * dx, qy = ry - u * dy;
  return qx * qx + qy * qy;
}

constexpr int WC_THREADS = 64;

// One wave per robot: lanes stride over the primitives of its world (brought into the robot frame), wave-uniform trip
// counts, then a minimum over the lanes.
__global__ __launch_bounds__(WC_THREADS) void world_clearance_kernel(
    WorldStepParams K, const double* __restrict__ circles, const double* __restrict__ segments,
    const int* __restrict__ n_circles, const int* __restrict__ n_segments, const double* __restrict__ state,
    double* __restrict__ clearance) {
  __shared__ Polygon G;
  const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int E = K.E;
  if (lane == 0) {
#pragma unroll
    for (int e = 0; e < NPA_MAX_E; ++e) {
      G.ax[e] = K.ax[e]; G.ay[e] = K.ay[e]; G.dx[e] = K.dx[e]; G.dy[e] = K.dy[e]; G.il[e] = K.il[e];
    }
  }
  __syncthreads();
  const int w = K.n_worlds == 1 ? 0 : b;
  int nC = K.c_stride > 0 ? n_circles[w] : 0, nS = K.s_stride > 0 ? n_segments[w] : 0;
  nC = nC < 0 ? 0 : (nC > K.c_stride ? K.c_stride : nC);
  nS = nS < 0 ? 0 : (nS > K.s_stride ? K.s_stride : nS);
  const double* cw = circles + (size_t)w * K.c_stride * 6;
  const double* sw = segments + (size_t)w * K.s_stride * 6;
  const double sx = state[b * 3 + 0], sy = state[b * 3 + 1], th = state[b * 3 + 2];
  const double c = cos(th), s = sin(th);
  const int own0 = K.peer_base >= 0 ? K.peer_base + b * E : 0, own1 = K.peer_base >= 0 ? own0 + E : 0;
  double best = __builtin_inf();
  for (int p0 = 0; p0 < nC; p0 += WC_THREADS) {
    const int p = p0 + lane;
    const bool have = p < nC;
    const double* q = cw + (size_t)(have ? p : 0) * 6;
    const double gx = q[0] - sx, gy = q[1] - sy;
    const double d = poly_dist(G, E, c * gx + s * gy, c * gy - s * gx) - q[2];
    best = have && d < best ? d : best;
  }
  for (int p0 = 0; p0 < nS; p0 += WC_THREADS) {
    const int p = p0 + lane;
    const bool have = p < nS && !(p >= own0 && p < own1);
    const double* q = sw + (size_t)(p < nS ? p : 0) * 6;
    const double g0x = q[0] - sx, g0y = q[1] - sy, g1x = q[2] - sx, g1y = q[3] - sy;
    const double px = c * g0x + s * g0y, py = c * g0y - s * g0x;
    const double qx = c * g1x + s * g1y, qy = c * g1y - s * g1x;
    const double ex = qx - px, ey = qy - py;
    const double dp = poly_dist(G, E, px, py), dq = poly_dist(G, E, qx, qy);
    bool touch = dp <= 0.0 || dq <= 0.0;
    double m2 = __builtin_inf();
    for (int e = 0; e < E; ++e) {
      const double ax = G.ax[e], ay = G.ay[e], edx = G.dx[e], edy = G.dy[e];
      m2 = fmin(m2, point_seg2(ax, ay, px, py, ex, ey));
      // proper crossing of the segment and edge e: each one's ends on opposite sides of the other
      const double o1 = ex * (ay - py) - ey * (ax - px);
      const double o2 = ex * ((ay + edy) - py) - ey * ((ax + edx) - px);
      const double o3 = edx * (py - ay) - edy * (px - ax);
      const double o4 = edx * (qy - ay) - edy * (qx - ax);
      touch = touch || (o1 * o2 < 0.0 && o3 * o4 < 0.0);
    }
    const double d = touch ? 0.0 : fmin(fmin(dp, dq), sqrt(m2));
    best = have && d < best ? d : best;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) best = fmin(best, __shfl_xor(best, m, 64));
  if (lane == 0) clearance[b] = best;
}

}  // namespace

extern "C" int npa_world_list_capacity(void) { return WS_CAP; }

extern "C" int npa_world_scan(int batch, int n_worlds, int c_stride, int s_stride, const double* circles,
                              const double* segments, const int32_t* n_circles, const int32_t* n_segments,
                              const npa_scan_params* params, const int32_t* n_beams, int beam_stride, const int32_t* skip,
                              double* ranges, double* beam_vel, int32_t* hit, void* stream) {
  if (batch <= 0 || beam_stride <= 0 || c_stride < 0 || s_stride < 0 || !params || !ranges || !n_circles || !n_segments ||
      (c_stride > 0 && !circles) || (s_stride > 0 && !segments))
    return fail(NPA_E_ARG, "npa_world_scan: bad argument");
  if (n_worlds != 1 && n_worlds != batch) return fail(NPA_E_ARG, "npa_world_scan: n_worlds must be 1 or batch");
  if (batch > 65535) return fail(NPA_E_ARG, "npa_world_scan: batch above 65535");
  hipLaunchKernelGGL(world_scan_kernel<false>, dim3((beam_stride + WS_THREADS - 1) / WS_THREADS, batch), dim3(WS_THREADS), 0,
                     (hipStream_t)stream, n_worlds, c_stride, s_stride, circles, segments, n_circles, n_segments, params,
                     n_beams, beam_stride, skip, ranges, beam_vel, hit, ScanNoise{});
  HIP_TRY(hipGetLastError());
  return NPA_OK;
}

static bool noise_level_ok(double x) { return x >= 0.0 && std::isfinite(x); }

extern "C" int npa_world_scan_noisy(int batch, int n_worlds, int c_stride, int s_stride, const double* circles,
                                    const double* segments, const int32_t* n_circles, const int32_t* n_segments,
                                    const npa_scan_params* params, const int32_t* n_beams, int beam_stride,
                                    const int32_t* skip, double* ranges, double* beam_vel, int32_t* hit, double std,
                                    double angle_std, uint64_t seed, int scene_base, int draw, void* stream) {
  if (batch <= 0 || beam_stride <= 0 || c_stride < 0 || s_stride < 0 || !params || !ranges || !n_circles || !n_segments ||
      (c_stride > 0 && !circles) || (s_stride > 0 && !segments))
    return fail(NPA_E_ARG, "npa_world_scan_noisy: bad argument");
  if (n_worlds != 1 && n_worlds != batch) return fail(NPA_E_ARG, "npa_world_scan_noisy: n_worlds must be 1 or batch");
  if (batch > 65535) return fail(NPA_E_ARG, "npa_world_scan_noisy: batch above 65535");
  if (!noise_level_ok(std) || !noise_level_ok(angle_std))
    return fail(NPA_E_ARG, "npa_world_scan_noisy: std and angle_std must be finite and >= 0");
  if (draw < 0 || scene_base < 0 || scene_base > 0x7fffffff - batch)
    return fail(NPA_E_ARG, "npa_world_scan_noisy: draw and scene_base must be >= 0 (and scene_base + batch an int)");
  ScanNoise Z;
  Z.std = std; Z.angle_std = angle_std; Z.seed = seed; Z.scene_base = scene_base; Z.draw = draw;
  hipLaunchKernelGGL(world_scan_kernel<true>, dim3((beam_stride + WS_THREADS - 1) / WS_THREADS, batch), dim3(WS_THREADS), 0,
                     (hipStream_t)stream, n_worlds, c_stride, s_stride, circles, segments, n_circles, n_segments, params,
                     n_beams, beam_stride, skip, ranges, beam_vel, hit, Z);
  HIP_TRY(hipGetLastError());
  return NPA_OK;
}

extern "C" int npa_scan_noise_draws(uint64_t seed, int scene, int draw, int first_beam, int n, double* out) {
  if (scene < 0 || draw < 0 || first_beam < 0 || n < 0 || !out || first_beam > 0x7fffffff - n)
    return fail(NPA_E_ARG, "npa_scan_noise_draws: bad argument");
  for (int k = 0; k < n; ++k) npa_noise::draws(seed, scene, first_beam + k, draw, out[2 * k], out[2 * k + 1]);
  return NPA_OK;
}

extern "C" int npa_world_step(int batch, int n_worlds, int c_stride, int s_stride, double* circles, double* segments,
                              const int32_t* n_circles, const int32_t* n_segments, double* state, const float* action,
                              const int32_t* frozen, double dt, int kinematics, double wheelbase, const double* bounds,
                              int edge_num, const double* vertices, int peer_base, double* clearance, void* stream) {
  if (batch <= 0 || c_stride < 0 || s_stride < 0 || !state || !action || !n_circles || !n_segments ||
      (c_stride > 0 && !circles) || (s_stride > 0 && !segments) || !(dt >= 0.0))
    return fail(NPA_E_ARG, "npa_world_step: bad argument");
  if (n_worlds != 1 && n_worlds != batch) return fail(NPA_E_ARG, "npa_world_step: n_worlds must be 1 or batch");
  if (kinematics < 0 || kinematics > 2) return fail(NPA_E_ARG, "npa_world_step: unknown kinematics");
  if (kinematics == NPA_KIN_ACKER && !(wheelbase > 0)) return fail(NPA_E_ARG, "npa_world_step: acker needs wheelbase > 0");
  const bool peers = peer_base >= 0;
  if ((peers || clearance) && !vertices) return fail(NPA_E_ARG, "npa_world_step: peers and clearance need the robot's vertices");
  if (vertices && (edge_num < 3 || edge_num > NPA_MAX_E)) return fail(NPA_E_ARG, "npa_world_step: edge_num outside [3,NPA_MAX_E]");
  if (peers && n_worlds != 1) return fail(NPA_E_ARG, "npa_world_step: peers need one shared world (n_worlds == 1)");
  if (peers && (long long)peer_base + (long long)batch * edge_num > (long long)s_stride)
    return fail(NPA_E_ARG, "npa_world_step: the peer tail does not fit s_stride");
  WorldStepParams K = {};
  K.batch = batch; K.n_worlds = n_worlds; K.c_stride = c_stride; K.s_stride = s_stride; K.kin = kinematics;
  K.E = vertices ? edge_num : 0; K.peer_base = peers ? peer_base : -1; K.has_bounds = bounds ? 1 : 0;
  K.dt = dt; K.L = wheelbase;
  for (int k = 0; k < 4; ++k) K.bounds[k] = bounds ? bounds[k] : 0.0;
  for (int e = 0; e < K.E; ++e) {
    const int f = (e + 1) % K.E;
    K.ax[e] = vertices[2 * e]; K.ay[e] = vertices[2 * e + 1]; K.bx[e] = vertices[2 * f]; K.by[e] = vertices[2 * f + 1];
    K.dx[e] = K.bx[e] - K.ax[e]; K.dy[e] = K.by[e] - K.ay[e];
    const double len = std::sqrt(K.dx[e] * K.dx[e] + K.dy[e] * K.dy[e]);
    if (!(len > 0.0)) return fail(NPA_E_ARG, "npa_world_step: a polygon edge of zero length");
    K.il[e] = 1.0 / len;
  }
  const long long total = (long long)batch + (long long)n_worlds * c_stride + (long long)n_worlds * s_stride;
  if ((total + WM_THREADS - 1) / WM_THREADS > 0x7fffffffLL) return fail(NPA_E_ARG, "npa_world_step: world too large");
  hipLaunchKernelGGL(world_move_kernel, dim3((unsigned)((total + WM_THREADS - 1) / WM_THREADS)), dim3(WM_THREADS), 0,
                     (hipStream_t)stream, K, circles, segments, n_circles, n_segments, state, action, frozen);
  HIP_TRY(hipGetLastError());
  if (clearance) {
    hipLaunchKernelGGL(world_clearance_kernel, dim3(batch), dim3(WC_THREADS), 0, (hipStream_t)stream, K, circles, segments,
                       n_circles, n_segments, state, clearance);
    HIP_TRY(hipGetLastError());
  }
  return NPA_OK;
}
