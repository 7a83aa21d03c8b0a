// An occupancy grid as the third kind of obstacle of the device world (gfx950 only; include/neupan_amd_grid.h is the
// specification): libneupan_amd_grid.so, a library of its own because libneupan_amd.so is held below 2 MiB.
//   grid_scan_kernel       one lane per beam: walks the cells along the ray and merges the map's range into the ranges the
//                          primitive scan (npa_world_scan[_noisy]) left; <true>: with the bearing and range noise of scan_noise.h
//   grid_clearance_kernel  one wave per robot: the exact distance of its polygon to the occupied cells near it, merged into the
//                          clearance npa_world_step left
// All arithmetic is float64 in a fixed operation order: no FMA contraction in this file (a face coordinate is x0 + i * res and a
// crossing time (X - o) / d, each operation rounded once, whichever cell the walk reaches it from).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "../../include/neupan_amd_grid.h"
#include "scan_beam.h"
#include "scan_noise.h"

namespace {

constexpr int GS_THREADS = 256;            // beams of a workgroup
constexpr int GC_THREADS = 64;             // one wave per robot
constexpr int LOCATE_FIXES = 2;            // corrections of the first cell's estimate, per axis

struct GridArg {
  const uint8_t* cells;
  int nx, ny;
  double x0, y0, res;
};

struct GridNoise {
  double std, angle_std;
  unsigned long long seed;
  int scene_base, draw;
};

// the coordinate of face k of an axis: one multiply, one add
__device__ __forceinline__ double face(double g0, double res, int k) { return g0 + (double)k * res; }

// the time at which the ray o + t d (d != 0) crosses face k
__device__ __forceinline__ double cross_t(double g0, double res, int k, double o, double d) { return (face(g0, res, k) - o) / d; }

// The index, on one axis, of a cell whose slab holds the ray at time t0 (d != 0: near <= t0 <= far by the crossing times
// themselves; d == 0: face(i) <= o <= face(i + 1)).  An estimate from the position, then LOCATE_FIXES corrections by one cell:
// the estimate is off by more only at coordinates so large that a cell is below their rounding.  False: the axis has no such
// cell (d == 0 and o outside the grid).  The index is always in [0, n).
__device__ __forceinline__ bool locate(double g0, double res, int n, double o, double d, double t0, int& idx) {
  const double p = o + t0 * d;
  double e = floor((p - g0) / res);
  e = fmin(fmax(e, 0.0), (double)(n - 1));                    // (a NaN becomes 0)
  int i = (int)e;
  if (d != 0.0) {
    const int s = d > 0.0 ? 1 : -1;
#pragma unroll
    for (int k = 0; k < LOCATE_FIXES; ++k) {
      const double tn = cross_t(g0, res, s > 0 ? i : i + 1, o, d), tf = cross_t(g0, res, s > 0 ? i + 1 : i, o, d);
      const int back = i - s, fwd = i + s;
      if (tn > t0 && back >= 0 && back < n) i = back;
      else if (tf < t0 && fwd >= 0 && fwd < n) i = fwd;
    }
    idx = i;
    return true;
  }
#pragma unroll
  for (int k = 0; k < LOCATE_FIXES; ++k) {
    if (face(g0, res, i) > o && i > 0) i = i - 1;
    else if (face(g0, res, i + 1) < o && i < n - 1) i = i + 1;
  }
  idx = i;
  return face(g0, res, i) <= o && o <= face(g0, res, i + 1);
}

// t_g of the header for the ray o + t d: the smallest t_c over the occupied cells, +inf for a miss or once it is known to be
// at or above rmax.  The inputs are finite.  The walk: near / far are the current cell's slab times per axis; the axis with the
// smaller far time is left first, and the far time left behind is, bit for bit, the near time of the cell entered (the same
// face, the same formula).  Every iteration moves an index by one in a fixed direction, so nx + ny bounds the trip count; the
// counter states it.
__device__ __forceinline__ double cast(const GridArg& M, double ox, double oy, double dx, double dy, double rmax) {
  const double INF = __builtin_inf();
  const int nx = M.nx, ny = M.ny;
  // the grid as one box: where the ray is inside it
  double gnx = -INF, gfx = INF, gny = -INF, gfy = INF;
  if (dx != 0.0) {
    const double a = cross_t(M.x0, M.res, 0, ox, dx), b = cross_t(M.x0, M.res, nx, ox, dx);
    gnx = a < b ? a : b; gfx = a < b ? b : a;
  } else if (!(face(M.x0, M.res, 0) <= ox && ox <= face(M.x0, M.res, nx))) {
    return INF;
  }
  if (dy != 0.0) {
    const double a = cross_t(M.y0, M.res, 0, oy, dy), b = cross_t(M.y0, M.res, ny, oy, dy);
    gny = a < b ? a : b; gfy = a < b ? b : a;
  } else if (!(face(M.y0, M.res, 0) <= oy && oy <= face(M.y0, M.res, ny))) {
    return INF;
  }
  const double gen = gnx > gny ? gnx : gny, glv = gfx < gfy ? gfx : gfy;
  const double t0 = gen > 0.0 ? gen : 0.0;
  if (!(t0 <= glv) || !(t0 < rmax)) return INF;
  int i, j;
  if (!locate(M.x0, M.res, nx, ox, dx, t0, i) || !locate(M.y0, M.res, ny, oy, dy, t0, j)) return INF;
  const int sx = dx > 0.0 ? 1 : (dx < 0.0 ? -1 : 0), sy = dy > 0.0 ? 1 : (dy < 0.0 ? -1 : 0);
  const int fx = sx > 0 ? 1 : 0, fy = sy > 0 ? 1 : 0;          // the far face of cell i is face i + fx
  double nearx = sx != 0 ? cross_t(M.x0, M.res, i + 1 - fx, ox, dx) : -INF;
  double farx = sx != 0 ? cross_t(M.x0, M.res, i + fx, ox, dx) : INF;
  double neary = sy != 0 ? cross_t(M.y0, M.res, j + 1 - fy, oy, dy) : -INF;
  double fary = sy != 0 ? cross_t(M.y0, M.res, j + fy, oy, dy) : INF;
  const int cap = nx + ny + 2;
  for (int it = 0; it < cap; ++it) {                           // here 0 <= i < nx and 0 <= j < ny
    const double enter = nearx > neary ? nearx : neary;
    if (!(enter < rmax)) return INF;
    if (M.cells[(size_t)j * nx + i] != 0) return enter > 0.0 ? enter : 0.0;
    if (farx < fary) {
      i += sx;
      if ((unsigned)i >= (unsigned)nx) return INF;
      nearx = farx;
      farx = cross_t(M.x0, M.res, i + fx, ox, dx);
    } else if (fary < farx) {
      j += sy;
      if ((unsigned)j >= (unsigned)ny) return INF;
      neary = fary;
      fary = cross_t(M.y0, M.res, j + fy, oy, dy);
    } else if (farx == fary) {                                 // through a corner: the two cells beside it are touched at that time
      const double t = farx;
      if (!(t < rmax)) return INF;
      const int i2 = i + sx, j2 = j + sy;
      const bool inx = (unsigned)i2 < (unsigned)nx, iny = (unsigned)j2 < (unsigned)ny;
      const bool side_x = inx && M.cells[(size_t)j * nx + i2] != 0, side_y = iny && M.cells[(size_t)j2 * nx + i] != 0;
      if (side_x || side_y) return t > 0.0 ? t : 0.0;
      if (!inx || !iny || (sx == 0 && sy == 0)) return INF;
      i = i2; j = j2;
      nearx = farx; neary = fary;
      farx = sx != 0 ? cross_t(M.x0, M.res, i + fx, ox, dx) : INF;
      fary = sy != 0 ? cross_t(M.y0, M.res, j + fy, oy, dy) : INF;
    } else {
      return INF;                                              // (a NaN time: not reachable from finite inputs)
    }
  }
  return INF;
}

template <bool NOISE>
__global__ __launch_bounds__(GS_THREADS) void grid_scan_kernel(GridArg M, const npa_scan_params* __restrict__ params,
                                                               const int* __restrict__ n_beams, int beam_stride,
                                                               double* __restrict__ ranges, double* __restrict__ beam_vel,
                                                               int* __restrict__ hit, GridNoise Z) {
  const int b = (int)blockIdx.y;
  int n = n_beams ? n_beams[b] : beam_stride;
  n = n < 0 ? 0 : (n > beam_stride ? beam_stride : n);
  const int i = (int)blockIdx.x * GS_THREADS + (int)threadIdx.x;
  if (i >= n) return;
  const npa_scan_params P = params[b];
  const npa_beam::Sensor S = npa_beam::sensor(P);
  double ang = npa_beam::angle(P, n, i);
  double g_r = 0.0;
  if constexpr (NOISE) {                                        // the statements of world_scan_kernel<true>
    double g_a;
    npa_noise::draws(Z.seed, Z.scene_base + b, i, Z.draw, g_a, g_r);
    const double turn = Z.angle_std * g_a;
    ang = Z.angle_std != 0.0 ? ang + turn : ang;
  }
  double dx, dy;
  npa_beam::direction(S, ang, dx, dy);
  const double rmax = P.range_max;
  double tg = __builtin_inf();
  if (__builtin_isfinite(S.ox) && __builtin_isfinite(S.oy) && __builtin_isfinite(dx) && __builtin_isfinite(dy) &&
      __builtin_isfinite(rmax))
    tg = cast(M, S.ox, S.oy, dx, dy, rmax);
  double g = rmax;
  if (tg < rmax) {
    g = tg;
    if constexpr (NOISE) {
      const double v = tg + Z.std * g_r;
      const double p = (v > 0.0 ? v : 0.0) + 0.0;               // (+ 0: no negative zero)
      g = Z.std != 0.0 ? (p < rmax ? p : rmax) : tg;
    }
  }
  const size_t at = (size_t)b * beam_stride + i;
  if (g < ranges[at]) {                                         // a tie keeps the primitive
    ranges[at] = g;
    if (hit) hit[at] = NPA_HIT_GRID;
    if (beam_vel) {
      beam_vel[(size_t)b * 2 * beam_stride + i] = 0.0;
      beam_vel[(size_t)b * 2 * beam_stride + beam_stride + i] = 0.0;
    }
  }
}

// The robot polygon in the robot frame, by value: edge e runs from (ax, ay)[e] along (dx, dy)[e], counter-clockwise, il = 1 /
// its length.  Entries at or beyond E are not read.
struct ClearanceArg {
  int E;
  double reach;
  double ax[NPA_MAX_E], ay[NPA_MAX_E], dx[NPA_MAX_E], dy[NPA_MAX_E], il[NPA_MAX_E];
};

__device__ __forceinline__ int clamp_index(double v, int n) { return (int)fmin(fmax(v, 0.0), (double)(n - 1)); }

// One wave per robot.  The polygon is brought to the world frame once (every edge loop below is unrolled over NPA_MAX_E with
// compile-time indices: registers, no scratch); the lanes stride over the window's cells.  Squared distances until the end:
// the minimum commutes with the square root.
__global__ __launch_bounds__(GC_THREADS) void grid_clearance_kernel(GridArg M, ClearanceArg K, const double* __restrict__ state,
                                                                    double* __restrict__ clearance) {
  const double INF = __builtin_inf();
  const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
  const double px = state[b * 3 + 0], py = state[b * 3 + 1], th = state[b * 3 + 2];
  if (!(__builtin_isfinite(px) && __builtin_isfinite(py) && __builtin_isfinite(th))) return;     // (the same in every lane)
  const double c = cos(th), s = sin(th);
  double Ax[NPA_MAX_E], Ay[NPA_MAX_E], Dx[NPA_MAX_E], Dy[NPA_MAX_E];
  double xlo = INF, xhi = -INF, ylo = INF, yhi = -INF;
#pragma unroll
  for (int e = 0; e < NPA_MAX_E; ++e) {
    Ax[e] = Ay[e] = Dx[e] = Dy[e] = 0.0;
    if (e < K.E) {
      Ax[e] = (c * K.ax[e] + (-s) * K.ay[e]) + px;
      Ay[e] = (s * K.ax[e] + c * K.ay[e]) + py;
      Dx[e] = c * K.dx[e] + (-s) * K.dy[e];
      Dy[e] = s * K.dx[e] + c * K.dy[e];
      xlo = fmin(xlo, Ax[e]); xhi = fmax(xhi, Ax[e]);
      ylo = fmin(ylo, Ay[e]); yhi = fmax(yhi, Ay[e]);
    }
  }
  // the window, a cell wider on every side than the rule asks for: what it adds is farther than reach
  const int i0 = clamp_index(floor(((xlo - K.reach) - M.x0) / M.res) - 1.0, M.nx);
  const int i1 = clamp_index(floor(((xhi + K.reach) - M.x0) / M.res) + 1.0, M.nx);
  const int j0 = clamp_index(floor(((ylo - K.reach) - M.y0) / M.res) - 1.0, M.ny);
  const int j1 = clamp_index(floor(((yhi + K.reach) - M.y0) / M.res) + 1.0, M.ny);
  const int wn = i1 - i0 + 1, hn = j1 - j0 + 1;                // (>= 1 each; wn * hn <= nx * ny < 2^31)
  const int total = wn * hn;
  // The window's occupied cells are few (a tenth of a typical map) and each costs a few hundred operations, so they are
  // gathered first: every trip the lanes look at 64 cells and queue the occupied ones in LDS, in window order, and a full
  // batch of 64 (at the end: what is left) is measured with every lane busy.  All trip counts and branches are the wave's.
  __shared__ int queue[2 * GC_THREADS];
  double best = INF;
  int queued = 0;
  for (int k0 = 0; k0 < total || queued > 0; k0 += GC_THREADS) {
    if (k0 < total) {
      const int k = k0 + lane;
      const bool occ = k < total && M.cells[(size_t)(j0 + k / wn) * M.nx + (i0 + k % wn)] != 0;
      const unsigned long long m = __ballot(occ);
      const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
      if (occ) queue[queued + before] = k;                     // (queued < 64 here, so the slot is below 128)
      queued += (int)__popcll(m);
      __syncthreads();
      if (queued < GC_THREADS && k0 + GC_THREADS < total) continue;
    }
    const int take = queued < GC_THREADS ? queued : GC_THREADS;
    const int mine = lane < take ? queue[lane] : -1;
    const int carry = GC_THREADS + lane < queued ? queue[GC_THREADS + lane] : -1;
    __syncthreads();
    if (carry >= 0) queue[lane] = carry;
    queued -= take;
    __syncthreads();
    if (mine < 0) continue;
    const int jj = j0 + mine / wn, ii = i0 + mine % wn;
    const double X0 = face(M.x0, M.res, ii), X1 = face(M.x0, M.res, ii + 1);
    const double Y0 = face(M.y0, M.res, jj), Y1 = face(M.y0, M.res, jj + 1);
    bool touch = false;
    double m2 = INF, deep0 = -INF, deep1 = -INF, deep2 = -INF, deep3 = -INF;
#pragma unroll
    for (int e = 0; e < NPA_MAX_E; ++e) {
      if (e < K.E) {
        const double ax = Ax[e], ay = Ay[e], ex = Dx[e], ey = Dy[e], il = K.il[e];
        const double bx = ax + ex, by = ay + ey;
        // the polygon's vertex against the box: inside it, or its distance to it (= to the nearest of its four edges)
        touch = touch || (X0 <= ax && ax <= X1 && Y0 <= ay && ay <= Y1);
        const double qx = fmax(fmax(X0 - ax, ax - X1), 0.0), qy = fmax(fmax(Y0 - ay, ay - Y1), 0.0);
        m2 = fmin(m2, qx * qx + qy * qy);
        // the box's corners (X0,Y0), (X1,Y0), (X1,Y1), (X0,Y1) against edge e: side (outward normal (ey, -ex)) and distance
        const double rx0 = X0 - ax, rx1 = X1 - ax, ry0 = Y0 - ay, ry1 = Y1 - ay;
        const double o0 = ey * rx0 - ex * ry0, o1 = ey * rx1 - ex * ry0, o2 = ey * rx1 - ex * ry1, o3 = ey * rx0 - ex * ry1;
        deep0 = fmax(deep0, o0 * il); deep1 = fmax(deep1, o1 * il); deep2 = fmax(deep2, o2 * il); deep3 = fmax(deep3, o3 * il);
        {
          const double u = fmin(fmax(((rx0 * ex + ry0 * ey) * il) * il, 0.0), 1.0), wx = rx0 - u * ex, wy = ry0 - u * ey;
          m2 = fmin(m2, wx * wx + wy * wy);
        }
        {
          const double u = fmin(fmax(((rx1 * ex + ry0 * ey) * il) * il, 0.0), 1.0), wx = rx1 - u * ex, wy = ry0 - u * ey;
          m2 = fmin(m2, wx * wx + wy * wy);
        }
        {
          const double u = fmin(fmax(((rx1 * ex + ry1 * ey) * il) * il, 0.0), 1.0), wx = rx1 - u * ex, wy = ry1 - u * ey;
          m2 = fmin(m2, wx * wx + wy * wy);
        }
        {
          const double u = fmin(fmax(((rx0 * ex + ry1 * ey) * il) * il, 0.0), 1.0), wx = rx0 - u * ex, wy = ry1 - u * ey;
          m2 = fmin(m2, wx * wx + wy * wy);
        }
        // proper crossing of edge e and a box edge: the box edge's corners on opposite sides of e's line, e's ends on opposite
        // sides of the box edge's line (bottom, right, top, left)
        touch = touch || (o0 * o1 < 0.0 && (ay - Y0) * (by - Y0) < 0.0) || (o1 * o2 < 0.0 && (ax - X1) * (bx - X1) < 0.0) ||
                (o2 * o3 < 0.0 && (ay - Y1) * (by - Y1) < 0.0) || (o3 * o0 < 0.0 && (ax - X0) * (bx - X0) < 0.0);
      }
    }
    touch = touch || deep0 <= 0.0 || deep1 <= 0.0 || deep2 <= 0.0 || deep3 <= 0.0;     // a corner in or on the polygon
    best = fmin(best, touch ? 0.0 : m2);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) best = fmin(best, __shfl_xor(best, m, 64));
  if (lane == 0) {
    const double cg = sqrt(best);
    if (cg <= K.reach && cg < clearance[b]) clearance[b] = cg;   // (above reach: +inf, which lowers nothing)
  }
}

thread_local std::string g_grid_err;
int fail(int code, const std::string& msg) { g_grid_err = msg; return code; }

#define GRID_HIP_TRY(expr)                                                                              \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) return fail(NPA_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
  } while (0)

bool positive(double x) { return x > 0.0 && std::isfinite(x); }
bool level_ok(double x) { return x >= 0.0 && std::isfinite(x); }

// the map's own refusals, shared by the two calls; 0 when it is fine
int check_map(const char* who, const uint8_t* cells, int nx, int ny, double x0, double y0, double res) {
  const std::string w(who);
  if (!cells) return fail(NPA_E_ARG, w + ": cells is null");
  if (nx < 1 || ny < 1) return fail(NPA_E_ARG, w + ": nx and ny must be >= 1");
  if (!std::isfinite(x0) || !std::isfinite(y0)) return fail(NPA_E_ARG, w + ": the origin must be finite");
  if (!positive(res)) return fail(NPA_E_ARG, w + ": res must be positive and finite");
  if ((long long)nx * (long long)ny >= (1LL << 31)) return fail(NPA_E_UNSUPPORTED, w + ": nx * ny must be below 2^31");
  return NPA_OK;
}

}  // namespace

extern "C" const char* npa_grid_last_error(void) { return g_grid_err.c_str(); }

extern "C" int npa_grid_scan(const uint8_t* cells, int nx, int ny, double x0, double y0, double res, int batch,
                             const npa_scan_params* params, const int32_t* n_beams, int beam_stride, double* ranges,
                             double* beam_vel, int32_t* hit, double std, double angle_std, uint64_t seed, int scene_base,
                             int draw, void* stream) {
  if (const int rc = check_map("npa_grid_scan", cells, nx, ny, x0, y0, res)) return rc;
  if (!params || !ranges) return fail(NPA_E_ARG, "npa_grid_scan: params or ranges is null");
  if (batch <= 0 || batch > 65535) return fail(NPA_E_ARG, "npa_grid_scan: batch must be in 1 .. 65535");
  if (beam_stride <= 0) return fail(NPA_E_ARG, "npa_grid_scan: beam_stride must be positive");
  if (!level_ok(std) || !level_ok(angle_std)) return fail(NPA_E_ARG, "npa_grid_scan: std and angle_std must be finite and >= 0");
  if (draw < 0 || scene_base < 0 || scene_base > 0x7fffffff - batch)
    return fail(NPA_E_ARG, "npa_grid_scan: draw and scene_base must be >= 0 (and scene_base + batch an int)");
  const GridArg M = {cells, nx, ny, x0, y0, res};
  GridNoise Z;
  Z.std = std; Z.angle_std = angle_std; Z.seed = seed; Z.scene_base = scene_base; Z.draw = draw;
  const dim3 grid((beam_stride + GS_THREADS - 1) / GS_THREADS, batch);
  if (std != 0.0 || angle_std != 0.0)
    hipLaunchKernelGGL(grid_scan_kernel<true>, grid, dim3(GS_THREADS), 0, (hipStream_t)stream, M, params, n_beams, beam_stride,
                       ranges, beam_vel, hit, Z);
  else
    hipLaunchKernelGGL(grid_scan_kernel<false>, grid, dim3(GS_THREADS), 0, (hipStream_t)stream, M, params, n_beams, beam_stride,
                       ranges, beam_vel, hit, Z);
  GRID_HIP_TRY(hipGetLastError());
  return NPA_OK;
}

extern "C" int npa_grid_clearance(const uint8_t* cells, int nx, int ny, double x0, double y0, double res, int batch,
                                  const double* state, int edge_num, const double* vertices, double reach, double* clearance,
                                  void* stream) {
  if (const int rc = check_map("npa_grid_clearance", cells, nx, ny, x0, y0, res)) return rc;
  if (!state || !vertices || !clearance) return fail(NPA_E_ARG, "npa_grid_clearance: state, vertices or clearance is null");
  if (batch <= 0) return fail(NPA_E_ARG, "npa_grid_clearance: batch must be positive");
  if (!positive(reach)) return fail(NPA_E_ARG, "npa_grid_clearance: reach must be positive and finite");
  if (edge_num < 3 || edge_num > NPA_MAX_E) return fail(NPA_E_UNSUPPORTED, "npa_grid_clearance: edge_num outside [3,NPA_MAX_E]");
  ClearanceArg K = {};
  K.E = edge_num; K.reach = reach;
  for (int e = 0; e < edge_num; ++e) {
    const int f = (e + 1) % edge_num;
    K.ax[e] = vertices[2 * e]; K.ay[e] = vertices[2 * e + 1];
    K.dx[e] = vertices[2 * f] - K.ax[e]; K.dy[e] = vertices[2 * f + 1] - K.ay[e];
    const double len = std::sqrt(K.dx[e] * K.dx[e] + K.dy[e] * K.dy[e]);
    if (!(len > 0.0) || !std::isfinite(len)) return fail(NPA_E_ARG, "npa_grid_clearance: a polygon edge of zero or infinite length");
    K.il[e] = 1.0 / len;
  }
  const GridArg M = {cells, nx, ny, x0, y0, res};
  hipLaunchKernelGGL(grid_clearance_kernel, dim3(batch), dim3(GC_THREADS), 0, (hipStream_t)stream, M, K, state, clearance);
  GRID_HIP_TRY(hipGetLastError());
  return NPA_OK;
}
