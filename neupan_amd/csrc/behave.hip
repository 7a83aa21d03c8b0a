// Reactive obstacles of the lidar world (gfx950 only): the agents of a world choose their velocity every cycle by the sampled
// penalty of van den Berg, Lin, Manocha, "Reciprocal Velocity Obstacles for Real-Time Multi-Agent Navigation", ICRA 2008:
// cost(v') = w / tc(v') + |v_pref - v'| over a table of candidate velocities.  include/neupan_amd.h is the specification.
//   behave_choose_kernel   one wave per agent: neighbours culled and compacted into LDS, candidates cast against the list, a
//                          wave reduction of (cost, index); writes the agent's row only
//   behave_commit_kernel   one thread per primitive: an owned primitive takes its agent's chosen velocity
// Handle-free, stream-ordered, no workspace, no atomics.  All arithmetic is float64 in a fixed operation order: no FMA
// contraction in this file (a (candidate, neighbour) pair must give the same tc whichever chunk or call it is met in).
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "handle.h"

namespace {

constexpr int BH_THREADS = 64;             // one wave: lanes are neighbours in phase 1 and candidates in phase 2
constexpr int BH_CAP = BH_THREADS;         // capacity of the LDS list: a chunk of BH_CAP neighbours cannot overflow it
constexpr int BH_MAX_CAND = 512;           // candidates of one agent (their tc_min lives in LDS between the chunks)
constexpr double BH_CULL_SLACK = 1.0 + 1e-9;   // on squared distances: rounding of the cull test must not drop a tc <= horizon
constexpr int AG_W = NPA_AGENT_DOUBLES, AGI_W = NPA_AGENT_INTS;
constexpr int BC_THREADS = 256;

struct BehaveK {
  int batch, n_worlds, c_stride, s_stride, a_stride, seg_limit, n_dir, n_speed, n_cand, world_base;
  unsigned long long seed;
  double weight, horizon, share, inv_share, lo[2], hi[2], robot_radius, dt;
};

// the wander generator (the header states it): four rounds of the splitmix64 finaliser over seed, world, agent, draw, coordinate
__device__ __forceinline__ unsigned long long bh_mix(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ double bh_uniform(unsigned long long seed, unsigned world, unsigned agent, unsigned draw, unsigned coord) {
  unsigned long long z = bh_mix(seed + world);
  z = bh_mix(z + agent);
  z = bh_mix(z + draw);
  z = bh_mix(z + coord);
  return (double)(z >> 11) * 0x1.0p-53;
}

// an agent row is used only when its primitives exist: a circle agent owns one circle, a polygon agent a run of segments
__device__ __forceinline__ bool agent_ok(int first, int count, int nC, int nS) {
  return first >= 0 && count >= 1 && (first < nC ? count == 1 : (long long)first - nC + count <= (long long)nS);
}

struct Lists {
  double a[12][BH_CAP];
  double tc[BH_MAX_CAND];
};

// slot of this lane's survivor in the wave's list (index order) and the number of survivors
__device__ __forceinline__ int wave_slot(bool keep, int& total) {
  const unsigned long long m = __ballot(keep);
  total = __builtin_amdgcn_readfirstlane(__popcll(m));
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
}

struct Cand {
  double vpx, vpy, vcx, vcy, vmax;
  int n_dir, n_speed, n_cand;
  const double* dirs;
  __device__ __forceinline__ void get(int i, double& vx, double& vy) const {
    const int g = i >= 3 ? i - 3 : 0;
    const int j = n_dir > 0 ? g / n_dir : 0, k = g - j * n_dir;
    const double s = (vmax * (double)(j + 1)) / (double)(n_speed > 0 ? n_speed : 1);
    const double ux = n_dir > 0 ? dirs[2 * k] : 0.0, uy = n_dir > 0 ? dirs[2 * k + 1] : 0.0;
    const double gx = s * ux, gy = s * uy;
    vx = i == 0 ? 0.0 : (i == 1 ? vpx : (i == 2 ? vcx : gx));
    vy = i == 0 ? 0.0 : (i == 1 ? vpy : (i == 2 ? vcy : gy));
  }
};

// time at which the ray from the origin with velocity (ux, uy) meets the disc of centre (cx, cy), c2 = |c|^2 - rho^2; +inf: none
__device__ __forceinline__ double disc_tc(double cx, double cy, double c2, double ux, double uy) {
  const double b = cx * ux + cy * uy;
  const double u2 = ux * ux + uy * uy;
  const bool touching = c2 <= 0.0;
  const double disc = b * b - u2 * c2;
  const bool hit = b > 0.0 && (touching || disc >= 0.0);
  const double sq = sqrt(disc > 0.0 ? disc : 0.0);
  const double den = hit && !touching ? b + sq : 1.0;
  const double t = touching ? 0.0 : c2 / den;                  // the near root, without its cancellation
  return hit ? t : __builtin_inf();
}

// the same for the segment from (wx, wy) along (ex, ey): the scan kernel's sign-corrected validity test, then one division
__device__ __forceinline__ double seg_tc(double wx, double wy, double ex, double ey, double ux, double uy) {
  const double wxe = wx * ey - wy * ex;
  const double det = ux * ey - uy * ex;
  const double un = wx * uy - wy * ux;
  const bool neg = det < 0.0;
  const double ad = neg ? -det : det, tn = neg ? -wxe : wxe, us = neg ? -un : un;
  const bool valid = ad > 0.0 && tn >= 0.0 && us >= 0.0 && us <= ad;
  const double t = tn / (valid ? ad : 1.0) + 0.0;
  return valid ? t : __builtin_inf();
}

// phase 2 over a list of discs: a[0..1] = centre - p, a[2] = c2, a[3..4] = apex, a[5] = 1 / alpha
__device__ __forceinline__ void cast_discs(Lists& S, const Cand& Q, int cnt, int lane, double horizon) {
  #pragma unroll 1
  for (int t0 = 0; t0 < Q.n_cand; t0 += BH_THREADS) {
    const int i = t0 + lane;
    const bool live = i < Q.n_cand;
    double vx, vy;
    Q.get(live ? i : 0, vx, vy);
    double tc = S.tc[live ? i : 0];
    #pragma unroll 1
    for (int k = 0; k < cnt; ++k) {
      const double inv = S.a[5][k];
      const double ux = (vx - S.a[3][k]) * inv, uy = (vy - S.a[4][k]) * inv;
      const double t = disc_tc(S.a[0][k], S.a[1][k], S.a[2][k], ux, uy);
      tc = (t <= horizon && t < tc) ? t : tc;
    }
    if (live) S.tc[i] = tc;
  }
}

// phase 2 over a list of capsules (alpha = 1): a[0..1] = a - p, a[2..3] = b - p, a[4..5] = b - a, a[6..7] = R_A n,
// a[8] / a[9] = c2 of the end discs, a[10..11] = apex
__device__ __forceinline__ void cast_capsules(Lists& S, const Cand& Q, int cnt, int lane, double horizon) {
  #pragma unroll 1
  for (int t0 = 0; t0 < Q.n_cand; t0 += BH_THREADS) {
    const int i = t0 + lane;
    const bool live = i < Q.n_cand;
    double vx, vy;
    Q.get(live ? i : 0, vx, vy);
    double tc = S.tc[live ? i : 0];
    #pragma unroll 1
    for (int k = 0; k < cnt; ++k) {
      const double ux = vx - S.a[10][k], uy = vy - S.a[11][k];
      const double wx = S.a[0][k], wy = S.a[1][k], ex = S.a[4][k], ey = S.a[5][k], nx = S.a[6][k], ny = S.a[7][k];
      double t = disc_tc(wx, wy, S.a[8][k], ux, uy);
      t = fmin(t, disc_tc(S.a[2][k], S.a[3][k], S.a[9][k], ux, uy));
      t = fmin(t, seg_tc(wx + nx, wy + ny, ex, ey, ux, uy));
      t = fmin(t, seg_tc(wx - nx, wy - ny, ex, ey, ux, uy));
      tc = (t <= horizon && t < tc) ? t : tc;
    }
    if (live) S.tc[i] = tc;
  }
}

// One wave (= one workgroup) per agent row.  Every loop is wave-uniform; what depends on the lane is a select.
__global__ __launch_bounds__(BH_THREADS) void behave_choose_kernel(
    BehaveK K, const double* __restrict__ circles, const double* __restrict__ segments, const int* __restrict__ n_circles,
    const int* __restrict__ n_segments, double* agents, int* agent_idx, const int* __restrict__ n_agents,
    const double* __restrict__ state, const double* __restrict__ prev_state, const double* __restrict__ dirs) {
  __shared__ Lists S;
  const int lane = (int)threadIdx.x;
  const int w = (int)(blockIdx.x / (unsigned)K.a_stride), a = (int)(blockIdx.x % (unsigned)K.a_stride);
  int nA = n_agents[w];
  nA = nA < 0 ? 0 : (nA > K.a_stride ? K.a_stride : nA);
  if (a >= nA) return;                                         // (the same in every lane)
  int nC = K.c_stride > 0 ? n_circles[w] : 0, nS = K.s_stride > 0 ? n_segments[w] : 0;
  nC = nC < 0 ? 0 : (nC > K.c_stride ? K.c_stride : nC);
  nS = nS < 0 ? 0 : (nS > K.s_stride ? K.s_stride : nS);
  const double* cw = circles + (size_t)w * K.c_stride * 6;
  const double* sw = segments + (size_t)w * K.s_stride * 6;
  double* aw = agents + (size_t)w * K.a_stride * AG_W;
  int* iw = agent_idx + (size_t)w * K.a_stride * AGI_W;
  const int first = iw[a * AGI_W + 0], count = iw[a * AGI_W + 1], wander = iw[a * AGI_W + 2];
  unsigned draws = (unsigned)iw[a * AGI_W + 3];
  if (!agent_ok(first, count, nC, nS)) return;
  double* row = aw + (size_t)a * AG_W;
  const double* anchor = first < nC ? cw + (size_t)first * 6 : sw + (size_t)(first - nC) * 6;
  const double* avel = first < nC ? anchor + 3 : anchor + 4;
  const double px = anchor[0] + row[4], py = anchor[1] + row[5];
  const double RA = row[6], vmax = row[7], thr = row[8];
  const double vax = avel[0], vay = avel[1];

  // ---- step 1: goal and preferred velocity
  double gx = row[0], gy = row[1];
  double dx = gx - px, dy = gy - py;
  double L = sqrt(dx * dx + dy * dy);
  const bool arrived = L <= thr;
  const bool redraw = arrived && wander != 0;
  if (redraw) {                                                // (uniform)
    const unsigned id = (unsigned)first, wid = (unsigned)(K.world_base + w);
    gx = K.lo[0] + (K.hi[0] - K.lo[0]) * bh_uniform(K.seed, wid, id, draws, 0u);
    gy = K.lo[1] + (K.hi[1] - K.lo[1]) * bh_uniform(K.seed, wid, id, draws, 1u);
    draws += 1u;
    dx = gx - px; dy = gy - py;
    L = sqrt(dx * dx + dy * dy);
  }
  const bool rest = (arrived && !redraw) || !(L > 0.0);
  const double s = fmin(vmax, L / K.dt);
  const double il = rest ? 1.0 : L;
  Cand Q;
  Q.vpx = rest ? 0.0 : (dx / il) * s;
  Q.vpy = rest ? 0.0 : (dy / il) * s;
  const double sp = sqrt(vax * vax + vay * vay);
  const bool fast = sp > vmax;
  const double sc = vmax / (fast ? sp : 1.0);
  Q.vcx = fast ? vax * sc : vax;
  Q.vcy = fast ? vay * sc : vay;
  Q.vmax = vmax; Q.n_dir = K.n_dir; Q.n_speed = K.n_speed; Q.n_cand = K.n_cand; Q.dirs = dirs;

  #pragma unroll 1
  for (int i = lane; i < K.n_cand; i += BH_THREADS) S.tc[i] = __builtin_inf();
  __syncthreads();
  const double hz = K.horizon;

  // ---- the discs: circles that no agent owns (alpha = 1), the other agents of the world (alpha = 1/2), the robots (alpha =
  //      robot_share: the world's own robot, or every robot of a shared world), as one index space cut into chunks
  const int nR = K.n_worlds == K.batch ? 1 : K.batch;
  const int r_base = K.n_worlds == K.batch ? w : 0;
  const int nD = nC + nA + nR;
  #pragma unroll 1
  for (int d0 = 0; d0 < nD; d0 += BH_CAP) {
    const int t = d0 + lane;
    const bool is_c = t < nC, is_a = !is_c && t < nC + nA, is_r = !is_c && !is_a && t < nD;
    // a circle
    const int p = is_c ? t : 0;
    bool owned = false;
    const int n_own = d0 < nC ? nA : 0;                         // (uniform: a chunk behind the circles asks nobody)
    #pragma unroll 1
    for (int k = 0; k < n_own; ++k) {
      const int f = iw[k * AGI_W + 0], n = iw[k * AGI_W + 1];
      owned = owned || (agent_ok(f, n, nC, nS) && p >= f && p < f + n);
    }
    const double* qc = cw + (size_t)p * 6;                      // (read only where is_c: nC > 0 then)
    // an agent
    const int kk = is_a ? t - nC : a;
    const int f = iw[kk * AGI_W + 0], n = iw[kk * AGI_W + 1];
    const bool ok_a = is_a && kk != a && agent_ok(f, n, nC, nS);
    const int ff = ok_a ? f : first;
    const double* qa = ff < nC ? cw + (size_t)ff * 6 : sw + (size_t)(ff - nC) * 6;
    const double* qv = ff < nC ? qa + 3 : qa + 4;
    const double* rb = aw + (size_t)kk * AG_W;
    // a robot
    const int b = r_base + (is_r ? t - nC - nA : 0);
    const double sx = state[b * 3 + 0], sy = state[b * 3 + 1];
    const double ox = prev_state ? prev_state[b * 3 + 0] : sx, oy = prev_state ? prev_state[b * 3 + 1] : sy;
    const double vrx = prev_state ? (sx - ox) / K.dt : 0.0, vry = prev_state ? (sy - oy) / K.dt : 0.0;

    const double ccx = is_c ? qc[0] : 0.0, ccy = is_c ? qc[1] : 0.0, ccr = is_c ? qc[2] : 0.0;
    const double cvx = is_c ? qc[3] : 0.0, cvy = is_c ? qc[4] : 0.0;
    const double ctrx = is_c ? ccx : (is_a ? qa[0] + rb[4] : sx), ctry = is_c ? ccy : (is_a ? qa[1] + rb[5] : sy);
    const double rB = is_c ? ccr : (is_a ? rb[6] : K.robot_radius);
    const double vbx = is_c ? cvx : (is_a ? qv[0] : vrx), vby = is_c ? cvy : (is_a ? qv[1] : vry);
    const double al = is_c ? 1.0 : (is_a ? 0.5 : K.share), inv = is_c ? 1.0 : (is_a ? 2.0 : K.inv_share);
    const double cx = ctrx - px, cy = ctry - py, rho = RA + rB;
    const double apx = (1.0 - al) * vax + al * vbx, apy = (1.0 - al) * vay + al * vby;
    const double d2 = cx * cx + cy * cy;
    const double reach = hz * ((vmax + sqrt(apx * apx + apy * apy)) * inv) + rho;
    const bool keep = ((is_c && !owned) || ok_a || is_r) && !(d2 > (reach * reach) * BH_CULL_SLACK);
    int cnt;
    const int slot = wave_slot(keep, cnt);
    if (keep) {
      S.a[0][slot] = cx; S.a[1][slot] = cy; S.a[2][slot] = d2 - rho * rho; S.a[3][slot] = apx; S.a[4][slot] = apy;
      S.a[5][slot] = inv;
    }
    __syncthreads();
    cast_discs(S, Q, cnt, lane, hz);
    __syncthreads();
  }

  // ---- segments that no agent owns, below seg_limit (alpha = 1): capsules of radius R_A
  const int nSv = K.seg_limit >= 0 && K.seg_limit < nS ? K.seg_limit : nS;
  #pragma unroll 1
  for (int s0 = 0; s0 < nSv; s0 += BH_CAP) {
    const int p = s0 + lane;
    const bool have = p < nSv;
    bool owned = false;
    #pragma unroll 1
    for (int k = 0; k < nA; ++k) {
      const int f = iw[k * AGI_W + 0], n = iw[k * AGI_W + 1];
      owned = owned || (agent_ok(f, n, nC, nS) && nC + p >= f && nC + p < f + n);
    }
    const double* q = sw + (size_t)(have ? p : 0) * 6;
    const double wx = q[0] - px, wy = q[1] - py, bx = q[2] - px, by = q[3] - py;
    const double ex = q[2] - q[0], ey = q[3] - q[1];
    const double apx = q[4], apy = q[5];
    const double e2 = ex * ex + ey * ey;
    double u = e2 > 0.0 ? -(wx * ex + wy * ey) / e2 : 0.0;    // the agent's foot point on the segment
    u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
    const double fx = wx + u * ex, fy = wy + u * ey;
    const double reach = hz * (vmax + sqrt(apx * apx + apy * apy)) + RA;
    const bool keep = have && !owned && !(fx * fx + fy * fy > (reach * reach) * BH_CULL_SLACK);
    const double len = sqrt(e2);
    const double nx = e2 > 0.0 ? (ey / len) * RA : 0.0, ny = e2 > 0.0 ? ((-ex) / len) * RA : 0.0;
    int cnt;
    const int slot = wave_slot(keep, cnt);
    if (keep) {
      S.a[0][slot] = wx; S.a[1][slot] = wy; S.a[2][slot] = bx; S.a[3][slot] = by; S.a[4][slot] = ex; S.a[5][slot] = ey;
      S.a[6][slot] = nx; S.a[7][slot] = ny;
      S.a[8][slot] = (wx * wx + wy * wy) - RA * RA; S.a[9][slot] = (bx * bx + by * by) - RA * RA;
      S.a[10][slot] = apx; S.a[11][slot] = apy;
    }
    __syncthreads();
    cast_capsules(S, Q, cnt, lane, hz);
    __syncthreads();
  }

  // ---- cost and choice: the lane's best over its trips (index order), then the wave's; ties to the lowest index
  double bc = __builtin_inf();
  int bi = lane < K.n_cand ? lane : 0x7fffffff;
  #pragma unroll 1
  for (int t0 = 0; t0 < K.n_cand; t0 += BH_THREADS) {
    const int i = t0 + lane;
    const bool live = i < K.n_cand;
    double vx, vy;
    Q.get(live ? i : 0, vx, vy);
    const double tc = S.tc[live ? i : 0];
    const double ddx = Q.vpx - vx, ddy = Q.vpy - vy;
    const double cost = K.weight / tc + sqrt(ddx * ddx + ddy * ddy);
    const bool upd = live && cost < bc;
    bc = upd ? cost : bc;
    bi = upd ? i : bi;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double oc = __shfl_xor(bc, m, 64);
    const int oi = __shfl_xor(bi, m, 64);
    const bool take = oc < bc || (oc == bc && oi < bi);
    bc = take ? oc : bc;
    bi = take ? oi : bi;
  }
  bi = __builtin_amdgcn_readfirstlane(bi);
  double cvx, cvy;
  Q.get(bi, cvx, cvy);
  if (lane == 0) {
    if (redraw) {
      row[0] = gx; row[1] = gy;
      iw[a * AGI_W + 3] = (int)draws;
    }
    row[2] = cvx; row[3] = cvy;
    row[9] = (double)bi;
  }
}

// thread = primitive of a world: the velocity columns of an owned primitive become its agent's chosen velocity (the lowest
// agent row that claims it); no other column and no other primitive is written
__global__ __launch_bounds__(BC_THREADS) void behave_commit_kernel(
    BehaveK K, int blocks_per_world, double* __restrict__ circles, double* __restrict__ segments,
    const int* __restrict__ n_circles, const int* __restrict__ n_segments, const double* __restrict__ agents,
    const int* __restrict__ agent_idx, const int* __restrict__ n_agents) {
  const int w = (int)(blockIdx.x / (unsigned)blocks_per_world);
  const int t = (int)(blockIdx.x % (unsigned)blocks_per_world) * BC_THREADS + (int)threadIdx.x;
  int nA = n_agents[w];
  nA = nA < 0 ? 0 : (nA > K.a_stride ? K.a_stride : nA);
  int nC = K.c_stride > 0 ? n_circles[w] : 0, nS = K.s_stride > 0 ? n_segments[w] : 0;
  nC = nC < 0 ? 0 : (nC > K.c_stride ? K.c_stride : nC);
  nS = nS < 0 ? 0 : (nS > K.s_stride ? K.s_stride : nS);
  const bool is_c = t < K.c_stride;
  const int p = is_c ? t : t - K.c_stride;                     // the row in its array
  const bool have = is_c ? p < nC : p < nS;
  const int idx = is_c ? p : nC + p;                           // the primitive's index in the world's numbering
  const int* iw = agent_idx + (size_t)w * K.a_stride * AGI_W;
  int src = -1;
  #pragma unroll 1
  for (int k = 0; k < nA; ++k) {                               // (uniform: a workgroup lies in one world)
    const int f = iw[k * AGI_W + 0], n = iw[k * AGI_W + 1];
    const bool own = have && agent_ok(f, n, nC, nS) && idx >= f && idx < f + n;
    src = own && src < 0 ? k : src;
  }
  if (src >= 0) {
    const double* row = agents + ((size_t)w * K.a_stride + src) * AG_W;
    double* q = is_c ? circles + ((size_t)w * K.c_stride + p) * 6 + 3 : segments + ((size_t)w * K.s_stride + p) * 6 + 4;
    q[0] = row[2]; q[1] = row[3];
  }
}

}  // namespace

extern "C" int npa_behave_list_capacity(void) { return BH_CAP; }
extern "C" int npa_behave_max_candidates(void) { return BH_MAX_CAND; }

extern "C" int npa_world_behave(int batch, int n_worlds, int c_stride, int s_stride, double* circles, double* segments,
                                const int32_t* n_circles, const int32_t* n_segments, int a_stride, double* agents,
                                int32_t* agent_idx, const int32_t* n_agents, const npa_behave_params* params,
                                const double* state, const double* prev_state, double robot_radius, int seg_limit,
                                int n_dir, const double* dirs, int n_speed, double dt, void* stream) {
  if (batch <= 0 || c_stride < 0 || s_stride < 0 || a_stride <= 0 || !agents || !agent_idx || !n_agents || !params || !state ||
      !n_circles || !n_segments || (c_stride > 0 && !circles) || (s_stride > 0 && !segments))
    return fail(NPA_E_ARG, "npa_world_behave: bad argument");
  if (n_worlds != 1 && n_worlds != batch) return fail(NPA_E_ARG, "npa_world_behave: n_worlds must be 1 or batch");
  if (params->world_base < 0 || params->world_base > 0x7fffffff - n_worlds)
    return fail(NPA_E_ARG, "npa_world_behave: world_base must be >= 0 (and world_base + n_worlds an int)");
  if ((long long)c_stride + (long long)s_stride <= 0) return fail(NPA_E_ARG, "npa_world_behave: strides: agents without primitives");
  if (!(dt > 0.0)) return fail(NPA_E_ARG, "npa_world_behave: dt must be > 0");
  if (!(params->weight > 0.0)) return fail(NPA_E_ARG, "npa_world_behave: weight must be > 0");
  if (!(params->horizon > 0.0)) return fail(NPA_E_ARG, "npa_world_behave: horizon must be > 0");
  if (!(params->robot_share > 0.0 && params->robot_share <= 1.0))
    return fail(NPA_E_ARG, "npa_world_behave: robot_share outside (0, 1]");
  if (!(params->range_low[0] <= params->range_high[0] && params->range_low[1] <= params->range_high[1]))
    return fail(NPA_E_ARG, "npa_world_behave: range_low above range_high");
  if (!(robot_radius >= 0.0)) return fail(NPA_E_ARG, "npa_world_behave: robot_radius must be >= 0");
  if (n_dir < 0 || n_speed < 0 || (n_dir > 0 && n_speed > 0 && !dirs))
    return fail(NPA_E_ARG, "npa_world_behave: bad candidate grid");
  const long long grid = (n_dir > 0 && n_speed > 0) ? (long long)n_dir * n_speed : 0;
  if (3 + grid > BH_MAX_CAND) return fail(NPA_E_ARG, "npa_world_behave: more candidates than npa_behave_max_candidates()");
  if (seg_limit > s_stride) return fail(NPA_E_ARG, "npa_world_behave: strides: seg_limit beyond s_stride");
  const long long rows = (long long)n_worlds * a_stride;
  const long long per_world = ((long long)c_stride + s_stride + BC_THREADS - 1) / BC_THREADS;
  if (rows > 0x7fffffffLL || per_world * n_worlds > 0x7fffffffLL)
    return fail(NPA_E_ARG, "npa_world_behave: strides: world too large");
  BehaveK K = {};
  K.batch = batch; K.n_worlds = n_worlds; K.c_stride = c_stride; K.s_stride = s_stride; K.a_stride = a_stride;
  K.seg_limit = seg_limit < 0 ? -1 : seg_limit;
  K.n_dir = grid > 0 ? n_dir : 0; K.n_speed = grid > 0 ? n_speed : 0; K.n_cand = 3 + (int)grid;
  K.world_base = params->world_base; K.seed = params->seed;
  K.weight = params->weight; K.horizon = params->horizon; K.share = params->robot_share; K.inv_share = 1.0 / params->robot_share;
  #pragma unroll 1
  for (int k = 0; k < 2; ++k) { K.lo[k] = params->range_low[k]; K.hi[k] = params->range_high[k]; }
  K.robot_radius = robot_radius; K.dt = dt;
  hipLaunchKernelGGL(behave_choose_kernel, dim3((unsigned)rows), dim3(BH_THREADS), 0, (hipStream_t)stream, K, circles, segments,
                     n_circles, n_segments, agents, agent_idx, n_agents, state, prev_state, dirs);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(behave_commit_kernel, dim3((unsigned)(per_world * n_worlds)), dim3(BC_THREADS), 0, (hipStream_t)stream, K,
                     (int)per_world, circles, segments, n_circles, n_segments, agents, agent_idx, n_agents);
  HIP_TRY(hipGetLastError());
  return NPA_OK;
}
