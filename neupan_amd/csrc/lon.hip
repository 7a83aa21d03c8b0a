// Training the NRMP adjust parameters inside the device-resident closed loop (gfx950 only): what example/LON/LON_corridor.py does
// on the host between its planner call and the next one, as three launches behind npa_cycle_commit -- and, where groups of
// robots share a parameter row, two more around the Adam step.
//   lon_loss_kernel   stuck bookkeeping, the distance loss and its upstream gradient, the episode's end   LON_corridor.py:10-19, :62-82, :102
//   lon_chain_kernel  the body of the gradient chain through the PAN iterations                           pan.py (_grad_backward_rows)
//   lon_adam_kernel   torch.optim.Adam.step and zero_grad, one parameter row per robot                    LON_corridor.py:41, :94-95, :127
//   lon_reduce_kernel   the gradient rows of a group's robots summed into the group's row, one wave per group, fixed order
//   lon_scatter_kernel  a group's parameter row copied to the rows of its robots
// The launch sequence of one cycle (neupan_amd.lon.LonLoop), on one stream:
//   npa_cycle_progress -> npa_world_scan -> npa_scan_to_points -> npa_nominal_ref_states
//   -> npa_forward_begin, K x { cur_s, cur_u -> snapshot k; npa_forward_iter(k); mu, lam, pts, count -> snapshot k }, npa_forward_end
//   -> npa_cycle_act (override_row = the loop's override buffer) -> npa_world_step -> npa_cycle_commit
//   -> npa_lon_loss
//   -> for k = K-1 .. first: npa_nrmp_backward(snapshot k, gs, gu, gd) -> npa_lon_chain(k)
//   -> npa_lon_adam(t)                                                 (one row per robot), or
//   -> npa_lon_reduce -> npa_lon_adam(t) on the G group rows -> npa_lon_scatter        (rows shared by groups of robots)
// One thread per robot (lon_reduce_kernel: one wave per group), no workspace, no atomics, no device-side counter; handle-free and stream-ordered like cycle.hip.  Every
// per-robot decision is a select and every loop bound a launch argument.  Every arithmetic statement is ONE IEEE operation in
// a stated order (contraction is off for the whole file), so numpy float32 / float64 restates the kernels bit for bit and a
// host-paced loop that calls the same exports gives the same bits.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "handle.h"

namespace {

constexpr int LON_THREADS = 64;
constexpr int LON_COLS = 7;        // q_s[0..2], p_u, eta, d_max, d_min: the trainable columns of a [8] parameter row

struct LonBounds { float lo[8], hi[8]; };

__global__ __launch_bounds__(LON_THREADS) void lon_loss_kernel(
    int batch, int T, int cycle, const double* __restrict__ state, double* __restrict__ last_xy, const float* __restrict__ opt_d,
    const float* __restrict__ min_distance, const uint8_t* __restrict__ stop, const int* __restrict__ arrived,
    const int* __restrict__ collided, float threshold, double stuck_threshold, int stuck_patience, float weight, float offset,
    int* __restrict__ stuck_count, int* __restrict__ ended, int* __restrict__ active, float* __restrict__ loss,
    float* __restrict__ grad_s, float* __restrict__ grad_u, float* __restrict__ grad_d, float* __restrict__ override_row,
    float* __restrict__ log_loss, uint8_t* __restrict__ log_stuck, uint8_t* __restrict__ log_ended) {
  const int b = blockIdx.x * LON_THREADS + threadIdx.x;
  if (b >= batch) return;
  const bool was = ended[b] != 0;
  const double x = state[b * 3 + 0], y = state[b * 3 + 1];
  const double dx = x - last_xy[b * 2 + 0], dy = y - last_xy[b * 2 + 1];
  const double disp = sqrt(dx * dx + dy * dy);                       // LON_corridor.py:67
  const int count0 = stuck_count[b];
  const int count = was ? count0 : count0 + (disp < stuck_threshold ? 1 : 0);      // :69-70 (cumulative over the episode)
  const bool stuck = count > stuck_patience;                         // :72-75
  const float* d = opt_d + (size_t)b * T;
  float S = 0.f;
  for (int t = 0; t < T; ++t) S = S + d[t];                          // torch.sum(distance), first to last
  const bool hit = min_distance[b] <= threshold;                     // :12 (the collision branch wins)
  const bool fire_hit = !was && hit, fire_stuck = !was && !hit && stuck;
  const float l_hit = weight * (offset - S), l_stuck = weight * (offset + S);      // :13, :15, :82
  const float l = fire_hit ? l_hit : (fire_stuck ? l_stuck : 0.f);
  const float g = fire_hit ? -weight : (fire_stuck ? weight : 0.f);
  float* gs = grad_s + (size_t)b * 3 * (T + 1);
  float* gu = grad_u + (size_t)b * 2 * T;
  float* gd = grad_d + (size_t)b * T;
  for (int i = 0; i < 3 * (T + 1); ++i) gs[i] = 0.f;
  for (int i = 0; i < 2 * T; ++i) gu[i] = 0.f;
  for (int t = 0; t < T; ++t) gd[t] = g;
  const bool end_now = arrived[b] != 0 || collided[b] != 0 || stop[b] != 0 || stuck;          // :102
  const bool end = was || end_now;
  stuck_count[b] = count;
  ended[b] = end ? 1 : 0;
  active[b] = was ? 0 : 1;
  loss[b] = l;
  const float o0 = override_row[b * 2 + 0], o1 = override_row[b * 2 + 1];
  override_row[b * 2 + 0] = end ? 0.f : o0;                          // an ended robot stands still from the next cycle on
  override_row[b * 2 + 1] = end ? 0.f : o1;
  last_xy[b * 2 + 0] = x;
  last_xy[b * 2 + 1] = y;
  const size_t row = (size_t)cycle * batch + b;
  if (log_loss) log_loss[row] = l;
  if (log_stuck) log_stuck[row] = stuck ? 1 : 0;
  if (log_ended) log_ended[row] = end ? 1 : 0;
}

__global__ __launch_bounds__(LON_THREADS) void lon_chain_kernel(
    int batch, int T, int k, const int* __restrict__ iters, const float* __restrict__ grad_theta,
    const float* __restrict__ grad_nom_s, double* __restrict__ tot, float* __restrict__ gs, float* __restrict__ gu,
    float* __restrict__ gd, int* __restrict__ bad) {
  const int b = blockIdx.x * LON_THREADS + threadIdx.x;
  if (b >= batch) return;
  const bool ran = iters[b] > k;                 // a robot whose stop test ended the PAN loop earlier skipped this solve
  const float* gt = grad_theta + (size_t)b * 8;
  double* tb = tot + (size_t)b * 8;
  for (int c = 0; c < LON_COLS; ++c) {
    const double old = tb[c], sum = old + (double)gt[c];
    tb[c] = ran ? sum : old;
  }
  const float* gn = grad_nom_s + (size_t)b * 3 * (T + 1);
  float* s = gs + (size_t)b * 3 * (T + 1);
  float* u = gu + (size_t)b * 2 * T;
  float* d = gd + (size_t)b * T;
  for (int i = 0; i < 3 * (T + 1); ++i) { const float old = s[i], nw = gn[i]; s[i] = ran ? nw : old; }
  for (int i = 0; i < 2 * T; ++i) { const float old = u[i]; u[i] = ran ? 0.f : old; }
  for (int t = 0; t < T; ++t) { const float old = d[t]; d[t] = ran ? 0.f : old; }
  const int nb = bad[b];
  bad[b] = (ran && gt[7] != 0.f) ? nb + 1 : nb;                      // the solver status column: 0 = converged
}

__global__ __launch_bounds__(LON_THREADS) void lon_adam_kernel(
    int batch, int mask, int accumulate, double* __restrict__ tot, float* __restrict__ gacc, float* __restrict__ m,
    float* __restrict__ v, float* __restrict__ theta, const int* __restrict__ active, float b1, float omb1, float b2, float omb2,
    float step_size, float bc2_sqrt, float eps, LonBounds bounds, int* __restrict__ skipped) {
  const int b = blockIdx.x * LON_THREADS + threadIdx.x;
  if (b >= batch) return;
  const size_t r = (size_t)b * 8;
  bool finite = true;
#pragma unroll
  for (int c = 0; c < LON_COLS; ++c) {                               // opt.zero_grad runs once per episode: .grad accumulates
    const float g32 = (float)tot[r + c];
    const float old = gacc[r + c];
    const float sum = old + g32;
    const float g = accumulate ? sum : g32;
    gacc[r + c] = g;
    tot[r + c] = 0.0;
    const bool in_mask = ((mask >> c) & 1) != 0;
    finite = finite && (!in_mask || __builtin_isfinite(g));
  }
  const bool on = active[b] != 0;
  const bool step = on && finite;
  const int ns = skipped[b];
  skipped[b] = (on && !finite) ? ns + 1 : ns;
#pragma unroll
  for (int c = 0; c < LON_COLS; ++c) {
    if (((mask >> c) & 1) == 0) continue;                            // (uniform: the mask is a launch argument)
    const float g = gacc[r + c];
    const float m0 = m[r + c], v0 = v[r + c], th0 = theta[r + c];
    const float t1 = b1 * m0, t2 = omb1 * g;
    const float m1 = t1 + t2;                                        // m = b1 m + (1 - b1) g
    const float t3 = b2 * v0, t4 = omb2 * g, t5 = t4 * g;
    const float v1 = t3 + t5;                                        // v = b2 v + ((1 - b2) g) g
    // (the correctly rounded sqrtf: the double root of a float rounds to it, 53 >= 2 * 24 + 2 bits -- the device's own sqrtf
    // is the 1 ulp instruction)
    const float sq = (float)sqrt((double)v1), q = sq / bc2_sqrt;
    const float denom = q + eps;
    const float ratio = m1 / denom, upd = step_size * ratio;
    const float th1 = th0 - upd;                                     // theta -= step_size (m / denom)
    const float th2 = fminf(fmaxf(th1, bounds.lo[c]), bounds.hi[c]);
    m[r + c] = step ? m1 : m0;
    v[r + c] = step ? v1 : v0;
    theta[r + c] = step ? th2 : th0;
  }
}

// One wave per group: lane l holds column c = l & 7 of slot s = l >> 3, so the 64-byte tot row of a robot is one load of 8
// lanes.  Slot s sums the members s, s + 8, s + 16, ... in that order (the trip count ceil(n / 8) is the same for the whole wave:
// the offsets are read through readfirstlane), then slots 4..7 are added to 0..3, 2..3 to 0..1, 1 to 0, the lower slot on the
// left.  A lane past the end of the group reads the last member again and adds +0.0.  Column 7 carries the loss.
__global__ __launch_bounds__(LON_THREADS) void lon_reduce_kernel(
    int mask, int mean, const int* __restrict__ group_first, const int* __restrict__ group_members, double* __restrict__ tot,
    const int* __restrict__ active, const float* __restrict__ loss, double* __restrict__ gtot, int* __restrict__ gactive,
    int* __restrict__ n_used, int* __restrict__ dropped, double* __restrict__ gloss) {
  const int g = blockIdx.x;
  const int lane = threadIdx.x, c = lane & 7, s = lane >> 3;
  const int first = __builtin_amdgcn_readfirstlane(group_first[g]);
  const int n = __builtin_amdgcn_readfirstlane(group_first[g + 1]) - first;
  const int trips = (n + 7) >> 3;
  const bool in_mask = ((mask >> c) & 1) != 0;                       // (bit 7 is never set: the loss column always passes)
  const bool has_loss = loss != nullptr;                             // (uniform: a launch argument)
  double a = 0.0;
  int used = 0, drop = 0;
  for (int i = 0; i < trips; ++i) {
    const int j = i * 8 + s;
    const bool in = j < n;
    const int b = group_members[first + (in ? j : n - 1)];
    const size_t r = (size_t)b * 8 + c;
    const double t = tot[r];
    const bool on = active[b] != 0;
    const float lv = has_loss ? loss[b] : 0.f;
    const bool ok = !in_mask || __builtin_isfinite((float)t);       // what npa_lon_adam would see of this entry
    const unsigned long long oks = __ballot(ok);
    const bool fin = ((oks >> (s * 8)) & 0xffull) == 0xffull;        // ... of the whole row
    const bool use = in && on && fin;
    const double xg = use ? t : 0.0;
    const double xl = (in && on && has_loss) ? (double)lv : 0.0;
    const double x = c == 7 ? xl : xg;
    a = a + x;
    used += __popcll(__ballot(use && c == 0));
    drop += __popcll(__ballot(in && on && !fin && c == 0));
    tot[r] = c == 7 ? t : 0.0;                                       // cleared behind the read; column 7 keeps its bits
  }
  a = a + __shfl_down(a, 32);
  a = a + __shfl_down(a, 16);
  a = a + __shfl_down(a, 8);
  const double q = a / (double)(used > 0 ? used : 1);
  const double out = (mean != 0 && used > 0) ? q : a;
  if (lane < LON_COLS) gtot[(size_t)g * 8 + lane] = out;
  if (lane == 7 && gloss) gloss[g] = a;
  if (lane == 0) {
    gactive[g] = used > 0 ? 1 : 0;
    n_used[g] = used;
    dropped[g] = dropped[g] + drop;
  }
}

__global__ __launch_bounds__(LON_THREADS) void lon_scatter_kernel(
    int batch, int groups, const int* __restrict__ group_of, const float* __restrict__ group_theta, float* __restrict__ theta) {
  const int b = blockIdx.x * LON_THREADS + threadIdx.x;
  if (b >= batch) return;
  const int g = group_of[b];
  const bool member = g >= 0 && g < groups;
  const float* src = group_theta + (size_t)(member ? g : 0) * 8;
  float* dst = theta + (size_t)b * 8;
#pragma unroll
  for (int c = 0; c < LON_COLS; ++c) {
    const float old = dst[c], nw = src[c];
    dst[c] = member ? nw : old;
  }
}

}  // namespace

extern "C" int npa_lon_loss(int batch, int receding, int cycle, const double* state, double* last_xy, const float* opt_d,
                            const float* min_distance, const uint8_t* stop, const int32_t* arrived, const int32_t* collided,
                            float collision_threshold, double stuck_threshold, int stuck_patience, float loss_weight,
                            float loss_offset, int32_t* stuck_count, int32_t* ended, int32_t* active, float* loss,
                            float* grad_s, float* grad_u, float* grad_d, float* override_row, float* log_loss,
                            uint8_t* log_stuck, uint8_t* log_ended, void* stream) {
  if (batch < 1 || cycle < 0 || !state || !last_xy || !opt_d || !min_distance || !stop || !arrived || !collided || !stuck_count ||
      !ended || !active || !loss || !grad_s || !grad_u || !grad_d || !override_row)
    return fail(NPA_E_ARG, "npa_lon_loss: bad argument");
  if (receding < 1 || receding > NPA_MAX_T) return fail(NPA_E_ARG, "npa_lon_loss: receding outside [1,NPA_MAX_T]");
  hipLaunchKernelGGL(lon_loss_kernel, dim3((batch + LON_THREADS - 1) / LON_THREADS), dim3(LON_THREADS), 0, (hipStream_t)stream,
                     batch, receding, cycle, state, last_xy, opt_d, min_distance, stop, arrived, collided, collision_threshold,
                     stuck_threshold, stuck_patience, loss_weight, loss_offset, stuck_count, ended, active, loss, grad_s, grad_u,
                     grad_d, override_row, log_loss, log_stuck, log_ended);
  HIP_TRY(hipGetLastError());
  return NPA_OK;
}

extern "C" int npa_lon_chain(int batch, int receding, int k, const int32_t* iters, const float* grad_theta,
                             const float* grad_nom_s, double* tot, float* grad_s, float* grad_u, float* grad_d, int32_t* bad,
                             void* stream) {
  if (batch < 1 || k < 0 || !iters || !grad_theta || !grad_nom_s || !tot || !grad_s || !grad_u || !grad_d || !bad)
    return fail(NPA_E_ARG, "npa_lon_chain: bad argument");
  if (receding < 1 || receding > NPA_MAX_T) return fail(NPA_E_ARG, "npa_lon_chain: receding outside [1,NPA_MAX_T]");
  hipLaunchKernelGGL(lon_chain_kernel, dim3((batch + LON_THREADS - 1) / LON_THREADS), dim3(LON_THREADS), 0, (hipStream_t)stream,
                     batch, receding, k, iters, grad_theta, grad_nom_s, tot, grad_s, grad_u, grad_d, bad);
  HIP_TRY(hipGetLastError());
  return NPA_OK;
}

extern "C" int npa_lon_adam(int batch, int column_mask, int accumulate, double* tot, float* gacc, float* m, float* v,
                            float* theta, const int32_t* active, float beta1, float one_minus_beta1, float beta2,
                            float one_minus_beta2, float step_size, float bc2_sqrt, float eps, const float* lo, const float* hi,
                            int32_t* skipped, void* stream) {
  if (batch < 1 || !tot || !gacc || !m || !v || !theta || !active || !skipped) return fail(NPA_E_ARG, "npa_lon_adam: bad argument");
  if (column_mask < 0 || column_mask > 0x7f) return fail(NPA_E_ARG, "npa_lon_adam: the column mask has bits above 6");
  LonBounds bounds;
  for (int c = 0; c < 8; ++c) {
    bounds.lo[c] = lo ? lo[c] : -INFINITY;
    bounds.hi[c] = hi ? hi[c] : INFINITY;
  }
  hipLaunchKernelGGL(lon_adam_kernel, dim3((batch + LON_THREADS - 1) / LON_THREADS), dim3(LON_THREADS), 0, (hipStream_t)stream,
                     batch, column_mask, accumulate, tot, gacc, m, v, theta, active, beta1, one_minus_beta1, beta2,
                     one_minus_beta2, step_size, bc2_sqrt, eps, bounds, skipped);
  HIP_TRY(hipGetLastError());
  return NPA_OK;
}

extern "C" int npa_lon_reduce(int batch, int groups, int column_mask, int mean, const int32_t* group_first,
                              const int32_t* group_members, double* tot, const int32_t* active, const float* loss, double* gtot,
                              int32_t* gactive, int32_t* n_used, int32_t* dropped, double* gloss, void* stream) {
  if (batch < 1 || groups < 1 || !group_first || !group_members || !tot || !active || !gtot || !gactive || !n_used || !dropped)
    return fail(NPA_E_ARG, "npa_lon_reduce: bad argument");
  if (column_mask < 0 || column_mask > 0x7f) return fail(NPA_E_ARG, "npa_lon_reduce: the column mask has bits above 6");
  hipLaunchKernelGGL(lon_reduce_kernel, dim3(groups), dim3(LON_THREADS), 0, (hipStream_t)stream, column_mask, mean, group_first,
                     group_members, tot, active, loss, gtot, gactive, n_used, dropped, gloss);
  HIP_TRY(hipGetLastError());
  return NPA_OK;
}

extern "C" int npa_lon_scatter(int batch, int groups, const int32_t* group_of, const float* group_theta, float* theta,
                               void* stream) {
  if (batch < 1 || groups < 1 || !group_of || !group_theta || !theta) return fail(NPA_E_ARG, "npa_lon_scatter: bad argument");
  hipLaunchKernelGGL(lon_scatter_kernel, dim3((batch + LON_THREADS - 1) / LON_THREADS), dim3(LON_THREADS), 0, (hipStream_t)stream,
                     batch, groups, group_of, group_theta, theta);
  HIP_TRY(hipGetLastError());
  return NPA_OK;
}
