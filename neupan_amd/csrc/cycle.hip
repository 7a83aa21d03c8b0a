// The bookkeeping between the kernels of a closed-loop control cycle, on the device (gfx950 only):
//   cycle_switch_kernel  curve switching and the arrival latch behind progress_kernel   initial_path.py:247-315
//   cycle_act_kernel     warm start, stop test, action, scripted override, freeze       neupan.py:137, :150-164
//   cycle_commit_kernel  the collision latch and the cycle's log rows behind the plant step
//   curve_wave_kernel    an arrived robot's next goal: a new curve into its region of the table       neupan.py:288-294, :314-318
//                        (and, for npa_curve_batch, plain curves: csrc/curves.hip)
//   route_wave_kernel    curve_wave_kernel's routed sibling: the next goal's path down its goal field, `line` curves between the
//                        turns of the chain (npa_cycle_retask_routed; for npa_route_curve_batch, plain paths: csrc/curves.hip)
//   route_sweep_kernel   not part of the cycle: one relaxation sweep of the goal fields behind npa_route_relax (csrc/curves.hip),
//                        here because this unit has device code and the product library a size limit
// One thread per robot (curve_wave_kernel, route_wave_kernel: one wave), no workspace, no atomics; handle-free and stream-ordered like frontend.hip.  Every per-robot decision
// is a select and every loop bound is a launch argument: the kernels only choose and copy, so a loop built from them gives
// the bits of the host-paced loop (FleetPlanner.forward + run_closed_loop) whose rules they restate.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"
#include "curves.h"

namespace {

constexpr int CY_THREADS = 64;

// FleetPlanner.forward's rule for a robot whose progress reports arrival and that is not latched: on its last curve it starts
// over (`loop`) or latches, else it moves to its next curve; a robot that moves starts the new curve at point 0.  The pose
// goes into the `state` field of the two parameter blocks the scans of this cycle read.
__global__ __launch_bounds__(CY_THREADS) void cycle_switch_kernel(
    int batch, int loop, const double* __restrict__ state, const int* __restrict__ curve_arrived,
    const int* __restrict__ curve_off, const int* __restrict__ curve_len, const int* __restrict__ robot_first,
    int* __restrict__ curve_index, int* __restrict__ cur_off, int* __restrict__ cur_len, int* __restrict__ point_index,
    int* __restrict__ arrived, npa_scan_params* __restrict__ par_a, npa_scan_params* __restrict__ par_b) {
  const int b = blockIdx.x * CY_THREADS + threadIdx.x;
  if (b >= batch) return;
  const int first = robot_first[b], count = robot_first[b + 1] - first;
  const int ci = curve_index[b], latched = arrived[b];
  const bool now = curve_arrived[b] != 0 && latched == 0;
  const bool last = ci + 1 >= count;
  const bool move = now && (!last || loop != 0);
  int next = last ? 0 : ci + 1;
  next = move ? next : ci;
  next = next < 0 ? 0 : (next > count - 1 ? count - 1 : next);       // (a table entry is read: never outside the robot's curves)
  curve_index[b] = next;
  cur_off[b] = curve_off[first + next];
  cur_len[b] = curve_len[first + next];
  point_index[b] = move ? 0 : point_index[b];
  arrived[b] = (latched != 0 || (now && last && loop == 0)) ? 1 : 0;
  const double x = state[b * 3 + 0], y = state[b * 3 + 1], th = state[b * 3 + 2];
  par_a[b].state[0] = x; par_a[b].state[1] = y; par_a[b].state[2] = th;
  par_b[b].state[0] = x; par_b[b].state[1] = y; par_b[b].state[2] = th;
}

__global__ __launch_bounds__(CY_THREADS) void cycle_act_kernel(
    int batch, int T, int kin, int first_cycle, int cycle, const float* __restrict__ opt_u, const float* __restrict__ min_distance,
    float threshold, const int* __restrict__ arrived, const int* __restrict__ collided, const float* __restrict__ override_row,
    const int* __restrict__ n_points, float* __restrict__ cur_vel, float* __restrict__ action, uint8_t* __restrict__ stop_out,
    int* __restrict__ frozen, float* __restrict__ log_actions, uint8_t* __restrict__ log_stop, float* __restrict__ log_controls,
    int* __restrict__ log_n_points) {
  const int b = blockIdx.x * CY_THREADS + threadIdx.x;
  if (b >= batch) return;
  const bool done = arrived[b] != 0;
  const bool keep = done && first_cycle == 0;                 // neupan.py:137 is not reached by a robot that has arrived
  const float* u = opt_u + (size_t)b * 2 * T;
  float* cv = cur_vel + (size_t)b * 2 * T;
  float* lc = log_controls ? log_controls + ((size_t)cycle * batch + b) * 2 * T : nullptr;
  for (int i = 0; i < 2 * T; ++i) {
    const float ui = u[i], old = cv[i];
    cv[i] = keep ? old : ui;
    if (lc) lc[i] = ui;
  }
  const bool stop = min_distance[b] < threshold;              // neupan.py:150-154, :169
  const float v = u[0], w = u[T];
  float a0 = v, a1 = w;
  if (kin == NPA_KIN_OMNI) {                                  // neupan.py:158-164
    a0 = v * cosf(w);
    a1 = v * sinf(w);
  }
  const bool zero = done || stop;
  a0 = zero ? 0.f : a0;
  a1 = zero ? 0.f : a1;
  if (override_row) {                                         // scripted robots: entries that are not NaN replace the action
    const float o0 = override_row[b * 2 + 0], o1 = override_row[b * 2 + 1];
    a0 = o0 != o0 ? a0 : o0;
    a1 = o1 != o1 ? a1 : o1;
  }
  const bool frz = done || collided[b] != 0;
  a0 = frz ? 0.f : a0;
  a1 = frz ? 0.f : a1;
  const uint8_t s = (stop && !done) ? 1 : 0;
  action[b * 2 + 0] = a0;
  action[b * 2 + 1] = a1;
  stop_out[b] = s;
  frozen[b] = frz ? 1 : 0;
  const size_t row = (size_t)cycle * batch + b;
  if (log_actions) { log_actions[row * 2 + 0] = a0; log_actions[row * 2 + 1] = a1; }
  if (log_stop) log_stop[row] = s;
  if (log_n_points) log_n_points[row] = n_points ? n_points[b] : 0;
}

__global__ __launch_bounds__(CY_THREADS) void cycle_commit_kernel(
    int batch, int cycle, const double* __restrict__ state, const double* __restrict__ clearance, int* __restrict__ collided,
    double* __restrict__ log_states, double* __restrict__ log_clearance) {
  const int b = blockIdx.x * CY_THREADS + threadIdx.x;
  if (b >= batch) return;
  const double c = clearance[b];
  collided[b] = (collided[b] != 0 || c <= 0.0) ? 1 : 0;
  if (log_clearance) log_clearance[(size_t)cycle * batch + b] = c;
  if (log_states) {
    double* row = log_states + ((size_t)(cycle + 1) * batch + b) * 3;
    row[0] = state[b * 3 + 0]; row[1] = state[b * 3 + 1]; row[2] = state[b * 3 + 2];
  }
}

// The arguments of curve_wave_kernel, by value as ONE kernel argument (a code object describes every kernel argument in its
// metadata; 28 of them were 2 KB of the library).  retask == 0 (npa_curve_batch): B plain curves, start / goals [B][3], g_stride 1,
// one capacity, rows [B][capacity][4], n_rows; the fields behind n_rows are not read.  retask != 0 (npa_cycle_retask): start is
// the state, rows the curve table, n_rows the retask_status.
struct CurveWaveArgs {                       // (what a wave reads first comes first: the registers of the rest load late)
  int retask, batch, T, cycle, style, g_stride, capacity;
  const int *mask, *collided, *n_goals, *robot_first, *curve_off, *row_capacity;
  int *goal_index, *arrived, *log_goal;
  double rho;
  const double *start, *goals, *interval;
  double* rows;
  int *n_rows, *curve_len, *curve_index, *cur_off, *cur_len, *point_index;
  float* cur_vel;
};

// One wave per curve, two callers: npa_curve_batch and npa_cycle_retask (the next goal of a robot that has arrived, into its
// region of the curve table).  ONE kernel, because the curve is some 10 KB of inlined double-precision library code and the
// product library has a size limit; `retask` is a launch argument, so the branch is the whole wave's.  Everything a re-task's
// decision reads is loaded before anything is written, and a wave with nothing to do leaves at its first test.
__global__ __launch_bounds__(npa_curve::kWave) void curve_wave_kernel(CurveWaveArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int gi = 0, off = 0, cap = a.capacity;
  size_t row0 = (size_t)b * a.capacity;
  // Lane l owns word l of what the wave writes behind the curve (WORDS below): its address is chosen here, in front of the curve,
  // so that the nine array arguments are not held in scalar registers across it; the curve's own code needs those.
  int* word = lane == 0 ? a.n_rows + b : nullptr;
  float* vel = nullptr;
  if (a.retask) {
    gi = a.goal_index[b];
    const bool go = a.arrived[b] != 0 && a.collided[b] == 0 && gi >= 0 && gi < a.n_goals[b];
    int* lg = a.log_goal ? a.log_goal + (size_t)a.cycle * a.batch + b : nullptr;
    if (!go) {
      if (lane == 0) {
        a.n_rows[b] = 0;
        if (lg) *lg = gi;
      }
      return;
    }
    const int first = a.robot_first[b];
    off = a.curve_off[first];
    cap = a.row_capacity[b];
    row0 = (size_t)off;
    word = lane == 1 ? lg : word;                         // WORDS: 0 retask_status, 1 the log row, 2 goal_index, 3 arrived,
    word = lane == 2 ? a.goal_index + b : word;           // 4 point_index, 5 curve_index, 6 cur_off, 7 cur_len, 8 curve_len
    word = lane == 3 ? a.arrived + b : word;
    word = lane == 4 ? a.point_index + b : word;
    word = lane == 5 ? a.curve_index + b : word;
    word = lane == 6 ? a.cur_off + b : word;
    word = lane == 7 ? a.cur_len + b : word;
    word = lane == 8 ? a.curve_len + first : word;
    vel = lane < 2 * a.T ? a.cur_vel + (size_t)b * 2 * a.T + lane : nullptr;
  } else if (a.mask && a.mask[b] == 0) {
    return;
  }
  const int needed = npa_curve::curve_wave(a.style, a.start + (size_t)b * 3, a.goals + ((size_t)b * a.g_stride + gi) * 3,
                                           a.interval[b], a.rho, cap, a.rows + row0 * 4, lane);
  if (!word && !vel) return;
  if (!a.retask) {
    *word = needed > cap ? -needed : needed;              // (lane 0)
    return;
  }
  const bool fits = needed >= 1 && needed <= cap;
  if (!fits) {                                            // the robot stays arrived, the goal is not consumed
    if (word && lane < 2) *word = lane == 0 ? 2 : gi;
    return;
  }
  if (vel) *vel = 0.f;                                    // reset(): neupan.py:288-294
  const int value = lane == 0 ? 1 : (lane <= 2 ? gi + 1 : (lane <= 5 ? 0 : (lane == 6 ? off : needed)));
  if (word) *word = value;
}

// The arguments of route_wave_kernel, one struct as CurveWaveArgs and in its order; what differs: no style and no radius, the
// fields and the map's frame, field_of [B][g_stride] beside the goals.  retask == 0: npa_route_curve_batch, != 0:
// npa_cycle_retask_routed.  shortcut != 0: their `_los` forms (the header's "line-of-sight shortcutting").
struct RouteWaveArgs {
  int retask, batch, T, cycle, g_stride, capacity, nx, ny, n_fields, shortcut;
  const int *mask, *collided, *n_goals, *robot_first, *curve_off, *row_capacity, *field_of;
  int *goal_index, *arrived, *log_goal;
  const uint32_t* fields;
  double x0, y0, res;
  const double *start, *goals, *interval;
  double* rows;
  int *n_rows, *curve_len, *curve_index, *cur_off, *cur_len, *point_index;
  float* cur_vel;
};

constexpr int RW_NO_ROUTE = 0, RW_NO_CURVE = -2147483647 - 1;    // what route_wave returns besides a row count (the second is what
                                                                 // npa_route_curve_batch stores: more rows than any capacity)

// move k of E, W, N, S, NE, NW, SE, SW (route.MOVES): its step and its cost
__device__ __forceinline__ int move_di(int k) { return k < 4 ? (k == 0 ? 1 : (k == 1 ? -1 : 0)) : ((k & 1) ? -1 : 1); }
__device__ __forceinline__ int move_dj(int k) { return k < 4 ? (k == 2 ? 1 : (k == 3 ? -1 : 0)) : (k < 6 ? 1 : -1); }
__device__ __forceinline__ uint32_t move_cost(int k) { return k < 4 ? 5u : 7u; }

// The header's "visibility" of cells (i0, j0) and (i1, j1), both inside the array, across the wave: lane l takes columns l,
// l + 64, ... of the major axis and loads the two or three cells the segment between the centres meets there; ONE ballot of
// "a cell of mine is BLOCKED" decides, so the answer is the whole wave's.  32-bit integers only.  With N = (2c - 1) ay + ax
// (>= ax - ay >= 0) and d = 2 ax: the header's lo = ceil(N / d) - 1 and hi = floor((N + 2 ay) / d) = q + (r + 2 ay >= d), since
// r + 2 ay < 2 d -- one unsigned division per column.  ax == 0 (one cell): d = 1 gives lo = hi = 0.
__device__ __forceinline__ bool route_visible(const uint32_t* field, int nx, int i0, int j0, int i1, int j1, int lane) {
  const int di = i1 - i0, dj = j1 - j0, adi = di < 0 ? -di : di, adj = dj < 0 ? -dj : dj;
  const bool swap = adj > adi;
  const int ax = swap ? adj : adi, ay = swap ? adi : adj;
  const int si = (di > 0) - (di < 0), sj = ((dj > 0) - (dj < 0)) * nx;       // a step along x, along y, in words of the field
  const int major = swap ? sj : si, minor = swap ? si : sj;
  const uint32_t d = ax ? 2u * (uint32_t)ax : 1u;
  const int base = j0 * nx + i0;                                              // (nx ny <= NPA_ROUTE_MAX_CELLS: every product below 2^29)
  bool hit = false;
#pragma nounroll
  for (int c0 = 0; c0 <= ax; c0 += npa_curve::kWave) {
    const int c = c0 + lane;
    if (c <= ax) {
      const uint32_t n = (uint32_t)((2 * c - 1) * ay + ax);
      const uint32_t q = n / d, r = n - q * d;
      int lo = (int)q - 1 + (r != 0u ? 1 : 0), hi = (int)q + (r + 2u * (uint32_t)ay >= d ? 1 : 0);
      lo = lo < 0 ? 0 : lo;
      hi = hi > ay ? ay : hi;
      for (int m = lo; m <= hi; ++m) hit |= field[base + c * major + m * minor] == NPA_ROUTE_BLOCKED;
    }
  }
  return __ballot(hit) == 0;
}

// lane l's double of a vector register as a wave-uniform value (two readlanes): how route_wave keeps the uniform doubles it
// needs rarely -- the two poses, the interval -- out of the scalar registers, which the walk, the visibility test and the curve need
__device__ __forceinline__ double lane_double(double v, int l) {
  const long long w = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)w, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(w >> 32), l);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// One wave, one routed path (include/neupan_amd.h, "routed curves"): the chain from the start's cell down field f, a `line`
// curve between the way-points.  Everything the walk decides is the whole wave's: the cell, its value and the move are the same
// in every lane (the move is the lowest bit of a ballot), so the loops are uniform and only the row stores are per lane.  The
// walk runs twice, counting and then writing, in ONE loop body: nothing is kept between the passes but the row count.  Returns
// the rows of the path (written iff <= capacity), RW_NO_ROUTE or RW_NO_CURVE (a segment outside the curve specification).
// a.shortcut: a way-point is a candidate -- while it is visible from the anchor's cell (route_visible) it is only remembered as
// `last`; the first that is not emits the segment to `last`, which becomes the anchor; the goal emits to `last` if it is not
// visible and then to itself.  Anchor and `last` are four wave-uniform integers: no list of turns.  Without it every
// candidate is the one emit to itself, with the operations and so the bits this loop had before it knew of shortcuts.
__device__ __forceinline__ int route_wave(const RouteWaveArgs& a, int f, const double* start, const double* goal, double interval,
                                          int capacity, double* rows, int lane) {
#pragma clang fp contract(off)
  const double sx = start[0], sy = start[1], gx = goal[0], gy = goal[1], gth = goal[2];
  if (f < 0 || f >= a.n_fields) return RW_NO_ROUTE;
  const double fi = floor((sx - a.x0) / a.res), fj = floor((sy - a.y0) / a.res);       // route.cells_of
  if (!(fi >= 0.0 && fi < (double)a.nx && fj >= 0.0 && fj < (double)a.ny)) return RW_NO_ROUTE;      // (a NaN is outside)
  const uint32_t* field = a.fields + (size_t)f * ((size_t)a.nx * a.ny);
  const int i0 = (int)fi, j0 = (int)fj;
  const uint32_t v0 = field[j0 * a.nx + i0];                                             // (nx ny <= NPA_ROUTE_MAX_CELLS: an int)
  if (v0 >= NPA_ROUTE_UNREACHED) return RW_NO_ROUTE;
  // lane k < 8 looks at neighbour k; the two axis moves beside it (an axis move is beside itself) are bits of the free mask
  const int k = lane & 7, di = move_di(k), dj = move_dj(k);
  const uint32_t cost = move_cost(k);
  const int side_i = k < 4 ? k : (k & 1), side_j = k < 4 ? k : (k < 6 ? 2 : 3);
  long long count = 0;
  // lane_double's lanes 0 .. 5: sx, sy, gx, gy, gth, the interval
  const double keep = lane == 0 ? sx : (lane == 1 ? sy : (lane == 2 ? gx : (lane == 3 ? gy : (lane == 4 ? gth : interval))));
  double h = gth;
#pragma nounroll
  for (int pass = 0; pass < 2; ++pass) {
    int i = i0, j = j0, prev = -1;
    // the anchor's cell and `last` (shortcut), four wave-uniform integers held in ONE vector register -- lanes 0 .. 3 hold ai, aj,
    // li, lj -- because the walk has no scalar registers to spare.  (The first candidate ends a straight run from the start's
    // cell: it is visible, so `last` is set before it is read.)
    int cells = (lane & 1) ? j0 : i0;
    uint32_t v = v0;
    double wx = lane_double(keep, 0), wy = lane_double(keep, 1);                // the way-point behind the walk
    count = 0;
    h = lane_double(keep, 4);
    for (;;) {
      int move = -1;
      if (v != 0) {
        const int ni = i + di, nj = j + dj;
        uint32_t nv = NPA_ROUTE_BLOCKED;
        if (lane < 8 && ni >= 0 && ni < a.nx && nj >= 0 && nj < a.ny) nv = field[nj * a.nx + ni];
        const unsigned long long open = __ballot(nv != NPA_ROUTE_BLOCKED);
        // (v - cost is below UNREACHED, so a neighbour that holds it is free, and a lane above 7 holds BLOCKED)
        const bool ok = ((open >> side_i) & (open >> side_j) & 1ull) != 0 && v >= cost && nv == v - cost;
        const unsigned long long allowed = __ballot(ok);
        if (allowed == 0) return RW_NO_ROUTE;                  // (not a converged field)
        move = __builtin_ctzll(allowed);
      }
      if (v == 0 || (prev >= 0 && move != prev)) {             // a way-point: the goal, or a cell at which the chain turns
        const bool cut = a.shortcut && !route_visible(field, a.nx, __builtin_amdgcn_readlane(cells, 0),
                                                      __builtin_amdgcn_readlane(cells, 1), i, j, lane);
#pragma nounroll
        for (int e = cut ? 0 : 1; e < 2; ++e) {                // e == 0: the emit to `last`; e == 1: to the way-point itself
          if (e && a.shortcut && v != 0) break;                // (a visible turn, or one that `last` was emitted for: remembered)
          int ci = i, cj = j;
          if (!e) {                                            // `last` becomes the anchor
            ci = __builtin_amdgcn_readlane(cells, 2);
            cj = __builtin_amdgcn_readlane(cells, 3);
            cells = lane == 0 ? ci : (lane == 1 ? cj : cells);
          }
          double px = lane_double(keep, 2), py = lane_double(keep, 3);      // the goal's own point, or a cell's centre
          if (!e || v != 0) {
            px = a.x0 + ((double)ci + 0.5) * a.res;            // route.centres_of
            py = a.y0 + ((double)cj + 0.5) * a.res;
          }
          if (!(wx == px && wy == py)) {
            const double from[3] = {wx, wy, 0.0}, to[3] = {px, py, 0.0};
            npa_curve::Curve c;
            npa_curve::curve_plan(NPA_CURVE_LINE, from, to, lane_double(keep, 5), 0.0, c);
            if (c.rows < 1) return RW_NO_CURVE;
            if (pass)
              for (int r = lane; r < c.n; r += npa_curve::kWave) {          // (the segment's goal row is the next one's first)
                double o[4];
                npa_curve::curve_row(c, r, o);
                double* out = rows + (size_t)(count + r) * 4;
                out[0] = o[0]; out[1] = o[1]; out[2] = o[2]; out[3] = o[3];
              }
            count += c.n;
            h = c.psi;
          }
          wx = px; wy = py;
        }
        cells = lane == 2 ? i : (lane == 3 ? j : cells);
      }
      if (v == 0) break;
      i += move_di(move); j += move_dj(move);
      v -= move_cost(move);                                    // (the chosen neighbour's value: every step lowers v)
      prev = move;
    }
    if (count + 1 > 0x7FFFFFFFll) return RW_NO_CURVE;          // (the row count is an int32)
    if (count + 1 > capacity) return (int)(count + 1);
  }
  if (lane == 0) {
    double* out = rows + (size_t)count * 4;
    out[0] = lane_double(keep, 2); out[1] = lane_double(keep, 3); out[2] = h; out[3] = 1.0;
  }
  return (int)(count + 1);
}

// curve_wave_kernel's routed sibling: the same gate, the same words behind the path, the same two callers' shapes
// (npa_route_curve_batch, npa_cycle_retask_routed); retask_status 3 is "no route".
__global__ __launch_bounds__(npa_curve::kWave) void route_wave_kernel(RouteWaveArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int gi = 0, off = 0, cap = a.capacity;
  size_t row0 = (size_t)b * a.capacity;
  int* word = lane == 0 ? a.n_rows + b : nullptr;
  float* vel = nullptr;
  if (a.retask) {
    gi = a.goal_index[b];
    const bool go = a.arrived[b] != 0 && a.collided[b] == 0 && gi >= 0 && gi < a.n_goals[b];
    int* lg = a.log_goal ? a.log_goal + (size_t)a.cycle * a.batch + b : nullptr;
    if (!go) {
      if (lane == 0) {
        a.n_rows[b] = 0;
        if (lg) *lg = gi;
      }
      return;
    }
    const int first = a.robot_first[b];
    off = a.curve_off[first];
    cap = a.row_capacity[b];
    row0 = (size_t)off;
    word = lane == 1 ? lg : word;                         // WORDS: as curve_wave_kernel's
    word = lane == 2 ? a.goal_index + b : word;
    word = lane == 3 ? a.arrived + b : word;
    word = lane == 4 ? a.point_index + b : word;
    word = lane == 5 ? a.curve_index + b : word;
    word = lane == 6 ? a.cur_off + b : word;
    word = lane == 7 ? a.cur_len + b : word;
    word = lane == 8 ? a.curve_len + first : word;
    vel = lane < 2 * a.T ? a.cur_vel + (size_t)b * 2 * a.T + lane : nullptr;
  } else if (a.mask && a.mask[b] == 0) {
    return;
  }
  const size_t g = (size_t)b * a.g_stride + gi;
  const int needed = route_wave(a, a.field_of[g], a.start + (size_t)b * 3, a.goals + g * 3, a.interval[b], cap, a.rows + row0 * 4, lane);
  if (!word && !vel) return;
  if (!a.retask) {
    *word = needed > cap ? -needed : needed;              // (lane 0)
    return;
  }
  if (needed < 1 || needed > cap) {                       // the robot stays arrived, the goal is not consumed
    if (word && lane < 2) *word = lane == 0 ? (needed == RW_NO_ROUTE ? 3 : 2) : gi;
    return;
  }
  if (vel) *vel = 0.f;                                    // reset(): neupan.py:288-294
  const int value = lane == 0 ? 1 : (lane <= 2 ? gi + 1 : (lane <= 5 ? 0 : (lane == 6 ? off : needed)));
  if (word) *word = value;
}

// One sweep of npa_route_relax (include/neupan_amd.h, "goal fields"): a workgroup owns a 16 x 16 tile of one field, relaxes it
// in LDS against a one-cell halo and stores the cells that fell.  Blocked cells and cells outside the array are BLOCKED in LDS,
// so the rounds test values only.  No atomics: a cell of `fields` is written by its own thread alone and only ever lower; the
// halo may be read while a neighbouring tile stores it -- the old or the new word, both lengths of real paths (the header has
// the whole argument).  Arguments in one struct, as CurveWaveArgs.
constexpr int RT_TILE = 16, RT_SPAN = RT_TILE + 2, RT_ROUNDS = 16;

struct RouteArgs {
  const uint8_t* blocked;
  uint32_t *fields, *changed;
  int nx, ny;
  uint32_t mark;
};

__global__ __launch_bounds__(RT_TILE* RT_TILE) void route_sweep_kernel(RouteArgs a) {
  __shared__ uint32_t tile[RT_SPAN * RT_SPAN];
  const int tid = threadIdx.x, i0 = blockIdx.x * RT_TILE - 1, j0 = blockIdx.y * RT_TILE - 1;
  uint32_t* field = a.fields + (size_t)blockIdx.z * ((size_t)a.nx * a.ny);
  for (int k = tid; k < RT_SPAN * RT_SPAN; k += RT_TILE * RT_TILE) {
    const int i = i0 + k % RT_SPAN, j = j0 + k / RT_SPAN;
    uint32_t v = NPA_ROUTE_BLOCKED;
    if (i >= 0 && i < a.nx && j >= 0 && j < a.ny) {
      const int c = j * a.nx + i;                             // (nx ny <= NPA_ROUTE_MAX_CELLS: an int)
      if (a.blocked[c] == 0) v = field[c];
    }
    tile[k] = v;
  }
  __syncthreads();
  const int at = ((tid >> 4) + 1) * RT_SPAN + (tid & 15) + 1;
  const uint32_t began = tile[at];
  uint32_t v = began;
#pragma nounroll
  for (int round = 0; round < RT_ROUNDS; ++round) {
    const uint32_t e = tile[at + 1], w = tile[at - 1], n = tile[at + RT_SPAN], s = tile[at - RT_SPAN];
    uint32_t m = v;
    // (a value below UNREACHED is below 7 * 2^26: the sums cannot wrap)
    m = e < NPA_ROUTE_UNREACHED ? min(m, e + 5u) : m;
    m = w < NPA_ROUTE_UNREACHED ? min(m, w + 5u) : m;
    m = n < NPA_ROUTE_UNREACHED ? min(m, n + 5u) : m;
    m = s < NPA_ROUTE_UNREACHED ? min(m, s + 5u) : m;
    const bool fe = e != NPA_ROUTE_BLOCKED, fw = w != NPA_ROUTE_BLOCKED, fn = n != NPA_ROUTE_BLOCKED, fs = s != NPA_ROUTE_BLOCKED;
    const uint32_t ne = tile[at + RT_SPAN + 1], nw = tile[at + RT_SPAN - 1], se = tile[at - RT_SPAN + 1], sw = tile[at - RT_SPAN - 1];
    m = (fe && fn && ne < NPA_ROUTE_UNREACHED) ? min(m, ne + 7u) : m;
    m = (fw && fn && nw < NPA_ROUTE_UNREACHED) ? min(m, nw + 7u) : m;
    m = (fe && fs && se < NPA_ROUTE_UNREACHED) ? min(m, se + 7u) : m;
    m = (fw && fs && sw < NPA_ROUTE_UNREACHED) ? min(m, sw + 7u) : m;
    const bool fell = began != NPA_ROUTE_BLOCKED && m < v;
    if (!__syncthreads_or(fell)) break;                       // (also: every read of this round is in front of its writes)
    if (fell) tile[at] = v = m;
    __syncthreads();
  }
  if (v < began) {                                            // (a blocked or outside cell kept `began`)
    field[(j0 + 1 + (tid >> 4)) * a.nx + i0 + 1 + (tid & 15)] = v;
    a.changed[blockIdx.z] = a.mark;
  }
}

}  // namespace

hipError_t npa_launch_route_relax(const uint8_t* blocked, int nx, int ny, int n_fields, uint32_t* fields, int sweeps,
                                             uint32_t sweep_base, uint32_t* changed, hipStream_t stream) {
  RouteArgs a = {blocked, fields, changed, nx, ny, sweep_base};
  const dim3 grid((nx + RT_TILE - 1) / RT_TILE, (ny + RT_TILE - 1) / RT_TILE, n_fields);
  for (int s = 0; s < sweeps; ++s) {
    a.mark = sweep_base + (uint32_t)s + 1u;
    hipLaunchKernelGGL(route_sweep_kernel, grid, dim3(RT_TILE * RT_TILE), 0, stream, a);
  }
  return hipGetLastError();
}

hipError_t npa_launch_curve_batch(int batch, int style, const double* start, const double* goal, const double* interval,
                                             double min_radius, int capacity, const int* mask, double* rows_out, int* n_rows,
                                             hipStream_t stream) {
  CurveWaveArgs a = {};
  a.batch = batch; a.T = 1; a.style = style; a.g_stride = 1; a.capacity = capacity; a.rho = min_radius;
  a.start = start; a.goals = goal; a.interval = interval; a.mask = mask; a.rows = rows_out; a.n_rows = n_rows;
  hipLaunchKernelGGL(curve_wave_kernel, dim3(batch), dim3(npa_curve::kWave), 0, stream, a);
  return hipGetLastError();
}

hipError_t npa_launch_cycle_retask(int batch, int T, int cycle, int style, double min_radius, const double* state,
                                              int* arrived, const int* collided, double* path, const int* curve_off,
                                              int* curve_len, const int* robot_first, const int* row_capacity,
                                              const double* goals, int g_stride, const int* n_goals, int* goal_index,
                                              const double* interval, int* curve_index, int* cur_off, int* cur_len,
                                              int* point_index, float* cur_vel, int* status, int* log_goal, hipStream_t stream) {
  const CurveWaveArgs a = {1, batch, T, cycle, style, g_stride, 0, nullptr, collided, n_goals, robot_first, curve_off, row_capacity,
                           goal_index, arrived, log_goal, min_radius, state, goals, interval, path, status, curve_len, curve_index,
                           cur_off, cur_len, point_index, cur_vel};
  hipLaunchKernelGGL(curve_wave_kernel, dim3(batch), dim3(npa_curve::kWave), 0, stream, a);
  return hipGetLastError();
}

// both routed exports: t == nullptr is npa_route_curve_batch (start, goal, capacity, mask, rows_out, n_rows), else the re-task
hipError_t npa_launch_route_wave(int batch, const RouteFrame& m, const int* field_of, const double* start, const double* goals,
                                 const double* interval, int capacity, const int* mask, double* rows, int* n_rows,
                                 const RetaskTable* t, hipStream_t stream) {
  RouteWaveArgs a = {};
  a.batch = batch; a.T = 1; a.g_stride = 1; a.capacity = capacity; a.nx = m.nx; a.ny = m.ny; a.n_fields = m.n_fields;
  a.shortcut = m.shortcut;
  a.mask = mask; a.field_of = field_of; a.fields = m.fields; a.x0 = m.x0; a.y0 = m.y0; a.res = m.resolution;
  a.start = start; a.goals = goals; a.interval = interval; a.rows = rows; a.n_rows = n_rows;
  if (t) {
    a.retask = 1; a.T = t->T; a.cycle = t->cycle; a.g_stride = t->g_stride; a.capacity = 0;
    a.collided = t->collided; a.n_goals = t->n_goals; a.robot_first = t->robot_first; a.curve_off = t->curve_off;
    a.row_capacity = t->row_capacity; a.goal_index = t->goal_index; a.arrived = t->arrived; a.log_goal = t->log_goal;
    a.curve_len = t->curve_len; a.curve_index = t->curve_index; a.cur_off = t->cur_off; a.cur_len = t->cur_len;
    a.point_index = t->point_index; a.cur_vel = t->cur_vel;
  }
  hipLaunchKernelGGL(route_wave_kernel, dim3(batch), dim3(npa_curve::kWave), 0, stream, a);
  return hipGetLastError();
}

hipError_t npa_launch_cycle_switch(int batch, int loop, const double* state, const int* curve_arrived,
                                              const int* curve_off, const int* curve_len, const int* robot_first,
                                              int* curve_index, int* cur_off, int* cur_len, int* point_index, int* arrived,
                                              npa_scan_params* params_a, npa_scan_params* params_b, hipStream_t stream) {
  hipLaunchKernelGGL(cycle_switch_kernel, dim3((batch + CY_THREADS - 1) / CY_THREADS), dim3(CY_THREADS), 0, stream, batch, loop,
                     state, curve_arrived, curve_off, curve_len, robot_first, curve_index, cur_off, cur_len, point_index, arrived,
                     params_a, params_b);
  return hipGetLastError();
}

hipError_t npa_launch_cycle_act(int batch, int T, int kin, int first_cycle, int cycle, const float* opt_u,
                                           const float* min_distance, float threshold, const int* arrived, const int* collided,
                                           const float* override_row, const int* n_points, float* cur_vel, float* action,
                                           uint8_t* stop, int* frozen, float* log_actions, uint8_t* log_stop,
                                           float* log_controls, int* log_n_points, hipStream_t stream) {
  hipLaunchKernelGGL(cycle_act_kernel, dim3((batch + CY_THREADS - 1) / CY_THREADS), dim3(CY_THREADS), 0, stream, batch, T, kin,
                     first_cycle, cycle, opt_u, min_distance, threshold, arrived, collided, override_row, n_points, cur_vel,
                     action, stop, frozen, log_actions, log_stop, log_controls, log_n_points);
  return hipGetLastError();
}

hipError_t npa_launch_cycle_commit(int batch, int cycle, const double* state, const double* clearance, int* collided,
                                              double* log_states, double* log_clearance, hipStream_t stream) {
  hipLaunchKernelGGL(cycle_commit_kernel, dim3((batch + CY_THREADS - 1) / CY_THREADS), dim3(CY_THREADS), 0, stream, batch, cycle,
                     state, clearance, collided, log_states, log_clearance);
  return hipGetLastError();
}
