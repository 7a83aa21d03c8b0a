// curves.hip -- way-point curves between two poses: the exports of include/neupan_amd.h's curve block.
//   npa_curve_rows, npa_curve_generate   the host's evaluation of curves.h: no kernel, no HIP runtime call (like pack_image.hip)
//   npa_curve_batch                      B curves on the device, one wave per curve: the launch of curve_wave_kernel (cycle.hip),
//                                        the kernel npa_cycle_retask runs -- one copy of the curve's device code in the library
//   npa_route_relax                      the goal fields of a map (the header's "goal fields" block): the checks and the launches
//                                        of route_sweep_kernel (cycle.hip)
//   npa_route_curve_batch,               routed curves (the header's block of that name): the checks and the launch of
//   npa_cycle_retask_routed              route_wave_kernel (cycle.hip), B plain paths or the re-task of a cycle; each with a
//                                        `_los` form that shortcuts the way-points by line of sight
// The curve itself is curves.h, compiled for both sides.
#include "curves.h"

#include <cmath>

#include "handle.h"
#include "launch.h"

namespace {

using namespace npa_curve;

bool finite3(const double* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

// the argument list the two host exports share, then the plan (once for both: the host keeps one copy of it); 0: sound
__attribute__((noinline, minsize)) int host_plan(const char* who, int style, const double* start, const double* goal, double interval,
                                        double min_radius, Curve& c) {
  const char* what = nullptr;
  if (!start || !goal) what = "bad argument";
  else if (style != NPA_CURVE_LINE && style != NPA_CURVE_DUBINS) what = "style outside 0..1";
  else if (!(interval > 0.0) || !std::isfinite(interval)) what = "interval must be > 0";
  else if (style == NPA_CURVE_DUBINS && (!(min_radius > 0.0) || !std::isfinite(min_radius))) what = "dubins needs min_radius > 0";
  else if (!finite3(start) || !finite3(goal)) what = "a pose is not finite";
  if (!what) {
    curve_plan(style, start, goal, interval, min_radius, c);
    if (c.rows < 1) what = "the curve has more rows than an int32 counts";
  }
  return what ? fail(NPA_E_ARG, std::string(who) + ": " + what) : NPA_OK;
}

__attribute__((noinline, minsize)) void host_rows(const Curve& c, double* rows_out) {
  for (int i = 0; i < c.rows; ++i) curve_row(c, i, rows_out + (size_t)i * 4);
}

}  // namespace

extern "C" int npa_curve_rows(int style, const double* start, const double* goal, double interval, double min_radius) {
  Curve c;
  if (int rc = host_plan("npa_curve_rows", style, start, goal, interval, min_radius, c)) return rc;
  return c.rows;
}

extern "C" int npa_curve_generate(int style, const double* start, const double* goal, double interval, double min_radius,
                                  int capacity, double* rows_out, int32_t* n_rows) {
  if (capacity < 1 || !rows_out || !n_rows) return fail(NPA_E_ARG, "npa_curve_generate: bad argument");
  Curve c;
  if (int rc = host_plan("npa_curve_generate", style, start, goal, interval, min_radius, c)) return rc;
  if (c.rows > capacity) return fail(NPA_E_ARG, "npa_curve_generate: the curve does not fit the capacity");
  host_rows(c, rows_out);
  *n_rows = c.rows;
  return NPA_OK;
}

extern "C" int npa_curve_batch(int batch, int style, const double* start, const double* goal, const double* interval,
                               double min_radius, int capacity, const int32_t* mask, double* rows_out, int32_t* n_rows,
                               void* stream) {
  const char* what = nullptr;                                    // (one message object: the library has a size limit)
  if (batch < 1 || capacity < 1 || !start || !goal || !interval || !rows_out || !n_rows) what = "npa_curve_batch: bad argument";
  else if (style != NPA_CURVE_LINE && style != NPA_CURVE_DUBINS) what = "npa_curve_batch: style outside 0..1";
  else if (style == NPA_CURVE_DUBINS && (!(min_radius > 0.0) || !std::isfinite(min_radius)))
    what = "npa_curve_batch: dubins needs min_radius > 0";
  if (what) return fail(NPA_E_ARG, what);
  HIP_TRY(npa_launch_curve_batch(batch, style, start, goal, interval, min_radius, capacity, mask, rows_out, n_rows,
                                 (hipStream_t)stream));
  return NPA_OK;
}

// The goal fields of include/neupan_amd.h's "goal fields" block: `sweeps` launches of route_sweep_kernel (cycle.hip), no
// synchronisation.  It lives in this unit beside the other export that only checks and launches.
extern "C" int npa_route_relax(const uint8_t* blocked, int nx, int ny, int n_fields, uint32_t* fields, int sweeps,
                               uint32_t sweep_base, uint32_t* changed, void* stream) {
  const char* what = nullptr;                                    // (one message object, as npa_curve_batch)
  int code = NPA_E_ARG;
  if (!blocked || !fields || !changed) what = "npa_route_relax: a null pointer";
  else if (nx < 1 || ny < 1) what = "npa_route_relax: nx, ny must be >= 1";
  else if (n_fields < 1 || n_fields > 65535) what = "npa_route_relax: n_fields outside 1..65535";
  else if (sweeps < 1 || (uint64_t)sweep_base + (uint64_t)sweeps > 0xFFFFFFFFull) what = "npa_route_relax: sweeps < 1 or sweep_base + sweeps beyond uint32";
  else if ((int64_t)nx * ny > NPA_ROUTE_MAX_CELLS || ny > 16 * 65535) {
    what = "npa_route_relax: more than NPA_ROUTE_MAX_CELLS cells, or more than 16 * 65535 rows";
    code = NPA_E_UNSUPPORTED;
  }
  if (what) return fail(code, what);
  HIP_TRY(npa_launch_route_relax(blocked, nx, ny, n_fields, fields, sweeps, sweep_base, changed, (hipStream_t)stream));
  return NPA_OK;
}

// The routed curves of include/neupan_amd.h: all four exports check and launch route_wave_kernel (cycle.hip).  `sound`: the
// caller's own test (its pointers, batch, capacity / g_stride, receding, cycle); the fields and the frame are tested here.
namespace {
__attribute__((noinline, minsize)) int route_wave_call(const char* who, bool sound, int batch, const RouteFrame& m, const int* field_of,
                                                       const double* start, const double* goals, const double* interval, int capacity,
                                                       const int* mask, double* rows, int* n_rows, const RetaskTable* t, void* stream) {
  const char* what = nullptr;
  int code = NPA_E_ARG;
  if (!sound || !m.fields || !field_of) what = ": bad argument";
  else if (m.nx < 1 || m.ny < 1) what = ": nx, ny must be >= 1";
  else if (m.n_fields < 1 || m.n_fields > 65535) what = ": n_fields outside 1..65535";
  else if (!(m.resolution > 0.0) || !std::isfinite(m.resolution) || !std::isfinite(m.x0) || !std::isfinite(m.y0))
    what = ": the resolution must be finite and > 0, x0 and y0 finite";
  else if ((int64_t)m.nx * m.ny > NPA_ROUTE_MAX_CELLS) {
    what = ": more than NPA_ROUTE_MAX_CELLS cells";
    code = NPA_E_UNSUPPORTED;
  }
  if (what) return fail(code, std::string(who) + what);
  HIP_TRY(npa_launch_route_wave(batch, m, field_of, start, goals, interval, capacity, mask, rows, n_rows, t, (hipStream_t)stream));
  return NPA_OK;
}
}  // namespace

// each export beside its `_los` form (line-of-sight shortcutting: RouteFrame::shortcut): one body, two thunks
namespace {
__attribute__((noinline, minsize)) int route_batch_call(const char* who, int shortcut, int batch, const uint32_t* fields, int n_fields, int nx,
                                                        int ny, double x0, double y0, double resolution, const int32_t* field_of,
                                                        const double* start, const double* goal, const double* interval, int capacity,
                                                        const int32_t* mask, double* rows_out, int32_t* n_rows, void* stream) {
  const bool sound = batch >= 1 && capacity >= 1 && start && goal && interval && rows_out && n_rows;
  return route_wave_call(who, sound, batch, {fields, n_fields, nx, ny, x0, y0, resolution, shortcut}, field_of, start, goal, interval,
                         capacity, mask, rows_out, n_rows, nullptr, stream);
}

__attribute__((noinline, minsize)) int route_retask_call(const char* who, int shortcut, int batch, int receding, int cycle, const double* state,
                                                         int32_t* arrived, const int32_t* collided, double* path, const int32_t* curve_off,
                                                         int32_t* curve_len, const int32_t* robot_first, const int32_t* row_capacity,
                                                         const double* goals, int g_stride, const int32_t* n_goals, int32_t* goal_index,
                                                         const double* interval, int32_t* curve_index, int32_t* cur_off, int32_t* cur_len,
                                                         int32_t* point_index, float* cur_vel, int32_t* retask_status, int32_t* log_goal,
                                                         const uint32_t* fields, int n_fields, int nx, int ny, double x0, double y0,
                                                         double resolution, const int32_t* field_of, void* stream) {
  const bool sound = batch >= 1 && cycle >= 0 && g_stride >= 1 && receding >= 1 && receding <= NPA_MAX_T && state && arrived &&
                     collided && path && curve_off && curve_len && robot_first && row_capacity && goals && n_goals && goal_index &&
                     interval && curve_index && cur_off && cur_len && point_index && cur_vel && retask_status;
  const RetaskTable t = {receding, cycle, g_stride, arrived, collided, curve_off, robot_first, row_capacity, n_goals, curve_len,
                         goal_index, curve_index, cur_off, cur_len, point_index, cur_vel, log_goal};
  return route_wave_call(who, sound, batch, {fields, n_fields, nx, ny, x0, y0, resolution, shortcut}, field_of, state, goals, interval, 0,
                         nullptr, path, retask_status, &t, stream);
}
}  // namespace

#define NPA_ROUTE_BATCH_ARGS                                                                                                      \
  int batch, const uint32_t *fields, int n_fields, int nx, int ny, double x0, double y0, double resolution, const int32_t *field_of, \
      const double *start, const double *goal, const double *interval, int capacity, const int32_t *mask, double *rows_out,         \
      int32_t *n_rows, void *stream
#define NPA_ROUTE_BATCH_PASS \
  batch, fields, n_fields, nx, ny, x0, y0, resolution, field_of, start, goal, interval, capacity, mask, rows_out, n_rows, stream
extern "C" int npa_route_curve_batch(NPA_ROUTE_BATCH_ARGS) { return route_batch_call("npa_route_curve_batch", 0, NPA_ROUTE_BATCH_PASS); }
extern "C" int npa_route_curve_batch_los(NPA_ROUTE_BATCH_ARGS) {
  return route_batch_call("npa_route_curve_batch_los", 1, NPA_ROUTE_BATCH_PASS);
}

#define NPA_ROUTE_RETASK_ARGS                                                                                                       \
  int batch, int receding, int cycle, const double *state, int32_t *arrived, const int32_t *collided, double *path,                  \
      const int32_t *curve_off, int32_t *curve_len, const int32_t *robot_first, const int32_t *row_capacity, const double *goals,    \
      int g_stride, const int32_t *n_goals, int32_t *goal_index, const double *interval, int32_t *curve_index, int32_t *cur_off,     \
      int32_t *cur_len, int32_t *point_index, float *cur_vel, int32_t *retask_status, int32_t *log_goal, const uint32_t *fields,     \
      int n_fields, int nx, int ny, double x0, double y0, double resolution, const int32_t *field_of, void *stream
#define NPA_ROUTE_RETASK_PASS                                                                                                       \
  batch, receding, cycle, state, arrived, collided, path, curve_off, curve_len, robot_first, row_capacity, goals, g_stride, n_goals, \
      goal_index, interval, curve_index, cur_off, cur_len, point_index, cur_vel, retask_status, log_goal, fields, n_fields, nx, ny,  \
      x0, y0, resolution, field_of, stream
extern "C" int npa_cycle_retask_routed(NPA_ROUTE_RETASK_ARGS) {
  return route_retask_call("npa_cycle_retask_routed", 0, NPA_ROUTE_RETASK_PASS);
}
extern "C" int npa_cycle_retask_routed_los(NPA_ROUTE_RETASK_ARGS) {
  return route_retask_call("npa_cycle_retask_routed_los", 1, NPA_ROUTE_RETASK_PASS);
}
#undef NPA_ROUTE_BATCH_ARGS
#undef NPA_ROUTE_BATCH_PASS
#undef NPA_ROUTE_RETASK_ARGS
#undef NPA_ROUTE_RETASK_PASS
