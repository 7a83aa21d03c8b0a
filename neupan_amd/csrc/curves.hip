// curves.hip -- way-point curves between two poses: the exports of include/neupan_amd.h's curve block.
//   npa_curve_rows, npa_curve_generate   the host's evaluation of curves.h: no kernel, no HIP runtime call (like pack_image.hip)
//   npa_curve_batch                      B curves on the device, one wave per curve: the launch of curve_wave_kernel (cycle.hip),
//                                        the kernel npa_cycle_retask runs -- one copy of the curve's device code in the library
// The curve itself is curves.h, compiled for both sides.
#include "curves.h"

#include <cmath>

#include "handle.h"

extern "C" hipError_t npa_launch_curve_batch(int batch, int style, const double* start, const double* goal, const double* interval,
                                             double min_radius, int capacity, const int* mask, double* rows_out, int* n_rows,
                                             hipStream_t stream);

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
