// launch.h -- the ONE declaration of every function that one translation unit of libneupan_amd.so defines and another calls:
// the launchers of the kernels, what sizes them, the device-free part of creation, the merged group path.  A unit that defines
// or calls one includes this file and writes no prototype of its own.  They are C++ functions: the types are part of the symbol,
// so a definition that drifts from its declaration fails to link, and with the build's hidden visibility none of them is
// exported.  (The exports are include/neupan_amd.h's, and the six diagnostics at the end of this file.)
#pragma once
#include "../../include/neupan_amd.h"
#include "pan_common.h"

#include <vector>

// ---- dune.hip: keys, selection, calibration ----------------------------------------------------------------------------
// A SelGeoCall names a call's inputs and outputs for all three launches of the selection (the key launch and select_kernel
// read what they need of it); t0 = the first horizon slice to evaluate; ev_start / ev_stop may be null.
hipError_t npa_launch_trig(const float* cur_s, int batch, int T, float* trig, hipStream_t stream);
hipError_t npa_launch_encode(const DevParams& P, const SelGeoCall& c, int batch, int t0, unsigned* gkeys, int n_cu, int blocks_per_cu,
                             int key_terms, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop);
hipError_t npa_launch_select(const DevParams& P, const SelGeoCall& c, int batch, int t0, const unsigned* gkeys, int key_terms, float e0,
                             int debug, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop);
hipError_t npa_launch_select_geo(const DevParams& P, const SelGeoCall& c, int batch, int t0, int debug, unsigned audit_thresh,
                                 float margin_scale, int rows_bf16, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop);
int npa_select_geo_group_supported(int E);
hipError_t npa_launch_select_geo_group(const DevParams& P, const SelGeoGroup& G, int n, int batch, int t0, int n_stride_max, int debug,
                                       unsigned audit_thresh, float margin_scale, int rows_bf16, hipStream_t stream,
                                       hipEvent_t ev_start, hipEvent_t ev_stop);
hipError_t npa_launch_key_calib(const DevParams& P, const float* wpack, int key_terms, int nside, float half, unsigned* out,
                                hipStream_t stream);
hipError_t npa_launch_geo_calib(const DevParams& P, const float* wpack, int nside, float half, float inner, float shift, unsigned* out,
                                int n_cu, hipStream_t stream);
hipError_t npa_launch_k16_calib(const DevParams& P, const float* wpack, int nside, float half, float inner, unsigned* out, int n_cu,
                                hipStream_t stream);
hipError_t npa_launch_geo_table(const DevParams& P, float* wpack, float* nodes, int n_cu, hipStream_t stream);
hipError_t npa_launch_ktab_calib(const DevParams& P, const float* wpack, int nside, float half, float inner, float cx, float cy,
                                 unsigned* out, int n_cu, hipStream_t stream);

// ---- nrmp_qp.hip -------------------------------------------------------------------------------------------------------
// `extra`: the gradient pointers (npa_launch_qp_backward) or dbg_abc / dbg_f / dbg_x (npa_launch_qp); a value-initialised one
// for a plain solve.  A field of the QpCall that is left null is a null kernel argument.
size_t npa_qp_shmem_bytes(int T, int M);
hipError_t npa_launch_qp(const DevParams& P, const QpCall& c, int batch, const QpBackward& extra, hipStream_t stream,
                         hipEvent_t ev_start, hipEvent_t ev_stop);
hipError_t npa_launch_qp_backward(const DevParams& P, const QpCall& c, int batch, const QpBackward& extra, hipStream_t stream);
int npa_qp_group_supported(int T, int M);
hipError_t npa_launch_qp_group(const DevParams& P, const QpGroup& G, int n, int batch, hipStream_t stream, hipEvent_t ev_start,
                               hipEvent_t ev_stop);

// ---- frontend.hip, dune_labels.hip, ingest.hip, clearance.hip ------------------------------------------------------------
hipError_t npa_launch_nominal(int batch, int T, int kin, double dt, double L, const double* state, const float* vel,
                              const double* ref_speed, const double* path, const int* curve_off, const int* curve_len,
                              const int* point_index, const double* interval, float* nom_s, float* nom_u, float* ref_s, float* ref_us,
                              hipStream_t stream);
hipError_t npa_launch_progress(int batch, const double* state, const double* path, const int* curve_off, const int* curve_len,
                               int* point_index, double close_threshold, int ind_range, double arrive_threshold,
                               int arrive_index_threshold, float* min_dis, int* arrived, hipStream_t stream);
hipError_t npa_launch_scan(int batch, int beam_stride, const double* ranges, const double* beam_vel, const int* n_beams,
                           const npa_scan_params* params, int mode, int out_stride, float* points, float* velocities, int* count,
                           hipStream_t stream);
hipError_t npa_launch_labels(int E, const double* G, const double* h, long long n, const double* points, float* mu, float* dist,
                             hipStream_t stream);
int npa_ingest_offsets(int batch, int T, int n_stride, int with_vel, size_t* out, int n);
hipError_t npa_launch_ingest_unpack(int batch, int T, int n_stride, int with_vel, const void* record, size_t record_bytes,
                                    float* nom_s, float* nom_u, float* ref_s, float* ref_us, float* points, float* velocities,
                                    int* n_points, int* status, hipStream_t stream);
hipError_t npa_launch_clearance(const DevParams& P, int batch, int n_stride, const float* traj, const float* points,
                                const float* velocities, const int* n_points, float threshold, float* clearance, int* nearest,
                                float* min_clearance, int* first_violation, hipStream_t stream);

// ---- cycle.hip ---------------------------------------------------------------------------------------------------------
hipError_t npa_launch_route_relax(const uint8_t* blocked, int nx, int ny, int n_fields, uint32_t* fields, int sweeps,
                                  uint32_t sweep_base, uint32_t* changed, hipStream_t stream);
hipError_t npa_launch_curve_batch(int batch, int style, const double* start, const double* goal, const double* interval,
                                  double min_radius, int capacity, const int* mask, double* rows_out, int* n_rows, hipStream_t stream);
hipError_t npa_launch_cycle_retask(int batch, int T, int cycle, int style, double min_radius, const double* state, int* arrived,
                                   const int* collided, double* path, const int* curve_off, int* curve_len, const int* robot_first,
                                   const int* row_capacity, const double* goals, int g_stride, const int* n_goals, int* goal_index,
                                   const double* interval, int* curve_index, int* cur_off, int* cur_len, int* point_index,
                                   float* cur_vel, int* status, int* log_goal, hipStream_t stream);
// route_wave_kernel (the header's "routed curves"): the fields with the map's frame, and -- for the re-task alone -- the arguments
// of npa_cycle_retask that are not the curve's, by name.  t == nullptr: npa_route_curve_batch (start, goals [B][3], one
// capacity, mask, rows [B][capacity][4], n_rows); else npa_cycle_retask_routed (start = the state, goals [B][g_stride][3], rows =
// the curve table, n_rows = the retask_status; capacity and mask are not read).  shortcut: 1 from the `_los` exports, else 0.
struct RouteFrame {
  const uint32_t* fields;
  int n_fields, nx, ny;
  double x0, y0, resolution;
  int shortcut;
};
struct RetaskTable {
  int T, cycle, g_stride;
  int* arrived;
  const int *collided, *curve_off, *robot_first, *row_capacity, *n_goals;
  int *curve_len, *goal_index, *curve_index, *cur_off, *cur_len, *point_index;
  float* cur_vel;
  int* log_goal;
};
hipError_t npa_launch_route_wave(int batch, const RouteFrame& m, const int* field_of, const double* start, const double* goals,
                                 const double* interval, int capacity, const int* mask, double* rows, int* n_rows,
                                 const RetaskTable* t, hipStream_t stream);
hipError_t npa_launch_cycle_switch(int batch, int loop, const double* state, const int* curve_arrived, const int* curve_off,
                                   const int* curve_len, const int* robot_first, int* curve_index, int* cur_off, int* cur_len,
                                   int* point_index, int* arrived, npa_scan_params* params_a, npa_scan_params* params_b,
                                   hipStream_t stream);
hipError_t npa_launch_cycle_act(int batch, int T, int kin, int first_cycle, int cycle, const float* opt_u, const float* min_distance,
                                float threshold, const int* arrived, const int* collided, const float* override_row,
                                const int* n_points, float* cur_vel, float* action, uint8_t* stop, int* frozen, float* log_actions,
                                uint8_t* log_stop, float* log_controls, int* log_n_points, hipStream_t stream);
hipError_t npa_launch_cycle_commit(int batch, int cycle, const double* state, const double* clearance, int* collided,
                                   double* log_states, double* log_clearance, hipStream_t stream);

// ---- pack_image.hip: what npa_create derives from a configuration and a checkpoint WITHOUT a device --------------------
// Pure host arithmetic: the unit contains no kernel and calls nothing of the HIP runtime, so it also builds into a stand-alone
// host program (tests/tools/host/pack_image_check.cpp).
// Vertices of {x : G x <= h} for the geometric distance keys, from P.E / P.G / P.h of a P that is otherwise zero-filled or set
// from the configuration: pvx / pvy / pdx / pdy / pil, geo_rect, and rc* / rh* (the box itself for an axis-aligned rectangle,
// the bounding box grown by 10 um for any other polygon).  Returns geo_valid: the rows are consecutive counter-clockwise edges.
bool npa_polygon_geometry(DevParams& P);
// The WP_TOTAL floats of the pack as they are uploaded (layout: pan_common.h, WP_*): header of the key table (WP_TABH), +inf
// margins, and -- with weights -- every weight layout.  w == nullptr (a planner without obstacle stage): header and margins only.
void npa_build_pack_image(const DevParams& P, bool geo_valid, const npa_dune_weights* w, std::vector<float>& image);

// ---- c_api.hip, for serve_group.hip -------------------------------------------------------------------------------------
int npa_group_mergeable(int n, const npa_forward_call* calls);
// npa_forward_begin on a call record; launch_stage = false: everything but the staging launch (npa_group_begin_merged stages
// all its calls with one launch)
int npa_forward_begin_call(const npa_forward_call& a, int flags, bool launch_stage);

// ---- exported, in no public header: read through ctypes by tests/ and tests/tools/ ---------------------------------------
// npa_qp_shmem_bytes_path (nrmp_qp.hip)                    tests/test_abi.py: the LDS bytes the launchers ask for
// npa_group_begin_merged, npa_group_iter_merged (c_api.hip) tests/test_qp_dispatch_order.py drives the merged path by hand;
//                                                          serve_group.hip calls them too
// npa_dbg_group_merged_launches (c_api.hip)                the GPU tests check that the merged path ran
// npa_dbg_pack_image (create.hip)                          tests/test_pack_image.py
// npa_dbg_sel_prof (dune_device.h, -DNPA_SEL_PROF only)    tests/tools/select_phase_cycles.py
#pragma GCC visibility push(default)
extern "C" {
size_t npa_qp_shmem_bytes_path(int T, int M, int fast);
int npa_group_begin_merged(int n, const npa_forward_call* calls, int flags, int* begun);
int npa_group_iter_merged(int n, const npa_forward_call* calls, int k);
unsigned long long npa_dbg_group_merged_launches(void);
int npa_dbg_pack_image(const npa_config* cfg, const npa_dune_weights* w, float* image, size_t image_floats, void* params,
                       size_t params_bytes, size_t* params_size, int* geo_valid, size_t* offsets, int n_offsets);
int npa_dbg_sel_prof(unsigned long long* out16, int reset);
}
#pragma GCC visibility pop
