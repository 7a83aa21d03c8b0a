/* neupan_amd_grid.h -- C ABI of the occupancy-grid obstacle of the device world (libneupan_amd_grid.so).
 *
 * A third library next to libneupan_amd.so (include/neupan_amd.h) and libneupan_amd_train.so, with this header as its
 * specification.  The device world of neupan_amd.h is a list of circles and segments; a floor plan, a maze or a recorded
 * SLAM map is an occupancy grid of 10^5 .. 10^6 occupied cells, which a primitive list cannot hold.  The two calls here
 * put such a map BEHIND the primitives of a world: npa_grid_scan merges the map into the ranges npa_world_scan[_noisy]
 * wrote, npa_grid_clearance into the clearance npa_world_step wrote.  A world without a map calls neither.
 * The conventions are neupan_amd.h's: int status (0 = ok, < 0 = NPA_E_*), device pointers owned by the caller, `stream` a
 * hipStream_t passed as void*, nothing synchronises, no workspace, no atomics, float64 C-contiguous arrays.
 *
 * The map.  cells [ny][nx] uint8 is a DEVICE array shared by every scene: cell (i, j), i < nx the column and j < ny the
 * row, is cells[j * nx + i] and is occupied iff that byte is non-zero.  (x0, y0) is the world position of the lower-left
 * corner of cell (0, 0), res > 0 the cell size.  With
 *       X(i) = x0 + i * res,   Y(j) = y0 + j * res        (float64: one multiply, one add, no contraction)
 * cell (i, j) is the CLOSED box [X(i), X(i+1)] x [Y(j), Y(j+1)].  Everything outside the grid is free.
 * Limits: 1 <= nx, ny and nx * ny < 2^31.
 *
 * npa_grid_scan (one launch; one lane per beam, 256-thread workgroups, grid (ceil(beam_stride / 256), batch)).
 *   Beam i < n_beams[b] of scene b (n_beams null: beam_stride; clamped to [0, beam_stride]) starts at the sensor pose
 *   o = state o offset of params[b] and has the angle `ang` of npa_world_scan, bit for bit (one definition, csrc/scan_beam.h,
 *   compiled into both libraries; used fields of npa_scan_params: state, offset, angle_min, angle_max, range_max).  With
 *   angle_std != 0 the angle is ang' = ang + angle_std * g_a of npa_world_scan_noisy, (g_a, g_r) the draws of
 *   (seed, scene_base + b, i, draw) (csrc/scan_noise.h, the same header).  d = (dx, dy) = the unit direction at that angle.
 *   Slab times of an occupied cell c = (i, j), float64, every operation rounded once:
 *       tx0 = (X(i) - ox) / dx,  tx1 = (X(i+1) - ox) / dx,   near_x = min(tx0, tx1),  far_x = max(tx0, tx1)
 *       dx == 0:  the x-slab is (-inf, +inf) when X(i) <= ox <= X(i+1), and empty otherwise;          the same in y
 *       enter = max(near_x, near_y),  leave = min(far_x, far_y)
 *   The ray meets c iff enter <= leave and leave >= 0, at t_c = max(enter, 0) (never -0).  The beam's grid range is
 *       t_g = min over the occupied cells of t_c                                       (+inf when the ray meets none)
 *   and the value reported for it is
 *       g = range_max exactly                                      when t_g >= range_max (a miss: never a phantom point)
 *       g = t_g                                                    when t_g < range_max and std == 0 (no add)
 *       g = min(max(t_g + std * g_r, 0) + 0, range_max)            when t_g < range_max and std != 0
 *   Merge (ranges, beam_vel, hit are IN/OUT: what npa_world_scan[_noisy] left there, or range_max / 0 / -1 for a map alone):
 *       g < ranges[b][i]:  ranges[b][i] = g,  hit[b][i] = NPA_HIT_GRID,  beam_vel[b][:][i] = 0;   otherwise all three stay.
 *   A tie keeps the primitive: the grid ranks behind every primitive index.  beam_vel [B][2][beam_stride] and hit
 *   [B][beam_stride] may be null.  Columns at or beyond n_beams[b] are not touched.
 *   The noisy range is a non-decreasing function of t (one add of the same std * g_r, two clamps), and both kernels use the
 *   same draw for a beam: the minimum of the two REPORTED values is the reported value of the minimum of the two casts, so
 *   the merged noisy scan is the noisy scan of the merged world.
 *   How the kernel finds the minimum is its own business.  It walks the cells along the ray (a DDA): every crossing time is
 *   computed from the cell indices by the formulas above, never accumulated, and the times are monotone in the index, so the
 *   first occupied cell met carries the minimum, with these bits.  Where the ray passes exactly through a cell corner
 *   (far_x == far_y) the two cells beside the corner are looked at too before the walk goes on diagonally.
 *   Two cases sit where the closed-box definition is unstable under a one-ulp change of the direction or of the origin;
 *   for them EITHER outcome -- the hit at that t, or the pass -- is accepted:
 *     - a ray that only touches a box: enter == leave in an axis, or the ray t >= 0 has one point in common with the box
 *       (an origin on a face, looking away);
 *     - an origin coordinate equal to a face coordinate with a zero direction component (a ray running along a face).
 *   Bounds.  The walk takes at most nx + ny + 2 steps, by a counter; finding the first cell takes a fixed number of
 *   corrections.  A NaN or infinite pose, offset, angle or range_max ends the beam as a miss (g = range_max; nothing is
 *   written unless range_max < ranges[b][i]).  No read leaves cells[0 .. nx * ny).
 *   A scene's result does not depend on the batch it is in (given scene_base) and the same call gives the same bytes.
 *
 * npa_grid_clearance (one launch; one wave per robot: the lanes stride over the window and gather its occupied cells, measure
 *   them 64 at a time, and a wave minimum ends it).
 *   state [B][3] f64 DEVICE: the poses;  vertices: HOST [E][2] f64, the robot's polygon in the robot frame, counter-clockwise,
 *   as npa_world_step takes them;  clearance [B] f64 DEVICE, IN/OUT.
 *   The window of robot b is every cell whose box meets the axis-aligned bounding box of the polygon at pose b, inflated by
 *   `reach` (the kernel may look at a few cells more: they cannot change the result).  For an occupied cell of the window:
 *       d = 0 when box and polygon intersect: an edge of one properly crosses an edge of the other, a corner of the box lies
 *           in or on the polygon, or a vertex of the polygon lies in or on the box (this covers containment either way);
 *       d = otherwise the smallest vertex-to-edge distance between the two: the corners of the box to the polygon's edges,
 *           the polygon's vertices to the box's edges (the segment rule of npa_world_step, applied to the box's four edges).
 *   c_g = the minimum of d over the window; a c_g above `reach`, and a window without an occupied cell, is +inf: cells outside
 *   the window are farther than `reach`, so c_g is exact exactly when it is <= reach.  clearance[b] = min(clearance[b], c_g).
 *   The minimum does not depend on the order of the reduction.  A robot with a NaN or infinite pose keeps its clearance.
 *   Every loop is bounded by the window, the window by the grid.
 *
 * Errors, returned before anything touches a device:
 *   NPA_E_ARG          a null required pointer (cells, params, ranges; cells, state, vertices, clearance); batch <= 0 (or
 *                      above 65535 scenes in a scan); nx or ny < 1; x0, y0 not finite; res, reach not positive or not
 *                      finite; std or angle_std negative or not finite; draw < 0; scene_base < 0 (or scene_base + batch
 *                      beyond an int); beam_stride <= 0; a polygon edge of zero length
 *   NPA_E_UNSUPPORTED  edge_num outside [3, NPA_MAX_E]; nx * ny >= 2^31
 */
#ifndef NEUPAN_AMD_GRID_H
#define NEUPAN_AMD_GRID_H

#include "neupan_amd.h"

#define NPA_HIT_GRID (-2)   /* hit[b][i] of a beam whose range is the map's */

#ifdef __cplusplus
extern "C" {
#endif
/* the exports of the library: everything else in it is built with hidden visibility */
#pragma GCC visibility push(default)

int npa_grid_scan(const uint8_t *cells, int nx, int ny, double x0, double y0, double res,
                  int batch, const npa_scan_params *params, const int32_t *n_beams, int beam_stride,
                  double *ranges, double *beam_vel, int32_t *hit,
                  double std, double angle_std, uint64_t seed, int scene_base, int draw, void *stream);

int npa_grid_clearance(const uint8_t *cells, int nx, int ny, double x0, double y0, double res,
                       int batch, const double *state, int edge_num, const double *vertices, double reach,
                       double *clearance, void *stream);

/* message of the calling thread's last failed call of this library */
const char *npa_grid_last_error(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
