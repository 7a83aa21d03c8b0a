/* neupan_amd.h -- C ABI of the MI355X-native PAN inner solver (libneupan_amd.so).
 *
 * The reference (hanruihua/NeuPAN, pure Python) has NO FFI/plugin interface; its seam for
 * this path is the torch.nn.Module contract of `PAN` (neupan/blocks/pan.py:28-147), built
 * at neupan/neupan.py:84 and called at neupan/neupan.py:129-131.  The entry points below
 * are what a ctypes binding behind that class needs; each cites the reference code it
 * replaces.  INTEGRATION.md shows the reference-side binding.
 *
 * Conventions
 *   - every function returns an int status: 0 = ok, <0 = NPA_E_* (never throws);
 *   - all array arguments of npa_forward_batch are DEVICE pointers owned by the caller
 *     (torch-ROCm tensors' data_ptr()); the library allocates nothing per call;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     all work is enqueued on it, nothing synchronises;
 *   - layouts are the reference's tensors with a leading scene (batch) axis, fp32,
 *     C-contiguous: coordinates on the slow axis, time/points on the fast axis.
 */
#ifndef NEUPAN_AMD_H
#define NEUPAN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the exports of the library: everything else in it is built with hidden visibility */
#pragma GCC visibility push(default)

#define NPA_OK 0
#define NPA_E_ARG (-1)      /* bad argument (null pointer, size out of range)            */
#define NPA_E_HIP (-2)      /* a HIP runtime call failed; see npa_last_error()           */
#define NPA_E_UNSUPPORTED (-3) /* configuration outside the compiled limits (NPA_MAX_*)  */

#define NPA_MAX_T 21        /* receding horizon (3T <= 64: one KKT row per lane)          */
#define NPA_MAX_M 32        /* nrmp_max_num (points kept per horizon step)                */
#define NPA_MAX_E 8         /* polytope edges of the robot (rows of G)                    */

#define NPA_KIN_DIFF 0
#define NPA_KIN_ACKER 1
#define NPA_KIN_OMNI 2

/* Constructor arguments of PAN (pan.py:43-56), of its adjust_kwargs (pan.py:75-82) and the
 * robot attributes the path reads (robot.py:53-71: G, h, kinematics, L, speed_bound,
 * acce_bound = max_acce*dt).  Unbounded speed/acceleration = INFINITY (robot.py:37-38). */
typedef struct npa_config {
  int32_t receding;        /* T   */
  int32_t iter_num;        /* K: PAN iterations per forward (pan.py:128)                  */
  int32_t dune_max_num;    /* points fed to DUNE per scene after decimation (pan.py:171)  */
  int32_t nrmp_max_num;    /* M: nearest points kept per step (nrmp.py:254)               */
  int32_t edge_num;        /* E = G.shape[0]                                              */
  int32_t kinematics;      /* NPA_KIN_*                                                   */
  float iter_threshold;    /* pan.py:243; <= 0 disables the early exit                    */
  /* python floats in the reference (fp64): */
  double step_time;        /* dt  */
  double wheelbase;        /* L (acker only)                                              */
  double speed_bound[2];
  double acce_bound[2];
  double ro_obs, bk;
  /* fp32 tensors in the reference (nrmp.py:79-95, configuration/__init__.py:27): */
  float q_s[3];            /* scalar q_s is passed replicated                             */
  float p_u, eta, d_max, d_min;
  float G[NPA_MAX_E][2];
  float h[NPA_MAX_E];
} npa_config;

/* The 18 tensors of a DUNE checkpoint in state_dict order (obs_point_net.py:31-46;
 * written by dune_train.py:266-274, loaded by dune.py:131-144), HOST pointers, fp32,
 * torch layout: Linear weight is (out,in) row-major. */
typedef struct npa_dune_weights {
  const float *lin_w[6];   /* MLP.{0,3,5,8,10,13}.weight : (32,2) (32,32)x4 (E,32)        */
  const float *lin_b[6];   /* MLP.{0,3,5,8,10,13}.bias                                    */
  const float *ln_w[3];    /* MLP.{1,6,11}.weight (32,)                                   */
  const float *ln_b[3];    /* MLP.{1,6,11}.bias   (32,)                                   */
} npa_dune_weights;

typedef struct npa_handle npa_handle;

/* Replaces PAN.__init__ + DUNE.load_model (pan.py:43-107, dune.py:131-144).  Uploads the
 * repacked weights (a few KiB) to the current device.  One handle per (device, config). */
int npa_create(const npa_config *cfg, const npa_dune_weights *w, npa_handle **out);
int npa_destroy(npa_handle *h);

/* How this handle computes the distance KEYS that nominate the nrmp_max_num nearest points of a slice (the rows it
 * emits are always re-encoded with the exact fp32 encoder and ranked on the exact result; dune.py:100 argsort is
 * reproduced on those):
 *   key_terms 4 = geometric: closed-form distance to the robot polygon, computed inside the selection kernel (no
 *               encoder pass over all points); measured_error = largest |network distance - geometric distance| [m]
 *               over the distance bands 0.25 .. 8 m, margin_e0 = the largest candidate margin over those bands
 *               (1.5 x (error + grid slack), NPA_KEY_SAFETY); both measured by npa_create for THIS checkpoint on nested
 *               4096 x 4096 grids out to +-128 m; points further out are always candidates;
 *   key_terms 1 = network keys with single fp16 products, 3 = fp16x2 split products, 0 = exact fp32 encoder:
 *               measured_error = max |key - exact| / (1 + |exact|) over a 1024 x 1024 grid of the training square
 *               (|x|, |y| <= 25 m), margin_e0 = 5 x that (NPA_KEY_SAFETY). */
int npa_key_mode(const npa_handle *h, int *key_terms, float *measured_error, float *margin_e0);

/* What npa_create measured about the geometric keys of THIS checkpoint (key_terms 4 or not), out[0..n), n <= 6:
 *   [0] 1 when the polygon's rows are consecutive counter-clockwise edges (else geometric keys are never used),
 *   [1] largest |network distance - geometric distance| [m] and [2] largest candidate margin over the bands 0.25 .. 8 m,
 *   [3] refinement ratio: |f| measured at the CELL CENTRES of the calibration grids over what the grid nodes predicted for
 *       the space between them (node maximum + neighbour difference), largest over the distance bands; <= 1 when the
 *       grids resolve f, and a checkpoint above 1.25 keeps network keys (a ridge narrower than a grid cell),
 *   [4] steepest neighbour difference per metre on the finest grid (an estimate of the Lipschitz constant of f next to
 *       the robot), [5] g_far: points at or beyond this geometric distance are always candidates,
 *   [6], [7] (handles created with NPA_KEYS_PRECISION=bf16, else 0): largest measured |bf16-encoder distance - exact distance|
 *       and the largest margin built from it over the bands below 8 m (the bf16 KEY tier: a slice whose candidate list
 *       overflows is filtered with the bf16-MFMA encoder, the survivors re-encoded exactly -- rows bitwise the default path's).
 *   [8], [9] (0 when the handle has no key table: NPA_GEO_TABLE=0, network keys): largest measured |g + f_table - exact
 *       distance| and the largest margin built from it over the bands below 8 m -- the TABLE-corrected geometric key, the
 *       second-stage filter of candidate lists longer than one encoder tile (f = network - geometric distance tabulated at
 *       creation on four nested 512 x 512-cell squares (half extents 2 .. 128 m), bilinear; survivors re-encoded exactly and audited: rows bitwise).
 * The margin is MEASURED, not proven (LayerNorm leaves no usable analytic Lipschitz bound); npa_audit_read is the
 * run-time check. */
int npa_geo_report(const npa_handle *h, float *out, int n);

/* Run-time audit of the geometric-key margin (key_terms 4).  Every launch of the selection kernel checks the bound
 * |exact network distance - geometric distance| <= margin on every point it encodes exactly (the candidates), and a
 * fraction of its slice waves (default 1 in 64; NPA_AUDIT_RATE) on 32 further points spread over the slice.  Counters
 * since creation (or the last reset): audit tiles run, points they checked, violations seen (candidates included),
 * largest excess over the margin [m].  While violations != 0 the kernel treats EVERY point as a candidate (exact keys for
 * the whole slice: slow and right), so a wrong margin cannot keep producing wrong plans; the owner should then rebuild
 * the handle with network keys (NPA_KEY_TERMS=1).  Synchronises the device.  reset != 0 zeroes the counters (and with them
 * the distrust). */
int npa_audit_read(npa_handle *h, uint64_t *tiles, uint64_t *points, uint64_t *violations, float *worst_excess, int reset);

/* The violation count of npa_audit_read WITHOUT synchronising the device: the selection kernel mirrors every violation
 * it counts into pinned host memory, and this reads that word.  Cheap enough to poll after every step of a serving loop
 * (neupan_amd.PAN does, and warns).  A non-zero value means: at least one launch may have emitted rows from a selection
 * that missed a true member (the plans of THAT launch are suspect), every later launch ran on exact keys (slow, right).
 * What to do then: npa_use_network_keys (or rebuild the handle with NPA_KEY_TERMS=1), re-plan the affected step. */
int npa_audit_peek(const npa_handle *h, uint64_t *violations);

/* Switch a handle from geometric to network keys for good (calibrates them, resets the audit).  The workspace grows by the
 * key buffer: call npa_workspace_bytes again and re-allocate (a forward call with the old size fails with NPA_E_ARG).  No
 * forward call may be in progress; synchronises the device.  A no-op on a handle that already uses network keys. */
int npa_use_network_keys(npa_handle *h);

/* What the create-time self-test (npa_create runs every kernel of the handle once on a fixed synthetic problem sized to
 * the robot) changed about this handle.  Hard failures of npa_create are only: two runs that differ bitwise, a control
 * that is not finite or outside its speed bound.  Soft outcomes are reported here:
 *   NPA_SELFTEST_WARM_OFF      warm- and cold-started solves of the test problem differed by more than 1e-4 (a QP that is
 *                              flat along steering directions can do that legitimately): the interior-point warm start
 *                              across PAN iterations is switched off for this handle;
 *   NPA_SELFTEST_GEO_REJECTED  the geometric-key selection missed a member of the exact selection on the test cloud: the
 *                              handle uses network keys (npa_key_mode tells which). */
#define NPA_SELFTEST_WARM_OFF 1
#define NPA_SELFTEST_GEO_REJECTED 2
int npa_selftest_flags(const npa_handle *h, int *flags);

/* Handles of the same checkpoint, polygon, calibration knobs and device SHARE what npa_create derives from the checkpoint: the
 * repacked weights, the margins of the geometric key, the 8.4 MB key table and its margins (the reference loads one model per
 * planner, dune.py:131-144; a serving process makes one handle per batch in flight).  The first npa_create of a key measures
 * (ten calibration launches, ~35 ms), the later ones take the device buffer and the figures and run only their self-test.  The
 * buffer lives as long as a handle uses it.  Everything a handle can change stays its own: the key mode in force
 * (npa_use_network_keys), audit counters, statistics, self-test outcomes.  This reports, for the process: packs calibrated,
 * creations that shared one, packs alive now.  NPA_PACK_CACHE=0 in the environment gives every handle a private pack. */
int npa_pack_cache_stats(int64_t *calibrations, int64_t *shared_creates, int64_t *alive);

/* Replaces NRMP.update_adjust_parameters_value (nrmp.py:170-217). */
int npa_set_adjust(npa_handle *h, const float q_s[3], float p_u, float eta, float d_max, float d_min);

/* Per-scene adjust parameters.  The reference makes (q_s, p_u, eta, d_max, d_min) parameters of ONE problem
 * (neupan/blocks/nrmp.py:79-95) that are set per planner (nrmp.py:170-217); a batch here is B such problems, and this gives
 * every scene its own set -- a fleet whose robots want different d_max / eta, a population of candidate sets for LON.
 *   theta: DEVICE pointer to [batch][8] fp32: q_s[0..2], p_u, eta, d_max, d_min, reserved -- the columns of
 *   npa_nrmp_backward's grad_theta, so a gradient row and a parameter row line up.
 * The block is caller-owned and is READ AT KERNEL RUN TIME, in stream order: writing new rows into it changes what the
 * next launch -- or the next replay of a captured graph -- uses, and it must stay valid while work that uses it is in
 * flight.  The pointer is sticky on the handle; theta == NULL (any batch) returns the handle to its uniform set, which
 * npa_set_adjust keeps updating meanwhile.  While it is set, every entry point that solves the QP uses row b for scene b:
 * npa_forward_batch / _flags / _begin / _iter / _end, npa_forward_batch_group (calls that differ only in their block
 * still share merged launches), npa_nrmp_stage and npa_nrmp_backward, whose grad_theta[b] is then the gradient with
 * respect to theta[b].  A call with another batch than the registered one returns NPA_E_ARG.  A block that repeats the
 * uniform set in every row gives the uniform path's results bitwise. */
int npa_set_adjust_batch(npa_handle *h, const float *theta, int batch);

/* Bytes of caller-owned device memory npa_forward_batch needs for `batch` scenes:
 * scratch (no meaning between calls) and state (the stop criterion's memory of the
 * previous iterate, pan.py:100-105 / 215-243; zero it to reset a scene). */
size_t npa_workspace_bytes(const npa_handle *h, int batch);
size_t npa_state_bytes(const npa_handle *h, int batch);
/* Byte offsets inside the workspace of the arrays a caller may look at BETWEEN npa_forward_iter calls (stream-ordered),
 * out[0..n), n <= 9: the working nominal cur_s [B][3][T+1], cur_u [B][2][T], cur_d [B][T], and the sorted rows the last
 * selection launch emitted -- mu [B][T+1][M][E], lam [B][T+1][M][2], pts [B][T+1][M][2], dist [B][T+1][M], count [B][T+1]
 * (int32): the layout of npa_dune_stage's outputs, so a gradient pass can reuse them instead of re-running the stage.
 * n = 9 adds out[8], the dispatch-order block of the QP launches (int32; diagnostics): cnt [K][32] -- per QP launch of the
 * forward call, how many scenes it filed under each class of iteration counts (class c: 31 - c iterations, clamped) --, then
 * list [2][32][B] -- the scenes of each class, ping-pong by launch parity --, then ticket [B], the workgroup a scene was last
 * solved under.  Launch j hands its scenes out in the order of row j - 1's lists, the longest solves first; a handle created
 * with NPA_QP_ORDER=0 in the environment uses scene order and files nothing (the results are the same bits either way). */
int npa_workspace_layout(const npa_handle *h, int batch, size_t *out, int n);
/* Byte offset inside the workspace of the per-scene QP diagnostics written by the last NRMP launch
 * of npa_forward_batch: [B][16] doubles per scene:
 *   [0] iteration of the iterate that was kept   [1] its merit (max of the scaled KKT residuals and the gap)   [2] last mu
 *   [3] solver status: 0 converged, 2 non-finite data, 3 factorisation lost positive definiteness above 1e-11,
 *       4 ended above 1e-9 after both cold attempts
 *   [4] interior-point iterations of the last attempt   [14] iterations over all attempts of the solve
 *   [15] how the solve started: 0 cold, 1 from the previous PAN iteration's solution (warm), 2 / 3 a warm attempt refused at
 *       iteration 0 / dropped at iteration 6 and restarted cold, 4 a warm attempt that ended above 1e-10 and was repeated
 *       cold, 5 a cold attempt that jammed and was repeated from unit multipliers
 *   [5..13] per-phase cycle counters of the -DNPA_QP_PROF builds (0 otherwise). */
size_t npa_workspace_qp_info_offset(const npa_handle *h, int batch);

/* Replaces PAN.forward (pan.py:109-147) for `batch` independent scenes:
 *   K x { generate_point_flow (pan.py:150-212) -> DUNE.forward (dune.py:58-127) ->
 *         NRMP.forward (nrmp.py:114-150, robot.py:239-316, the QP of nrmp.py:263-383) ->
 *         stop_criteria (pan.py:215-243) }.
 * Inputs  nom_s [B][3][T+1], nom_u [B][2][T], ref_s [B][3][T+1], ref_us [B][T],
 *         points [B][2][n_stride] (global frame), velocities same shape or NULL,
 *         n_points [B] int32 (0 = no obstacle points for that scene; values outside [0, n_stride] are clamped
 *         into it by the kernels) or NULL meaning every scene has n_stride points.  Point sets larger than dune_max_num
 *         are decimated in-kernel exactly like util.downsample_decimation (util:285-305).
 * Outputs out_s [B][3][T+1], out_u [B][2][T], out_d [B][T] (undefined when nrmp_max_num=0),
 *         out_min_distance [B] (DUNE.min_distance, dune.py:97-98; +inf without points),
 *         out_iters [B] int32 iterations executed, out_nrmp_points [B][2][M] or NULL
 *         (NRMP.obstacle_points, nrmp.py:135-138).
 * Inputs are not modified.  Everything is enqueued on `stream`. */
int npa_forward_batch(npa_handle *h, int batch, int n_stride,
                      const float *nom_s, const float *nom_u, const float *ref_s, const float *ref_us,
                      const float *points, const float *velocities, const int32_t *n_points,
                      float *out_s, float *out_u, float *out_d, float *out_min_distance,
                      int32_t *out_iters, float *out_nrmp_points,
                      void *workspace, size_t workspace_bytes, void *state, size_t state_bytes,
                      void *stream);

/* npa_forward_batch with the flags of npa_forward_begin (NPA_FWD_RESET_STATE): one call per step of a serving loop. */
int npa_forward_batch_flags(npa_handle *h, int batch, int n_stride,
                            const float *nom_s, const float *nom_u, const float *ref_s, const float *ref_us,
                            const float *points, const float *velocities, const int32_t *n_points,
                            float *out_s, float *out_u, float *out_d, float *out_min_distance,
                            int32_t *out_iters, float *out_nrmp_points,
                            void *workspace, size_t workspace_bytes, void *state, size_t state_bytes,
                            void *stream, int flags);

/* npa_forward_batch == npa_forward_begin + iter_num x npa_forward_iter(k) + npa_forward_end, all enqueued on `stream`.
 * The split lets a caller look at the working nominal between PAN iterations (it sits at the head of the workspace:
 * cur_s [B][3][T+1], then cur_u [B][2][T] at the next 16-byte boundary).  Same arguments as npa_forward_batch; buffers
 * must stay valid until the enqueued work has completed.  Independent batches overlap by running on different
 * streams, one handle each.
 * flags: NPA_FWD_RESET_STATE zeroes the stop criterion's state buffer first (a fresh planner), inside the staging launch. */
#define NPA_FWD_RESET_STATE 2
int npa_forward_begin(npa_handle *h, int batch, int n_stride,
                      const float *nom_s, const float *nom_u, const float *ref_s, const float *ref_us,
                      const float *points, const float *velocities, const int32_t *n_points,
                      float *out_s, float *out_u, float *out_d, float *out_min_distance,
                      int32_t *out_iters, float *out_nrmp_points,
                      void *workspace, size_t workspace_bytes, void *state, size_t state_bytes,
                      void *stream, int flags);
int npa_forward_iter(npa_handle *h, int k);
int npa_forward_end(npa_handle *h);
/* A burst of n INDEPENDENT forward calls -- n planners of the reference (one PAN.forward each, pan.py:109-147), one handle, one
 * stream and one argument set per call -- enqueued BREADTH-FIRST: the staging launch of every call, then PAN iteration 0 of
 * every call, then iteration 1, ...  The launches and the results are those of n npa_forward_batch_flags calls in a row;
 * what changes is the order in which the host enqueues them: issued call by call, the last of 20 chains starts ~1.8 ms
 * after the first (420 launches later) and a short burst is mostly that ramp; issued breadth-first every chain is running
 * after the first 2 n launches.  The handles must be distinct (a handle plans one batch at a time).  iter_num = PAN iterations
 * of that call, 1 .. the handle's iter_num (the reference's PAN.iter_num is an attribute its callers may lower between
 * calls).  On an error the calls already begun are ended and the error is returned; work enqueued before it stays enqueued. */
typedef struct npa_forward_call {
  npa_handle *h;
  int32_t batch, n_stride, iter_num;
  const float *nom_s, *nom_u, *ref_s, *ref_us, *points, *velocities;
  const int32_t *n_points;
  float *out_s, *out_u, *out_d, *out_min_distance;
  int32_t *out_iters;
  float *out_nrmp_points;
  void *workspace;
  size_t workspace_bytes;
  void *state;
  size_t state_bytes;
  void *stream;
} npa_forward_call;
int npa_forward_batch_group(int n, const npa_forward_call *calls, int flags);
/* MERGED LAUNCHES.  Calls of a group that share ONE stream, a batch size and a configuration (same npa_config, geometric
 * keys, T = 10 or 20 with M = 10, E = 4 or 8) run every stage of theirs as ONE launch over all their scenes, in runs of
 * <= 8 calls: blockIdx.y = the call, the kernels' statements and every result bitwise those of the call-by-call form.  A
 * launch is a barrier over its scenes (the chain goes on when its slowest scene is done): merged, the wave slots a
 * straggler leaves idle are refilled from the same launch and the run occupies one hardware queue instead of one per
 * call.  Same ownership rules: every call keeps its own handle, tensors, workspace and planner state.
 * npa_forward_group_merged: 1 when npa_forward_batch_group(n, calls, .) would run calls[0..n) as ONE merged run, else 0
 * (different streams / batch sizes / configurations, network keys, n < 2 or n > 8, NPA_GROUP_MERGE=0 in the environment). */
int npa_forward_group_merged(int n, const npa_forward_call *calls);

/* Stage entry points (used by the parity tests and for profiling one stage alone).
 * npa_dune_stage  = generate_point_flow + DUNE.forward + the top-M gather:
 *   mu_sorted [B][T+1][M][E], lam_sorted [B][T+1][M][2], pts_sorted [B][T+1][M][2],
 *   dist_sorted [B][T+1][M], count [B][T+1] (= min(N,M); rows >= count replicate row 0).
 * npa_nrmp_stage  = generate_state_parameter_value + generate_coefficient_parameter_value
 *   + the QP solve, from those arrays; writes s,u,d plus qp_info [B][16] doubles
 *   (best iteration, final merit, mu, status, iterations run; rest reserved for profiling builds), and, when x64 is
 *   not NULL, the fp64 solution before the cast to fp32 (nrmp.py:145-148): x64 [B][3T] = u_0x, u_0y, ..., u_(T-1)y,
 *   d_0..d_(T-1) -- what an optimality certificate should be computed on. */
int npa_dune_stage(npa_handle *h, int batch, int n_stride, const float *nom_s,
                   const float *points, const float *velocities, const int32_t *n_points,
                   float *mu_sorted, float *lam_sorted, float *pts_sorted, float *dist_sorted,
                   int32_t *count, void *stream);
int npa_nrmp_stage(npa_handle *h, int batch, const float *nom_s, const float *nom_u,
                   const float *ref_s, const float *ref_us, const float *mu_sorted,
                   const float *lam_sorted, const float *pts_sorted, const int32_t *count,
                   float *out_s, float *out_u, float *out_d, double *qp_info, double *x64, void *stream);

/* npa_nrmp_params = the parameter build of npa_nrmp_stage alone, for parity tests: what generate_state_parameter_value
 * (robot.py:239-316: A_t, B_t, C_t of the linearised model) and generate_coefficient_parameter_value (nrmp.py:220-261:
 * fa, fb of the hinge rows, slice t+1 of the sorted DUNE output, padding rule nrmp.py:258-259) hand to the solver, in
 * fp32 exactly as the kernel built them (they never leave LDS otherwise):
 *   out_abc [B][T][11]: A[0][2] A[1][2] B[0][0] B[0][1] B[1][0] B[1][1] B[2][0] B[2][1] C[0] C[1] C[2]
 *                       (A's other entries are those of the identity);
 *   out_f   [B][T][M][3]: fa[.,0], fa[.,1], fb (NULL allowed when nrmp_max_num == 0). */
int npa_nrmp_params(npa_handle *h, int batch, const float *nom_s, const float *nom_u, const float *mu_sorted,
                    const float *lam_sorted, const float *pts_sorted, const int32_t *count, float *out_abc,
                    float *out_f, void *stream);

/* npa_nrmp_backward = npa_nrmp_stage + the gradient of a scalar loss L(opt_s, opt_u, opt_d) w.r.t. the
 * adjust parameters.  Replaces what cvxpylayers provides in the reference (the adjust parameters are
 * created with requires_grad=True, neupan/blocks/nrmp.py:79-95; the layer is differentiated at
 * nrmp.py:144; example/LON/LON_corridor.py:94-127 trains p_u, eta, d_max through it): one extra
 * solve with the Newton matrix of the converged interior-point iterate (implicit differentiation of
 * the KKT system).  Covers the direct dependence of THIS solve on (q_s[3], p_u, eta, d_max, d_min),
 * including their appearance in gamma_a = q_s*ref_s and gamma_b = p_u*ref_us (nrmp.py:158-160).
 *   grad_s [B][3][T+1], grad_u [B][2][T], grad_d [B][T] (may be NULL): dL/d(opt_s, opt_u, opt_d);
 *   grad_theta [B][8]: dL/d q_s[0..2], p_u, eta, d_max, d_min, and the solver status (0 = converged);
 *   grad_nom_s [B][3][T+1] (may be NULL): dL/d nom_s as the PROXIMAL CENTRE of this solve (robot.py:178), the one
 *   input besides theta that the reference keeps on its autograd graph between PAN iterations (A/B/C are rebuilt
 *   from python floats, robot.py:272-316; mu under no_grad, dune.py:81; R from python floats, pan.py:207).
 *   Feeding it back as grad_s of the previous iteration's solve (grad_u = 0) chains the gradient through the
 *   whole PAN loop, as PAN.forward_batch_grad does. */
int npa_nrmp_backward(npa_handle *h, int batch, const float *nom_s, const float *nom_u,
                      const float *ref_s, const float *ref_us, const float *mu_sorted,
                      const float *lam_sorted, const float *pts_sorted, const int32_t *count,
                      float *out_s, float *out_u, float *out_d, const float *grad_s,
                      const float *grad_u, const float *grad_d, float *grad_theta,
                      float *grad_nom_s, double *qp_info, void *stream);

/* Timing hook for bench.py: HIP events around every kernel launch of subsequent forward calls (on the stream each
 * launch goes to) and the average per-launch durations in ms: dune_kernel (0 when the handle uses geometric keys:
 * there is no such launch), select_kernel, nrmp_qp_kernel; launches = QP launches timed.  enable=0 turns it off. */
int npa_profile_enable(npa_handle *h, int enable);
int npa_profile_read(npa_handle *h, double *dune_ms_avg, double *select_ms_avg, double *nrmp_ms_avg, int64_t *launches);

/* ---- the two steps in front of PAN.forward (handle-free, stream-ordered) --------------------------
 *
 * npa_nominal_ref_states replaces InitialPath.generate_nom_ref_state (+ motion_predict_model)
 *   neupan/blocks/initial_path.py:68-126, :388-444, called at neupan/neupan.py:117-119:
 *   for each scene the T-step rollout of the previous control (nom_s, nom_u) and the reference
 *   states / gears sampled along its current path curve (ref_s, ref_us).  float64 arithmetic in
 *   the reference's order, float32 outputs in the layout npa_forward_batch consumes
 *   (the reference casts at neupan.py:121).
 *   state [B][3] f64; cur_vel [B][2][T] f32 (PAN's previous opt_u; NULL = zeros, the reference's
 *   first call, neupan.py:73); ref_speed [B] f64; path [rows][4] f64 rows (x, y, theta, gear) of
 *   every scene's CURRENT curve (initial_path.py:446-448), scene b owns rows
 *   curve_off[b] .. curve_off[b]+curve_len[b]-1; point_index [B] (closest_point's result,
 *   :160-181); interval [B] f64 (:56, :139).  The path is not modified (the reference writes
 *   2*pi-equivalent headings back into it, :111-112, :190-192).
 *   The index increment: with fwd = ref_speed * step_time >= interval the reference adds
 *   int(fwd / interval), a Python integer without an upper end, and any index past the curve's end
 *   becomes the last point with gear 0 (:93-101).  Here the quotient is compared in double first: a
 *   quotient >= curve_len - index, or one that is not finite (interval == 0), is that clamp, and only a
 *   smaller one is converted to an integer.  So an interval as small as 1e-10, or the 0.0 an average over
 *   a one-point path gives, is the last point with gear 0 and never an index outside the curve.
 *   Preconditions the ABI cannot check, because the arrays live on the device: curve_len[b] >= 1,
 *   0 <= point_index[b] < curve_len[b], rows curve_off[b] .. curve_off[b]+curve_len[b]-1 inside `path`,
 *   interval[b] >= 0.  Outputs: scene b's rows of nom_s / ref_s [B][3][T+1], nom_u [B][2][T],
 *   ref_us [B][T] and nothing else.
 *
 * npa_scan_to_points replaces neupan.scan_to_point (mode 0, neupan/neupan.py:173-222) and
 *   neupan.scan_to_point_velocity (mode 1, :224-281): range/angle filter, polar -> sensor frame ->
 *   robot frame -> world frame, ordered compaction, down-sampling of the kept list.
 *   ranges [B][beam_stride] f64, beam_vel [B][2][beam_stride] f64 or NULL, n_beams [B] or NULL
 *   (= beam_stride); points / velocities [B][2][out_stride] f32 (velocities may be NULL), count [B]
 *   (0 where the reference returns None).  Beams beyond out_stride kept points are dropped.
 *   n_beams[b] is clamped to [0, beam_stride] (the rule of npa_world_scan, which a closed loop feeds from
 *   the same array): a count of 0 or below gives count[b] = 0, a count above the stride is the scan of
 *   beam_stride beams, and no read leaves scene b's rows.  velocities, when given, is filled in both
 *   modes (zeros without beam_vel).  Columns at or beyond count[b] are not written. */
typedef struct npa_scan_params {
  double angle_min, angle_max;   /* scan["angle_min"], scan["angle_max"]                         */
  double range_min, range_max;   /* scan["range_min"], scan["range_max"]                         */
  double state[3];               /* robot pose x, y, theta                                        */
  double offset[3];              /* scan_offset: sensor pose in the robot frame                   */
  double angle_range[2];         /* beams outside (lo, hi) are dropped                            */
  int32_t down_sample;           /* keep every down_sample-th of the surviving points             */
  int32_t reserved;
} npa_scan_params;

int npa_nominal_ref_states(int batch, int receding, int kinematics, double step_time, double wheelbase,
                           const double *state, const float *cur_vel, const double *ref_speed,
                           const double *path, const int32_t *curve_off, const int32_t *curve_len,
                           const int32_t *point_index, const double *interval, float *nom_s,
                           float *nom_u, float *ref_s, float *ref_us, void *stream);
/* npa_path_progress replaces InitialPath.closest_point + check_curve_arrive as check_arrive runs them
 *   (neupan/blocks/initial_path.py:160-181, :279-287, :247-252; called at neupan/neupan.py:113):
 *   point_index [B] is advanced to the closest of the next `ind_range` path points (first one closer than
 *   close_threshold wins), arrived [B] = 1 when the pose is within arrive_threshold of the curve's last
 *   point and point_index >= len - arrive_index_threshold - 2.  min_dis [B] f32 may be NULL.  Switching
 *   to the next curve / gear stays with the host.  The same device-side preconditions as above:
 *   curve_len[b] >= 1 and 0 <= point_index[b] < curve_len[b] are not checked.  Ties go to the lower index; a distance
 *   equal to close_threshold does not end the search, one equal to arrive_threshold has not arrived. */
int npa_path_progress(int batch, const double *state, const double *path, const int32_t *curve_off,
                      const int32_t *curve_len, int32_t *point_index, double close_threshold, int ind_range,
                      double arrive_threshold, int arrive_index_threshold, float *min_dis, int32_t *arrived,
                      void *stream);
int npa_scan_to_points(int batch, int beam_stride, const double *ranges, const double *beam_vel,
                       const int32_t *n_beams, const npa_scan_params *params, int mode,
                       int out_stride, float *points, float *velocities, int32_t *count,
                       void *stream);

/* ---- the packed input record: host-fed serving loops (handle-free, stream-ordered) ------------------
 *
 * The reference's contract is neupan.forward(state, points): the obstacle cloud arrives from the HOST on every control
 * cycle and is converted to tensors at neupan/neupan.py:123-127 (np_to_tensor; the nominal / reference tensors at :121).
 * Here a cycle's inputs travel as ONE record: a contiguous block of 4-byte words the host builds in pinned memory and ships
 * with one DMA, and npa_ingest_unpack turns its device copy into the tensors npa_forward_batch takes.  fp32 is the wire
 * type because the reference casts to fp32 at exactly this boundary.
 *
 * Sections, in this order, each starting on a 256-byte boundary of the record:
 *   [0] n_points  [B] int32        points of scene b (ragged clouds: 0 .. n_stride)
 *   [1] cloud_off [B] int32        WORD offset of scene b's cloud inside the cloud section
 *   [2] nom_s [B][3][T+1]  [3] nom_u [B][2][T]  [4] ref_s [B][3][T+1]  [5] ref_us [B][T]   fp32, npa_forward_batch's layouts
 *   [6] the cloud section: scene b owns the words cloud_off[b] .. cloud_off[b] + c n_b - 1 (c = 2, or 4 with velocities):
 *       x[n_b], y[n_b] (, vx[n_b], vy[n_b]).  Clouds sit back to back -- the exclusive prefix sums of c n_b -- with no
 *       padding to the stride and no alignment beyond the word; only the words in use need to be uploaded.
 * npa_ingest_layout: out[0..n), n <= 8 = the byte offsets of sections [0] .. [6] and, out[7], the worst-case bytes of a
 *   record (every scene at n_stride points): the size of a record buffer.  NPA_E_ARG when the cloud section would exceed
 *   2^31 words.
 * npa_ingest_unpack (csrc/ingest.hip, one launch on `stream`): record = DEVICE copy of a record (4-byte aligned; 16-byte
 *   accesses are taken where a cloud's source and destination both allow), record_bytes = the bytes of it that were
 *   uploaded, a multiple of 4 with out[6] <= record_bytes <= out[7].  Writes nom_s, nom_u, ref_s, ref_us, n_points [B] and
 *   columns [0, n_b) of points [B][2][n_stride] (and of velocities, same shape, when with_velocities != 0); columns beyond
 *   n_b are NOT written (the selection kernel bounds its reads by n_points).
 *   A malformed header never causes an out-of-range access: a scene with n_b < 0, n_b > n_stride, or a cloud that does not
 *   lie inside [0, (record_bytes - out[6]) / 4) words gets n_points = 0 (it is planned without obstacle points), status[0]
 *   is incremented and status[1] lowered to the scene's index (atomic add / min on a DEVICE int32 pair the caller
 *   initialises to {0, INT32_MAX} and reads when it wants to); the other scenes are unaffected. */
int npa_ingest_layout(int batch, int receding, int n_stride, int with_velocities, size_t *out, int n);
int npa_ingest_unpack(int batch, int receding, int n_stride, int with_velocities,
                      const void *record, size_t record_bytes,
                      float *nom_s, float *nom_u, float *ref_s, float *ref_us,
                      float *points, float *velocities, int32_t *n_points, int32_t *status, void *stream);

/* ---- exact clearance of a plan against the full cloud (stream-ordered, one launch) --------------------
 *
 * The reference's safety signal is min_distance: the NETWORK's distance at horizon step 0 over the cloud after decimation
 * to dune_max_num points (dune.py:98; the decimation and the point flow: pan.py:171-212), compared with
 * collision_threshold by check_stop (neupan.py:169-170); info["collision"] is declared (neupan.py:86) and never set.
 * npa_plan_clearance (csrc/clearance.hip) is the independent check: the closed-form distance of the robot polygon to EVERY
 * point of the cloud at every step of a trajectory.  For scene b, step t = 0..T, point n < n_points[b]:
 *     q = p_n + t dt v_n (pan.py:182),  p0 = R(theta_t)^T (q - s_t[0:2]) (pan.py:205-210),
 *     d = the distance of p0 to the polygon: outside, the smallest point-segment distance over the edges; inside, the largest
 *         signed distance to an edge line (<= 0: minus the penetration depth).
 * traj_s [B][3][T+1] (T = the handle's receding: opt_s, or any other trajectory of that shape); points, velocities
 * [B][2][n_stride] and n_points [B] as npa_forward_batch takes them (velocities null: static points; n_points null: every scene
 * has n_stride points; n_points[b] is clamped to [0, n_stride]).  ALL n_points[b] points count -- dune_max_num does not
 * apply -- and columns at or beyond n_points[b] are never read.
 * Outputs: clearance [B][T+1] = min_n d (+inf for a scene without points), nearest [B][T+1] = the smallest n that attains it
 * (-1 without points); min_clearance [B] = min_t clearance, first_violation [B] = the smallest t with clearance < threshold,
 * -1 if there is none (either of the two may be null).  fp32 arithmetic; deterministic (no atomics: the result does not
 * depend on the order of the reduction).  No workspace, no allocation, no host synchronisation.
 * NPA_E_ARG: a null handle or required pointer, batch <= 0, n_stride <= 0, a pointer that is not 4-byte aligned (16-byte
 *   loads are taken where a scene's rows allow them) -- checked before anything touches a device.
 * NPA_E_UNSUPPORTED: the handle's G, h rows are not consecutive counter-clockwise edges (no vertices: npa_geo_report). */
int npa_plan_clearance(npa_handle *h, int batch, int n_stride, const float *traj_s, const float *points,
                       const float *velocities, const int32_t *n_points, float threshold,
                       float *clearance, int32_t *nearest, float *min_clearance, int32_t *first_violation,
                       void *stream);

/* ---- a lidar world on the device: ray-cast scans and the plant step of a closed loop (csrc/world.hip) -----------------
 *
 * The reference closes its loop through a simulator (example/run_exp.py: env.get_lidar_scan() -> scan_to_point ->
 * neupan_planner(...) -> env.step(action)).  These two calls are that simulator's part for B robots, handle-free and
 * stream-ordered: no workspace, no atomics, no host synchronisation.
 *
 * The world, float64 DEVICE arrays:
 *   circles  [W][c_stride][6]  cx, cy, r, vx, vy, 0          segments [W][s_stride][6]  ax, ay, bx, by, vx, vy
 *   n_circles [W], n_segments [W] int32 (clamped to their strides; entries at or beyond them are never read).
 *   W = n_worlds is 1 (one world shared by every scene) or batch (scene b has world b).  Polygons and rectangles are their
 *   edges.  Primitive indices: circles 0 .. C-1, segments C .. C+S-1 with C = n_circles[w].
 *
 * npa_world_scan (one launch): beam i < n_beams[b] of scene b starts at the sensor pose state o offset of params[b]
 *   (composed as npa_scan_to_points composes them; used fields: state, offset, angle_min, angle_max, range_min, range_max --
 *   angle_range and down_sample belong to npa_scan_to_points) at the angle numpy.linspace(angle_min, angle_max, n)[i], bit
 *   for bit the value npa_scan_to_points uses.  ranges [B][beam_stride] = the smallest t >= 0 at which the ray meets a
 *   primitive -- circle: the near root (a tangent ray hits), 0 when the origin is inside or on it, whichever way the ray
 *   points; segment: the ray / segment intersection with the segment parameter in [0, 1], both ends included; parallel and
 *   collinear rays and segments of zero length miss --, ties to the lowest primitive index.  The range is never -0.
 *   A smallest t at or above range_max, or no hit: ranges = range_max exactly, hit = -1, velocity 0.  Hits below range_min
 *   are reported as they are.
 *   beam_vel [B][2][beam_stride] (nullable) = (vx, vy) of the primitive hit, hit [B][beam_stride] int32 (nullable) its index.
 *   Columns at or beyond n_beams[b] (null: beam_stride) are not written.  skip [B][2] int32 (nullable): scene b's beams
 *   ignore the SEGMENT indices skip[b][0] <= s < skip[b][1] (a robot's own edges, below).
 *   Primitives are culled against the sensor's reach and cast in chunks of npa_world_list_capacity(); the result does not
 *   depend on the chunking, and a scene's result does not depend on the batch it is in.
 *
 * npa_world_step (two launches; one when clearance is null):
 *   1. plant: state [B][3] f64 is advanced in place by action [B][2] f32 over dt unless frozen[b] != 0 (frozen nullable).
 *      diff and acker: motion_predict_model (initial_path.py:388-432) in the float32 / float64 mix of
 *      npa_nominal_ref_states; omni: the action is (vx, vy) as neupan.forward returns it (neupan.py:158-164),
 *      x += dt vx, y += dt vy in float64, heading unchanged.
 *   2. world: every primitive with a non-zero velocity is translated by v dt, once per step.  bounds (HOST, xlo, ylo, xhi,
 *      yhi; nullable): a moving circle whose centre has left the box (a centre on a wall has not) gets the offending velocity
 *      component turned back inside; segments and circles at rest are not turned.
 *   3. peers (peer_base >= 0, n_worlds == 1): the edge_num edges of robot b's polygon (vertices: HOST [E][2] f64, robot
 *      frame, counter-clockwise) at its new pose are written to segments[peer_base + b E + e], their velocity the robot's
 *      displacement of this step / dt (0 when dt == 0).  With skip[b] = [peer_base + b E, peer_base + (b + 1) E) the robots
 *      see each other in the next scan as moving obstacles.  The caller sizes n_segments to include this tail; the tail is
 *      not translated by 2.
 *   4. clearance [B] f64 (nullable): the exact signed distance of robot b's polygon at its new pose to the nearest primitive
 *      of its world, its own edges excluded; +inf without primitives.  Circle: distance(centre, polygon) - r, the polygon
 *      distance negative inside as in npa_plan_clearance.  Segment: 0 when it crosses an edge or has an end inside the
 *      polygon, else the smaller of its ends' polygon distances and the vertices' point-segment distances.  <= 0: collided.
 * NPA_E_ARG (before anything touches a device): a null required pointer, batch <= 0, n_worlds not in {1, batch}, dt < 0,
 *   edge_num outside [3, NPA_MAX_E], peers or clearance without vertices, peers with n_worlds != 1 or a tail beyond s_stride. */
int npa_world_list_capacity(void);
int npa_world_scan(int batch, int n_worlds, int c_stride, int s_stride, const double *circles, const double *segments,
                   const int32_t *n_circles, const int32_t *n_segments, const npa_scan_params *params,
                   const int32_t *n_beams, int beam_stride, const int32_t *skip,
                   double *ranges, double *beam_vel, int32_t *hit, void *stream);

/* npa_world_scan_noisy (one launch): npa_world_scan with Gaussian bearing and range noise, drawn on the device by the
 *   counter-based generator of npa_world_behave.  IR-SIM's lidar2d has the switches noise / std / angle_std; its code was
 *   not available to compare with, so this specification is the project's own.
 *   Generator.  mix is the splitmix64 finaliser of npa_world_behave; all integer arithmetic is 64-bit wrap-around:
 *       z = mix(mix(mix(mix(seed + scene) + beam) + draw) + k),   U(seed, scene, beam, draw, k) = (z >> 11) * 2^-53
 *       g(k0) = sqrt(-2 ln(1 - U(.., k0))) * cos(2 pi U(.., k0 + 1))     (float64; 1 - U is in (0, 1], so |g| < 8.6)
 *       g_a = g(0),  g_r = g(2)
 *   The integer part is exact.  ln and cos may differ in the last bits between the host's libm and the device library
 *   (the device evaluates cospi(2 U)); whatever must be bit-equal between two runs is computed by this one kernel.
 *   Beam i of scene b uses scene = scene_base + b, beam = i and the call's `draw`.  It is cast along
 *       ang' = ang + angle_std * g_a          (one multiply, one add, no contraction; ang is npa_world_scan's, bit for bit)
 *   and the cast is npa_world_scan's: same forms, same tie rule, same culling, same skip.  hit and beam_vel are that cast's.
 *   A beam that hit (hit >= 0):  ranges = min(max(t + std * g_r, 0) + 0, range_max);  a miss: ranges = range_max exactly,
 *   without noise (a noisy miss never becomes a phantom point).  The range is reported at the NOMINAL beam i:
 *   npa_scan_to_points keeps using the nominal angle -- that is what bearing noise means.
 *   With std == 0 and angle_std == 0 the three outputs are npa_world_scan's bit for bit.  A scene's result does not depend
 *   on the batch (given scene_base), on n_beams of other scenes, or on the chunking.
 *   Not IR-SIM's: the generator (IR-SIM draws from numpy's global stream), the clamp to [0, range_max], misses without noise.
 * NPA_E_ARG (before anything touches a device): everything npa_world_scan refuses; std or angle_std negative or not
 *   finite; draw < 0; scene_base < 0 (or scene_base + batch beyond an int).
 *
 * npa_scan_noise_draws (HOST, no device): out [n][2] f64 = (g_a, g_r) of the beams first_beam .. first_beam + n - 1 of
 *   `scene` and `draw`.  NPA_E_ARG: scene, draw, first_beam or n negative, a null out. */
int npa_world_scan_noisy(int batch, int n_worlds, int c_stride, int s_stride, const double *circles, const double *segments,
                         const int32_t *n_circles, const int32_t *n_segments, const npa_scan_params *params,
                         const int32_t *n_beams, int beam_stride, const int32_t *skip,
                         double *ranges, double *beam_vel, int32_t *hit,
                         double std, double angle_std, uint64_t seed, int scene_base, int draw, void *stream);
int npa_scan_noise_draws(uint64_t seed, int scene, int draw, int first_beam, int n, double *out);

int npa_world_step(int batch, int n_worlds, int c_stride, int s_stride, double *circles, double *segments,
                   const int32_t *n_circles, const int32_t *n_segments, double *state, const float *action,
                   const int32_t *frozen, double dt, int kinematics, double wheelbase, const double *bounds,
                   int edge_num, const double *vertices, int peer_base, double *clearance, void *stream);

/* ---- reactive obstacles: agents of the lidar world that choose their own velocity (csrc/behave.hip) --------------------
 *
 * The method is the sampled penalty of J. van den Berg, M. Lin, D. Manocha, "Reciprocal Velocity Obstacles for Real-Time
 * Multi-Agent Navigation", ICRA 2008: every agent takes, of a table of candidate velocities v', the one with the lowest
 * w / tc(v') + |v_pref - v'|, tc the time to the first collision if every neighbour kept its share of the avoidance.  This
 * comment is the specification (tests/behave_ref.py restates it in numpy).  Handle-free, stream-ordered: no workspace, no
 * atomics, no host synchronisation; float64 in the operation order written here, no FMA contraction.
 *
 * An AGENT is a primitive, or a run of primitives, of a world: a circle agent owns one circle, a polygon agent `count`
 * consecutive segments.  Two DEVICE tables per world, with a row stride and counts like the primitives':
 *   agents    [W][a_stride][NPA_AGENT_DOUBLES] f64   0 gx  1 gy (the goal)   2 vx  3 vy (the velocity chosen by the last call)
 *                                                    4 ox  5 oy: centre - anchor, the anchor being the circle's centre or end a
 *                                                    of the first segment (constant under translation: the centre is never
 *                                                    stored)   6 R (bounding radius about the centre)   7 v_max
 *                                                    8 goal_threshold   9 the index of the candidate chosen by the last call
 *   agent_idx [W][a_stride][NPA_AGENT_INTS] int32    0 first primitive (the world's numbering: circles, then segments)
 *                                                    1 count (1 for a circle)   2 wander (0 / 1)   3 draws (uint32: wander
 *                                                    goals drawn so far, modulo 2^32)
 *   n_agents  [W] int32 (clamped to a_stride).  A row whose primitives do not exist (first < 0, count < 1, a circle with
 *   count != 1, a run beyond n_segments) is no agent: it is neither moved nor anybody's neighbour.  Runs must not overlap.
 * npa_behave_params (HOST): weight (the w of the penalty, > 0), horizon (seconds, > 0), robot_share (in (0, 1]),
 *   range_low / range_high (the box wander goals are drawn from), seed, world_base (added to the world's index in the
 *   generator, so that a world computes the same whichever batch it is in).
 *
 * npa_world_behave (two launches).  Per agent A: centre p = anchor + (ox, oy); v_A = the velocity columns of its first
 * primitive (the velocities of the cycle before: launch 1 writes agent rows only).
 *   1. d = g - p, L = sqrt(dx dx + dy dy); arrived: L <= goal_threshold.  Arrived with wander: a new goal is drawn, draws += 1,
 *      d and L are recomputed (no second arrival test).  Arrived without wander, or L == 0: v_pref = 0 (goal and draws
 *      untouched).  Otherwise s = min(v_max, L / dt), v_pref = ((dx / L) s, (dy / L) s).
 *      The generator: mix(z) = { z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) 0xBF58476D1CE4E5B9; z = (z ^ z >> 27)
 *      0x94D049BB133111EB; z ^ z >> 31 } on uint64; z = mix(mix(mix(mix(seed + world_base + w) + first) + draw) + coordinate),
 *      coordinate 0 for x and 1 for y, draw = `draws` before the increment; u = (z >> 11) 2^-53, g = lo + (hi - lo) u.  The
 *      agent is named by its first primitive, not by its row.
 *   2. candidates: 0 = (0, 0); 1 = v_pref; 2 = v_A, times v_max / |v_A| when |v_A| > v_max; 3 + j n_dir + k =
 *      (s_j dirs[k].x, s_j dirs[k].y), s_j = (v_max (j + 1)) / n_speed, j < n_speed, k < n_dir.  dirs [n_dir][2] f64 DEVICE: unit
 *      directions tabulated by the caller.  3 + n_speed n_dir <= npa_behave_max_candidates().
 *   3. neighbours, each with the share alpha of the avoidance A takes: apex = (1 - alpha) v_A + alpha v_B, relative velocity
 *      u = (v' - apex) (1 / alpha).
 *        another agent of the world      alpha = 1/2          disc of radius R_A + R_B at its centre
 *        a circle no agent owns          alpha = 1            disc of radius R_A + r
 *        a segment no agent owns, index below seg_limit (seg_limit < 0: all)
 *                                        alpha = 1            the capsule: discs of radius R_A at both ends and the segment
 *                                                             shifted by +- R_A n, n = (ey, -ex) / |e|, e = b - a
 *        a robot                         alpha = robot_share  disc of radius R_A + robot_radius at state[b]; v_B = (state -
 *                                                             prev_state) / dt, 0 when prev_state is null
 *      An agent of world w sees robot w when n_worlds == batch and all `batch` robots when n_worlds == 1.
 *   4. tc: the ray p + t u against each shape, in npa_world_scan's forms.  Disc, c = centre - p, c2 = |c|^2 - rho^2,
 *      b = c . u: c2 <= 0 (touching): tc = 0 when b > 0, else no collision; otherwise a hit when b > 0 and disc = b^2 - |u|^2 c2
 *      >= 0, tc = c2 / (b + sqrt(disc)).  Segment: the sign-corrected cross-multiplied validity test, then one division.
 *      tc > horizon: no collision.  tc_min = the minimum over the neighbours, +inf without one.
 *   5. cost = weight / tc_min + sqrt((v_pref.x - v'.x)^2 + (v_pref.y - v'.y)^2) (+inf for tc_min = 0); the lowest cost wins,
 *      ties to the lowest index.  Launch 1 writes columns 0 - 3 and 9 of the agent's row and `draws`; launch 2 copies the
 *      chosen velocity into the velocity columns of every primitive the agent owns and touches nothing else.
 *      npa_world_step then translates them as any moving primitive.
 *   Neighbours are culled against horizon (v_max + |apex|) / alpha + rho and cast in chunks of npa_behave_list_capacity();
 *   the result does not depend on the chunking, on the order of the agent rows or on the batch a world is in.
 * NPA_E_ARG (before anything touches a device): a null required pointer (prev_state may be null; dirs when there is no
 *   grid), batch <= 0, a_stride <= 0, n_worlds not in {1, batch}, dt <= 0, weight <= 0, horizon <= 0, robot_share outside
 *   (0, 1], range_low above range_high, robot_radius < 0, more candidates than the cap, strides that do not fit (no
 *   primitives at all, seg_limit beyond s_stride, more rows than a launch addresses), world_base < 0 (or world_base +
 *   n_worlds beyond an int: the generator's world is world_base + w as a uint32, zero-extended). */
#define NPA_AGENT_DOUBLES 10
#define NPA_AGENT_INTS 4
typedef struct npa_behave_params {
  double weight, horizon, robot_share;
  double range_low[2], range_high[2];
  uint64_t seed;
  int32_t world_base, reserved;
} npa_behave_params;
int npa_behave_list_capacity(void);
int npa_behave_max_candidates(void);
int npa_world_behave(int batch, int n_worlds, int c_stride, int s_stride, double *circles, double *segments,
                     const int32_t *n_circles, const int32_t *n_segments, int a_stride, double *agents,
                     int32_t *agent_idx, const int32_t *n_agents, const npa_behave_params *params,
                     const double *state, const double *prev_state, double robot_radius, int seg_limit,
                     int n_dir, const double *dirs, int n_speed, double dt, void *stream);

/* ---- way-point curves: the initial path between two poses (csrc/curves.h, csrc/curves.hip) ----------------------------
 *
 * The reference leaves the curve between two way-points to the third-party gctl package (curve_generator.generate_curve,
 * neupan/blocks/initial_path.py:337-339), which is not part of it; gctl's sampling is therefore NOT what this is compared
 * with.  This comment is the specification (tests/curves_ref.py restates it in numpy); it is taken from the literature: the
 * Dubins words are the normalised closed forms of A. M. Shkel and V. Lumelsky, "Classification of the Dubins set", Robotics
 * and Autonomous Systems 34 (2001) 179-202.  Reeds-Shepp curves (48 words, several gears) are not generated.
 * One definition in float64, compiled for the host and for the device (csrc/curves.h); every arithmetic statement below is one
 * rounded operation in the order written (no contraction), so two device kernels give the same bits and host and device
 * differ only where libm and the device math library do.
 *
 * Inputs: style (NPA_CURVE_LINE, NPA_CURVE_DUBINS), start (x0, y0, th0), goal (x1, y1, th1), interval > 0 and, for Dubins,
 *   the turning radius rho = min_radius > 0.  dx = x1 - x0, dy = y1 - y0, D = sqrt(dx dx + dy dy), psi = atan2(dy, dx).
 * Rows: (x, y, theta, gear = +1).  With the curve's length L: L == 0 gives ONE row, the goal pose (x1, y1, th1).  Otherwise
 *   n = max(ceil(L / interval - 1e-9), 1) (planner.line_curve's rule), rows i = 0 .. n-1 lie at arc length i L / n and row n is
 *   the goal: n + 1 rows.  A curve of 2^30 steps or more, or one whose length is not finite, is no curve.
 * Line: L = D; row i < n is (x0 + f dx, y0 + f dy) with f = i / n; theta of EVERY row, row n included, is psi (what the
 *   reference's _ensure_consistent_angles, initial_path.py:476-497, makes of a segment); th0 and th1 are not used.
 * Dubins: mod2pi(x) = x - 2 pi floor(x c), c = 0.15915494309189535 (1 / (2 pi)), moved into [0, 2 pi) by one addition or
 *   subtraction of 2 pi when rounding left it outside.  d = D / rho, alpha = mod2pi(th0 - psi), beta = mod2pi(th1 - psi), sa = sin alpha, sb = sin beta,
 *   ca = cos alpha, cb = cos beta, cab = ca cb + sa sb.  D == 0 with alpha == beta: L = 0.  Otherwise the six words, in this
 *   order, each (t, p, q) in radii, each with a direction (ya, xa):
 *     0 LSL  p2 = 2 + d d - 2 cab + 2 d (sa - sb)    (ya, xa) = (cb - ca, d + sa - sb)     t = mod2pi(u - alpha)     q = mod2pi(beta - u)
 *     1 LSR  p2 = -2 + d d + 2 cab + 2 d (sa + sb)   (ya, xa) = (-ca - cb, d + sa + sb)    t = mod2pi(u - alpha)     q = mod2pi(-(beta - u))
 *     2 RSL  p2 = -2 + d d + 2 cab - 2 d (sa + sb)   (ya, xa) = (ca + cb, d - sa - sb)     t = mod2pi(-(u - alpha))  q = mod2pi(beta - u)
 *     3 RSR  p2 = 2 + d d - 2 cab + 2 d (sb - sa)    (ya, xa) = (ca - cb, d - sa + sb)     t = mod2pi(-(u - alpha))  q = mod2pi(-(beta - u))
 *            p = sqrt(p2); infeasible when p2 < -1e-12, a p2 in [-1e-12, 0) counts as 0.  LSL, RSR: u = atan2(ya, xa).  LSR, RSL:
 *            the paper's atan2(ya, xa) - atan2(yb, p), yb = -2 for LSR and +2 for RSL, as ONE atan2 of the quotient of the two
 *            directions: u = atan2(ya p - xa yb, xa p + ya yb) (the same angle modulo 2 pi, which is all mod2pi keeps)
 *     4 RLR  a = (6 - d d + 2 cab + 2 d (sa - sb)) / 8   (ya, xa) = (ca - cb, d - sa + sb)   u = atan2(ya, xa)
 *            p = mod2pi(2 pi - acos a)   t = mod2pi(p / 2 - u + alpha)   q = mod2pi(-(beta - alpha) - t + p)
 *     5 LRL  a = (6 - d d + 2 cab - 2 d (sa - sb)) / 8   (ya, xa) = (ca - cb, d + sa - sb)   u = atan2(ya, xa)
 *            p = mod2pi(2 pi - acos a)   t = mod2pi(p / 2 - u - alpha)   q = mod2pi((beta - alpha) - t + p)
 *            infeasible when a is outside [-1, 1] by more than 1e-12; inside that margin it is clamped
 *   The word with the smallest t + p + q wins, ties to the lowest index; L = rho (t + p + q).
 *   A segment of type k (L: +1, S: 0, R: -1) carries a pose (x, y, h) over the length l (in radii) to
 *     k == 0: (x + rho (l cos h), y + rho (l sin h), h);   else with e = h + k l: (x + rho (k (sin e - sin h)), y - rho (k (cos e - cos h)), e).
 *   The poses at the start of the three segments follow from the start pose by that rule with l = t, then l = p (the heading is
 *   not wrapped).  Row i < n: s = (i (t + p + q)) / n; segment 0 when s < t, 1 when s < t + p, else 2; the row is that segment's
 *   start pose carried over s, s - t or s - (t + p).  Row 0 is therefore the start pose, bit for bit; row n is (x1, y1, th1) as
 *   given (its heading may differ from the heading the curve arrives with by a multiple of 2 pi).
 *
 * npa_curve_rows (HOST, no device): the number of rows, n + 1, or a negative error.
 * npa_curve_generate (HOST, no device): rows_out [capacity][4] f64 and *n_rows; a curve that does not fit `capacity` is
 *   NPA_E_ARG and nothing is written.
 * npa_curve_batch (one launch, one wave per curve, no workspace, no atomics, nothing allocated): B curves of one style and
 *   radius; start, goal [B][3] f64, interval [B] f64, rows_out [B][capacity][4] f64, n_rows [B] int32, mask [B] int32
 *   (nullable), all DEVICE.  Every lane evaluates the same six words; lane l writes rows l, l + 64, ...  A curve that needs
 *   more than `capacity` rows: n_rows[b] = -needed, its rows untouched.  Inputs outside the specification (interval not > 0,
 *   a pose that is not finite, 2^30 steps or more): n_rows[b] = 0, its rows untouched.  mask[b] == 0: rows and n_rows[b] untouched.
 * NPA_E_ARG (before anything touches a device): a null required pointer, style outside 0..1, Dubins with min_radius <= 0,
 *   capacity < 1, batch < 1; the host calls also: interval not > 0, a pose that is not finite. */
#define NPA_CURVE_LINE 0
#define NPA_CURVE_DUBINS 1
int npa_curve_rows(int style, const double *start, const double *goal, double interval, double min_radius);
int npa_curve_generate(int style, const double *start, const double *goal, double interval, double min_radius,
                       int capacity, double *rows_out, int32_t *n_rows);
int npa_curve_batch(int batch, int style, const double *start, const double *goal, const double *interval,
                    double min_radius, int capacity, const int32_t *mask, double *rows_out, int32_t *n_rows,
                    void *stream);

/* ---- goal fields: the cost-to-goal of every cell of an occupancy map (csrc/cycle.hip, csrc/curves.hip) -----------------
 *
 * The curves above know no walls.  An initial path through a map follows the cost-to-goal field of its goal downhill
 * (neupan_amd/route.py, in PyTorch); the field itself, one shortest-path relaxation over every cell of the map and shared by
 * every robot that drives to that goal, is this call.  The reference has nothing of the kind; this comment is the
 * specification (tests/route_ref.py restates it as a heap Dijkstra on Python integers).
 *
 * Inputs: blocked [ny][nx] uint8, DEVICE, cell (i, j) at blocked[j nx + i], non-zero = not traversable.  Everything OUTSIDE
 *   the array is blocked (npa_grid_scan, include/neupan_amd_grid.h, treats the outside as free: a beam may leave the map, a
 *   route may not).  fields [n_fields][ny][nx] uint32, DEVICE, in and out.  changed [n_fields] uint32, DEVICE.
 * Moves: the four axis steps at cost 5, the four diagonal steps at cost 7 (7 / 5 = 1.4 for sqrt 2).  A diagonal step from c
 *   to c + (dx, dy) exists only if c + (dx, 0) and c + (0, dy) are both free: nothing squeezes between two blocked cells that
 *   touch at a corner.  (The rule names the same two cells in both directions, so dist below is symmetric.)
 * Result: with dist(s, c) the cost of the cheapest move sequence from s to c over free cells, the converged field is
 *     d(c) = min over the free cells s with init(s) < NPA_ROUTE_UNREACHED of (init(s) + dist(s, c)),
 *   NPA_ROUTE_UNREACHED where no such s reaches c.  The caller seeds: 0 in the goal cells, NPA_ROUTE_UNREACHED in every other
 *   free cell; several seeds and seeds above 0 are allowed, a free cell's seed is at most NPA_ROUTE_UNREACHED.  The entries of
 *   blocked cells are neither read nor written.  Integer and exact: with at most 2^26 cells a reached value is below 7 2^26
 *   (seeds are the caller's to keep below 2^32 - 7 2^26), so v + 7 cannot wrap; the kernel adds only to values below
 *   NPA_ROUTE_UNREACHED.
 * One sweep is one launch: grid (ceil(nx / 16), ceil(ny / 16), n_fields), 256 threads, under 2 KB of LDS, no workspace, no
 *   atomics.  A workgroup loads its 16 x 16 tile of one field and a one-cell halo into LDS -- blocked cells and cells outside
 *   the array as NPA_ROUTE_BLOCKED --, relaxes the tile there for at most 16 rounds (a round: every thread takes the minimum of
 *   its cell and its eight neighbours plus their move costs; barriers keep a round's reads in front of its writes) and leaves
 *   early after a round in which no cell fell.  A thread whose cell ended lower than it began stores it to `fields` and stores
 *   the sweep's mark, sweep_base + s + 1 for sweep s = 0 .. sweeps - 1 of this call, to changed[f].
 * Why the result is exact, and the same bits in every run, without atomics or a barrier across workgroups:
 *   (1) a cell of `fields` is written by its own thread alone, and only with a lower value;
 *   (2) every value ever held is a seed plus the cost of a real move sequence from it (induction over the writes), so no value
 *       is below d;
 *   (3) a halo cell read while its own tile stores it yields the old or the new aligned 32-bit word, never a mixture: by (2)
 *       either is sound;
 *   (4) a sweep in which no cell fell stored nothing, so every workgroup of it read values nothing wrote meanwhile and found
 *       no cell to lower in its tile (its last round changed nothing): the field is a fixed point of the relaxation;
 *   (5) a fixed point f >= d equals d: along a cheapest move sequence from the minimising seed s to c, f(s) <= init(s), and
 *       f(next) <= f(this) + cost at every move, so f(c) <= d(c).
 *   Hence the converged field is unique -- whatever the timing, whatever `sweeps` per call.  Only the NUMBER of sweeps it took
 *   may differ between runs.  After k sweeps every cell whose cheapest sequence has at most k moves is final (a sweep
 *   relaxes every cell at least once against values at least as low as the previous sweep left), so nx ny + 1 sweeps always
 *   suffice, and every loop of the kernel has a constant bound.
 * The call issues `sweeps` launches on `stream` and does not synchronise.  The fields are converged iff, after the call,
 *   changed[f] < sweep_base + sweeps for every f: the last sweep lowered nothing.  The caller zeroes `changed` once, reads it
 *   after each call and passes the sweeps issued so far as the next sweep_base.
 * NPA_E_ARG (before anything touches a device): blocked, fields or changed null; nx or ny < 1; n_fields outside 1 .. 65535
 *   (a launch's z extent); sweeps < 1; sweep_base + sweeps beyond uint32.  NPA_E_UNSUPPORTED: nx ny > NPA_ROUTE_MAX_CELLS, or
 *   ny > 16 * 65535 (a launch's y extent). */
#define NPA_ROUTE_BLOCKED   0xFFFFFFFFu
#define NPA_ROUTE_UNREACHED 0xFFFFFFFEu
#define NPA_ROUTE_MAX_CELLS (1 << 26)
int npa_route_relax(const uint8_t *blocked, int nx, int ny, int n_fields, uint32_t *fields, int sweeps,
                    uint32_t sweep_base, uint32_t *changed, void *stream);

/* ---- routed curves: a path down a goal field, as `line` curves between its turns (csrc/cycle.hip, csrc/curves.hip) -------
 *
 * The way a robot takes through the map to a goal whose field has converged: route.trace's chain, route.waypoints' positions
 * and planner.generate_curve("line", ...)'s rows (neupan_amd/route.py, neupan_amd/planner.py), in ONE kernel with one wave per
 * robot, route_wave_kernel, without the host: no workspace, no atomics, no LDS, nothing allocated, no cap on the turns.  This
 * comment is the specification (tests/route_wave_ref.py restates it in plain Python).
 *
 * Inputs per robot: a start pose (x, y, theta), a goal (x, y, theta), the index f of the goal's field in fields
 *   [n_fields][ny][nx] uint32 (DEVICE; converged, seeded with 0 in the goal's cell only: GoalFields.fields), the map's frame
 *   x0, y0, resolution (cell (i, j) covers [x0 + i res, x0 + (i + 1) res) x [y0 + j res, y0 + (j + 1) res)), an interval.
 * Start cell: i = floor((x - x0) / res), j = floor((y - y0) / res), each one rounded fp64 operation per step (no contraction).
 * Chain: from a cell of value v > 0 the walk goes to the first neighbour in the order E, W, N, S, NE, NW, SE, SW that lies
 *   inside the array, is not NPA_ROUTE_BLOCKED, for a diagonal has both axis cells beside it inside and not BLOCKED, and holds
 *   exactly v - 5 (axis) or v - 7 (diagonal); it ends at value 0.  Lanes 0 .. 7 load one neighbour each, one ballot is the free
 *   mask, a second the allowed moves, its lowest bit the move.  Every step lowers v: the walk ends on any input.
 * Way-points: the start's (x, y); the centre (x0 + (i + 0.5) res, y0 + (j + 0.5) res) of every cell whose move out differs
 *   from the move in; the goal's own (x, y).
 * Rows: between consecutive way-points a segment whose two ends are equal in both coordinates is skipped; any other is the
 *   NPA_CURVE_LINE curve of the block above at `interval` without its goal row (rows 0 .. n - 1; lane l writes rows l, l + 64,
 *   ...).  The last row is (goal x, goal y, h, 1): h = the psi of the last segment that was not skipped, the goal's theta if all
 *   were.  rows = the sum of the segments' n, plus 1.
 * Nothing is written unless the whole path fits: the walk runs twice, counting and then writing.
 * No route: f outside [0, n_fields); a start cell outside the array (a pose that is not finite is outside); a start value of
 *   NPA_ROUTE_BLOCKED or NPA_ROUTE_UNREACHED; a step with no allowed move (the field is not converged).
 * No curve: a segment outside the curve specification (interval not > 0, a goal that is not finite, 2^30 steps or more), or a
 *   path of 2^31 rows or more.
 *
 * npa_route_curve_batch (one launch): B routed paths.  field_of [B] int32, start, goal [B][3] f64, interval [B] f64, mask [B]
 *   int32 (nullable), rows_out [B][capacity][4] f64, n_rows [B] int32, all DEVICE.  n_rows[b] = rows when 1 <= rows <= capacity
 *   (the rows are written); -rows when rows > capacity (nothing is written); 0 when there is no route; -2^31 when there is no
 *   curve (the count no capacity holds: a caller that maps n_rows < 0 to "does not fit" gives npa_cycle_retask_routed's status).
 *   mask[b] == 0: rows and n_rows[b] untouched, as npa_curve_batch.
 * npa_cycle_retask_routed (one launch, runs where npa_cycle_retask runs; the cycle block below describes that call and its
 *   arguments): the same gate (arrived, not collided, 0 <= goal_index < n_goals), and the path from state[b] to
 *   goals[b][goal_index[b]] down field field_of[b][goal_index[b]] (field_of [B][g_stride] int32) in place of the curve.  It fits:
 *   the same writes and retask_status[b] = 1.  It does not fit row_capacity[b], or no curve: retask_status[b] = 2.  No route:
 *   retask_status[b] = 3.  For 2 and 3 nothing else of the robot is written: it stays arrived and the goal is not consumed.
 *   log_goal as npa_cycle_retask.
 * NPA_E_ARG (before anything touches a device): a null required pointer; batch, capacity or g_stride < 1; nx or ny < 1;
 *   n_fields outside 1 .. 65535; a resolution that is not finite and > 0, an x0 or y0 that is not finite; receding outside
 *   [1, NPA_MAX_T]; cycle < 0.  NPA_E_UNSUPPORTED: nx ny > NPA_ROUTE_MAX_CELLS.
 *
 * Line-of-sight shortcutting: npa_route_curve_batch_los and npa_cycle_retask_routed_los.  The argument lists, refusals,
 *   statuses and counts of the exports they stand beside, the same kernel (a launch argument), and every rule above but the
 *   way-points: those of the chain are CANDIDATES, and a candidate the anchor sees is left out.  tests/route_los_ref.py restates
 *   it.
 * Visibility of two cells a = (i0, j0), b = (i1, j1) inside the array: no cell whose closed box meets the closed segment
 *   between the two cell centres holds NPA_ROUTE_BLOCKED (NPA_ROUTE_UNREACHED does not block).  Those cells in integers: dx =
 *   i1 - i0, dy = j1 - j0, the axes' roles swapped if |dy| > |dx|; ax = |dx|, ay = |dy|, sx, sy the signs.  Column c = 0 .. ax
 *   of the major axis holds the minor offsets m = max(lo, 0) .. min(hi, ay) with
 *       lo = ceil(((2c - 1) ay - ax) / (2 ax)),   hi = floor(((2c + 1) ay + ax) / (2 ax))
 *   (ax == 0: the one cell), the cell (i0 + sx c, j0 + sy m) or its transpose when swapped; every product is below 2^29
 *   because nx ny <= NPA_ROUTE_MAX_CELLS.  32-bit integers, no math library.  A segment through a cell corner takes both cells
 *   beside the corner -- the diagonal rule of the fields --, so a straight run of a chain is always visible; the relation is
 *   symmetric in a and b.  Lane l takes columns l, l + 64, ... and loads its two or three cells; one ballot decides.
 * Shortcutting: the candidates are the way-points above in their order -- the cell of every turn of the chain, then the
 *   goal's cell.  The anchor is the start (its cell stands for it in the test).  While the candidate's cell is visible from
 *   the anchor's cell it is remembered as `last`.  At the first candidate that is not visible the segment anchor -> `last` is
 *   emitted, `last` becomes the anchor and the candidate becomes `last` (the chain's next turn after the new anchor: a straight
 *   run, visible).  At the goal: anchor -> `last` if the goal's cell is not visible, then the segment to the goal's own (x, y).
 *   Segment points are the start's (x, y), cell centres and the goal's (x, y); rows, skipped segments, h, "nothing is written
 *   unless the whole path fits", the two passes, no route and no curve are as above.  No list of turns is kept: anchor and
 *   `last` are two cells.
 * Only cell CENTRES are tested: the start and the goal lie up to half a cell off theirs, and a segment clears the inflated
 *   cells, not a swept disc -- the radius the caller inflated the map by must carry both (half a cell's diagonal more). */
int npa_route_curve_batch(int batch, const uint32_t *fields, int n_fields, int nx, int ny, double x0, double y0,
                          double resolution, const int32_t *field_of, const double *start, const double *goal,
                          const double *interval, int capacity, const int32_t *mask, double *rows_out, int32_t *n_rows,
                          void *stream);
int npa_cycle_retask_routed(int batch, int receding, int cycle, const double *state, int32_t *arrived,
                            const int32_t *collided, double *path, const int32_t *curve_off, int32_t *curve_len,
                            const int32_t *robot_first, const int32_t *row_capacity, const double *goals, int g_stride,
                            const int32_t *n_goals, int32_t *goal_index, const double *interval, int32_t *curve_index,
                            int32_t *cur_off, int32_t *cur_len, int32_t *point_index, float *cur_vel,
                            int32_t *retask_status, int32_t *log_goal, const uint32_t *fields, int n_fields, int nx,
                            int ny, double x0, double y0, double resolution, const int32_t *field_of, void *stream);
int npa_route_curve_batch_los(int batch, const uint32_t *fields, int n_fields, int nx, int ny, double x0, double y0,
                              double resolution, const int32_t *field_of, const double *start, const double *goal,
                              const double *interval, int capacity, const int32_t *mask, double *rows_out, int32_t *n_rows,
                              void *stream);
int npa_cycle_retask_routed_los(int batch, int receding, int cycle, const double *state, int32_t *arrived,
                                const int32_t *collided, double *path, const int32_t *curve_off, int32_t *curve_len,
                                const int32_t *robot_first, const int32_t *row_capacity, const double *goals, int g_stride,
                                const int32_t *n_goals, int32_t *goal_index, const double *interval, int32_t *curve_index,
                                int32_t *cur_off, int32_t *cur_len, int32_t *point_index, float *cur_vel,
                                int32_t *retask_status, int32_t *log_goal, const uint32_t *fields, int n_fields, int nx,
                                int ny, double x0, double y0, double resolution, const int32_t *field_of, void *stream);

/* ---- the bookkeeping of a device-resident closed loop (csrc/cycle.hip) -----------------------------------------------
 *
 * What the host does between the kernels of a control cycle, as three calls (and a fourth for fleets whose robots have goal
 * queues): handle-free, stream-ordered, one thread per robot (npa_cycle_retask: one wave), no workspace, no atomics, nothing
 * allocated, no host synchronisation.  The three only select and copy, so a cycle
 *     npa_cycle_progress -> npa_world_scan -> npa_scan_to_points -> npa_nominal_ref_states -> npa_forward_batch
 *     [-> npa_plan_clearance] -> npa_cycle_act -> npa_world_step -> npa_cycle_commit [-> npa_cycle_retask]
 * on one stream over buffers that stay where they are gives the bits of the same cycle paced by the host (the fourth computes a
 * curve: the host-paced cycle takes its rows from npa_curve_batch, the same device function).
 *
 * The curve table holds ALL curves of all robots: path [rows][4] f64 rows (x, y, theta, gear), curve c owns rows
 * curve_off[c] .. curve_off[c] + curve_len[c] - 1, robot b owns the curves robot_first[b] .. robot_first[b + 1] - 1
 * (robot_first [B + 1]; every robot has at least one curve of at least one point).  Per-robot state, device int32 [B]:
 * curve_index (into the robot's curves), cur_off / cur_len (= the table's entry of the current curve: the curve arguments
 * of npa_nominal_ref_states), point_index, arrived (a latch: 0 / 1).  The caller initialises them once: curve_index = 0,
 * cur_off / cur_len = the robot's first curve, point_index = 0, arrived = 0.
 *
 * npa_cycle_progress replaces check_arrive and the curve switching around it (neupan/blocks/initial_path.py:247-315, called
 *   at neupan/neupan.py:113).  Two launches: npa_path_progress's kernel on (cur_off, cur_len, point_index) -- the same
 *   arithmetic, curve_arrived [B] receives its arrival flags --, then for a robot that reports arrival and is not latched:
 *   on its last curve with loop != 0 curve_index = 0 and point_index = 0; on its last curve without loop arrived = 1;
 *   otherwise curve_index += 1 and point_index = 0.  cur_off / cur_len follow curve_index.  state [B][3] f64 is also written
 *   into the `state` field of params_a[b] and params_b[b] (the rows npa_world_scan and npa_scan_to_points read; the two may
 *   be the same block).
 *
 * npa_cycle_act replaces the tail of neupan.forward behind the PAN call (neupan/neupan.py:137 and :150-164) and the driver's
 *   freeze, in this order.  done = arrived[b] != 0.  cur_vel [B][2][T] <- opt_u [B][2][T] unless done (first_cycle != 0: for
 *   every robot -- the reference's cur_vel_array of zeros has just been consumed).  stop = min_distance[b] <
 *   collision_threshold (f32).  The action is opt_u[b][:][0]; kinematics 2 (omni): (v cos phi, v sin phi) in f32.  It is
 *   zeroed where done or stop; then override_row [B][2] f32 (nullable) replaces the entries it holds that are not NaN; then
 *   frozen[b] = arrived[b] | collided[b] and the action is zeroed where frozen.  Outputs: action [B][2] f32 and frozen [B]
 *   int32 (npa_world_step's arguments), stop [B] uint8 = stop and not done, and row `cycle` of the logs (each nullable):
 *   log_actions [cycles][B][2] f32, log_stop [cycles][B] uint8, log_controls [cycles][B][2][T] f32 (opt_u), log_n_points
 *   [cycles][B] int32 (n_points [B], nullable: zeros).  `cycle` travels by value: there is no device-side counter.
 *
 * npa_cycle_commit runs behind npa_world_step: collided[b] |= clearance[b] <= 0 (clearance [B] f64), and the cycle's rows of
 *   the logs (nullable): log_clearance [cycles][B] f64 row `cycle`, log_states [cycles + 1][B][3] f64 row `cycle + 1` (row 0
 *   is the caller's: the initial poses).
 *
 * npa_cycle_retask (optional, one launch, one WAVE per robot) runs behind npa_cycle_commit and gives a robot that has arrived
 *   its next goal -- the reference's reset() followed by update_initial_path_from_goal(state, goal) (neupan/neupan.py:288-294,
 *   :314-318), without the host.  It needs a table in which robot b owns ONE curve (robot_first[b + 1] - robot_first[b] == 1)
 *   whose region, the rows from curve_off[robot_first[b]] on, has room for row_capacity[b] rows ([B] int32; the regions must
 *   not overlap: they are not checked).  goals [B][g_stride][3] f64 (x, y, theta), n_goals [B] int32 (<= g_stride), goal_index
 *   [B] int32 (in / out; the caller zeroes it), interval [B] f64 (the spacing of the new curve: npa_nominal_ref_states'
 *   argument), style and min_radius as for npa_curve_batch.
 *   Robot b re-tasks when arrived[b] != 0, collided[b] == 0 and 0 <= goal_index[b] < n_goals[b].  Then the curve from state[b]
 *   (the pose after the step) to goals[b][goal_index[b]] is generated by npa_curve_batch's device function (the same bits).  It
 *   fits (1 <= rows <= row_capacity[b]): the rows are written into the region; curve_len of that curve = rows; cur_off[b] =
 *   the region's start, cur_len[b] = rows; curve_index[b] = 0; point_index[b] = 0; arrived[b] = 0; cur_vel [B][2][receding]
 *   f32: the robot's row <- 0 (reset()); goal_index[b] += 1; retask_status[b] = 1.  It does not fit, or its inputs are outside
 *   the curve specification: retask_status[b] = 2 and nothing else of the robot is written -- it stays arrived and the goal
 *   is not consumed.  A robot that does not re-task: retask_status[b] = 0, nothing else.  log_goal [cycles][B] int32
 *   (nullable): row `cycle` receives goal_index after the call.  The planner's own state record (the stop criterion's state,
 *   min_distance, the QP warm start) is not touched, as the reference does not touch it.
 *
 * NPA_E_ARG (before anything touches a device): a null required pointer, batch < 1, cycle < 0, ind_range < 1, receding
 *   outside [1, NPA_MAX_T], kinematics outside 0..2; npa_cycle_retask also: style outside 0..1, Dubins with min_radius <= 0,
 *   g_stride < 1. */
int npa_cycle_progress(int batch, const double *state, const double *path, const int32_t *curve_off,
                       const int32_t *curve_len, const int32_t *robot_first, int loop, double close_threshold,
                       int ind_range, double arrive_threshold, int arrive_index_threshold, int32_t *curve_index,
                       int32_t *cur_off, int32_t *cur_len, int32_t *point_index, int32_t *curve_arrived,
                       int32_t *arrived, npa_scan_params *params_a, npa_scan_params *params_b, void *stream);
int npa_cycle_act(int batch, int receding, int kinematics, int first_cycle, int cycle, const float *opt_u,
                  const float *min_distance, float collision_threshold, const int32_t *arrived,
                  const int32_t *collided, const float *override_row, const int32_t *n_points, float *cur_vel,
                  float *action, uint8_t *stop, int32_t *frozen, float *log_actions, uint8_t *log_stop,
                  float *log_controls, int32_t *log_n_points, void *stream);
int npa_cycle_commit(int batch, int cycle, const double *state, const double *clearance, int32_t *collided,
                     double *log_states, double *log_clearance, void *stream);
int npa_cycle_retask(int batch, int receding, int cycle, int style, double min_radius, const double *state,
                     int32_t *arrived, const int32_t *collided, double *path, const int32_t *curve_off,
                     int32_t *curve_len, const int32_t *robot_first, const int32_t *row_capacity, const double *goals,
                     int g_stride, const int32_t *n_goals, int32_t *goal_index, const double *interval,
                     int32_t *curve_index, int32_t *cur_off, int32_t *cur_len, int32_t *point_index, float *cur_vel,
                     int32_t *retask_status, int32_t *log_goal, void *stream);

/* ---- training the adjust parameters inside the resident loop (csrc/lon.hip) ------------------------------------------
 *
 * The reference's LON examples (example/LON/LON_corridor.py) tune p_u, eta, d_max by driving a robot through a world: per
 * cycle a loss on info["distance_tensor"], its gradient through the QP, an Adam step; the episode ends on arrive, stop or
 * stuck.  These three calls are the host's part of that loop for B robots with one parameter row each, handle-free and
 * stream-ordered like the cycle calls: one thread per robot, no workspace, no atomics, no device-side counter, nothing
 * allocated, no host synchronisation.  Every arithmetic statement is one IEEE operation in the order given here (no
 * contraction), so numpy restates them bit for bit.  One training cycle on one stream:
 *     npa_cycle_progress -> npa_world_scan -> npa_scan_to_points -> npa_nominal_ref_states
 *     -> npa_forward_begin, K x { copy cur_s, cur_u; npa_forward_iter(k); copy the mu / lam / pts / count rows }, npa_forward_end
 *     -> npa_cycle_act (override_row = the override buffer below) -> npa_world_step -> npa_cycle_commit
 *     -> npa_lon_loss -> for k = K-1 .. first: npa_nrmp_backward(the copies of k, grad_s, grad_u, grad_d) -> npa_lon_chain(k)
 *     -> npa_lon_adam
 * Parameter-shaped arrays are rows of 8 like npa_set_adjust_batch's theta: q_s[0..2], p_u, eta, d_max, d_min, reserved;
 * column 7 is never read or written here (npa_lon_chain reads the status that npa_nrmp_backward puts there).
 *
 * npa_lon_loss replaces LON_corridor.py:10-19 (cal_distance_loss), :62-82 (the stuck test, loss = 10 * distance_loss) and
 *   :102 (the end of the episode); it runs behind npa_cycle_commit.  Inputs per robot: state [B][3] f64 (after the step),
 *   last_xy [B][2] f64 (in / out: the position at the previous call; the caller initialises it to the start), opt_d [B][T],
 *   min_distance [B] f32, stop [B] uint8 (npa_cycle_act's), arrived / collided [B] int32 (the latches), stuck_count and
 *   ended [B] int32 (in / out, the caller zeroes them when an episode starts).
 *   A robot with ended[b] != 0 at the call: active[b] = 0, loss 0, grad_d 0, stuck_count and ended unchanged.
 *   Otherwise active[b] = 1 and: disp = sqrt(dx*dx + dy*dy) in f64; stuck_count += disp < stuck_threshold (cumulative over
 *   the episode, as in the example); stuck = stuck_count > stuck_patience; S = ((0 + opt_d[b][0]) + opt_d[b][1]) + ... in f32;
 *   min_distance[b] <= collision_threshold (f32): loss = loss_weight * (loss_offset - S), grad_d[b][t] = -loss_weight; else
 *   stuck: loss = loss_weight * (loss_offset + S), grad_d[b][t] = +loss_weight; else loss 0, grad_d 0.  Then
 *   ended[b] |= arrived | collided | stop | stuck.
 *   For every robot: loss [B] f32; grad_s [B][3][T+1] and grad_u [B][2][T] are written as zeros (with grad_d [B][T] the
 *   upstream gradients of the first npa_nrmp_backward); a robot whose ended flag is set after the call gets (0, 0) in its row
 *   of override_row [B][2] f32 -- the buffer the NEXT npa_cycle_act takes as its override_row; the other rows keep what the
 *   caller put there (NaN: the planner's action) --; last_xy = state[0:2]; row `cycle` of the logs (each nullable): log_loss
 *   [cycles][B] f32, log_stuck [cycles][B] uint8 (the stuck test; for an ended robot, of its unchanged count), log_ended
 *   [cycles][B] uint8 (ended after the call).
 *
 * npa_lon_chain is the step between two npa_nrmp_backward calls, run after the one that re-solved PAN iteration k.  For a robot
 *   with iters[b] > k (it executed iteration k): tot[b][c] += (double) grad_theta[b][c], c = 0 .. 6 (tot [B][8] f64);
 *   grad_s[b] <- grad_nom_s[b]; grad_u[b] <- 0; grad_d[b] <- 0; bad[b] += grad_theta[b][7] != 0 (the solver status).  Other
 *   robots are untouched: their upstream gradients wait for an earlier iteration.
 *
 * npa_lon_adam replaces torch.optim.Adam.step and opt.zero_grad (LON_corridor.py:41, :94-95, :127), one thread per row.
 *   For c = 0 .. 6: g32 = (float) tot[b][c]; gacc[b][c] = accumulate ? gacc[b][c] + g32 : g32 (the reference clears the
 *   gradients once per episode, so a caller that follows it accumulates and zeroes gacc between episodes); tot[b][c] = 0.
 *   Then, when active[b] != 0 and gacc[b][c] is finite for every c in column_mask (bit c = column c), for every c in the mask,
 *   each line one rounded f32 operation per operator, left to right:
 *       m = beta1 * m + one_minus_beta1 * g            v = beta2 * v + (one_minus_beta2 * g) * g
 *       denom = sqrtf(v) / bc2_sqrt + eps               theta = theta - step_size * (m / denom)
 *       theta = fminf(fmaxf(theta, lo[c]), hi[c])                 (sqrtf and / correctly rounded, as numpy's are)
 *   with g = gacc[b][c]; m, v, theta [B][8] f32 (theta: the block npa_set_adjust_batch registered, rewritten in place).  An
 *   active row with a non-finite masked entry is not stepped and skipped[b] += 1; a row that is not active is not stepped.
 *   The scalars travel by value, computed by the host in double as torch computes them: one_minus_beta = 1 - beta,
 *   step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t), t = 1, 2, ... the step count; lo / hi: HOST arrays of 8 f32
 *   (null: -inf / +inf), copied into the launch.
 *
 * Rows shared by groups of robots.  The reference tunes ONE parameter set by driving; with npa_lon_reduce and npa_lon_scatter a
 *   row is trained from the rollouts of every robot that shares it (different corridors, obstacles, start poses, agents):
 *       ... npa_lon_chain(first) -> npa_lon_reduce -> npa_lon_adam on the G group rows -> npa_lon_scatter
 *   npa_lon_adam is unchanged: batch = G, tot = gtot, active = gactive, and the group's own gacc, m, v, theta, skipped.
 *
 * npa_lon_reduce sums the gradient rows of the robots of a group, one wave (a 64-thread workgroup) per group, in a fixed order.
 *   The groups are a CSR table: group_first [groups + 1] int32 (group_first[0] = 0), group_members [group_first[groups]] int32,
 *   robot indices, ascending inside a group.  CONTRACT: every index lies in [0, batch) and a robot appears in at most one
 *   group (no two waves write one word; the indices are not checked).  Lane l holds column c = l & 7 of slot s = l >> 3.
 *   For group g let n = group_first[g+1] - group_first[g] and b_j = group_members[group_first[g] + j], j = 0 .. n-1:
 *     use_j   = active[b_j] != 0 and, for every c in column_mask, (float) tot[b_j][c] is finite (what npa_lon_adam would see);
 *     x_j[c]  = use_j ? tot[b_j][c] : +0.0                                              for c = 0 .. 6,
 *     x_j[7]  = (loss != NULL and active[b_j] != 0) ? (double) loss[b_j] : +0.0;
 *     slot sums: a_s[c] = +0.0, then for j = s, s + 8, s + 16, ... < n in that order a_s[c] = a_s[c] + x_j[c] -- ceil(n / 8)
 *             trips for the whole wave; a slot whose j is past the end reads the last member again and adds +0.0;
 *     combine: a_s = a_s + a_{s+4} for s < 4, then a_s = a_s + a_{s+2} for s < 2, then a_0 = a_0 + a_1 (the lower slot is the
 *             left operand), every addition one rounded f64 operation;
 *     n_used[g] = #{j: use_j};  dropped[g] += #{j: active[b_j] != 0 and not use_j} (cumulative);  gactive[g] = n_used[g] > 0;
 *     gtot[g][c] = (mean != 0 and n_used[g] > 0) ? a_0[c] / (double) n_used[g] : a_0[c] for c = 0 .. 6 (gtot [G][8] f64;
 *             gtot[g][7] is not written);  gloss[g] = a_0[7] (f64, nullable; a sum, never divided);
 *     tot[b_j][c] = 0 for c = 0 .. 6 of every member, used or not, as npa_lon_adam clears behind its read.
 *   Column 7 of tot keeps its bits; rows of robots in no group are untouched.  An empty group: gactive 0, n_used 0, the sums
 *   +0.0, dropped unchanged.
 *
 * npa_lon_scatter is the way back, one thread per robot: with g = group_of[b] (group_of [B] int32), when 0 <= g < groups
 *   theta[b][c] = group_theta[g][c] for c = 0 .. 6 (group_theta [G][8], theta [B][8] f32); any other g (-1: a robot that keeps
 *   a fixed row of its own) leaves the row as it is.  Column 7 is never written.
 *
 * NPA_E_ARG (before anything touches a device): a null required pointer, batch < 1, groups < 1, cycle < 0, k < 0, receding
 *   outside [1, NPA_MAX_T], a column_mask with bits above 6. */
int npa_lon_loss(int batch, int receding, int cycle, const double *state, double *last_xy, const float *opt_d,
                 const float *min_distance, const uint8_t *stop, const int32_t *arrived, const int32_t *collided,
                 float collision_threshold, double stuck_threshold, int stuck_patience, float loss_weight,
                 float loss_offset, int32_t *stuck_count, int32_t *ended, int32_t *active, float *loss,
                 float *grad_s, float *grad_u, float *grad_d, float *override_row, float *log_loss,
                 uint8_t *log_stuck, uint8_t *log_ended, void *stream);
int npa_lon_chain(int batch, int receding, int k, const int32_t *iters, const float *grad_theta,
                  const float *grad_nom_s, double *tot, float *grad_s, float *grad_u, float *grad_d, int32_t *bad,
                  void *stream);
int npa_lon_adam(int batch, int column_mask, int accumulate, double *tot, float *gacc, float *m, float *v,
                 float *theta, const int32_t *active, float beta1, float one_minus_beta1, float beta2,
                 float one_minus_beta2, float step_size, float bc2_sqrt, float eps, const float *lo, const float *hi,
                 int32_t *skipped, void *stream);
int npa_lon_reduce(int batch, int groups, int column_mask, int mean, const int32_t *group_first,
                   const int32_t *group_members, double *tot, const int32_t *active, const float *loss, double *gtot,
                   int32_t *gactive, int32_t *n_used, int32_t *dropped, double *gloss, void *stream);
int npa_lon_scatter(int batch, int groups, const int32_t *group_of, const float *group_theta, float *theta, void *stream);

/* ---- DUNE training labels (offline) ---------------------------------------------------------------
 * npa_dune_labels replaces DUNETrain.prob_solve / generate_data_set
 *   (neupan/blocks/dune_train.py:82-99, :109-140): for every point p the maximiser mu of
 *   mu^T (G p - h) s.t. ||G^T mu|| <= 1, mu >= 0 and the optimal value (the distance of p to the
 *   robot polygon), by closed form instead of one ECOS call per point.
 *   G [E][2], h [E]: HOST arrays (float64), consecutive counter-clockwise edges as
 *   gen_inequal_from_vertex produces them (util/__init__.py:161-206);
 *   points [n][2] f64 (device); mu [n][E] f32, dist [n] f32 (device; the reference stores float32
 *   tensors, dune_train.py:101-107).
 *   A point with max_e (G_e p - h_e) <= 0 (inside or on the polygon) gets zeros.  Outside, mu has one
 *   entry (1/|G_e|, the nearest point inside edge e) or the two of the edges at the nearest vertex; where
 *   the vertex solve does not give two positive entries (the point on the boundary of the vertex's normal
 *   cone, or within rounding of the vertex) it is the one entry of the edge the direction leans to, so
 *   |G^T mu| = 1 always.  NPA_E_ARG: G, h NULL, n < 0, a NULL array with n > 0; NPA_E_UNSUPPORTED:
 *   edge_num outside [3, NPA_MAX_E]; NPA_E_HIP ("invalid argument", before any launch): parallel
 *   consecutive rows or a zero row in G.  n == 0 returns NPA_OK without a launch. */
int npa_dune_labels(int edge_num, const double *G, const double *h, int64_t n, const double *points,
                    float *mu, float *dist, void *stream);

const char *npa_last_error(void);
const char *npa_version(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* NEUPAN_AMD_H */
