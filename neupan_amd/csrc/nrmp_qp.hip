// nrmp_qp.hip -- NRMP step of the PAN loop: parameter build + convex QP solve + stop test,
// one wavefront per scene, fp64.  gfx950 (MI355X) only.
//
// Replaces (reference file:line)
//   robot.generate_state_parameter_value / linear_*_model   neupan/robot/robot.py:239-316
//   NRMP.generate_coefficient_parameter_value               neupan/blocks/nrmp.py:220-261
//   NRMP.forward -> CvxpyLayer (cvxpylayers/diffcp/ECOS)     neupan/blocks/nrmp.py:114-150
//        the problem itself: nrmp.py:263-383, robot.py:142-236
//   PAN.stop_criteria                                        neupan/blocks/pan.py:215-243
//
// The problem (variables s(3,T+1), u(2,T), d(T)):
//   min  sum (q_s s - q_s ref)^2 + sum (p_u u0 - p_u ref_us)^2 + bk/2 |s - nom_s|^2
//        - eta sum d + ro/2 sum_{t,j} max(0, -(fa_tj . s_xy(t+1) - fb_tj - d_t))^2
//   s.t. s(t+1) = A_t s(t) + B_t u(t) + C_t, s(0) = nom_s(0), |u| <= speed, |du| <= acce,
//        max(d_min,0) <= d <= d_max.
//
// Algorithm (transliterated in oracle/condensed_ipm.py, which the tests check against the
// uncondensed fp64 oracle and HiGHS): states eliminated through the linearised dynamics
// (s(t+1) = Phi_t u + c_t), hinge rows carried through their own stationarity condition
// e = lam_f/ro (no epigraph variables), Mehrotra predictor-corrector on x = (u, d).  Each
// Newton system is reduced once more by eliminating d (its block of the KKT matrix is
// diagonal), which leaves a dense SPD 2T x 2T system in u:
//      K' = H + C_u' D C_u + sum_t Phi_xy(t)' S'_t Phi_xy(t),   S'_t = S_t - v_t v_t'/kappa_t
// factored by a Cholesky with one matrix row per lane (right-looking in the register-resident instantiations, pivot
// chain on v_readlane; left-looking over the LDS matrix in the generic one).
//
// Why one wave per scene: the solve is a serial chain of small dense steps (latency bound);
// scenes are independent, so throughput comes from the batch.  Matrices live in LDS with odd
// leading dimensions (conflict-free row-per-lane access), cross-lane broadcast is v_readlane,
// wave reductions are DPP (quad_perm / row_mirror) + 4 readlanes, and every division in a
// serial loop is replaced by a reciprocal computed once per iteration.
#include "launch.h"
#include <hip/hip_ext.h>
#include <cstdlib>
#include <type_traits>

#include "nrmp_qp_device.h"

static bool qp_fast_path(int T, int M) { return (T == 10 || T == 20) && M == 10; }

// LDS bytes of one scene; `fast` = the register-resident instantiation (packed H, L and P staging, the scan forms in place
// of a stored Phi)
extern "C" size_t npa_qp_shmem_bytes_path(int T, int M, int fast) {
  const bool obs = M > 0;
  size_t nu = 2 * T, ldp = nu + 1, mcd = 8 * T - 4 + 2 * T, mf = obs ? (size_t)T * M : 0, npair = nu * (nu + 1) / 2;
  const size_t mfe = (mf + 1) & ~(size_t)1;
  // (mirrors the kernel's carve: REGROWS keeps 3 of the 6 u / d row arrays and 5 of the 9 hinge row arrays in LDS)
  const bool regrows = fast && M > 0 && M % 2 == 0 && T * M / 2 <= QP_THREADS && 5 * T - 2 <= QP_THREADS;
  const size_t rows = (regrows ? 3 : 6) * mcd + (regrows ? 5 : 9) * mfe;
  // (SLIM, nrmp_qp_body.inc: the wide-scan instantiation folds the packed H and the packed factor L into one block)
  const bool slim = fast && T > 16;
  const size_t mats = slim ? nu * (nu + 1) / 2 : (fast ? nu * (nu + 1) / 2 + nu * ldp : (size_t)T * 2 * ldp + 2 * nu * ldp);
  const size_t phi = fast ? 0 : (size_t)T * 3 * ldp;
  size_t d = rows + phi + mats + 4 * (T * 3) + T * QP_ABC_LD + (((size_t)T * QP_ST_LD + 1) & ~(size_t)1) + nu + T + (nu + T) + nu + T + nu +
             (fast ? 2 * (size_t)T : 0);
  size_t bytes = d * sizeof(double) + (fast ? 0 : 2 * ((npair + 7) & ~(size_t)7));
  return (bytes + 15) & ~(size_t)15;
}

size_t npa_qp_shmem_bytes(int T, int M) { return npa_qp_shmem_bytes_path(T, M, 0); }

// the kernel's argument list from a launcher's (c, batch, extra); every launch covers the scenes 0 .. batch - 1 of its call
#define QP_KERNEL_ARGS                                                                                                          \
  P, c.cur_s_in, c.cur_u_in, c.ref_s, c.ref_us, c.mu_sorted, c.lam_sorted, c.pts_sorted, c.dist_sorted, c.count, c.cur_s_out,   \
      c.cur_u_out, c.cur_d_out, c.out_s, c.out_u, c.out_d, c.out_min_distance, c.out_iters, c.out_nrmp_points, c.flags, c.state, \
      c.qp_info, c.warm, 0, batch, extra, c.trig_out, c.theta, c.sched

hipError_t npa_launch_qp(const DevParams& P, const QpCall& c, int batch, const QpBackward& extra, hipStream_t stream,
                         hipEvent_t ev_start, hipEvent_t ev_stop) {
  static const bool force_generic = getenv("NPA_QP_GENERIC") != nullptr;     // tests: the generic (LDS) instantiation for every (T, M)
  const bool fast = qp_fast_path(P.T, P.M) && !force_generic;
  const size_t shmem = npa_qp_shmem_bytes_path(P.T, P.M, fast ? 1 : 0);      // one scene (wave) per workgroup, see the kernel
  const int nblocks = batch;
  static NpaDeviceOnce attr_set;       // (per device: the attribute is, and a process may hold handles on several GPUs)
  int dev_ = 0;
  if (attr_set.need(&dev_)) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(nrmp_qp_kernel<0, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute(reinterpret_cast<const void*>(nrmp_qp_kernel<10, 10>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute(reinterpret_cast<const void*>(nrmp_qp_kernel<20, 10, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set.done(dev_);
  }
#define QP_LAUNCH(...)                                                                                           \
  hipExtLaunchKernelGGL((nrmp_qp_kernel<__VA_ARGS__>), dim3(nblocks), dim3(QP_THREADS), shmem, stream, ev_start, ev_stop, 0, \
                        QP_KERNEL_ARGS)
  if (fast && P.T == 10) QP_LAUNCH(10, 10);
  else if (fast && P.T == 20) QP_LAUNCH(20, 10, false, true);
  else QP_LAUNCH(0, 0);
#undef QP_LAUNCH
  return hipGetLastError();
}

// nrmp_qp_kernel for a group of n forward calls that share the configuration, the batch size and the stream: ONE launch,
// grid (batch, n).  The register-resident instantiations only (c_api.hip keeps everything else call by call).
int npa_qp_group_supported(int T, int M) {
  static const bool force_generic = getenv("NPA_QP_GENERIC") != nullptr;
  return !force_generic && M == 10 && (T == 10 || T == 20) ? 1 : 0;
}
hipError_t npa_launch_qp_group(const DevParams& P, const QpGroup& G, int n, int batch, hipStream_t stream,
                                          hipEvent_t ev_start, hipEvent_t ev_stop) {
  if (n < 1 || n > NPA_GROUP_MAX || !npa_qp_group_supported(P.T, P.M)) return hipErrorInvalidValue;
  const size_t shmem = npa_qp_shmem_bytes_path(P.T, P.M, 1);
  static NpaDeviceOnce attr_set;
  int dev_ = 0;
  if (attr_set.need(&dev_)) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(nrmp_qp_group_kernel<10, 10>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute(reinterpret_cast<const void*>(nrmp_qp_group_kernel<20, 10, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set.done(dev_);
  }
  if (P.T == 10)
    hipExtLaunchKernelGGL((nrmp_qp_group_kernel<10, 10>), dim3(batch, n), dim3(QP_THREADS), shmem, stream, ev_start, ev_stop, 0, P, G, batch, n);
  else
    hipExtLaunchKernelGGL((nrmp_qp_group_kernel<20, 10, true>), dim3(batch, n), dim3(QP_THREADS), shmem, stream, ev_start, ev_stop, 0, P, G, batch, n);
  return hipGetLastError();
}

// forward solve + gradient w.r.t. the adjust parameters (generic kernel, one scene per workgroup)
hipError_t npa_launch_qp_backward(const DevParams& P, const QpCall& c, int batch, const QpBackward& extra, hipStream_t stream) {
  static const bool force_generic = getenv("NPA_QP_GENERIC") != nullptr;
  const bool fast = qp_fast_path(P.T, P.M) && !force_generic;
  const size_t wave_bytes = npa_qp_shmem_bytes_path(P.T, P.M, fast ? 1 : 0);
  static NpaDeviceOnce attr_set;
  int dev_ = 0;
  if (attr_set.need(&dev_)) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(nrmp_qp_kernel<0, 0, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute(reinterpret_cast<const void*>(nrmp_qp_kernel<10, 10, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute(reinterpret_cast<const void*>(nrmp_qp_kernel<20, 10, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr_set.done(dev_);
  }
  // (the register-resident instantiations since round 3: the gradient pass reads the multiplier directions of the d rows
  // from their owner lanes; NPA_QP_GENERIC=1 keeps the LDS kernel)
#define QPB_LAUNCH(...) \
  hipLaunchKernelGGL((nrmp_qp_kernel<__VA_ARGS__>), dim3(batch), dim3(QP_THREADS), wave_bytes, stream, QP_KERNEL_ARGS)
  if (fast && P.T == 10) QPB_LAUNCH(10, 10, true);
  else if (fast && P.T == 20) QPB_LAUNCH(20, 10, true, true);
  else QPB_LAUNCH(0, 0, true);
#undef QPB_LAUNCH
#undef QP_KERNEL_ARGS
  return hipGetLastError();
}
