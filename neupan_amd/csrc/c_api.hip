// c_api.hip -- the forward path behind the extern "C" boundary of libneupan_amd.so (see include/neupan_amd.h): workspace
// carving, launch sequencing, the stage entry points, the front-end / ingest / label wrappers.  Creation, calibration and the
// self-test are create.hip; the two share the handle (handle.h) and nothing else.  Host-side only, no torch types.
#include "handle.h"
#include "launch.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

// The one experiment on record that is still compiled (measured slower than the default path) is the
// first form of the geometric selection, select_kernel<E, true> behind NPA_SELECT_V1, and only with -DNPA_EXPERIMENTS
// (NPA_EXPERIMENTS=1 python -m neupan_amd.build).  The default build has neither its kernel nor its environment knob.
// (Retired from the tree, their measurements kept in DESIGN.md sections 3.3 and 7: round 6's two one-launch experiments -- the
// forward call as one launch, the selection with one wave per scene: a wave that walks the ten slices of its scene one after
// the other cannot win where launches are cheap and the chip is empty, and lost 2 x where it is full -- then the active-set
// launch in front of the interior-point launch and the T = 20 QP instantiation with a stored Phi.)
#ifdef NPA_EXPERIMENTS
#define NPA_VERSION_SUFFIX " +experiments"
#else
#define NPA_VERSION_SUFFIX ""
#endif

extern "C" const char* npa_last_error(void) { return g_err.c_str(); }
extern "C" const char* npa_version(void) { return "neupan_amd 0.5.2 (gfx950, hipcc " NPA_HIPCC_VERSION ")" NPA_VERSION_SUFFIX; }
// per-slice stride of the key buffer inside the workspace: none with geometric keys (select_kernel keeps them in LDS)
static int kstride(const npa_handle* h) { return h->key_terms == 4 ? 0 : h->P.key_stride; }
// the selection launchers' rows_bf16: 1 = the reduced-precision tier of the rows, 2 = the bf16 tier of the keys, 0 = exact
static int rows_tier(const npa_handle* h) { return h->rows_bf16 ? 1 : (h->cal.keys_bf16 ? 2 : 0); }
// the workspace of a forward call of `batch` scenes on this handle
static ScratchLayout layout_of(const npa_handle* h, int batch) {
  return npa_scratch_layout(batch, h->P.T, mdim(h->P), h->P.E, kstride(h), h->P.K);
}

// a solve of `batch` scenes on a handle whose block was registered for another number of rows would read past it (or leave
// rows unread): refused
static int check_theta_batch(const npa_handle* h, int batch, const char* who) {
  if (h->theta && batch != h->theta_batch)
    return fail(NPA_E_ARG, std::string(who) + ": batch " + std::to_string(batch) + " differs from the " + std::to_string(h->theta_batch) +
                               " rows registered with npa_set_adjust_batch");
  return NPA_OK;
}

extern "C" size_t npa_workspace_bytes(const npa_handle* h, int batch) {
  if (!h || batch < 1) return 0;
  return layout_of(h, batch).total * sizeof(float);
}
extern "C" size_t npa_workspace_qp_info_offset(const npa_handle* h, int batch) {
  if (!h || batch < 1) return 0;
  return layout_of(h, batch).qp_info * sizeof(float);
}
extern "C" int npa_workspace_layout(const npa_handle* h, int batch, size_t* out, int n) {
  if (!h || batch < 1 || !out || n < 1) return fail(NPA_E_ARG, "npa_workspace_layout: bad argument");
  const ScratchLayout L = layout_of(h, batch);
  // ([8]: the dispatch-order block of the QP launches -- cnt [K][32], list [2][32][batch], ticket [batch], ints; pan_common.h)
  const size_t v[9] = {L.cur_s * 4, L.cur_u * 4, L.cur_d * 4, L.mu * 4, L.lam * 4, L.pts * 4, L.dist * 4, L.count * 4, L.sched * 4};
  for (int i = 0; i < n && i < 9; ++i) out[i] = v[i];
  return NPA_OK;
}
extern "C" size_t npa_state_bytes(const npa_handle* h, int batch) {
  if (!h || batch < 1) return 0;
  return (size_t)batch * npa_state_floats(h->P.T, mdim(h->P), h->P.E) * sizeof(float);
}

static EventPair* next_event(npa_handle* h, std::vector<EventPair>& pool, size_t& used) {
  if (!h->prof) return nullptr;
  if (used == pool.size()) {
    if (pool.size() >= 8192) return nullptr;
    EventPair p;
    if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) return nullptr;
    pool.push_back(p);
  }
  return &pool[used++];
}

extern "C" int npa_profile_enable(npa_handle* h, int enable) {
  if (!h) return fail(NPA_E_ARG, "null handle");
  h->prof = enable != 0;
  h->n_dune = h->n_sel = h->n_qp = 0;
  return NPA_OK;
}

extern "C" int npa_profile_read(npa_handle* h, double* dune_ms_avg, double* select_ms_avg, double* nrmp_ms_avg,
                                int64_t* launches) {
  if (!h) return fail(NPA_E_ARG, "null handle");
  auto avg = [](std::vector<EventPair>& pool, size_t used, double* out) -> hipError_t {
    double tot = 0;
    for (size_t i = 0; i < used; ++i) {
      hipError_t e = hipEventSynchronize(pool[i].b);
      if (e != hipSuccess) return e;
      float ms = 0;
      e = hipEventElapsedTime(&ms, pool[i].a, pool[i].b);
      if (e != hipSuccess) return e;
      tot += ms;
    }
    if (out) *out = used ? tot / used : 0.0;
    return hipSuccess;
  };
  HIP_TRY(avg(h->ev_dune, h->n_dune, dune_ms_avg));
  HIP_TRY(avg(h->ev_sel, h->n_sel, select_ms_avg));
  HIP_TRY(avg(h->ev_qp, h->n_qp, nrmp_ms_avg));
  if (launches) *launches = (int64_t)h->n_qp;
  h->n_dune = h->n_sel = h->n_qp = 0;
  return NPA_OK;
}

extern "C" int npa_dune_stage(npa_handle* h, int batch, int n_stride, const float* nom_s, const float* points,
                              const float* velocities, const int32_t* n_points, float* mu_sorted, float* lam_sorted,
                              float* pts_sorted, float* dist_sorted, int32_t* count, void* stream) {
  if (!h || batch < 1 || n_stride < 1 || !nom_s || !points || !mu_sorted || !lam_sorted || !pts_sorted ||
      !dist_sorted || !count)
    return fail(NPA_E_ARG, "npa_dune_stage: bad argument");
  if (h->P.M <= 0) return fail(NPA_E_ARG, "npa_dune_stage: planner has no obstacle stage (nrmp_max_num or dune_max_num is 0)");
  {
    int nmax = n_stride < h->P.dune_max_num ? n_stride : h->P.dune_max_num;
    if (nmax > h->P.key_stride) return fail(NPA_E_UNSUPPORTED, "more than 32768 points per scene after decimation");
  }
  // key scratch owned by the handle (the stage entry point is a test / profiling hook, the production path carves
  // it from the caller's workspace); none with geometric keys
  const bool geo = h->key_terms == 4;
  const size_t key_bytes = geo ? 0 : (size_t)batch * (h->P.T + 1) * h->P.key_stride * sizeof(unsigned);
  const size_t trig_bytes = ((size_t)batch * (h->P.T + 1) * 2 * sizeof(float) + 63) / 64 * 64;
  const size_t need = key_bytes + trig_bytes + 64;
  if (need > h->stage_cand_bytes) {
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (h->stage_cand) HIP_TRY(hipFree(h->stage_cand));
    h->stage_cand = nullptr; h->stage_cand_bytes = 0;
    HIP_TRY(hipMalloc(&h->stage_cand, need));
    h->stage_cand_bytes = need;
  }
  float* trig = reinterpret_cast<float*>(reinterpret_cast<char*>(h->stage_cand) + key_bytes);
  HIP_TRY(npa_launch_trig(nom_s, batch, h->P.T, trig, (hipStream_t)stream));
  SelGeoCall c{};                        // (flags stay null: no scene of a stage call is done)
  c.wpack = h->wpack; c.cur_s = nom_s; c.points = points; c.vel = velocities; c.n_points = n_points; c.n_stride = n_stride;
  c.mu_sorted = mu_sorted; c.lam_sorted = lam_sorted; c.pts_sorted = pts_sorted; c.dist_sorted = dist_sorted; c.count = count;
  c.stats = h->sel_stats_dev; c.trig = trig; c.audit = h->rows_bf16 ? nullptr : h->audit_dev;
  if (!geo)
    HIP_TRY(npa_launch_encode(h->P, c, batch, 0, (unsigned*)h->stage_cand, h->n_cu, 5, h->key_terms, (hipStream_t)stream, nullptr,
                              nullptr));
  if (geo && !h->select_v1) {
    c.audit_seed = h->launch_seq++;
    HIP_TRY(npa_launch_select_geo(h->P, c, batch, 0, h->sel_debug, h->audit_thresh, h->margin_scale, rows_tier(h),
                                  (hipStream_t)stream, nullptr, nullptr));
  } else {
    HIP_TRY(npa_launch_select(h->P, c, batch, 0, (const unsigned*)h->stage_cand, h->key_terms, h->key_e0, h->sel_debug,
                              (hipStream_t)stream, nullptr, nullptr));
  }
  return NPA_OK;
}

extern "C" int npa_nrmp_stage(npa_handle* h, int batch, const float* nom_s, const float* nom_u, const float* ref_s,
                              const float* ref_us, const float* mu_sorted, const float* lam_sorted,
                              const float* pts_sorted, const int32_t* count, float* out_s, float* out_u,
                              float* out_d, double* qp_info, double* x64, void* stream) {
  if (!h || batch < 1 || !nom_s || !nom_u || !ref_s || !ref_us || !out_s || !out_u)
    return fail(NPA_E_ARG, "npa_nrmp_stage: bad argument");
  if (h->P.M > 0 && (!mu_sorted || !lam_sorted || !pts_sorted || !count || !out_d))
    return fail(NPA_E_ARG, "npa_nrmp_stage: obstacle arrays required when nrmp_max_num > 0");
  if (int rc = check_theta_batch(h, batch, "npa_nrmp_stage")) return rc;
  // (one solve from the nominal: the iterate's slots receive the solution, the forward path's outputs and its state stay null)
  QpCall c{};
  c.cur_s_in = nom_s; c.cur_u_in = nom_u; c.ref_s = ref_s; c.ref_us = ref_us; c.mu_sorted = mu_sorted; c.lam_sorted = lam_sorted;
  c.pts_sorted = pts_sorted; c.count = count;
  c.cur_s_out = out_s; c.cur_u_out = out_u; c.cur_d_out = out_d; c.qp_info = qp_info; c.theta = h->theta;
  QpBackward extra{};
  extra.dbg_x = x64;
  HIP_TRY(npa_launch_qp(h->P, c, batch, extra, (hipStream_t)stream, nullptr, nullptr));
  return NPA_OK;
}

extern "C" int npa_nrmp_params(npa_handle* h, int batch, const float* nom_s, const float* nom_u, const float* mu_sorted,
                               const float* lam_sorted, const float* pts_sorted, const int32_t* count, float* out_abc,
                               float* out_f, void* stream) {
  if (!h || batch < 1 || !nom_s || !nom_u || !out_abc) return fail(NPA_E_ARG, "npa_nrmp_params: bad argument");
  if (h->P.M > 0 && (!mu_sorted || !lam_sorted || !pts_sorted || !count || !out_f))
    return fail(NPA_E_ARG, "npa_nrmp_params: obstacle arrays required when nrmp_max_num > 0");
  // (no theta: the linearisation and the hinge rows do not depend on the adjust parameters; the reference trajectory only enters
  // the cost: the nominal arrays stand in for it, the kernel returns before the solve)
  QpCall c{};
  c.cur_s_in = nom_s; c.cur_u_in = nom_u; c.ref_s = nom_s; c.ref_us = nom_u; c.mu_sorted = mu_sorted; c.lam_sorted = lam_sorted;
  c.pts_sorted = pts_sorted; c.count = count;
  QpBackward extra{};
  extra.dbg_abc = out_abc; extra.dbg_f = h->P.M > 0 ? out_f : nullptr;
  HIP_TRY(npa_launch_qp(h->P, c, batch, extra, (hipStream_t)stream, nullptr, nullptr));
  return NPA_OK;
}

extern "C" int npa_nrmp_backward(npa_handle* h, int batch, const float* nom_s, const float* nom_u, const float* ref_s,
                                 const float* ref_us, const float* mu_sorted, const float* lam_sorted,
                                 const float* pts_sorted, const int32_t* count, float* out_s, float* out_u, float* out_d,
                                 const float* grad_s, const float* grad_u, const float* grad_d, float* grad_theta,
                                 float* grad_nom_s, double* qp_info, void* stream) {
  if (!h || batch < 1 || !nom_s || !nom_u || !ref_s || !ref_us || !out_s || !out_u || !grad_s || !grad_u || !grad_theta)
    return fail(NPA_E_ARG, "npa_nrmp_backward: bad argument");
  if (h->P.M > 0 && (!mu_sorted || !lam_sorted || !pts_sorted || !count || !out_d))
    return fail(NPA_E_ARG, "npa_nrmp_backward: obstacle arrays required when nrmp_max_num > 0");
  if (int rc = check_theta_batch(h, batch, "npa_nrmp_backward")) return rc;
  QpCall c{};
  c.cur_s_in = nom_s; c.cur_u_in = nom_u; c.ref_s = ref_s; c.ref_us = ref_us; c.mu_sorted = mu_sorted; c.lam_sorted = lam_sorted;
  c.pts_sorted = pts_sorted; c.count = count;
  c.cur_s_out = out_s; c.cur_u_out = out_u; c.cur_d_out = out_d; c.qp_info = qp_info; c.theta = h->theta;
  QpBackward extra{};
  extra.grad_s = grad_s; extra.grad_u = grad_u; extra.grad_d = grad_d; extra.grad_theta = grad_theta; extra.grad_nom_s = grad_nom_s;
  HIP_TRY(npa_launch_qp_backward(h->P, c, batch, extra, (hipStream_t)stream));
  return NPA_OK;
}

// staging of one forward call: working copy of the nominal trajectory, cleared flags / counts / state.  ONE body for the two
// kernels below.
__device__ __forceinline__ void stage_body(const StageCall& q, size_t ns, size_t nu, size_t nflag, size_t ncount, size_t nstate, int T,
                                           size_t nsched) {
  float* __restrict__ cur_s = q.cur_s; const float* __restrict__ nom_s = q.nom_s; float* __restrict__ cur_u = q.cur_u;
  const float* __restrict__ nom_u = q.nom_u; int* __restrict__ flags = q.flags; int* __restrict__ count = q.count;
  int* __restrict__ state = q.state; float* __restrict__ trig = q.trig; int* __restrict__ sched_cnt = q.sched_cnt;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;; i += stride) {
    bool any = false;
    if (i < ns) { cur_s[i] = nom_s[i]; any = true; }
    if (i < ncount) {                       // ncount = scenes x (T+1): one heading each
      const size_t b = i / (size_t)(T + 1), t = i - b * (size_t)(T + 1);
      float c, sn;
      npa_trig(nom_s[b * 3 * (size_t)(T + 1) + 2 * (size_t)(T + 1) + t], c, sn);
      trig[2 * i] = c; trig[2 * i + 1] = sn;
    }
    if (i < nu) { cur_u[i] = nom_u[i]; any = true; }
    if (i < nflag) { flags[i] = 0; any = true; }
    if (i < ncount) { count[i] = 0; any = true; }
    if (i < nstate) { state[i] = 0; any = true; }
    if (i < nsched) { sched_cnt[i] = 0; any = true; }      // the class counters of every QP launch of the call (pan_common.h)
    if (!any) break;
  }
}

__global__ void stage_kernel(float* __restrict__ cur_s, const float* __restrict__ nom_s, size_t ns,
                             float* __restrict__ cur_u, const float* __restrict__ nom_u, size_t nu,
                             int* __restrict__ flags, size_t nflag, int* __restrict__ count, size_t ncount,
                             int* __restrict__ state, size_t nstate, float* __restrict__ trig, int T,
                             int* __restrict__ sched_cnt, size_t nsched) {
  stage_body(StageCall{cur_s, nom_s, cur_u, nom_u, flags, count, state, trig, sched_cnt}, ns, nu, nflag, ncount, nstate, T, nsched);
}

// for a group of forward calls of one size (merged launches, pan_common.h): blockIdx.y = the call
__global__ void stage_group_kernel(StageGroup G, size_t ns, size_t nu, size_t nflag, size_t ncount, size_t nstate, int T,
                                   size_t nsched) {
  stage_body(G.c[blockIdx.y], ns, nu, nflag, ncount, nstate, T, nsched);
}

// what a staging launch covers, and its grid: one launch instead of two copies and up to three memsets (each costs tens of
// microseconds of stream time)
struct StageSizes { size_t ns, nu, nflag, ncount, nstate, nsched; int blocks; };
static const int kStageThreads = 256;
static StageSizes stage_sizes(const npa_handle* h, int batch, bool reset_state) {
  const int T = h->P.T;
  StageSizes z;
  z.ns = (size_t)batch * 3 * (T + 1); z.nu = (size_t)batch * 2 * T;
  z.nflag = (size_t)batch * 4; z.ncount = (size_t)batch * (T + 1);
  z.nstate = reset_state ? npa_state_bytes(h, batch) / 4 : 0;
  z.nsched = npa_sched_cnt_ints(h->P.K);
  const size_t work = std::max(std::max(std::max(z.ns, z.nu), z.nsched), std::max(std::max(z.nflag, z.ncount), z.nstate));
  z.blocks = (int)std::min<size_t>((work + kStageThreads - 1) / kStageThreads, 512);
  return z;
}

// The dispatch-order block of one QP launch (pan_common.h NPA_SCHED_NCLS; the kernels: nrmp_qp_device.h qp_sched_pick): launch j
// of a forward call -- counted since npa_forward_begin, every launch of the forward path covers the whole batch -- reads counter
// row j - 1 and list set (j - 1) & 1 (nothing for j = 0: scene order) and writes row j and set j & 1.  Beyond the K rows, or on
// a handle created under NPA_QP_ORDER=0, everything is null: scene order, nothing filed.
static QpSched sched_ptrs(const npa_handle* h, PendingCall* pc, const ScratchLayout& L) {
  QpSched s{nullptr, nullptr, nullptr, nullptr, nullptr};
  const int j = pc->qp_seq++;
  if (!h->qp_order || j >= h->P.K) return s;
  int* cnt = (int*)(pc->ws + L.sched);
  int* list = cnt + npa_sched_cnt_ints(h->P.K);
  const size_t set = (size_t)NPA_SCHED_NCLS * pc->batch;
  if (j > 0) { s.in_cnt = cnt + (size_t)(j - 1) * NPA_SCHED_NCLS; s.in_list = list + (size_t)((j - 1) & 1) * set; }
  s.out_cnt = cnt + (size_t)j * NPA_SCHED_NCLS; s.out_list = list + (size_t)(j & 1) * set;
  s.ticket = list + 2 * set;
  return s;
}

// ---- the records of one forward call's launches, from (handle, pending call, layout) -------------------------------------------
// Both the call-by-call path (npa_forward_begin / npa_forward_iter) and the merged one (npa_group_*_merged) launch from these.
static StageCall stage_call(const PendingCall& pc, const ScratchLayout& L) {
  StageCall s{};
  s.cur_s = pc.ws + L.cur_s; s.nom_s = pc.nom_s; s.cur_u = pc.ws + L.cur_u; s.nom_u = pc.nom_u;
  s.flags = (int*)(pc.ws + L.flags); s.count = (int*)(pc.ws + L.count); s.state = (int*)pc.state; s.trig = pc.ws + L.trig;
  s.sched_cnt = (int*)(pc.ws + L.sched);
  return s;
}

// (audit_seed stays 0: the caller that launches the geometric selection gives it h->launch_seq++)
static SelGeoCall sel_call(const npa_handle* h, const PendingCall& pc, const ScratchLayout& L) {
  float* ws = pc.ws;
  SelGeoCall s{};
  s.wpack = h->wpack; s.cur_s = ws + L.cur_s; s.points = pc.points; s.vel = pc.velocities; s.n_points = pc.n_points;
  s.flags = (const int*)(ws + L.flags); s.n_stride = pc.n_stride;
  s.mu_sorted = ws + L.mu; s.lam_sorted = ws + L.lam; s.pts_sorted = ws + L.pts; s.dist_sorted = ws + L.dist;
  s.count = (int*)(ws + L.count); s.stats = h->sel_stats_dev; s.trig = ws + L.trig;
  s.audit = h->rows_bf16 ? nullptr : h->audit_dev;
  return s;
}

// (counts a QP launch of the call: sched_ptrs)
static QpCall qp_call(const npa_handle* h, PendingCall* pc, const ScratchLayout& L) {
  float* ws = pc->ws;
  QpCall q{};
  q.cur_s_in = q.cur_s_out = ws + L.cur_s; q.cur_u_in = q.cur_u_out = ws + L.cur_u; q.cur_d_out = ws + L.cur_d;
  q.ref_s = pc->ref_s; q.ref_us = pc->ref_us;
  q.mu_sorted = ws + L.mu; q.lam_sorted = ws + L.lam; q.pts_sorted = ws + L.pts; q.dist_sorted = ws + L.dist;
  q.count = (const int*)(ws + L.count);
  q.out_s = pc->out_s; q.out_u = pc->out_u; q.out_d = pc->out_d; q.out_min_distance = pc->out_md; q.out_iters = pc->out_iters;
  q.out_nrmp_points = pc->out_np;
  q.flags = (int*)(ws + L.flags); q.state = pc->state; q.qp_info = (double*)(ws + L.qp_info);
  q.warm = h->qp_warm ? (double*)(ws + L.warm) : nullptr; q.trig_out = pc->dune ? ws + L.trig : nullptr;
  q.theta = pc->theta; q.sched = sched_ptrs(h, pc, L);
  return q;
}

// ---- forward = begin + K x iter + end ------------------------------------------------------------
// One forward call is a chain of launches on ONE stream: staging, then per PAN iteration the selection (preceded by
// the key launch when the handle uses network keys) and the QP.  Independent batches overlap by running on different
// streams (one handle each; neupan_amd.pan.forward_interleaved, bench.py): every kernel here is latency bound, and
// the waves of one batch fill the SIMDs the others leave idle.  The split into begin / iter / end exists for the
// callers that look at the working nominal between iterations (PAN.forward_batch_trace, the gradient chain).
// Network keys only.  Single fp16 products make the key launch ~25 % cheaper but put more points inside
// select_kernel's margin; when they do not fit the final ranking the slice re-encodes them exactly, ~3 key-tile units
// per tile.  Every 8 forward calls compare the two: if the re-encoded tiles cost more than the saving, use the split
// products for the next 256 calls, then try again.  (The outputs are bitwise the same in either mode; only the time
// differs.)  The counter is read from a pinned copy that trails the device by a call or two -- good enough for a policy.
static void key_policy(npa_handle* h, int batch, int n_stride) {
  if (!h->cal.key_auto) return;
  const DevParams& P = h->P;
  const unsigned now = *(volatile unsigned*)h->sel_stats_host;
  if (h->key_terms == 3) {
    if (--h->hold > 0) return;
    h->key_terms = 1; h->key_err = h->cal.err_mode[0]; h->key_e0 = h->cal.e0_mode[0];
    h->stats_mark = now; h->tiles_window = 0; h->calls_window = 0;
  } else if (h->calls_window >= 8) {
    const unsigned redone = now - h->stats_mark;
    if ((unsigned long long)redone * 12ull > h->tiles_window) {
      h->key_terms = 3; h->key_err = h->cal.err_mode[1]; h->key_e0 = h->cal.e0_mode[1]; h->hold = 256;
      return;
    }
    h->stats_mark = now; h->tiles_window = 0; h->calls_window = 0;
  }
  const int n_use = n_stride < P.dune_max_num ? n_stride : P.dune_max_num;
  h->tiles_window += (unsigned long long)batch * ((n_use + 31) / 32) * ((P.T + 1) + (size_t)(P.K - 1) * P.T);
  ++h->calls_window;
}

// npa_forward_begin on a call record (launch.h); launch_stage = false: everything except the staging launch (the merged group
// path stages all its calls with one launch, npa_group_begin_merged below)
int npa_forward_begin_call(const npa_forward_call& a, int flags, bool launch_stage) {
  npa_handle* h = a.h;
  if (!h || a.batch < 1 || !a.nom_s || !a.nom_u || !a.ref_s || !a.ref_us || !a.out_s || !a.out_u || !a.workspace || !a.state)
    return fail(NPA_E_ARG, "npa_forward_begin: null argument");
  const DevParams& P = h->P;
  if (P.M > 0 && !a.out_d) return fail(NPA_E_ARG, "npa_forward_begin: out_d required when nrmp_max_num > 0");
  if (a.workspace_bytes < npa_workspace_bytes(h, a.batch)) return fail(NPA_E_ARG, "workspace too small");
  if (a.state_bytes < npa_state_bytes(h, a.batch)) return fail(NPA_E_ARG, "state buffer too small");
  if (a.points && a.n_stride < 1) return fail(NPA_E_ARG, "n_stride < 1");
  if (a.points && (a.n_stride < P.dune_max_num ? a.n_stride : P.dune_max_num) > P.key_stride)
    return fail(NPA_E_UNSUPPORTED, "more than 32768 points per scene after decimation");
  std::lock_guard<std::mutex> lock(h->mu);
  PendingCall* pc = &h->pc;
  if (pc->active) return fail(NPA_E_ARG, "npa_forward_begin: previous forward on this handle not ended");
  if (int rc = check_theta_batch(h, a.batch, "npa_forward_begin")) return rc;
  pc->batch = a.batch; pc->n_stride = a.n_stride; pc->ref_s = a.ref_s; pc->ref_us = a.ref_us; pc->points = a.points;
  pc->velocities = a.velocities; pc->n_points = a.n_points; pc->out_s = a.out_s; pc->out_u = a.out_u; pc->out_d = a.out_d;
  pc->out_md = a.out_min_distance; pc->out_iters = a.out_iters; pc->out_np = a.out_nrmp_points; pc->ws = (float*)a.workspace;
  pc->state = (float*)a.state; pc->stream = (hipStream_t)a.stream;
  pc->dune = P.M > 0 && a.points != nullptr;
  pc->nom_s = a.nom_s; pc->nom_u = a.nom_u; pc->reset_state = (flags & NPA_FWD_RESET_STATE) != 0;
  pc->theta = h->theta;
  pc->qp_seq = 0;
  if (pc->dune) key_policy(h, a.batch, a.n_stride);
  if (launch_stage) {
    const StageCall s = stage_call(*pc, layout_of(h, a.batch));
    const StageSizes z = stage_sizes(h, a.batch, pc->reset_state);
    hipLaunchKernelGGL(stage_kernel, dim3(z.blocks), dim3(kStageThreads), 0, pc->stream, s.cur_s, s.nom_s, z.ns, s.cur_u, s.nom_u, z.nu,
                       s.flags, z.nflag, s.count, z.ncount, s.state, z.nstate, s.trig, P.T, s.sched_cnt, z.nsched);
    HIP_TRY(hipGetLastError());
  }
  pc->active = true;
  return NPA_OK;
}

extern "C" int npa_forward_begin(npa_handle* h, int batch, int n_stride, const float* nom_s, const float* nom_u,
                                 const float* ref_s, const float* ref_us, const float* points,
                                 const float* velocities, const int32_t* n_points, float* out_s, float* out_u,
                                 float* out_d, float* out_min_distance, int32_t* out_iters, float* out_nrmp_points,
                                 void* workspace, size_t workspace_bytes, void* state, size_t state_bytes,
                                 void* stream_, int flags) {
  npa_forward_call a{};                  // (iter_num is not begin's business: 0)
  a.h = h; a.batch = batch; a.n_stride = n_stride; a.nom_s = nom_s; a.nom_u = nom_u; a.ref_s = ref_s; a.ref_us = ref_us;
  a.points = points; a.velocities = velocities; a.n_points = n_points; a.out_s = out_s; a.out_u = out_u; a.out_d = out_d;
  a.out_min_distance = out_min_distance; a.out_iters = out_iters; a.out_nrmp_points = out_nrmp_points;
  a.workspace = workspace; a.workspace_bytes = workspace_bytes; a.state = state; a.state_bytes = state_bytes; a.stream = stream_;
  return npa_forward_begin_call(a, flags, true);
}

// ---- merged launches of a group of forward calls (npa_forward_batch_group, serve_group.hip) --------------------------------
// n calls qualify when one launch per stage can serve them all: one stream, one batch size, byte-identical kernel parameters,
// the default selection (geometric keys; exact or bf16 rows alike) and the register-resident interior-point solve, nothing
// that needs a launch of its own in between.  Everything else keeps the breadth-first call-by-call order.
int npa_group_mergeable(int n, const npa_forward_call* calls) {
  if (n < 2 || n > NPA_GROUP_MAX || !calls) return 0;
  static const bool off = getenv("NPA_GROUP_MERGE") != nullptr && atoi(getenv("NPA_GROUP_MERGE")) == 0;
  if (off) return 0;
  const npa_handle* h0 = calls[0].h;
  if (!h0) return 0;
  const DevParams& P = h0->P;
  const bool dune0 = P.M > 0 && calls[0].points != nullptr;
  if (dune0 && !(h0->key_terms == 4 && !h0->select_v1 && !h0->rows_bf16 && npa_select_geo_group_supported(P.E))) return 0;
  if (!npa_qp_group_supported(P.T, P.M) || h0->qp_generic || h0->cal.key_auto) return 0;
  if (calls[0].iter_num < 1 || calls[0].iter_num > P.K) return 0;       // (the call-by-call path reports that)
  for (int c = 0; c < n; ++c) {
    const npa_handle* h = calls[c].h;
    if (!h || calls[c].stream != calls[0].stream || calls[c].batch != calls[0].batch || calls[c].iter_num != calls[0].iter_num ||
        h->device != h0->device || memcmp(&h->P, &P, sizeof(DevParams)) != 0 || h->key_terms != h0->key_terms ||
        h->select_v1 != h0->select_v1 || h->rows_bf16 != h0->rows_bf16 || h->cal.keys_bf16 != h0->cal.keys_bf16 ||
        h->sel_debug != h0->sel_debug || h->audit_thresh != h0->audit_thresh || h->margin_scale != h0->margin_scale ||
        h->qp_generic != h0->qp_generic || h->qp_warm != h0->qp_warm || h->cal.key_auto ||
        (P.M > 0 && calls[c].points != nullptr) != dune0 || (calls[c].out_d == nullptr) != (calls[0].out_d == nullptr))
      return 0;
  }
  return 1;
}

extern "C" int npa_forward_group_merged(int n, const npa_forward_call* calls) { return npa_group_mergeable(n, calls); }

// The merged path reads and advances per-handle state of up to NPA_GROUP_MAX handles (pc, launch_seq, the profile events of the
// first): every member's mutex, taken in address order (two groups that share handles cannot deadlock), like begin / iter / end
// hold their handle's.  A concurrent call on a member handle from another thread waits instead of racing.
struct GroupLock {
  std::mutex* m[NPA_GROUP_MAX];
  int n = 0;
  GroupLock(int cnt, const npa_forward_call* calls) {
    for (int c = 0; c < cnt && n < NPA_GROUP_MAX; ++c)
      if (calls[c].h) m[n++] = &calls[c].h->mu;
    std::sort(m, m + n);
    n = (int)(std::unique(m, m + n) - m);
    for (int i = 0; i < n; ++i) m[i]->lock();
  }
  ~GroupLock() { for (int i = n - 1; i >= 0; --i) m[i]->unlock(); }
  GroupLock(const GroupLock&) = delete;
  GroupLock& operator=(const GroupLock&) = delete;
};

// begin of every call without its staging launch, then ONE staging launch for the group.  *begun = calls begun (the caller
// ends them whatever happens).
extern "C" int npa_group_begin_merged(int n, const npa_forward_call* calls, int flags, int* begun) {
  *begun = 0;
  for (int c = 0; c < n; ++c) {
    const int rc = npa_forward_begin_call(calls[c], flags, false);
    if (rc != NPA_OK) return rc;
    *begun = c + 1;
  }
  GroupLock group_lock(n, calls);
  npa_handle* h0 = calls[0].h;
  const int batch = calls[0].batch;
  const ScratchLayout L = layout_of(h0, batch);
  StageGroup G;
  memset(&G, 0, sizeof(G));
  for (int c = 0; c < n; ++c) G.c[c] = stage_call(calls[c].h->pc, L);
  const StageSizes z = stage_sizes(h0, batch, h0->pc.reset_state);
  hipLaunchKernelGGL(stage_group_kernel, dim3(z.blocks, n), dim3(kStageThreads), 0, h0->pc.stream, G, z.ns, z.nu, z.nflag, z.ncount,
                     z.nstate, h0->P.T, z.nsched);
  HIP_TRY(hipGetLastError());
  return NPA_OK;
}

// (diagnostics, exported through launch.h: merged QP launches issued by this process so far -- the tests check that the merged path ran)
static std::atomic<unsigned long long> g_merged_launches{0};
extern "C" unsigned long long npa_dbg_group_merged_launches(void) { return g_merged_launches.load(); }

// PAN iteration k of every call of the group: one selection launch, one QP launch (profile events: the first call's)
extern "C" int npa_group_iter_merged(int n, const npa_forward_call* calls, int k) {
  GroupLock group_lock(n, calls);
  npa_handle* h0 = calls[0].h;
  const DevParams& P = h0->P;
  if (k < 0 || k >= P.K) return fail(NPA_E_ARG, "npa_forward_batch_group: iteration index out of range");
  const int batch = calls[0].batch;
  const ScratchLayout L = layout_of(h0, batch);
  hipStream_t stream = h0->pc.stream;
  for (int c = 0; c < n; ++c)
    if (!calls[c].h->pc.active) return fail(NPA_E_ARG, "npa_forward_batch_group: a call of the group is not in progress");
  if (h0->pc.dune) {
    SelGeoGroup G;
    memset(&G, 0, sizeof(G));
    int n_stride_max = 1;
    for (int c = 0; c < n; ++c) {
      npa_handle* h = calls[c].h;
      G.c[c] = sel_call(h, h->pc, L);
      G.c[c].audit_seed = h->launch_seq++;
      if (h->pc.n_stride > n_stride_max) n_stride_max = h->pc.n_stride;
    }
    EventPair* evs = next_event(h0, h0->ev_sel, h0->n_sel);
    HIP_TRY(npa_launch_select_geo_group(P, G, n, batch, k == 0 ? 0 : 1, n_stride_max, 0, h0->audit_thresh, h0->margin_scale,
                                        rows_tier(h0), stream, evs ? evs->a : nullptr, evs ? evs->b : nullptr));
  }
  QpGroup Q;
  memset(&Q, 0, sizeof(Q));
  for (int c = 0; c < n; ++c) Q.c[c] = qp_call(calls[c].h, &calls[c].h->pc, L);
  EventPair* ev = next_event(h0, h0->ev_qp, h0->n_qp);
  HIP_TRY(npa_launch_qp_group(P, Q, n, batch, stream, ev ? ev->a : nullptr, ev ? ev->b : nullptr));
  g_merged_launches.fetch_add(1);
  return NPA_OK;
}

extern "C" int npa_forward_iter(npa_handle* h, int k) {
  if (!h) return fail(NPA_E_ARG, "npa_forward_iter: null handle");
  std::lock_guard<std::mutex> lock(h->mu);
  PendingCall* pc = &h->pc;
  if (!pc->active) return fail(NPA_E_ARG, "npa_forward_iter: no forward in progress on this handle");
  const DevParams& P = h->P;
  if (k < 0 || k >= P.K) return fail(NPA_E_ARG, "npa_forward_iter: iteration index out of range");
  const int batch = pc->batch;
  const bool geo = h->key_terms == 4;
  const ScratchLayout L = layout_of(h, batch);
  hipStream_t stream = pc->stream;
  if (pc->dune) {
    // slice 0 does not depend on the iterate (s(0) is pinned, robot.py:234): after the first iteration of a forward
    // call only slices 1..T are redone
    const int t0 = k == 0 ? 0 : 1;
    SelGeoCall sel = sel_call(h, *pc, L);
    unsigned* gkeys = (unsigned*)(pc->ws + L.keys);
    if (!geo) {
      EventPair* ev = next_event(h, h->ev_dune, h->n_dune);
      HIP_TRY(npa_launch_encode(P, sel, batch, t0, gkeys, h->n_cu, 5, h->key_terms, stream, ev ? ev->a : nullptr, ev ? ev->b : nullptr));
    }
    EventPair* evs = next_event(h, h->ev_sel, h->n_sel);
    if (geo && !h->select_v1) {
      sel.audit_seed = h->launch_seq++;
      HIP_TRY(npa_launch_select_geo(P, sel, batch, t0, 0, h->audit_thresh, h->margin_scale, rows_tier(h), stream,
                                    evs ? evs->a : nullptr, evs ? evs->b : nullptr));
    } else {
      HIP_TRY(npa_launch_select(P, sel, batch, t0, gkeys, h->key_terms, h->key_e0, 0, stream, evs ? evs->a : nullptr,
                                evs ? evs->b : nullptr));
    }
  }
  EventPair* ev = next_event(h, h->ev_qp, h->n_qp);
  HIP_TRY(npa_launch_qp(P, qp_call(h, pc, L), batch, QpBackward{}, stream, ev ? ev->a : nullptr, ev ? ev->b : nullptr));
  if (h->cal.key_auto && pc->dune && k == P.K - 1)
    HIP_TRY(hipMemcpyAsync(h->sel_stats_host, h->sel_stats_dev, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
  return NPA_OK;
}

extern "C" int npa_forward_end(npa_handle* h) {
  if (!h) return fail(NPA_E_ARG, "npa_forward_end: null handle");
  std::lock_guard<std::mutex> lock(h->mu);
  PendingCall* pc = &h->pc;
  if (!pc->active) return fail(NPA_E_ARG, "npa_forward_end: no forward in progress on this handle");
  pc->active = false;
  return NPA_OK;
}

extern "C" int npa_forward_batch_flags(npa_handle* h, int batch, int n_stride, const float* nom_s, const float* nom_u,
                                       const float* ref_s, const float* ref_us, const float* points,
                                       const float* velocities, const int32_t* n_points, float* out_s, float* out_u,
                                       float* out_d, float* out_min_distance, int32_t* out_iters, float* out_nrmp_points,
                                       void* workspace, size_t workspace_bytes, void* state, size_t state_bytes,
                                       void* stream_, int flags) {
  if (!h) return fail(NPA_E_ARG, "npa_forward_batch: null handle");
  int rc = npa_forward_begin(h, batch, n_stride, nom_s, nom_u, ref_s, ref_us, points, velocities, n_points, out_s,
                             out_u, out_d, out_min_distance, out_iters, out_nrmp_points, workspace, workspace_bytes,
                             state, state_bytes, stream_, flags);
  if (rc != NPA_OK) return rc;
  for (int k = 0; k < h->P.K; ++k) {
    rc = npa_forward_iter(h, k);
    if (rc != NPA_OK) { npa_forward_end(h); return rc; }
  }
  return npa_forward_end(h);
}

extern "C" int npa_forward_batch(npa_handle* h, int batch, int n_stride, const float* nom_s, const float* nom_u,
                                 const float* ref_s, const float* ref_us, const float* points,
                                 const float* velocities, const int32_t* n_points, float* out_s, float* out_u,
                                 float* out_d, float* out_min_distance, int32_t* out_iters, float* out_nrmp_points,
                                 void* workspace, size_t workspace_bytes, void* state, size_t state_bytes,
                                 void* stream_) {
  return npa_forward_batch_flags(h, batch, n_stride, nom_s, nom_u, ref_s, ref_us, points, velocities, n_points, out_s, out_u,
                                 out_d, out_min_distance, out_iters, out_nrmp_points, workspace, workspace_bytes, state,
                                 state_bytes, stream_, 0);
}

// ---- front end (frontend.hip) ----------------------------------------------------------------------
extern "C" int npa_nominal_ref_states(int batch, int receding, int kinematics, double step_time, double wheelbase,
                                      const double* state, const float* cur_vel, const double* ref_speed,
                                      const double* path, const int32_t* curve_off, const int32_t* curve_len,
                                      const int32_t* point_index, const double* interval, float* nom_s, float* nom_u,
                                      float* ref_s, float* ref_us, void* stream) {
  if (batch < 1 || !state || !ref_speed || !path || !curve_off || !curve_len || !point_index || !interval || !nom_s ||
      !nom_u || !ref_s || !ref_us)
    return fail(NPA_E_ARG, "npa_nominal_ref_states: bad argument");
  if (receding < 1 || receding > NPA_MAX_T) return fail(NPA_E_UNSUPPORTED, "receding outside [1,NPA_MAX_T]");
  if (kinematics < 0 || kinematics > 2) return fail(NPA_E_ARG, "unknown kinematics");
  if (kinematics == NPA_KIN_ACKER && !(wheelbase > 0)) return fail(NPA_E_ARG, "acker needs wheelbase > 0");
  HIP_TRY(npa_launch_nominal(batch, receding, kinematics, step_time, wheelbase, state, cur_vel, ref_speed, path,
                             curve_off, curve_len, point_index, interval, nom_s, nom_u, ref_s, ref_us,
                             (hipStream_t)stream));
  return NPA_OK;
}

extern "C" int npa_path_progress(int batch, const double* state, const double* path, const int32_t* curve_off,
                                 const int32_t* curve_len, int32_t* point_index, double close_threshold, int ind_range,
                                 double arrive_threshold, int arrive_index_threshold, float* min_dis, int32_t* arrived,
                                 void* stream) {
  if (batch < 1 || !state || !path || !curve_off || !curve_len || !point_index || !arrived || ind_range < 1)
    return fail(NPA_E_ARG, "npa_path_progress: bad argument");
  HIP_TRY(npa_launch_progress(batch, state, path, curve_off, curve_len, point_index, close_threshold, ind_range,
                              arrive_threshold, arrive_index_threshold, min_dis, arrived, (hipStream_t)stream));
  return NPA_OK;
}

extern "C" int npa_scan_to_points(int batch, int beam_stride, const double* ranges, const double* beam_vel,
                                  const int32_t* n_beams, const npa_scan_params* params, int mode, int out_stride,
                                  float* points, float* velocities, int32_t* count, void* stream) {
  if (batch < 1 || beam_stride < 1 || out_stride < 1 || !ranges || !params || !points || !count)
    return fail(NPA_E_ARG, "npa_scan_to_points: bad argument");
  if (mode != 0 && mode != 1) return fail(NPA_E_ARG, "npa_scan_to_points: mode must be 0 or 1");
  HIP_TRY(npa_launch_scan(batch, beam_stride, ranges, beam_vel, n_beams, params, mode, out_stride, points, velocities,
                          count, (hipStream_t)stream));
  return NPA_OK;
}

// ---- the bookkeeping of a device-resident closed loop (cycle.hip) ------------------------------------

extern "C" int npa_cycle_progress(int batch, const double* state, const double* path, const int32_t* curve_off,
                                  const int32_t* curve_len, const int32_t* robot_first, int loop, double close_threshold,
                                  int ind_range, double arrive_threshold, int arrive_index_threshold, int32_t* curve_index,
                                  int32_t* cur_off, int32_t* cur_len, int32_t* point_index, int32_t* curve_arrived,
                                  int32_t* arrived, npa_scan_params* params_a, npa_scan_params* params_b, void* stream) {
  if (batch < 1 || !state || !path || !curve_off || !curve_len || !robot_first || !curve_index || !cur_off || !cur_len ||
      !point_index || !curve_arrived || !arrived || !params_a || !params_b || ind_range < 1)
    return fail(NPA_E_ARG, "npa_cycle_progress: bad argument");
  // the arithmetic of the progress is progress_kernel's own, on every robot's CURRENT curve; the switch runs behind it
  HIP_TRY(npa_launch_progress(batch, state, path, cur_off, cur_len, point_index, close_threshold, ind_range, arrive_threshold,
                              arrive_index_threshold, nullptr, curve_arrived, (hipStream_t)stream));
  HIP_TRY(npa_launch_cycle_switch(batch, loop, state, curve_arrived, curve_off, curve_len, robot_first, curve_index, cur_off,
                                  cur_len, point_index, arrived, params_a, params_b, (hipStream_t)stream));
  return NPA_OK;
}

extern "C" int npa_cycle_act(int batch, int receding, int kinematics, int first_cycle, int cycle, const float* opt_u,
                             const float* min_distance, float collision_threshold, const int32_t* arrived,
                             const int32_t* collided, const float* override_row, const int32_t* n_points, float* cur_vel,
                             float* action, uint8_t* stop, int32_t* frozen, float* log_actions, uint8_t* log_stop,
                             float* log_controls, int32_t* log_n_points, void* stream) {
  if (batch < 1 || cycle < 0 || !opt_u || !min_distance || !arrived || !collided || !cur_vel || !action || !stop || !frozen)
    return fail(NPA_E_ARG, "npa_cycle_act: bad argument");
  if (receding < 1 || receding > NPA_MAX_T) return fail(NPA_E_ARG, "npa_cycle_act: receding outside [1,NPA_MAX_T]");
  if (kinematics < 0 || kinematics > 2) return fail(NPA_E_ARG, "npa_cycle_act: unknown kinematics");
  HIP_TRY(npa_launch_cycle_act(batch, receding, kinematics, first_cycle, cycle, opt_u, min_distance, collision_threshold, arrived,
                               collided, override_row, n_points, cur_vel, action, stop, frozen, log_actions, log_stop,
                               log_controls, log_n_points, (hipStream_t)stream));
  return NPA_OK;
}

extern "C" int npa_cycle_commit(int batch, int cycle, const double* state, const double* clearance, int32_t* collided,
                                double* log_states, double* log_clearance, void* stream) {
  if (batch < 1 || cycle < 0 || !state || !clearance || !collided) return fail(NPA_E_ARG, "npa_cycle_commit: bad argument");
  HIP_TRY(npa_launch_cycle_commit(batch, cycle, state, clearance, collided, log_states, log_clearance, (hipStream_t)stream));
  return NPA_OK;
}


extern "C" int npa_cycle_retask(int batch, int receding, int cycle, int style, double min_radius, const double* state,
                                int32_t* arrived, const int32_t* collided, double* path, const int32_t* curve_off,
                                int32_t* curve_len, const int32_t* robot_first, const int32_t* row_capacity, const double* goals,
                                int g_stride, const int32_t* n_goals, int32_t* goal_index, const double* interval,
                                int32_t* curve_index, int32_t* cur_off, int32_t* cur_len, int32_t* point_index, float* cur_vel,
                                int32_t* retask_status, int32_t* log_goal, void* stream) {
  const char* what = nullptr;
  if (batch < 1 || cycle < 0 || !state || !arrived || !collided || !path || !curve_off || !curve_len || !robot_first ||
      !row_capacity || !goals || !n_goals || !goal_index || !interval || !curve_index || !cur_off || !cur_len || !point_index ||
      !cur_vel || !retask_status)
    what = "npa_cycle_retask: bad argument";
  else if (receding < 1 || receding > NPA_MAX_T) what = "npa_cycle_retask: receding outside [1,NPA_MAX_T]";
  else if (style != NPA_CURVE_LINE && style != NPA_CURVE_DUBINS) what = "npa_cycle_retask: style outside 0..1";
  else if (style == NPA_CURVE_DUBINS && (!(min_radius > 0.0) || !std::isfinite(min_radius)))
    what = "npa_cycle_retask: dubins needs min_radius > 0";
  else if (g_stride < 1) what = "npa_cycle_retask: g_stride < 1";
  if (what) return fail(NPA_E_ARG, what);
  HIP_TRY(npa_launch_cycle_retask(batch, receding, cycle, style, min_radius, state, arrived, collided, path, curve_off, curve_len,
                                  robot_first, row_capacity, goals, g_stride, n_goals, goal_index, interval, curve_index, cur_off,
                                  cur_len, point_index, cur_vel, retask_status, log_goal, (hipStream_t)stream));
  return NPA_OK;
}

// ---- the packed input record (csrc/ingest.hip) ----
static int ingest_args_ok(int batch, int receding, int n_stride) {
  return batch >= 1 && receding >= 1 && receding <= NPA_MAX_T && n_stride >= 1;
}

extern "C" int npa_ingest_layout(int batch, int receding, int n_stride, int with_velocities, size_t* out, int n) {
  if (!ingest_args_ok(batch, receding, n_stride) || !out || n < 1 || n > 8)
    return fail(NPA_E_ARG, "npa_ingest_layout: bad argument");
  if (npa_ingest_offsets(batch, receding, n_stride, with_velocities != 0, out, n) != 0)
    return fail(NPA_E_ARG, "npa_ingest_layout: the cloud section would not fit int32 word offsets");
  return NPA_OK;
}

extern "C" int npa_ingest_unpack(int batch, int receding, int n_stride, int with_velocities, const void* record,
                                 size_t record_bytes, float* nom_s, float* nom_u, float* ref_s, float* ref_us, float* points,
                                 float* velocities, int32_t* n_points, int32_t* status, void* stream) {
  if (!ingest_args_ok(batch, receding, n_stride) || !record || !nom_s || !nom_u || !ref_s || !ref_us || !points ||
      !n_points || !status || (with_velocities && !velocities))
    return fail(NPA_E_ARG, "npa_ingest_unpack: bad argument");
  const void* ptrs[] = {record, nom_s, nom_u, ref_s, ref_us, points, velocities, n_points, status};
  for (const void* p : ptrs)
    if (((uintptr_t)p & 3) != 0) return fail(NPA_E_ARG, "npa_ingest_unpack: pointers must be 4-byte aligned");
  size_t off[8];
  if (npa_ingest_offsets(batch, receding, n_stride, with_velocities != 0, off, 8) != 0)
    return fail(NPA_E_ARG, "npa_ingest_unpack: the cloud section would not fit int32 word offsets");
  // the header and the dense sections must be inside what was uploaded; the cloud section may be cut short (ragged clouds)
  if (record_bytes < off[6] || record_bytes > off[7] || (record_bytes & 3) != 0)
    return fail(NPA_E_ARG, "npa_ingest_unpack: record_bytes must be a multiple of 4 between the cloud section's offset (" +
                               std::to_string(off[6]) + ") and the layout's total (" + std::to_string(off[7]) + "), got " +
                               std::to_string(record_bytes));
  HIP_TRY(npa_launch_ingest_unpack(batch, receding, n_stride, with_velocities != 0, record, record_bytes, nom_s, nom_u, ref_s,
                                   ref_us, points, velocities, n_points, status, (hipStream_t)stream));
  return NPA_OK;
}

// ---- exact clearance of a plan against the full cloud (csrc/clearance.hip) ----
extern "C" int npa_plan_clearance(npa_handle* h, int batch, int n_stride, const float* traj_s, const float* points,
                                  const float* velocities, const int32_t* n_points, float threshold, float* clearance,
                                  int32_t* nearest, float* min_clearance, int32_t* first_violation, void* stream) {
  // (everything that can be refused without the handle's content is refused first: no device call, no read of *h)
  if (!h || batch <= 0 || n_stride <= 0 || !traj_s || !points || !clearance || !nearest)
    return fail(NPA_E_ARG, "npa_plan_clearance: bad argument");
  const void* ptrs[] = {traj_s, points, velocities, n_points, clearance, nearest, min_clearance, first_violation};
  for (const void* p : ptrs)
    if (((uintptr_t)p & 3) != 0) return fail(NPA_E_ARG, "npa_plan_clearance: pointers must be 4-byte aligned");
  if (!h->geo_valid)
    return fail(NPA_E_UNSUPPORTED, "npa_plan_clearance: the robot polygon's rows are not consecutive counter-clockwise edges "
                                   "(no vertices could be derived from G, h)");
  HIP_TRY(npa_launch_clearance(h->P, batch, n_stride, traj_s, points, velocities, n_points, threshold, clearance, nearest,
                               min_clearance, first_violation, (hipStream_t)stream));
  return NPA_OK;
}

extern "C" int npa_dune_labels(int edge_num, const double* G, const double* h, int64_t n, const double* points,
                               float* mu, float* dist, void* stream) {
  if (!G || !h || n < 0 || (n > 0 && (!points || !mu || !dist))) return fail(NPA_E_ARG, "npa_dune_labels: bad argument");
  if (edge_num < 3 || edge_num > NPA_MAX_E) return fail(NPA_E_UNSUPPORTED, "edge_num outside [3,NPA_MAX_E]");
  HIP_TRY(npa_launch_labels(edge_num, G, h, (long long)n, points, mu, dist, (hipStream_t)stream));
  return NPA_OK;
}
