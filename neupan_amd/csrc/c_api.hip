// c_api.hip -- the extern "C" boundary of libneupan_amd.so (see include/neupan_amd.h).
// Host-side only: weight repacking, workspace carving, launch sequencing.  No torch types.
#include "../../include/neupan_amd.h"
#include "pan_common.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

extern "C" hipError_t npa_launch_encode(const DevParams& P, const float* wpack, int batch, int scene0, int t0,
                                        int n_stride, const float* cur_s, const float* points, const float* vel,
                                        const int* n_points, const int* flags, unsigned* gkeys, const float* trig,
                                        int n_cu, int blocks_per_cu, int key_terms, hipStream_t stream,
                                        hipEvent_t ev_start, hipEvent_t ev_stop);
extern "C" hipError_t npa_launch_trig(const float* cur_s, int batch, int T, float* trig, hipStream_t stream);
extern "C" hipError_t npa_launch_key_calib(const DevParams& P, const float* wpack, int key_terms, int nside, float half,
                                           unsigned* out, hipStream_t stream);
extern "C" hipError_t npa_launch_geo_table(const DevParams& P, float* wpack, float* nodes, int n_cu, hipStream_t stream);
extern "C" hipError_t npa_launch_ktab_calib(const DevParams& P, const float* wpack, int nside, float half, float inner, float cx, float cy,
                                            unsigned* out, int n_cu, hipStream_t stream);
extern "C" hipError_t npa_launch_geo_calib(const DevParams& P, const float* wpack, int nside, float half, float inner,
                                           float shift, unsigned* out, int n_cu, hipStream_t stream);
extern "C" hipError_t npa_launch_select_geo(const DevParams& P, const float* wpack, int batch, int scene0, int t0,
                                            int n_stride, const float* cur_s, const float* points, const float* vel,
                                            const int* n_points, const int* flags, const float* trig, float* mu_sorted,
                                            float* lam_sorted, float* pts_sorted, float* dist_sorted, int* count,
                                            unsigned* stats, int debug, unsigned* audit, unsigned audit_thresh,
                                            unsigned audit_seed, float margin_scale, int rows_bf16, hipStream_t stream,
                                            hipEvent_t ev_start, hipEvent_t ev_stop);
// Experiments on record (measured slower than the default path, or not finished) are compiled only with
// -DNPA_EXPERIMENTS (NPA_EXPERIMENTS=1 python -m neupan_amd.build): the active-set launch in front of the interior-point launch
// (aset_reduce.*), the first form of the geometric selection.  The default build has neither their kernels nor their environment
// knobs.  (Round 6 retired the two one-launch experiments -- the forward call as one launch, the selection with one wave per
// scene: a wave that walks the ten slices of its scene one after the other cannot win where launches are cheap and the chip is
// empty, and lost 2 x where it is full)
#ifdef NPA_EXPERIMENTS
#define NPA_VERSION_SUFFIX " +experiments"
#else
#define NPA_VERSION_SUFFIX ""
#endif
extern "C" hipError_t npa_launch_select(const DevParams& P, const float* wpack, int batch, int scene0, int t0,
                                        int n_stride, const float* cur_s, const float* points, const float* vel,
                                        const int* n_points, const int* flags, const unsigned* gkeys,
                                        const float* trig, float* mu_sorted, float* lam_sorted, float* pts_sorted,
                                        float* dist_sorted, int* count, int key_terms, float e0, unsigned* stats,
                                        int debug, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop);
extern "C" hipError_t npa_launch_qp(const DevParams& P, int batch, int scene0, const float* cur_s_in,
                                    const float* cur_u_in, const float* ref_s, const float* ref_us, const float* mu_sorted,
                                    const float* lam_sorted, const float* pts_sorted, const float* dist_sorted,
                                    const int* count, float* cur_s_out, float* cur_u_out, float* cur_d_out,
                                    float* out_s, float* out_u, float* out_d, float* out_min_distance,
                                    int* out_iters, float* out_nrmp_points, int* flags, float* state,
                                    double* qp_info, double* warm, float* trig_out, float* dbg_abc, float* dbg_f, double* dbg_x,
                                    hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop, int aset_launch, const float* theta);
extern "C" size_t npa_qp_shmem_bytes(int T, int M);
extern "C" int npa_select_geo_group_supported(int E);
extern "C" hipError_t npa_launch_k16_calib(const DevParams& P, const float* wpack, int nside, float half, float inner, unsigned* out,
                                           int n_cu, hipStream_t stream);
extern "C" hipError_t npa_launch_select_geo_group(const DevParams& P, const SelGeoGroup& G, int n, int batch, int t0, int n_stride_max,
                                                  int debug, unsigned audit_thresh, float margin_scale, int rows_bf16,
                                                  hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop);
extern "C" int npa_qp_group_supported(int T, int M);
extern "C" hipError_t npa_launch_qp_group(const DevParams& P, const QpGroup& G, int n, int batch, hipStream_t stream,
                                          hipEvent_t ev_start, hipEvent_t ev_stop);
extern "C" hipError_t npa_launch_nominal(int batch, int T, int kin, double dt, double L, const double* state,
                                         const float* vel, const double* ref_speed, const double* path,
                                         const int* curve_off, const int* curve_len, const int* point_index,
                                         const double* interval, float* nom_s, float* nom_u, float* ref_s,
                                         float* ref_us, hipStream_t stream);
extern "C" hipError_t npa_launch_scan(int batch, int beam_stride, const double* ranges, const double* beam_vel,
                                      const int* n_beams, const npa_scan_params* params, int mode, int out_stride,
                                      float* points, float* velocities, int* count, hipStream_t stream);
extern "C" int npa_ingest_offsets(int batch, int T, int n_stride, int with_vel, size_t* out, int n);
extern "C" hipError_t npa_launch_ingest_unpack(int batch, int T, int n_stride, int with_vel, const void* record,
                                               size_t record_bytes, float* nom_s, float* nom_u, float* ref_s, float* ref_us,
                                               float* points, float* velocities, int* n_points, int* status,
                                               hipStream_t stream);

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return fail(NPA_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

struct EventPair { hipEvent_t a, b; };

// state of a forward call between npa_forward_begin and npa_forward_end (one per handle: a handle plans one batch at a
// time; different handles are independent and may be driven from different host threads)
struct PendingCall {
  bool active = false;
  int batch = 0, n_stride = 0;
  const float *ref_s = nullptr, *ref_us = nullptr, *points = nullptr, *velocities = nullptr;
  const int32_t* n_points = nullptr;
  float *out_s = nullptr, *out_u = nullptr, *out_d = nullptr, *out_md = nullptr, *out_np = nullptr;
  int32_t* out_iters = nullptr;
  float* ws = nullptr;
  float* state = nullptr;
  hipStream_t stream = nullptr;
  bool dune = false;
  const float *nom_s = nullptr, *nom_u = nullptr;     // (the staging launch's sources: the merged group path launches it later)
  bool reset_state = false;
  const float* theta = nullptr;      // the handle's per-scene parameter block as it was when the call began (npa_set_adjust_batch)
};

// ---- one weight pack, one calibration and one key table per (checkpoint, polygon, knobs, device) per PROCESS -----------------
// The reference loads one model per planner (dune.py:131-144); a serving process makes tens of handles of the SAME checkpoint
// (one per batch in flight).  What npa_create derives from the checkpoint -- the repacked weights, the margins of the geometric
// key (6 x geo_calib_kernel), the 8.4 MB key table and its margins (4 x ktab_calib_kernel), the bf16 key margins -- is read-only
// after creation and a pure function of (the host image of the pack, E / G / h, the calibration knobs of the environment, the
// device): handles with the same key SHARE the device buffer and the measured figures.  The cache holds weak references: the
// buffer lives as long as a handle uses it.  Per handle: the audit block, statistics, the self-test and its outcomes, the key
// mode in force (npa_use_network_keys switches ONE handle).  NPA_PACK_CACHE=0 gives every handle a private pack (tests).
struct SharedPack {
  float* wpack = nullptr;
  int device = 0;
  // the figures the calibration leaves in the handle / its DevParams
  int key_terms = 0;
  float key_err = 0.f, key_e0 = 0.f;
  bool key_auto = false;
  float e0_mode[2] = {0.f, 0.f}, err_mode[2] = {0.f, 0.f};
  float geo_err = 0.f, geo_margin = 0.f, geo_refine = 0.f, geo_slope = 0.f, geo_rcal = 0.f, geo_far = 0.f;
  int geo_tab = 0;
  float ktab_err = 0.f, ktab_margin = 0.f;
  bool keys_bf16 = false;
  float k16_err = 0.f, k16_margin = 0.f;
  ~SharedPack() {
    if (!wpack) return;
    int cur = -1;
    const bool sw = hipGetDevice(&cur) == hipSuccess && cur != device;
    if (sw) (void)hipSetDevice(device);
    (void)hipFree(wpack);
    if (sw) (void)hipSetDevice(cur);
  }
};
static std::mutex g_pack_mu;                                   // held across a creation's calibration: same-key creates queue up
static std::map<std::string, std::weak_ptr<SharedPack>> g_packs;
static long long g_pack_calibrations = 0, g_pack_hits = 0;     // (npa_pack_cache_stats)

struct npa_handle {
  std::shared_ptr<SharedPack> pack;     // owns wpack (possibly with other handles)
  PendingCall pc;
  std::mutex mu;              // guards pc (two threads on ONE handle are a caller's bug; this makes it an error, not a race)
  DevParams P;
  // per-scene adjust parameters (npa_set_adjust_batch): a caller-owned DEVICE block [theta_batch][8] the QP launches read at run
  // time, or null: the uniform set in P.  Not part of P -- calls that differ in it still share a merged launch (QpCall::theta)
  const float* theta = nullptr;
  int theta_batch = 0;
  float* wpack = nullptr;     // device
  int device = 0;
  int n_cu = 256;
  float* stage_cand = nullptr;   // scratch of npa_dune_stage (keys, trig table), grown on demand
  size_t stage_cand_bytes = 0;
  // distance keys (dune_kernel): 1 = single fp16 products, 3 = fp16x2 split products, 0 = the exact fp32 encoder.
  // key_e0: select_kernel's candidate margin e0 (1 + |d|), a multiple of the key error measured at creation
  int key_terms = 1;                     // 4 = geometric keys computed by select_kernel itself (no dune_kernel launch)
  float key_e0 = 0.f, key_err = 0.f;
  bool qp_warm = true;                   // interior-point warm start across the PAN iterations of a forward call (NPA_QP_COLD=1: off)
  // NPA_SEL_DEBUG at creation: npa_dune_stage's count[] carries candidate statistics.  ONLY there: inside a forward call count[]
  // is the row count the QP kernel sizes its loops with (a debug word in it once sent the stop test ~200 k rows past its buffer)
  int sel_debug = 0;
  bool geo_valid = false;                // the polygon could be turned into vertices (consecutive CCW edges)
  float geo_err = 0.f, geo_margin = 0.f; // largest |network - geometric distance| / margin over the bands g in [0.25, 8] m
  // grid-refinement check of the margin (npa_create): largest ratio, over the bands, of |f| seen at the CELL CENTRES of a
  // calibration grid to what its nodes predicted for the space between them (node maximum + neighbour difference);
  // <= 1 when the grid resolves f.  geo_slope: largest neighbour difference / spacing on the finest grid (a Lipschitz
  // estimate of f next to the robot, m per m)
  float geo_refine = 0.f, geo_slope = 0.f;
  bool select_v1 = false;                // NPA_SELECT_V1: the first form of the geometric-key selection (select_kernel<E, true>)
  // run-time audit of the margin (select_geo_kernel): [0] audit tiles run, [1] points they checked, [2] bound violations seen
  // (candidates and audit tiles), [3] float bits of the largest excess |exact - g| - margin
  unsigned* audit_dev = nullptr;
  unsigned* audit_host = nullptr;        // pinned, host-mapped mirror of the violation count (words 6, 7 of audit_dev point at it)
  bool rows_bf16 = false;                // NPA_ROWS_PRECISION=bf16: the labelled reduced-precision tier of the rows (geometric keys, E = 4 / 8)
  // NPA_KEYS_PRECISION=bf16: the bf16 tier of the KEYS -- a slice whose candidate list overflows runs the list through the
  // bf16-MFMA encoder, keeps what lies within 2 x the measured |bf16 - exact| of the M-th smallest, re-encodes the survivors
  // exactly: the rows are bitwise those of the default path (BASELINE configs[4] "bf16 DUNE on MFMA", parity-holding reading)
  bool keys_bf16 = false;
  float k16_err = 0.f, k16_margin = 0.f; // largest measured |bf16 - exact| / margin over the bands g in [0, 8] m
  // the table-corrected geometric key (second-stage filter of long candidate lists, P.geo_tab; NPA_GEO_TABLE=0 switches it off):
  // largest measured |g + f_table - exact| / margin over the bands of the exact distance in [0, 8] m
  float ktab_err = 0.f, ktab_margin = 0.f;
  int selftest_flags = 0;                // NPA_SELFTEST_* : what the create-time self-test changed about this handle
  double key_safety = -1.0;              // NPA_KEY_SAFETY at creation (< 0: the defaults)
  unsigned audit_thresh = 0;             // fraction of the slice waves that run an audit tile, x 2^32
  unsigned launch_seq = 0;
  float margin_scale = 1.f;              // NPA_GEO_MARGIN_SCALE (tests only: a deliberately wrong margin)
  // key_auto: both reduced-precision modes are calibrated and the handle switches between them by what the
  // single-product keys cost in select_kernel (tiles it had to re-encode because more candidates fell inside the
  // margin than one tile holds -- walls at constant distance, dense clouds), see key_policy()
  bool key_auto = false;
  float e0_mode[2] = {0.f, 0.f}, err_mode[2] = {0.f, 0.f};        // [0] single, [1] split
  unsigned* sel_stats_dev = nullptr;     // cumulative overflow tiles (select_kernel)
  unsigned* sel_stats_host = nullptr;    // pinned copy, refreshed behind every forward call
  unsigned stats_mark = 0;
  unsigned long long tiles_window = 0;
  int calls_window = 0, hold = 0;
  // profiling (bench.py): HIP events on the launch stream around every stage launch
  bool prof = false;
  std::vector<EventPair> ev_dune, ev_sel, ev_qp, ev_aset;
  size_t n_dune = 0, n_sel = 0, n_qp = 0, n_aset = 0;
  double last_aset_ms = 0.0;             // average of the active-set launches seen by the last npa_profile_read
  long long last_aset_n = 0;
  int aset_min_batch = 32;               // NPA_QP_ASET_MIN_BATCH: smallest batch that gets the extra active-set launch when NPA_QP_ASET=1
  // a call of very few scenes is bound by the LATENCY of its solves (one wave each, nothing else on the chip), not by wave
  // slots; measured over 24 scenes one at a time (profiles/r04_latency_breakdown.txt) the active-set launch from PAN iteration
  // 4 on takes 2.5 % off the mean and 9 % off the median of a single-scene call -- too little to put another code path on the
  // default single-scene route, so the rule ships switched off: NPA_QP_ASET_SMALL=1 (largest batch it applies to) turns it on,
  // NPA_QP_ASET_FROM moves its first iteration.
  bool aset_auto = true, qp_generic = false;
  int aset_small_batch = 0, aset_from_iter = 4;
  bool qp_scan_wide = true;              // (NPA_QP_NOSCAN_WIDE unset: the wide-scan T = 20 instantiation; experiments build only otherwise)
};

extern "C" const char* npa_last_error(void) { return g_err.c_str(); }
#ifndef NPA_HIPCC_VERSION
#define NPA_HIPCC_VERSION "unknown"
#endif
extern "C" const char* npa_version(void) { return "neupan_amd 0.4 (gfx950, hipcc " NPA_HIPCC_VERSION ")" NPA_VERSION_SUFFIX; }
static int mdim(const DevParams& P) { return P.M > 0 ? P.M : 1; }
// per-slice stride of the key buffer inside the workspace: none with geometric keys (select_kernel keeps them in LDS)
static int kstride(const npa_handle* h) { return h->key_terms == 4 ? 0 : h->P.key_stride; }

// Network keys (dune_kernel): measure the key error of the single-product (1) and the split-product (3) mode on a
// 1024 x 1024 grid over the training square and pick the cheapest mode whose margin stays under its cap; neither -> the
// exact fp32 encoder (0).  forced = 1 / 3 pins a mode (NPA_KEY_TERMS), < 0 = automatic.  Also the fallback of a handle
// whose geometric keys were rejected (self-test) or distrusted at run time (npa_use_network_keys).
static hipError_t calibrate_network_keys(npa_handle* h, int forced) {
  const DevParams& P = h->P;
  unsigned* dmax = nullptr;
  const int modes[2] = {1, 3};
  const float floor_e0[2] = {1e-4f, 2e-5f}, cap_e0[2] = {5e-2f, 1e-3f};
  bool ok[2] = {false, false};
  const double sf = h->key_safety > 0 ? h->key_safety : 5.0;
  hipError_t e = hipMalloc(&dmax, sizeof(unsigned));
  for (int m = 0; m < 2 && e == hipSuccess; ++m) {
    if (forced > 0 && forced != modes[m]) continue;
    unsigned bits = 0;
    e = hipMemset(dmax, 0, sizeof(unsigned));
    if (e == hipSuccess) e = npa_launch_key_calib(P, h->wpack, modes[m], 1024, 25.0f, dmax, nullptr);
    if (e == hipSuccess) e = hipMemcpy(&bits, dmax, sizeof(unsigned), hipMemcpyDeviceToHost);
    if (e != hipSuccess) break;
    float err;
    memcpy(&err, &bits, sizeof(err));
    h->err_mode[m] = err;
    h->e0_mode[m] = std::max((float)(sf * err), floor_e0[m]);
    ok[m] = h->e0_mode[m] <= cap_e0[m] || forced == modes[m];
  }
  if (dmax) hipFree(dmax);
  if (e != hipSuccess) return e;
  const int pick = ok[0] ? 0 : (ok[1] ? 1 : -1);
  h->key_terms = 0; h->key_err = 0.f; h->key_e0 = 0.f;
  if (pick >= 0) { h->key_terms = modes[pick]; h->key_err = h->err_mode[pick]; h->key_e0 = h->e0_mode[pick]; }
  h->key_auto = forced < 0 && ok[0] && ok[1];
  return hipSuccess;
}

// the audit block: words 0..4 counters (npa_audit_read), 6..7 the address of the pinned host mirror of the violation count
static hipError_t audit_block_reset(npa_handle* h) {
  if (!h->audit_dev) return hipSuccess;
  unsigned blk[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  void* mirror = nullptr;                        // the device's address of the pinned counter
  if (h->audit_host && hipHostGetDevicePointer(&mirror, h->audit_host, 0) != hipSuccess) mirror = nullptr;
  memcpy(&blk[6], &mirror, sizeof(mirror));
  if (h->audit_host) *(volatile unsigned*)h->audit_host = 0;
  return hipMemcpy(h->audit_dev, blk, sizeof(blk), hipMemcpyHostToDevice);
}

static int npa_self_test(npa_handle* h);
extern "C" int npa_create(const npa_config* cfg, const npa_dune_weights* w, npa_handle** out) {
  if (!cfg || !out) return fail(NPA_E_ARG, "npa_create: null argument");
  if (cfg->receding < 1 || cfg->receding > NPA_MAX_T) return fail(NPA_E_UNSUPPORTED, "receding outside [1,NPA_MAX_T]");
  if (cfg->nrmp_max_num < 0 || cfg->nrmp_max_num > NPA_MAX_M) return fail(NPA_E_UNSUPPORTED, "nrmp_max_num outside [0,NPA_MAX_M]");
  if (cfg->edge_num < 3 || cfg->edge_num > NPA_MAX_E) return fail(NPA_E_UNSUPPORTED, "edge_num outside [3,NPA_MAX_E]");
  if (cfg->kinematics < 0 || cfg->kinematics > 2) return fail(NPA_E_ARG, "unknown kinematics");
  if (cfg->iter_num < 1) return fail(NPA_E_ARG, "iter_num < 1");
  if (npa_qp_shmem_bytes(cfg->receding, cfg->nrmp_max_num) > 160 * 1024) return fail(NPA_E_UNSUPPORTED, "T*M too large for LDS");
  const bool need_w = cfg->nrmp_max_num > 0 && cfg->dune_max_num > 0;
  if (need_w && !w) return fail(NPA_E_ARG, "DUNE weights required unless nrmp_max_num == 0 or dune_max_num == 0");

  npa_handle* h = new npa_handle();
  DevParams& P = h->P;
  memset(&P, 0, sizeof(P));
  P.T = cfg->receding; P.M = (cfg->dune_max_num > 0) ? cfg->nrmp_max_num : 0; P.E = cfg->edge_num;
  P.kin = cfg->kinematics; P.K = cfg->iter_num; P.dune_max_num = cfg->dune_max_num;
  {
    long long n = cfg->dune_max_num > 0 ? cfg->dune_max_num : 1;
    if (n > NPA_MAX_POINTS) n = NPA_MAX_POINTS;
    P.key_stride = (int)((n + 31) / 32 * 32);
  }
  P.iter_threshold = cfg->iter_threshold;
  P.dt = cfg->step_time; P.dt32 = (float)cfg->step_time; P.L = cfg->wheelbase;
  for (int k = 0; k < 2; ++k) { P.speed_bound[k] = cfg->speed_bound[k]; P.acce_bound[k] = cfg->acce_bound[k]; }
  P.ro_obs = cfg->ro_obs; P.bk = cfg->bk;
  for (int k = 0; k < 3; ++k) P.q_s[k] = cfg->q_s[k];
  P.p_u = cfg->p_u; P.eta = cfg->eta; P.d_max = cfg->d_max; P.d_min = cfg->d_min;
  for (int e = 0; e < NPA_MAX_E; ++e) { P.G[e][0] = cfg->G[e][0]; P.G[e][1] = cfg->G[e][1]; P.h[e] = cfg->h[e]; }
  // Vertices of {x : G x <= h} for the geometric distance keys: vertex e = edges e-1 and e, which holds when the rows
  // are consecutive counter-clockwise edges (util.gen_inequal_from_vertex, util/__init__.py:161-206, produces them
  // so).  Any other row order fails the check below and the handle keeps network keys.
  {
    const int E = P.E;
    double V[NPA_MAX_E][2];
    bool ok = true;
    for (int e = 0; e < E && ok; ++e) {
      const int p = e == 0 ? E - 1 : e - 1;
      const double a = P.G[p][0], b = P.G[p][1], c = P.G[e][0], d = P.G[e][1];
      const double det = a * d - b * c;
      if (!(det > 0.0)) { ok = false; break; }                 // counter-clockwise turn from edge e-1 to edge e
      V[e][0] = ((double)P.h[p] * d - b * (double)P.h[e]) / det;
      V[e][1] = (a * (double)P.h[e] - (double)P.h[p] * c) / det;
    }
    for (int e = 0; e < E && ok; ++e) {
      const int n = e + 1 == E ? 0 : e + 1;
      const double dx = V[n][0] - V[e][0], dy = V[n][1] - V[e][1], l2 = dx * dx + dy * dy;
      // edge e must run along row e: G_e parallel to (dy, -dx), and every vertex must satisfy every row
      const double gn = std::sqrt((double)P.G[e][0] * P.G[e][0] + (double)P.G[e][1] * P.G[e][1]);
      if (!(l2 > 0.0) || !(gn > 0.0) || std::fabs(P.G[e][0] * dx + P.G[e][1] * dy) > 1e-5 * gn * std::sqrt(l2) ||
          !(P.G[e][0] * dy - P.G[e][1] * dx > 0.0))
        ok = false;
      for (int r = 0; r < E && ok; ++r)
        if (P.G[r][0] * V[e][0] + P.G[r][1] * V[e][1] - P.h[r] > 1e-5 * (1.0 + std::fabs((double)P.h[r]))) ok = false;
      P.pvx[e] = (float)V[e][0]; P.pvy[e] = (float)V[e][1]; P.pdx[e] = (float)dx; P.pdy[e] = (float)dy;
      P.pil[e] = l2 > 0.0 ? (float)(1.0 / l2) : 0.f;
    }
    h->geo_valid = ok;
    P.geo_rcal = 0.f;
    // axis-aligned rectangle?  (edges alternately parallel to x and y: every vertex shares x or y with its successor)
    P.geo_rect = 0;
    if (ok && E == 4) {
      bool rect = true;
      double xmin = 1e300, xmax = -1e300, ymin = 1e300, ymax = -1e300;
      for (int e = 0; e < 4; ++e) {
        const int n = (e + 1) & 3;
        const double dx = std::fabs(V[n][0] - V[e][0]), dy = std::fabs(V[n][1] - V[e][1]);
        if (!(dx <= 1e-9 * (1 + dy) || dy <= 1e-9 * (1 + dx))) rect = false;
        xmin = std::min(xmin, V[e][0]); xmax = std::max(xmax, V[e][0]);
        ymin = std::min(ymin, V[e][1]); ymax = std::max(ymax, V[e][1]);
      }
      if (rect) {
        P.geo_rect = 1;
        P.rcx = (float)(0.5 * (xmin + xmax)); P.rcy = (float)(0.5 * (ymin + ymax));
        P.rhx = (float)(0.5 * (xmax - xmin)); P.rhy = (float)(0.5 * (ymax - ymin));
      }
    }
  }

  std::vector<float> pack(WP_TOTAL, 0.f);
  for (int i = 0; i < NPA_GEO_BANDS; ++i) pack[WP_GEO + i] = pack[WP_KTAB + i] = INFINITY;
  {
    // header of the key table (pan_common.h, WP_TABH): its squares are centred on the polygon's bounding box
    float xmin = 3e38f, xmax = -3e38f, ymin = 3e38f, ymax = -3e38f;
    for (int e = 0; e < P.E && h->geo_valid; ++e) {
      xmin = std::min(xmin, P.pvx[e]); xmax = std::max(xmax, P.pvx[e]); ymin = std::min(ymin, P.pvy[e]); ymax = std::max(ymax, P.pvy[e]);
    }
    const bool okb = h->geo_valid && xmax >= xmin && ymax >= ymin;
    const float h0 = okb ? std::max(NPA_TAB_HALF0, 1.25f * 0.5f * std::max(xmax - xmin, ymax - ymin)) : NPA_TAB_HALF0;
    pack[WP_TABH] = okb ? 0.5f * (xmin + xmax) : 0.f; pack[WP_TABH + 1] = okb ? 0.5f * (ymin + ymax) : 0.f;
    pack[WP_TABH + 2] = h0; pack[WP_TABH + 3] = 0.5f * (float)NPA_TAB_N / h0;
    // a polygon that is not an axis-aligned box: its bounding box (grown by 10 um: it must CONTAIN the polygon in fp32) for the
    // key pass, and the slack S = the largest distance from a corner of that box to the polygon
    pack[WP_TABH + 4] = 0.f;
    if (okb && !P.geo_rect) {
      P.rcx = 0.5f * (xmin + xmax); P.rcy = 0.5f * (ymin + ymax);
      P.rhx = 0.5f * (xmax - xmin) + 1e-5f; P.rhy = 0.5f * (ymax - ymin) + 1e-5f;
      double S = 0.0;
      for (int cxs = -1; cxs <= 1; cxs += 2)
        for (int cys = -1; cys <= 1; cys += 2) {
          const double qx = (double)P.rcx + cxs * (double)P.rhx, qy = (double)P.rcy + cys * (double)P.rhy;
          double best = 1e300;
          for (int e = 0; e < P.E; ++e) {
            const double rx = qx - P.pvx[e], ry = qy - P.pvy[e];
            double t = (rx * P.pdx[e] + ry * P.pdy[e]) * P.pil[e];
            t = std::min(std::max(t, 0.0), 1.0);
            const double ux = rx - t * P.pdx[e], uy = ry - t * P.pdy[e];
            best = std::min(best, ux * ux + uy * uy);
          }
          S = std::max(S, std::sqrt(best));
        }
      pack[WP_TABH + 4] = (float)(S * (1.0 + 1e-5) + 1e-5);
    }
  }
  if (need_w) {
    const int E = P.E;
    for (int l = 0; l < 64; ++l) pack[WP_W1 + l] = w->lin_w[0][(l & 31) * 2 + (l >> 5)];   // A[i][k] = W1[i][k]
    for (int L = 0; L < 4; ++L)
      for (int r = 0; r < 16; ++r)
        for (int l = 0; l < 64; ++l)
          pack[WP_WLS + (L * 64 + l) * 16 + r] = pack[WP_WL + (L * 16 + r) * 64 + l] = w->lin_w[1 + L][(l & 31) * 32 + npa_feat(r, l >> 5)];
    auto putv = [&](int slot, const float* src, float scale) {
      for (int i = 0; i < 32; ++i) pack[WP_VEC + slot * 32 + i] = src[i] * scale;
    };
    // the LayerNorm affine feeds tanh only: pre-scale gamma/beta by 2*log2(e) so the kernel's
    // tanh is exp2 + rcp + fma with no extra multiply (dune.hip: tanh_scaled)
    const float k2 = 2.885390081777927f;
    putv(V_B1, w->lin_b[0], 1.f); putv(V_G1, w->ln_w[0], k2); putv(V_BE1, w->ln_b[0], k2);
    putv(V_B2, w->lin_b[1], 1.f);
    putv(V_B3, w->lin_b[2], 1.f); putv(V_G2, w->ln_w[1], k2); putv(V_BE2, w->ln_b[1], k2);
    putv(V_B4, w->lin_b[3], 1.f);
    putv(V_B5, w->lin_b[4], 1.f); putv(V_G3, w->ln_w[2], k2); putv(V_BE3, w->ln_b[2], k2);
    for (int e = 0; e < E; ++e) {
      memcpy(&pack[WP_W6 + e * 32], w->lin_w[5] + e * 32, 32 * sizeof(float));
      pack[WP_B6 + e] = w->lin_b[5][e];
    }
    // the 16-point tile's images (pan_common.h, WP_W116): row i of block mb of a layer's A-fragments is output feature
    // npa_feat16(4 mb + (i & 3), i >> 2), K entry (s, kq) is input feature npa_feat16(s, kq)
    {
      auto fo = [](int mb, int row) { return npa_feat16(4 * mb + (row & 3), row >> 2); };
      for (int mb = 0; mb < 2; ++mb)
        for (int l = 0; l < 64; ++l)
          pack[WP_W116 + mb * 64 + l] = (l >> 4) < 2 ? w->lin_w[0][fo(mb, l & 15) * 2 + (l >> 4)] : 0.f;
      for (int L = 0; L < 4; ++L)
        for (int l = 0; l < 64; ++l)
          for (int s = 0; s < 8; ++s)
            for (int mb = 0; mb < 2; ++mb)
              pack[WP_WL16 + (L * 64 + l) * 16 + 2 * s + mb] = w->lin_w[1 + L][fo(mb, l & 15) * 32 + npa_feat16(s, l >> 4)];
      for (int v = 0; v < 11 + 8; ++v)               // (the eleven vectors, then the eight rows of Linear(32,E): WP_W6 follows WP_VEC)
        for (int kq = 0; kq < 4; ++kq)
          for (int s = 0; s < 8; ++s)
            pack[WP_VEC16 + v * 32 + kq * 8 + s] = pack[WP_VEC + v * 32 + npa_feat16(s, kq)];
      for (int e = 0; e < 8; ++e) pack[WP_VEC16 + 19 * 32 + e] = pack[WP_B6 + e];
    }
    // ---- key path (dune_kernel): see pan_common.h --------------------------------------------------
    // LayerNorm centring folded into Linear 1, 3, 5 (fp64, rounded once)
    std::vector<float> wkey[4];                       // the four 32x32 layers as the key path sees them
    for (int L = 0; L < 4; ++L) wkey[L].assign(w->lin_w[1 + L], w->lin_w[1 + L] + 32 * 32);
    auto centre_cols = [](const float* W, int ncol, float* out) {   // out = (I - 11'/32) W, W is [32][ncol]
      for (int c = 0; c < ncol; ++c) {
        double m = 0;
        for (int i = 0; i < 32; ++i) m += (double)W[i * ncol + c];
        m /= 32.0;
        for (int i = 0; i < 32; ++i) out[i * ncol + c] = (float)((double)W[i * ncol + c] - m);
      }
    };
    centre_cols(w->lin_w[2], 32, wkey[1].data());     // Linear 3
    centre_cols(w->lin_w[4], 32, wkey[3].data());     // Linear 5
    float bkey[5][32];                                // biases of Linear 1..5 as the key path sees them
    {
      float w1c[32 * 2];
      centre_cols(w->lin_w[0], 2, w1c);
      for (int l = 0; l < 64; ++l) pack[WP_KW1 + l] = w1c[(l & 31) * 2 + (l >> 5)];
      centre_cols(w->lin_b[0], 1, bkey[0]);
      memcpy(bkey[1], w->lin_b[1], sizeof(bkey[1]));
      centre_cols(w->lin_b[2], 1, bkey[2]);
      memcpy(bkey[3], w->lin_b[3], sizeof(bkey[3]));
      centre_cols(w->lin_b[4], 1, bkey[4]);
    }
    // exact power-of-two scales.  tanh outputs are produced as 2^10 * tanh; a Linear->ReLU layer
    // (key layers 0, 2) gets the largest weight scale for which its output provably fits fp16
    // (|z_i| <= sum_j |W_ij| + |b_i| because |tanh| <= 1); a Linear->LayerNorm layer (1, 3) is
    // scale-free downstream, its weights are scaled into [512, 1024).
    const double TANH_SCALE = 1024.0;
    double sig_out[4];                                 // scale of each key layer's accumulator
    double wscale[4];
    for (int L = 0; L < 4; ++L) {
      double wmax = 0, bound = 0;
      for (int i = 0; i < 32; ++i) {
        double r = std::fabs((double)bkey[1 + L][i]);
        for (int jx = 0; jx < 32; ++jx) {
          r += std::fabs((double)wkey[L][i * 32 + jx]);
          wmax = std::max(wmax, std::fabs((double)wkey[L][i * 32 + jx]));
        }
        bound = std::max(bound, r);
      }
      if (!(wmax > 0)) wmax = 1;
      if (L == 0 || L == 2) {
        const double sig_in = TANH_SCALE;
        int e = (int)std::floor(std::log2(30000.0 / (sig_in * std::max(bound, 1e-30))));
        e = std::max(-14, std::min(14, e));
        while (e > -14 && std::ldexp(wmax, e) > 30000.0) --e;
        wscale[L] = std::ldexp(1.0, e);
        sig_out[L] = sig_in * wscale[L];
      } else {
        const double sig_in = sig_out[L - 1];
        int e = (int)std::floor(std::log2(1023.0 / wmax));
        e = std::max(-14, std::min(24, e));
        wscale[L] = std::ldexp(1.0, e);
        sig_out[L] = sig_in * wscale[L];
      }
    }
    for (int i = 0; i < 32; ++i) {
      pack[WP_KVEC + 0 * 32 + i] = bkey[0][i];
      for (int L = 0; L < 4; ++L) pack[WP_KVEC + (1 + L) * 32 + i] = (float)((double)bkey[1 + L][i] * sig_out[L]);
    }
    pack[WP_KSC + 0] = 1e-5f;
    pack[WP_KSC + 1] = (float)(1e-5 * sig_out[1] * sig_out[1]);
    pack[WP_KSC + 2] = (float)(1e-5 * sig_out[3] * sig_out[3]);
    pack[WP_KSC + 3] = (float)TANH_SCALE;              // after LayerNorm 1, 2: feeds a split layer
    pack[WP_KSC + 4] = (float)TANH_SCALE;
    pack[WP_KSC + 5] = 1.0f;                           // after LayerNorm 3: feeds the output layer
    {
      // bf16 A-fragments of the exact network's four 32x32 layers (RNE), for the reduced-precision tier of the rows
      uint16_t* wb = reinterpret_cast<uint16_t*>(&pack[WP_WB16]);
      auto to_bf16 = [](float f) -> uint16_t {
        uint32_t u;
        memcpy(&u, &f, 4);
        if ((u & 0x7F800000u) == 0x7F800000u) return (uint16_t)(u >> 16);        // inf / nan: truncate
        u += 0x7FFFu + ((u >> 16) & 1u);                                           // round to nearest even
        return (uint16_t)(u >> 16);
      };
      for (int L = 0; L < 4; ++L)
        for (int s2 = 0; s2 < 2; ++s2)
          for (int l = 0; l < 64; ++l)
            for (int q = 0; q < 8; ++q)
              wb[(((size_t)L * 2 + s2) * 64 + l) * 8 + q] = to_bf16(w->lin_w[1 + L][(l & 31) * 32 + npa_feat(8 * s2 + q, l >> 5)]);
    }
    _Float16* kh = reinterpret_cast<_Float16*>(&pack[WP_BF]);
    for (int L = 0; L < 4; ++L)
      for (int s2 = 0; s2 < 2; ++s2)
        for (int l = 0; l < 64; ++l)
          for (int q = 0; q < 8; ++q) {
            const float wv = (float)((double)wkey[L][(l & 31) * 32 + npa_feat(8 * s2 + q, l >> 5)] * wscale[L]);
            const _Float16 h1 = (_Float16)wv;                       // RNE
            const _Float16 h2 = (_Float16)(wv - (float)h1);
            kh[((((size_t)L * 2 + 0) * 2 + s2) * 64 + l) * 8 + q] = h1;
            kh[((((size_t)L * 2 + 1) * 2 + s2) * 64 + l) * 8 + q] = h2;
          }
  }
  h->sel_debug = getenv("NPA_SEL_DEBUG") != nullptr;
  h->qp_warm = getenv("NPA_QP_COLD") == nullptr;
  h->qp_generic = getenv("NPA_QP_GENERIC") != nullptr;
  P.qp_aset = 0;
#ifdef NPA_EXPERIMENTS
  h->qp_scan_wide = getenv("NPA_QP_NOSCAN_WIDE") == nullptr;
  P.qp_aset = (getenv("NPA_QP_ASET") != nullptr && atoi(getenv("NPA_QP_ASET")) != 0) ? 1 : 0;
  h->aset_auto = getenv("NPA_QP_ASET") == nullptr;
  if (const char* env = getenv("NPA_QP_ASET_SMALL")) { int v = atoi(env); if (v >= 0) h->aset_small_batch = v; }
  if (const char* env = getenv("NPA_QP_ASET_FROM")) { int v = atoi(env); if (v >= 1) h->aset_from_iter = v; }
  if (const char* env = getenv("NPA_QP_ASET_MIN_BATCH")) { int v = atoi(env); if (v >= 1) h->aset_min_batch = v; }
#endif
  hipError_t e = hipGetDevice(&h->device);
  if (e == hipSuccess) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0)
      h->n_cu = prop.multiProcessorCount;
  }
  // the pack's identity (SharedPack above): host image + polygon + calibration knobs + device
  std::string pack_key;
  {
    static const char* const knobs[] = {"NPA_DUNE_FP32KEYS", "NPA_KEY_TERMS", "NPA_KEY_SAFETY", "NPA_GEO_GRID", "NPA_GEO_NOCHECK",
                                        "NPA_GEO_TABLE", "NPA_KTAB_SAFETY", "NPA_KEYS_PRECISION", "NPA_K16_SAFETY", "NPA_ROWS_PRECISION"};
    pack_key.assign(reinterpret_cast<const char*>(pack.data()), pack.size() * sizeof(float));
    pack_key.append(reinterpret_cast<const char*>(&P.E), sizeof(P.E));
    pack_key.append(reinterpret_cast<const char*>(P.G), sizeof(P.G));
    pack_key.append(reinterpret_cast<const char*>(P.h), sizeof(P.h));
    pack_key.append(reinterpret_cast<const char*>(&h->device), sizeof(h->device));
    pack_key.push_back(need_w ? 'w' : '-');
    for (const char* k : knobs) { const char* v = getenv(k); pack_key.push_back('|'); if (v) pack_key.append(v); else pack_key.push_back('\x01'); }
  }
  const bool use_cache = !(getenv("NPA_PACK_CACHE") && atoi(getenv("NPA_PACK_CACHE")) == 0);
  std::unique_lock<std::mutex> pack_lock(g_pack_mu);
  bool pack_hit = false;
  if (e == hipSuccess && use_cache) {
    auto it = g_packs.find(pack_key);
    if (it != g_packs.end()) {
      h->pack = it->second.lock();
      if (!h->pack) g_packs.erase(it);
    }
    pack_hit = (bool)h->pack;
  }
  if (e == hipSuccess && !pack_hit) {
    h->pack = std::make_shared<SharedPack>();
    h->pack->device = h->device;
    e = hipMalloc(&h->pack->wpack, ((size_t)WP_TAB + WP_TAB_FLOATS) * sizeof(float));      // (the pack, then the key table)
    if (e == hipSuccess) e = hipMemcpy(h->pack->wpack, pack.data(), WP_TOTAL * sizeof(float), hipMemcpyHostToDevice);
  }
  if (h->pack) h->wpack = h->pack->wpack;
  // Key mode and candidate margin.  Distance KEYS only nominate candidates (select_kernel re-encodes them with the
  // exact network and ranks on the exact result), so their error decides nothing but how many candidates there are
  // -- PROVIDED the margin covers it.  The error is a property of the checkpoint and is measured here:
  //  * geometric keys (mode 4, preferred): |network distance - closed-form distance to the polygon| per distance
  //    band on three nested 4096 x 4096 grids (half extents 8 / 32 / 128 m, spacing 4 / 16 / 63 mm, each skipping
  //    the square the finer one covers); margin[band] = NPA_KEY_SAFETY (default 1.5 here: the error is a smooth
  //    deterministic function, not rounding noise) x (max |f| + max neighbour difference of f), over the band and
  //    its two neighbours.  Used when the margin stays <= 0.15 m over the bands g in [0.25, 8] m, where the M
  //    nearest points of a slice normally lie; a checkpoint that fits the geometry worse than that (a quick fit, a
  //    foreign polygon) keeps network keys;
  //  * network keys from dune_kernel: single fp16 products (1) when e0 = 5 x the largest |key - exact| / (1 + |exact|)
  //    on a 1024 x 1024 grid over |x|, |y| <= 25 m stays below 5e-2, else fp16x2 split products (3), else the exact
  //    encoder (0).
  // NPA_DUNE_FP32KEYS=1 / NPA_KEY_TERMS=1|3|4 force a mode (tests).
  if (e == hipSuccess && need_w) {
    int forced = -1;
    if (getenv("NPA_DUNE_FP32KEYS")) forced = 0;
    else if (const char* env = getenv("NPA_KEY_TERMS")) { int v = atoi(env); if (v == 1 || v == 3 || v == 4) forced = v; }
    double safety = -1.0;
    if (const char* env = getenv("NPA_KEY_SAFETY")) { double v = atof(env); if (v >= 1.0 && v <= 1e3) safety = v; }
    h->key_terms = 0;
    bool geo_ok = false;
    if (pack_hit) {
      // a handle of the same key measured all of this already: its figures, no launches
      const SharedPack& S = *h->pack;
      h->key_terms = S.key_terms; h->key_err = S.key_err; h->key_e0 = S.key_e0; h->key_auto = S.key_auto;
      for (int m = 0; m < 2; ++m) { h->e0_mode[m] = S.e0_mode[m]; h->err_mode[m] = S.err_mode[m]; }
      h->geo_err = S.geo_err; h->geo_margin = S.geo_margin; h->geo_refine = S.geo_refine; h->geo_slope = S.geo_slope;
      P.geo_rcal = S.geo_rcal; P.geo_far = S.geo_far; P.geo_tab = S.geo_tab;
      h->ktab_err = S.ktab_err; h->ktab_margin = S.ktab_margin;
      geo_ok = S.key_terms == 4;
      ++g_pack_hits;
    } else if (h->geo_valid && (forced < 0 || forced == 4)) {
      unsigned* tab = nullptr;
      e = hipMalloc(&tab, 2 * NPA_GEO_BANDS * sizeof(unsigned));
      if (e == hipSuccess) e = hipMemset(tab, 0, 2 * NPA_GEO_BANDS * sizeof(unsigned));
      const float halves[3] = {8.f, 32.f, 128.f};
      // NPA_GEO_GRID (tests): nodes per side of the three calibration grids (default 4096; a multiple of 8)
      int nside = 4096;
      if (const char* env = getenv("NPA_GEO_GRID")) { int v = atoi(env); if (v >= 64 && v <= 8192) nside = v / 8 * 8; }
      for (int gI = 0; gI < 3 && e == hipSuccess; ++gI)
        e = npa_launch_geo_calib(P, h->wpack, nside, halves[gI], gI == 0 ? 0.f : 0.97f * halves[gI - 1], 0.f, tab, h->n_cu, nullptr);
      // the same three grids shifted by half a cell: their nodes are the cell centres of the first pass
      unsigned* tab2 = nullptr;
      if (e == hipSuccess) e = hipMalloc(&tab2, 2 * NPA_GEO_BANDS * sizeof(unsigned));
      if (e == hipSuccess) e = hipMemset(tab2, 0, 2 * NPA_GEO_BANDS * sizeof(unsigned));
      for (int gI = 0; gI < 3 && e == hipSuccess; ++gI)
        e = npa_launch_geo_calib(P, h->wpack, nside, halves[gI], gI == 0 ? 0.f : 0.97f * halves[gI - 1], 0.5f, tab2, h->n_cu, nullptr);
      unsigned bits[2 * NPA_GEO_BANDS], bits2[2 * NPA_GEO_BANDS];
      if (e == hipSuccess) e = hipMemcpy(bits, tab, sizeof(bits), hipMemcpyDeviceToHost);
      if (e == hipSuccess) e = hipMemcpy(bits2, tab2, sizeof(bits2), hipMemcpyDeviceToHost);
      if (tab) hipFree(tab);
      if (tab2) hipFree(tab2);
      if (e == hipSuccess) {
        const double sf = safety > 0 ? safety : 1.5;
        float raw[NPA_GEO_BANDS], mg[NPA_GEO_BANDS];
        bool seen[NPA_GEO_BANDS];
        // Refinement check.  The margin rests on "between the nodes f stays within (node maximum + neighbour difference)".
        // The cell centres are where that is most at risk; they were just measured: per band (with its two neighbours, a
        // centre may fall into the next band) the largest |f| at the centres over what the nodes predicted.  A ratio above 1
        // means the grid does not resolve f (a ridge narrower than a cell): the checkpoint keeps network keys.  No Lipschitz
        // constant of the network gives a usable analytic bound (LayerNorm divides by a data-dependent deviation: the
        // product of the layer norms is 1e6 and more for the shipped checkpoints, tests/tools/lipschitz_bound.py), so the
        // claim is checked where it can fail, and audited at run time (select_geo_kernel).
        float refine = 0.f, slope = 0.f;
        {
          float pred[NPA_GEO_BANDS], cen[NPA_GEO_BANDS];
          for (int bnd = 0; bnd < NPA_GEO_BANDS; ++bnd) {
            float f0, f1, c0;
            memcpy(&f0, &bits[bnd], 4); memcpy(&f1, &bits[NPA_GEO_BANDS + bnd], 4); memcpy(&c0, &bits2[bnd], 4);
            pred[bnd] = f0 + f1; cen[bnd] = c0;
          }
          for (int bnd = 0; bnd < NPA_GEO_BANDS; ++bnd) {
            if (bits2[bnd] == 0u) continue;
            float pr = 0.f;
            for (int q = std::max(bnd - 1, 0); q <= std::min(bnd + 1, NPA_GEO_BANDS - 1); ++q) pr = std::max(pr, pred[q]);
            pr = std::max(pr, 1e-3f);                  // (below a millimetre the ratio is rounding noise, and irrelevant)
            if (!(cen[bnd] < 1e30f)) { refine = INFINITY; continue; }
            refine = std::max(refine, cen[bnd] / pr);
          }
          // steepest neighbour difference next to the robot (bands below 8 m are on the finest grid) per metre
          const float h0 = 2.0f * halves[0] / (float)(nside - 1);
          for (int bnd = 0; bnd <= npa_geo_band(6.0f); ++bnd) {
            float f1;
            memcpy(&f1, &bits[NPA_GEO_BANDS + bnd], 4);
            if (f1 < 1e30f) slope = std::max(slope, f1 / h0);
          }
        }
        h->geo_refine = refine; h->geo_slope = slope;
        for (int bnd = 0; bnd < NPA_GEO_BANDS; ++bnd) {
          float f0, f1, c0, c1;
          memcpy(&f0, &bits[bnd], 4); memcpy(&f1, &bits[NPA_GEO_BANDS + bnd], 4);
          memcpy(&c0, &bits2[bnd], 4); memcpy(&c1, &bits2[NPA_GEO_BANDS + bnd], 4);
          seen[bnd] = bits[bnd] != 0u || bits[NPA_GEO_BANDS + bnd] != 0u || bits2[bnd] != 0u;
          raw[bnd] = std::max(f0, c0) + std::max(f1, c1);      // both grids feed the margin
        }
        float worst_err = 0.f, worst_margin = 0.f;
        for (int bnd = 0; bnd < NPA_GEO_BANDS; ++bnd) {
          float m = -1.f;
          for (int q = std::max(bnd - 1, 0); q <= std::min(bnd + 1, NPA_GEO_BANDS - 1); ++q)
            if (seen[q]) m = std::max(m, raw[q]);
          // a band no grid point fell into (beyond the corners of the largest square) stays uncalibrated: +inf
          mg[bnd] = (m < 0.f || !(m < 1e30f)) ? INFINITY : std::max((float)(sf * m), 1e-4f);
          if (bnd >= npa_geo_band(0.25f) && bnd <= npa_geo_band(8.0f)) {
            worst_margin = std::max(worst_margin, mg[bnd]);
            float f0;
            memcpy(&f0, &bits[bnd], 4);
            worst_err = std::max(worst_err, f0);
          }
        }
        h->geo_err = worst_err; h->geo_margin = worst_margin;
        // (1.25, not 1: a centre may legitimately exceed the nodes' prediction by a little where f is curved; the margin
        // carries a factor 1.5 on top of the prediction)
        const bool resolved = refine <= 1.25f || getenv("NPA_GEO_NOCHECK") != nullptr;
        geo_ok = ((worst_margin <= 0.15f && resolved) || forced == 4);
        if (geo_ok) {
          e = hipMemcpy(h->wpack + WP_GEO, mg, sizeof(mg), hipMemcpyHostToDevice);
          P.geo_rcal = halves[2];
          {
            double rmax = 0;
            for (int v = 0; v < P.E; ++v) rmax = std::max(rmax, std::sqrt((double)P.pvx[v] * P.pvx[v] + (double)P.pvy[v] * P.pvy[v]));
            P.geo_far = (float)std::max(1.0, (double)halves[2] - rmax);
          }
          h->key_terms = 4; h->key_err = worst_err; h->key_e0 = worst_margin;
        }
      }
      // The correction table of the geometric key and the margin of the corrected key (pan_common.h, WP_TAB / WP_KTAB): f at
      // the nodes of the four squares, then |g + f_table - exact| per band of the exact distance on the calibration grids
      // (whose nodes drift through every offset inside a cell).  Margin = NPA_KTAB_SAFETY (default 2) x the largest residual over
      // the band and its two neighbours, at least 0.1 mm; every survivor of the filter is audited against it at run time.
      const char* tab_env = getenv("NPA_GEO_TABLE");
      if (e == hipSuccess && geo_ok && (P.E == 4 || P.E == 8) && !(tab_env && atoi(tab_env) == 0)) {
        float* nodes = nullptr;
        unsigned* tabk = nullptr;
        e = hipMalloc(&nodes, (size_t)NPA_TAB_LEVELS * (NPA_TAB_N + 1) * (NPA_TAB_N + 1) * sizeof(float));
        if (e == hipSuccess) e = npa_launch_geo_table(P, h->wpack, nodes, h->n_cu, nullptr);
        if (e == hipSuccess) e = hipMalloc(&tabk, NPA_GEO_BANDS * sizeof(unsigned));
        if (e == hipSuccess) e = hipMemset(tabk, 0, NPA_GEO_BANDS * sizeof(unsigned));
        // (one calibration square per level of the table, nside^2 nodes each: 8 x 8 samples per cell at the default 4096)
        const float th0 = pack[WP_TABH + 2];
        const float khalves[NPA_TAB_LEVELS] = {th0, 4.f * th0, 16.f * th0, 64.f * th0};
        for (int gI = 0; gI < NPA_TAB_LEVELS && e == hipSuccess; ++gI)
          e = npa_launch_ktab_calib(P, h->wpack, nside, khalves[gI], gI == 0 ? 0.f : 0.97f * khalves[gI - 1], pack[WP_TABH], pack[WP_TABH + 1],
                                    tabk, h->n_cu, nullptr);
        unsigned kb[NPA_GEO_BANDS];
        if (e == hipSuccess) e = hipMemcpy(kb, tabk, sizeof(kb), hipMemcpyDeviceToHost);
        if (nodes) hipFree(nodes);
        if (tabk) hipFree(tabk);
        if (e == hipSuccess) {
          double sfk = 2.0;
          if (const char* e2 = getenv("NPA_KTAB_SAFETY")) { double v = atof(e2); if (v >= 1.0 && v <= 100.0) sfk = v; }
          float raw[NPA_GEO_BANDS], mk[(NPA_GEO_BANDS + 3) & ~3];
          for (int bnd = 0; bnd < NPA_GEO_BANDS; ++bnd) memcpy(&raw[bnd], &kb[bnd], 4);
          for (int bnd = 0; bnd < (int)(sizeof(mk) / sizeof(mk[0])); ++bnd) mk[bnd] = INFINITY;
          float worst = 0.f, worst_m = 0.f;
          for (int bnd = 0; bnd < NPA_GEO_BANDS; ++bnd) {
            float m = -1.f;
            for (int q = std::max(bnd - 1, 0); q <= std::min(bnd + 1, NPA_GEO_BANDS - 1); ++q)
              if (kb[q] != 0u) m = std::max(m, raw[q]);
            mk[bnd] = (m < 0.f || !(m < 1e30f)) ? INFINITY : std::max((float)(sfk * m), 1e-4f);
            if (bnd <= npa_geo_band(8.0f) && m >= 0.f) { worst = std::max(worst, m); worst_m = std::max(worst_m, mk[bnd]); }
          }
          h->ktab_err = worst; h->ktab_margin = worst_m;
          e = hipMemcpy(h->wpack + WP_KTAB, mk, sizeof(mk), hipMemcpyHostToDevice);
          if (e == hipSuccess) P.geo_tab = 1;
        }
      }
    }
    h->key_safety = safety;
    if (!pack_hit && !geo_ok && e == hipSuccess && forced != 0 && forced != 4) e = calibrate_network_keys(h, forced);
    // word 0: overflow tiles of the selection (key policy); words 1 .. 3 spare (npa_dbg_select_stats)
    if (e == hipSuccess) e = hipMalloc(&h->sel_stats_dev, 4 * sizeof(unsigned));
    if (e == hipSuccess) e = hipMemset(h->sel_stats_dev, 0, 4 * sizeof(unsigned));
    if (e == hipSuccess) e = hipHostMalloc(&h->sel_stats_host, sizeof(unsigned), hipHostMallocDefault);
    if (e == hipSuccess) *h->sel_stats_host = 0;
    if (e == hipSuccess) e = hipMalloc(&h->audit_dev, 8 * sizeof(unsigned));       // [4]: launches seen (device side)
    if (e == hipSuccess) e = hipHostMalloc(&h->audit_host, sizeof(unsigned), hipHostMallocMapped);
    if (e == hipSuccess) e = audit_block_reset(h);
#ifdef NPA_EXPERIMENTS
    h->select_v1 = getenv("NPA_SELECT_V1") != nullptr;
#endif
    if (const char* env = getenv("NPA_ROWS_PRECISION")) {
      if (!strcmp(env, "bf16")) {
        if (e == hipSuccess && !(h->key_terms == 4 && !h->select_v1 && (P.E == 4 || P.E == 8))) {
          pack_lock.unlock(); npa_destroy(h);
          return fail(NPA_E_UNSUPPORTED, "NPA_ROWS_PRECISION=bf16 needs geometric keys (select_geo_kernel) and a polygon of 4 or 8 edges");
        }
        h->rows_bf16 = true;
      } else if (strcmp(env, "fp32") != 0) {
        pack_lock.unlock(); npa_destroy(h);
        return fail(NPA_E_ARG, "NPA_ROWS_PRECISION must be fp32 or bf16");
      }
    }
    if (const char* env = getenv("NPA_KEYS_PRECISION")) {
      if (!strcmp(env, "bf16")) {
        if (e == hipSuccess && !(h->key_terms == 4 && !h->select_v1 && !h->rows_bf16 && (P.E == 4 || P.E == 8))) {
          pack_lock.unlock(); npa_destroy(h);
          return fail(NPA_E_UNSUPPORTED, "NPA_KEYS_PRECISION=bf16 needs geometric keys, exact rows and a polygon of 4 or 8 edges");
        }
        // margin per band of the exact distance: safety (NPA_KEY_SAFETY, default 2: rounding noise sampled on 3 M grid nodes,
        // and every survivor is audited at run time) x the largest |bf16 - exact| over the band and its two neighbours
        if (pack_hit) {                                    // (measured by the handle that made the pack: NPA_KEYS_PRECISION is part of its key)
          h->k16_err = h->pack->k16_err; h->k16_margin = h->pack->k16_margin; h->keys_bf16 = h->pack->keys_bf16;
        } else {
        unsigned* tab = nullptr;
        if (e == hipSuccess) e = hipMalloc(&tab, NPA_GEO_BANDS * sizeof(unsigned));
        if (e == hipSuccess) e = hipMemset(tab, 0, NPA_GEO_BANDS * sizeof(unsigned));
        const float halves[3] = {8.f, 32.f, 128.f};
        for (int gI = 0; gI < 3 && e == hipSuccess; ++gI)
          e = npa_launch_k16_calib(P, h->wpack, 1024, halves[gI], gI == 0 ? 0.f : 0.97f * halves[gI - 1], tab, h->n_cu, nullptr);
        unsigned bits[NPA_GEO_BANDS];
        if (e == hipSuccess) e = hipMemcpy(bits, tab, sizeof(bits), hipMemcpyDeviceToHost);
        if (tab) hipFree(tab);
        if (e == hipSuccess) {
          double sf = 2.0;
          if (const char* e2 = getenv("NPA_K16_SAFETY")) { double v = atof(e2); if (v >= 1.0 && v <= 100.0) sf = v; }
          float raw[NPA_GEO_BANDS], mg[(NPA_GEO_BANDS + 3) & ~3];
          for (int bnd = 0; bnd < NPA_GEO_BANDS; ++bnd) memcpy(&raw[bnd], &bits[bnd], 4);
          for (int bnd = 0; bnd < (int)(sizeof(mg) / sizeof(mg[0])); ++bnd) mg[bnd] = INFINITY;
          float worst = 0.f, worst_m = 0.f;
          for (int bnd = 0; bnd < NPA_GEO_BANDS; ++bnd) {
            float m = -1.f;
            for (int q = std::max(bnd - 1, 0); q <= std::min(bnd + 1, NPA_GEO_BANDS - 1); ++q)
              if (bits[q] != 0u) m = std::max(m, raw[q]);
            mg[bnd] = (m < 0.f || !(m < 1e30f)) ? INFINITY : std::max((float)(sf * m), 1e-5f);
            if (bnd <= npa_geo_band(8.0f) && m >= 0.f) { worst = std::max(worst, m); worst_m = std::max(worst_m, mg[bnd]); }
          }
          h->k16_err = worst; h->k16_margin = worst_m;
          e = hipMemcpy(h->wpack + WP_K16, mg, sizeof(mg), hipMemcpyHostToDevice);
          h->keys_bf16 = true;
        }
        }
      } else if (strcmp(env, "fp32") != 0) {
        pack_lock.unlock(); npa_destroy(h);
        return fail(NPA_E_ARG, "NPA_KEYS_PRECISION must be fp32 or bf16");
      }
    }
    {
      double rate = 1.0 / 64.0;              // audit tiles: one slice wave in 64 (NPA_AUDIT_RATE in [0, 1]; 0 = candidates only)
      if (const char* env = getenv("NPA_AUDIT_RATE")) { double v = atof(env); if (v >= 0.0 && v <= 1.0) rate = v; }
      h->audit_thresh = rate >= 1.0 ? 0xFFFFFFFFu : (unsigned)(rate * 4294967296.0);
      if (const char* env = getenv("NPA_GEO_MARGIN_SCALE")) { double v = atof(env); if (v > 0.0 && v <= 100.0) h->margin_scale = (float)v; }
    }
  }
  if (e != hipSuccess) {
    pack_lock.unlock();
    npa_destroy(h);                                      // releases whatever was created so far
    return fail(NPA_E_HIP, std::string("npa_create: ") + hipGetErrorString(e));
  }
  if (!pack_hit && h->pack) {
    // the figures for the handles that follow (the device buffer is complete: every write to it happened above)
    SharedPack& S = *h->pack;
    S.key_terms = h->key_terms; S.key_err = h->key_err; S.key_e0 = h->key_e0; S.key_auto = h->key_auto;
    for (int m = 0; m < 2; ++m) { S.e0_mode[m] = h->e0_mode[m]; S.err_mode[m] = h->err_mode[m]; }
    S.geo_err = h->geo_err; S.geo_margin = h->geo_margin; S.geo_refine = h->geo_refine; S.geo_slope = h->geo_slope;
    S.geo_rcal = P.geo_rcal; S.geo_far = P.geo_far; S.geo_tab = P.geo_tab;
    S.ktab_err = h->ktab_err; S.ktab_margin = h->ktab_margin;
    S.keys_bf16 = h->keys_bf16; S.k16_err = h->k16_err; S.k16_margin = h->k16_margin;
    if (need_w) ++g_pack_calibrations;
    if (use_cache) g_packs[pack_key] = h->pack;
  }
  pack_lock.unlock();
  if (!getenv("NPA_SKIP_SELFTEST")) {
    const int rc = npa_self_test(h);
    if (rc != NPA_OK) {
      const std::string msg = g_err;
      npa_destroy(h);
      return fail(rc, msg);
    }
  }
  *out = h;
  return NPA_OK;
}

static void drop_pending(npa_handle* h);
extern "C" int npa_destroy(npa_handle* h) {
  if (!h) return NPA_OK;
  drop_pending(h);
  {
    // launches of this handle may still be queued on streams it does not own (and a 4-byte counter copy into its
    // pinned buffer behind the last forward call): let the device finish before anything is freed
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess) {
      if (cur != h->device) (void)hipSetDevice(h->device);
      (void)hipDeviceSynchronize();
      if (cur != h->device) (void)hipSetDevice(cur);
    }
    (void)hipGetLastError();
  }
  for (auto& p : h->ev_dune) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
  for (auto& p : h->ev_sel) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
  for (auto& p : h->ev_qp) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
  for (auto& p : h->ev_aset) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
  h->wpack = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_pack_mu);           // (the last owner frees the buffer; a create of the same key waits or misses)
    h->pack.reset();
  }
  if (h->sel_stats_dev) hipFree(h->sel_stats_dev);
  if (h->sel_stats_host) hipHostFree(h->sel_stats_host);
  if (h->audit_dev) hipFree(h->audit_dev);
  if (h->audit_host) hipHostFree(h->audit_host);
  if (h->stage_cand) hipFree(h->stage_cand);
  delete h;
  return NPA_OK;
}

extern "C" int npa_key_mode(const npa_handle* h, int* key_terms, float* measured_error, float* margin_e0) {
  if (!h) return fail(NPA_E_ARG, "npa_key_mode: null handle");
  if (key_terms) *key_terms = h->key_terms;
  if (measured_error) *measured_error = h->key_err;
  if (margin_e0) *margin_e0 = h->key_e0;
  return NPA_OK;
}

extern "C" int npa_pack_cache_stats(int64_t* calibrations, int64_t* shared_creates, int64_t* alive) {
  std::lock_guard<std::mutex> lk(g_pack_mu);
  if (calibrations) *calibrations = g_pack_calibrations;
  if (shared_creates) *shared_creates = g_pack_hits;
  if (alive) {
    int64_t n = 0;
    for (auto& kv : g_packs) n += kv.second.expired() ? 0 : 1;
    *alive = n;
  }
  return NPA_OK;
}

extern "C" int npa_geo_report(const npa_handle* h, float* out, int n) {
  if (!h || !out || n < 1) return fail(NPA_E_ARG, "npa_geo_report: bad argument");
  const float v[10] = {h->geo_valid ? 1.f : 0.f, h->geo_err, h->geo_margin, h->geo_refine, h->geo_slope, h->P.geo_far,
                       h->keys_bf16 ? h->k16_err : 0.f, h->keys_bf16 ? h->k16_margin : 0.f,
                       h->P.geo_tab ? h->ktab_err : 0.f, h->P.geo_tab ? h->ktab_margin : 0.f};
  for (int i = 0; i < n && i < 10; ++i) out[i] = v[i];
  return NPA_OK;
}

extern "C" int npa_audit_read(npa_handle* h, uint64_t* tiles, uint64_t* points, uint64_t* violations, float* worst_excess, int reset) {
  if (!h) return fail(NPA_E_ARG, "npa_audit_read: null handle");
  unsigned v[4] = {0, 0, 0, 0};
  if (h->audit_dev) {
    int cur = -1;
    HIP_TRY(hipGetDevice(&cur));
    if (cur != h->device) HIP_TRY(hipSetDevice(h->device));
    hipError_t e = hipDeviceSynchronize();          // the counters of every queued launch of this handle
    if (e == hipSuccess) e = hipMemcpy(v, h->audit_dev, sizeof(v), hipMemcpyDeviceToHost);
    if (e == hipSuccess && reset) {
      e = hipMemset(h->audit_dev, 0, sizeof(v));
      if (h->audit_host) *(volatile unsigned*)h->audit_host = 0;
    }
    if (cur != h->device) (void)hipSetDevice(cur);
    HIP_TRY(e);
  }
  if (tiles) *tiles = v[0];
  if (points) *points = v[1];
  if (violations) *violations = v[2];
  if (worst_excess) memcpy(worst_excess, &v[3], 4);
  return NPA_OK;
}

extern "C" int npa_audit_peek(const npa_handle* h, uint64_t* violations) {
  if (!h || !violations) return fail(NPA_E_ARG, "npa_audit_peek: null argument");
  *violations = h->audit_host ? (uint64_t)*(volatile unsigned*)h->audit_host : 0;
  return NPA_OK;
}

extern "C" int npa_selftest_flags(const npa_handle* h, int* flags) {
  if (!h || !flags) return fail(NPA_E_ARG, "npa_selftest_flags: null argument");
  *flags = h->selftest_flags;
  return NPA_OK;
}

extern "C" int npa_use_network_keys(npa_handle* h) {
  if (!h) return fail(NPA_E_ARG, "npa_use_network_keys: null handle");
  std::lock_guard<std::mutex> lock(h->mu);
  if (h->pc.active) return fail(NPA_E_ARG, "npa_use_network_keys: a forward call is in progress on this handle");
  if (h->key_terms != 4) return NPA_OK;
  int cur = -1;
  HIP_TRY(hipGetDevice(&cur));
  if (cur != h->device) HIP_TRY(hipSetDevice(h->device));
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = calibrate_network_keys(h, -1);
  if (e == hipSuccess) e = audit_block_reset(h);
  // (the reduced-precision tiers belong to the geometric selection: a handle on network keys emits exact fp32 rows, and says so)
  if (e == hipSuccess) { h->rows_bf16 = false; h->keys_bf16 = false; }
  if (cur != h->device) (void)hipSetDevice(cur);
  HIP_TRY(e);
  h->stats_mark = 0; h->tiles_window = 0; h->calls_window = 0; h->hold = 0;
  return NPA_OK;
}

extern "C" int npa_set_adjust(npa_handle* h, const float q_s[3], float p_u, float eta, float d_max, float d_min) {
  if (!h || !q_s) return fail(NPA_E_ARG, "npa_set_adjust: null argument");
  for (int k = 0; k < 3; ++k) h->P.q_s[k] = q_s[k];
  h->P.p_u = p_u; h->P.eta = eta; h->P.d_max = d_max; h->P.d_min = d_min;
  return NPA_OK;
}

extern "C" int npa_set_adjust_batch(npa_handle* h, const float* theta, int batch) {
  if (!h) return fail(NPA_E_ARG, "npa_set_adjust_batch: null handle");
  if (theta && batch < 1) return fail(NPA_E_ARG, "npa_set_adjust_batch: batch < 1");
  std::lock_guard<std::mutex> lock(h->mu);
  h->theta = theta;
  h->theta_batch = theta ? batch : 0;
  return NPA_OK;
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
  return npa_scratch_layout(batch, h->P.T, mdim(h->P), h->P.E, kstride(h)).total * sizeof(float);
}
extern "C" size_t npa_workspace_qp_info_offset(const npa_handle* h, int batch) {
  if (!h || batch < 1) return 0;
  return npa_scratch_layout(batch, h->P.T, mdim(h->P), h->P.E, kstride(h)).qp_info * sizeof(float);
}
extern "C" int npa_workspace_layout(const npa_handle* h, int batch, size_t* out, int n) {
  if (!h || batch < 1 || !out || n < 1) return fail(NPA_E_ARG, "npa_workspace_layout: bad argument");
  const ScratchLayout L = npa_scratch_layout(batch, h->P.T, mdim(h->P), h->P.E, kstride(h));
  const size_t v[8] = {L.cur_s * 4, L.cur_u * 4, L.cur_d * 4, L.mu * 4, L.lam * 4, L.pts * 4, L.dist * 4, L.count * 4};
  for (int i = 0; i < n && i < 8; ++i) out[i] = v[i];
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
  h->n_dune = h->n_sel = h->n_qp = h->n_aset = 0;
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
  HIP_TRY(avg(h->ev_aset, h->n_aset, &h->last_aset_ms));
  h->last_aset_n = (long long)h->n_aset;
  if (launches) *launches = (int64_t)h->n_qp;
  h->n_dune = h->n_sel = h->n_qp = h->n_aset = 0;
  return NPA_OK;
}

extern "C" int npa_profile_read_aset(npa_handle* h, double* aset_ms_avg, int64_t* launches) {
  if (!h) return fail(NPA_E_ARG, "null handle");
  if (aset_ms_avg) *aset_ms_avg = h->last_aset_ms;
  if (launches) *launches = (int64_t)h->last_aset_n;
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
  if (!geo)
    HIP_TRY(npa_launch_encode(h->P, h->wpack, batch, 0, 0, n_stride, nom_s, points, velocities, n_points, nullptr,
                              (unsigned*)h->stage_cand, trig, h->n_cu, 5, h->key_terms, (hipStream_t)stream,
                              nullptr, nullptr));
  if (geo && !h->select_v1)
    HIP_TRY(npa_launch_select_geo(h->P, h->wpack, batch, 0, 0, n_stride, nom_s, points, velocities, n_points, nullptr, trig,
                                  mu_sorted, lam_sorted, pts_sorted, dist_sorted, count, h->sel_stats_dev, h->sel_debug,
                                  h->rows_bf16 ? nullptr : h->audit_dev, h->audit_thresh, h->launch_seq++, h->margin_scale,
                                  h->rows_bf16 ? 1 : (h->keys_bf16 ? 2 : 0), (hipStream_t)stream, nullptr, nullptr));
  else
    HIP_TRY(npa_launch_select(h->P, h->wpack, batch, 0, 0, n_stride, nom_s, points, velocities, n_points, nullptr,
                              (const unsigned*)h->stage_cand, trig, mu_sorted, lam_sorted, pts_sorted, dist_sorted, count,
                              h->key_terms, h->key_e0, h->sel_stats_dev, h->sel_debug, (hipStream_t)stream, nullptr, nullptr));
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
  HIP_TRY(npa_launch_qp(h->P, batch, 0, nom_s, nom_u, ref_s, ref_us, mu_sorted, lam_sorted, pts_sorted, nullptr, count,
                        out_s, out_u, out_d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                        qp_info, nullptr, nullptr, nullptr, nullptr, x64, (hipStream_t)stream, nullptr, nullptr, 0, h->theta));
  return NPA_OK;
}

extern "C" int npa_nrmp_params(npa_handle* h, int batch, const float* nom_s, const float* nom_u, const float* mu_sorted,
                               const float* lam_sorted, const float* pts_sorted, const int32_t* count, float* out_abc,
                               float* out_f, void* stream) {
  if (!h || batch < 1 || !nom_s || !nom_u || !out_abc) return fail(NPA_E_ARG, "npa_nrmp_params: bad argument");
  if (h->P.M > 0 && (!mu_sorted || !lam_sorted || !pts_sorted || !count || !out_f))
    return fail(NPA_E_ARG, "npa_nrmp_params: obstacle arrays required when nrmp_max_num > 0");
  // (the reference trajectory only enters the cost: the nominal arrays stand in for it, the kernel returns before the solve)
  HIP_TRY(npa_launch_qp(h->P, batch, 0, nom_s, nom_u, nom_s, nom_u, mu_sorted, lam_sorted, pts_sorted, nullptr, count,
                        nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                        nullptr, nullptr, nullptr, out_abc, h->P.M > 0 ? out_f : nullptr, nullptr, (hipStream_t)stream, nullptr, nullptr, 0,
                        nullptr));         // (the linearisation and the hinge rows do not depend on the adjust parameters)
  return NPA_OK;
}

extern "C" hipError_t npa_launch_qp_backward(const DevParams& P, int batch, const float* nom_s, const float* nom_u,
                                             const float* ref_s, const float* ref_us, const float* mu_sorted,
                                             const float* lam_sorted, const float* pts_sorted, const int* count,
                                             float* out_s, float* out_u, float* out_d, const float* grad_s,
                                             const float* grad_u, const float* grad_d, float* grad_theta,
                                             float* grad_nom_s, double* qp_info, hipStream_t stream, const float* theta);
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
  HIP_TRY(npa_launch_qp_backward(h->P, batch, nom_s, nom_u, ref_s, ref_us, mu_sorted, lam_sorted, pts_sorted, count,
                                 out_s, out_u, out_d, grad_s, grad_u, grad_d, grad_theta, grad_nom_s, qp_info, (hipStream_t)stream, h->theta));
  return NPA_OK;
}

// staging of one forward call: working copy of the nominal trajectory, cleared flags / counts / state
__global__ void stage_kernel(float* __restrict__ cur_s, const float* __restrict__ nom_s, size_t ns,
                             float* __restrict__ cur_u, const float* __restrict__ nom_u, size_t nu,
                             int* __restrict__ flags, size_t nflag, int* __restrict__ count, size_t ncount,
                             int* __restrict__ state, size_t nstate, float* __restrict__ trig, int T) {
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
    if (!any) break;
  }
}

// stage_kernel for a group of forward calls of one size (merged launches, pan_common.h): blockIdx.y = the call
__global__ void stage_group_kernel(StageGroup G, size_t ns, size_t nu, size_t nflag, size_t ncount, size_t nstate, int T) {
  const StageCall& q = G.c[blockIdx.y];
  float* __restrict__ cur_s = q.cur_s; const float* __restrict__ nom_s = q.nom_s; float* __restrict__ cur_u = q.cur_u;
  const float* __restrict__ nom_u = q.nom_u; int* __restrict__ flags = q.flags; int* __restrict__ count = q.count;
  int* __restrict__ state = q.state; float* __restrict__ trig = q.trig;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;; i += stride) {
    bool any = false;
    if (i < ns) { cur_s[i] = nom_s[i]; any = true; }
    if (i < ncount) {
      const size_t b = i / (size_t)(T + 1), t = i - b * (size_t)(T + 1);
      float c, sn;
      npa_trig(nom_s[b * 3 * (size_t)(T + 1) + 2 * (size_t)(T + 1) + t], c, sn);
      trig[2 * i] = c; trig[2 * i + 1] = sn;
    }
    if (i < nu) { cur_u[i] = nom_u[i]; any = true; }
    if (i < nflag) { flags[i] = 0; any = true; }
    if (i < ncount) { count[i] = 0; any = true; }
    if (i < nstate) { state[i] = 0; any = true; }
    if (!any) break;
  }
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
  if (!h->key_auto) return;
  const DevParams& P = h->P;
  const unsigned now = *(volatile unsigned*)h->sel_stats_host;
  if (h->key_terms == 3) {
    if (--h->hold > 0) return;
    h->key_terms = 1; h->key_err = h->err_mode[0]; h->key_e0 = h->e0_mode[0];
    h->stats_mark = now; h->tiles_window = 0; h->calls_window = 0;
  } else if (h->calls_window >= 8) {
    const unsigned redone = now - h->stats_mark;
    if ((unsigned long long)redone * 12ull > h->tiles_window) {
      h->key_terms = 3; h->key_err = h->err_mode[1]; h->key_e0 = h->e0_mode[1]; h->hold = 256;
      return;
    }
    h->stats_mark = now; h->tiles_window = 0; h->calls_window = 0;
  }
  const int n_use = n_stride < P.dune_max_num ? n_stride : P.dune_max_num;
  h->tiles_window += (unsigned long long)batch * ((n_use + 31) / 32) * ((P.T + 1) + (size_t)(P.K - 1) * P.T);
  ++h->calls_window;
}

// launch_stage = false: everything of npa_forward_begin except the staging launch (the merged group path stages all its
// calls with one launch, npa_group_stage_merged below)
static int forward_begin_impl(npa_handle* h, int batch, int n_stride, const float* nom_s, const float* nom_u,
                              const float* ref_s, const float* ref_us, const float* points,
                              const float* velocities, const int32_t* n_points, float* out_s, float* out_u,
                              float* out_d, float* out_min_distance, int32_t* out_iters, float* out_nrmp_points,
                              void* workspace, size_t workspace_bytes, void* state, size_t state_bytes,
                              void* stream_, int flags, bool launch_stage) {
  if (!h || batch < 1 || !nom_s || !nom_u || !ref_s || !ref_us || !out_s || !out_u || !workspace || !state)
    return fail(NPA_E_ARG, "npa_forward_begin: null argument");
  const DevParams& P = h->P;
  if (P.M > 0 && !out_d) return fail(NPA_E_ARG, "npa_forward_begin: out_d required when nrmp_max_num > 0");
  if (workspace_bytes < npa_workspace_bytes(h, batch)) return fail(NPA_E_ARG, "workspace too small");
  if (state_bytes < npa_state_bytes(h, batch)) return fail(NPA_E_ARG, "state buffer too small");
  if (points && n_stride < 1) return fail(NPA_E_ARG, "n_stride < 1");
  if (points && (n_stride < P.dune_max_num ? n_stride : P.dune_max_num) > P.key_stride)
    return fail(NPA_E_UNSUPPORTED, "more than 32768 points per scene after decimation");
  std::lock_guard<std::mutex> lock(h->mu);
  PendingCall* pc = &h->pc;
  if (pc->active) return fail(NPA_E_ARG, "npa_forward_begin: previous forward on this handle not ended");
  if (int rc = check_theta_batch(h, batch, "npa_forward_begin")) return rc;
  hipStream_t stream = (hipStream_t)stream_;
  const int T = P.T;
  const bool reset_state = (flags & NPA_FWD_RESET_STATE) != 0;
  const ScratchLayout L = npa_scratch_layout(batch, T, mdim(P), P.E, kstride(h));
  float* ws = (float*)workspace;
  pc->batch = batch; pc->n_stride = n_stride; pc->ref_s = ref_s; pc->ref_us = ref_us; pc->points = points;
  pc->velocities = velocities; pc->n_points = n_points; pc->out_s = out_s; pc->out_u = out_u; pc->out_d = out_d;
  pc->out_md = out_min_distance; pc->out_iters = out_iters; pc->out_np = out_nrmp_points; pc->ws = ws;
  pc->state = (float*)state; pc->stream = stream;
  pc->dune = P.M > 0 && points != nullptr;
  pc->nom_s = nom_s; pc->nom_u = nom_u; pc->reset_state = reset_state;
  pc->theta = h->theta;
  if (pc->dune) key_policy(h, batch, n_stride);
  if (launch_stage) {
    // one launch instead of two copies and up to three memsets (each costs tens of microseconds of stream time)
    const size_t ns = (size_t)batch * 3 * (T + 1), nu2 = (size_t)batch * 2 * T;
    const size_t nflag = (size_t)batch * 4, ncount = (size_t)batch * (T + 1);
    const size_t nstate = reset_state ? npa_state_bytes(h, batch) / 4 : 0;
    const size_t work = std::max(std::max(ns, nu2), std::max(std::max(nflag, ncount), nstate));
    const int threads = 256;
    const int blocks = (int)std::min<size_t>((work + threads - 1) / threads, 512);
    hipLaunchKernelGGL(stage_kernel, dim3(blocks), dim3(threads), 0, stream, ws + L.cur_s, nom_s, ns, ws + L.cur_u, nom_u, nu2,
                       (int*)(ws + L.flags), nflag, (int*)(ws + L.count), ncount, (int*)state, nstate, ws + L.trig, T);
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
  return forward_begin_impl(h, batch, n_stride, nom_s, nom_u, ref_s, ref_us, points, velocities, n_points, out_s, out_u, out_d,
                            out_min_distance, out_iters, out_nrmp_points, workspace, workspace_bytes, state, state_bytes, stream_,
                            flags, true);
}

// ---- merged launches of a group of forward calls (npa_forward_batch_group, serve_group.hip) --------------------------------
// n calls qualify when one launch per stage can serve them all: one stream, one batch size, byte-identical kernel parameters,
// the default selection (geometric keys; exact or bf16 rows alike) and the register-resident interior-point solve, nothing
// that needs a launch of its own in between.  Everything else keeps the breadth-first call-by-call order.
extern "C" int npa_group_mergeable(int n, const npa_forward_call* calls) {
  if (n < 2 || n > NPA_GROUP_MAX || !calls) return 0;
  static const bool off = getenv("NPA_GROUP_MERGE") != nullptr && atoi(getenv("NPA_GROUP_MERGE")) == 0;
  if (off) return 0;
  const npa_handle* h0 = calls[0].h;
  if (!h0) return 0;
  const DevParams& P = h0->P;
  const bool dune0 = P.M > 0 && calls[0].points != nullptr;
  if (dune0 && !(h0->key_terms == 4 && !h0->select_v1 && !h0->rows_bf16 && npa_select_geo_group_supported(P.E))) return 0;
  if (!npa_qp_group_supported(P.T, P.M) || h0->qp_generic || P.qp_aset || (h0->aset_auto && calls[0].batch <= h0->aset_small_batch) ||
      h0->key_auto)
    return 0;
  if (calls[0].iter_num < 1 || calls[0].iter_num > P.K) return 0;       // (the call-by-call path reports that)
  for (int c = 0; c < n; ++c) {
    const npa_handle* h = calls[c].h;
    if (!h || calls[c].stream != calls[0].stream || calls[c].batch != calls[0].batch || calls[c].iter_num != calls[0].iter_num ||
        h->device != h0->device || memcmp(&h->P, &P, sizeof(DevParams)) != 0 || h->key_terms != h0->key_terms ||
        h->select_v1 != h0->select_v1 || h->rows_bf16 != h0->rows_bf16 || h->keys_bf16 != h0->keys_bf16 ||
        h->sel_debug != h0->sel_debug || h->audit_thresh != h0->audit_thresh || h->margin_scale != h0->margin_scale ||
        h->qp_generic != h0->qp_generic || h->qp_warm != h0->qp_warm || h->key_auto ||
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
    const npa_forward_call& a = calls[c];
    const int rc = forward_begin_impl(a.h, a.batch, a.n_stride, a.nom_s, a.nom_u, a.ref_s, a.ref_us, a.points, a.velocities,
                                      a.n_points, a.out_s, a.out_u, a.out_d, a.out_min_distance, a.out_iters, a.out_nrmp_points,
                                      a.workspace, a.workspace_bytes, a.state, a.state_bytes, a.stream, flags, false);
    if (rc != NPA_OK) return rc;
    *begun = c + 1;
  }
  GroupLock group_lock(n, calls);
  npa_handle* h0 = calls[0].h;
  const DevParams& P = h0->P;
  const int T = P.T, batch = calls[0].batch;
  const ScratchLayout L = npa_scratch_layout(batch, T, mdim(P), P.E, kstride(h0));
  StageGroup G;
  memset(&G, 0, sizeof(G));
  for (int c = 0; c < n; ++c) {
    const PendingCall& pc = calls[c].h->pc;
    G.c[c] = StageCall{pc.ws + L.cur_s, pc.nom_s, pc.ws + L.cur_u, pc.nom_u, (int*)(pc.ws + L.flags), (int*)(pc.ws + L.count),
                       (int*)pc.state, pc.ws + L.trig};
  }
  const size_t ns = (size_t)batch * 3 * (T + 1), nu2 = (size_t)batch * 2 * T;
  const size_t nflag = (size_t)batch * 4, ncount = (size_t)batch * (T + 1);
  const size_t nstate = h0->pc.reset_state ? npa_state_bytes(h0, batch) / 4 : 0;
  const size_t work = std::max(std::max(ns, nu2), std::max(std::max(nflag, ncount), nstate));
  const int threads = 256;
  const int blocks = (int)std::min<size_t>((work + threads - 1) / threads, 512);
  hipLaunchKernelGGL(stage_group_kernel, dim3(blocks, n), dim3(threads), 0, h0->pc.stream, G, ns, nu2, nflag, ncount, nstate, T);
  HIP_TRY(hipGetLastError());
  return NPA_OK;
}

// (diagnostics, not in the header: merged QP launches issued by this process so far -- the tests check that the merged path ran)
static std::atomic<unsigned long long> g_merged_launches{0};
extern "C" unsigned long long npa_dbg_group_merged_launches(void) { return g_merged_launches.load(); }

// PAN iteration k of every call of the group: one selection launch, one QP launch (profile events: the first call's)
extern "C" int npa_group_iter_merged(int n, const npa_forward_call* calls, int k) {
  GroupLock group_lock(n, calls);
  npa_handle* h0 = calls[0].h;
  const DevParams& P = h0->P;
  if (k < 0 || k >= P.K) return fail(NPA_E_ARG, "npa_forward_batch_group: iteration index out of range");
  const int T = P.T, batch = calls[0].batch;
  const ScratchLayout L = npa_scratch_layout(batch, T, mdim(P), P.E, kstride(h0));
  hipStream_t stream = h0->pc.stream;
  for (int c = 0; c < n; ++c)
    if (!calls[c].h->pc.active) return fail(NPA_E_ARG, "npa_forward_batch_group: a call of the group is not in progress");
  if (h0->pc.dune) {
    SelGeoGroup G;
    memset(&G, 0, sizeof(G));
    int n_stride_max = 1;
    for (int c = 0; c < n; ++c) {
      npa_handle* h = calls[c].h;
      const PendingCall& pc = h->pc;
      float* ws = pc.ws;
      G.c[c] = SelGeoCall{h->wpack, ws + L.cur_s, pc.points, pc.velocities, pc.n_points, (const int*)(ws + L.flags),
                          ws + L.mu, ws + L.lam, ws + L.pts, ws + L.dist, (int*)(ws + L.count), h->sel_stats_dev, ws + L.trig,
                          h->rows_bf16 ? nullptr : h->audit_dev, pc.n_stride, h->launch_seq++};
      if (pc.n_stride > n_stride_max) n_stride_max = pc.n_stride;
    }
    EventPair* evs = next_event(h0, h0->ev_sel, h0->n_sel);
    HIP_TRY(npa_launch_select_geo_group(P, G, n, batch, k == 0 ? 0 : 1, n_stride_max, 0, h0->audit_thresh,
                                        h0->margin_scale, h0->keys_bf16 ? 2 : 0, stream, evs ? evs->a : nullptr,
                                        evs ? evs->b : nullptr));
  }
  QpGroup Q;
  memset(&Q, 0, sizeof(Q));
  for (int c = 0; c < n; ++c) {
    npa_handle* h = calls[c].h;
    const PendingCall& pc = h->pc;
    float* ws = pc.ws;
    float *cur_s = ws + L.cur_s, *cur_u = ws + L.cur_u;
    Q.c[c] = QpCall{cur_s, cur_u, pc.ref_s, pc.ref_us, ws + L.mu, ws + L.lam, ws + L.pts, ws + L.dist, (const int*)(ws + L.count),
                    cur_s, cur_u, ws + L.cur_d, pc.out_s, pc.out_u, pc.out_d, pc.out_md, pc.out_iters, pc.out_np,
                    (int*)(ws + L.flags), pc.state, (double*)(ws + L.qp_info), h->qp_warm ? (double*)(ws + L.warm) : nullptr,
                    pc.dune ? ws + L.trig : nullptr, pc.theta};
  }
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
  const int T = P.T, batch = pc->batch;
  const bool geo = h->key_terms == 4;
  const ScratchLayout L = npa_scratch_layout(batch, T, mdim(P), P.E, kstride(h));
  float* ws = pc->ws;
  float *cur_s = ws + L.cur_s, *cur_u = ws + L.cur_u, *cur_d = ws + L.cur_d;
  float *mu = ws + L.mu, *lam = ws + L.lam, *pts = ws + L.pts, *dist = ws + L.dist;
  int* count = (int*)(ws + L.count);
  int* flags = (int*)(ws + L.flags);
  double* qp_info = (double*)(ws + L.qp_info);
  unsigned* gkeys = (unsigned*)(ws + L.keys);
  hipStream_t stream = pc->stream;
  if (pc->dune) {
    // slice 0 does not depend on the iterate (s(0) is pinned, robot.py:234): after the first iteration of a forward
    // call only slices 1..T are redone
    const int t0 = k == 0 ? 0 : 1;
    if (!geo) {
      EventPair* ev = next_event(h, h->ev_dune, h->n_dune);
      HIP_TRY(npa_launch_encode(P, h->wpack, batch, 0, t0, pc->n_stride, cur_s, pc->points, pc->velocities,
                                pc->n_points, flags, gkeys, ws + L.trig, h->n_cu, 5, h->key_terms, stream,
                                ev ? ev->a : nullptr, ev ? ev->b : nullptr));
    }
    EventPair* evs = next_event(h, h->ev_sel, h->n_sel);
    if (geo && !h->select_v1)
      HIP_TRY(npa_launch_select_geo(P, h->wpack, batch, 0, t0, pc->n_stride, cur_s, pc->points, pc->velocities, pc->n_points,
                                    flags, ws + L.trig, mu, lam, pts, dist, count, h->sel_stats_dev, 0,
                                    h->rows_bf16 ? nullptr : h->audit_dev, h->audit_thresh, h->launch_seq++, h->margin_scale,
                                    h->rows_bf16 ? 1 : (h->keys_bf16 ? 2 : 0), stream, evs ? evs->a : nullptr, evs ? evs->b : nullptr));
    else
      HIP_TRY(npa_launch_select(P, h->wpack, batch, 0, t0, pc->n_stride, cur_s, pc->points, pc->velocities,
                                pc->n_points, flags, gkeys, ws + L.trig, mu, lam, pts, dist, count, h->key_terms, h->key_e0,
                                h->sel_stats_dev, 0, stream, evs ? evs->a : nullptr, evs ? evs->b : nullptr));
  }
  // the active-set launch in front of the interior-point launch (nrmp_qp.hip, top of the kernel): scenes it finishes are skipped
  // by the launch behind it.  Register-resident T = 10 / M = 10 instantiation only; small batches keep the single launch (a
  // launch boundary costs ~10 us of a latency-bound chain: NPA_QP_ASET_MIN_BATCH, default 32)
  const bool aset_forced = P.qp_aset && batch >= h->aset_min_batch;
  const bool aset_small = h->aset_auto && batch <= h->aset_small_batch && k >= h->aset_from_iter;
  if ((aset_forced || aset_small) && h->qp_warm && P.T == 10 && P.M == 10 && !h->qp_generic) {
    EventPair* eva = next_event(h, h->ev_aset, h->n_aset);
    DevParams Pa = P;
    Pa.qp_aset = 1;
    HIP_TRY(npa_launch_qp(Pa, batch, 0, cur_s, cur_u, pc->ref_s, pc->ref_us, mu, lam, pts, dist, count, cur_s, cur_u,
                          cur_d, pc->out_s, pc->out_u, pc->out_d, pc->out_md, pc->out_iters, pc->out_np, flags,
                          pc->state, qp_info, (double*)(ws + L.warm), pc->dune ? ws + L.trig : nullptr,
                          nullptr, nullptr, nullptr, stream, eva ? eva->a : nullptr, eva ? eva->b : nullptr, 1, pc->theta));
  }
  EventPair* ev = next_event(h, h->ev_qp, h->n_qp);
  HIP_TRY(npa_launch_qp(P, batch, 0, cur_s, cur_u, pc->ref_s, pc->ref_us, mu, lam, pts, dist, count, cur_s, cur_u,
                        cur_d, pc->out_s, pc->out_u, pc->out_d, pc->out_md, pc->out_iters, pc->out_np, flags,
                        pc->state, qp_info, h->qp_warm ? (double*)(ws + L.warm) : nullptr, pc->dune ? ws + L.trig : nullptr,
                        nullptr, nullptr, nullptr, stream,
                        ev ? ev->a : nullptr, ev ? ev->b : nullptr, 0, pc->theta));
  if (h->key_auto && pc->dune && k == P.K - 1)
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

// (diagnostics, not in the header: the four words of the selection's statistics since the handle was created; synchronises the device)
extern "C" int npa_dbg_select_stats(npa_handle* h, unsigned out[4]) {
  if (!h || !out || !h->sel_stats_dev) return NPA_E_ARG;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, h->sel_stats_dev, 4 * sizeof(unsigned), hipMemcpyDeviceToHost));
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

extern "C" hipError_t npa_launch_progress(int batch, const double* state, const double* path, const int* curve_off,
                                          const int* curve_len, int* point_index, double close_threshold, int ind_range,
                                          double arrive_threshold, int arrive_index_threshold, float* min_dis,
                                          int* arrived, hipStream_t stream);
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

extern "C" hipError_t npa_launch_labels(int E, const double* G, const double* h, long long n, const double* points,
                                        float* mu, float* dist, hipStream_t stream);
extern "C" int npa_dune_labels(int edge_num, const double* G, const double* h, int64_t n, const double* points,
                               float* mu, float* dist, void* stream) {
  if (!G || !h || n < 0 || (n > 0 && (!points || !mu || !dist))) return fail(NPA_E_ARG, "npa_dune_labels: bad argument");
  if (edge_num < 3 || edge_num > NPA_MAX_E) return fail(NPA_E_UNSUPPORTED, "edge_num outside [3,NPA_MAX_E]");
  HIP_TRY(npa_launch_labels(edge_num, G, h, (long long)n, points, mu, dist, (hipStream_t)stream));
  return NPA_OK;
}

// ---- create-time self-test ----------------------------------------------------------------------------------------
// Two symptoms of this toolchain were caged rather than explained: a packed-fp32 form of the key
// path that produced non-deterministic keys, and register-starved builds of the QP kernel whose warm-start logic ran
// on corrupted loop scalars.  Both would ship WRONG PLANS silently if a different compiler / runtime brought them back
// (the driver's box runs another HIP runtime than the one the library was built with).  So every handle runs its own
// kernels once on a fixed synthetic problem before it is handed out (a few ms):
//   1. the forward call twice: outputs bitwise equal (determinism of every instantiated kernel);
//   2. the same with the QP's warm start off: controls equal to 1e-4, finite, inside the speed bounds;
//   3. geometric keys: the DUNE stage's rows bitwise equal to those of the exact whole-slice path (the audit's
//      distrust mode) -- the nomination leaves no true member out on this cloud;
//   network keys: the DUNE stage twice, bitwise equal.
// A failure returns NPA_E_UNSUPPORTED with the failing check in npa_last_error().  NPA_SKIP_SELFTEST=1 skips it.
static int npa_self_test(npa_handle* h) {
  const DevParams& P = h->P;
  const int B = 2, T = P.T, M = mdim(P), E = P.E, N = 96;
  const bool obs = P.M > 0;
  const int kmax = P.K < 3 ? P.K : 3;
  std::vector<float> nom_s((size_t)B * 3 * (T + 1)), nom_u((size_t)B * 2 * T), ref_s(nom_s.size()), ref_us((size_t)B * T),
      pts((size_t)B * 2 * N);
  float rbody = 2.5f;
  if (h->geo_valid) {
    rbody = 0.f;
    for (int e = 0; e < P.E; ++e) rbody = std::max(rbody, std::sqrt(P.pvx[e] * P.pvx[e] + P.pvy[e] * P.pvy[e]));
  }
  unsigned lcg = 12345u;
  auto rnd = [&]() { lcg = lcg * 1664525u + 1013904223u; return (float)((lcg >> 8) & 0xFFFF) / 65535.0f; };
  for (int b = 0; b < B; ++b) {
    const float th = 0.05f * (float)(b + 1), v = 1.0f + 0.5f * (float)b;
    for (int t = 0; t <= T; ++t) {
      const float d = v * (float)P.dt * (float)t;
      nom_s[(size_t)b * 3 * (T + 1) + t] = d * std::cos(th);
      nom_s[(size_t)b * 3 * (T + 1) + (T + 1) + t] = d * std::sin(th);
      nom_s[(size_t)b * 3 * (T + 1) + 2 * (T + 1) + t] = th;
      ref_s[(size_t)b * 3 * (T + 1) + t] = 1.1f * d;
      ref_s[(size_t)b * 3 * (T + 1) + (T + 1) + t] = 0.f;
      ref_s[(size_t)b * 3 * (T + 1) + 2 * (T + 1) + t] = 0.f;
    }
    for (int t = 0; t < T; ++t) {
      nom_u[(size_t)b * 2 * T + t] = v; nom_u[(size_t)b * 2 * T + T + t] = 0.f;
      ref_us[(size_t)b * T + t] = v;
    }
    // a ring of points around the path's start and a cluster ahead and to the side of it that the horizon approaches, both
    // placed relative to the robot's own size (rbody = its largest vertex radius: the ring starts at least 1.5 m outside the
    // body whatever polygon the handle was created with; 2.5 m stands in when the rows are not a recognisable polygon)
    // (never closer than the cloud the shipped robots were validated on: ring from 4 m, cluster at (5.5, 2.5))
    const float ring0 = std::max(4.0f, rbody + 1.5f), cx = std::max(5.5f, (rbody + 3.0f) * 0.9f), cy = std::max(2.5f, (rbody + 3.0f) * 0.43f);
    for (int n = 0; n < N; ++n) {
      const float ang = 6.2831853f * rnd(), r = ring0 + 5.0f * rnd();
      pts[(size_t)b * 2 * N + n] = (n < 80) ? r * std::cos(ang) : cx + 0.6f * rnd();
      pts[(size_t)b * 2 * N + N + n] = (n < 80) ? r * std::sin(ang) : cy + 0.6f * rnd();
    }
  }
  const size_t wsb = npa_workspace_bytes(h, B), stb = npa_state_bytes(h, B);
  const size_t n_in = nom_s.size() * 2 + nom_u.size() + ref_us.size() + pts.size();
  const size_t n_out = (size_t)B * 3 * (T + 1) + (size_t)B * 2 * T + (size_t)B * T + B + B + (size_t)B * 2 * M;
  const size_t n_stage = (size_t)B * (T + 1) * M * (E + 5) + (size_t)B * (T + 1);
  char* dev = nullptr;
  const size_t bytes = (n_in + 3 * n_out + 2 * n_stage) * 4 + wsb + stb + 1024;
  HIP_TRY(hipMalloc(&dev, bytes));
  struct Free { char* p; ~Free() { if (p) hipFree(p); } } guard{dev};
  HIP_TRY(hipMemset(dev, 0, bytes));
  float* d_nom_s = (float*)dev;
  float* d_ref_s = d_nom_s + nom_s.size();
  float* d_nom_u = d_ref_s + ref_s.size();
  float* d_ref_us = d_nom_u + nom_u.size();
  float* d_pts = d_ref_us + ref_us.size();
  float* d_out[3];
  d_out[0] = d_pts + pts.size(); d_out[1] = d_out[0] + n_out; d_out[2] = d_out[1] + n_out;
  float* d_stage[2];
  d_stage[0] = d_out[2] + n_out; d_stage[1] = d_stage[0] + n_stage;
  char* d_ws = (char*)(((uintptr_t)(d_stage[1] + n_stage) + 255) & ~(uintptr_t)255);
  char* d_state = (char*)(((uintptr_t)(d_ws + wsb) + 255) & ~(uintptr_t)255);
  HIP_TRY(hipMemcpy(d_nom_s, nom_s.data(), nom_s.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_ref_s, ref_s.data(), ref_s.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_nom_u, nom_u.data(), nom_u.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_ref_us, ref_us.data(), ref_us.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_pts, pts.data(), pts.size() * 4, hipMemcpyHostToDevice));
  auto run = [&](float* o) -> int {
    float* os = o; float* ou = os + (size_t)B * 3 * (T + 1); float* od = ou + (size_t)B * 2 * T;
    float* omd = od + (size_t)B * T; int32_t* oit = (int32_t*)(omd + B); float* onp = (float*)(oit + B);
    int rc = npa_forward_begin(h, B, N, d_nom_s, d_nom_u, d_ref_s, d_ref_us, obs ? d_pts : nullptr, nullptr, nullptr, os, ou, od,
                               omd, oit, onp, d_ws, wsb, d_state, stb, nullptr, NPA_FWD_RESET_STATE);
    for (int k = 0; k < kmax && rc == NPA_OK; ++k) rc = npa_forward_iter(h, k);
    const int rc2 = npa_forward_end(h);
    return rc != NPA_OK ? rc : rc2;
  };
  std::vector<float> o0(n_out), o1(n_out), o2(n_out);
  int rc = run(d_out[0]);
  if (rc == NPA_OK) rc = run(d_out[1]);
  const bool warm_was = h->qp_warm;
  h->qp_warm = false;
  if (rc == NPA_OK) rc = run(d_out[2]);
  h->qp_warm = warm_was;
  if (rc != NPA_OK) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(o0.data(), d_out[0], n_out * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(o1.data(), d_out[1], n_out * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(o2.data(), d_out[2], n_out * 4, hipMemcpyDeviceToHost));
  const size_t n_su = (size_t)B * 3 * (T + 1) + (size_t)B * 2 * T;          // states and controls: compared
  if (memcmp(o0.data(), o1.data(), n_su * 4) != 0)
    return fail(NPA_E_UNSUPPORTED, "npa_create self-test: two runs of the same forward call differ (non-deterministic kernel: "
                                   "this build / runtime combination is not usable; library built with hipcc " NPA_HIPCC_VERSION ")");
  // HARD failures are the two things no valid configuration can produce: a run-to-run difference (above) and a control
  // that is not finite or leaves its box.  Warm against cold is a SOFT check: two converged solves of a QP that is flat
  // along steering directions (car-like robots, tight bounds, a body overlapping the test cluster) may legitimately
  // stop 1e-4 apart, so a disagreement only switches the warm start off for this handle (NPA_SELFTEST_WARM_OFF).
  const float* u0 = o0.data() + (size_t)B * 3 * (T + 1);
  const float* u2 = o2.data() + (size_t)B * 3 * (T + 1);
  float warm_gap = 0.f;
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < 2; ++k)
      for (int t = 0; t < T; ++t) {
        const float a = u0[(size_t)b * 2 * T + k * T + t], c = u2[(size_t)b * 2 * T + k * T + t];
        const double sb = P.speed_bound[k];
        for (const float v : {a, c})
          if (!(v == v) || !(std::fabs(v) < 1e30f) || (std::isfinite(sb) && std::fabs(v) > sb + 1e-4 * (1.0 + sb))) {
            char msg[256];
            snprintf(msg, sizeof(msg), "npa_create self-test: control [%d][%d][%d] = %g (bound %g): the QP kernel misbehaves on this "
                                       "build / runtime (hipcc " NPA_HIPCC_VERSION ")", b, k, t, (double)v, sb);
            return fail(NPA_E_UNSUPPORTED, msg);
          }
        warm_gap = std::max(warm_gap, std::fabs(a - c));
      }
  if (warm_gap > 1e-4f && h->qp_warm) {
    h->qp_warm = false;
    h->selftest_flags |= NPA_SELFTEST_WARM_OFF;
  }
  if (obs) {
    auto stage = [&](float* o) -> int {
      float* mu = o; float* lam = mu + (size_t)B * (T + 1) * M * E; float* pt = lam + (size_t)B * (T + 1) * M * 2;
      float* ds = pt + (size_t)B * (T + 1) * M * 2; int32_t* cn = (int32_t*)(ds + (size_t)B * (T + 1) * M);
      return npa_dune_stage(h, B, N, d_nom_s, d_pts, nullptr, nullptr, mu, lam, pt, ds, cn, nullptr);
    };
    rc = stage(d_stage[0]);
    // (reduced-precision rows: the audit is off -- its bound is about the exact network -- so the two runs are a plain
    // determinism check, like network keys)
    const bool geo2 = h->key_terms == 4 && !h->select_v1 && h->audit_dev && !h->rows_bf16;
    const unsigned one[4] = {0, 0, 1, 0};
    if (rc == NPA_OK && geo2) HIP_TRY(hipMemcpy(h->audit_dev, one, sizeof(one), hipMemcpyHostToDevice));   // distrust: exact keys
    if (rc == NPA_OK) rc = stage(d_stage[1]);
    if (rc != NPA_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    std::vector<float> s0(n_stage), s1(n_stage);
    HIP_TRY(hipMemcpy(s0.data(), d_stage[0], n_stage * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(s1.data(), d_stage[1], n_stage * 4, hipMemcpyDeviceToHost));
    // (rows only, and the number of rows: with NPA_SEL_DEBUG the upper bits of count[] carry candidate statistics, which
    // differ between the two runs by design)
    const size_t n_rows = (size_t)B * (T + 1) * M * (E + 5);
    auto same_rows = [&]() {
      bool eq = memcmp(s0.data(), s1.data(), n_rows * 4) == 0;
      for (size_t i = n_rows; i < n_stage && eq; ++i) {
        int c0, c1;
        memcpy(&c0, &s0[i], 4); memcpy(&c1, &s1[i], 4);
        eq = (c0 & 0xFF) == (c1 & 0xFF);
      }
      return eq;
    };
    bool same = same_rows();
    if (!same && geo2) {
      // the nomination left a true member out on the test cloud: this handle does not use geometric keys.  Network keys
      // (calibrated now) take over, and THEIR determinism is checked like that of any network-key handle.
      HIP_TRY(audit_block_reset(h));
      HIP_TRY(calibrate_network_keys(h, -1));
      h->selftest_flags |= NPA_SELFTEST_GEO_REJECTED;
      rc = stage(d_stage[0]);
      if (rc == NPA_OK) rc = stage(d_stage[1]);
      if (rc != NPA_OK) return rc;
      HIP_TRY(hipDeviceSynchronize());
      HIP_TRY(hipMemcpy(s0.data(), d_stage[0], n_stage * 4, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(s1.data(), d_stage[1], n_stage * 4, hipMemcpyDeviceToHost));
      same = same_rows();
    }
    if (!same)
      return fail(NPA_E_UNSUPPORTED, "npa_create self-test: two runs of the DUNE stage differ (non-deterministic keys: this build / "
                                     "runtime combination is not usable; library built with hipcc " NPA_HIPCC_VERSION ")");
  }
  // leave no trace: counters, sequence numbers, the key policy's window
  HIP_TRY(audit_block_reset(h));
  if (h->sel_stats_dev) HIP_TRY(hipMemset(h->sel_stats_dev, 0, sizeof(unsigned)));
  if (h->sel_stats_host) *h->sel_stats_host = 0;
  h->launch_seq = 0; h->stats_mark = 0; h->tiles_window = 0; h->calls_window = 0; h->hold = 0;
  HIP_TRY(hipDeviceSynchronize());
  return NPA_OK;
}

static void drop_pending(npa_handle* h) { (void)h; }
