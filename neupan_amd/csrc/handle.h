// handle.h -- the state create.hip (creation, calibration, self-test, introspection) and c_api.hip (the forward path) share:
// the handle, the pack its handles share, the calibration record, the error plumbing.  Host side only.
#pragma once
#include "../../include/neupan_amd.h"
#include "pan_common.h"

#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

inline thread_local std::string g_err;
inline int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return fail(NPA_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

#ifndef NPA_HIPCC_VERSION
#define NPA_HIPCC_VERSION "unknown"
#endif

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
  int qp_seq = 0;                    // QP launches of this call so far: the row of class counters the next one writes (pan_common.h)
  const float* theta = nullptr;      // the handle's per-scene parameter block as it was when the call began (npa_set_adjust_batch)
};

// The calibration knobs of the environment, read once at the top of npa_create (create.hip: read_knobs).  The calibration
// functions take this record and never read the environment; the pack's cache key is made from the same list of variables.
enum class Precision { fp32, bf16, invalid };
struct CalibKnobs {
  int forced_mode = -1;          // NPA_DUNE_FP32KEYS (0), NPA_KEY_TERMS = 1 | 3 | 4; < 0: automatic
  double key_safety = -1.0;      // NPA_KEY_SAFETY in [1, 1e3]; < 0: each key kind's default
  int geo_grid = 4096;           // NPA_GEO_GRID (tests): nodes per side of the calibration grids, a multiple of 8 in [64, 8192]
  bool geo_nocheck = false;      // NPA_GEO_NOCHECK: accept geometric keys whose grid-refinement check fails
  bool geo_table = true;         // NPA_GEO_TABLE=0 switches the table-corrected key off
  double ktab_safety = 2.0, k16_safety = 2.0;                                   // NPA_KTAB_SAFETY, NPA_K16_SAFETY in [1, 100]
  Precision keys_precision = Precision::fp32, rows_precision = Precision::fp32; // NPA_KEYS_PRECISION, NPA_ROWS_PRECISION
};

// Everything the calibration of one pack leaves behind.  Measured once per pack (under g_pack_mu), stored in the pack, and
// applied to every handle of the pack by ONE function (create.hip: apply_calibration) -- the handle that calibrated included.
struct Calibration {
  // distance keys: 1 = single fp16 products, 3 = fp16x2 split products, 0 = the exact fp32 encoder, 4 = geometric keys computed
  // by the selection itself (no key launch).  key_e0: the candidate margin, a multiple of the measured key_err
  int key_terms = 0;
  float key_err = 0.f, key_e0 = 0.f;
  // key_auto: both reduced-precision network modes are calibrated and a handle switches between them by what the single-product
  // keys cost in select_kernel (c_api.hip: key_policy).  [0] single, [1] split
  bool key_auto = false;
  float e0_mode[2] = {0.f, 0.f}, err_mode[2] = {0.f, 0.f};
  // geometric keys: largest |network - geometric distance| / margin over the bands g in [0.25, 8] m.  geo_refine: largest ratio,
  // over the bands, of |f| seen at the CELL CENTRES of a calibration grid to what its nodes predicted for the space between
  // them (node maximum + neighbour difference); <= 1 when the grid resolves f.  geo_slope: largest neighbour difference /
  // spacing on the finest grid (a Lipschitz estimate of f next to the robot, m per m).  geo_rcal / geo_far / geo_tab: DevParams
  float geo_err = 0.f, geo_margin = 0.f, geo_refine = 0.f, geo_slope = 0.f, geo_rcal = 0.f, geo_far = 0.f;
  int geo_tab = 0;
  // the table-corrected geometric key (second-stage filter of long candidate lists): largest measured |g + f_table - exact| /
  // margin over the bands of the exact distance in [0, 8] m
  float ktab_err = 0.f, ktab_margin = 0.f;
  // NPA_KEYS_PRECISION=bf16: the bf16 tier of the KEYS -- a slice whose candidate list overflows runs the list through the
  // bf16-MFMA encoder, keeps what lies within 2 x the measured |bf16 - exact| of the M-th smallest, re-encodes the survivors
  // exactly: the rows are bitwise those of the default path.  Largest measured |bf16 - exact| / margin over g in [0, 8] m
  bool keys_bf16 = false;
  float k16_err = 0.f, k16_margin = 0.f;
};

// ---- one weight pack, one calibration and one key table per (checkpoint, polygon, knobs, device) per PROCESS -----------------
// The reference loads one model per planner (dune.py:131-144); a serving process makes tens of handles of the SAME checkpoint
// (one per batch in flight).  What npa_create derives from the checkpoint -- the repacked weights, the margins of the geometric
// key (6 x geo_calib_kernel), the 8.4 MB key table and its margins (4 x ktab_calib_kernel), the bf16 key margins -- is read-only
// after creation and a pure function of (the host image of the pack, E / G / h, the calibration knobs of the environment, the
// device): handles with the same key SHARE the device buffer and the calibration record.  The cache holds weak references: the
// buffer lives as long as a handle uses it.  Per handle: the audit block, statistics, the self-test and its outcomes, the key
// mode in force (npa_use_network_keys switches ONE handle).  NPA_PACK_CACHE=0 gives every handle a private pack (tests).
struct SharedPack {
  float* wpack = nullptr;
  int device = 0;
  Calibration cal;
  ~SharedPack() {
    if (!wpack) return;
    int cur = -1;
    const bool sw = hipGetDevice(&cur) == hipSuccess && cur != device;
    if (sw) (void)hipSetDevice(device);
    (void)hipFree(wpack);
    if (sw) (void)hipSetDevice(cur);
  }
};

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
  // The pack's calibration record as this handle sees it: a copy, for the introspection calls and the key policy.  A handle
  // that leaves the geometric keys (npa_use_network_keys, a rejected self-test) re-measures the network keys into ITS copy.
  Calibration cal;
  CalibKnobs knobs;                      // the calibration knobs at creation (a later switch to network keys calibrates with them)
  // the key mode in force (Calibration::key_terms / key_err / key_e0; key_policy switches between the two network modes)
  int key_terms = 1;
  float key_e0 = 0.f, key_err = 0.f;
  bool qp_warm = true;                   // interior-point warm start across the PAN iterations of a forward call (NPA_QP_COLD=1: off)
  // NPA_SEL_DEBUG at creation: npa_dune_stage's count[] carries candidate statistics.  ONLY there: inside a forward call count[]
  // is the row count the QP kernel sizes its loops with (a debug word in it once sent the stop test ~200 k rows past its buffer)
  int sel_debug = 0;
  bool geo_valid = false;                // the polygon could be turned into vertices (consecutive CCW edges)
  bool select_v1 = false;                // NPA_SELECT_V1: the first form of the geometric-key selection (select_kernel<E, true>)
  // run-time audit of the margin (select_geo_kernel): [0] audit tiles run, [1] points they checked, [2] bound violations seen
  // (candidates and audit tiles), [3] float bits of the largest excess |exact - g| - margin
  unsigned* audit_dev = nullptr;
  unsigned* audit_host = nullptr;        // pinned, host-mapped mirror of the violation count (words 6, 7 of audit_dev point at it)
  bool rows_bf16 = false;                // NPA_ROWS_PRECISION=bf16: the labelled reduced-precision tier of the rows (geometric keys, E = 4 / 8)
  int selftest_flags = 0;                // NPA_SELFTEST_* : what the create-time self-test changed about this handle
  unsigned audit_thresh = 0;             // fraction of the slice waves that run an audit tile, x 2^32
  unsigned launch_seq = 0;
  float margin_scale = 1.f;              // NPA_GEO_MARGIN_SCALE (tests only: a deliberately wrong margin)
  unsigned* sel_stats_dev = nullptr;     // cumulative overflow tiles (select_kernel)
  unsigned* sel_stats_host = nullptr;    // pinned copy, refreshed behind every forward call
  unsigned stats_mark = 0;
  unsigned long long tiles_window = 0;
  int calls_window = 0, hold = 0;
  // profiling (bench.py): HIP events on the launch stream around every stage launch
  bool prof = false;
  std::vector<EventPair> ev_dune, ev_sel, ev_qp;
  size_t n_dune = 0, n_sel = 0, n_qp = 0;
  bool qp_generic = false;
  bool qp_order = true;                  // the QP launches dispatch their solves longest-first from the lists of the launch before (NPA_QP_ORDER=0: off)
};

inline int mdim(const DevParams& P) { return P.M > 0 ? P.M : 1; }
