// create.hip -- npa_create / npa_destroy: configuration -> DevParams, the shared weight pack and its calibration, the per-handle
// buffers, the create-time self-test; and the introspection / setter exports of what creation leaves in a handle.
// Host-side only.  Shares state with c_api.hip (the forward path) through handle.h alone; what it calls in other units: launch.h.
#include "handle.h"
#include "launch.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

static std::mutex g_pack_mu;                                   // held across a creation's calibration: same-key creates queue up
static std::map<std::string, std::weak_ptr<SharedPack>> g_packs;
static long long g_pack_calibrations = 0, g_pack_hits = 0;     // (npa_pack_cache_stats)

// ---- the environment, read once ---------------------------------------------------------------------------------------------
// The calibration knobs: ONE list gives both the CalibKnobs record the calibration functions see and the knob part of the
// pack's cache key (the raw strings, in this order) -- a knob cannot be read by a calibration without being part of the key.
struct CalibKnobDef { const char* name; void (*parse)(const char* v, CalibKnobs& k); };
static Precision parse_precision(const char* v) {
  return !strcmp(v, "bf16") ? Precision::bf16 : (!strcmp(v, "fp32") ? Precision::fp32 : Precision::invalid);
}
static const CalibKnobDef kCalibKnobs[] = {
    {"NPA_DUNE_FP32KEYS", [](const char*, CalibKnobs& k) { k.forced_mode = 0; }},
    {"NPA_KEY_TERMS", [](const char* v, CalibKnobs& k) { const int t = atoi(v); if (k.forced_mode != 0 && (t == 1 || t == 3 || t == 4)) k.forced_mode = t; }},
    {"NPA_KEY_SAFETY", [](const char* v, CalibKnobs& k) { const double s = atof(v); if (s >= 1.0 && s <= 1e3) k.key_safety = s; }},
    {"NPA_GEO_GRID", [](const char* v, CalibKnobs& k) { const int n = atoi(v); if (n >= 64 && n <= 8192) k.geo_grid = n / 8 * 8; }},
    {"NPA_GEO_NOCHECK", [](const char*, CalibKnobs& k) { k.geo_nocheck = true; }},
    {"NPA_GEO_TABLE", [](const char* v, CalibKnobs& k) { k.geo_table = atoi(v) != 0; }},
    {"NPA_KTAB_SAFETY", [](const char* v, CalibKnobs& k) { const double s = atof(v); if (s >= 1.0 && s <= 100.0) k.ktab_safety = s; }},
    {"NPA_KEYS_PRECISION", [](const char* v, CalibKnobs& k) { k.keys_precision = parse_precision(v); }},
    {"NPA_K16_SAFETY", [](const char* v, CalibKnobs& k) { const double s = atof(v); if (s >= 1.0 && s <= 100.0) k.k16_safety = s; }},
    {"NPA_ROWS_PRECISION", [](const char* v, CalibKnobs& k) { k.rows_precision = parse_precision(v); }},
};

struct Knobs {
  CalibKnobs calib;
  std::string calib_key;           // knob part of the pack's cache key
  // per handle, not part of the key
  bool sel_debug = false, qp_cold = false, qp_generic = false, skip_selftest = false, pack_cache = true;
  bool qp_order = true;            // NPA_QP_ORDER=0: the QP launches hand their scenes out in scene order
  bool sel_first_tile = true;      // NPA_SEL_FIRST_TILE=0: candidate lists of 17-32 go to one 32-point tile, as before
  double audit_rate = 1.0 / 64.0;  // audit tiles: one slice wave in 64 (NPA_AUDIT_RATE in [0, 1]; 0 = candidates only)
  float margin_scale = 1.f;
};

static Knobs read_knobs() {
  Knobs k;
  for (const CalibKnobDef& d : kCalibKnobs) {
    const char* v = getenv(d.name);
    k.calib_key.push_back('|');
    if (v) { k.calib_key.append(v); d.parse(v, k.calib); } else k.calib_key.push_back('\x01');
  }
  k.sel_debug = getenv("NPA_SEL_DEBUG") != nullptr;
  k.qp_cold = getenv("NPA_QP_COLD") != nullptr;
  k.qp_generic = getenv("NPA_QP_GENERIC") != nullptr;
  if (const char* env = getenv("NPA_QP_ORDER")) k.qp_order = atoi(env) != 0;
  if (const char* env = getenv("NPA_SEL_FIRST_TILE")) k.sel_first_tile = atoi(env) != 0;
  k.skip_selftest = getenv("NPA_SKIP_SELFTEST") != nullptr;
  if (const char* env = getenv("NPA_PACK_CACHE")) k.pack_cache = atoi(env) != 0;
  if (const char* env = getenv("NPA_AUDIT_RATE")) { double v = atof(env); if (v >= 0.0 && v <= 1.0) k.audit_rate = v; }
  if (const char* env = getenv("NPA_GEO_MARGIN_SCALE")) { double v = atof(env); if (v > 0.0 && v <= 100.0) k.margin_scale = (float)v; }
  return k;
}

#ifdef NPA_EXPERIMENTS
// the knob of the experiments build, per handle
static void read_experiment_knobs(npa_handle* h) { h->select_v1 = getenv("NPA_SELECT_V1") != nullptr; }
#endif

// ---- calibration ------------------------------------------------------------------------------------------------------------
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
// Every phase works on the uncalibrated DevParams plus the record so far, fills its part of the record and writes its margins
// into the pack on the device; none of them reads the environment.

// device scratch of a calibration phase
template <class T>
struct DevScratch {
  T* p = nullptr;
  hipError_t alloc_zeroed(size_t n) {
    hipError_t e = hipMalloc(&p, n * sizeof(T));
    return e == hipSuccess ? hipMemset(p, 0, n * sizeof(T)) : e;
  }
  ~DevScratch() { if (p) (void)hipFree(p); }
};

static void set_calibrated(DevParams& P, const Calibration& c) { P.geo_rcal = c.geo_rcal; P.geo_far = c.geo_far; P.geo_tab = c.geo_tab; }

// The one place a record reaches a handle: the creating handle (miss) and every later one (hit) alike.
static void use_key_mode(npa_handle* h) { h->key_terms = h->cal.key_terms; h->key_err = h->cal.key_err; h->key_e0 = h->cal.key_e0; }
static void apply_calibration(npa_handle* h, const Calibration& c) {
  h->cal = c;
  set_calibrated(h->P, c);
  use_key_mode(h);
}

static constexpr int kBandsPadded = (NPA_GEO_BANDS + 3) & ~3;
static const float kCalibHalves[3] = {8.f, 32.f, 128.f};

// margin[b] = safety x the largest raw[] over band b and its two neighbours (the seen ones), at least `floor`; a band whose
// neighbourhood no grid point fell into (beyond the corners of the largest square) stays uncalibrated: +inf.  near[b] = that
// largest value (< 0: none)
static void band_margins(const float* raw, const bool* seen, double safety, float floor, float* margin, float* near) {
  for (int bnd = 0; bnd < NPA_GEO_BANDS; ++bnd) {
    float m = -1.f;
    for (int q = std::max(bnd - 1, 0); q <= std::min(bnd + 1, NPA_GEO_BANDS - 1); ++q)
      if (seen[q]) m = std::max(m, raw[q]);
    near[bnd] = m;
    margin[bnd] = (m < 0.f || !(m < 1e30f)) ? INFINITY : std::max((float)(safety * m), floor);
  }
}

// margins of a residual measured per band of the exact distance (table-corrected key, bf16 key): the padded margin block as it
// is uploaded, and the largest residual / margin over the bands up to 8 m
static void residual_margins(const unsigned* bits, double safety, float floor, float (&margin)[kBandsPadded], float& worst_err,
                             float& worst_margin) {
  float raw[NPA_GEO_BANDS], near[NPA_GEO_BANDS];
  bool seen[NPA_GEO_BANDS];
  for (int bnd = 0; bnd < NPA_GEO_BANDS; ++bnd) { memcpy(&raw[bnd], &bits[bnd], 4); seen[bnd] = bits[bnd] != 0u; }
  for (int bnd = 0; bnd < kBandsPadded; ++bnd) margin[bnd] = INFINITY;
  band_margins(raw, seen, safety, floor, margin, near);
  worst_err = 0.f; worst_margin = 0.f;
  for (int bnd = 0; bnd <= npa_geo_band(8.0f) && bnd < NPA_GEO_BANDS; ++bnd)
    if (near[bnd] >= 0.f) { worst_err = std::max(worst_err, near[bnd]); worst_margin = std::max(worst_margin, margin[bnd]); }
}

// Network keys (dune_kernel): measure the key error of the single-product (1) and the split-product (3) mode on a
// 1024 x 1024 grid over the training square and pick the cheapest mode whose margin stays under its cap; neither -> the
// exact fp32 encoder (0).  forced = 1 / 3 pins a mode (NPA_KEY_TERMS), < 0 = automatic.  Also the fallback of a handle
// whose geometric keys were rejected (self-test) or distrusted at run time (npa_use_network_keys).
static hipError_t calibrate_network_keys(const DevParams& P, const float* wpack, const CalibKnobs& k, int forced, Calibration& c) {
  const int modes[2] = {1, 3};
  const float floor_e0[2] = {1e-4f, 2e-5f}, cap_e0[2] = {5e-2f, 1e-3f};
  bool ok[2] = {false, false};
  const double sf = k.key_safety > 0 ? k.key_safety : 5.0;
  DevScratch<unsigned> dmax;
  hipError_t e = hipMalloc(&dmax.p, sizeof(unsigned));
  for (int m = 0; m < 2 && e == hipSuccess; ++m) {
    if (forced > 0 && forced != modes[m]) continue;
    unsigned bits = 0;
    e = hipMemset(dmax.p, 0, sizeof(unsigned));
    if (e == hipSuccess) e = npa_launch_key_calib(P, wpack, modes[m], 1024, 25.0f, dmax.p, nullptr);
    if (e == hipSuccess) e = hipMemcpy(&bits, dmax.p, sizeof(unsigned), hipMemcpyDeviceToHost);
    if (e != hipSuccess) break;
    float err;
    memcpy(&err, &bits, sizeof(err));
    c.err_mode[m] = err;
    c.e0_mode[m] = std::max((float)(sf * err), floor_e0[m]);
    ok[m] = c.e0_mode[m] <= cap_e0[m] || forced == modes[m];
  }
  if (e != hipSuccess) return e;
  const int pick = ok[0] ? 0 : (ok[1] ? 1 : -1);
  c.key_terms = 0; c.key_err = 0.f; c.key_e0 = 0.f;
  if (pick >= 0) { c.key_terms = modes[pick]; c.key_err = c.err_mode[pick]; c.key_e0 = c.e0_mode[pick]; }
  c.key_auto = forced < 0 && ok[0] && ok[1];
  return hipSuccess;
}

// Geometric keys: measure, decide (c.key_terms == 4 on acceptance), upload the margins (WP_GEO).
static hipError_t calibrate_geo_keys(const DevParams& P0, float* wpack, int n_cu, const CalibKnobs& k, Calibration& c) {
  DevParams P = P0;
  set_calibrated(P, c);
  const float* halves = kCalibHalves;
  const int nside = k.geo_grid;
  const int forced = k.forced_mode;
  unsigned bits[2 * NPA_GEO_BANDS], bits2[2 * NPA_GEO_BANDS];
  {
    DevScratch<unsigned> tab, tab2;
    hipError_t e = tab.alloc_zeroed(2 * NPA_GEO_BANDS);
    for (int gI = 0; gI < 3 && e == hipSuccess; ++gI)
      e = npa_launch_geo_calib(P, wpack, nside, halves[gI], gI == 0 ? 0.f : 0.97f * halves[gI - 1], 0.f, tab.p, n_cu, nullptr);
    // the same three grids shifted by half a cell: their nodes are the cell centres of the first pass
    if (e == hipSuccess) e = tab2.alloc_zeroed(2 * NPA_GEO_BANDS);
    for (int gI = 0; gI < 3 && e == hipSuccess; ++gI)
      e = npa_launch_geo_calib(P, wpack, nside, halves[gI], gI == 0 ? 0.f : 0.97f * halves[gI - 1], 0.5f, tab2.p, n_cu, nullptr);
    if (e == hipSuccess) e = hipMemcpy(bits, tab.p, sizeof(bits), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(bits2, tab2.p, sizeof(bits2), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
  }
  const double sf = k.key_safety > 0 ? k.key_safety : 1.5;
  float raw[NPA_GEO_BANDS], mg[NPA_GEO_BANDS], near[NPA_GEO_BANDS];
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
  c.geo_refine = refine; c.geo_slope = slope;
  for (int bnd = 0; bnd < NPA_GEO_BANDS; ++bnd) {
    float f0, f1, c0, c1;
    memcpy(&f0, &bits[bnd], 4); memcpy(&f1, &bits[NPA_GEO_BANDS + bnd], 4);
    memcpy(&c0, &bits2[bnd], 4); memcpy(&c1, &bits2[NPA_GEO_BANDS + bnd], 4);
    seen[bnd] = bits[bnd] != 0u || bits[NPA_GEO_BANDS + bnd] != 0u || bits2[bnd] != 0u;
    raw[bnd] = std::max(f0, c0) + std::max(f1, c1);      // both grids feed the margin
  }
  band_margins(raw, seen, sf, 1e-4f, mg, near);
  float worst_err = 0.f, worst_margin = 0.f;
  for (int bnd = npa_geo_band(0.25f); bnd <= npa_geo_band(8.0f) && bnd < NPA_GEO_BANDS; ++bnd) {
    worst_margin = std::max(worst_margin, mg[bnd]);
    float f0;
    memcpy(&f0, &bits[bnd], 4);
    worst_err = std::max(worst_err, f0);
  }
  c.geo_err = worst_err; c.geo_margin = worst_margin;
  // (1.25, not 1: a centre may legitimately exceed the nodes' prediction by a little where f is curved; the margin
  // carries a factor 1.5 on top of the prediction)
  const bool resolved = refine <= 1.25f || k.geo_nocheck;
  if (!((worst_margin <= 0.15f && resolved) || forced == 4)) return hipSuccess;
  hipError_t e = hipMemcpy(wpack + WP_GEO, mg, sizeof(mg), hipMemcpyHostToDevice);
  c.geo_rcal = halves[2];
  double rmax = 0;
  for (int v = 0; v < P.E; ++v) rmax = std::max(rmax, std::sqrt((double)P.pvx[v] * P.pvx[v] + (double)P.pvy[v] * P.pvy[v]));
  c.geo_far = (float)std::max(1.0, (double)halves[2] - rmax);
  c.key_terms = 4; c.key_err = worst_err; c.key_e0 = worst_margin;
  return e;
}

// The correction table of the geometric key and the margin of the corrected key (pan_common.h, WP_TAB / WP_KTAB): f at
// the nodes of the four squares, then |g + f_table - exact| per band of the exact distance on the calibration grids
// (whose nodes drift through every offset inside a cell).  Margin = NPA_KTAB_SAFETY (default 2) x the largest residual over
// the band and its two neighbours, at least 0.1 mm; every survivor of the filter is audited against it at run time.
// tabh: the table's header in the host image (WP_TABH: centre x, y, half extent of level 0).
static hipError_t calibrate_key_table(const DevParams& P0, float* wpack, int n_cu, const float* tabh, const CalibKnobs& k, Calibration& c) {
  DevParams P = P0;
  set_calibrated(P, c);
  unsigned kb[NPA_GEO_BANDS];
  {
    DevScratch<float> nodes;
    DevScratch<unsigned> tabk;
    hipError_t e = hipMalloc(&nodes.p, (size_t)NPA_TAB_LEVELS * (NPA_TAB_N + 1) * (NPA_TAB_N + 1) * sizeof(float));
    if (e == hipSuccess) e = npa_launch_geo_table(P, wpack, nodes.p, n_cu, nullptr);
    if (e == hipSuccess) e = tabk.alloc_zeroed(NPA_GEO_BANDS);
    // (one calibration square per level of the table, nside^2 nodes each: 8 x 8 samples per cell at the default 4096)
    const float th0 = tabh[2];
    const float khalves[NPA_TAB_LEVELS] = {th0, 4.f * th0, 16.f * th0, 64.f * th0};
    for (int gI = 0; gI < NPA_TAB_LEVELS && e == hipSuccess; ++gI)
      e = npa_launch_ktab_calib(P, wpack, k.geo_grid, khalves[gI], gI == 0 ? 0.f : 0.97f * khalves[gI - 1], tabh[0], tabh[1], tabk.p,
                                n_cu, nullptr);
    if (e == hipSuccess) e = hipMemcpy(kb, tabk.p, sizeof(kb), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
  }
  float mk[kBandsPadded];
  residual_margins(kb, k.ktab_safety, 1e-4f, mk, c.ktab_err, c.ktab_margin);
  const hipError_t e = hipMemcpy(wpack + WP_KTAB, mk, sizeof(mk), hipMemcpyHostToDevice);
  if (e == hipSuccess) c.geo_tab = 1;
  return e;
}

// The bf16 tier of the keys: margin per band of the exact distance = NPA_K16_SAFETY (default 2: rounding noise sampled on 3 M
// grid nodes, and every survivor is audited at run time) x the largest |bf16 - exact| over the band and its two neighbours
static hipError_t calibrate_bf16_keys(const DevParams& P0, float* wpack, int n_cu, const CalibKnobs& k, Calibration& c) {
  DevParams P = P0;
  set_calibrated(P, c);
  const float* halves = kCalibHalves;
  unsigned bits[NPA_GEO_BANDS];
  {
    DevScratch<unsigned> tab;
    hipError_t e = tab.alloc_zeroed(NPA_GEO_BANDS);
    for (int gI = 0; gI < 3 && e == hipSuccess; ++gI)
      e = npa_launch_k16_calib(P, wpack, 1024, halves[gI], gI == 0 ? 0.f : 0.97f * halves[gI - 1], tab.p, n_cu, nullptr);
    if (e == hipSuccess) e = hipMemcpy(bits, tab.p, sizeof(bits), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
  }
  float mg[kBandsPadded];
  residual_margins(bits, k.k16_safety, 1e-5f, mg, c.k16_err, c.k16_margin);
  const hipError_t e = hipMemcpy(wpack + WP_K16, mg, sizeof(mg), hipMemcpyHostToDevice);
  c.keys_bf16 = true;
  return e;
}

// the key mode of a fresh pack: geometric keys (and their table) when the polygon and the checkpoint allow, else network keys
static hipError_t calibrate_key_mode(const DevParams& P, float* wpack, int n_cu, bool geo_valid, const float* tabh, const CalibKnobs& k,
                                     Calibration& c) {
  const int forced = k.forced_mode;
  hipError_t e = hipSuccess;
  if (geo_valid && (forced < 0 || forced == 4)) {
    e = calibrate_geo_keys(P, wpack, n_cu, k, c);
    if (e == hipSuccess && c.key_terms == 4 && (P.E == 4 || P.E == 8) && k.geo_table) e = calibrate_key_table(P, wpack, n_cu, tabh, k, c);
  }
  if (e == hipSuccess && c.key_terms != 4 && forced != 0 && forced != 4) e = calibrate_network_keys(P, wpack, k, forced, c);
  return e;
}

// the reduced-precision tiers belong to the default geometric selection of a 4- or 8-edge polygon
static int check_precision_tiers(npa_handle* h, const CalibKnobs& k, int key_terms) {
  const bool geo48 = key_terms == 4 && !h->select_v1 && (h->P.E == 4 || h->P.E == 8);
  if (k.rows_precision == Precision::invalid) return fail(NPA_E_ARG, "NPA_ROWS_PRECISION must be fp32 or bf16");
  if (k.rows_precision == Precision::bf16) {
    if (!geo48) return fail(NPA_E_UNSUPPORTED, "NPA_ROWS_PRECISION=bf16 needs geometric keys (select_geo_kernel) and a polygon of 4 or 8 edges");
    h->rows_bf16 = true;
  }
  if (k.keys_precision == Precision::invalid) return fail(NPA_E_ARG, "NPA_KEYS_PRECISION must be fp32 or bf16");
  if (k.keys_precision == Precision::bf16 && !(geo48 && !h->rows_bf16))
    return fail(NPA_E_UNSUPPORTED, "NPA_KEYS_PRECISION=bf16 needs geometric keys, exact rows and a polygon of 4 or 8 edges");
  return NPA_OK;
}

static int hip_status(hipError_t e) { return e == hipSuccess ? NPA_OK : fail(NPA_E_HIP, std::string("npa_create: ") + hipGetErrorString(e)); }

// The handle's pack: the one a handle of the same key made, or a fresh one, uploaded and calibrated here.  g_pack_mu is held
// from the lookup to the insertion, so creates of one key queue up behind the one that calibrates.
static int acquire_pack(npa_handle* h, const std::vector<float>& image, bool need_w, const Knobs& knobs) {
  const DevParams& P = h->P;
  const CalibKnobs& ck = knobs.calib;
  // the pack's identity: host image + polygon + device + calibration knobs
  std::string key(reinterpret_cast<const char*>(image.data()), image.size() * sizeof(float));
  key.append(reinterpret_cast<const char*>(&P.E), sizeof(P.E));
  key.append(reinterpret_cast<const char*>(P.G), sizeof(P.G));
  key.append(reinterpret_cast<const char*>(P.h), sizeof(P.h));
  key.append(reinterpret_cast<const char*>(&h->device), sizeof(h->device));
  key.push_back(need_w ? 'w' : '-');
  key.append(knobs.calib_key);
  std::lock_guard<std::mutex> lock(g_pack_mu);
  if (knobs.pack_cache) {
    auto it = g_packs.find(key);
    if (it != g_packs.end()) {
      h->pack = it->second.lock();
      if (!h->pack) g_packs.erase(it);
    }
  }
  const bool hit = (bool)h->pack;
  if (!hit) {
    h->pack = std::make_shared<SharedPack>();
    h->pack->device = h->device;
    hipError_t e = hipMalloc(&h->pack->wpack, ((size_t)WP_TAB + WP_TAB_FLOATS) * sizeof(float));      // (the pack, then the key table)
    if (e == hipSuccess) e = hipMemcpy(h->pack->wpack, image.data(), WP_TOTAL * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_status(e);
  }
  SharedPack& S = *h->pack;
  h->wpack = S.wpack;
  if (need_w) {
    // a hit: a handle of the same key measured all of this already -- its record, no launches
    if (hit) ++g_pack_hits;
    else if (int rc = hip_status(calibrate_key_mode(P, S.wpack, h->n_cu, h->geo_valid, &image[WP_TABH], ck, S.cal))) return rc;
    if (int rc = check_precision_tiers(h, ck, S.cal.key_terms)) return rc;
    if (!hit && ck.keys_precision == Precision::bf16)
      if (int rc = hip_status(calibrate_bf16_keys(P, S.wpack, h->n_cu, ck, S.cal))) return rc;
    apply_calibration(h, S.cal);
  }
  if (!hit) {
    // (the device buffer is complete: every write to it happened above)
    if (need_w) ++g_pack_calibrations;
    if (knobs.pack_cache) g_packs[key] = h->pack;
  }
  return NPA_OK;
}

// ---- configuration ----------------------------------------------------------------------------------------------------------
// validates the configuration and fills the DevParams it determines (everything but the calibration's three fields); P arrives
// zero-filled -- npa_group_mergeable compares DevParams bytewise, padding included
static int params_from_config(const npa_config* cfg, const npa_dune_weights* w, DevParams& P, bool& need_w, bool& geo_valid) {
  if (cfg->receding < 1 || cfg->receding > NPA_MAX_T) return fail(NPA_E_UNSUPPORTED, "receding outside [1,NPA_MAX_T]");
  if (cfg->nrmp_max_num < 0 || cfg->nrmp_max_num > NPA_MAX_M) return fail(NPA_E_UNSUPPORTED, "nrmp_max_num outside [0,NPA_MAX_M]");
  if (cfg->edge_num < 3 || cfg->edge_num > NPA_MAX_E) return fail(NPA_E_UNSUPPORTED, "edge_num outside [3,NPA_MAX_E]");
  if (cfg->kinematics < 0 || cfg->kinematics > 2) return fail(NPA_E_ARG, "unknown kinematics");
  if (cfg->iter_num < 1) return fail(NPA_E_ARG, "iter_num < 1");
  if (npa_qp_shmem_bytes(cfg->receding, cfg->nrmp_max_num) > 160 * 1024) return fail(NPA_E_UNSUPPORTED, "T*M too large for LDS");
  need_w = cfg->nrmp_max_num > 0 && cfg->dune_max_num > 0;
  if (need_w && !w) return fail(NPA_E_ARG, "DUNE weights required unless nrmp_max_num == 0 or dune_max_num == 0");
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
  geo_valid = npa_polygon_geometry(P);
  return NPA_OK;
}

// (diagnostics, exported through launch.h: the device-free part of npa_create -- the pack's host image, the DevParams bytes as they
// stand before any calibration, geo_valid and the image's named offsets WP_W1, WP_WL, WP_VEC, WP_W6, WP_B6, WP_BF, WP_WLS,
// WP_WB16, WP_TABH, WP_W116, WP_WL16, WP_VEC16, WP_TOTAL, in floats.  Every output may be null; *params_size = sizeof(DevParams).
// Touches no device.)
extern "C" int npa_dbg_pack_image(const npa_config* cfg, const npa_dune_weights* w, float* image, size_t image_floats, void* params,
                                  size_t params_bytes, size_t* params_size, int* geo_valid, size_t* offsets, int n_offsets) {
  if (!cfg) return fail(NPA_E_ARG, "npa_dbg_pack_image: null configuration");
  const size_t off[13] = {WP_W1, WP_WL, WP_VEC, WP_W6, WP_B6, WP_BF, WP_WLS, WP_WB16, WP_TABH, WP_W116, WP_WL16, WP_VEC16, WP_TOTAL};
  for (int i = 0; offsets && i < n_offsets && i < 13; ++i) offsets[i] = off[i];
  if (params_size) *params_size = sizeof(DevParams);
  DevParams P;
  memset(&P, 0, sizeof(P));
  bool need_w = false, valid = false;
  if (int rc = params_from_config(cfg, w, P, need_w, valid)) return rc;
  if (geo_valid) *geo_valid = valid ? 1 : 0;
  if (params) memcpy(params, &P, std::min(params_bytes, sizeof(P)));
  if (image) {
    std::vector<float> img;
    npa_build_pack_image(P, valid, need_w ? w : nullptr, img);
    memcpy(image, img.data(), std::min(image_floats, img.size()) * sizeof(float));
  }
  return NPA_OK;
}

// ---- creation ---------------------------------------------------------------------------------------------------------------
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

static hipError_t alloc_handle_buffers(npa_handle* h) {
  // word 0: overflow tiles of the selection (key policy); words 1 .. 3 spare
  hipError_t e = hipMalloc(&h->sel_stats_dev, 4 * sizeof(unsigned));
  if (e == hipSuccess) e = hipMemset(h->sel_stats_dev, 0, 4 * sizeof(unsigned));
  if (e == hipSuccess) e = hipHostMalloc(&h->sel_stats_host, sizeof(unsigned), hipHostMallocDefault);
  if (e == hipSuccess) *h->sel_stats_host = 0;
  if (e == hipSuccess) e = hipMalloc(&h->audit_dev, 8 * sizeof(unsigned));       // [4]: launches seen (device side)
  if (e == hipSuccess) e = hipHostMalloc(&h->audit_host, sizeof(unsigned), hipHostMallocMapped);
  if (e == hipSuccess) e = audit_block_reset(h);
  return e;
}

static int npa_self_test(npa_handle* h);

// everything of npa_create behind the validated configuration; a status other than NPA_OK leaves the handle for the caller to destroy
static int create_handle(npa_handle* h, bool need_w, const npa_dune_weights* w) {
  std::vector<float> image;
  npa_build_pack_image(h->P, h->geo_valid, need_w ? w : nullptr, image);
  const Knobs knobs = read_knobs();
  h->knobs = knobs.calib;
  h->sel_debug = knobs.sel_debug; h->qp_warm = !knobs.qp_cold; h->qp_generic = knobs.qp_generic;
  h->qp_order = knobs.qp_order;
#ifdef NPA_EXPERIMENTS
  read_experiment_knobs(h);
#endif
  if (int rc = hip_status(hipGetDevice(&h->device))) return rc;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) h->n_cu = prop.multiProcessorCount;
  if (int rc = acquire_pack(h, image, need_w, knobs)) return rc;
  // (per handle, not part of the calibration record: handles of one pack may differ in it; merged launches compare DevParams)
  if (h->P.geo_tab && knobs.sel_first_tile) h->P.geo_tab |= NPA_GEO_TAB_FIRST_TILE;
  if (need_w) {
    if (int rc = hip_status(alloc_handle_buffers(h))) return rc;
    h->audit_thresh = knobs.audit_rate >= 1.0 ? 0xFFFFFFFFu : (unsigned)(knobs.audit_rate * 4294967296.0);
    h->margin_scale = knobs.margin_scale;
  }
  return knobs.skip_selftest ? NPA_OK : npa_self_test(h);
}

// validate -> geometry -> image -> knobs -> the pack (calibrated on a miss) -> per-handle buffers -> self-test
extern "C" int npa_create(const npa_config* cfg, const npa_dune_weights* w, npa_handle** out) {
  if (!cfg || !out) return fail(NPA_E_ARG, "npa_create: null argument");
  DevParams P;
  memset(&P, 0, sizeof(P));
  bool need_w = false, geo_valid = false;
  if (int rc = params_from_config(cfg, w, P, need_w, geo_valid)) return rc;
  npa_handle* h = new npa_handle();
  memcpy(&h->P, &P, sizeof(P));
  h->geo_valid = geo_valid;
  const int rc = create_handle(h, need_w, w);
  if (rc != NPA_OK) {
    const std::string msg = g_err;
    npa_destroy(h);                                      // releases whatever was created so far (the pack lock is no longer held)
    return fail(rc, msg);
  }
  *out = h;
  return NPA_OK;
}

extern "C" int npa_destroy(npa_handle* h) {
  if (!h) return NPA_OK;
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

// ---- introspection and setters ------------------------------------------------------------------------------------------------
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
  const Calibration& c = h->cal;
  const float v[10] = {h->geo_valid ? 1.f : 0.f, c.geo_err, c.geo_margin, c.geo_refine, c.geo_slope, h->P.geo_far,
                       c.keys_bf16 ? c.k16_err : 0.f, c.keys_bf16 ? c.k16_margin : 0.f,
                       h->P.geo_tab ? c.ktab_err : 0.f, h->P.geo_tab ? c.ktab_margin : 0.f};
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

// this handle leaves the geometric keys: the network keys are measured into ITS copy of the record (the pack and the other
// handles keep theirs) and become its key mode
static hipError_t switch_to_network_keys(npa_handle* h) {
  const hipError_t e = calibrate_network_keys(h->P, h->wpack, h->knobs, -1, h->cal);
  if (e == hipSuccess) use_key_mode(h);
  return e;
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
  if (e == hipSuccess) e = switch_to_network_keys(h);
  if (e == hipSuccess) e = audit_block_reset(h);
  // (the reduced-precision tiers belong to the geometric selection: a handle on network keys emits exact fp32 rows, and says so)
  if (e == hipSuccess) { h->rows_bf16 = false; h->cal.keys_bf16 = false; }
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
      HIP_TRY(switch_to_network_keys(h));
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
