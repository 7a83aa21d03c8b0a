// pack_image.hip -- polygon geometry and the host image of the weight pack (declared in launch.h).  No kernel, no HIP runtime call: the
// suffix only keeps the build uniform.
#include "launch.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

// bounding box of the vertices (fp32, as the key table's header and the key pass see it); false: no usable polygon
static bool vertex_bounds(const DevParams& P, bool geo_valid, float& xmin, float& xmax, float& ymin, float& ymax) {
  xmin = 3e38f; xmax = -3e38f; ymin = 3e38f; ymax = -3e38f;
  for (int e = 0; e < P.E && geo_valid; ++e) {
    xmin = std::min(xmin, P.pvx[e]); xmax = std::max(xmax, P.pvx[e]); ymin = std::min(ymin, P.pvy[e]); ymax = std::max(ymax, P.pvy[e]);
  }
  return geo_valid && xmax >= xmin && ymax >= ymin;
}

// vertex e = edges e-1 and e, which holds when the rows are consecutive counter-clockwise edges (util.gen_inequal_from_vertex,
// util/__init__.py:161-206, produces them so).  Any other row order fails the check below and the handle keeps network keys.
bool npa_polygon_geometry(DevParams& P) {
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
  // a polygon that is not an axis-aligned box: its bounding box (grown by 10 um: it must CONTAIN the polygon in fp32) for the
  // key pass
  float xmin, xmax, ymin, ymax;
  if (vertex_bounds(P, ok, xmin, xmax, ymin, ymax) && !P.geo_rect) {
    P.rcx = 0.5f * (xmin + xmax); P.rcy = 0.5f * (ymin + ymax);
    P.rhx = 0.5f * (xmax - xmin) + 1e-5f; P.rhy = 0.5f * (ymax - ymin) + 1e-5f;
  }
  return ok;
}

// 16-bit images inside the float vector (bf16 fragments, fp16 split terms): written through memcpy, element i of the array
// that starts at float offset `at`
static void put16(std::vector<float>& image, int at, size_t i, const void* v) {
  memcpy(reinterpret_cast<unsigned char*>(image.data() + at) + 2 * i, v, 2);
}

void npa_build_pack_image(const DevParams& P, bool geo_valid, const npa_dune_weights* w, std::vector<float>& pack) {
  pack.assign(WP_TOTAL, 0.f);
  for (int i = 0; i < NPA_GEO_BANDS; ++i) pack[WP_GEO + i] = pack[WP_KTAB + i] = INFINITY;
  {
    // header of the key table (pan_common.h, WP_TABH): its squares are centred on the polygon's bounding box
    float xmin, xmax, ymin, ymax;
    const bool okb = vertex_bounds(P, geo_valid, xmin, xmax, ymin, ymax);
    const float h0 = okb ? std::max(NPA_TAB_HALF0, 1.25f * 0.5f * std::max(xmax - xmin, ymax - ymin)) : NPA_TAB_HALF0;
    pack[WP_TABH] = okb ? 0.5f * (xmin + xmax) : 0.f; pack[WP_TABH + 1] = okb ? 0.5f * (ymin + ymax) : 0.f;
    pack[WP_TABH + 2] = h0; pack[WP_TABH + 3] = 0.5f * (float)NPA_TAB_N / h0;
    // a polygon that is not an axis-aligned box: the slack S = the largest distance from a corner of its bounding box (P.rc* /
    // P.rh*, npa_polygon_geometry) to the polygon
    pack[WP_TABH + 4] = 0.f;
    if (okb && !P.geo_rect) {
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
  if (!w) return;
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
  // bf16 A-fragments of the exact network's four 32x32 layers (RNE), for the reduced-precision tier of the rows
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
        for (int q = 0; q < 8; ++q) {
          const uint16_t b = to_bf16(w->lin_w[1 + L][(l & 31) * 32 + npa_feat(8 * s2 + q, l >> 5)]);
          put16(pack, WP_WB16, (((size_t)L * 2 + s2) * 64 + l) * 8 + q, &b);
        }
  // the key path's fp16 split terms of the scaled weights: h1 = RNE(w), h2 = RNE(w - h1)
  for (int L = 0; L < 4; ++L)
    for (int s2 = 0; s2 < 2; ++s2)
      for (int l = 0; l < 64; ++l)
        for (int q = 0; q < 8; ++q) {
          const float wv = (float)((double)wkey[L][(l & 31) * 32 + npa_feat(8 * s2 + q, l >> 5)] * wscale[L]);
          const _Float16 h1 = (_Float16)wv;                       // RNE
          const _Float16 h2 = (_Float16)(wv - (float)h1);
          put16(pack, WP_BF, ((((size_t)L * 2 + 0) * 2 + s2) * 64 + l) * 8 + q, &h1);
          put16(pack, WP_BF, ((((size_t)L * 2 + 1) * 2 + s2) * 64 + l) * 8 + q, &h2);
        }
}
