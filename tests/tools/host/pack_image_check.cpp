// Stand-alone host program around csrc/pack_image.hip (polygon geometry, the weight pack's host image): a box, the 8-edge hull
// and a polygon that is none, with weights from a fixed generator.  Meant to be built with a host sanitizer (README.md here);
// exits 0 when every case gives the expected geo_valid / geo_rect and an image without NaN.
#include "../../../neupan_amd/csrc/launch.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

struct Weights {
  std::vector<float> buf[18];
  npa_dune_weights w;
  explicit Weights(int E) {
    unsigned lcg = 2463534242u;
    auto fill = [&](std::vector<float>& v, size_t n, float scale, float offset) {
      v.resize(n);
      for (float& x : v) { lcg = lcg * 1664525u + 1013904223u; x = offset + scale * ((float)((lcg >> 8) & 0xFFFF) / 32767.5f - 1.0f); }
    };
    const size_t rows[6] = {32, 32, 32, 32, 32, (size_t)E}, cols[6] = {2, 32, 32, 32, 32, 32};
    for (int i = 0; i < 6; ++i) {
      fill(buf[i], rows[i] * cols[i], 0.4f, 0.f); fill(buf[6 + i], rows[i], 0.1f, 0.f);
      w.lin_w[i] = buf[i].data(); w.lin_b[i] = buf[6 + i].data();
    }
    for (int i = 0; i < 3; ++i) {
      fill(buf[12 + i], 32, 0.2f, 1.f); fill(buf[15 + i], 32, 0.1f, 0.f);
      w.ln_w[i] = buf[12 + i].data(); w.ln_b[i] = buf[15 + i].data();
    }
  }
};

// rows G x <= h of the polygon with these vertices, counter-clockwise (edge normal (dy, -dx)), or the same rows reversed
static DevParams polygon(const std::vector<float>& xy, bool reversed) {
  DevParams P;
  memset(&P, 0, sizeof(P));
  const int E = (int)xy.size() / 2;
  P.E = E;
  for (int e = 0; e < E; ++e) {
    const int n = (e + 1) % E, r = reversed ? E - 1 - e : e;
    const float dx = xy[2 * n] - xy[2 * e], dy = xy[2 * n + 1] - xy[2 * e + 1];
    P.G[r][0] = dy; P.G[r][1] = -dx; P.h[r] = dy * xy[2 * e] - dx * xy[2 * e + 1];
  }
  return P;
}

static int check(const char* name, DevParams P, bool with_weights, bool want_valid, int want_rect, bool want_slack) {
  const bool valid = npa_polygon_geometry(P);
  Weights W(P.E);
  std::vector<float> image;
  npa_build_pack_image(P, valid, with_weights ? &W.w : nullptr, image);
  int bad = 0;
  for (float v : image) bad += std::isnan(v) ? 1 : 0;
  const float slack = image[WP_TABH + 4];
  const bool ok = valid == want_valid && P.geo_rect == want_rect && (slack > 0.f) == want_slack && bad == 0 && (int)image.size() == WP_TOTAL;
  printf("%-10s geo_valid %d geo_rect %d slack %.6f h0 %.3f nan %d : %s\n", name, (int)valid, P.geo_rect, slack, image[WP_TABH + 2], bad,
         ok ? "ok" : "UNEXPECTED");
  return ok ? 0 : 1;
}

int main() {
  const std::vector<float> box = {-0.8f, -1.0f, 0.8f, -1.0f, 0.8f, 1.0f, -0.8f, 1.0f};
  const std::vector<float> hull = {-0.6f, -0.8f, 0.6f, -0.8f, 1.0f, -0.4f, 1.0f, 0.4f, 0.6f, 0.8f, -0.6f, 0.8f, -1.0f, 0.4f, -1.0f, -0.4f};
  int rc = 0;
  rc |= check("box", polygon(box, false), true, true, 1, false);
  rc |= check("hull8", polygon(hull, false), true, true, 0, true);
  rc |= check("clockwise", polygon(hull, true), true, false, 0, false);
  rc |= check("no-weights", polygon(box, false), false, true, 1, false);
  return rc;
}
