// curves.h -- way-point curves (include/neupan_amd.h, "way-point curves"): ONE definition in fp64 that the host exports
// (npa_curve_rows, npa_curve_generate) and the device kernels (npa_curve_batch, npa_cycle_retask) both compile.  Every
// arithmetic statement is one rounded operation (contraction is off inside every function here), so two kernels that call
// curve_wave give the same bits; host and device differ only where libm and the device math library do.
// The Dubins words are the normalised closed forms of Shkel and Lumelsky, "Classification of the Dubins set", Robotics and
// Autonomous Systems 34 (2001): start at the origin heading alpha, goal at (d, 0) heading beta, unit turning radius.
// The device inlines the math library at every call, and the product library has a size limit: the plan therefore takes its
// sines and cosines in ONE loop over the five angles it needs and its words in one loop with one atan2, instead of a call
// per formula.
#ifndef NPA_CURVES_H
#define NPA_CURVES_H

#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/neupan_amd.h"

#define NPA_HD __host__ __device__ __forceinline__

namespace npa_curve {

constexpr double kTwoPi = 6.283185307179586;
constexpr double kInvTwoPi = 0.15915494309189535;
constexpr double kMargin = 1e-12;            // how far outside its domain a word's p^2 / acos argument may be and is clamped
constexpr double kMaxSteps = 1073741824.0;   // a curve of 2^30 rows or more is no curve (the row count is an int32)
constexpr int kWave = 64;

// start, goal, the chosen word and the pose (with the heading's sine and cosine) at the start of each of its three segments.
// Scalars only: nothing here is indexed at run time, so the device keeps it in registers.
struct Curve {
  int rows;                        // n + 1; 0: the inputs are outside the specification (no curve)
  int n;
  int style, word;
  double ax, ay, gx, gy, gth;
  double dx, dy, psi;              // the chord and its direction (the heading of a line's rows)
  double rho, total;               // Dubins: the radius and t + p + q
  double t, p, q;
  double k0, k1, k2;               // the segments' turns: +1 left, 0 straight, -1 right
  double x0, y0, h0, s0, c0, x1, y1, h1, s1, c1, x2, y2, h2, s2, c2;
};

NPA_HD double mod2pi(double x) {
#pragma clang fp contract(off)
  double r = x - kTwoPi * floor(x * kInvTwoPi);
  r = r < 0.0 ? r + kTwoPi : r;
  r = r >= kTwoPi ? r - kTwoPi : r;
  return r;
}

// the value of segment `seg` (by value: a conditional between two members would be one between their addresses)
NPA_HD double pick(int seg, double v0, double v1, double v2) { return seg == 0 ? v0 : (seg == 1 ? v1 : v2); }

// `len` (in radii) along a segment of turn k from the pose (x, y, h) with (sh, ch) = (sin h, cos h); (se, ce) = the sine and
// cosine of the heading at the end, e = h + k len
NPA_HD void carry(double x, double y, double sh, double ch, double k, double len, double se, double ce, double rho, double& ox,
                  double& oy) {
#pragma clang fp contract(off)
  const double ux = k == 0.0 ? len * ch : k * (se - sh);
  const double uy = k == 0.0 ? len * sh : -(k * (ce - ch));
  ox = x + rho * ux;
  oy = y + rho * uy;
}

// word w of LSL, LSR, RSL, RSR, RLR, LRL; false: infeasible
NPA_HD bool dubins_word(int w, double al, double be, double d, double sa, double sb, double ca, double cb, double cab, double& t,
                        double& p, double& q) {
#pragma clang fp contract(off)
  // the direction every word has: (y, x) = (+-(ca - cb), d +- (sa - sb)) for LSL / RSR / RLR / LRL, (-+(ca + cb), d +- (sa + sb))
  // for LSR / RSL
  double ya, xa;
  if (w == 0) { ya = cb - ca; xa = d + sa - sb; }
  else if (w == 1) { ya = -ca - cb; xa = d + sa + sb; }
  else if (w == 2) { ya = ca + cb; xa = d - sa - sb; }
  else if (w == 3 || w == 4) { ya = ca - cb; xa = d - sa + sb; }
  else { ya = ca - cb; xa = d + sa - sb; }
  double yy = ya, xx = xa;
  bool ok;
  if (w < 4) {
    double p2;
    if (w == 0) p2 = 2.0 + d * d - 2.0 * cab + 2.0 * d * (sa - sb);
    else if (w == 1) p2 = -2.0 + d * d + 2.0 * cab + 2.0 * d * (sa + sb);
    else if (w == 2) p2 = -2.0 + d * d + 2.0 * cab - 2.0 * d * (sa + sb);
    else p2 = 2.0 + d * d - 2.0 * cab + 2.0 * d * (sb - sa);
    ok = p2 >= -kMargin;
    p = sqrt(p2 < 0.0 ? 0.0 : p2);
    // LSR, RSL: the direction turned back by atan2(-+2, p), as the quotient of the two directions (one atan2)
    const double yb = w == 1 ? -2.0 : 2.0;
    if (w == 1 || w == 2) { yy = ya * p - xa * yb; xx = xa * p + ya * yb; }
  } else {
    const double sgn = w == 4 ? 1.0 : -1.0;
    const double a = (6.0 - d * d + 2.0 * cab + sgn * (2.0 * d * (sa - sb))) / 8.0;
    ok = a >= -1.0 - kMargin && a <= 1.0 + kMargin;
    p = mod2pi(kTwoPi - acos(a < -1.0 ? -1.0 : (a > 1.0 ? 1.0 : a)));
  }
  if (!ok) return false;
  const double u = atan2(yy, xx);
  const double st = (w == 0 || w == 1 || w == 5) ? 1.0 : -1.0;     // the first turn: L +1, R -1
  const double sq = (w == 0 || w == 2) ? 1.0 : -1.0;              // the last turn of a word with a straight
  t = mod2pi(w < 4 ? st * (u - al) : p / 2.0 - u - st * al);
  q = mod2pi(w < 4 ? sq * (be - u) : st * (be - al) - t + p);
  return true;
}

// the curve from start (x, y, theta) to goal (x, y, theta); c.rows == 0 when the inputs are outside the specification
NPA_HD void curve_plan(int style, const double* start, const double* goal, double interval, double rho, Curve& c) {
#pragma clang fp contract(off)
  c.rows = 0; c.n = 0; c.style = style; c.word = -1;
  c.k0 = c.k1 = c.k2 = 0.0;
  c.ax = start[0]; c.ay = start[1]; c.gx = goal[0]; c.gy = goal[1]; c.gth = goal[2];
  c.dx = c.gx - c.ax; c.dy = c.gy - c.ay;
  c.rho = rho; c.total = 0.0; c.t = c.p = c.q = 0.0;
  c.x0 = c.x1 = c.x2 = c.ax; c.y0 = c.y1 = c.y2 = c.ay; c.h0 = c.h1 = c.h2 = start[2];
  c.s0 = c.s1 = c.s2 = 0.0; c.c0 = c.c1 = c.c2 = 1.0;
  const double D = sqrt(c.dx * c.dx + c.dy * c.dy);
  c.psi = atan2(c.dy, c.dx);
  if (!(interval > 0.0)) return;
  double L = D;
  if (style == NPA_CURVE_DUBINS) {
    if (!(rho > 0.0)) return;
    const double d = D / rho;
    const double al = mod2pi(start[2] - c.psi), be = mod2pi(goal[2] - c.psi);
    if (!(D == 0.0 && al == be)) {                            // (the same pose: L = 0; the words would give a full circle)
      // the five angles whose sine and cosine the curve needs, one after the other: alpha, beta (then the words are
      // compared), the start heading, the headings at the start of the second and of the third segment
      double ang = al, sa = 0.0, ca = 1.0;
      bool found = true;
#pragma nounroll
      for (int k = 0; k < 5 && found; ++k) {
        double sn, cs;
        sincos(ang, &sn, &cs);
        if (k == 0) {
          sa = sn; ca = cs; ang = be;
        } else if (k == 1) {
          const double cab = ca * cs + sa * sn;
          double best = 0.0;
#pragma nounroll
          for (int w = 0; w < 6; ++w) {
            double t, p, q;
            if (!dubins_word(w, al, be, d, sa, sn, ca, cs, cab, t, p, q)) continue;
            const double len = t + p + q;
            if (c.word < 0 || len < best) { best = len; c.word = w; c.t = t; c.p = p; c.q = q; }
          }
          const int w = c.word;
          found = w >= 0;
          c.k0 = (w == 0 || w == 1 || w == 5) ? 1.0 : -1.0;
          c.k1 = w < 4 ? 0.0 : (w == 4 ? 1.0 : -1.0);
          c.k2 = (w == 0 || w == 2 || w == 5) ? 1.0 : -1.0;
          c.total = best;
          ang = c.h0;
        } else if (k == 2) {
          c.s0 = sn; c.c0 = cs;
          c.h1 = c.h0 + c.k0 * c.t;
          ang = c.h1;
        } else if (k == 3) {
          c.s1 = sn; c.c1 = cs;
          carry(c.x0, c.y0, c.s0, c.c0, c.k0, c.t, sn, cs, rho, c.x1, c.y1);
          c.h2 = c.h1 + c.k1 * c.p;
          ang = c.h2;
        } else {
          c.s2 = sn; c.c2 = cs;
          carry(c.x1, c.y1, c.s1, c.c1, c.k1, c.p, sn, cs, rho, c.x2, c.y2);
        }
      }
      if (!found) return;
    }
    L = rho * c.total;
  }
  if (!(L >= 0.0 && L <= 1.79769313486231570e308)) return;      // (a NaN or an infinity in the inputs)
  if (L == 0.0) { c.rows = 1; return; }
  const double steps = L / interval - 1e-9;
  if (!(steps < kMaxSteps)) return;
  c.n = steps > 1.0 ? (int)ceil(steps) : 1;
  c.rows = c.n + 1;
}

// row i of the curve, 0 <= i < c.rows: (x, y, theta, gear)
NPA_HD void curve_row(const Curve& c, int i, double* out) {
#pragma clang fp contract(off)
  double x = c.gx, y = c.gy, h = c.gth;
  if (i < c.n) {
    if (c.style == NPA_CURVE_LINE) {
      const double f = (double)i / (double)c.n;
      x = c.ax + f * c.dx;
      y = c.ay + f * c.dy;
      h = c.psi;
    } else {
      const double sig = ((double)i * c.total) / (double)c.n;
      const double tp = c.t + c.p;
      const int seg = sig < c.t ? 0 : (sig < tp ? 1 : 2);
      const double bx = pick(seg, c.x0, c.x1, c.x2), by = pick(seg, c.y0, c.y1, c.y2), bh = pick(seg, c.h0, c.h1, c.h2);
      const double bs = pick(seg, c.s0, c.s1, c.s2), bc = pick(seg, c.c0, c.c1, c.c2);
      const double k = pick(seg, c.k0, c.k1, c.k2);
      const double len = pick(seg, sig, sig - c.t, sig - tp);
      h = bh + k * len;
      double se, ce;
      sincos(h, &se, &ce);
      carry(bx, by, bs, bc, k, len, se, ce, c.rho, x, y);
    }
  } else if (c.style == NPA_CURVE_LINE && c.n > 0) {
    h = c.psi;
  }
  out[0] = x; out[1] = y; out[2] = h; out[3] = 1.0;
}

#ifdef __HIPCC__
// One wave, one curve: every lane plans the same curve (no cross-lane traffic), lane l writes rows l, l + 64, ...  Returns the
// rows the curve needs (0: no curve); nothing is written unless 1 <= needed <= capacity.
__device__ __forceinline__ int curve_wave(int style, const double* start, const double* goal, double interval, double rho,
                                          int capacity, double* rows, int lane) {
  Curve c;
  curve_plan(style, start, goal, interval, rho, c);
  if (c.rows < 1 || c.rows > capacity) return c.rows;
  for (int i = lane; i < c.rows; i += kWave) {
    double r[4];
    curve_row(c, i, r);
    double* o = rows + (size_t)i * 4;
    o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3];
  }
  return c.rows;
}
#endif

}  // namespace npa_curve

#endif  // NPA_CURVES_H
