// Fused DUNE training step (gfx950): forward, the four losses, backward and Adam of the ObsPointNet
// 2 -> 32 -> 32 -> 32 -> 32 -> 32 -> E as ONE persistent workgroup per run, `steps` steps per launch, no host in between.
// include/neupan_amd_train.h is the specification (parameter pack, losses, Adam, the order of every sum); DESIGN.md
// section 3.5 has the mapping and why it is one ROW PER LANE on the vector ALU and not 32-row tiles on the f32 MFMA.
//
// One workgroup = 256 threads = one wave per SIMD; a batch is taken in chunks of 256 rows, thread t = row t of the chunk.
//   - the weights (and the transposes of the four 32 x 32 matrices, for the backward products) sit in LDS and are read
//     as wave-wide broadcasts (ds_read_b128: four weights per read);
//   - a row's saved activations (LayerNorm x-hat, tanh and ReLU outputs: 8 x 32 + E floats) stay in the lane's registers
//     from the forward to the backward pass;
//   - the output of a 32 x 32 product is indexed by the loop counter, so it goes through the lane's own column of an LDS
//     image S[j][row] and comes back with constant indices (no register is indexed dynamically: no scratch);
//   - a weight gradient dW[j][k] = sum_rows dy[row][j] x[row][k] is ONE thread's sum over the rows in ascending order, read
//     from two such images ([32][260] floats: the row stride 260 = 65 slots of 16 B keeps the b128 reads of 8 / 16
//     neighbouring j or k on distinct banks): no partial sums across waves, no atomics, nothing depends on timing;
//   - Adam is one pass of the 256 threads over the P parameters, m and v in global memory (thread t always the same
//     elements), the parameters themselves in LDS until the launch ends.
// __syncthreads() stands only in wave-uniform control flow; every loop's trip count is known at launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <math.h>

#include <string>

#include "../../include/neupan_amd_train.h"

namespace {

constexpr int NT = 256, H = 32, EP = NPA_MAX_E, RS = 260;
// offsets in the pack (neupan_amd_train.h); in LDS the last layer is padded to EP rows (rows >= E are zero), its bias behind
constexpr int O_W0 = 0, O_B0 = 64, O_G0 = 96, O_BE0 = 128, O_W1 = 160, O_B1 = 1184, O_W2 = 1216, O_B2 = 2240, O_G1 = 2272,
              O_BE1 = 2304, O_W3 = 2336, O_B3 = 3360, O_W4 = 3392, O_B4 = 4416, O_G2 = 4448, O_BE2 = 4480, O_W5 = 4512,
              O_B5L = O_W5 + EP * H, PL = O_B5L + EP;

struct TrainArgs {
  int E, batch, steps, train;
  long long n, first_row;
  const float *G, *h, *points, *mu, *dist, *rot;
  float *params, *adam_m, *adam_v, *losses, *grad_out;
  int32_t* step_count;
  double log_beta1, log_beta2, lr;    // of the decimal-rounded values (neupan_amd_train.h); beta^t = exp(t log beta)
  float om_beta1, om_beta2, beta2f, eps, weight_decay;
};

// A kernel argument read where it is used, from the kernarg segment: arguments used once per launch or once per step (the
// state pointers, the Adam constants) would otherwise sit in SGPRs through the whole kernel, which spilled 56 of them.
template <class T>
__device__ __forceinline__ T late(const T& field) { return *const_cast<const volatile T*>(&field); }

__device__ __forceinline__ int lds_index(int i, int E) { return i < O_W5 + H * E ? i : O_B5L + (i - (O_W5 + H * E)); }

// y = W x (+ b): W [NOUT][NIN] row-major in LDS, read as broadcasts; the outputs pass through the lane's own column of S
template <int NIN, int NOUT, bool BIAS>
__device__ __forceinline__ void linear(const float* W, const float* b, const float (&x)[NIN], float (&y)[NOUT], float* S, int tid) {
#pragma unroll 1
  for (int j = 0; j < NOUT; ++j) {
    const float4* w = reinterpret_cast<const float4*>(W + j * NIN);
    float acc = BIAS ? b[j] : 0.f;
#pragma unroll
    for (int q = 0; q < NIN / 4; ++q) {
      const float4 v = w[q];
      acc = fmaf(v.x, x[4 * q], acc);
      acc = fmaf(v.y, x[4 * q + 1], acc);
      acc = fmaf(v.z, x[4 * q + 2], acc);
      acc = fmaf(v.w, x[4 * q + 3], acc);
    }
    S[j * RS + tid] = acc;
  }
#pragma unroll
  for (int j = 0; j < NOUT; ++j) y[j] = S[j * RS + tid];
}

__device__ __forceinline__ void put32(float* S, const float (&v)[H], int tid) {
#pragma unroll
  for (int j = 0; j < H; ++j) S[j * RS + tid] = v[j];
}

// LayerNorm(eps 1e-5) and tanh of one row
__device__ __forceinline__ void ln_tanh(const float* g, const float* be, const float (&z)[H], float (&xh)[H], float (&t)[H], float& rstd) {
  float mean = 0.f;
#pragma unroll
  for (int j = 0; j < H; ++j) mean += z[j];
  mean *= 1.f / H;
  float var = 0.f;
#pragma unroll
  for (int j = 0; j < H; ++j) { const float d = z[j] - mean; var = fmaf(d, d, var); }
  rstd = 1.f / sqrtf(var * (1.f / H) + 1e-5f);
#pragma unroll
  for (int j = 0; j < H; ++j) {
    xh[j] = (z[j] - mean) * rstd;
    t[j] = tanhf(fmaf(xh[j], g[j], be[j]));
  }
}

// dt -> da through tanh, in place (da: the gradient at the LayerNorm's output, also what its weight / bias gradients need)
__device__ __forceinline__ void tanh_bwd(float (&d)[H], const float (&t)[H]) {
#pragma unroll
  for (int j = 0; j < H; ++j) d[j] *= 1.f - t[j] * t[j];
}

// da -> dz through the LayerNorm of one row
__device__ __forceinline__ void ln_bwd(const float* g, const float (&da)[H], const float (&xh)[H], float rstd, float (&dz)[H]) {
  float m1 = 0.f, m2 = 0.f;
#pragma unroll
  for (int j = 0; j < H; ++j) {
    const float dxh = da[j] * g[j];
    m1 += dxh;
    m2 = fmaf(dxh, xh[j], m2);
  }
  m1 *= 1.f / H;
  m2 *= 1.f / H;
#pragma unroll
  for (int j = 0; j < H; ++j) dz[j] = rstd * (da[j] * g[j] - m1 - xh[j] * m2);
}

// dW[j][k] += sum_r A[j][r] B[k][r], db[j] += sum_r A[j][r], r = 0 .. cnt4-1 ascending; thread t owns KPT elements of one j:
// k = m + (NIN / KPT) q, q < KPT (neighbouring lanes neighbouring k: distinct banks)
template <int NOUT, int NIN, int KPT>
__device__ __forceinline__ void dw_pass(const float* A, const float* B, int cnt4, float* gW, float* gb, int tid) {
  constexpr int PER_J = NIN / KPT;
  if (tid >= NOUT * PER_J) return;                 // (whole waves: NOUT * PER_J is 64 or 256)
  const int j = tid / PER_J, m = tid % PER_J;
  float acc[KPT], accb = 0.f;
#pragma unroll
  for (int q = 0; q < KPT; ++q) acc[q] = 0.f;
  const float* pa = A + j * RS;
  const float* pb = B + m * RS;
  for (int r = 0; r < cnt4; r += 4) {
    const float4 a = *reinterpret_cast<const float4*>(pa + r);
    accb += a.x; accb += a.y; accb += a.z; accb += a.w;
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
      const float4 x = *reinterpret_cast<const float4*>(pb + q * PER_J * RS + r);
      acc[q] = fmaf(a.x, x.x, acc[q]);
      acc[q] = fmaf(a.y, x.y, acc[q]);
      acc[q] = fmaf(a.z, x.z, acc[q]);
      acc[q] = fmaf(a.w, x.w, acc[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < KPT; ++q) {
    float* d = gW + j * NIN + m + q * PER_J;
    *d += acc[q];
  }
  if (m == 0) gb[j] += accb;
}

// LayerNorm weight / bias gradient: dg[j] = sum_r A[j][r] B[j][r], dbe[j] = sum_r A[j][r]; 8 threads per j
__device__ __forceinline__ void ln_reduce(const float* A, const float* B, int cnt4, float* gg, float* gbe, int tid) {
  const int j = tid >> 3, q = tid & 7;
  float sg = 0.f, sb = 0.f;
  for (int r = 4 * q; r < cnt4; r += 32) {
    const float4 a = *reinterpret_cast<const float4*>(A + j * RS + r);
    const float4 x = *reinterpret_cast<const float4*>(B + j * RS + r);
    sg = fmaf(a.x, x.x, sg); sg = fmaf(a.y, x.y, sg); sg = fmaf(a.z, x.z, sg); sg = fmaf(a.w, x.w, sg);
    sb += a.x; sb += a.y; sb += a.z; sb += a.w;
  }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) {
    sg += __shfl_xor(sg, o, 64);
    sb += __shfl_xor(sb, o, 64);
  }
  if (q == 0) {
    gg[j] += sg;
    gbe[j] += sb;
  }
}

__global__ __launch_bounds__(NT) void dune_train_kernel(const TrainArgs a) {
  __shared__ __attribute__((aligned(16))) float sW[PL];          // parameters, pack order, last layer padded to EP rows
  __shared__ __attribute__((aligned(16))) float sGr[PL];         // gradient of the step, same layout
  __shared__ __attribute__((aligned(16))) float sWT[4 * H * H];  // transposes of MLP.3 / 5 / 8 / 10
  __shared__ __attribute__((aligned(16))) float sA[H * RS];      // [j][row] images: gradients at a layer's output ..
  __shared__ __attribute__((aligned(16))) float sB[H * RS];      // .. and the layer's inputs
  __shared__ __attribute__((aligned(16))) float sWT5[H * EP];    // transpose of the padded MLP.13: [k][e]
  __shared__ float sGh[EP * 3], sM[EP * 2], sRed[16], sLoss[4];

  const int tid = threadIdx.x, run = blockIdx.x, E = a.E;
  const TrainArgs& ka = *(const TrainArgs*)__builtin_amdgcn_kernarg_segment_ptr();   // = a, see late()

  for (int i = tid; i < PL; i += NT) { sW[i] = 0.f; sGr[i] = 0.f; }
  if (tid < EP) {
    const bool on = tid < E;
    const float *G = late(ka.G), *h = late(ka.h);
    sGh[2 * tid] = on ? G[((size_t)run * E + tid) * 2] : 0.f;
    sGh[2 * tid + 1] = on ? G[((size_t)run * E + tid) * 2 + 1] : 0.f;
    sGh[2 * EP + tid] = on ? h[(size_t)run * E + tid] : 0.f;
  }
  __syncthreads();
  {
    const int P = O_W5 + (H + 1) * late(ka.E);                 // (per lane, as everything that is used once per launch or step)
    const float* gparams = late(ka.params) + (size_t)run * P;
    for (int i = tid; i < P; i += NT) sW[lds_index(i, E)] = gparams[i];
  }
  __syncthreads();
  const int woff[4] = {O_W1, O_W2, O_W3, O_W4};
#pragma unroll
  for (int l = 0; l < 4; ++l)
    for (int i = tid; i < H * H; i += NT) sWT[l * H * H + (i & 31) * H + (i >> 5)] = sW[woff[l] + i];
  sWT5[(tid & 31) * EP + (tid >> 5)] = sW[O_W5 + tid];
  const int t0 = a.train ? late(ka.step_count)[run] : 0;
  __syncthreads();

  for (int s = 0; s < a.steps; ++s) {
    const long long n = late(ka.n), batch = late(ka.batch), row0 = late(ka.first_row) + s * batch;      // (per lane: no SGPRs held)
    const int nb = __builtin_amdgcn_readfirstlane((int)(n - row0 < batch ? n - row0 : batch));
    if (tid < EP) {
      const float* rot = late(ka.rot);
      const float c = rot[2 * s], sn = rot[2 * s + 1], g0 = sGh[2 * tid], g1 = sGh[2 * tid + 1];
      sM[tid] = -(c * g0 - sn * g1);
      sM[EP + tid] = -(sn * g0 + c * g1);
    }
    if (tid < 4) sLoss[tid] = 0.f;
    if (a.train)
      for (int i = tid; i < PL; i += NT) sGr[i] = 0.f;          // the chunks of the batch add into it
    __syncthreads();
    const float inv_b = 1.f / (float)nb;
    const float cm = 2.f / ((float)nb * (float)E), cd = 2.f * inv_b, ca = inv_b, cb = 2.f * inv_b;

    for (int c0 = 0; c0 < nb; c0 += NT) {
      const int cnt = nb - c0 < NT ? nb - c0 : NT, cnt4 = (cnt + 3) & ~3;
      const bool valid = tid < cnt;
      float px = 0.f, py = 0.f, dl = 0.f, mul[EP];
#pragma unroll
      for (int e = 0; e < EP; ++e) mul[e] = 0.f;
      if (valid) {
        const long long r = (long long)run * n + row0 + c0 + tid;          // row of the stacked data sets
        const float *gpts = late(ka.points), *gmu = late(ka.mu);
        px = gpts[2 * r];
        py = gpts[2 * r + 1];
        dl = late(ka.dist)[r];
#pragma unroll
        for (int e = 0; e < EP; ++e)
          if (e < E) mul[e] = gmu[r * E + e];
      }
      // ---- forward ----
      float z[H], xh1[H], t1[H], r1[H], xh2[H], t2[H], r2[H], xh3[H], t3[H], mu[EP], rs1, rs2, rs3;
#pragma unroll
      for (int j = 0; j < H; ++j) z[j] = fmaf(sW[O_W0 + 2 * j + 1], py, fmaf(sW[O_W0 + 2 * j], px, sW[O_B0 + j]));
      ln_tanh(sW + O_G0, sW + O_BE0, z, xh1, t1, rs1);
      linear<H, H, true>(sW + O_W1, sW + O_B1, t1, z, sA, tid);
#pragma unroll
      for (int j = 0; j < H; ++j) r1[j] = fmaxf(z[j], 0.f);
      linear<H, H, true>(sW + O_W2, sW + O_B2, r1, z, sA, tid);
      ln_tanh(sW + O_G1, sW + O_BE1, z, xh2, t2, rs2);
      linear<H, H, true>(sW + O_W3, sW + O_B3, t2, z, sA, tid);
#pragma unroll
      for (int j = 0; j < H; ++j) r2[j] = fmaxf(z[j], 0.f);
      linear<H, H, true>(sW + O_W4, sW + O_B4, r2, z, sA, tid);
      ln_tanh(sW + O_G2, sW + O_BE2, z, xh3, t3, rs3);
      linear<H, EP, true>(sW + O_W5, sW + O_B5L, t3, mu, sA, tid);
#pragma unroll
      for (int e = 0; e < EP; ++e) mu[e] = fmaxf(mu[e], 0.f);
      // ---- the four loss terms of the row (rows e >= E of G, h, M and of both mu are zero) ----
      float dist = 0.f, fa0 = 0.f, fa1 = 0.f, fl0 = 0.f, fl1 = 0.f, mh = 0.f, mlh = 0.f, smu = 0.f;
#pragma unroll
      for (int e = 0; e < EP; ++e) {
        const float gpe = fmaf(sGh[2 * e + 1], py, sGh[2 * e] * px) - sGh[2 * EP + e];
        dist = fmaf(mu[e], gpe, dist);
        fa0 = fmaf(mu[e], sM[e], fa0);
        fa1 = fmaf(mu[e], sM[EP + e], fa1);
        fl0 = fmaf(mul[e], sM[e], fl0);
        fl1 = fmaf(mul[e], sM[EP + e], fl1);
        mh = fmaf(mu[e], sGh[2 * EP + e], mh);
        mlh = fmaf(mul[e], sGh[2 * EP + e], mlh);
        const float d = mu[e] - mul[e];
        smu = fmaf(d, d, smu);
      }
      const float fb = fmaf(fa1, py, fa0 * px) + mh, fbl = fmaf(fl1, py, fl0 * px) + mlh;
      const float ed = dist - dl, ea0 = fa0 - fl0, ea1 = fa1 - fl1, eb = fb - fbl;
      float ls[4] = {valid ? smu : 0.f, valid ? ed * ed : 0.f, valid ? fmaf(ea1, ea1, ea0 * ea0) : 0.f, valid ? eb * eb : 0.f};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ls[k] += __shfl_xor(ls[k], o, 64);
      }
      if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sRed[(tid >> 6) * 4 + k] = ls[k];
      }
      __syncthreads();
      if (tid < 4) sLoss[tid] += ((sRed[tid] + sRed[4 + tid]) + sRed[8 + tid]) + sRed[12 + tid];
      __syncthreads();
      if (!a.train) continue;                                    // (uniform)

      // ---- backward ----
      float dy[H], dx[H], d5[EP];
#pragma unroll
      for (int e = 0; e < EP; ++e) {
        const float gpe = fmaf(sGh[2 * e + 1], py, sGh[2 * e] * px) - sGh[2 * EP + e];
        const float dfb = fmaf(sM[EP + e], py, sM[e] * px) + sGh[2 * EP + e];
        float g = cm * (mu[e] - mul[e]);
        g = fmaf(cd * ed, gpe, g);
        g = fmaf(ca * ea0, sM[e], g);
        g = fmaf(ca * ea1, sM[EP + e], g);
        g = fmaf(cb * eb, dfb, g);
        d5[e] = (valid && mu[e] > 0.f) ? g : 0.f;                // through the last ReLU; rows past the batch: zero
      }
      // MLP.13: weight / bias gradient, then dt3 = W5^T dz5
#pragma unroll
      for (int e = 0; e < EP; ++e) sA[e * RS + tid] = d5[e];
      put32(sB, t3, tid);
      __syncthreads();
      dw_pass<EP, H, 1>(sA, sB, cnt4, sGr + O_W5, sGr + O_B5L, tid);
      __syncthreads();
      linear<EP, H, false>(sWT5, nullptr, d5, dx, sA, tid);
      // block 3: LayerNorm MLP.11, Linear MLP.10 (input r2)
      tanh_bwd(dx, t3);
      put32(sA, dx, tid);
      put32(sB, xh3, tid);
      __syncthreads();
      ln_reduce(sA, sB, cnt4, sGr + O_G2, sGr + O_BE2, tid);
      __syncthreads();
      ln_bwd(sW + O_G2, dx, xh3, rs3, dy);
      put32(sA, dy, tid);
      put32(sB, r2, tid);
      __syncthreads();
      dw_pass<H, H, 4>(sA, sB, cnt4, sGr + O_W4, sGr + O_B4, tid);
      __syncthreads();
      linear<H, H, false>(sWT + 3 * H * H, nullptr, dy, dx, sA, tid);
      // Linear MLP.8 (input t2) behind its ReLU
#pragma unroll
      for (int j = 0; j < H; ++j) dy[j] = r2[j] > 0.f ? dx[j] : 0.f;
      put32(sA, dy, tid);
      put32(sB, t2, tid);
      __syncthreads();
      dw_pass<H, H, 4>(sA, sB, cnt4, sGr + O_W3, sGr + O_B3, tid);
      __syncthreads();
      linear<H, H, false>(sWT + 2 * H * H, nullptr, dy, dx, sA, tid);
      // block 2: LayerNorm MLP.6, Linear MLP.5 (input r1)
      tanh_bwd(dx, t2);
      put32(sA, dx, tid);
      put32(sB, xh2, tid);
      __syncthreads();
      ln_reduce(sA, sB, cnt4, sGr + O_G1, sGr + O_BE1, tid);
      __syncthreads();
      ln_bwd(sW + O_G1, dx, xh2, rs2, dy);
      put32(sA, dy, tid);
      put32(sB, r1, tid);
      __syncthreads();
      dw_pass<H, H, 4>(sA, sB, cnt4, sGr + O_W2, sGr + O_B2, tid);
      __syncthreads();
      linear<H, H, false>(sWT + 1 * H * H, nullptr, dy, dx, sA, tid);
      // Linear MLP.3 (input t1) behind its ReLU
#pragma unroll
      for (int j = 0; j < H; ++j) dy[j] = r1[j] > 0.f ? dx[j] : 0.f;
      put32(sA, dy, tid);
      put32(sB, t1, tid);
      __syncthreads();
      dw_pass<H, H, 4>(sA, sB, cnt4, sGr + O_W1, sGr + O_B1, tid);
      __syncthreads();
      linear<H, H, false>(sWT, nullptr, dy, dx, sA, tid);
      // block 1: LayerNorm MLP.1, Linear MLP.0 (input p)
      tanh_bwd(dx, t1);
      put32(sA, dx, tid);
      put32(sB, xh1, tid);
      __syncthreads();
      ln_reduce(sA, sB, cnt4, sGr + O_G0, sGr + O_BE0, tid);
      __syncthreads();
      ln_bwd(sW + O_G0, dx, xh1, rs1, dy);
      put32(sA, dy, tid);
      sB[tid] = px;
      sB[RS + tid] = py;
      __syncthreads();
      dw_pass<H, 2, 1>(sA, sB, cnt4, sGr + O_W0, sGr + O_B0, tid);
      __syncthreads();
    }

    if (tid < 4) {
      const float cnt = tid == 0 ? (float)nb * (float)E : (tid == 2 ? 2.f * (float)nb : (float)nb);
      late(ka.losses)[((size_t)run * a.steps + s) * 4 + tid] = sLoss[tid] / cnt;
    }
    if (a.train) {
      // ---- Adam (torch.optim.Adam), t = step_count + s + 1 ----
      const int t = t0 + s + 1, P = O_W5 + (H + 1) * late(ka.E);
      const float step_size = (float)(late(ka.lr) / (1.0 - exp((double)t * late(ka.log_beta1))));
      const float bc2s = (float)sqrt(1.0 - exp((double)t * late(ka.log_beta2)));
      const float om_beta1 = late(ka.om_beta1), om_beta2 = late(ka.om_beta2), beta2 = late(ka.beta2f), eps = late(ka.eps),
                  weight_decay = late(ka.weight_decay);
      float *adam_m = late(ka.adam_m) + (size_t)run * P, *adam_v = late(ka.adam_v) + (size_t)run * P;
      float* grad_out = s == a.steps - 1 ? late(ka.grad_out) : nullptr;      // (the last step's gradient only)
      for (int i = tid; i < P; i += NT) {
        const int li = lds_index(i, E);
        float g = sGr[li];
        if (grad_out) grad_out[(size_t)run * P + i] = g;
        float p = sW[li], m = adam_m[i], v = adam_v[i];
        // torch's kernels to the bit (measured on the device against torch.optim.Adam, every candidate rounding tried): each
        // of its foreach kernels contracts its one multiply-add -- add(alpha), lerp, addcmul = self + value (g g), addcdiv =
        // self + value (m / denom) -- and its sqrt is the correctly rounded one (the double root of a float rounds to it)
        g = fmaf(weight_decay, p, g);
        m = fmaf(om_beta1, __fsub_rn(g, m), m);
        v = fmaf(om_beta2, __fmul_rn(g, g), __fmul_rn(beta2, v));
        const float denom = __fadd_rn(__fdiv_rn((float)sqrt((double)v), bc2s), eps);
        p = fmaf(-step_size, __fdiv_rn(m, denom), p);
        sW[li] = p;
        adam_m[i] = m;
        adam_v[i] = v;
      }
      __syncthreads();
#pragma unroll
      for (int l = 0; l < 4; ++l)
        for (int i = tid; i < H * H; i += NT) sWT[l * H * H + (i & 31) * H + (i >> 5)] = sW[woff[l] + i];
      sWT5[(tid & 31) * EP + (tid >> 5)] = sW[O_W5 + tid];
    }
    __syncthreads();
  }
  if (a.train) {
    const int P = O_W5 + (H + 1) * late(ka.E);
    float* gparams = late(ka.params) + (size_t)run * P;
    for (int i = tid; i < P; i += NT) gparams[i] = sW[lds_index(i, E)];
    if (tid == 0) late(ka.step_count)[run] = t0 + a.steps;
  }
}

thread_local std::string g_train_err;
int fail(int code, const std::string& msg) { g_train_err = msg; return code; }

// a float that was written as a decimal number, as that number (7 significant digits)
double decimal7(float x) {
  if (!(x > 0.f) || !__builtin_isfinite(x)) return (double)x;
  char buf[32];
  snprintf(buf, sizeof buf, "%.7g", (double)x);
  return strtod(buf, nullptr);
}

}  // namespace

extern "C" const char* npa_dune_train_last_error(void) { return g_train_err.c_str(); }

extern "C" int npa_dune_train_param_count(int edge_num) {
  if (edge_num < 3 || edge_num > NPA_MAX_E) return fail(NPA_E_ARG, "npa_dune_train_param_count: edge_num outside [3,NPA_MAX_E]");
  return O_W5 + (H + 1) * edge_num;
}

extern "C" int npa_dune_train_steps(int runs, int edge_num, const float* G, const float* h, int64_t n, const float* points,
                                    const float* mu, const float* dist, int64_t first_row, int batch, int steps, const float* rot,
                                    float lr, float beta1, float beta2, float eps, float weight_decay, int train, float* params,
                                    float* adam_m, float* adam_v, int32_t* step_count, float* losses, float* grad_out,
                                    void* stream) {
  if (edge_num < 3 || edge_num > NPA_MAX_E) return fail(NPA_E_ARG, "npa_dune_train_steps: edge_num outside [3,NPA_MAX_E]");
  if (runs < 1 || batch < 1 || steps < 1 || n < 1 || first_row < 0)
    return fail(NPA_E_ARG, "npa_dune_train_steps: runs, batch, steps, n must be >= 1 and first_row >= 0");
  if (first_row + (int64_t)(steps - 1) * batch >= n) return fail(NPA_E_ARG, "npa_dune_train_steps: a step past the last row (empty batch)");
  if (!G || !h || !points || !mu || !dist || !rot || !params || !losses)
    return fail(NPA_E_ARG, "npa_dune_train_steps: a required pointer is NULL");
  if (train && (!adam_m || !adam_v || !step_count))
    return fail(NPA_E_ARG, "npa_dune_train_steps: adam_m, adam_v and step_count are required when train != 0");
  TrainArgs a;
  a.E = edge_num; a.batch = batch; a.steps = steps; a.train = train ? 1 : 0;
  a.n = n; a.first_row = first_row;
  a.G = G; a.h = h; a.points = points; a.mu = mu; a.dist = dist; a.rot = rot;
  a.params = params; a.adam_m = adam_m; a.adam_v = adam_v; a.losses = losses; a.grad_out = train ? grad_out : nullptr;
  a.step_count = step_count;
  const double b1 = decimal7(beta1), b2 = decimal7(beta2);
  a.log_beta1 = b1 > 0.0 ? log(b1) : -1e300; a.log_beta2 = b2 > 0.0 ? log(b2) : -1e300; a.lr = decimal7(lr);
  a.om_beta1 = (float)(1.0 - b1); a.om_beta2 = (float)(1.0 - b2); a.beta2f = (float)b2;
  a.eps = eps; a.weight_decay = weight_decay;
  hipLaunchKernelGGL(dune_train_kernel, dim3((unsigned)runs), dim3(NT), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NPA_E_HIP, std::string("npa_dune_train_steps: launch: ") + hipGetErrorString(e));
  return NPA_OK;
}
