// dune_device.h -- device side of dune.hip up to and including select_geo_kernel (helpers, encoder, key and selection
// kernels); the host launchers and the calibration kernels stay in dune.hip.  Included by dune.hip.
#pragma once

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define DUNE_THREADS 256
#define DUNE_WAVES 4

#define WSYNC()                                              \
  do {                                                       \
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   \
    __builtin_amdgcn_wave_barrier();                         \
  } while (0)

__device__ __forceinline__ float pair_sum(float x) {
  // value + value of lane^32 (bitwise identical in both lanes: fp add commutes)
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

__device__ __forceinline__ float tanh_scaled(float y) {
  // tanh(x) = 1 - 2/(exp(2x)+1) with y = 2*log2(e)*x prepared by the caller (the factor is
  // folded into the LayerNorm affine vectors on the host); |abs err| <~ 1.5e-7, saturates at +-1
  float e = __builtin_amdgcn_exp2f(y);
  return fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
}

__device__ __forceinline__ void load_vec16(const float* v, int hf, float out[16]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float4 t = *reinterpret_cast<const float4*>(v + 8 * q + 4 * hf);
    out[4 * q + 0] = t.x; out[4 * q + 1] = t.y; out[4 * q + 2] = t.z; out[4 * q + 3] = t.w;
  }
}

// PERM: the vector is the PERMUTED image of the 16-point tile (pan_common.h WP_VEC16: [kq 4][s 8]).  Register r = 2 i + h2 of a
// lane of the 32-point tile holds feature npa_feat16(i, hf + 2 h2): entry i of group hf (even registers) / 2 + hf (odd ones), so the
// same four 16-byte loads serve -- the selection keeps ONE image of the vectors in LDS for both tile shapes.
template <bool PERM>
__device__ __forceinline__ void load_vec16x(const float* v, int hf, float out[16]) {
  if constexpr (!PERM) {
    load_vec16(v, hf, out);
  } else {
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
      for (int qq = 0; qq < 2; ++qq) {
        const float4 t = *reinterpret_cast<const float4*>(v + 16 * h2 + 8 * hf + 4 * qq);
        out[2 * (4 * qq + 0) + h2] = t.x; out[2 * (4 * qq + 1) + h2] = t.y; out[2 * (4 * qq + 2) + h2] = t.z; out[2 * (4 * qq + 3) + h2] = t.w;
      }
  }
}
template <bool PERM = false>
__device__ __forceinline__ f32x16 bias_init(const float* v, int hf) {
  float b[16];
  load_vec16x<PERM>(v, hf, b);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = b[r];
  return acc;
}

// ---- the canonical reduction order of a point's 32 features (shared by the 32-point and the 16-point tile) ------------------
// The features fall into four groups of eight, group kq = {npa_feat16(s, kq), s = 0..7} (pan_common.h): what ONE lane of the
// 16-point tile holds, and what the even (kq = hf) / odd (kq = 2 + hf) accumulator registers of a lane of the 32-point tile hold.
// A sum over the 32 features is p_kq = the chain over s = 0..7 inside each group, then (p_0 + p_1) + (p_2 + p_3): the same
// operations in the same order in both layouts (fp addition commutes), so the two tile shapes give BITWISE the same rows.
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float quad_sum(float x) {
  // (row 0 + row 1) + (row 2 + row 3) of the four 16-lane rows, the same bits in all four
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return pair_sum(__uint_as_float(r[0]) + __uint_as_float(r[1]));
}

// LayerNorm(32, eps=1e-5, affine) + tanh on a point's 32 features (16 here, 16 in lane^32)
template <bool PERM = false>
__device__ __forceinline__ void ln_tanh(f32x16 acc, const float* g, const float* be, int hf, float a[16]) {
  float se = acc[0], so = acc[1];
#pragma unroll
  for (int r = 2; r < 16; r += 2) { se += acc[r]; so += acc[r + 1]; }
  float mean = (pair_sum(se) + pair_sum(so)) * (1.0f / 32.0f);
  float qe = 0.f, qo = 0.f;
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    a[r] = acc[r] - mean; qe = fmaf(a[r], a[r], qe);
    a[r + 1] = acc[r + 1] - mean; qo = fmaf(a[r + 1], a[r + 1], qo);
  }
  float var = (pair_sum(qe) + pair_sum(qo)) * (1.0f / 32.0f);
  float ve = var + 1e-5f;
  float rstd = __builtin_amdgcn_rsqf(ve);                 // v_rsq_f32 (1 ulp) + one Newton step
  rstd = rstd * fmaf(-0.5f * ve * rstd, rstd, 1.5f);
  // affine vectors fetched four features at a time (keeps the live register set small)
  if constexpr (PERM) {
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
      for (int qq = 0; qq < 2; ++qq) {
        const float4 gv = *reinterpret_cast<const float4*>(g + 16 * h2 + 8 * hf + 4 * qq);
        const float4 bv = *reinterpret_cast<const float4*>(be + 16 * h2 + 8 * hf + 4 * qq);
        const int r0 = 2 * (4 * qq) + h2;
        a[r0 + 0] = tanh_scaled(fmaf(a[r0 + 0] * rstd, gv.x, bv.x));
        a[r0 + 2] = tanh_scaled(fmaf(a[r0 + 2] * rstd, gv.y, bv.y));
        a[r0 + 4] = tanh_scaled(fmaf(a[r0 + 4] * rstd, gv.z, bv.z));
        a[r0 + 6] = tanh_scaled(fmaf(a[r0 + 6] * rstd, gv.w, bv.w));
      }
    return;
  }
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    float4 gv = *reinterpret_cast<const float4*>(g + 8 * qd + 4 * hf);
    float4 bv = *reinterpret_cast<const float4*>(be + 8 * qd + 4 * hf);
    a[4 * qd + 0] = tanh_scaled(fmaf(a[4 * qd + 0] * rstd, gv.x, bv.x));
    a[4 * qd + 1] = tanh_scaled(fmaf(a[4 * qd + 1] * rstd, gv.y, bv.y));
    a[4 * qd + 2] = tanh_scaled(fmaf(a[4 * qd + 2] * rstd, gv.z, bv.z));
    a[4 * qd + 3] = tanh_scaled(fmaf(a[4 * qd + 3] * rstd, gv.w, bv.w));
  }
}

// max / min / ReLU WITHOUT the canonicalising v_max_f32 x, x, x that fmaxf / fminf get in front of them whenever the compiler cannot
// prove an operand quiet (an MFMA accumulator, a DPP or lane read, a load): the median of (a, b, +inf) IS max(a, b), one
// v_med3_f32, and takes its operands as they are.  With one NaN operand v_med3_f32 returns min3, the other operand: what fmaxf
// returns.  The sites (select_geo_body.inc, the exact encoder's ReLU) and what a NaN does at each: DESIGN.md section 3.1.
// (the +inf sits in a register behind an empty asm: as a literal the compiler folds the median back into fmaxf, canonicalisation and all)
__device__ __forceinline__ float inf_reg() { float v = __builtin_inff(); asm("" : "+v"(v)); return v; }
__device__ __forceinline__ float max_nc(float a, float b) { return __builtin_amdgcn_fmed3f(a, b, inf_reg()); }
__device__ __forceinline__ float min_nc(float a, float b) { return -__builtin_amdgcn_fmed3f(-a, -b, inf_reg()); }
__device__ __forceinline__ float relu_acc(float x) { return max_nc(x, 0.f); }

__device__ __forceinline__ f32x16 layer32(const float (&w)[16], const float (&a)[16], f32x16 acc) {
#pragma unroll
  for (int r = 0; r < 16; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[r], a[r], acc, 0, 0, 0);
  return acc;
}

// ---- fp16x2 split-precision layer (dune_kernel only: distance keys) ------------------------------
// x = x1 + x2, w = w1 + w2 with fp16 terms (RNE of the running residual: |x - x1 - x2| <= 2^-22 |x|
// while the terms are normal numbers, which the host-chosen power-of-two scales guarantee for
// every value that matters), product terms (2,1) (1,2) (1,1); the dropped (2,2) term is <= 2^-22
// relative.  Each fp16 x fp16 product is exact in the fp32 accumulator.  6 x 32-cycle MFMAs per
// layer instead of 16 x 64-cycle fp32-input ones.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));


// RELU = true: the split is taken of max(a, 0) (the activation of the Linear->ReLU layers)
template <bool RELU>
__device__ __forceinline__ void split2(const float (&a)[16], f16x8 (&x1)[2], f16x8 (&x2)[2]) {
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    f32x2_t v = {a[2 * p], a[2 * p + 1]};
    if constexpr (RELU) {
      // integer max on the bit pattern = ReLU in ONE instruction (fmaxf would first canonicalise the
      // MFMA result with a second v_max; negative floats are negative ints, -0 -> +0)
      v.x = __int_as_float(max(__float_as_int(v.x), 0));
      v.y = __int_as_float(max(__float_as_int(v.y), 0));
    }
    const f16x2 b1 = __builtin_convertvector(v, f16x2);                 // v_cvt_pk_f16_f32 (RNE)
    const f32x2_t r1 = v - __builtin_convertvector(b1, f32x2_t);
    const f16x2 b2 = __builtin_convertvector(r1, f16x2);
    const int s = p >> 2, q = (2 * p) & 7;
    x1[s][q] = b1.x; x1[s][q + 1] = b1.y;
    x2[s][q] = b2.x; x2[s][q + 1] = b2.y;
  }
}

// wl: LDS image of one layer's split A-fragments [term 2][step 2][lane 64] x 16 B
// TERMS = 3: the split product above.  TERMS = 1: leading fp16 terms only (2^-11 relative per factor): two MFMAs and
// eight conversions per layer; usable because the keys only nominate candidates (select_kernel's margin).
template <bool RELU, int TERMS>
__device__ __forceinline__ f32x16 layer32_f16x2(const f16x8* wl, int lane, const float (&a)[16], f32x16 acc) {
  if constexpr (TERMS == 1) {
    f16x8 x[2];
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      f16x2 b1 = __builtin_convertvector(f32x2_t{a[2 * p], a[2 * p + 1]}, f16x2);       // v_cvt_pk_f16_f32
      if constexpr (RELU) b1 = __builtin_elementwise_max(b1, f16x2{(_Float16)0.f, (_Float16)0.f});   // v_pk_max_f16
      const int s = p >> 2, q = (2 * p) & 7;
      x[s][q] = b1.x; x[s][q + 1] = b1.y;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[(0 * 2 + s) * 64 + lane], x[s], acc, 0, 0, 0);
    return acc;
  }
  f16x8 x1[2], x2[2];
  split2<RELU>(a, x1, x2);
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const f16x8 w1 = wl[(0 * 2 + s) * 64 + lane], w2 = wl[(1 * 2 + s) * 64 + lane];
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(w2, x1[s], acc, 0, 0, 0);      // small terms first
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1, x2[s], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1, x1[s], acc, 0, 0, 0);
  }
  return acc;
}

// ---- key path: reassociated encoder (packed fp32 VALU, LayerNorm centring folded into the weights) --
typedef float f32x2 __attribute__((ext_vector_type(2)));

// acc holds CENTRED pre-activations (mean removed through W_c, b_c): var = sum(acc^2)/32
__device__ __forceinline__ void ln_tanh_centred(f32x16 acc, const float* g, const float* be, int hf, float eps,
                                                float out_scale, float a[16]) {
  f32x2 q2 = {0.f, 0.f};
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const f32x2 v = {acc[2 * p], acc[2 * p + 1]};
    q2 = __builtin_elementwise_fma(v, v, q2);
  }
  const float ve = fmaf(pair_sum(q2.x + q2.y), 1.0f / 32.0f, eps);
  float rstd = __builtin_amdgcn_rsqf(ve);
  rstd = rstd * fmaf(-0.5f * ve * rstd, rstd, 1.5f);
  // out_scale * tanh: out_scale - 2 out_scale / (e + 1)
  const f32x2 rs = {rstd, rstd}, one = {1.f, 1.f}, osc = {out_scale, out_scale}, mtwo = {-2.f * out_scale, -2.f * out_scale};
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    const float4 gv = *reinterpret_cast<const float4*>(g + 8 * qd + 4 * hf);
    const float4 bv = *reinterpret_cast<const float4*>(be + 8 * qd + 4 * hf);
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const f32x2 x = {acc[4 * qd + 2 * hh], acc[4 * qd + 2 * hh + 1]};
      const f32x2 gg = hh ? f32x2{gv.z, gv.w} : f32x2{gv.x, gv.y};
      const f32x2 bb = hh ? f32x2{bv.z, bv.w} : f32x2{bv.x, bv.y};
      const f32x2 y = __builtin_elementwise_fma(x * rs, gg, bb);
      f32x2 e = {__builtin_amdgcn_exp2f(y.x), __builtin_amdgcn_exp2f(y.y)};
      e = e + one;
      const f32x2 r = {__builtin_amdgcn_rcpf(e.x), __builtin_amdgcn_rcpf(e.y)};
      const f32x2 th = __builtin_elementwise_fma(r, mtwo, osc);
      a[4 * qd + 2 * hh] = th.x; a[4 * qd + 2 * hh + 1] = th.y;
    }
  }
}

// LDS image of the key path: split fragments, then kvec [5][32], then ksc [8] (pan_common.h)
template <int E, int TERMS>
__device__ __forceinline__ void encode_tile_keys(float kw1, const f16x8* wbf, const float* vec, const float* w6,
                                                 const float* b6, float p0x, float p0y, int lane, float mu[E]) {
  const int hf = lane >> 5;
  const float* kvec = reinterpret_cast<const float*>(wbf) + WP_BF_FLOATS;
  const float* ksc = kvec + 5 * 32;
  constexpr int LSTR = 2 * 2 * 64;          // fragments per layer
  float a[16];
  {
    f32x16 acc = bias_init(kvec + 0 * 32, hf);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kw1, hf ? p0y : p0x, acc, 0, 0, 0);
    ln_tanh_centred(acc, vec + V_G1 * 32, vec + V_BE1 * 32, hf, ksc[0], ksc[3], a);
  }
  // the ReLU of Linear 2 / Linear 4 is applied inside the split of the following layer
  {
    f32x16 acc = layer32_f16x2<false, TERMS>(wbf + 0 * LSTR, lane, a, bias_init(kvec + 1 * 32, hf));
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = acc[r];
  }
  {
    f32x16 acc = layer32_f16x2<true, TERMS>(wbf + 1 * LSTR, lane, a, bias_init(kvec + 2 * 32, hf));
    ln_tanh_centred(acc, vec + V_G2 * 32, vec + V_BE2 * 32, hf, ksc[1], ksc[4], a);
  }
  {
    f32x16 acc = layer32_f16x2<false, TERMS>(wbf + 2 * LSTR, lane, a, bias_init(kvec + 3 * 32, hf));
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = acc[r];
  }
  {
    f32x16 acc = layer32_f16x2<true, TERMS>(wbf + 3 * LSTR, lane, a, bias_init(kvec + 4 * 32, hf));
    ln_tanh_centred(acc, vec + V_G3 * 32, vec + V_BE3 * 32, hf, ksc[2], ksc[5], a);
  }
  // output layer: two features per packed FMA (rows of Linear 6 as stored for the exact path)
#pragma unroll
  for (int e = 0; e < E; ++e) {
    float wv[16];
    load_vec16(w6 + e * 32, hf, wv);
    f32x2 s2 = {0.f, 0.f};
#pragma unroll
    for (int p = 0; p < 8; ++p)
      s2 = __builtin_elementwise_fma(f32x2{wv[2 * p], wv[2 * p + 1]}, f32x2{a[2 * p], a[2 * p + 1]}, s2);
    mu[e] = fmaxf(pair_sum(s2.x + s2.y) + b6[e], 0.f);
  }
}

struct WaveWeights {
  float w1;
  float wl[4][16];
};

// Encoder for the 32 points of a tile.  p0x/p0y: the point in the robot frame (both lanes of
// a pair hold both).  Returns mu[e] (e<E) in BOTH lanes of the pair.
// Exact fp32 MFMA (v_mfma_f32_32x32x2_f32), weights in W.wl; the reference's operation order.
template <int E>
__device__ __forceinline__ void encode_tile(const WaveWeights& W, const float* vec, const float* w6, const float* b6,
                                            float p0x, float p0y, int lane, float mu[E]) {
  const int hf = lane >> 5;
  auto layer = [&](int L, const float (&a_)[16], f32x16 acc) -> f32x16 { return layer32(W.wl[L], a_, acc); };
  float a[16];
  {
    f32x16 acc = bias_init(vec + V_B1 * 32, hf);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(W.w1, hf ? p0y : p0x, acc, 0, 0, 0);
    ln_tanh(acc, vec + V_G1 * 32, vec + V_BE1 * 32, hf, a);
  }
  {
    f32x16 acc = layer(0, a, bias_init(vec + V_B2 * 32, hf));
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = fmaxf(acc[r], 0.f);
  }
  {
    f32x16 acc = layer(1, a, bias_init(vec + V_B3 * 32, hf));
    ln_tanh(acc, vec + V_G2 * 32, vec + V_BE2 * 32, hf, a);
  }
  {
    f32x16 acc = layer(2, a, bias_init(vec + V_B4 * 32, hf));
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = fmaxf(acc[r], 0.f);
  }
  {
    f32x16 acc = layer(3, a, bias_init(vec + V_B5 * 32, hf));
    ln_tanh(acc, vec + V_G3 * 32, vec + V_BE3 * 32, hf, a);
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    float wv[16];
    load_vec16(w6 + e * 32, hf, wv);
    float se = 0.f, so = 0.f;                 // (the canonical order: even / odd registers are two of the four feature groups)
#pragma unroll
    for (int r = 0; r < 16; r += 2) { se = fmaf(wv[r], a[r], se); so = fmaf(wv[r + 1], a[r + 1], so); }
    mu[e] = fmaxf((pair_sum(se) + pair_sum(so)) + b6[e], 0.f);
  }
}

// The same encoder with the weights of the four 32x32 layers STREAMED from the lane-major copy (WP_WLS) instead of held
// in 64 registers: the next layer's sixteen fragments are requested (four 16-byte loads, L1 / L2 resident: every wave of
// the chip reads the same 16 KB) before the current layer's sixteen MFMAs start, which take ~1000 cycles.  Same
// arithmetic in the same order as encode_tile: bitwise the same rows.
__device__ __forceinline__ void load_layer(const float* __restrict__ wls, int L, int lane, float (&w)[16]) {
  // (the LANE INDEX passes through an opaque asm: the loads are loop-invariant, and the compiler would otherwise hoist all
  // four layers out of the tile loop and keep them in 64 registers -- the layout this form exists to avoid.  The index, not the
  // pointer: a pointer that went through an asm loses its address space and every access behind it becomes a FLAT load, which
  // counts on vmcnt AND lgkmcnt and made the compiler put s_waitcnt vmcnt(0) lgkmcnt(0) in front of every layer -- the
  // prefetched next layer's round trip in full, four times per tile)
  asm volatile("" : "+v"(lane));
  const float4* p = reinterpret_cast<const float4*>(wls + ((size_t)L * 64 + lane) * 16);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 v = p[q];
    w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
  }
}
// PERM: vec / w6 are the permuted images of the 16-point tile (load_vec16x)
template <int E, bool PERM = false>
__device__ __forceinline__ void encode_tile_stream(float w1, const float* __restrict__ wls, const float* vec, const float* w6,
                                                   const float* b6, float p0x, float p0y, int lane, float mu[E]) {
  int hf = lane >> 5;
  if constexpr (PERM) asm volatile("" : "+v"(hf));      // (both tile shapes sit in one tile loop: keep the LDS reads in place, see encode_tile16_stream)
  float a[16], wa[16], wb[16];
  // (scheduling barriers between the blocks: left alone the scheduler hoists all four layers' loads to the top -- the
  // 64 registers this form exists to avoid)
  load_layer(wls, 0, lane, wa);
  __builtin_amdgcn_sched_barrier(0);       // (the prefetch is ISSUED here: left to the scheduler it sinks to the end of the layer in front of it)
  {
    f32x16 acc = bias_init<PERM>(vec + V_B1 * 32, hf);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w1, hf ? p0y : p0x, acc, 0, 0, 0);
    ln_tanh<PERM>(acc, vec + V_G1 * 32, vec + V_BE1 * 32, hf, a);
  }
  __builtin_amdgcn_sched_barrier(0);
  load_layer(wls, 1, lane, wb);
  __builtin_amdgcn_sched_barrier(0);       // (the prefetch is ISSUED here: left to the scheduler it sinks to the end of the layer in front of it)
  {
    f32x16 acc = layer32(wa, a, bias_init<PERM>(vec + V_B2 * 32, hf));
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = relu_acc(acc[r]);
  }
  __builtin_amdgcn_sched_barrier(0);
  load_layer(wls, 2, lane, wa);
  __builtin_amdgcn_sched_barrier(0);       // (the prefetch is ISSUED here: left to the scheduler it sinks to the end of the layer in front of it)
  {
    f32x16 acc = layer32(wb, a, bias_init<PERM>(vec + V_B3 * 32, hf));
    ln_tanh<PERM>(acc, vec + V_G2 * 32, vec + V_BE2 * 32, hf, a);
  }
  __builtin_amdgcn_sched_barrier(0);
  load_layer(wls, 3, lane, wb);
  __builtin_amdgcn_sched_barrier(0);       // (the prefetch is ISSUED here: left to the scheduler it sinks to the end of the layer in front of it)
  {
    f32x16 acc = layer32(wa, a, bias_init<PERM>(vec + V_B4 * 32, hf));
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = relu_acc(acc[r]);
  }
  __builtin_amdgcn_sched_barrier(0);
  {
    f32x16 acc = layer32(wb, a, bias_init<PERM>(vec + V_B5 * 32, hf));
    ln_tanh<PERM>(acc, vec + V_G3 * 32, vec + V_BE3 * 32, hf, a);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    float wv[16];
    load_vec16x<PERM>(w6 + e * 32, hf, wv);
    float se = 0.f, so = 0.f;                 // (the canonical order: even / odd registers are two of the four feature groups)
#pragma unroll
    for (int r = 0; r < 16; r += 2) { se = fmaf(wv[r], a[r], se); so = fmaf(wv[r + 1], a[r + 1], so); }
    mu[e] = fmaxf((pair_sum(se) + pair_sum(so)) + b6[e], 0.f);
  }
}

// ---- the exact encoder on a tile of SIXTEEN points (v_mfma_f32_16x16x4_f32) -------------------------------------------------
// The selection's candidate lists carry a median of 14-19 points: a 32-point tile is half padding.  Here a
// point is four lanes (lane group kq = lane >> 4 holds eight of its 32 features, pan_common.h WP_W116), a layer is 16 MFMAs of 32
// cycles on two independent accumulators (dependent latency 40 cycles: alternating them runs at the issue rate), the elementwise
// work per lane is half a 32-point tile's.  Same fma chains in the same K order and the canonical reductions above: bitwise the
// rows of encode_tile / encode_tile_stream.  vec / w6 / b6: the PERMUTED images (WP_VEC16).
__device__ __forceinline__ f32x4 ld4(const float* p) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  return f32x4{t.x, t.y, t.z, t.w};
}
__device__ __forceinline__ void ln_tanh16(f32x4 c0, f32x4 c1, const float* g, const float* be, int kq, float a[8]) {
  float s = c0[0];
  s += c0[1]; s += c0[2]; s += c0[3]; s += c1[0]; s += c1[1]; s += c1[2]; s += c1[3];
  const float mean = quad_sum(s) * (1.0f / 32.0f);
  float q = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) { a[r] = c0[r] - mean; q = fmaf(a[r], a[r], q); }
#pragma unroll
  for (int r = 0; r < 4; ++r) { a[4 + r] = c1[r] - mean; q = fmaf(a[4 + r], a[4 + r], q); }
  const float var = quad_sum(q) * (1.0f / 32.0f);
  const float ve = var + 1e-5f;
  float rstd = __builtin_amdgcn_rsqf(ve);
  rstd = rstd * fmaf(-0.5f * ve * rstd, rstd, 1.5f);
#pragma unroll
  for (int qd = 0; qd < 2; ++qd) {
    const float4 gv = *reinterpret_cast<const float4*>(g + 8 * kq + 4 * qd);
    const float4 bv = *reinterpret_cast<const float4*>(be + 8 * kq + 4 * qd);
    a[4 * qd + 0] = tanh_scaled(fmaf(a[4 * qd + 0] * rstd, gv.x, bv.x));
    a[4 * qd + 1] = tanh_scaled(fmaf(a[4 * qd + 1] * rstd, gv.y, bv.y));
    a[4 * qd + 2] = tanh_scaled(fmaf(a[4 * qd + 2] * rstd, gv.z, bv.z));
    a[4 * qd + 3] = tanh_scaled(fmaf(a[4 * qd + 3] * rstd, gv.w, bv.w));
  }
}
__device__ __forceinline__ void layer16(const float (&w)[16], const float (&a)[8], f32x4& c0, f32x4& c1) {
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[2 * s], a[s], c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[2 * s + 1], a[s], c1, 0, 0, 0);
  }
}
template <int E>
__device__ __forceinline__ void encode_tile16_stream(float w1a, float w1b, const float* __restrict__ wls16, const float* vec,
                                                     const float* w6, const float* b6, float p0x, float p0y, int lane, float mu[E]) {
  // (the LDS reads below are loop-invariant for the caller's tile loop: behind an opaque lane-group INDEX they stay where they
  // are instead of being hoisted into ~120 registers; the index, not the address -- see load_layer)
  int kq = lane >> 4;
  asm volatile("" : "+v"(kq));
  const float* vq = vec + 8 * kq;
  float a[8], wa[16], wb[16];
  load_layer(wls16, 0, lane, wa);
  __builtin_amdgcn_sched_barrier(0);       // (the prefetch is ISSUED here: left to the scheduler it sinks to the end of the layer in front of it)
  {
    f32x4 c0 = ld4(vq + V_B1 * 32), c1 = ld4(vq + V_B1 * 32 + 4);
    // K = 4 with two entries used: the chain is fma(W[i][1], y, fma(W[i][0], x, b)) then twice + 0 * 0 (exact)
    const float bx = kq == 0 ? p0x : (kq == 1 ? p0y : 0.f);
    c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1a, bx, c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1b, bx, c1, 0, 0, 0);
    ln_tanh16(c0, c1, vec + V_G1 * 32, vec + V_BE1 * 32, kq, a);
  }
  __builtin_amdgcn_sched_barrier(0);
  load_layer(wls16, 1, lane, wb);
  __builtin_amdgcn_sched_barrier(0);       // (the prefetch is ISSUED here: left to the scheduler it sinks to the end of the layer in front of it)
  {
    f32x4 c0 = ld4(vq + V_B2 * 32), c1 = ld4(vq + V_B2 * 32 + 4);
    layer16(wa, a, c0, c1);
#pragma unroll
    for (int r = 0; r < 4; ++r) { a[r] = relu_acc(c0[r]); a[4 + r] = relu_acc(c1[r]); }
  }
  __builtin_amdgcn_sched_barrier(0);
  load_layer(wls16, 2, lane, wa);
  __builtin_amdgcn_sched_barrier(0);       // (the prefetch is ISSUED here: left to the scheduler it sinks to the end of the layer in front of it)
  {
    f32x4 c0 = ld4(vq + V_B3 * 32), c1 = ld4(vq + V_B3 * 32 + 4);
    layer16(wb, a, c0, c1);
    ln_tanh16(c0, c1, vec + V_G2 * 32, vec + V_BE2 * 32, kq, a);
  }
  __builtin_amdgcn_sched_barrier(0);
  load_layer(wls16, 3, lane, wb);
  __builtin_amdgcn_sched_barrier(0);       // (the prefetch is ISSUED here: left to the scheduler it sinks to the end of the layer in front of it)
  {
    f32x4 c0 = ld4(vq + V_B4 * 32), c1 = ld4(vq + V_B4 * 32 + 4);
    layer16(wa, a, c0, c1);
#pragma unroll
    for (int r = 0; r < 4; ++r) { a[r] = relu_acc(c0[r]); a[4 + r] = relu_acc(c1[r]); }
  }
  __builtin_amdgcn_sched_barrier(0);
  {
    f32x4 c0 = ld4(vq + V_B5 * 32), c1 = ld4(vq + V_B5 * 32 + 4);
    layer16(wb, a, c0, c1);
    ln_tanh16(c0, c1, vec + V_G3 * 32, vec + V_BE3 * 32, kq, a);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const f32x4 w0 = ld4(w6 + e * 32 + 8 * kq), w1 = ld4(w6 + e * 32 + 8 * kq + 4);
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) s = fmaf(w0[r], a[r], s);
#pragma unroll
    for (int r = 0; r < 4; ++r) s = fmaf(w1[r], a[4 + r], s);
    mu[e] = fmaxf(quad_sum(s) + b6[e], 0.f);
  }
}

// ---- reduced-precision tier of the ROWS (BASELINE.json configs[4]: "bf16 DUNE on MFMA"; NPA_ROWS_PRECISION=bf16) ------------
// The four 32x32 layers as TWO v_mfma_f32_32x32x16_bf16 each (weights rounded to bf16 once on the host, activations rounded
// per layer with v_cvt_pk_bf16_f32, fp32 accumulation) instead of sixteen v_mfma_f32_32x32x2_f32; the 2 -> 32 input layer, the
// LayerNorms / tanh and the 32 -> E output layer stay fp32 as in encode_tile.  NOT the reference's arithmetic: the rows differ
// from the exact ones by ~2^-8 relative per layer, a different selection at rank-M ties follows, and the controls leave the
// 1e-4 band on most scenes (measured distribution: DESIGN.md section 5, tests/test_gpu_parity.py) -- a labelled tier, off by default.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x16 layer32_bf16(const bf16x8* __restrict__ wb, int L, int lane, const float (&a)[16], f32x16 acc) {
  bf16x8 x[2];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const bf16x2 b = __builtin_convertvector(f32x2_t{a[2 * p], a[2 * p + 1]}, bf16x2);       // v_cvt_pk_bf16_f32 (RNE)
    const int s = p >> 2, q = (2 * p) & 7;
    x[s][q] = b.x; x[s][q + 1] = b.y;
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wb[(L * 2 + s) * 64 + lane], x[s], acc, 0, 0, 0);
  return acc;
}
template <int E>
__device__ __forceinline__ void encode_tile_bf16(float w1, const float* __restrict__ wb16, const float* vec, const float* w6,
                                                 const float* b6, float p0x, float p0y, int lane, float mu[E]) {
  const int hf = lane >> 5;
  const bf16x8* wb = reinterpret_cast<const bf16x8*>(wb16);
  float a[16];
  {
    f32x16 acc = bias_init(vec + V_B1 * 32, hf);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w1, hf ? p0y : p0x, acc, 0, 0, 0);
    ln_tanh(acc, vec + V_G1 * 32, vec + V_BE1 * 32, hf, a);
  }
  {
    f32x16 acc = layer32_bf16(wb, 0, lane, a, bias_init(vec + V_B2 * 32, hf));
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = relu_acc(acc[r]);
  }
  {
    f32x16 acc = layer32_bf16(wb, 1, lane, a, bias_init(vec + V_B3 * 32, hf));
    ln_tanh(acc, vec + V_G2 * 32, vec + V_BE2 * 32, hf, a);
  }
  {
    f32x16 acc = layer32_bf16(wb, 2, lane, a, bias_init(vec + V_B4 * 32, hf));
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = relu_acc(acc[r]);
  }
  {
    f32x16 acc = layer32_bf16(wb, 3, lane, a, bias_init(vec + V_B5 * 32, hf));
    ln_tanh(acc, vec + V_G3 * 32, vec + V_BE3 * 32, hf, a);
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    float wv[16];
    load_vec16(w6 + e * 32, hf, wv);
    float se = 0.f, so = 0.f;                 // (the canonical order: even / odd registers are two of the four feature groups)
#pragma unroll
    for (int r = 0; r < 16; r += 2) { se = fmaf(wv[r], a[r], se); so = fmaf(wv[r + 1], a[r + 1], so); }
    mu[e] = fmaxf((pair_sum(se) + pair_sum(so)) + b6[e], 0.f);
  }
}

__device__ __forceinline__ unsigned ordered_key(float d) {
  // monotone float -> uint map; NaN sorts last
  if (d != d) return 0xFFFFFFFEu;
  unsigned b = __float_as_uint(d);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_u64(unsigned long long v) {
  unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xF, 0xF, false);
  unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xF, 0xF, false);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long umin64(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int l) {
  unsigned lo = __builtin_amdgcn_readlane((unsigned)v, l), hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}
// full-wave min of a 64-bit key (DPP inside each 16-lane row, then 4 readlanes); uniform result
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
  v = umin64(v, dpp_u64<0xB1>(v));
  v = umin64(v, dpp_u64<0x4E>(v));
  v = umin64(v, dpp_u64<0x141>(v));
  v = umin64(v, dpp_u64<0x140>(v));
  return umin64(umin64(readlane_u64(v, 0), readlane_u64(v, 16)), umin64(readlane_u64(v, 32), readlane_u64(v, 48)));
}

struct SliceFrame {
  float c, s, tx, ty;         // rotation (fp32 cos/sin of theta) and translation of the robot
  float tstep;                // (float)t
  float rg[2][NPA_MAX_E];     // (-R) @ G^T          (dune.py:89)
};

// source column of logical point n after decimation (util/__init__.py:300: linspace->int)
__device__ __forceinline__ int src_index(int n, int n_raw, int n_use) {
  if (n_use >= n_raw) return n;
  if (n == n_use - 1) return n_raw - 1;
  double step = (double)(n_raw - 1) / (double)(n_use - 1);
  return (int)((double)n * step);
}

// frame of a slice: robot pose at horizon step t, (-R)G^T
// RG_LDS (select_geo_body.inc): the frame's image in LDS, frg[6][NPA_MAX_E] = (-R) G^T (2 rows), G^T (2 rows), h, then c, s, tx, ty,
// tstep -- what the stage loop's point flow and row epilogue read, instead of 5 E + 5 scalars held from here to the emit
// (F.rg is left unset; the caller's wave barrier in front of the first read orders the store)
template <int E, bool RG_LDS = false>
__device__ __forceinline__ void load_frame(const DevParams& P, const float* __restrict__ cur_s,
                                           const float* __restrict__ trig, int b, int t, SliceFrame& F, float* frg = nullptr) {
  // cos / sin come from the table written together with cur_s (stage_kernel, the QP's write-out, trig_kernel): the
  // fp64 libm evaluation costs ~250 slow VALU instructions, which a wave of dune_kernel would otherwise pay for
  // every work ticket (nearly every ticket of a wave lands in a new slice)
  const int T = P.T;
  const float* s = cur_s + (size_t)b * 3 * (T + 1);
  F.tx = s[t];
  F.ty = s[(T + 1) + t];
  F.c = trig[((size_t)b * (T + 1) + t) * 2];
  F.s = trig[((size_t)b * (T + 1) + t) * 2 + 1];
  F.tstep = (float)t;
#pragma unroll
  for (int e = 0; e < E; ++e) {     // (-R) @ G^T, R = [[c,-s],[s,c]]
    F.rg[0][e] = fmaf(-F.c, P.G[e][0], __fmul_rn(F.s, P.G[e][1]));
    F.rg[1][e] = fmaf(-F.s, P.G[e][0], -__fmul_rn(F.c, P.G[e][1]));
  }
  // the frame is wave-uniform: park it in SGPRs, the VGPR budget (128) is tight
  auto uni = [](float v) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v))); };
  if constexpr (RG_LDS) {
    if (threadIdx.x == 0) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        frg[e] = F.rg[0][e]; frg[NPA_MAX_E + e] = F.rg[1][e];
        frg[2 * NPA_MAX_E + e] = P.G[e][0]; frg[3 * NPA_MAX_E + e] = P.G[e][1]; frg[4 * NPA_MAX_E + e] = P.h[e];
      }
      frg[5 * NPA_MAX_E + 0] = F.c; frg[5 * NPA_MAX_E + 1] = F.s; frg[5 * NPA_MAX_E + 2] = F.tx; frg[5 * NPA_MAX_E + 3] = F.ty;
      frg[5 * NPA_MAX_E + 4] = F.tstep;
    }
  }
  F.c = uni(F.c); F.s = uni(F.s); F.tx = uni(F.tx); F.ty = uni(F.ty); F.tstep = uni(F.tstep);
  if constexpr (!RG_LDS) {
#pragma unroll
    for (int e = 0; e < E; ++e) { F.rg[0][e] = uni(F.rg[0][e]); F.rg[1][e] = uni(F.rg[1][e]); }
  }
}

// one point (two lanes) through point flow + encoder + lam/distance
template <int E, int SPLIT>      // 0: exact fp32 encoder; 3 / 1: key path with that many fp16 product terms
__device__ __forceinline__ void point_features(const DevParams& P, const SliceFrame& F, const WaveWeights& W,
                                               const f16x8* wbf, const float* vec, const float* w6, const float* b6,
                                               const float* px_row, const float* py_row, const float* vx_row,
                                               const float* vy_row, int src, int lane, float mu[E], float& gx,
                                               float& gy, float& lx, float& ly, float& dist) {
  // pan.py:182  receding_obs_points = obs_points + i * (point_velocities * dt)
  gx = px_row[src];
  gy = py_row[src];
  if (vx_row) {
    gx = __fadd_rn(gx, __fmul_rn(F.tstep, __fmul_rn(vx_row[src], P.dt32)));
    gy = __fadd_rn(gy, __fmul_rn(F.tstep, __fmul_rn(vy_row[src], P.dt32)));
  }
  // pan.py:210  p0 = R.T @ (obs_points - trans)
  float dx = __fsub_rn(gx, F.tx), dy = __fsub_rn(gy, F.ty);
  float p0x = fmaf(F.c, dx, __fmul_rn(F.s, dy));
  float p0y = fmaf(F.c, dy, -__fmul_rn(F.s, dx));
  if constexpr (SPLIT != 0) encode_tile_keys<E, SPLIT>(W.w1, wbf, vec, w6, b6, p0x, p0y, lane, mu);   // W.w1 = centred fragment
  else encode_tile<E>(W, vec, w6, b6, p0x, p0y, lane, mu);
  lx = 0.f; ly = 0.f; dist = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    lx = fmaf(F.rg[0][e], mu[e], lx);                                  // dune.py:89
    ly = fmaf(F.rg[1][e], mu[e], ly);
    float tmp = __fsub_rn(fmaf(P.G[e][0], p0x, __fmul_rn(P.G[e][1], p0y)), P.h[e]);   // dune.py:121
    dist = fmaf(mu[e], tmp, dist);                                     // dune.py:124
  }
}

// element i of the weight pack with the index, constant part included, in a VECTOR register (behind an empty asm): the
// address is wpack + 4 i as the load forms it.  Written wpack[K + i] with a large constant K, the compiler keeps wpack + 4 K as
// one more 64-bit scalar per K, computed in front of the loop the load sits in, however rarely the load runs
__device__ __forceinline__ float wpack_at(const float* __restrict__ wpack, int i) { asm("" : "+v"(i)); return wpack[i]; }
// point `src` of a scene by INDEX into its two rows -- x at [src], y at [src + n_stride] of ONE base pointer, velocities alike
// (vel null: a static cloud) -- moved to the slice's time and into the robot frame; pan.py:182, :210, the operations of point_features
__device__ __forceinline__ void slice_point(const DevParams& P, const SliceFrame& F, const float* __restrict__ pts,
                                            const float* __restrict__ vel, int n_stride, int src, float& gx, float& gy,
                                            float& p0x, float& p0y) {
  int sy = src + n_stride;
  asm("" : "+v"(sy));                       // (the sum stays an index: folded into the base it is a second row pointer to carry)
  gx = pts[src];
  gy = pts[sy];
  if (vel) {
    gx = __fadd_rn(gx, __fmul_rn(F.tstep, __fmul_rn(vel[src], P.dt32)));
    gy = __fadd_rn(gy, __fmul_rn(F.tstep, __fmul_rn(vel[sy], P.dt32)));
  }
  const float dx = __fsub_rn(gx, F.tx), dy = __fsub_rn(gy, F.ty);
  p0x = fmaf(F.c, dx, __fmul_rn(F.s, dy));
  p0y = fmaf(F.c, dy, -__fmul_rn(F.s, dx));
}

// point_features with the streamed-weight encoder on a 16-point tile (exact rows; same operation order): a point is the four lanes {j, j + 16, j + 32, j + 48}; all four return its row
template <int E>
__device__ __forceinline__ void point_features_stream16(const DevParams& P, const SliceFrame& F, float w1a, float w1b,
                                                        const float* __restrict__ wls16, const float* vec, const float* w6,
                                                        const float* b6, const float* px_row, const float* py_row,
                                                        const float* vx_row, const float* vy_row, int src, int lane, float mu[E],
                                                        float& gx, float& gy, float& lx, float& ly, float& dist, float& p0x,
                                                        float& p0y) {
  gx = px_row[src];
  gy = py_row[src];
  if (vx_row) {
    gx = __fadd_rn(gx, __fmul_rn(F.tstep, __fmul_rn(vx_row[src], P.dt32)));
    gy = __fadd_rn(gy, __fmul_rn(F.tstep, __fmul_rn(vy_row[src], P.dt32)));
  }
  float dx = __fsub_rn(gx, F.tx), dy = __fsub_rn(gy, F.ty);
  p0x = fmaf(F.c, dx, __fmul_rn(F.s, dy));
  p0y = fmaf(F.c, dy, -__fmul_rn(F.s, dx));
  encode_tile16_stream<E>(w1a, w1b, wls16, vec, w6, b6, p0x, p0y, lane, mu);
  lx = 0.f; ly = 0.f; dist = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    lx = fmaf(F.rg[0][e], mu[e], lx);
    ly = fmaf(F.rg[1][e], mu[e], ly);
    float tmp = __fsub_rn(fmaf(P.G[e][0], p0x, __fmul_rn(P.G[e][1], p0y)), P.h[e]);
    dist = fmaf(mu[e], tmp, dist);
  }
}

__device__ __forceinline__ void load_weights(const float* __restrict__ wpack, int lane, WaveWeights& W) {
  W.w1 = wpack[WP_W1 + lane];
#pragma unroll
  for (int l = 0; l < 4; ++l)
#pragma unroll
    for (int r = 0; r < 16; ++r) W.wl[l][r] = wpack[WP_WL + (l * 16 + r) * 64 + lane];
}

// ---- launch 1: distance key of every point of every slice -----------------------------------------
// tile id -> (scene, slice, tile in slice); tiles_per_slice = key_stride/32
// WAVES = waves per workgroup.  4: five workgroups per CU (<= 96 VGPRs).  16: ONE workgroup per CU,
// 4 waves per SIMD at <= 72 VGPRs and a single LDS copy of the weight fragments, which leaves room
// (216 VGPRs per SIMD, 130 KB LDS) for a QP workgroup of another batch to be co-resident.
template <int E, int SPLIT, int WAVES>
// (exact keys for six to eight edges: three waves per SIMD -- the canonical reductions cost the 128-register build 6 - 10 spills)
__global__ __attribute__((amdgpu_flat_work_group_size(64 * WAVES, 64 * WAVES), amdgpu_waves_per_eu(WAVES >= 8 ? 7 : ((SPLIT == 0 && E >= 6) ? 3 : 4))))
void dune_kernel(
    DevParams P, const float* __restrict__ wpack, int n_stride, const float* __restrict__ cur_s,
    const float* __restrict__ points, const float* __restrict__ vel, const int* __restrict__ n_points,
    const int* __restrict__ flags, unsigned* __restrict__ gkeys, int key_stride, int scene0, int nscene, int t0,
    int chunk, const float* __restrict__ trig) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int wg_ticket_s;
  int* wg_ticket = &wg_ticket_s;
  if (threadIdx.x == 0) wg_ticket_s = 0;
  float* vec = smem;                       // [11][32]
  float* w6 = vec + 11 * 32;               // [8][32]
  float* b6 = w6 + 8 * 32;                 // [8]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, hf = lane >> 5;
  const int T = P.T;

  for (int i = tid; i < 11 * 32 + 8 * 32 + 8; i += 64 * WAVES) smem[i] = wpack[WP_VEC + i];
  WaveWeights W;
  const f16x8* wbf = nullptr;
  if constexpr (SPLIT != 0) {
    float* wb = b6 + 8;                     // 16-byte aligned: (11*32 + 8*32 + 8) floats precede it
    for (int i = tid; i < WP_KEY_LDS_FLOATS; i += 64 * WAVES) wb[i] = wpack[WP_BF + i];
    wbf = reinterpret_cast<const f16x8*>(wb);
    W.w1 = wpack[WP_KW1 + lane];
  } else {
    load_weights(wpack, lane, W);
  }
  __syncthreads();                          // the only workgroup barrier: vectors / fragments staged

  const int nsl = T + 1 - t0;
  const int tps = key_stride >> 5;                          // tiles per slice
  const int total = nscene * nsl * tps;                     // < 2^31: checked by the launcher
  // Work distribution: the tile stream is cut into equal contiguous ranges, one per workgroup; inside
  // a workgroup the waves (one per SIMD) draw `chunk`-tile tickets from an LDS counter.  A purely
  // static split per wave is balanced only while the kernel has the chip to itself: a QP wave of
  // another batch in flight slows the DUNE waves on its SIMD by ~1.3x, and every launch would wait
  // for those.  (Tickets from a global counter were measured: same-address device-scope atomics
  // serialise at ~20 ns each, far too slow for 10^4 tickets per launch.)
  const int wg_lo = (int)((long long)total * blockIdx.x / gridDim.x);
  const int wg_hi = (int)((long long)total * (blockIdx.x + 1) / gridDim.x);
  int g = 0, hi = 0, sl = 0, tile = 0;
  int cur_sl = -1, n_raw = 0, n_use = 0, t = 0;
  bool skip = false;
  SliceFrame F;
  const float *px_row = nullptr, *py_row = nullptr, *vx_row = nullptr, *vy_row = nullptr;
  unsigned* key_row = nullptr;
#pragma unroll 1
  for (;; ++g, ++tile) {
    if (g >= hi) {                                          // next ticket: locate it in the stream
      int c = 0;
      if (lane == 0) c = atomicAdd(wg_ticket, chunk);
      g = wg_lo + __builtin_amdgcn_readfirstlane(c);
      if (g >= wg_hi) break;
      hi = g + chunk < wg_hi ? g + chunk : wg_hi;
      sl = (int)((unsigned)g / (unsigned)tps);
      tile = g - sl * tps;
    } else if (tile == tps) {                               // ran into the next slice
      tile = 0;
      ++sl;
    }
    if (sl != cur_sl) {                                     // wave-uniform: a few times per workgroup range
      cur_sl = sl;
      const int bl = (int)((unsigned)sl / (unsigned)nsl), b = bl + scene0;
      t = sl - bl * nsl + t0;
      n_raw = n_points ? n_points[b] : n_stride;
      n_raw = n_raw < 0 ? 0 : (n_raw > n_stride ? n_stride : n_raw);      // the documented contract, enforced
      n_use = n_raw < P.dune_max_num ? n_raw : P.dune_max_num;
      skip = (flags && flags[b * 4 + 0]) || n_use <= 0;     // converged scene (pan.py:144-145) / no points
      if (!skip) {
        load_frame<E>(P, cur_s, trig, b, t, F);
        px_row = points + (size_t)b * 2 * n_stride;
        py_row = px_row + n_stride;
        vx_row = vel ? vel + (size_t)b * 2 * n_stride : nullptr;
        vy_row = vel ? vx_row + n_stride : nullptr;
        key_row = gkeys + ((size_t)b * (T + 1) + t) * key_stride;
      }
    }
    if (skip || tile * 32 >= n_use) continue;
    {
      const int n = tile * 32 + j;
      const int nc = n < n_use ? n : n_use - 1;
      float mu[E], gx, gy, lx, ly, dist;
      point_features<E, SPLIT>(P, F, W, wbf, vec, w6, b6, px_row, py_row, vx_row, vy_row, src_index(nc, n_raw, n_use),
                               lane, mu, gx, gy, lx, ly, dist);
      if (hf == 0 && n < n_use) key_row[n] = ordered_key(dist);
    }
  }
}

// ---- geometric distance of a robot-frame point to the robot polygon (0 inside) ---------------------------
// min over the edges of the point-segment distance: ~12 VALU instructions per edge.  Only ever used as a KEY.
template <int E>
__device__ __forceinline__ float geo_dist(const DevParams& P, float x, float y) {
  if (P.geo_rect) {                          // wave-uniform: distance to an axis-aligned box, ~8 instructions
    const float dx = fmaxf(fabsf(x - P.rcx) - P.rhx, 0.f), dy = fmaxf(fabsf(y - P.rcy) - P.rhy, 0.f);
    return __builtin_sqrtf(fmaf(dx, dx, dy * dy));
  }
  float best = 3.0e38f;
  bool inside = true;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const float rx = x - P.pvx[e], ry = y - P.pvy[e];
    inside = inside && (fmaf(P.pdy[e], rx, -(P.pdx[e] * ry)) <= 0.f);     // G_e . p - h_e with G_e = (dy, -dx)
    float t = fmaf(rx, P.pdx[e], ry * P.pdy[e]) * P.pil[e];
    t = fminf(fmaxf(t, 0.f), 1.f);
    const float qx = fmaf(-t, P.pdx[e], rx), qy = fmaf(-t, P.pdy[e], ry);
    best = fminf(best, fmaf(qx, qx, qy * qy));
  }
  return inside ? 0.f : __builtin_sqrtf(best);
}

// ---- launch 2: the M nearest of a slice, one wave per slice -----------------------------------------
// GEO = true: the slice's distance keys are computed HERE from the robot polygon (no dune_kernel launch, no key
// buffer): key = closed-form distance g of the point, candidates = every point that the measured bound
// |network distance - g| <= margin[band(g)] cannot exclude from the M nearest (below).  GEO = false: keys read from
// gkeys (dune_kernel: reduced-precision or exact network distances).
// LDS per slice stays < 9 KB at 1000 points so that all (T+1) slices of a CU's scenes are resident.
#define SEL_CAP 64                               // candidates the final exact ranking holds (two 32-point tiles)
template <int E, bool GEO>
// (four waves per SIMD -- 128 VGPRs -- up to six edges; the wider rows of E = 7, 8 spill there and stay at three)
__global__ __attribute__((amdgpu_flat_work_group_size(64, 64), amdgpu_waves_per_eu(E <= 6 ? 4 : 3, E <= 6 ? 4 : 3))) void select_kernel(
    DevParams P, const float* __restrict__ wpack, int n_stride, const float* __restrict__ cur_s,
    const float* __restrict__ points, const float* __restrict__ vel, const int* __restrict__ n_points,
    const int* __restrict__ flags, const unsigned* __restrict__ gkeys, int key_stride,
    float* __restrict__ mu_sorted, float* __restrict__ lam_sorted, float* __restrict__ pts_sorted,
    float* __restrict__ dist_sorted, int* __restrict__ count, int scene0, int t0, int approx_keys, float e0,
    unsigned* __restrict__ stats, const float* __restrict__ trig) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* vec = smem;                       // [11][32]
  float* w6 = vec + 11 * 32;               // [8][32]
  float* b6 = w6 + 8 * 32;                 // [8]
  float* etab = b6 + 8;                    // [NPA_GEO_BANDS] margin per distance band (GEO)
  int* sel = reinterpret_cast<int*>(etab + NPA_GEO_BANDS);   // [SEL_CAP]: the candidates of this slice
  unsigned* skey = reinterpret_cast<unsigned*>(sel + SEL_CAP);   // [NPA_MAX_M] keys of the msel extracted entries
  int* lst = reinterpret_cast<int*>(skey + NPA_MAX_M);        // [64]: short list of the first extraction
  constexpr int ROW_W = E + 5;                                // mu[E], lam[2], point[2], distance
  unsigned* dkey = reinterpret_cast<unsigned*>(lst + 64);     // [n_use] keys; later the candidate list + their exact keys
  // the exact rows of the final candidates take over the key area once the candidates stand in sel[] (the launcher
  // sizes the area for whichever is larger)
  float* rows = reinterpret_cast<float*>(dkey);               // [SEL_CAP][ROW_W]
  unsigned* rkey = reinterpret_cast<unsigned*>(rows + SEL_CAP * (NPA_MAX_E + 5));   // [SEL_CAP][2]: (index, exact key)
  const int t = blockIdx.x + t0, b = blockIdx.y + scene0, lane = threadIdx.x;
  const int j = lane & 31, hf = lane >> 5;
  const int T = P.T, M = P.M;
  if (flags && flags[b * 4 + 0]) return;
  int n_raw = n_points ? n_points[b] : n_stride;
  n_raw = n_raw < 0 ? 0 : (n_raw > n_stride ? n_stride : n_raw);      // the documented contract, enforced
  const int n_use = n_raw < P.dune_max_num ? n_raw : P.dune_max_num;
  const size_t orow = (size_t)b * (T + 1) + t;
  if (n_use <= 0) {
    if (lane == 0) count[orow] = 0;
    return;
  }
  for (int i = lane; i < 11 * 32 + 8 * 32 + 8; i += 64) smem[i] = wpack[WP_VEC16 + i];      // (the 16-point tile's permuted vectors)
  if constexpr (GEO)
    for (int i = lane; i < NPA_GEO_BANDS; i += 64) etab[i] = wpack[WP_GEO + i];
  SliceFrame F;
  load_frame<E>(P, cur_s, trig, b, t, F);
  const float* px_row = points + (size_t)b * 2 * n_stride;
  const float* py_row = px_row + n_stride;
  const float* vx_row = vel ? vel + (size_t)b * 2 * n_stride : nullptr;
  const float* vy_row = vel ? vx_row + n_stride : nullptr;
  if constexpr (GEO) {
    // Keys of every point of the slice.  Four points per lane and trip, their loads issued together: one point per
    // trip made the pass a chain of n_use / 64 dependent memory round trips -- the longest stretch of this wave's life.
    constexpr int KU = 4;
    auto key_of = [&](float gx, float gy, float vx, float vy) -> unsigned {     // the point flow of point_features
      if (vx_row) {
        gx = __fadd_rn(gx, __fmul_rn(F.tstep, __fmul_rn(vx, P.dt32)));
        gy = __fadd_rn(gy, __fmul_rn(F.tstep, __fmul_rn(vy, P.dt32)));
      }
      const float dx = __fsub_rn(gx, F.tx), dy = __fsub_rn(gy, F.ty);
      const float p0x = fmaf(F.c, dx, __fmul_rn(F.s, dy)), p0y = fmaf(F.c, dy, -__fmul_rn(F.s, dx));
      const bool calibrated = fmaxf(fabsf(p0x), fabsf(p0y)) <= P.geo_rcal;     // false for NaN / inf too
      return calibrated ? __float_as_uint(geo_dist<E>(P, p0x, p0y)) : NPA_GEO_KEY_FAR;
    };
    for (int n0 = lane; n0 < n_use; n0 += 64 * KU) {
      float gx[KU], gy[KU], vx[KU], vy[KU];
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const int n = n0 + 64 * u;
        const int src = src_index(n < n_use ? n : n_use - 1, n_raw, n_use);     // (clamped: a valid address, value unused)
        gx[u] = px_row[src]; gy[u] = py_row[src];
        vx[u] = vx_row ? vx_row[src] : 0.f; vy[u] = vy_row ? vy_row[src] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const int n = n0 + 64 * u;
        if (n < n_use) dkey[n] = key_of(gx[u], gy[u], vx[u], vy[u]);
      }
    }
  } else {
    const unsigned* gk = gkeys + orow * key_stride;
    for (int n = lane; n < n_use; n += 64) dkey[n] = gk[n];
  }
  const float w1a = wpack[WP_W116 + lane], w1b = wpack[WP_W116 + 64 + lane];
  const float* wls16 = wpack + WP_WL16;
  WSYNC();

  const int msel = n_use < M ? n_use : M;
  unsigned last_key = 0;
  auto extract = [&]() {                      // the msel smallest (key, index) pairs -> sel[0..msel), skey[0..msel)
    for (int m = 0; m < msel; ++m) {
      unsigned long long best = ~0ull;
      for (int n = lane; n < n_use; n += 64) best = umin64(best, ((unsigned long long)dkey[n] << 32) | (unsigned)n);
      best = wave_min_u64(best);
      const int idx = (int)(best & 0xFFFFFFFFu);
      last_key = (unsigned)(best >> 32);
      if (lane == 0) { sel[m] = idx; skey[m] = last_key; dkey[idx] = 0xFFFFFFFFu; }
      WSYNC();
    }
  };
  // First extraction without msel full passes: the msel-th smallest of the 64 per-lane minima bounds the msel-th
  // smallest key from above (each of those lanes holds a key that small), found by bisection on its bits (one
  // compare + scalar popcount per bit); one more pass lists the keys up to that bound -- msel plus a few for
  // unstructured data -- and the list is ranked in registers.  Long lists (heavy ties) take the plain loop.
  auto extract_short = [&]() -> bool {
    unsigned lmin = 0xFFFFFFFFu;
    for (int n = lane; n < n_use; n += 64) lmin = min(lmin, dkey[n]);
    unsigned bound = 0;
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned trial = bound | ((1u << bit) - 1u);
      if (__popcll(__ballot(lmin <= trial)) < msel) bound |= 1u << bit;
    }
    int L = 0;
    for (int n0 = 0; n0 < n_use; n0 += 64) {
      const int n = n0 + lane;
      const bool hit = n < n_use && dkey[n] <= bound;
      const unsigned long long bal = __ballot(hit);
      const int pos = L + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
      if (hit && pos < 64) lst[pos] = n;
      L += __popcll(bal);
    }
    if (L > 64 || L < msel) return false;
    WSYNC();
    const int idx = lane < L ? lst[lane] : 0;
    const unsigned long long v = lane < L ? (((unsigned long long)dkey[idx] << 32) | (unsigned)idx) : ~0ull;
    int rk = 0;
    for (int i = 0; i < L; ++i) rk += readlane_u64(v, i) < v ? 1 : 0;
    if (lane < L && rk < msel) { sel[rk] = idx; skey[rk] = (unsigned)(v >> 32); dkey[idx] = 0xFFFFFFFFu; }
    const unsigned long long lastb = __ballot(lane < L && rk == msel - 1);
    last_key = (unsigned)(readlane_u64(v, (int)__builtin_ctzll(lastb)) >> 32);
    WSYNC();
    return true;
  };
  if (!extract_short()) extract();
  // The keys decide only WHO is a candidate; the candidates are re-encoded exactly below and ranked on the exact
  // (distance, index) key, so the emitted rows are those of an exact-key selection PROVIDED no true member of the
  // msel nearest is left out:
  //  * network keys (GEO = false, approx_keys): |key - exact| <= e = e0 (1 + |d|), e0 a multiple of the key error
  //    measured for this checkpoint (key_calib_kernel): every point with key <= key_M + 2e is a candidate;
  //  * geometric keys: exact in [g - m(g), g + m(g)], m = margin[band(g)] measured for this checkpoint
  //    (geo_calib_kernel).  U = max over the msel smallest-g points of g + m(g) bounds the msel-th smallest EXACT
  //    distance from above (those msel points all lie below it), so a point with g - m(g) > U cannot be among the
  //    msel nearest.  Points outside the calibrated square (key FAR) are always candidates.
  int ncand = msel, fellback = 0;
  bool widen = false;
  unsigned thr = 0;
  float U = 0.f;
  if constexpr (GEO) {
    widen = n_use > msel;
    float hi = -1.f;
    if (lane < msel) {
      const unsigned k = skey[lane];
      const float g = __uint_as_float(k);
      hi = (k == NPA_GEO_KEY_FAR) ? __builtin_inff() : g + etab[npa_geo_band(g)];
    }
    for (int i = 0; i < msel; ++i) U = fmaxf(U, __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(hi), i)));
  } else {
    widen = approx_keys && msel == M && n_use > M && last_key < 0xFFFFFFFEu;
    if (widen) {
      const float dM = __uint_as_float((last_key & 0x80000000u) ? (last_key & 0x7FFFFFFFu) : ~last_key);
      thr = ordered_key(dM + 2.0f * e0 * (1.0f + fabsf(dM)));
    }
  }
  bool overflow = false, all = false;
  int total = 0, extra = 0;
  if (widen) {
    // compact the indices of the points inside the window IN PLACE over the keys already scanned (slot <= index)
    for (int n0 = 0; n0 < n_use; n0 += 64) {
      const int n = n0 + lane;
      bool hit = false;
      if (n < n_use) {
        const unsigned k = dkey[n];                             // extracted entries are 0xFFFFFFFF
        if constexpr (GEO) {
          const float g = __uint_as_float(k);
          hit = k != 0xFFFFFFFFu && (k == NPA_GEO_KEY_FAR || g - etab[npa_geo_band(g)] <= U);
        } else {
          hit = k <= thr;
        }
      }
      const unsigned long long bal = __ballot(hit);
      const int pos = extra + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
      if (hit) dkey[pos] = (unsigned)n;                         // points besides the msel extracted ones
      extra += __popcll(bal);
    }
    WSYNC();
    if (msel + extra <= SEL_CAP) {                              // the usual case: everything fits the final ranking
      if (lane < extra) sel[msel + lane] = (int)dkey[lane];
      ncand = msel + extra;
      WSYNC();
    } else {
      // more candidates than the final ranking holds (many points within the margin of the M-th nearest: a wall at
      // constant distance, a cluster of exact zeros inside the robot): exact keys for the candidates -- stored behind
      // the list -- or, when the list takes more than half the slice, for the whole slice; then the msel smallest again
      overflow = true;
      fellback = 1;
      all = 2 * extra + msel > n_use;
      total = all ? n_use : msel + extra;
    }
  }
  unsigned* ckey = dkey + extra;                                // [total] exact keys of the candidates (compact form)
  auto cand_index = [&](int q) { return all ? q : (q < msel ? sel[q] : (int)dkey[q - msel]); };
  // Exact re-encoding.  Phase 0 (overflow only): exact KEYS of the long candidate list, then the msel smallest of
  // them become the candidates.  Phase 1: the final candidates (<= SEL_CAP, two tiles at most) with their ROWS
  // parked in LDS; they are ranked on the exact (distance, index) key and the msel nearest are emitted as sorted
  // rows.  ONE call site of the encoder for both (its 65 weight registers + 16 accumulators leave no room for a
  // second inlined copy inside 128 VGPRs).
#pragma unroll 1
  for (int phase = overflow ? 0 : 1;; phase = 1) {
    const int cnt = phase == 0 ? total : ncand;
#pragma unroll 1
    for (int q0 = 0; q0 < cnt; q0 += 16) {                      // (16-point tiles of the exact encoder, weights streamed)
      const int q = q0 + (lane & 15), qc = q < cnt ? q : cnt - 1;
      const int idx = phase == 0 ? cand_index(qc) : sel[qc];
      float mu[E], gx, gy, lx, ly, dist, p0x, p0y;
      point_features_stream16<E>(P, F, w1a, w1b, wls16, vec, w6, b6, px_row, py_row, vx_row, vy_row,
                                 src_index(idx, n_raw, n_use), lane, mu, gx, gy, lx, ly, dist, p0x, p0y);
      if (lane < 16 && q < cnt) {
        const unsigned k = ordered_key(dist);
        if (phase == 0) {
          if (all) dkey[idx] = k;
          else ckey[q] = k;
        } else {
          float* r = rows + q * ROW_W;
#pragma unroll
          for (int e = 0; e < E; ++e) r[e] = mu[e];
          r[E] = lx; r[E + 1] = ly; r[E + 2] = gx; r[E + 3] = gy; r[E + 4] = dist;
          rkey[2 * q] = (unsigned)idx; rkey[2 * q + 1] = k;
        }
      }
    }
    WSYNC();
    if (phase == 1) break;
    if (stats && lane == 0) atomicAdd(stats, (unsigned)((total + 31) / 32));
    if (all) {
      extract();
    } else {
      // the msel smallest exact (key, index) pairs among the candidates; lane m keeps the m-th winner
      int mywin = 0;
      for (int m2 = 0; m2 < msel; ++m2) {
        unsigned long long best = ~0ull;
        int bq = -1;
        for (int q = lane; q < total; q += 64) {
          const unsigned long long v = ((unsigned long long)ckey[q] << 32) | (unsigned)cand_index(q);
          if (v < best) { best = v; bq = q; }
        }
        const unsigned long long win = wave_min_u64(best);
        if (best == win && bq >= 0) ckey[bq] = 0xFFFFFFFFu;     // (key, index) pairs are distinct: one lane retires it
        if (lane == m2) mywin = (int)(win & 0xFFFFFFFFu);
        WSYNC();
      }
      if (lane < msel) sel[lane] = mywin;                       // sel[] was read through cand_index until here
      WSYNC();
    }
    ncand = msel;
  }
  // lane q speaks for candidate q: rank on the exact (distance, index) key, emit; rows >= msel replicate row 0
  const bool mine = lane < ncand;
  const unsigned long long kx = mine ? (((unsigned long long)rkey[2 * lane + 1] << 32) | rkey[2 * lane]) : ~0ull;
  int rank = 0;
  for (int i = 0; i < ncand; ++i) rank += readlane_u64(kx, i) < kx ? 1 : 0;
  if (mine && rank < msel) {
    const float* r = rows + lane * ROW_W;
    auto put = [&](int q) {
      const size_t o = orow * M + q;
#pragma unroll
      for (int e = 0; e < E; ++e) mu_sorted[o * E + e] = r[e];
      lam_sorted[o * 2 + 0] = r[E]; lam_sorted[o * 2 + 1] = r[E + 1];
      pts_sorted[o * 2 + 0] = r[E + 2]; pts_sorted[o * 2 + 1] = r[E + 3];
      dist_sorted[o] = r[E + 4];
    };
    put(rank);
    if (rank == 0)                          // the nearest row also fills rows >= msel: the padding rule of nrmp.py:258-259
      for (int q = msel; q < M; ++q) put(q);
  }
  if (lane == 0) count[orow] = approx_keys == 2 ? (msel | (ncand << 8) | (fellback << 16)) : msel;
}

// ---- launch 2, geometric keys, second form --------------------------------------------------------------------
// Same contract as select_kernel<E, true> (one wave per slice, keys from the closed-form distance g to the robot polygon,
// every point the measured bound |network distance - g| <= margin[band(g)] cannot exclude from the M nearest becomes a
// candidate, candidates re-encoded exactly and ranked on the exact (distance, index) key), built around what the first
// form's instruction census showed:
//  * key pass: strided buffer loads (32-bit offsets + immediates, out-of-range lanes read 0: no 64-bit address
//    arithmetic, no clamping), v_sqrt_f32 instead of the correctly rounded sqrt expansion (the key only nominates), the
//    lane minimum folded in: ~21 VALU instructions per point instead of ~60;
//  * no exact extraction of the M smallest keys: the M-th smallest of the 64 lane minima (bisection) bounds the M-th
//    smallest key, U = max over the lanes at or below it of g + m(g) bounds the M-th smallest EXACT distance, and the
//    per-band rule g - m(band(g)) <= U is folded into ONE threshold g* = max over bands of min(band end, U + m(band)):
//    the window pass is a compare per key, four keys per lane and trip (ds_read_b128);
//  * points at or beyond g_far = (calibrated half extent - robot radius), NaN and inf keys are always candidates;
//  * blockIdx -> (scene, slice) puts all slices of a scene on ONE XCD (workgroup w runs on XCD w % 8): the scene's
//    cloud is fetched into one L2 instead of up to eight;
//  * no register spills (tests/test_abi.py reads the code object).
// Run-time audit of the bound the candidates rest on (the margin is measured, not proven):
//  * every exactly encoded candidate is checked: |exact distance - g| <= margin[band(g)], violations counted;
//  * a hash-selected fraction of the waves (audit_thresh / 2^32) encodes one extra tile of 32 points spread over the slice
//    -- mostly NON-candidates -- and checks the same bound on them;
//  * once the violation counter is non-zero every wave treats ALL points as candidates (exact keys for the whole slice:
//    slow and right) until the host has looked (npa_audit_read) -- a wrong margin cannot keep producing wrong plans;
//  * the violation count is mirrored into pinned host memory (npa_audit_peek: no device synchronisation to poll it).
__device__ __forceinline__ float dpp_f32_b1(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false)); }
__device__ __forceinline__ float wave_max_f32(float v) {
  v = max_nc(v, dpp_f32_b1(v));
  v = max_nc(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false)));
  v = max_nc(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false)));
  v = max_nc(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false)));
  auto rl = [&](int l) { return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), l)); };
  return max_nc(max_nc(rl(0), rl(16)), max_nc(rl(32), rl(48)));
}
// geometric key of a robot-frame point: v_sqrt_f32 (1 ulp) -- nominates only.  RECT: the axis-aligned box form.
// PP: DevParams as the kernels hold it, or DevParams in the kernel-argument segment (geo_key_karg below): one copy of the arithmetic
template <int E, bool RECT, class PP>
__device__ __forceinline__ float geo_key_t(const PP& P, float x, float y) {
  if constexpr (RECT) {
    const float dx = fmaxf(fabsf(x - P.rcx) - P.rhx, 0.f), dy = fmaxf(fabsf(y - P.rcy) - P.rhy, 0.f);
    return __builtin_amdgcn_sqrtf(fmaf(dx, dx, dy * dy));
  } else {
    float best = 3.0e38f;
    bool inside = true;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const float rx = x - P.pvx[e], ry = y - P.pvy[e];
      inside = inside && (fmaf(P.pdy[e], rx, -(P.pdx[e] * ry)) <= 0.f);
      float t = fmaf(rx, P.pdx[e], ry * P.pdy[e]) * P.pil[e];
      t = fminf(fmaxf(t, 0.f), 1.f);
      const float qx = fmaf(-t, P.pdx[e], rx), qy = fmaf(-t, P.pdy[e], ry);
      best = fminf(best, fmaf(qx, qx, qy * qy));
    }
    return inside ? 0.f : __builtin_amdgcn_sqrtf(best);
  }
}
template <int E, class PP>
__device__ __forceinline__ float geo_key(const PP& P, float x, float y) {
  return P.geo_rect ? geo_key_t<E, true>(P, x, y) : geo_key_t<E, false>(P, x, y);
}

// correction of the geometric key from the table behind the weight pack (pan_common.h, WP_TAB): bilinear in the cell of the
// finest level whose square holds the point; ONE 8-byte gather (the cell's four corners as fp16) + ~25 VALU instructions.
// Points outside the largest square take its border cell (their keys are "far": always candidates, whatever this returns).
__device__ __forceinline__ float geo_tab_corr(const float* __restrict__ wpack, float x, float y) {
  const float cx = wpack[WP_TABH], cy = wpack[WP_TABH + 1], h0 = wpack[WP_TABH + 2], inv0 = wpack[WP_TABH + 3];     // (wave-uniform)
  const float rx = x - cx, ry = y - cy;
  const float a = fmaxf(fabsf(rx), fabsf(ry));
  const int lvl = a < h0 ? 0 : (a < 4.0f * h0 ? 1 : (a < 16.0f * h0 ? 2 : 3));
  const float sc = lvl == 0 ? 1.0f : (lvl == 1 ? 4.0f : (lvl == 2 ? 16.0f : 64.0f));
  const float half = h0 * sc, inv = inv0 * (1.0f / sc);
  const float fx = fminf(fmaxf((rx + half) * inv, 0.f), (float)NPA_TAB_N - 0.001f);
  const float fy = fminf(fmaxf((ry + half) * inv, 0.f), (float)NPA_TAB_N - 0.001f);
  const int ix = (int)fx, iy = (int)fy;
  const float tx = fx - (float)ix, ty = fy - (float)iy;
  const uint2 c = reinterpret_cast<const uint2*>(wpack + WP_TAB)[((size_t)lvl * NPA_TAB_N + iy) * NPA_TAB_N + ix];
  typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
  union { unsigned u; h2_t h; } lo, hi;
  lo.u = c.x; hi.u = c.y;                                      // (f(ix, iy), f(ix+1, iy)) , (f(ix, iy+1), f(ix+1, iy+1))
  const float f00 = (float)lo.h[0], f10 = (float)lo.h[1], f01 = (float)hi.h[0], f11 = (float)hi.h[1];
  const float r0 = fmaf(tx, f10 - f00, f00), r1 = fmaf(tx, f11 - f01, f01);
  return fmaf(ty, r1 - r0, r0);
}

#define SEL2_TRIP 256                            // points per trip of the key pass (4 per lane)
// key pass of select_geo_kernel: dkey[n] = bits of g(point n) (0xFFFFFFFF behind the slice's end); returns the lane's
// smallest key.  The wave-uniform cases (box or polygon, moving points, decimation) are template parameters: inside
// the loop they were branches on spilled scalars plus both arms of the point flow.
template <int E, bool RECT, bool VEL, bool DEC>
__device__ __forceinline__ unsigned key_pass(const DevParams& P, const SliceFrame& F, const float* px_row, const float* py_row,
                                             const float* vx_row, const float* vy_row, unsigned* dkey, int n_raw, int n_use,
                                             int n_pad, int lane) {
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(px_row), 0, n_raw * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(py_row), 0, n_raw * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t rvx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(VEL ? vx_row : px_row), 0, n_raw * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t rvy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(VEL ? vy_row : py_row), 0, n_raw * 4, 0x00020000);
  const float tdt = F.tstep;
  unsigned lmin = 0xFFFFFFFFu;
  for (int n0 = 0; n0 < n_pad; n0 += SEL2_TRIP) {
    float gx[4], gy[4], vx[4], vy[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int n = n0 + lane + 64 * u;
      unsigned off = (unsigned)n * 4u;                 // (reads behind n_raw return 0: the key is discarded below)
      if constexpr (DEC) off = (unsigned)src_index(n < n_use ? n : n_use - 1, n_raw, n_use) * 4u;
      gx[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, off, 0, 0));
      gy[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ry, off, 0, 0));
      if constexpr (VEL) {
        vx[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rvx, off, 0, 0));
        vy[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rvy, off, 0, 0));
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int n = n0 + lane + 64 * u;
      float x = gx[u], y = gy[u];
      if constexpr (VEL) {      // pan.py:182 (the reference's rounding order: the kept rows recompute it the same way)
        x = __fadd_rn(x, __fmul_rn(tdt, __fmul_rn(vx[u], P.dt32)));
        y = __fadd_rn(y, __fmul_rn(tdt, __fmul_rn(vy[u], P.dt32)));
      }
      const float dx = x - F.tx, dy = y - F.ty;
      const float p0x = fmaf(F.c, dx, F.s * dy), p0y = fmaf(F.c, dy, -(F.s * dx));
      unsigned k = __float_as_uint(geo_key_t<E, RECT>(P, p0x, p0y));
      k = n < n_use ? k : 0xFFFFFFFFu;
      dkey[n] = k;
      lmin = min(lmin, k);
    }
  }
  return lmin;
}

// (select_geo_body.inc, the stage loop)
#define SEL_OPAQUE_V(x) asm volatile("" : "+v"(x))
#define SEL_OPAQUE_S(x) do { (x) = __builtin_amdgcn_readfirstlane(x); asm volatile("" : "+s"(x)); } while (0)   // (x is wave-uniform)
#define SEL_LDS_FRAME (6 * NPA_MAX_E)              // floats of the frame's image in LDS (select_geo_carve.inc; the launchers size it)
// the stage loop's wave-uniform switches, bits of the scalar `st`
// (ST_FIRST / ST_SECOND: the list of 17-32 that encodes its 16 nearest-by-g first -- pending / its survivors' tile is running)
enum { ST_OVERFLOW = 1, ST_ALL = 2, ST_USE16 = 4, ST_USET = 8, ST_AUD16 = 16, ST_AUDIT_WAVE = 32, ST_HAS_AUDIT = 64, ST_DISTRUST = 128,
       ST_FIRST = 256, ST_SECOND = 512 };
#define ST_IS(f) ((st & (unsigned)(f)) != 0u)
#define ST_PUT(f, v) (st = (v) ? (st | (unsigned)(f)) : (st & ~(unsigned)(f)))
#define SEL2_TRIP 256                            // points per trip of the key pass (4 per lane)
// -DNPA_SEL_PROF: s_memtime stamps between the phases of a wave, summed over all waves in npa_sel_prof[] (slot 15 counts
// the waves); tests/tools/select_phase_cycles.py builds that variant next to the product library and reads it back
#ifdef NPA_SEL_PROF
#define SELP_WAVES 4096
__device__ unsigned long long npa_sel_prof[SELP_WAVES][16];     // one row per workgroup index: no atomics, nothing shared between waves
extern "C" int npa_dbg_sel_prof(unsigned long long* out16, int reset) {
  static unsigned long long host[SELP_WAVES][16];
  if (out16) {
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(npa_sel_prof), sizeof(host)) != hipSuccess) return -1;
    for (int i = 0; i < 16; ++i) { out16[i] = 0; for (int w = 0; w < SELP_WAVES; ++w) out16[i] += host[w][i]; }
  }
  if (reset) {
    memset(host, 0, sizeof(host));
    if (hipMemcpyToSymbol(HIP_SYMBOL(npa_sel_prof), host, sizeof(host)) != hipSuccess) return -1;
  }
  return 0;
}
#define SELP_DECL unsigned long long spt_ = __builtin_amdgcn_s_memtime(), sacc_[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; const unsigned long long sp0_ = spt_
#define SELP(i) do { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); sacc_[i] += n_ - spt_; spt_ = n_; } while (0)
#else
#define SELP_DECL
#define SELP(i)
#endif
// ---- the kernel-argument segment, read by hand --------------------------------------------------------------------------
// What a wave needs of its arguments only at the END (the five output pointers, the statistics and audit counters) the compiler
// loads at the top with everything else and carries through the kernel: about a dozen 64-bit scalars parked in VGPR lanes and
// fetched back with v_readlane at the emit.  The body therefore takes them out of the argument segment itself, through a base
// pointer that passed an empty asm (the loads can neither be merged with the preamble's nor hoisted), one phase ahead of their
// use.  The pointer stays a pointer to the constant address space throughout: the loads are s_load_dword*.
// SelGeoArgs mirrors the parameter list of select_geo_kernel (arguments sit in the segment in order, each at its natural
// alignment: the layout of a struct); the group kernel's per-call block is SelGeoCall (pan_common.h) at G.c[blockIdx.y].
#define NPA_KARG __attribute__((address_space(4)))
#define NPA_GLOBAL __attribute__((address_space(1)))
typedef const char NPA_KARG* karg_ptr;
struct SelGeoArgs {
  DevParams P; const float* wpack; int n_stride; const float* cur_s; const float* points; const float* vel; const int* n_points;
  const int* flags; float* mu_sorted; float* lam_sorted; float* pts_sorted; float* dist_sorted; int* count; int scene0, t0, nsl,
  nscene, debug; unsigned* stats; const float* trig; unsigned* audit; unsigned audit_thresh, audit_seed; float margin_scale;
};
struct SelGeoGroupArgs { DevParams P; SelGeoGroup G; int t0, nsl, nscene, debug; unsigned audit_thresh; float margin_scale; };
struct SelOutPtrs { float* mu; float* lam; float* pts; float* dist; int* count; };      // (consecutive in both layouts)
static_assert(offsetof(SelGeoArgs, count) - offsetof(SelGeoArgs, mu_sorted) == 32 && offsetof(SelGeoCall, count) - offsetof(SelGeoCall, mu_sorted) == 32,
              "SelOutPtrs is read as one block");
// (what the compiler lays out for the two parameter lists on gfx950, read from the kernels' metadata; a parameter added to or
// moved in a kernel's list without its mirror fails here or at the offsets below)
static_assert(sizeof(DevParams) == 0x1a8 && offsetof(SelGeoArgs, wpack) == sizeof(DevParams) && offsetof(SelGeoGroupArgs, G) == sizeof(DevParams),
              "DevParams is the first argument of both kernels");
static_assert(sizeof(SelGeoCall) == 0x78 && sizeof(SelGeoGroupArgs) == 0x1a8 + 8 * 0x78 + 24 && offsetof(SelGeoGroupArgs, debug) == 0x1a8 + 8 * 0x78 + 12,
              "SelGeoGroupArgs mirrors select_geo_group_kernel(P, G, t0, nsl, nscene, debug, audit_thresh, margin_scale)");
static_assert(offsetof(SelGeoArgs, mu_sorted) == 0x1a8 + 0x38 && offsetof(SelGeoArgs, debug) == 0x1a8 + 0x70 && offsetof(SelGeoArgs, stats) == 0x1a8 + 0x78 &&
              offsetof(SelGeoArgs, audit) == 0x1a8 + 0x88 && sizeof(SelGeoArgs) == 0x1a8 + 0xa0,
              "SelGeoArgs mirrors the parameter list of select_geo_kernel");
__device__ __forceinline__ karg_ptr karg_fence(karg_ptr p) { asm volatile("" : "+s"(p)); return p; }
template <class T>
__device__ __forceinline__ T karg_load(karg_ptr p, size_t off) { return *reinterpret_cast<const T NPA_KARG*>(p + off); }
// SEL_KARG(member): the argument `member` of this wave's call, fetched now
#define SEL_KARG(T_, member) karg_load<T_>(SEL_KARGS_LATE(), SEL_KARG_OFF(member))
// geo_key with the polygon read from the kernel-argument segment (DevParams is the first argument of both kernels) through a
// fenced base: inside the stage loop.  Read through `P`, the twenty-odd dwords of the general polygon (pvy ... pil, loop-invariant
// scalar loads) were fetched in front of the loop and held through it, on a box robot that never takes that branch.
template <int E>
__device__ __forceinline__ float geo_key_karg(karg_ptr kbase, float x, float y) {
  return geo_key<E>(*reinterpret_cast<const DevParams NPA_KARG*>(karg_fence(kbase)), x, y);
}

// (SelGeoArgs above MUST follow this parameter list, member for member: the body reads some arguments through it)
template <int E, bool BF16 = false, bool KEYS16 = false>
__global__ __attribute__((amdgpu_flat_work_group_size(64, 64), amdgpu_waves_per_eu(E <= 6 ? 4 : 3, E <= 6 ? 4 : 3))) void select_geo_kernel(
    DevParams P, const float* __restrict__ wpack, int n_stride, const float* __restrict__ cur_s,
    const float* __restrict__ points, const float* __restrict__ vel, const int* __restrict__ n_points,
    const int* __restrict__ flags, float* __restrict__ mu_sorted_, float* __restrict__ lam_sorted_,
    float* __restrict__ pts_sorted_, float* __restrict__ dist_sorted_, int* __restrict__ count_, int scene0, int t0, int nsl,
    int nscene, int debug, unsigned* __restrict__ stats_, const float* __restrict__ trig, unsigned* __restrict__ audit,
    unsigned audit_thresh, unsigned audit_seed, float margin_scale) {
  // (the arguments with a trailing underscore are read by SEL_KARG where the body needs them, not here)
#define SEL_KARG_OFF(member) offsetof(SelGeoArgs, member)
#define SEL_KBASE_OFF(member) offsetof(SelGeoArgs, member)
  const karg_ptr sel_kbase = (karg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
#define SEL_KARGS_LATE() karg_fence(sel_kbase)
#define SEL_KOFF_STORE()
#define SEL_KOFF() 0
#include "select_geo_carve.inc"
  int lane = threadIdx.x;
  SELP_DECL;
  // workgroup w runs on XCD w % 8 (observed dispatch order; a speed assumption only): scene = 8 * (w / (8 nsl)) + w % 8
  const int w = blockIdx.x, xcd = w & 7, r_ = w >> 3;
  const int bl = (r_ / nsl) * 8 + xcd;
  if (bl >= nscene) return;
  const int t = r_ % nsl + t0, b = bl + scene0;
#include "select_geo_body.inc"
#undef SEL_KARG_OFF
#undef SEL_KBASE_OFF
#undef SEL_KARGS_LATE
#undef SEL_KOFF_STORE
#undef SEL_KOFF
}

// select_geo_kernel over a GROUP of forward calls (pan_common.h: merged launches): blockIdx.y = the call, blockIdx.x what it
// is above; the per-call pointers come out of the kernel arguments, everything else is the same statements.
// (SelGeoGroupArgs above MUST follow this parameter list)
template <int E, bool BF16 = false, bool KEYS16 = false>
__global__ __attribute__((amdgpu_flat_work_group_size(64, 64), amdgpu_waves_per_eu(E <= 6 ? 4 : 3, E <= 6 ? 4 : 3))) void select_geo_group_kernel(
    DevParams P, SelGeoGroup G, int t0, int nsl, int nscene, int debug, unsigned audit_thresh, float margin_scale) {
#define SEL_KARG_OFF(member) offsetof(SelGeoCall, member)
#define SEL_KBASE_OFF(member) offsetof(SelGeoGroupArgs, member)
  const karg_ptr sel_kbase = (karg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
  const int sel_koff = (int)offsetof(SelGeoGroupArgs, G) + (int)blockIdx.y * (int)sizeof(SelGeoCall);
  const karg_ptr sel_kargs = sel_kbase + sel_koff;
  // (behind the preamble the call's block is found again through its OFFSET, parked in the frame's LDS image by the body: the
  // 64-bit base held to the emit was the one pair the merged kernel had to park more than the single-call one)
#define SEL_KARGS_LATE() (karg_fence(sel_kbase) + __builtin_amdgcn_readfirstlane(__float_as_int(frg[5 * NPA_MAX_E + 7])))
#define SEL_KOFF_STORE() do { if (threadIdx.x == 0) frg[5 * NPA_MAX_E + 7] = __int_as_float(sel_koff); } while (0)
#define SEL_KOFF() sel_koff
  // (field by field: `G.c[blockIdx.y]` as a whole came in as two 16- and 8-dword loads and was parked as such)
  const float* __restrict__ wpack = karg_load<const float*>(sel_kargs, SEL_KARG_OFF(wpack));
  const float* __restrict__ cur_s = karg_load<const float*>(sel_kargs, SEL_KARG_OFF(cur_s));
  const float* __restrict__ points = karg_load<const float*>(sel_kargs, SEL_KARG_OFF(points));
  const float* __restrict__ vel = karg_load<const float*>(sel_kargs, SEL_KARG_OFF(vel));
  const int* __restrict__ n_points = karg_load<const int*>(sel_kargs, SEL_KARG_OFF(n_points));
  const int* __restrict__ flags = karg_load<const int*>(sel_kargs, SEL_KARG_OFF(flags));
  const float* __restrict__ trig = karg_load<const float*>(sel_kargs, SEL_KARG_OFF(trig));
  unsigned* __restrict__ audit = karg_load<unsigned*>(sel_kargs, SEL_KARG_OFF(audit));
  const int n_stride = karg_load<int>(sel_kargs, SEL_KARG_OFF(n_stride));
  unsigned audit_seed = karg_load<unsigned>(sel_kargs, SEL_KARG_OFF(audit_seed));
#include "select_geo_carve.inc"
  int lane = threadIdx.x;
  SELP_DECL;
  const int w = blockIdx.x, xcd = w & 7, r_ = w >> 3;
  const int bl = (r_ / nsl) * 8 + xcd;
  if (bl >= nscene) return;
  const int t = r_ % nsl + t0, b = bl;
#include "select_geo_body.inc"
#undef SEL_KARG_OFF
#undef SEL_KBASE_OFF
#undef SEL_KARGS_LATE
#undef SEL_KOFF_STORE
#undef SEL_KOFF
}
