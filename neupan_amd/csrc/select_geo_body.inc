// select_geo_body.inc -- the BODY of the geometric selection for ONE slice (scene b, horizon step t) on one wave, as
// statements: included by select_geo_kernel and select_geo_group_kernel (dune_device.h: workgroup -> (scene, slice) / (call,
// scene, slice)).  Textual for the same reason as nrmp_qp_body.inc: the kernel's
// token stream, hence its machine code, stays what the counter records were measured on.  Expects in scope: the kernel's
// parameters, the carve of select_geo_carve.inc, `lane`, `b`, `t`, `sel_kbase` and the SEL_K* macros (dune_device.h: the argument segment).
  const int T = P.T, M = P.M;
  // the exact encoder's tile, chosen PER TRIP on the exact-rows instantiation: 16 points (v_mfma_f32_16x16x4_f32, dune_device.h)
  // when at most 16 are left -- candidate lists carry a median of 14-19 points: half of a 32-point tile was padding --, 32 points
  // (v_mfma_f32_32x32x2_f32) otherwise: a long list's fixed work per tile (point loads, frame, weight stream) is paid once per 32.
  // Both shapes give bitwise the same rows (same fma chains in the same K order, canonical reductions) and read ONE image of the
  // vectors in LDS (the permuted one, WP_VEC16).  The bf16 instantiations keep the 32-point tile and the natural image.
  constexpr bool TILE16 = !BF16 && !KEYS16;
  if (flags && flags[b * 4 + 0]) return;
  int n_raw = n_points ? n_points[b] : n_stride;
  n_raw = n_raw < 0 ? 0 : (n_raw > n_stride ? n_stride : n_raw);
  int n_use = n_raw < P.dune_max_num ? n_raw : P.dune_max_num;
  // the output row (scenes x slices: far below 2^31), computed on the VECTOR side from a scene number behind an empty asm: the
  // early exit below and the emit (through LDS) use it; as a scalar it -- and T, b, t with it -- was parked from here to the
  // early exit's block, which the compiler lays out at the kernel's end
  int orow_v = b;
  asm volatile("" : "+v"(orow_v));
  orow_v = orow_v * (T + 1) + t;
  int koff_v = SEL_KOFF();                               // (likewise: where this call's arguments start, for the early exit)
  asm volatile("" : "+v"(koff_v));
  if (n_use <= 0) {
    if (lane == 0) ((int NPA_GLOBAL*)karg_load<int*>(karg_fence(sel_kbase) + __builtin_amdgcn_readfirstlane(koff_v), SEL_KARG_OFF(count)))[orow_v] = 0;
    return;
  }
  // the preamble's loads as ONE batch (written as loops they compiled to a load -> wait -> LDS write per trip: twelve global
  // round trips in series, 18 % of a wave's life -- profiles/r04_select_phase_cycles.txt)
  constexpr int NVEC = 11 * 32 + 8 * 32 + 8, NVT = (NVEC + 63) / 64, NGT = (NPA_GEO_BANDS + 63) / 64;
  float pre_v[NVT], pre_g[NGT];
#pragma unroll
  for (int i = 0; i < NVT; ++i) { const int k = lane + 64 * i; pre_v[i] = wpack[(TILE16 ? WP_VEC16 : WP_VEC) + (k < NVEC ? k : NVEC - 1)]; }
#pragma unroll
  for (int i = 0; i < NGT; ++i) { const int k = lane + 64 * i; pre_g[i] = wpack[WP_GEO + (k < NPA_GEO_BANDS ? k : NPA_GEO_BANDS - 1)]; }
  unsigned aud_viol = 0, aud_launches = 0;
  if (audit) {
    aud_viol = __hip_atomic_load(audit + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    aud_launches = __hip_atomic_load(audit + 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const float w1 = wpack[WP_W1 + lane];
  const float w1a = TILE16 ? wpack[WP_W116 + lane] : 0.f, w1b = TILE16 ? wpack[WP_W116 + 64 + lane] : 0.f;
  SliceFrame F;
  load_frame<E, true>(P, cur_s, trig, b, t, F, frg);        // (F.rg: in LDS, read by the row epilogue below)
  if (lane == 0) frg[5 * NPA_MAX_E + 5] = __int_as_float(orow_v);      // (read back at the emit)
  SEL_KOFF_STORE();
  const float* px_row = points + (size_t)b * 2 * n_stride;
  const float* vx_row = vel ? vel + (size_t)b * 2 * n_stride : nullptr;
  const bool has_vel = vel != nullptr, decim = n_use < n_raw;
  // (the audit block's pointer is used here and in the audit-wave hash below; the counters at the end fetch it again)
  const bool has_audit = audit != nullptr;             // (ST_HAS_AUDIT / ST_DISTRUST of `st` inside the stage loop)
  // a violation seen by an earlier launch (or an earlier wave of this one): everything is a candidate from here on
  const bool distrust = has_audit && __builtin_amdgcn_readfirstlane((int)aud_viol) != 0;
  // a polygon that is not an axis-aligned box: the key pass ranks on the distance to its BOUNDING BOX (a lower bound of g, 8
  // instructions instead of 12 per edge: at 8 edges and 5000 points the pass was most of this kernel), g <= key + S
  const float boxS = (P.geo_rect && E == 4) ? 0.f : __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(wpack[WP_TABH + 4])));
  const unsigned far_thr = __float_as_uint(fmaxf(P.geo_far - boxS, 0.f));
  SELP(0);

  // ---- key pass: dkey[n] = bits of g(point n) (0xFFFFFFFF behind the slice's end), lane minimum on the way ----------
  const int n_pad = (n_use + SEL2_TRIP - 1) & ~(SEL2_TRIP - 1);
  unsigned lmin;
#define KP(R_, V_, D_) \
  lmin = key_pass<E, R_, V_, D_>(P, F, px_row, px_row + n_stride, vx_row, vx_row ? vx_row + n_stride : nullptr, dkey, n_raw, n_use, n_pad, lane)
  if (has_vel) { if (decim) KP(true, true, true); else KP(true, true, false); }
  else { if (decim) KP(true, false, true); else KP(true, false, false); }
#undef KP
  // the vectors and margins requested in the preamble land in LDS only now: their round trip ran behind the key pass (the
  // counter of outstanding loads retires in order, so the pass's own first wait covered them) instead of in front of it
#pragma unroll
  for (int i = 0; i < NVT; ++i) { const int k = lane + 64 * i; if (k < NVEC) smem[k] = pre_v[i]; }
#pragma unroll
  for (int i = 0; i < NGT; ++i) { const int k = lane + 64 * i; if (k < NPA_GEO_BANDS) etab[k] = pre_g[i] * margin_scale; }
  const float* wls = wpack + (BF16 ? WP_WB16 : WP_WLS);
  const float* wls16 = wpack + WP_WL16;
  WSYNC();
  SELP(1);

  int msel = n_use < M ? n_use : M;
  // msel-th smallest of the 64 lane minima: an upper bound of the msel-th smallest key (each of those lanes holds a key
  // that small; consecutive points sit in different lanes, so a run of near points -- a scan of one obstacle -- does not
  // loosen it).  Fewer than msel lanes with a point (tiny slices): the bound is 0xFFFFFFFF and everything is a candidate.
  // (round 6: the search stops twelve bits short and fills them with ones -- still an upper bound of the msel-th smallest key, looser by
  // at most 5e-4 of the key, a millimetre at two metres against margins of centimetres: a lane or two more may nominate, the
  // candidates stay a superset.  Each step is six DEPENDENT instructions across the vector / scalar boundary, ~85 cycles: pure latency.)
  unsigned bound = 0;
  for (int bit = 31; bit >= 12; --bit) {
    const unsigned trial = bound | ((1u << bit) - 1u);
    if (__popcll(__ballot(lmin <= trial)) < msel) bound |= 1u << bit;
  }
  bound |= 0xFFFu;
  float hi = 0.f;
  if (lmin <= bound) {
    const float g = __uint_as_float(lmin);
    if (lmin >= far_thr) hi = __builtin_inff();                                   // (NaN keys are >= far_thr as bits)
    else {
      // the point's g lies in [key, key + S]: the largest margin over the bands of that range (one band for a box)
      float mm = 0.f;
      for (int bb = npa_geo_band(g), be = npa_geo_band(g + boxS); bb <= be; ++bb) mm = max_nc(mm, etab[bb]);
      hi = g + boxS + mm;
    }
  }
  const float U = wave_max_f32(hi);
  // one threshold for the window: a point of band b is a candidate iff g <= U + m[b]; g* = the largest such g over the
  // bands below g_far (a superset of the per-band rule: a band's points between U + m[b] and g* come along)
  unsigned thr = 0xFFFFFFFEu;
  if (!distrust && U < 3.0e38f) {
    float gs = 0.f;
#pragma unroll
    for (int rep = 0; rep < 2; ++rep) {
      const int bnd = lane + 64 * rep;
      if (bnd < NPA_GEO_BANDS) {
        const float lo_b = __uint_as_float((unsigned)(bnd + (0x3E800000u >> 20)) << 20) - 0.25f;
        const float hi_b = bnd == NPA_GEO_BANDS - 1 ? P.geo_far : __uint_as_float((unsigned)(bnd + 1 + (0x3E800000u >> 20)) << 20) - 0.25f;
        const float reach = U + etab[bnd];
        if (lo_b < P.geo_far && lo_b <= reach) gs = max_nc(gs, min_nc(hi_b, reach));
      }
    }
    gs = wave_max_f32(gs);
    thr = gs < 3.0e38f ? __float_as_uint(gs) : 0xFFFFFFFEu;
  }
  SELP(2);
  // ---- window pass: indices of the candidates, compacted IN PLACE over the keys already scanned ----------------------
  int ntot = 0;
  for (int n0 = 0; n0 < n_pad; n0 += SEL2_TRIP) {
    const uint4 k4 = *reinterpret_cast<const uint4*>(dkey + n0 + 4 * lane);
    const unsigned kk[4] = {k4.x, k4.y, k4.z, k4.w};
    bool hit[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) hit[u] = kk[u] <= thr || (kk[u] - far_thr) < (0xFFFFFFFFu - far_thr);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned long long bal = __ballot(hit[u]);
      const int pos = ntot + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
      if (hit[u]) dkey[pos] = (unsigned)(n0 + 4 * lane + u);
      ntot += __popcll(bal);
    }
  }
  WSYNC();
  SELP(3);
  int ncand = ntot, fellback = 0;
  // the wave-uniform switches of the stage loop as BITS of one scalar (as bools each was a 64-bit lane mask, parked and fetched back)
  unsigned st = (has_audit ? (unsigned)ST_HAS_AUDIT : 0u) | (distrust ? (unsigned)ST_DISTRUST : 0u);
  int total = 0;
  if (ntot <= SEL_CAP && ntot >= msel) {
    if (lane < ntot) sel[lane] = (int)dkey[lane];
    WSYNC();
  } else if (ntot < msel) {
    // cannot happen while the threshold covers the nominating lanes' own minima (it does, by construction); if it ever
    // did, exact keys for the whole slice are the answer, not fewer rows than promised
    ST_PUT(ST_OVERFLOW, true); fellback = 1; ST_PUT(ST_ALL, true); total = n_use;
  } else {
    // more candidates than the final ranking holds (a wall at constant distance, a blob inside the robot, a distrusted
    // margin): exact keys for the list -- stored behind it -- or, when it takes more than half the slice, for every point
    ST_PUT(ST_OVERFLOW, true);
    fellback = 1;
    ST_PUT(ST_ALL, 2 * ntot > n_use);
    total = ST_IS(ST_ALL) ? n_use : ntot;
  }
  unsigned* ckey = dkey + ntot;
  auto cand_index = [&](int q) { return ST_IS(ST_ALL) ? q : (int)dkey[q]; };
  auto extract = [&]() {                      // the msel smallest (key, index) pairs of dkey[0..n_use) -> sel[0..msel)
    for (int m = 0; m < msel; ++m) {
      unsigned long long best = ~0ull;
      for (int n = lane; n < n_use; n += 64) best = umin64(best, ((unsigned long long)dkey[n] << 32) | (unsigned)n);
      best = wave_min_u64(best);
      const int idx = (int)(best & 0xFFFFFFFFu);
      if (lane == 0) { sel[m] = idx; skey[m] = (unsigned)(best >> 32); dkey[idx] = 0xFFFFFFFFu; }
      WSYNC();
    }
  };
  // which waves run the extra audit tile: a hash of (launch, scene, slice).  The launch number is the host's sequence
  // number plus a device-side count of launches (audit[4], bumped by workgroup 0): a launch replayed from a HIP graph
  // carries a frozen host number, and should still audit other waves and other points each time
  if (audit && audit_thresh) {
    audit_seed += (unsigned)__builtin_amdgcn_readfirstlane((int)aud_launches);
    if (blockIdx.x == 0 && lane == 0) atomicAdd(audit + 4, 1u);
    unsigned hsh = (audit_seed * 0x9E3779B1u) ^ ((unsigned)b * 0x85EBCA77u) ^ ((unsigned)t * 0xC2B2AE3Du);
    hsh ^= hsh >> 15; hsh *= 0x2C1B3C6Du; hsh ^= hsh >> 12; hsh *= 0x297A2D39u; hsh ^= hsh >> 15;
    ST_PUT(ST_AUDIT_WAVE, hsh < audit_thresh || audit_thresh == 0xFFFFFFFFu);
    if (lane == 0) frg[5 * NPA_MAX_E + 6] = __uint_as_float(audit_seed + (unsigned)t);     // the audit tile's phase (stage 2, behind stage 1's barriers)
  }
  // Stage 0 (overflow only): exact KEYS of the long list, the msel smallest become the candidates.  Stage 1: the final
  // candidates (<= SEL_CAP) with their ROWS parked in LDS, ranked and emitted.  Stage 2 (audit waves): 32 points spread
  // over the slice, bound check only.  ONE call site of the encoder for all three.
  // KEYS16 (the bf16 KEY tier, NPA_KEYS_PRECISION=bf16): stage 0 runs the list through the bf16-MFMA encoder instead; every
  // point whose bf16 distance lies within 2 x m16 of the msel-th smallest one survives (m16 = measured |bf16 - exact| for the
  // band, x safety: a true member's exact distance is <= the msel-th smallest bf16 distance + m16, its own bf16 distance at
  // most m16 above that), the survivors are re-encoded EXACTLY and ranked on exact keys -- the rows are bitwise those of the
  // exact-key selection -- and every survivor's |exact - bf16| is checked against m16 (a violation is counted like one of the
  // geometric margin: the handle then distrusts both).  More survivors than the ranking holds: stage 0 again, exact.
  int viol = 0;
  float worst = 0.f;
  // (a list of up to four tiles goes straight to the exact encoder: the filter costs a bf16 pass plus the survivors' exact one)
  ST_PUT(ST_USE16, KEYS16 && ST_IS(ST_OVERFLOW) && !ST_IS(ST_ALL) && !ST_IS(ST_DISTRUST) && total > 128);
  // TABF (the default instantiation, when the handle carries the table: P.geo_tab): the same filter with the TABLE-corrected
  // geometric key g(p) + f_table(p) (dune_device.h, geo_tab_corr) in place of an encoder pass -- 64 list entries per trip at ~60
  // VALU instructions and two gathers, against 32 per ~16 k-cycle encoder tile; its error is what bilinear interpolation of the
  // smooth f leaves (millimetres; measured per band at creation, WP_KTAB), so a dense cloud's list of hundreds shrinks to the
  // ten-odd points that really compete for rank M, and those alone are encoded exactly.  It also runs on lists that do not
  // overflow but need a second encoder tile (more than 32 candidates).  Survivors are audited like the bf16 tier's.
  constexpr bool TABF = !BF16 && !KEYS16 && (E == 4 || E == 8);      // (the polygon sizes of the benchmark configurations)
  ST_PUT(ST_USET, TABF && P.geo_tab != 0 && !ST_IS(ST_DISTRUST) && ntot >= msel && (ST_IS(ST_OVERFLOW) || ntot > 32));
  if (ST_IS(ST_USET) && !ST_IS(ST_OVERFLOW)) total = ntot;       // (the list stands in dkey[0 .. ntot); sel[] is rebuilt from the survivors)
  ST_PUT(ST_AUD16, false);                                            // stage 1 checks every survivor's |exact - filter key| against m16
  float m16 = 0.f;
  // TABF, a list of 17-32 (two thirds of the flagship's slices): ONE 16-point tile first, the rest bounded by what it found.
  // Stage 0 takes every candidate's table key as it does for the filter (one lane each, one trip) and with it the geometric key
  // and the table key's LOWER bound tk - m_table[band(tk)]; the list is ordered by geometric key -- the keys broadcast out of
  // LDS, a rank of 32 subtractions per lane, no lane moves --, and its 16 smallest are encoded exactly (stage 1, first trip).  The
  // msel-th smallest EXACT distance among them, dM, bounds the msel-th smallest distance of the slice from above: these are 16
  // points of the slice and msel <= 16.  A candidate behind the first 16 whose lower bound lies strictly above dM has exact >=
  // that bound > dM: it is not among the msel nearest and cannot tie into them; it is dropped.  The others (mostly none) are
  // encoded in a second 16-point tile and audited like the filter's survivors.  Any superset of the true msel nearest, ranked
  // on the exact (distance, index) key, emits the same rows: WHICH 16 points come first decides the cost alone.
  // (Such a list never overflows: 17 <= ntot <= 32 <= SEL_CAP and msel <= 16 < ntot put it in the first arm of the decision above,
  // ST_OVERFLOW clear, sel[] filled; ranks below 32 index sel[], s16[] and skey[], which hold SEL_CAP, SEL_CAP and NPA_MAX_M words.
  // Audit waves never take this path, so ST_SECOND -- set for the survivors' tile and left set to the wave's end, where it moves
  // the start of the tile loop -- is never set when stage 2 runs.)
  static_assert(SEL_CAP >= 32 && NPA_MAX_M >= 32, "the first-tile path ranks up to 32 candidates into sel[], s16[] and skey[]");
  if constexpr (TABF) {
    if ((P.geo_tab & NPA_GEO_TAB_FIRST_TILE) != 0 && !ST_IS(ST_DISTRUST) && !ST_IS(ST_AUDIT_WAVE) && msel <= 16 && ntot > 16 && ntot <= 32) {
      ST_PUT(ST_FIRST, true);
      total = ntot;                                                      // (the list stands in dkey[0 .. ntot), as for the filter)
    }
  }
  SELP(4);
#pragma unroll 1
  for (int stage = (ST_IS(ST_OVERFLOW) || ST_IS(ST_USET) || ST_IS(ST_FIRST)) ? 0 : 1;;) {
    // What the stages derive from the lane number and the slice's sizes (compare masks, clamped counts, the decimation step, the
    // audit tile's stride: most of it for the rare stages) is loop-invariant, so the compiler computed ALL of it in front of this
    // loop and parked it in VGPR lanes: ~100 v_writelane per wave, whichever stage ran.  Behind an empty asm the values are
    // this trip's own: each is derived where it is used.  (Integers only: a pointer through an asm loses its address space.)
    SEL_OPAQUE_V(lane); SEL_OPAQUE_S(n_use); SEL_OPAQUE_S(n_raw); SEL_OPAQUE_S(msel);
    const int cnt = stage == 0 ? total : (stage == 1 ? ncand : (n_use < 32 ? n_use : 32));
    if (TABF && stage == 0 && (ST_IS(ST_USET) || ST_IS(ST_FIRST))) {
      unsigned* fk = ST_IS(ST_ALL) ? dkey : ckey;
      const bool first = (__builtin_amdgcn_readfirstlane((int)st) & ST_FIRST) != 0;      // (a scalar branch, not a lane mask)
#pragma unroll 1
      for (int q0 = 0; q0 < cnt; q0 += 64) {
        const int q = q0 + lane, qc = q < cnt ? q : cnt - 1;
        const int iq = cand_index(qc);
        const int src = src_index(iq, n_raw, n_use);
        SliceFrame Fl;      // (the frame out of LDS, per trip: the key pass's scalars are dead by now, and held across the encoder these are five registers)
        Fl.c = frg[5 * NPA_MAX_E + 0]; Fl.s = frg[5 * NPA_MAX_E + 1];
        Fl.tx = frg[5 * NPA_MAX_E + 2]; Fl.ty = frg[5 * NPA_MAX_E + 3]; Fl.tstep = frg[5 * NPA_MAX_E + 4];
        float gx, gy, p0x, p0y;
        slice_point(P, Fl, px_row, vx_row, n_stride, src, gx, gy, p0x, p0y);
        // a point outside the calibrated square (or a NaN): no bound on its distance, it survives whatever the others do
        const float gk = geo_key_karg<E>(sel_kbase, p0x, p0y);
        const float tk = gk + geo_tab_corr(wpack, p0x, p0y);
        // (ordered_key(tk), value for value: the sign's part as a mask behind an empty asm -- as a select it waits behind its compare)
        int tsg = __float_as_int(tk) >> 31;
        asm("" : "+v"(tsg));
        const unsigned tko = tk != tk ? 0xFFFFFFFEu : ~(__float_as_uint(tk) ^ (~(unsigned)tsg >> 1));      // (^ 0x7FFFFFFF, or ^ 0 below zero)
        const unsigned kc = gk < P.geo_far ? tko : NPA_TAB_KEY_FAR;
        if (q < cnt) fk[q] = kc;                                 // (all: entry q is point q, its geometric key is done with)
        if (first) {                                             // (one trip: cnt <= 32)
          // lower bound of the exact distance, by the filter's rules: beyond the calibrated square, a NaN, a band without a
          // calibration sample -- no bound, the candidate survives whatever dM turns out to be
          // (npa_geo_band(tk), value for value, as max / shift / min: its selects cost wait states behind their compares)
          const int tb = max(__float_as_int(tk + 0.25f), 0x3E800000) >> 20;
          unsigned ti = (unsigned)min(tb + (WP_KTAB - (int)(0x3E800000u >> 20)), WP_KTAB + NPA_GEO_BANDS - 1);
          asm("" : "+v"(ti));                                    // (an index, like wpack_at's; unsigned: no sign to extend)
          const float mt = wpack[ti] * margin_scale;
          // (a band without a sample carries an infinite margin: tk - mt is -inf or NaN there, and neither is above any dM)
          const float lb = gk < P.geo_far ? tk - mt : -3.0e38f;
          // the order: g >= 0, its bits order it; the low five give way to the POSITION in the list, so the 32 keys are distinct
          // and a rank is a count of smaller ones -- a subtraction's sign, nothing through VCC.  (The window pass compacts a trip
          // of 256 points u-major -- points 0, 4, 8, ... then 1, 5, 9, ... --, so the position is NOT the point's index: keys equal
          // in all but their last five bits are ordered by where the window pass put them.  Total and the same on every run,
          // which is all the order has to be: the rows do not depend on which sixteen come first.)
          const unsigned kb = (__float_as_uint(gk) & 0x7FFFFFE0u) | (unsigned)lane | ((unsigned)((cnt - 1 - q) >> 31) >> 1);      // (behind the list: the largest key)
          if (lane < 32) s16[32 + lane] = kb;
          WSYNC();
          int rk = 0;
#pragma unroll
          for (int j = 0; j < 32; ++j) rk -= (int)(s16[32 + j] - kb) >> 31;
          WSYNC();
          if (q < cnt) { sel[rk] = iq; s16[rk] = kc; skey[rk] = __float_as_uint(lb); }
        }
      }
      if (first) {
        WSYNC();
        ncand = 16;
        stage = 1;
        SELP(4);                                                 // (the ordering: with the candidate list's phase)
        continue;
      }
    } else
#pragma unroll 1
    for (int q0 = TABF ? (__builtin_amdgcn_readfirstlane((int)st) & ST_SECOND) >> 5 : 0, tw = 32; q0 < cnt; q0 += tw) {     // (ST_SECOND, never set on an audit wave: from 16, the first tile's rows are parked)
      const bool narrow = TILE16 && cnt - q0 <= 16;        // (wave-uniform)
      tw = narrow ? 16 : 32;
      const bool own = lane < tw;                          // tw lanes own the tile's points, the others mirror them
      const int q = q0 + (lane & (tw - 1)), qc = q < cnt ? q : cnt - 1;
      int idx;
      if (stage == 0) idx = cand_index(qc);
      else if (stage == 1) idx = sel[qc];
      else {                                  // audit tile: 32 points n_use / 32 apart, the phase moves with the launch
        const int step = n_use >> 5;
        idx = step > 0 ? qc * step + (int)(__float_as_uint(frg[5 * NPA_MAX_E + 6]) % (unsigned)step) : qc;
      }
      // the point flow, the encoder and the row epilogue of point_features_stream / _stream16 (dune_device.h), operation for
      // operation -- spelled out here because the point is fetched by INDEX from the scene's two rows (slice_point) and the
      // frame's rows come out of LDS: four row pointers and 2 E frame scalars less to carry through this loop
      float mu[E], gx, gy, lx = 0.f, ly = 0.f, dist = 0.f, p0x, p0y;
      SliceFrame Fl;      // (the frame out of LDS, per trip: the key pass's scalars are dead by now, and held across the encoder these are five registers)
      Fl.c = frg[5 * NPA_MAX_E + 0]; Fl.s = frg[5 * NPA_MAX_E + 1];
      Fl.tx = frg[5 * NPA_MAX_E + 2]; Fl.ty = frg[5 * NPA_MAX_E + 3]; Fl.tstep = frg[5 * NPA_MAX_E + 4];
      slice_point(P, Fl, px_row, vx_row, n_stride, src_index(idx, n_raw, n_use), gx, gy, p0x, p0y);
      if constexpr (KEYS16) {
        if (stage == 0 && ST_IS(ST_USE16)) encode_tile_bf16<E>(w1, wpack + WP_WB16, vec, w6, b6, p0x, p0y, lane, mu);
        else encode_tile_stream<E, false>(w1, wls, vec, w6, b6, p0x, p0y, lane, mu);
      } else if constexpr (TILE16) {
        if (narrow) encode_tile16_stream<E>(w1a, w1b, wls16, vec, w6, b6, p0x, p0y, lane, mu);
        else encode_tile_stream<E, true>(w1, wls, vec, w6, b6, p0x, p0y, lane, mu);
      } else if constexpr (BF16) encode_tile_bf16<E>(w1, wls, vec, w6, b6, p0x, p0y, lane, mu);
      else encode_tile_stream<E, false>(w1, wls, vec, w6, b6, p0x, p0y, lane, mu);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        lx = fmaf(frg[e], mu[e], lx);                                    // (uniform LDS addresses: broadcast reads)
        ly = fmaf(frg[NPA_MAX_E + e], mu[e], ly);
        const float tmp = __fsub_rn(fmaf(frg[2 * NPA_MAX_E + e], p0x, __fmul_rn(frg[3 * NPA_MAX_E + e], p0y)), frg[4 * NPA_MAX_E + e]);
        dist = fmaf(mu[e], tmp, dist);
      }
      if constexpr (KEYS16 || TABF) {
        if (stage == 1 && ST_IS(ST_AUD16)) {
          // the bound the survivors rest on, checked on every one of them: |exact - filter key| <= m16
          const unsigned k16 = s16[qc];
          const float d16 = __uint_as_float((k16 & 0x80000000u) ? (k16 & 0x7FFFFFFFu) : ~k16);
          const float ex = fabsf(dist - d16) - (TABF ? wpack_at(wpack, WP_KTAB + npa_geo_band(d16)) * margin_scale : m16);
          const bool bad = own && q < cnt && ex > 0.f;
          viol += bad ? 1 : 0;
          worst = bad ? max_nc(worst, ex) : worst;
        }
      }
      if (stage != 0 && ST_IS(ST_HAS_AUDIT)) {
        // the bound the candidates rest on, checked on every exactly encoded point: |exact - g| <= margin[band(g)]
        const float g = geo_key_karg<E>(sel_kbase, p0x, p0y);
        const float ex = fabsf(dist - g) - etab[npa_geo_band(g)];
        const bool bad = own && q < cnt && g < P.geo_far && ex > 0.f;          // (NaN distance: ex is NaN, not counted here;
        viol += bad ? 1 : 0;                                                       //  a NaN row is a broken checkpoint, not a key matter)
        worst = bad ? max_nc(worst, ex) : worst;
        if constexpr (TABF) {
          // The table filter EXCLUDES on its key: a wrong table margin drops a true member on the excluded side, where the audit of
          // the survivors (aud16 above) never looks.  The audit waves therefore check |exact - (g + f_table)| <= m_table[band(key)]
          // on every point they encode exactly -- their candidates and the 32 points of stage 2 spread over the slice, mostly
          // NON-candidates and non-survivors -- and count a failure like one of the geometric margin: the handle distrusts both.
          if (ST_IS(ST_AUDIT_WAVE) && karg_load<int>(karg_fence(sel_kbase), offsetof(DevParams, geo_tab)) != 0) {
            const float tk = g + geo_tab_corr(wpack, p0x, p0y);
            const float mt = wpack_at(wpack, WP_KTAB + npa_geo_band(tk)) * margin_scale;
            const float ext = fabsf(dist - tk) - mt;
            const bool badt = own && q < cnt && g < P.geo_far && mt < 3.0e38f && ext > 0.f;
            viol += badt ? 1 : 0;
            worst = badt ? max_nc(worst, ext) : worst;
          }
        }
      }
      if (own && q < cnt) {
        const unsigned k = ordered_key(dist);
        if (stage == 0) {
          if (ST_IS(ST_ALL)) dkey[idx] = k;
          else ckey[q] = k;
        } else if (stage == 1) {
          float* r = rows + q * ROW_W;
#pragma unroll
          for (int e = 0; e < E; ++e) r[e] = mu[e];
          r[E] = lx; r[E + 1] = ly; r[E + 2] = gx; r[E + 3] = gy; r[E + 4] = dist;
          rkey[2 * q] = (unsigned)idx; rkey[2 * q + 1] = k;
        }
      }
    }
    WSYNC();
    if (stage == 0) SELP(5); else if (stage == 1) SELP(6); else SELP(7);     // exact keys of a long list / the candidates' rows / audit tile
    if (stage == 2) break;
    if (stage == 1) {
      if constexpr (TABF) {
        if ((__builtin_amdgcn_readfirstlane((int)st) & ST_FIRST) != 0) {
          // the first tile's rows are parked.  dM: the msel-th smallest of its 16 exact keys, ROUNDED UP in the key's last bit (still
          // an upper bound): on keys of 31 bits a count of smaller ones is a subtraction's sign, nothing through VCC.  The lanes
          // that hold the msel-th smallest 31-bit key (equal keys: all of them) store the same word.  A NaN key sorts last; a
          // NaN dM drops nothing.  Then every candidate behind the first 16 against its lower bound, one lane each
          ST_PUT(ST_FIRST, false);
          unsigned myk = rkey[2 * (lane & 15) + 1] >> 1;
          asm volatile("" : "+v"(myk));                  // (its range unknown, the sign of a difference stays a shift: no compare, no carry)
          int below = 0, above = 0, j0 = 0;
          asm volatile("" : "+v"(j0));                   // (the keys' address is this trip's own, not a scalar held across the loop)
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const unsigned kj = rkey[2 * (j0 + j) + 1] >> 1;
            below -= (int)(kj - myk) >> 31;
            above -= (int)(myk - kj) >> 31;
          }
          if (below < msel && msel <= 16 - above) skey[0] = (myk << 1) | 1u;
          WSYNC();
          const unsigned kM = skey[0];
          int msg = (int)kM >> 31;
          asm("" : "+v"(msg));                                   // (a mask, not a select)
          const float dM = __uint_as_float(~(kM ^ ((unsigned)msg >> 1)));         // (ordered_key back to the float: ^ 0x7FFFFFFF for a number >= 0)
          int nrest = total;                                     // (= ntot on this path; derived here, not held as ntot - 16 across the loop)
          SEL_OPAQUE_S(nrest);
          nrest -= 16;
          const int j = 16 + min(lane, nrest - 1);
          const int ij = sel[j];
          const unsigned kj = s16[j];
          const bool hit = lane < nrest && !(__uint_as_float(skey[j]) > dM);          // dropped iff lower bound > dM, strictly
          const unsigned long long bal = __ballot(hit);
          const int pos = 16 + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
          WSYNC();
          if (hit) { sel[pos] = ij; s16[pos] = kj; }                    // (position <= source; the loads stand in front of the barrier)
          WSYNC();
          SELP(8);                                                       // (the bound and the test: with rank + emit)
          fellback = 4;                                                  // (debug statistics: decided behind the first tile)
          if (bal != 0ull) {
            fellback = 5;                                                // (first tile + a second one for the survivors)
            ncand = 16 + __popcll(bal);
            ST_PUT(ST_SECOND, true);
            ST_PUT(ST_AUD16, true);                                      // (|exact - table key| of every survivor, like the filter's)
            continue;
          }
        }
      }
      const size_t orow = (size_t)__float_as_int(frg[5 * NPA_MAX_E + 5]);
      const int Me = karg_load<int>(karg_fence(sel_kbase), offsetof(DevParams, M));      // (M, fetched for the emit: not carried to it)
      // lane q speaks for candidate q: rank on the exact (distance, index) key, emit; rows >= msel replicate row 0
      const bool mine = lane < ncand;
      const unsigned long long kx = mine ? (((unsigned long long)rkey[2 * lane + 1] << 32) | rkey[2 * lane]) : ~0ull;
      // the five output pointers leave the argument segment here: their round trip runs behind the rank loop, and they are
      // live from here to the emit only (fetched at the emit itself, the lone wave waited for them: DESIGN.md 3.1)
      const karg_ptr ko = SEL_KARGS_LATE() + SEL_KARG_OFF(mu_sorted);
      const SelOutPtrs O = {karg_load<float*>(ko, 0), karg_load<float*>(ko, 8), karg_load<float*>(ko, 16), karg_load<float*>(ko, 24),
                            karg_load<int*>(ko, 32)};
      int rank = 0;
      // (four candidates per trip: a lane behind the list holds ~0, which is smaller than nothing -- no remainder handling, a
      // quarter of the loop's scalar instructions)
      for (int i = 0; i < ncand; i += 4) {
        const unsigned long long k0 = readlane_u64(kx, i), k1 = readlane_u64(kx, (i + 1) & 63), k2 = readlane_u64(kx, (i + 2) & 63),
                                 k3 = readlane_u64(kx, (i + 3) & 63);
        rank += (k0 < kx ? 1 : 0) + (k1 < kx ? 1 : 0) + (k2 < kx ? 1 : 0) + (k3 < kx ? 1 : 0);
      }
      if (mine && rank < msel) {
        const float* r = rows + lane * ROW_W;
        float NPA_GLOBAL* mu_sorted = (float NPA_GLOBAL*)O.mu; float NPA_GLOBAL* lam_sorted = (float NPA_GLOBAL*)O.lam;
        float NPA_GLOBAL* pts_sorted = (float NPA_GLOBAL*)O.pts; float NPA_GLOBAL* dist_sorted = (float NPA_GLOBAL*)O.dist;
        auto put = [&](int q) {
          const size_t o = orow * Me + q;
#pragma unroll
          for (int e = 0; e < E; ++e) mu_sorted[o * E + e] = r[e];
          lam_sorted[o * 2 + 0] = r[E]; lam_sorted[o * 2 + 1] = r[E + 1];
          pts_sorted[o * 2 + 0] = r[E + 2]; pts_sorted[o * 2 + 1] = r[E + 3];
          dist_sorted[o] = r[E + 4];
        };
        put(rank);
        if (rank == 0)                          // the nearest row also fills rows >= msel: the padding rule of nrmp.py:258-259
#pragma unroll 1                                // (unrolled by two, its trip counts were eight scalars hoisted in front of the stage loop)
          for (int q = msel; q < Me; ++q) put(q);
      }
      if (lane == 0) {
        int word = msel;
        // (the debug flag and what the debug word is made of: read / derived here, behind a fence -- as loop invariants the
        // flag's compare mask and the shifted count were parked across the stage loop)
        if (karg_load<int>(karg_fence(sel_kbase), SEL_KBASE_OFF(debug))) {
          int nt = ntot;
          asm volatile("" : "+s"(nt));
          word |= ((nt < 255 ? nt : 255) << 8) | (fellback << 16);
        }
        ((int NPA_GLOBAL*)O.count)[orow] = word;
      }
      SELP(8);
      if (!ST_IS(ST_AUDIT_WAVE)) break;
      stage = 2;
      continue;
    }
    SEL_OPAQUE_S(st);                                           // (stage 0 only: the switches tested afresh, not as masks kept from the loop's top)
    const bool filt = (KEYS16 && ST_IS(ST_USE16)) || (TABF && ST_IS(ST_USET));
    if (lane == 0 && !(TABF && ST_IS(ST_USET))) {                                                              // (in 32-point tiles: the key policy's unit)
      unsigned* stats = SEL_KARG(unsigned*, stats);
      if (stats) atomicAdd(stats, (unsigned)((total + 31) / 32));
    }
    if (ST_IS(ST_ALL) && !filt) {
      extract();
    } else if (filt) {
      // kth = the msel-th smallest filter (key, index) pair, found WITHOUT retiring entries (the list is filtered below)
      const unsigned* fk = ST_IS(ST_ALL) ? dkey : ckey;
      // (ordered_key back to the float: distances of points inside the polygon are negative, and they are the nearest ones)
      auto key_float = [](unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); };
      // TABF: the margin of the table key is a function of the band of the KEY (WP_KTAB[band(key)]: the network has creases, and
      // where a cell straddles one -- next to the polygon's corners -- the residual is centimetres while it is a fraction of a
      // millimetre a metre away), so the bound is kept per point: U = max over the msel smallest keys of key + m(band(key)) bounds
      // the msel-th smallest EXACT distance, and a point survives iff key - m(band(key)) <= U (folded into one threshold like the
      // geometric window's g*).  Lane l holds the margins of bands l and 64 + l.
      float kt0 = 0.f, kt1 = 0.f, Ub = -3.0e38f;
      if constexpr (TABF) {
        kt0 = wpack_at(wpack, WP_KTAB + lane) * margin_scale;
        kt1 = wpack_at(wpack, WP_KTAB + 64 + (lane < NPA_GEO_BANDS - 64 ? lane : NPA_GEO_BANDS - 65)) * margin_scale;
      }
      unsigned long long prev = 0ull;
      for (int m2 = 0; m2 < msel; ++m2) {
        unsigned long long best = ~0ull;
        for (int q = lane; q < total; q += 64) {
          const unsigned long long v = ((unsigned long long)fk[q] << 32) | (unsigned)cand_index(q);
          if (v < best && (m2 == 0 || v > prev)) best = v;
        }
        prev = wave_min_u64(best);
        if constexpr (TABF) {
          const float km = key_float((unsigned)(prev >> 32));
          const int bm = __builtin_amdgcn_readfirstlane(npa_geo_band(km));
          const float mb = __uint_as_float(bm < 64 ? __builtin_amdgcn_readlane(__float_as_uint(kt0), bm & 63)
                                                   : __builtin_amdgcn_readlane(__float_as_uint(kt1), bm & 63));
          Ub = max_nc(Ub, km + mb);                                 // (a far / NaN key among them: inf or NaN, refused below)
          if (!(km == km)) Ub = __builtin_inff();
        }
      }
      const unsigned kth = (unsigned)(prev >> 32);
      const float dk = key_float(kth);
      bool bound_ok;
      unsigned thr16, thr_hi = NPA_TAB_KEY_FAR;
      if constexpr (TABF) {
        // bands without a margin (no calibration node produced such a key: beyond the corners of the largest square): their
        // points survive unconditionally, like the far ones -- every key at or above the lowest such band does
        float gs = -3.0e38f;
        unsigned long long noinf[2];
#pragma unroll
        for (int rep = 0; rep < 2; ++rep) {
          const int bnd = lane + 64 * rep;
          const float mb = rep == 0 ? kt0 : kt1;
          const bool have = bnd < NPA_GEO_BANDS && mb < 3.0e38f;
          noinf[rep] = __ballot(bnd < NPA_GEO_BANDS && !have);
          if (have) {
            const float lo_b = bnd == 0 ? -3.0e38f : __uint_as_float((unsigned)(bnd + (0x3E800000u >> 20)) << 20) - 0.25f;
            const float hi_b = bnd == NPA_GEO_BANDS - 1 ? 3.0e38f : __uint_as_float((unsigned)(bnd + 1 + (0x3E800000u >> 20)) << 20) - 0.25f;
            const float reach = Ub + mb;
            if (lo_b <= reach) gs = max_nc(gs, min_nc(hi_b, reach));
          }
        }
        gs = wave_max_f32(gs);
        const int binf = noinf[0] ? __builtin_ctzll(noinf[0]) : (noinf[1] ? 64 + __builtin_ctzll(noinf[1]) : NPA_GEO_BANDS);
        const float lo_inf = binf >= NPA_GEO_BANDS ? 3.0e38f
                                                   : (binf == 0 ? -3.0e38f : __uint_as_float((unsigned)(binf + (0x3E800000u >> 20)) << 20) - 0.25f);
        bound_ok = Ub == Ub && Ub < 3.0e38f && gs < lo_inf && gs >= dk;
        thr16 = ordered_key(gs);
        thr_hi = binf >= NPA_GEO_BANDS ? NPA_TAB_KEY_FAR : ordered_key(lo_inf);
        m16 = 0.f;                                               // (the audit of stage 1 looks the margin up per survivor)
      } else {
        // margin: the largest calibrated |bf16 - exact| over the bands around the threshold (bands are >= 32 mm wide, the margin is
        // centimetres: one band below, three above cover every survivor); uncalibrated (inf) or a broken key: exact keys
        float mm = 0.f;
        const int b0 = npa_geo_band(dk);
#pragma unroll
        for (int o = -1; o <= 3; ++o) {
          const int bb = b0 + o < 0 ? 0 : (b0 + o >= NPA_GEO_BANDS ? NPA_GEO_BANDS - 1 : b0 + o);
          mm = fmaxf(mm, wpack[WP_K16 + bb]);
        }
        m16 = mm * margin_scale;
        bound_ok = dk == dk && fabsf(dk) < 3.0e38f && m16 < 0.25f;
        thr16 = ordered_key(dk + 2.0f * m16);
      }
      ST_PUT(ST_USE16, false); ST_PUT(ST_USET, false);                               // (whatever follows, stage 0 does not run the filter again)
      bool decided = false;
      if (bound_ok) {
        // survivors: filter key at or below the threshold.  Their indices are compacted IN PLACE over the list (position <= source,
        // a chunk's loads precede its stores), the first SEL_CAP also into sel[] / s16[] for the final ranking and the audit
        int nsurv = 0;
        for (int q0 = 0; q0 < total; q0 += 64) {
          const int q = q0 + lane;
          const unsigned kq = q < total ? fk[q] : 0xFFFFFFFFu;
          const int iq = q < total ? cand_index(q) : 0;
          const bool hit = q < total && (kq <= thr16 || (TABF && kq >= thr_hi));
          const unsigned long long bal = __ballot(hit);
          const int pos = nsurv + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0));
          if (hit) {
            dkey[pos] = (unsigned)iq;
            if (pos < SEL_CAP) { sel[pos] = iq; s16[pos] = kq; }
          }
          nsurv += __popcll(bal);
        }
        WSYNC();
        decided = true;
        if (nsurv <= SEL_CAP && nsurv >= msel) {                 // the survivors fit the final ranking: straight to the exact rows
          fellback = 3;                                          // (debug statistics: the filter decided this slice)
          ST_PUT(ST_AUD16, true);                                          // (stage 1 audits |exact - filter key| of every survivor)
          ST_PUT(ST_ALL, false);
          ncand = nsurv;
          stage = 1;
          SELP(9);
          continue;
        }
        if (nsurv >= msel) {                                     // a shorter list for the exact keys (every true member is in it)
          fellback = 2;
          if (!ST_IS(ST_ALL)) total = nsurv;
          else if (2 * nsurv <= n_use) { ST_PUT(ST_ALL, false); total = nsurv; ckey = dkey + nsurv; }
          else total = n_use;                                    // (still most of the slice: exact keys for every point, in place)
        } else if (ST_IS(ST_ALL)) total = n_use;
      }
      if (!decided && !ST_IS(ST_OVERFLOW)) {                               // (a list that fitted anyway and an uncalibrated band: as without the filter)
        if (lane < ntot) sel[lane] = (int)dkey[lane];
        WSYNC();
        ncand = ntot;
        stage = 1;
        continue;
      }
      continue;                                                  // stage 0 again, exact keys
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
      if (lane < msel) sel[lane] = mywin;                       // the list was read through cand_index until here
      WSYNC();
    }
    ncand = msel;
    stage = 1;
    SELP(9);
  }
  if (ST_IS(ST_HAS_AUDIT)) {
    const unsigned long long vb = __ballot(viol > 0);
    if (vb != 0ull) {                          // rare: the counters are touched only then (and by audit waves)
      unsigned* audit_g = SEL_KARG(unsigned*, audit);
      int v = viol;
      float wv = worst;
      for (int o = 32; o > 0; o >>= 1) { v += __shfl_xor(v, o, 64); wv = max_nc(wv, __shfl_xor(wv, o, 64)); }
      if (lane == 0) {
        atomicAdd(audit_g + 2, (unsigned)v); atomicMax(audit_g + 3, __float_as_uint(wv));
        // mirror for the host: words 6, 7 of the block hold a pointer to a pinned, host-mapped counter (or null).  The owner
        // polls it without synchronising the device (npa_audit_peek); only this rare path ever writes across the bus
        unsigned* hp = *reinterpret_cast<unsigned* const*>(audit_g + 6);
        if (hp) __hip_atomic_fetch_add(hp, (unsigned)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
    if (ST_IS(ST_AUDIT_WAVE) && lane == 0) {
      unsigned* audit_g = SEL_KARG(unsigned*, audit);
      atomicAdd(audit_g + 0, 1u); atomicAdd(audit_g + 1, (unsigned)(n_use < 32 ? n_use : 32));
    }
  }
  SELP(10);
#ifdef NPA_SEL_PROF
  if (lane == 0 && blockIdx.x < SELP_WAVES) {
    unsigned long long* row = npa_sel_prof[blockIdx.x];
    row[15] += 1ull;
    row[14] += (unsigned long long)__builtin_amdgcn_s_memtime() - sp0_;
#pragma unroll
    for (int i = 0; i < 11; ++i) row[i] += sacc_[i];
  }
#endif
