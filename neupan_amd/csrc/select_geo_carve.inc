// select_geo_carve.inc -- the LDS carve of the geometric selection (one wave, one slice at a time); see select_geo_body.inc
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* vec = smem;                       // [11][32]
  float* w6 = vec + 11 * 32;               // [8][32]
  float* b6 = w6 + 8 * 32;                 // [8]
  float* etab = b6 + 8;                    // [NPA_GEO_BANDS] margin per distance band
  float* frg = etab + NPA_GEO_BANDS;       // [6][NPA_MAX_E] the slice's frame as the stage loop reads it (load_frame<E, true>; SEL_LDS_FRAME floats)
  int* sel = reinterpret_cast<int*>(frg + SEL_LDS_FRAME);    // [SEL_CAP]: the candidates of the final ranking
  unsigned* skey = reinterpret_cast<unsigned*>(sel + SEL_CAP);   // [NPA_MAX_M] scratch of extract()
  constexpr int ROW_W = E + 5;                                // mu[E], lam[2], point[2], distance
  unsigned* s16 = skey + NPA_MAX_M;                            // [SEL_CAP] bf16-encoder keys of the survivors (KEYS16 tier only)
  unsigned* dkey = s16 + SEL_CAP;                              // [n_use padded to SEL2_TRIP] keys; then the candidate list
  float* rows = reinterpret_cast<float*>(dkey);               // [SEL_CAP][ROW_W] (takes over the key area once sel[] stands)
  unsigned* rkey = reinterpret_cast<unsigned*>(rows + SEL_CAP * (NPA_MAX_E + 5));   // [SEL_CAP][2]: (index, exact key)
