// The Net glue arithmetic (model.py:38-39, 44-48, 54-55, 62-63), one definition of each expression
// for every layout: the planar heads and t-blend (head.hip) and the record heads and t-blends
// (glue_h8.hip).  reuse_flow needs a head and its matching t-blend kernel to give the same bits,
// and the layouts to agree where their inputs do: the operation order here is that contract.
// All without fp contraction (no FMA the reference does not have).
#pragma once
#include "common.hpp"

namespace rrin {

// Ft0 = (-(1-t)t) F01 + (t t) F10, Ft1 = ((1-t)^2) F01 - (t(1-t)) F10 (model.py:38-39);
// raw = F01 (u, v), F10 (u, v); cf[0..3] the four coefficients of the image
__device__ inline void flow_blend(const float* cf, const float* raw, float* ft0, float* ft1) {
#pragma clang fp contract(off)
  for (int k = 0; k < 2; ++k) {
    ft0[k] = cf[0] * raw[k] + cf[1] * raw[2 + k];
    ft1[k] = cf[2] * raw[k] - cf[3] * raw[2 + k];
  }
}

// out = (w1 xt1 + w2 xt2) / (w1 + w2 + 1e-8), w1 = (1-t) sigmoid(logit0), w2 = t sigmoid(logit1)
// (model.py:52-55); cf[4], cf[5] = 1-t, t
__device__ inline void mask_blend(const float* cf, float logit0, float logit1, const float* xt1, const float* xt2,
                                  float* o) {
#pragma clang fp contract(off)
  const float m0 = 1.0f / (1.0f + expf(-logit0));
  const float m1 = 1.0f / (1.0f + expf(-logit1));
  const float w1 = cf[4] * m0, w2 = cf[5] * m1;
  const float den = w1 + w2 + 1e-8f;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) o[ch] = (w1 * xt1[ch] + w2 * xt2[ch]) / den;
}

// q = clamp(acc + base, 0, 1) (model.py:62-63); a NaN passes
__device__ inline void final_clamp(const float* acc, const float* base, float* q) {
#pragma clang fp contract(off)
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float v = acc[ch] + base[ch];
    q[ch] = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
  }
}

// backwarp of channels c0 .. c0 + 2 of the record-layout Net buffer: load8(y, x, v) fetches the
// 8 channels 0-7 of pixel (y, x) into v, once per valid tap (taps outside the frame read 0)
template <class L>
__device__ inline void warp3(const WarpTaps& t, int c0, L load8, float* o) {
#pragma clang fp contract(off)
  float q[4][8];
  const bool ok[4] = {t.vy0 && t.vx0, t.vy0 && t.vx1, t.vy1 && t.vx0, t.vy1 && t.vx1};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (ok[k]) {
      load8(t.y0 + (k >> 1), t.x0 + (k & 1), q[k]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) q[k][e] = 0.0f;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
    o[c] = q[0][c0 + c] * t.nw + q[1][c0 + c] * t.ne + q[2][c0 + c] * t.sw + q[3][c0 + c] * t.se;
}

}  // namespace rrin
