// The integer colour conversion of the YUV frame path (4:2:0, and by rrin_chroma 4:2:2 / 4:4:4) (rrin_yuv_coef in rrin_hip.h), shared
// by the input pack (yuv.hip) and the FINAL head's store (glue_h8.hip), and the host-side checks
// of a rrin_yuv420 stack; below them the same for 10- and 12-bit samples in 16-bit words
// (rrin_yuv420_16).  int32 only: no float colour math, so no FMA contraction can change a bit.
#pragma once
#include "common.hpp"

namespace rrin {

__device__ inline int clip255(int v) { return min(max(v, 0), 255); }

// one pixel's RGB bytes from its luma and its block's chroma
__device__ inline void yuv_to_rgb(const rrin_yuv_coef& k, int y, int u, int v, int* rgb) {
  const int c = k.ay * (y - k.y0) + 8192, d = u - 128, e = v - 128;
  rgb[0] = clip255((c + k.rv * e) >> 14);
  rgb[1] = clip255((c + k.gu * d + k.gv * e) >> 14);
  rgb[2] = clip255((c + k.bu * d) >> 14);
}

__device__ inline int rgb_to_luma(const rrin_yuv_coef& k, const int* rgb) {
  return clip255(k.y0 + ((k.yr * rgb[0] + k.yg * rgb[1] + k.yb * rgb[2] + 8192) >> 14));
}

// a chroma sample from the sums of its block's four pixels' bytes
__device__ inline int rgb_sum_to_chroma(int kr, int kg, int kb, const int* sum) {
  return clip255(128 + ((kr * sum[0] + kg * sum[1] + kb * sum[2] + 32768) >> 16));
}

// the same for a block of P = 2^LOG2P pixels (4:2:2: 2, 4:4:4: 1): + 8192 P, >> (14 + log2 P);
// LOG2P 2 is rgb_sum_to_chroma
template <int LOG2P>
__device__ inline int rgb_block_to_chroma(int kr, int kg, int kb, const int* sum) {
  return clip255(128 + ((kr * sum[0] + kg * sum[1] + kb * sum[2] + (8192 << LOG2P)) >> (14 + LOG2P)));
}

// ---- 10- and 12-bit samples in 16-bit words (rrin_yuv420_16) -----------------------------
// the same formulas with mid = 2^(depth-1) for 128 and a clip to maxv = 2^depth - 1
__device__ inline int clip_to(int v, int maxv) { return min(max(v, 0), maxv); }

// the sample of a word: min(word >> shift, maxv)
__device__ inline int sample16(uint16_t word, int shift, int maxv) { return min((int)word >> shift, maxv); }

__device__ inline void yuv_to_rgb16(const rrin_yuv_coef& k, int mid, int maxv, int y, int u, int v, int* rgb) {
  const int c = k.ay * (y - k.y0) + 8192, d = u - mid, e = v - mid;
  rgb[0] = clip_to((c + k.rv * e) >> 14, maxv);
  rgb[1] = clip_to((c + k.gu * d + k.gv * e) >> 14, maxv);
  rgb[2] = clip_to((c + k.bu * d) >> 14, maxv);
}

__device__ inline int rgb_to_luma16(const rrin_yuv_coef& k, int maxv, const int* rgb) {
  return clip_to(k.y0 + ((k.yr * rgb[0] + k.yg * rgb[1] + k.yb * rgb[2] + 8192) >> 14), maxv);
}

__device__ inline int rgb_sum_to_chroma16(int kr, int kg, int kb, int mid, int maxv, const int* sum) {
  return clip_to(mid + ((kr * sum[0] + kg * sum[1] + kb * sum[2] + 32768) >> 16), maxv);
}

template <int LOG2P>
__device__ inline int rgb_block_to_chroma16(int kr, int kg, int kb, int mid, int maxv, const int* sum) {
  return clip_to(mid + ((kr * sum[0] + kg * sum[1] + kb * sum[2] + (8192 << LOG2P)) >> (14 + LOG2P)), maxv);
}

// float(v) / float(maxv) as torch computes it: the IEEE fp32 division (v_div_scale / v_div_fmas /
// v_div_fixup: correctly rounded; the library is built without fast-math), never a reciprocal
// multiply, which differs from it in the last bit for some v
__device__ inline float sample_to_float(int v, float maxv) { return __fdiv_rn((float)v, maxv); }

// ---- host side -------------------------------------------------------------------------
inline int yuv_coef_check(const rrin_yuv_coef* k) {
  if (!k || k->y0 < 0 || k->y0 > 255) return RRIN_E_ARG;
  const int32_t* v = &k->ay;
  for (int i = 0; i < 14; ++i)
    if (v[i] <= -65536 || v[i] >= 65536) return RRIN_E_ARG;
  return 0;
}

inline bool chroma_ok(int chroma) { return chroma >= RRIN_CHROMA_420 && chroma <= RRIN_CHROMA_444; }

// sizes, pitches and frame stride of n frames of h0 x w0 at a valid chroma format: 4:2:0 takes
// even sizes >= 2 and has h0/2 x w0/2 chroma samples, 4:2:2 an even w0 >= 2 and any h0 >= 1
// (h0 x w0/2), 4:4:4 any sizes >= 1 (h0 x w0); the frames of a stack must not overlap
inline int yuv_sizes_check(int chroma, int c_step, int64_t img_stride, int y_pitch, int c_pitch, int n, int h0,
                           int w0) {
  if (n < 1) return RRIN_E_SHAPE;
  if (chroma == RRIN_CHROMA_420) {
    if (h0 < 2 || w0 < 2 || (h0 & 1) || (w0 & 1)) return RRIN_E_SHAPE;
  } else if (chroma == RRIN_CHROMA_422) {
    if (h0 < 1 || w0 < 2 || (w0 & 1)) return RRIN_E_SHAPE;
  } else if (h0 < 1 || w0 < 1) {
    return RRIN_E_SHAPE;
  }
  const int ch = chroma == RRIN_CHROMA_420 ? h0 / 2 : h0, cw = chroma == RRIN_CHROMA_444 ? w0 : w0 / 2;
  if (y_pitch < w0 || c_pitch < (int64_t)cw * c_step) return RRIN_E_SHAPE;
  const int64_t y_span = (int64_t)(h0 - 1) * y_pitch + w0;
  const int64_t c_span = (int64_t)(ch - 1) * c_pitch + (int64_t)(cw - 1) * c_step + 1;
  if (n > 1 && (img_stride < y_span || img_stride < c_span)) return RRIN_E_SHAPE;
  return 0;
}

// n frames of h0 x w0 in s: planes, layout, sizes and pitches (nothing is dereferenced)
__attribute__((visibility("hidden"))) inline int yuv420_check(const rrin_yuv420& s, int n, int h0, int w0) {
  if (!s.y || !s.u || !s.v || (s.c_step != 1 && s.c_step != 2) || !chroma_ok(s.chroma)) return RRIN_E_ARG;
  return yuv_sizes_check(s.chroma, s.c_step, s.img_stride, s.y_pitch, s.c_pitch, n, h0, w0);
}

// the coefficient bounds of the 16-bit path (rrin_yuv420_16): with them every sum fits int32 at depth 12
inline int yuv_coef_check16(const rrin_yuv_coef* k, int depth) {
  if (!k || k->y0 < 0 || k->y0 > (1 << depth) - 1) return RRIN_E_ARG;
  const int32_t* v = &k->ay;
  for (int i = 0; i < 14; ++i) {
    const int32_t lim = i < 5 ? 65536 : 32768;
    if (v[i] <= -lim || v[i] >= lim) return RRIN_E_ARG;
  }
  return 0;
}

// yuv420_check for 16-bit words: depth, shift, then planes, sizes and pitches in samples
__attribute__((visibility("hidden"))) inline int yuv420_16_check(const rrin_yuv420_16& s, int n, int h0, int w0) {
  if ((s.depth != 10 && s.depth != 12) || (s.shift != 0 && s.shift != 16 - s.depth)) return RRIN_E_ARG;
  if (!s.y || !s.u || !s.v || (s.c_step != 1 && s.c_step != 2) || !chroma_ok(s.chroma)) return RRIN_E_ARG;
  return yuv_sizes_check(s.chroma, s.c_step, s.img_stride, s.y_pitch, s.c_pitch, n, h0, w0);
}

}  // namespace rrin
