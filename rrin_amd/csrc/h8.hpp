// Record layouts of the hot path, shared by the record conv (conv_h8.hip), the non-conv kernels
// of the record path (glue_h8.hip), the host-side packing (pack_h8.hip) and the ring fix-up
// (edge_fix.hpp): the fp16 hi / lo' split, record and element indexing, and the host-side view
// checks.
//
// H8 activation layout: per image and 8-channel group an hp x wp plane of 16-B records (8
// halves).  A pixel's 8 channels are one record, so the MFMA operands (8 consecutive k per lane)
// are single ds_read_b128s of the staged tile, and epilogue stores of 32 pixels x 8 B per
// half-wave are contiguous.  F16X3 keeps two such planes (hi and lo'), F16 one.  R32 (exact
// fp32): a record holds 4 fp32 channels, one plane.
#pragma once
#include "common.hpp"

namespace rrin {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float float2v __attribute__((ext_vector_type(2)));

constexpr int H8_LC = 34;  // staged input row: records of pixels x0-1 .. x0+32

// lo halves are stored pre-scaled by 2^11 so they stay normal fp16 for any
// |v| >= ~1e-4 (unscaled, v - hi ~ 2^-12 v would be subnormal below |v| = 0.125
// and lose its bits): v = hi + lo * 2^-11.
constexpr float kLoScale = 2048.0f;
constexpr float kF16Max = 65504.0f;  // largest finite fp16
constexpr float kLoUnscale = 1.0f / 2048.0f;
__device__ inline _Float16 lo_of(float v, _Float16 hi) { return (_Float16)((v - (float)hi) * kLoScale); }
__device__ inline float join(_Float16 hi, _Float16 lo) { return fmaf((float)lo, kLoUnscale, (float)hi); }

// hi/lo split of 4 consecutive channels into two 8-B record halves: hi = RNE fp16
// of v (v_cvt_pk_f16_f32, two values per op), lo = fp16 of (v - hi) * 2^11 as one
// v_fma_mix_f32 (hi read as f16) on v * 2^11 -- the exact difference, so the same
// bits as lo_of (the kernels are built without packed FP32 ops).
__device__ inline void split4(const float* v, uint2& hv, uint2& lv) {
  const half2v h0 = __builtin_convertvector((float2v){v[0], v[1]}, half2v);
  const half2v h1 = __builtin_convertvector((float2v){v[2], v[3]}, half2v);
  const float l0 = fmaf((float)h0[0], -kLoScale, v[0] * kLoScale), l1 = fmaf((float)h0[1], -kLoScale, v[1] * kLoScale);
  const float l2 = fmaf((float)h1[0], -kLoScale, v[2] * kLoScale), l3 = fmaf((float)h1[1], -kLoScale, v[3] * kLoScale);
  hv = make_uint2(__builtin_bit_cast(unsigned, h0), __builtin_bit_cast(unsigned, h1));
  lv = make_uint2(__builtin_bit_cast(unsigned, __builtin_convertvector((float2v){l0, l1}, half2v)),
                  __builtin_bit_cast(unsigned, __builtin_convertvector((float2v){l2, l3}, half2v)));
}

// keep floats [0, nvalid) of an fp32 record (nvalid in 1..3)
__device__ inline uint4 mask_floats(uint4 v, int nvalid) {
  if (nvalid < 2) v.y = 0u;
  if (nvalid < 3) v.z = 0u;
  v.w = 0u;
  return v;
}

__device__ inline uint4 mask_halves(uint4 v, int nvalid) {
  // keep halves [0, nvalid) of a record (nvalid in 1..7)
  unsigned* d = reinterpret_cast<unsigned*>(&v);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (2 * k >= nvalid)
      d[k] = 0u;
    else if (2 * k + 1 >= nvalid)
      d[k] &= 0xFFFFu;
  }
  return v;
}

// index (halves) of channel ch of pixel (y, x) in an H8 plane set
__device__ inline int64_t h8_half_index(int64_t img_stride, int64_t gp, int wp, int img, int ch, int y, int x) {
  return ((int64_t)img * img_stride + (int64_t)(ch >> 3) * gp + (int64_t)(y + 1) * wp + x + kH8PadLeft) * 8 +
         (ch & 7);
}
// the same in floats of an R32 plane set (4 channels per record)
__device__ inline int64_t r32_elem_index(int64_t img_stride, int64_t gp, int wp, int img, int ch, int y, int x) {
  return ((int64_t)img * img_stride + (int64_t)(ch >> 2) * gp + (int64_t)(y + 1) * wp + x + kH8PadLeft) * 4 +
         (ch & 3);
}
__device__ inline uint4 f4rec(float a, float b, float c, float d) {
  return make_uint4(__float_as_uint(a), __float_as_uint(b), __float_as_uint(c), __float_as_uint(d));
}

// float(u) / 255.0f, correctly rounded, for every byte value: evaluated by the host compiler
// (a multiply by 1 / 255.0f differs from the division for 126 of the 256 values).  The 8-bit
// input packs (glue_h8.hip, yuv.hip) each keep a __constant__ instance.
struct U8ScaleTab {
  float v[256];
  constexpr U8ScaleTab() : v{} {
    for (int i = 0; i < 256; ++i) v[i] = (float)i / 255.0f;
  }
};

// ---- host side: precisions and view checks -----------------------------------------
inline int planes_of(int prec) { return prec == RRIN_PREC_F16X3 ? 2 : 1; }
// record-layout precisions: F16X3 / F16 (8 halves per record), F32R (4 floats)
inline bool rec_prec(int prec) {
  return prec == RRIN_PREC_F16X3 || prec == RRIN_PREC_F16 || prec == RRIN_PREC_F32R;
}
inline int chans_per_rec(int prec) { return prec == RRIN_PREC_F32R ? 4 : 8; }

// (hidden: too large to inline everywhere, and the library exports nothing but its C ABI)
__attribute__((visibility("hidden"))) inline bool h8_ok(const rrin_h8& v, int prec) {
  if (!v.hi || (prec == RRIN_PREC_F16X3 && !v.lo)) return false;
  if (prec == RRIN_PREC_F32R && v.lo) return false;  // one plane
  const rrin_geom g = make_geom_h8(v.g.h, v.g.w);
  return g.hp == v.g.hp && g.wp == v.g.wp && g.plane == v.g.plane;
}

inline int64_t ring_pixels(int h, int w) {
  return h < 2 ? (int64_t)w : 2 * (int64_t)w + 2 * (int64_t)(h - 2);
}

}  // namespace rrin
