// The linear-light synthetic shutter (rrin_amd/exposure.py and rrin_amd/transfer.py are the definition;
// include/rrin_hip.h the contract): rrin_mean_frames_lut, the weighted mean of the frames ptr[start[g] ..
// start[g+1]) per stored element, through a transfer table or on code values, and rrin_mean_frames_yuv_lut,
// the same per pixel and channel of YUV frames between the integer conversions of yuv.hpp.
//
// Both follow mean_frames_kernel (exposure.hip): the sources are a table of pointers read through the scalar
// cache with their weights beside them (the index is uniform in a workgroup), blockIdx.y is the output,
// integer sums and no atomics: the same bits on every run.  What is new is the table: lin[maxval + 1] then
// thr[maxval + 1], int32, copied into LDS once per workgroup (2 KiB at 8 bits, 32 KiB at 12), which is why
// a workgroup walks its output's runs in a grid-stride loop over blockIdx.x instead of taking one.
// Decoding is one LDS gather per sample, encoding a branch-free binary search of depth steps over thr.
// Sums are 64-bit: a weight sum W <= 65535 times lin <= 2^30 stays below 2^46.  Nothing outside the
// frames is read or written, and elements between the frames of a strided output are not written.
#include "yuv.hpp"

namespace rrin {

// the divide by W: q = floor(n * M / 2^64) with M = floor(2^64 / W) + 1 is floor(n / W) for every
// n * e < 2^64, e = M * W - 2^64 in [1, W]: with n = q W + r, n M / 2^64 = q + (r + n e / 2^64) / W and
// r <= W - 1, so the floor is q while n e / 2^64 < 1.  Here n <= 65535 * 2^30 + 32767 < 2^46 + 2^15 and
// e <= W <= 65535 < 2^16, so n * e < 2^63.  W == 1 has no 64-bit M and needs none.
struct LutDiv {
  uint64_t magic, half;
  bool one;
  __device__ uint64_t operator()(uint64_t sum) const { return one ? sum : __umul64hi(sum + half, magic); }
};

__device__ inline LutDiv lut_div(uint32_t w) {
  // floor(2^64 / w) = floor((2^64 - 1) / w) unless w divides 2^64, a power of two: then the latter is one less
  const uint64_t f = ~0ull / w + ((w & (w - 1)) == 0 ? 1ull : 0ull);
  return LutDiv{w > 1 ? f + 1ull : 0ull, (uint64_t)(w >> 1), w == 1};
}

template <class E>
__device__ inline int lut_sample(E v, int maxval, int shift) {
  if constexpr (sizeof(E) == 1) return v;
  else return min((int)v >> shift, maxval);
}

template <class E, int ACCESS>
struct alignas(ACCESS) LutVec {
  E e[ACCESS / sizeof(E)];
};

// A frame pointer read from the table is a generic pointer to the compiler (flat_load); the frames are
// device memory, so say so: global_load.
template <int BYTES>
struct LutRaw;
template <>
struct LutRaw<16> {
  typedef uint32_t type __attribute__((ext_vector_type(4)));
};
template <>
struct LutRaw<4> {
  typedef uint32_t type;
};
template <>
struct LutRaw<2> {
  typedef uint16_t type;
};
template <>
struct LutRaw<1> {
  typedef uint8_t type;
};

template <class T, class E>
__device__ inline T lut_load(const E* p) {
  using R = typename LutRaw<sizeof(T)>::type;
  const R r = *(const __attribute__((address_space(1))) R*)p;
  T v;
  __builtin_memcpy(&v, &r, sizeof(T));
  return v;
}

// the table into LDS: 2 * (maxval + 1) int32, a multiple of 4, from a 16-byte aligned address
__device__ inline void lut_stage(int32_t* lds, const int32_t* __restrict__ table, int entries) {
  typedef int32_t i4 __attribute__((ext_vector_type(4)));
  const i4* src = reinterpret_cast<const i4*>(table);
  i4* dst = reinterpret_cast<i4*>(lds);
  for (int i = threadIdx.x; i < entries / 4; i += blockDim.x) dst[i] = src[i];
  __syncthreads();
}

// enc(v): the number of c in 1..maxval with thr[c] <= v (thr non-decreasing), depth steps, no branch:
// pos + step never passes maxval = 2^depth - 1
__device__ inline int lut_encode(const int32_t* thr, int depth, uint32_t v) {
  int pos = 0;
  for (int step = 1 << (depth - 1); step > 0; step >>= 1) pos += (uint32_t)thr[pos + step] <= v ? step : 0;
  return pos;
}

// one source's value of a sample: lin[s] with a table, the sample itself without
template <bool LUT>
__device__ inline uint32_t lut_value(const int32_t* lin, int s) {
  if constexpr (LUT) return (uint32_t)lin[s];
  else return (uint32_t)s;
}

// the weights of a group and their sum; false if the group is not one the Python layer makes
__device__ inline bool lut_group(const int32_t* __restrict__ start, const int32_t* __restrict__ weights, int g,
                                 int k_total, int& s0, int& s, uint32_t& wsum) {
  s0 = max(start[g], 0);
  s = min(start[g + 1], k_total) - s0;
  if (s < 1 || s > 256) return false;
  uint64_t t = 0;
  for (int k = 0; k < s; ++k) {
    const int32_t w = weights[s0 + k];
    if (w < 1 || w > 65535) return false;
    t += (uint32_t)w;
  }
  if (t > 65535) return false;
  wsum = (uint32_t)t;
  return true;
}

template <class E, int ACCESS, bool LUT>
__global__ void __launch_bounds__(256) mean_frames_lut_kernel(const E* const* __restrict__ ptr,
                                                              const int32_t* __restrict__ start,
                                                              const int32_t* __restrict__ weights,
                                                              const int32_t* __restrict__ table, int k_total,
                                                              E* __restrict__ out, int64_t out_stride, int64_t len,
                                                              int depth, int shift) {
  extern __shared__ __attribute__((aligned(16))) int32_t lut_lds[];
  constexpr int V = ACCESS / sizeof(E);
  using Vec = LutVec<E, ACCESS>;
  const int maxval = (1 << depth) - 1;
  const int g = blockIdx.y;
  int s0, s;
  uint32_t wsum;
  if (!lut_group(start, weights, g, k_total, s0, s, wsum)) return;  // uniform: nothing is read or written
  if constexpr (LUT) lut_stage(lut_lds, table, 2 * (maxval + 1));
  const int32_t* lin = lut_lds;
  const int32_t* thr = lut_lds + (maxval + 1);
  const LutDiv div = lut_div(wsum);
  const E* const* src = ptr + s0;
  const int32_t* wt = weights + s0;
  E* o = out + (int64_t)g * out_stride;
  const int64_t whole = len / V;
  const int64_t lanes = whole + (V > 1 && len % V ? 1 : 0);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < lanes; i += (int64_t)gridDim.x * 256) {
    if (i < whole) {
      const int64_t off = i * V;
      uint64_t acc[V];
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] = 0;
      int k = 0;
      for (; k + 2 <= s; k += 2) {
        const Vec a = lut_load<Vec>(src[k] + off), b = lut_load<Vec>(src[k + 1] + off);
        const uint32_t wa = (uint32_t)wt[k], wb = (uint32_t)wt[k + 1];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          acc[e] += (uint64_t)wa * lut_value<LUT>(lin, lut_sample(a.e[e], maxval, shift));
          acc[e] += (uint64_t)wb * lut_value<LUT>(lin, lut_sample(b.e[e], maxval, shift));
        }
      }
      if (k < s) {
        const Vec a = lut_load<Vec>(src[k] + off);
        const uint32_t wa = (uint32_t)wt[k];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] += (uint64_t)wa * lut_value<LUT>(lin, lut_sample(a.e[e], maxval, shift));
      }
      Vec r;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const uint32_t v = (uint32_t)div(acc[e]);
        r.e[e] = (E)((LUT ? lut_encode(thr, depth, v) : (int)v) << shift);
      }
      *reinterpret_cast<Vec*>(o + off) = r;
    } else {
      for (int64_t e = whole * V; e < len; ++e) {
        uint64_t acc = 0;
        for (int k = 0; k < s; ++k)
          acc += (uint64_t)(uint32_t)wt[k] * lut_value<LUT>(lin, lut_sample(lut_load<E>(src[k] + e), maxval, shift));
        const uint32_t v = (uint32_t)div(acc);
        o[e] = (E)((LUT ? lut_encode(thr, depth, v) : (int)v) << shift);
      }
    }
  }
}

// the workgroups of one launch: enough to fill the device a few times over, few enough that the table
// load (32 KiB per workgroup at 12 bits) is shared by several runs
constexpr int64_t LUT_MAX_GROUPS = 2048;

template <class E, int ACCESS, bool LUT>
int mean_frames_lut_launch(const void* const* ptr, const int32_t* start, const int32_t* weights, const int32_t* table,
                           int k_total, int g, void* out, int64_t out_stride, int64_t len, int depth, int shift,
                           hipStream_t st) {
  constexpr int V = ACCESS / sizeof(E);
  const int64_t lanes = len / V + (len % V ? 1 : 0);
  int64_t blocks = (lanes + 255) / 256;
  const int64_t cap = LUT ? (LUT_MAX_GROUPS + g - 1) / g : 0x7fffffff;
  if (blocks > cap) blocks = cap;
  const size_t lds = LUT ? sizeof(int32_t) * 2 * ((size_t)1 << depth) : 0;
  hipLaunchKernelGGL((mean_frames_lut_kernel<E, ACCESS, LUT>), dim3((unsigned)blocks, (unsigned)g), dim3(256), lds, st,
                     reinterpret_cast<const E* const*>(ptr), start, weights, table, k_total, static_cast<E*>(out),
                     out_stride, len, depth, shift);
  return hip_code(hipGetLastError());
}

template <class E, bool LUT>
int mean_frames_lut_access(int access, const void* const* ptr, const int32_t* start, const int32_t* weights,
                           const int32_t* table, int k_total, int g, void* out, int64_t out_stride, int64_t len,
                           int depth, int shift, hipStream_t st) {
  if (access == 16)
    return mean_frames_lut_launch<E, 16, LUT>(ptr, start, weights, table, k_total, g, out, out_stride, len, depth,
                                              shift, st);
  if (access == 4)
    return mean_frames_lut_launch<E, 4, LUT>(ptr, start, weights, table, k_total, g, out, out_stride, len, depth,
                                             shift, st);
  return mean_frames_lut_launch<E, sizeof(E), LUT>(ptr, start, weights, table, k_total, g, out, out_stride, len, depth,
                                                   shift, st);
}

// ---- YUV: one chroma block of BY x BX pixels per lane ------------------------------------------
// Every source's block goes to RGB code values by yuv_to_rgb[16], each of its 3 * BY * BX values through
// lin into a 64-bit sum; the sums go back through the divide and enc, and the block's RGB to one U, one V
// and BY * BX lumas by the helpers the forwards' stores use.
struct YuvLutGeom {
  int64_t u_off, v_off;  // elements from a frame's first luma to its first U and V sample
  int y_pitch, c_pitch, c_step, h0, w0, depth, shift;
};

template <class E, int BY, int BX>
__global__ void __launch_bounds__(256) mean_frames_yuv_lut_kernel(const E* const* __restrict__ ptr,
                                                                  const int32_t* __restrict__ start,
                                                                  const int32_t* __restrict__ weights,
                                                                  const int32_t* __restrict__ table, int k_total,
                                                                  E* __restrict__ out, int64_t out_stride,
                                                                  const YuvLutGeom q, const rrin_yuv_coef coef) {
  extern __shared__ __attribute__((aligned(16))) int32_t lut_lds[];
  constexpr int P = BY * BX, LOG2P = P == 4 ? 2 : (P == 2 ? 1 : 0);
  const int maxval = (1 << q.depth) - 1, mid = 1 << (q.depth - 1);
  const int g = blockIdx.y;
  int s0, s;
  uint32_t wsum;
  if (!lut_group(start, weights, g, k_total, s0, s, wsum)) return;  // uniform: nothing is read or written
  lut_stage(lut_lds, table, 2 * (maxval + 1));
  const int32_t* lin = lut_lds;
  const int32_t* thr = lut_lds + (maxval + 1);
  const LutDiv div = lut_div(wsum);
  const E* const* src = ptr + s0;
  const int32_t* wt = weights + s0;
  E* o = out + (int64_t)g * out_stride;
  const int cw = q.w0 / BX, ch = q.h0 / BY;
  const int64_t blocks = (int64_t)cw * ch;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < blocks; i += (int64_t)gridDim.x * 256) {
    const int cy = (int)(i / cw), cx = (int)(i - (int64_t)cy * cw);
    const int64_t y_at = (int64_t)cy * BY * q.y_pitch + (int64_t)cx * BX;
    const int64_t c_at = (int64_t)cy * q.c_pitch + (int64_t)cx * q.c_step;
    uint64_t acc[P][3];
#pragma unroll
    for (int p = 0; p < P; ++p) acc[p][0] = acc[p][1] = acc[p][2] = 0;
    for (int k = 0; k < s; ++k) {
      const E* f = src[k];
      const uint32_t w = (uint32_t)wt[k];
      E ye[P];
#pragma unroll
      for (int p = 0; p < P; ++p) ye[p] = lut_load<E>(f + y_at + (int64_t)(p / BX) * q.y_pitch + p % BX);
      const int u = lut_sample(lut_load<E>(f + q.u_off + c_at), maxval, q.shift);
      const int v = lut_sample(lut_load<E>(f + q.v_off + c_at), maxval, q.shift);
#pragma unroll
      for (int p = 0; p < P; ++p) {
        int rgb[3];
        if constexpr (sizeof(E) == 1) yuv_to_rgb(coef, ye[p], u, v, rgb);
        else yuv_to_rgb16(coef, mid, maxval, lut_sample(ye[p], maxval, q.shift), u, v, rgb);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[p][c] += (uint64_t)w * (uint32_t)lin[rgb[c]];
      }
    }
    int sum[3] = {0, 0, 0};
#pragma unroll
    for (int p = 0; p < P; ++p) {
      int rgb[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        rgb[c] = lut_encode(thr, q.depth, (uint32_t)div(acc[p][c]));
        sum[c] += rgb[c];
      }
      int luma;
      if constexpr (sizeof(E) == 1) luma = rgb_to_luma(coef, rgb);
      else luma = rgb_to_luma16(coef, maxval, rgb);
      o[y_at + (int64_t)(p / BX) * q.y_pitch + p % BX] = (E)(luma << q.shift);
    }
    int cu, cv;
    if constexpr (sizeof(E) == 1) {
      cu = rgb_block_to_chroma<LOG2P>(coef.ur, coef.ug, coef.ub, sum);
      cv = rgb_block_to_chroma<LOG2P>(coef.vr, coef.vg, coef.vb, sum);
    } else {
      cu = rgb_block_to_chroma16<LOG2P>(coef.ur, coef.ug, coef.ub, mid, maxval, sum);
      cv = rgb_block_to_chroma16<LOG2P>(coef.vr, coef.vg, coef.vb, mid, maxval, sum);
    }
    o[q.u_off + c_at] = (E)(cu << q.shift);
    o[q.v_off + c_at] = (E)(cv << q.shift);
  }
}

template <class E, int BY, int BX>
int mean_frames_yuv_lut_launch(const void* const* ptr, const int32_t* start, const int32_t* weights,
                               const int32_t* table, int k_total, int g, void* out, int64_t out_stride,
                               const YuvLutGeom& q, const rrin_yuv_coef& coef, hipStream_t st) {
  int64_t blocks = ((int64_t)(q.w0 / BX) * (q.h0 / BY) + 255) / 256;
  const int64_t cap = (LUT_MAX_GROUPS + g - 1) / g;
  if (blocks > cap) blocks = cap;
  const size_t lds = sizeof(int32_t) * 2 * ((size_t)1 << q.depth);
  hipLaunchKernelGGL((mean_frames_yuv_lut_kernel<E, BY, BX>), dim3((unsigned)blocks, (unsigned)g), dim3(256), lds, st,
                     reinterpret_cast<const E* const*>(ptr), start, weights, table, k_total, static_cast<E*>(out),
                     out_stride, q, coef);
  return hip_code(hipGetLastError());
}

template <class E>
int mean_frames_yuv_lut_chroma(int chroma, const void* const* ptr, const int32_t* start, const int32_t* weights,
                               const int32_t* table, int k_total, int g, void* out, int64_t out_stride,
                               const YuvLutGeom& q, const rrin_yuv_coef& coef, hipStream_t st) {
  if (chroma == RRIN_CHROMA_420)
    return mean_frames_yuv_lut_launch<E, 2, 2>(ptr, start, weights, table, k_total, g, out, out_stride, q, coef, st);
  if (chroma == RRIN_CHROMA_422)
    return mean_frames_yuv_lut_launch<E, 1, 2>(ptr, start, weights, table, k_total, g, out, out_stride, q, coef, st);
  return mean_frames_yuv_lut_launch<E, 1, 1>(ptr, start, weights, table, k_total, g, out, out_stride, q, coef, st);
}
}  // namespace rrin

using namespace rrin;

extern "C" int rrin_mean_frames_lut(const void* const* frames, int32_t k, const int32_t* start, int32_t g, void* out,
                                    int64_t out_stride, int64_t len, int32_t depth, int32_t shift, int32_t access,
                                    const int32_t* weights, const int32_t* table, void* stream) {
  if (!frames || !start || !out || !weights) return RRIN_E_ARG;
  if (g < 1 || len < 1) return RRIN_E_SHAPE;
  if (depth < 8 || depth > 16 || shift < 0 || shift > 16 - depth) return RRIN_E_ARG;
  if (depth == 8 && shift != 0) return RRIN_E_ARG;
  // the table of a depth above 12 bits does not fit in LDS beside anything else: 2 * 2^13 * 4 B and up
  if (table && (depth > 12 || ((uintptr_t)table & 15))) return RRIN_E_ARG;
  const int esize = depth == 8 ? 1 : 2;
  if (access != esize && access != 4 && access != 16) return RRIN_E_ARG;
  if (((uintptr_t)frames & 7) || ((uintptr_t)start & 3) || ((uintptr_t)weights & 3)) return RRIN_E_ARG;
  // every group has 1..256 frames
  if (k < g || (int64_t)k > (int64_t)g * 256) return RRIN_E_ARG;
  // out and, between frames, out_stride keep every access of the chosen width aligned (an odd
  // 16-bit address fails here too: access >= 2)
  if ((uintptr_t)out % (unsigned)access) return RRIN_E_ARG;
  if (g > 1 && (out_stride < len || (out_stride * esize) % access)) return RRIN_E_ARG;
  if (g > 65535) return RRIN_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (esize == 1) {
    if (table)
      return mean_frames_lut_access<uint8_t, true>(access, frames, start, weights, table, k, g, out, out_stride, len,
                                                   depth, shift, st);
    return mean_frames_lut_access<uint8_t, false>(access, frames, start, weights, table, k, g, out, out_stride, len,
                                                  depth, shift, st);
  }
  if (table)
    return mean_frames_lut_access<uint16_t, true>(access, frames, start, weights, table, k, g, out, out_stride, len,
                                                  depth, shift, st);
  return mean_frames_lut_access<uint16_t, false>(access, frames, start, weights, table, k, g, out, out_stride, len,
                                                 depth, shift, st);
}

extern "C" int rrin_mean_frames_yuv_lut(const void* const* frames, int32_t k, const int32_t* start, int32_t g,
                                        void* out, int64_t out_stride, const rrin_yuv_planes* geom,
                                        const rrin_yuv_coef* coef, int32_t h0, int32_t w0, const int32_t* weights,
                                        const int32_t* table, void* stream) {
  if (!frames || !start || !out || !weights || !table || !geom || !coef) return RRIN_E_ARG;
  const int depth = geom->depth, shift = geom->shift;
  if (depth != 8 && depth != 10 && depth != 12) return RRIN_E_ARG;
  if (shift != 0 && (depth == 8 || shift != 16 - depth)) return RRIN_E_ARG;
  if ((geom->c_step != 1 && geom->c_step != 2) || !chroma_ok(geom->chroma)) return RRIN_E_ARG;
  if (int rc = depth == 8 ? yuv_coef_check(coef) : yuv_coef_check16(coef, depth)) return rc;
  if (((uintptr_t)frames & 7) || ((uintptr_t)start & 3) || ((uintptr_t)weights & 3) || ((uintptr_t)table & 15))
    return RRIN_E_ARG;
  const int esize = depth == 8 ? 1 : 2;
  if ((uintptr_t)out % (unsigned)esize) return RRIN_E_ARG;
  if (g < 1 || g > 65535) return RRIN_E_SHAPE;
  if (k < g || (int64_t)k > (int64_t)g * 256) return RRIN_E_ARG;
  // sizes and pitches as the YUV forwards take them; the planes of a frame in the order Y, U, V (NV12
  // order: V one element behind U), none inside another, and the frames of out apart
  if (int rc = yuv_sizes_check(geom->chroma, geom->c_step, out_stride, geom->y_pitch, geom->c_pitch, g, h0, w0))
    return rc;
  const int ch = geom->chroma == RRIN_CHROMA_420 ? h0 / 2 : h0, cw = geom->chroma == RRIN_CHROMA_444 ? w0 : w0 / 2;
  const int64_t y_span = (int64_t)(h0 - 1) * geom->y_pitch + w0;
  const int64_t c_span = (int64_t)(ch - 1) * geom->c_pitch + (int64_t)(cw - 1) * geom->c_step + 1;
  if (geom->u_off < y_span || geom->v_off <= geom->u_off) return RRIN_E_SHAPE;
  if (geom->c_step == 1 && geom->v_off < geom->u_off + c_span) return RRIN_E_SHAPE;
  if (g > 1 && out_stride < geom->v_off + c_span) return RRIN_E_SHAPE;
  const YuvLutGeom q{geom->u_off, geom->v_off, geom->y_pitch, geom->c_pitch, geom->c_step, h0, w0, depth, shift};
  hipStream_t st = (hipStream_t)stream;
  if (esize == 1)
    return mean_frames_yuv_lut_chroma<uint8_t>(geom->chroma, frames, start, weights, table, k, g, out, out_stride, q,
                                               *coef, st);
  return mean_frames_yuv_lut_chroma<uint16_t>(geom->chroma, frames, start, weights, table, k, g, out, out_stride, q,
                                              *coef, st);
}
