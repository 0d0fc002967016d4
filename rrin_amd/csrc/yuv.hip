// 8-bit YUV frames (4:2:0 NV12 / I420; by rrin_chroma also 4:2:2 and 4:4:4) straight into the Net buffer g16 (rrin_pack_g16_yuv_h8) and
// the standard coefficient sets (rrin_yuv_coef_std), and their siblings for 10- and 12-bit samples in
// 16-bit words (rrin_pack_g16_yuv16_h8, rrin_yuv_coef_std16).  The conversion itself is yuv.hpp; the
// way out is the FINAL head's store (glue_h8.hip).
#include <type_traits>

#include "h8.hpp"
#include "yuv.hpp"

namespace rrin {

__constant__ const U8ScaleTab kU8Scale{};

// pack_g16_u8_kernel (glue_h8.hip) with the RGB bytes computed from 4:2:0 planes: one workgroup
// per padded row and run of 256 pixels.  Of each frame the run's 256 luma bytes are loaded one
// per lane, and its 128 U and 128 V samples by lanes 0-127 and 128-255 (byte loads: a frame of a
// [n+1] stack starts at any address), into LDS; then every lane converts its pixel -- source
// pixel (max(y - top, 0), min(x, w0 - 1)), the chroma of its 2x2 block -- to RGB bytes in
// integers, through the LDS copy of the scale table, and writes the whole records
// pack_g16_u8_kernel writes.  MODE 0: fp32 records, 1: fp16, 2: split16 (hi and lo planes).
// CH (rrin_chroma) is the chroma block: 4:2:0 as above; 4:2:2 the same 128 + 128 samples from
// chroma row sy instead of sy >> 1; 4:4:4 one U and one V per pixel, 256 + 256 samples, each lane
// loading those of its own pixel (the run may then be odd: nothing here assumes an even np).
// src: the frame of both stacks that image img of g16 reads (img itself, or its pair through a map).
template <int MODE, int CH>
__device__ inline void pack_g16_yuv_body(const rrin_yuv420& f0, const rrin_yuv420& f1, const rrin_yuv_coef& k, int w0,
                                         int top, uint4* ghi, uint4* glo, int64_t img_stride, int64_t gp, int wp,
                                         int w, int src, int img) {
  __shared__ float s_tab[256];
  __shared__ uint8_t s_y[2][256];
  constexpr int kCW = CH == RRIN_CHROMA_444 ? 256 : 128;  // chroma samples of a run, per plane
  __shared__ uint8_t s_c[2][2][kCW];  // [frame][U, V][block of the run]
  const int tid = threadIdx.x;
  const int xs = blockIdx.x * 256, y = blockIdx.y;
  s_tab[tid] = kU8Scale.v[tid];
  const int sy = y > top ? y - top : 0;
  // xs < w0: w is w0 rounded up to a multiple m of 16, 32 or 64 (16 * flow_scale), so the right pad is
  // < m columns; xs < w is a multiple of 256, hence of m: xs <= w - m < w0.  np is even unless 4:4:4 (w0 odd)
  const int np = min(256, w0 - xs);
  const int cy = CH == RRIN_CHROMA_420 ? sy >> 1 : sy;
  const int which = tid >> 7, blk = tid & 127;
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const rrin_yuv420& s = f ? f1 : f0;
    const int64_t base = (int64_t)src * s.img_stride;
    if (tid < np) s_y[f][tid] = s.y[base + (int64_t)sy * s.y_pitch + xs + tid];
    if constexpr (CH == RRIN_CHROMA_444) {
      if (tid < np) {
        const int64_t c = base + (int64_t)cy * s.c_pitch + (int64_t)(xs + tid) * s.c_step;
        s_c[f][0][tid] = s.u[c];
        s_c[f][1][tid] = s.v[c];
      }
    } else if (2 * blk < np) {
      s_c[f][which][blk] = (which ? s.v : s.u)[base + (int64_t)cy * s.c_pitch + (xs / 2 + blk) * s.c_step];
    }
  }
  __syncthreads();
  const int x = xs + tid;
  if (x >= w) return;
  const int sx = min(x, w0 - 1) - xs;
  const int cx = CH == RRIN_CHROMA_444 ? sx : sx >> 1;
  int rgb0[3], rgb1[3];
  yuv_to_rgb(k, s_y[0][sx], s_c[0][0][cx], s_c[0][1][cx], rgb0);
  yuv_to_rgb(k, s_y[1][sx], s_c[1][0][cx], s_c[1][1][cx], rgb1);
  float a[3], b[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a[c] = s_tab[rgb0[c]];
    b[c] = s_tab[rgb1[c]];
  }
  const int64_t rec = (int64_t)img * img_stride + (int64_t)(y + 1) * wp + x + kH8PadLeft;
  if constexpr (MODE == 0) {
    ghi[rec] = f4rec(a[0], a[1], a[2], b[0]);
    ghi[rec + gp] = f4rec(b[1], b[2], 0.f, 0.f);
    ghi[rec + 2 * gp] = make_uint4(0u, 0u, 0u, 0u);
    ghi[rec + 3 * gp] = make_uint4(0u, 0u, 0u, 0u);
  } else {
    half8 hi = {}, lo = {};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      hi[c] = (_Float16)a[c];
      hi[3 + c] = (_Float16)b[c];
      lo[c] = lo_of(a[c], hi[c]);
      lo[3 + c] = lo_of(b[c], hi[3 + c]);
    }
    ghi[rec] = __builtin_bit_cast(uint4, hi);
    ghi[rec + gp] = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (MODE == 2) {
      glo[rec] = __builtin_bit_cast(uint4, lo);
      glo[rec + gp] = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

template <int MODE, int CH>
__global__ void __launch_bounds__(256) pack_g16_yuv_kernel(rrin_yuv420 f0, rrin_yuv420 f1, rrin_yuv_coef k, int w0,
                                                           int top, uint4* ghi, uint4* glo, int64_t img_stride,
                                                           int64_t gp, int wp, int w) {
  pack_g16_yuv_body<MODE, CH>(f0, f1, k, w0, top, ghi, glo, img_stride, gp, wp, w, blockIdx.z, blockIdx.z);
}

// The item form (ABI 25): image k of g16 reads frame pair_of(map, k, n_pairs) of both stacks (f1
// is f0 one frame on: pair map[k] of one [n_pairs + 1] stack).
template <int MODE, int CH>
__global__ void __launch_bounds__(256) pack_g16_yuv_items_kernel(rrin_yuv420 f0, rrin_yuv420 f1, rrin_yuv_coef k,
                                                                 int w0, int top, uint4* ghi, uint4* glo,
                                                                 int64_t img_stride, int64_t gp, int wp, int w,
                                                                 const int32_t* __restrict__ map, int n_pairs) {
  pack_g16_yuv_body<MODE, CH>(f0, f1, k, w0, top, ghi, glo, img_stride, gp, wp, w, pair_of(map, blockIdx.z, n_pairs),
                              blockIdx.z);
}

// pack_g16_yuv_kernel for planes of 16-bit words (rrin_yuv420_16; depth 10 or 12, maxv = 2^depth - 1):
// the same run of 256 pixels and the same staging with 2-byte loads (pitches and strides count
// words, so a frame starts at any even address), the samples min(word >> shift, maxv), the
// conversion at that depth (yuv_to_rgb16) and every RGB sample divided by maxv
// (sample_to_float: the IEEE division, as rrin_pack_g16_u16_h8) -- no table.  CH as there.
template <int MODE, int CH>
__device__ inline void pack_g16_yuv16_body(const rrin_yuv420_16& f0, const rrin_yuv420_16& f1, const rrin_yuv_coef& k,
                                           int w0, int top, uint4* ghi, uint4* glo, int64_t img_stride, int64_t gp,
                                           int wp, int w, int src, int img) {
  __shared__ uint16_t s_y[2][256];
  constexpr int kCW = CH == RRIN_CHROMA_444 ? 256 : 128;  // chroma samples of a run, per plane
  __shared__ uint16_t s_c[2][2][kCW];  // [frame][U, V][block of the run]
  const int tid = threadIdx.x;
  const int xs = blockIdx.x * 256, y = blockIdx.y;
  const int sy = y > top ? y - top : 0;
  // xs < w0: w is w0 rounded up to a multiple m of 16, 32 or 64 (16 * flow_scale), so the right pad is
  // < m columns; xs < w is a multiple of 256, hence of m: xs <= w - m < w0.  np is even unless 4:4:4 (w0 odd)
  const int np = min(256, w0 - xs);
  const int cy = CH == RRIN_CHROMA_420 ? sy >> 1 : sy;
  const int which = tid >> 7, blk = tid & 127;
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const rrin_yuv420_16& s = f ? f1 : f0;
    const int64_t base = (int64_t)src * s.img_stride;
    if (tid < np) s_y[f][tid] = s.y[base + (int64_t)sy * s.y_pitch + xs + tid];
    if constexpr (CH == RRIN_CHROMA_444) {
      if (tid < np) {
        const int64_t c = base + (int64_t)cy * s.c_pitch + (int64_t)(xs + tid) * s.c_step;
        s_c[f][0][tid] = s.u[c];
        s_c[f][1][tid] = s.v[c];
      }
    } else if (2 * blk < np) {
      s_c[f][which][blk] = (which ? s.v : s.u)[base + (int64_t)cy * s.c_pitch + (xs / 2 + blk) * s.c_step];
    }
  }
  __syncthreads();
  const int x = xs + tid;
  if (x >= w) return;
  const int sx = min(x, w0 - 1) - xs;
  const int cx = CH == RRIN_CHROMA_444 ? sx : sx >> 1;
  const int shift = f0.shift, maxv = (1 << f0.depth) - 1, mid = 1 << (f0.depth - 1);
  int rgb0[3], rgb1[3];
  yuv_to_rgb16(k, mid, maxv, sample16(s_y[0][sx], shift, maxv), sample16(s_c[0][0][cx], shift, maxv),
               sample16(s_c[0][1][cx], shift, maxv), rgb0);
  yuv_to_rgb16(k, mid, maxv, sample16(s_y[1][sx], shift, maxv), sample16(s_c[1][0][cx], shift, maxv),
               sample16(s_c[1][1][cx], shift, maxv), rgb1);
  const float mv = (float)maxv;
  float a[3], b[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a[c] = sample_to_float(rgb0[c], mv);
    b[c] = sample_to_float(rgb1[c], mv);
  }
  const int64_t rec = (int64_t)img * img_stride + (int64_t)(y + 1) * wp + x + kH8PadLeft;
  if constexpr (MODE == 0) {
    ghi[rec] = f4rec(a[0], a[1], a[2], b[0]);
    ghi[rec + gp] = f4rec(b[1], b[2], 0.f, 0.f);
    ghi[rec + 2 * gp] = make_uint4(0u, 0u, 0u, 0u);
    ghi[rec + 3 * gp] = make_uint4(0u, 0u, 0u, 0u);
  } else {
    half8 hi = {}, lo = {};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      hi[c] = (_Float16)a[c];
      hi[3 + c] = (_Float16)b[c];
      lo[c] = lo_of(a[c], hi[c]);
      lo[3 + c] = lo_of(b[c], hi[3 + c]);
    }
    ghi[rec] = __builtin_bit_cast(uint4, hi);
    ghi[rec + gp] = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (MODE == 2) {
      glo[rec] = __builtin_bit_cast(uint4, lo);
      glo[rec + gp] = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

template <int MODE, int CH>
__global__ void __launch_bounds__(256) pack_g16_yuv16_kernel(rrin_yuv420_16 f0, rrin_yuv420_16 f1, rrin_yuv_coef k,
                                                             int w0, int top, uint4* ghi, uint4* glo,
                                                             int64_t img_stride, int64_t gp, int wp, int w) {
  pack_g16_yuv16_body<MODE, CH>(f0, f1, k, w0, top, ghi, glo, img_stride, gp, wp, w, blockIdx.z, blockIdx.z);
}

template <int MODE, int CH>
__global__ void __launch_bounds__(256) pack_g16_yuv16_items_kernel(rrin_yuv420_16 f0, rrin_yuv420_16 f1,
                                                                   rrin_yuv_coef k, int w0, int top, uint4* ghi,
                                                                   uint4* glo, int64_t img_stride, int64_t gp, int wp,
                                                                   int w, const int32_t* __restrict__ map,
                                                                   int n_pairs) {
  pack_g16_yuv16_body<MODE, CH>(f0, f1, k, w0, top, ghi, glo, img_stride, gp, wp, w,
                                pair_of(map, blockIdx.z, n_pairs), blockIdx.z);
}

// the launch of a pack kernel K<MODE, CH> (K8 / K16 below; with a map its item form K::items) for a
// record precision and a chroma format
template <template <int, int> class K, class Stack>
static int launch_yuv_pack(int prec, int chroma, dim3 grid, hipStream_t st, const Stack& f0, const Stack& f1,
                           const rrin_yuv_coef& k, int w0, int top, const rrin_h8& g16, int w, const int32_t* map,
                           int n_pairs) {
  uint4* hi = static_cast<uint4*>(g16.hi);
  uint4* lo = planes_of(prec) == 2 ? static_cast<uint4*>(g16.lo) : nullptr;
  const int mode = prec == RRIN_PREC_F32R ? 0 : (planes_of(prec) == 2 ? 2 : 1);
  auto go = [&](auto kern, auto items) {
    if (map)
      hipLaunchKernelGGL(items, grid, dim3(256), 0, st, f0, f1, k, w0, top, hi, lo, g16.img_stride, g16.g.plane,
                         g16.g.wp, w, map, n_pairs);
    else
      hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, f0, f1, k, w0, top, hi, lo, g16.img_stride, g16.g.plane,
                         g16.g.wp, w);
    return hip_code(hipGetLastError());
  };
  auto by_chroma = [&](auto m) {
    constexpr int M = decltype(m)::value;
    if (chroma == RRIN_CHROMA_422) return go(K<M, RRIN_CHROMA_422>::fn, K<M, RRIN_CHROMA_422>::items);
    if (chroma == RRIN_CHROMA_444) return go(K<M, RRIN_CHROMA_444>::fn, K<M, RRIN_CHROMA_444>::items);
    return go(K<M, RRIN_CHROMA_420>::fn, K<M, RRIN_CHROMA_420>::items);
  };
  if (mode == 0) return by_chroma(std::integral_constant<int, 0>{});
  if (mode == 2) return by_chroma(std::integral_constant<int, 2>{});
  return by_chroma(std::integral_constant<int, 1>{});
}
template <int MODE, int CH>
struct K8 {
  static constexpr auto fn = pack_g16_yuv_kernel<MODE, CH>;
  static constexpr auto items = pack_g16_yuv_items_kernel<MODE, CH>;
};
template <int MODE, int CH>
struct K16 {
  static constexpr auto fn = pack_g16_yuv16_kernel<MODE, CH>;
  static constexpr auto items = pack_g16_yuv16_items_kernel<MODE, CH>;
};

}  // namespace rrin

using namespace rrin;

extern "C" int rrin_yuv_coef_std(int32_t standard, int32_t full_range, rrin_yuv_coef* c) {
  // round(x * 2^14) of the matrices of Kr / Kb = 0.2126 / 0.0722 (BT.709) and 0.299 / 0.114
  // (BT.601), luma scaled by 219/255 and chroma by 224/255 for limited range; yg, ug, vg are
  // the remainders (rrin_hip.h)
  static const rrin_yuv_coef kStd[2][2] = {
      {{16, 19077, 29372, -3494, -8731, 34610, 2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660},
       {0, 16384, 25802, -3069, -7670, 30402, 3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751}},
      {{16, 19077, 26149, -6419, -13320, 33050, 4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170},
       {0, 16384, 22970, -5638, -11700, 29032, 4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332}}};
  if (!c || (standard != RRIN_YUV_BT709 && standard != RRIN_YUV_BT601)) return RRIN_E_ARG;
  *c = kStd[standard][full_range ? 1 : 0];
  return 0;
}

// rrin_pack_g16_yuv_h8 for n images that read the frames of n_pairs pairs through the device map
// (NULL: image k reads frame k, n_pairs == n); the stacks are checked for their n_pairs frames
int rrin::pack_g16_yuv_items(const rrin_yuv420* f0, const rrin_yuv420* f1, const rrin_yuv_coef* coef, int32_t n,
                             int32_t h0, int32_t w0, const rrin_h8* g16, int32_t prec, const int32_t* map,
                             int32_t n_pairs, hipStream_t stream, int32_t mult) {
  if (!f0 || !f1 || !g16 || n < 1 || !rec_prec(prec)) return RRIN_E_ARG;
  if (n_pairs < 1 || n_pairs > n || (!map && n_pairs != n)) return RRIN_E_ARG;
  if (int rc = yuv_coef_check(coef)) return rc;
  if (int rc = yuv420_check(*f0, n_pairs, h0, w0)) return rc;
  if (int rc = yuv420_check(*f1, n_pairs, h0, w0)) return rc;
  if (f0->chroma != f1->chroma) return RRIN_E_ARG;
  if (!h8_ok(*g16, prec) || g16->g_off != 0 || g16->groups * chans_per_rec(prec) < 16) return RRIN_E_SHAPE;
  const int h = g16->g.h, w = g16->g.w;
  if (h != pad_up(h0, mult) || w != pad_up(w0, mult)) return RRIN_E_SHAPE;
  if (n > 65535 || h > 65535) return RRIN_E_SHAPE;  // grid y / z
  const dim3 grid((w + 255) / 256, h, n);
  const int top = h - h0;
  return launch_yuv_pack<K8>(prec, f0->chroma, grid, stream, *f0, *f1, *coef, w0, top, *g16, w, map, n_pairs);
}

extern "C" int rrin_pack_g16_yuv_h8(const rrin_yuv420* f0, const rrin_yuv420* f1, const rrin_yuv_coef* coef,
                                    int32_t n, int32_t h0, int32_t w0, const rrin_h8* g16, int32_t prec,
                                    void* stream) {
  return pack_g16_yuv_items(f0, f1, coef, n, h0, w0, g16, prec, nullptr, n, (hipStream_t)stream);
}

extern "C" int rrin_yuv_coef_std16(int32_t standard, int32_t full_range, int32_t depth, rrin_yuv_coef* c) {
  if (!c || (standard != RRIN_YUV_BT709 && standard != RRIN_YUV_BT601) || depth < 8 || depth > 16) return RRIN_E_ARG;
  // rrin_amd.yuv.coefficients in the same double operations, rounded half to even as Python rounds
  const double kr = standard == RRIN_YUV_BT709 ? 0.2126 : 0.299, kb = standard == RRIN_YUV_BT709 ? 0.0722 : 0.114;
  const double kg = 1.0 - kr - kb;
  const double up = (double)(1 << (depth - 8)), maxval = (double)((1 << depth) - 1);
  const double ys = full_range ? 1.0 : 219.0 * up / maxval, cs = full_range ? 1.0 : 224.0 * up / maxval;
  auto q = [](double x) { return (int32_t)__builtin_nearbyint(x * 16384.0); };
  c->y0 = full_range ? 0 : 16 << (depth - 8);
  c->ay = q(1.0 / ys);
  c->rv = q(2 * (1 - kr) / cs);
  c->gu = q(-2 * (1 - kb) * kb / kg / cs);
  c->gv = q(-2 * (1 - kr) * kr / kg / cs);
  c->bu = q(2 * (1 - kb) / cs);
  c->yr = q(kr * ys);
  c->yb = q(kb * ys);
  c->yg = q(ys) - c->yr - c->yb;
  c->ur = q(-kr / (2 * (1 - kb)) * cs);
  c->ub = q(0.5 * cs);
  c->ug = -(c->ur + c->ub);
  c->vr = q(0.5 * cs);
  c->vb = q(-kb / (2 * (1 - kr)) * cs);
  c->vg = -(c->vr + c->vb);
  return 0;
}

int rrin::pack_g16_yuv16_items(const rrin_yuv420_16* f0, const rrin_yuv420_16* f1, const rrin_yuv_coef* coef,
                               int32_t n, int32_t h0, int32_t w0, const rrin_h8* g16, int32_t prec,
                               const int32_t* map, int32_t n_pairs, hipStream_t stream, int32_t mult) {
  if (!f0 || !f1 || !g16 || n < 1 || !rec_prec(prec)) return RRIN_E_ARG;
  if (n_pairs < 1 || n_pairs > n || (!map && n_pairs != n)) return RRIN_E_ARG;
  if (int rc = yuv420_16_check(*f0, n_pairs, h0, w0)) return rc;
  if (int rc = yuv420_16_check(*f1, n_pairs, h0, w0)) return rc;
  if (f0->depth != f1->depth || f0->shift != f1->shift || f0->chroma != f1->chroma) return RRIN_E_ARG;
  if (int rc = yuv_coef_check16(coef, f0->depth)) return rc;
  if (!h8_ok(*g16, prec) || g16->g_off != 0 || g16->groups * chans_per_rec(prec) < 16) return RRIN_E_SHAPE;
  const int h = g16->g.h, w = g16->g.w;
  if (h != pad_up(h0, mult) || w != pad_up(w0, mult)) return RRIN_E_SHAPE;
  if (n > 65535 || h > 65535) return RRIN_E_SHAPE;  // grid y / z
  const dim3 grid((w + 255) / 256, h, n);
  const int top = h - h0;
  return launch_yuv_pack<K16>(prec, f0->chroma, grid, stream, *f0, *f1, *coef, w0, top, *g16, w, map, n_pairs);
}

extern "C" int rrin_pack_g16_yuv16_h8(const rrin_yuv420_16* f0, const rrin_yuv420_16* f1, const rrin_yuv_coef* coef,
                                      int32_t n, int32_t h0, int32_t w0, const rrin_h8* g16, int32_t prec,
                                      void* stream) {
  return pack_g16_yuv16_items(f0, f1, coef, n, h0, w0, g16, prec, nullptr, n, (hipStream_t)stream);
}
