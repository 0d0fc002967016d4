// 8-bit YUV 4:2:0 frames (NV12 / I420) straight into the Net buffer g16 (rrin_pack_g16_yuv_h8) and
// the standard coefficient sets (rrin_yuv_coef_std), and their siblings for 10- and 12-bit samples in
// 16-bit words (rrin_pack_g16_yuv16_h8, rrin_yuv_coef_std16).  The conversion itself is yuv.hpp; the
// way out is the FINAL head's store (glue_h8.hip).
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
template <int MODE>
__global__ void __launch_bounds__(256) pack_g16_yuv_kernel(rrin_yuv420 f0, rrin_yuv420 f1, rrin_yuv_coef k, int w0,
                                                           int top, uint4* ghi, uint4* glo, int64_t img_stride,
                                                           int64_t gp, int wp, int w) {
  __shared__ float s_tab[256];
  __shared__ uint8_t s_y[2][256];
  __shared__ uint8_t s_c[2][2][128];  // [frame][U, V][block of the run]
  const int tid = threadIdx.x;
  const int xs = blockIdx.x * 256, y = blockIdx.y, img = blockIdx.z;
  s_tab[tid] = kU8Scale.v[tid];
  const int sy = y > top ? y - top : 0;
  const int np = min(256, w0 - xs);  // xs < w0: the right pad is < 16 columns, xs a multiple of 256; np is even
  const int which = tid >> 7, blk = tid & 127;
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const rrin_yuv420& s = f ? f1 : f0;
    const int64_t base = (int64_t)img * s.img_stride;
    if (tid < np) s_y[f][tid] = s.y[base + (int64_t)sy * s.y_pitch + xs + tid];
    if (2 * blk < np)
      s_c[f][which][blk] = (which ? s.v : s.u)[base + (int64_t)(sy >> 1) * s.c_pitch + (xs / 2 + blk) * s.c_step];
  }
  __syncthreads();
  const int x = xs + tid;
  if (x >= w) return;
  const int sx = min(x, w0 - 1) - xs;
  int rgb0[3], rgb1[3];
  yuv_to_rgb(k, s_y[0][sx], s_c[0][0][sx >> 1], s_c[0][1][sx >> 1], rgb0);
  yuv_to_rgb(k, s_y[1][sx], s_c[1][0][sx >> 1], s_c[1][1][sx >> 1], rgb1);
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

// pack_g16_yuv_kernel for planes of 16-bit words (rrin_yuv420_16; depth 10 or 12, maxv = 2^depth - 1):
// the same run of 256 pixels and the same staging with 2-byte loads (pitches and strides count
// words, so a frame starts at any even address), the samples min(word >> shift, maxv), the
// conversion at that depth (yuv_to_rgb16) and every RGB sample divided by maxv
// (sample_to_float: the IEEE division, as rrin_pack_g16_u16_h8) -- no table.
template <int MODE>
__global__ void __launch_bounds__(256) pack_g16_yuv16_kernel(rrin_yuv420_16 f0, rrin_yuv420_16 f1, rrin_yuv_coef k,
                                                             int w0, int top, uint4* ghi, uint4* glo,
                                                             int64_t img_stride, int64_t gp, int wp, int w) {
  __shared__ uint16_t s_y[2][256];
  __shared__ uint16_t s_c[2][2][128];  // [frame][U, V][block of the run]
  const int tid = threadIdx.x;
  const int xs = blockIdx.x * 256, y = blockIdx.y, img = blockIdx.z;
  const int sy = y > top ? y - top : 0;
  const int np = min(256, w0 - xs);  // xs < w0: the right pad is < 16 columns, xs a multiple of 256; np is even
  const int which = tid >> 7, blk = tid & 127;
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const rrin_yuv420_16& s = f ? f1 : f0;
    const int64_t base = (int64_t)img * s.img_stride;
    if (tid < np) s_y[f][tid] = s.y[base + (int64_t)sy * s.y_pitch + xs + tid];
    if (2 * blk < np)
      s_c[f][which][blk] = (which ? s.v : s.u)[base + (int64_t)(sy >> 1) * s.c_pitch + (xs / 2 + blk) * s.c_step];
  }
  __syncthreads();
  const int x = xs + tid;
  if (x >= w) return;
  const int sx = min(x, w0 - 1) - xs;
  const int shift = f0.shift, maxv = (1 << f0.depth) - 1, mid = 1 << (f0.depth - 1);
  int rgb0[3], rgb1[3];
  yuv_to_rgb16(k, mid, maxv, sample16(s_y[0][sx], shift, maxv), sample16(s_c[0][0][sx >> 1], shift, maxv),
               sample16(s_c[0][1][sx >> 1], shift, maxv), rgb0);
  yuv_to_rgb16(k, mid, maxv, sample16(s_y[1][sx], shift, maxv), sample16(s_c[1][0][sx >> 1], shift, maxv),
               sample16(s_c[1][1][sx >> 1], shift, maxv), rgb1);
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

extern "C" int rrin_pack_g16_yuv_h8(const rrin_yuv420* f0, const rrin_yuv420* f1, const rrin_yuv_coef* coef,
                                    int32_t n, int32_t h0, int32_t w0, const rrin_h8* g16, int32_t prec,
                                    void* stream) {
  if (!f0 || !f1 || !g16 || n < 1 || !rec_prec(prec)) return RRIN_E_ARG;
  if (int rc = yuv_coef_check(coef)) return rc;
  if (int rc = yuv420_check(*f0, n, h0, w0)) return rc;
  if (int rc = yuv420_check(*f1, n, h0, w0)) return rc;
  if (!h8_ok(*g16, prec) || g16->g_off != 0 || g16->groups * chans_per_rec(prec) < 16) return RRIN_E_SHAPE;
  const int h = g16->g.h, w = g16->g.w;
  if (h != (h0 + 15) / 16 * 16 || w != (w0 + 15) / 16 * 16) return RRIN_E_SHAPE;
  if (n > 65535 || h > 65535) return RRIN_E_SHAPE;  // grid y / z
  const dim3 grid((w + 255) / 256, h, n);
  const int top = h - h0;
  hipStream_t st = (hipStream_t)stream;
  if (prec == RRIN_PREC_F32R)
    hipLaunchKernelGGL(pack_g16_yuv_kernel<0>, grid, dim3(256), 0, st, *f0, *f1, *coef, w0, top,
                       static_cast<uint4*>(g16->hi), (uint4*)nullptr, g16->img_stride, g16->g.plane, g16->g.wp, w);
  else if (planes_of(prec) == 2)
    hipLaunchKernelGGL(pack_g16_yuv_kernel<2>, grid, dim3(256), 0, st, *f0, *f1, *coef, w0, top,
                       static_cast<uint4*>(g16->hi), static_cast<uint4*>(g16->lo), g16->img_stride, g16->g.plane,
                       g16->g.wp, w);
  else
    hipLaunchKernelGGL(pack_g16_yuv_kernel<1>, grid, dim3(256), 0, st, *f0, *f1, *coef, w0, top,
                       static_cast<uint4*>(g16->hi), (uint4*)nullptr, g16->img_stride, g16->g.plane, g16->g.wp, w);
  return hip_code(hipGetLastError());
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

extern "C" int rrin_pack_g16_yuv16_h8(const rrin_yuv420_16* f0, const rrin_yuv420_16* f1, const rrin_yuv_coef* coef,
                                      int32_t n, int32_t h0, int32_t w0, const rrin_h8* g16, int32_t prec,
                                      void* stream) {
  if (!f0 || !f1 || !g16 || n < 1 || !rec_prec(prec)) return RRIN_E_ARG;
  if (int rc = yuv420_16_check(*f0, n, h0, w0)) return rc;
  if (int rc = yuv420_16_check(*f1, n, h0, w0)) return rc;
  if (f0->depth != f1->depth || f0->shift != f1->shift) return RRIN_E_ARG;
  if (int rc = yuv_coef_check16(coef, f0->depth)) return rc;
  if (!h8_ok(*g16, prec) || g16->g_off != 0 || g16->groups * chans_per_rec(prec) < 16) return RRIN_E_SHAPE;
  const int h = g16->g.h, w = g16->g.w;
  if (h != (h0 + 15) / 16 * 16 || w != (w0 + 15) / 16 * 16) return RRIN_E_SHAPE;
  if (n > 65535 || h > 65535) return RRIN_E_SHAPE;  // grid y / z
  const dim3 grid((w + 255) / 256, h, n);
  const int top = h - h0;
  hipStream_t st = (hipStream_t)stream;
  if (prec == RRIN_PREC_F32R)
    hipLaunchKernelGGL(pack_g16_yuv16_kernel<0>, grid, dim3(256), 0, st, *f0, *f1, *coef, w0, top,
                       static_cast<uint4*>(g16->hi), (uint4*)nullptr, g16->img_stride, g16->g.plane, g16->g.wp, w);
  else if (planes_of(prec) == 2)
    hipLaunchKernelGGL(pack_g16_yuv16_kernel<2>, grid, dim3(256), 0, st, *f0, *f1, *coef, w0, top,
                       static_cast<uint4*>(g16->hi), static_cast<uint4*>(g16->lo), g16->img_stride, g16->g.plane,
                       g16->g.wp, w);
  else
    hipLaunchKernelGGL(pack_g16_yuv16_kernel<1>, grid, dim3(256), 0, st, *f0, *f1, *coef, w0, top,
                       static_cast<uint4*>(g16->hi), (uint4*)nullptr, g16->img_stride, g16->g.plane, g16->g.wp, w);
  return hip_code(hipGetLastError());
}
