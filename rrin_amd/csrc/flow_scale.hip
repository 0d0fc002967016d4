// Low-resolution flow estimation (flow_scale s = 2 or 4; rrin_amd/flowscale.py is the definition):
// the two glue kernels around the Flow U-Net of a plan at (H/s, W/s), each written once over a
// record format F (rec_fmt.hpp) and instantiated for RecH8<1>, RecH8<2> and RecR32.
//   rrin_g16_downscale_h8  F.avg_pool2d(x, s) of channels 0-5 of the full-size Net buffer g16 into
//                          the low-res plan's g16 (channels 6-15 zeroed)
//   rrin_flow_upscale_h8   s * F.interpolate(flow, scale_factor=s, bilinear, align_corners=False)
//                          of the low-res plan's raw Flow into the full-size plan's
// Both are memory-bound: one thread per output pixel, x fastest, so a wave's stores (and the
// upscale's loads) are runs of consecutive 16-B records of one row.  The downscale reads s
// consecutive records per lane and row, one per load instruction: a single load of a wave touches
// records 16 s bytes apart and uses 1 / s of each line it fetches, the rest is served from cache
// by the lane's next s - 1 loads of that row; over those s loads the wave covers 64 s records
// without a gap, so every byte is fetched from memory once.  Measured alone: DESIGN.md §6c.
#include "rec_fmt.hpp"

namespace rrin {

// One thread per low-res pixel (y, x) of image img: the S x S block of full-size pixels at
// (S*y, S*x), channels 0-5, summed in fp32 in raster order and scaled by 1 / S^2 (exact: a power
// of two), stored with the format's rounding as whole records with channels 6-15 zero.  Only
// interior records of dst are written.
template <class F, int S>
__global__ void __launch_bounds__(256) g16_downscale_kernel(RecView s, RecView d, int lh, int lw, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % lw);
  const int64_t t = i / lw;
  const int y = (int)(t % lh);
  const int img = (int)(t / lh);
  float acc[6];
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < S; ++r) {
      const int64_t row = s.rec(img, 0, S * y + r, S * x);
#pragma unroll
      for (int c = 0; c < S; ++c) {
        float p[8];
        F::load8(s, row + c, p);
#pragma unroll
        for (int e = 0; e < 6; ++e) acc[e] = (r == 0 && c == 0) ? p[e] : acc[e] + p[e];
      }
    }
  }
  float v[16] = {};
#pragma unroll
  for (int e = 0; e < 6; ++e) v[e] = acc[e] * (1.0f / (S * S));
  const int64_t rec = d.rec(img, 0, y, x);
#pragma unroll
  for (int k = 0; k < 16 / F::kChans; ++k) F::store_rec(d, rec + k * d.gp, v + k * F::kChans);
}

// One thread per full-size pixel (y, x): source coordinate (dst + 0.5) / S - 0.5 clamped at 0
// = num / (2 S) with num = max(2 dst + 1 - S, 0), so the index is num / (2 S) and the weight
// (num % (2 S)) / (2 S), an exact dyadic number; the second tap clamps to the last row / column.
// Four record loads (channels 0-3 are the raw Flow), the pinned fp32 arithmetic without
// contraction, times S, one whole-record store (the record's other channels zero).
template <class F, int S>
__global__ void __launch_bounds__(256) flow_upscale_kernel(RecView s, int lh, int lw, RecView d, int64_t total,
                                                           int* status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int w = S * lw, h = S * lh;
  const int x = (int)(i % w);
  const int64_t t = i / w;
  const int y = (int)(t % h);
  const int img = (int)(t / h);
  const int ny = max(2 * y + 1 - S, 0), nx = max(2 * x + 1 - S, 0);
  const int y0 = ny / (2 * S), x0 = nx / (2 * S);
  const int y1 = min(y0 + 1, lh - 1), x1 = min(x0 + 1, lw - 1);
  const float wy = (float)(ny % (2 * S)) * (0.5f / S), wx = (float)(nx % (2 * S)) * (0.5f / S);
  const int64_t rr[4] = {s.rec(img, 0, y0, x0), s.rec(img, 0, y0, x1), s.rec(img, 0, y1, x0), s.rec(img, 0, y1, x1)};
  float p[4][F::kChans];
#pragma unroll
  for (int k = 0; k < 4; ++k) F::load_rec(s, rr[k], p[k]);
  float o[F::kChans] = {};
  {
#pragma clang fp contract(off)
    const float uy = 1.0f - wy, ux = 1.0f - wx;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float top = ux * p[0][e] + wx * p[1][e];
      const float bot = ux * p[2][e] + wx * p[3][e];
      const float v = uy * top + wy * bot;
      o[e] = v * (float)S;
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) F::check_range(status, o[e]);
  F::store_rec(d, d.rec(img, 0, y, x), o);
}

}  // namespace rrin

using namespace rrin;

// src and dst of a scale step: dst.g * s == src.g for the downscale (the exact quotient)
static int scale_check(const rrin_h8* big, const rrin_h8* small, int32_t n, int32_t s, int32_t prec, int chans) {
  if (!big || !small || n < 1 || !rec_prec(prec) || (s != 2 && s != 4)) return RRIN_E_ARG;
  if (!h8_ok(*big, prec) || !h8_ok(*small, prec)) return RRIN_E_SHAPE;
  if (big->g_off != 0 || small->g_off != 0) return RRIN_E_SHAPE;
  if (small->g.h < 1 || small->g.w < 1 || (int64_t)small->g.h * s != big->g.h || (int64_t)small->g.w * s != big->g.w)
    return RRIN_E_SHAPE;
  if (big->groups * chans_per_rec(prec) < chans || small->groups * chans_per_rec(prec) < chans) return RRIN_E_SHAPE;
  return 0;
}

extern "C" int rrin_g16_downscale_h8(const rrin_h8* src, const rrin_h8* dst, int32_t n, int32_t s, int32_t prec,
                                     void* stream) {
  if (int rc = scale_check(src, dst, n, s, prec, 16)) return rc;
  const int lh = dst->g.h, lw = dst->g.w;
  const int64_t total = (int64_t)n * lh * lw;
  if ((total + 255) / 256 > 0x7fffffff) return RRIN_E_SHAPE;
  const int grid = (int)((total + 255) / 256);
  return with_format(prec, [&](auto f) {
    using F = decltype(f);
    if (s == 2)
      hipLaunchKernelGGL((g16_downscale_kernel<F, 2>), dim3(grid), dim3(256), 0, (hipStream_t)stream, rec_view(*src),
                         rec_view(*dst), lh, lw, total);
    else
      hipLaunchKernelGGL((g16_downscale_kernel<F, 4>), dim3(grid), dim3(256), 0, (hipStream_t)stream, rec_view(*src),
                         rec_view(*dst), lh, lw, total);
    return hip_code(hipGetLastError());
  });
}

extern "C" int rrin_flow_upscale_h8(const rrin_h8* src, const rrin_h8* dst, int32_t n, int32_t s, int32_t prec,
                                    int32_t* status, void* stream) {
  if (int rc = scale_check(dst, src, n, s, prec, 4)) return rc;
  const int lh = src->g.h, lw = src->g.w;
  const int64_t total = (int64_t)n * dst->g.h * dst->g.w;
  if ((total + 255) / 256 > 0x7fffffff) return RRIN_E_SHAPE;
  const int grid = (int)((total + 255) / 256);
  return with_format(prec, [&](auto f) {
    using F = decltype(f);
    if (s == 2)
      hipLaunchKernelGGL((flow_upscale_kernel<F, 2>), dim3(grid), dim3(256), 0, (hipStream_t)stream, rec_view(*src), lh,
                         lw, rec_view(*dst), total, status);
    else
      hipLaunchKernelGGL((flow_upscale_kernel<F, 4>), dim3(grid), dim3(256), 0, (hipStream_t)stream, rec_view(*src), lh,
                         lw, rec_view(*dst), total, status);
    return hip_code(hipGetLastError());
  });
}
