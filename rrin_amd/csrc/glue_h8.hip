// Every non-conv kernel of the record path (layouts in h8.hpp), each with its entry point:
// NCHW <-> records (rrin_nchw_to_h8 / rrin_h8_to_nchw), the frame pair into the Net buffer g16
// from fp32 or uint8 frames (rrin_pack_g16_h8 / rrin_pack_g16_u8_h8), nn.Upsample(bilinear, x2)
// (unet.py:77) as its own pass (rrin_upsample2x_h8), the head convs (Cout <= 4) fused with the
// model.py glue they feed (rrin_head_h8_fwd; the arithmetic itself in net_glue.hpp; the FINAL
// head also stores 8-bit frames, interleaved RGB or 4:2:0 planes through yuv.hpp), and the
// t-blend of a kept raw flow (rrin_flow_tblend_h8).  H8 kernels for F16X3 / F16, *_r32 kernels
// for the fp32 records.
#include <string.h>

#include "h8.hpp"
#include "net_glue.hpp"
#include "yuv.hpp"

namespace rrin {

// ---- bilinear x2 upsample pass (unet.py:77, align_corners=False) -------------
template <int PLANES>
__global__ void up2x_h8_kernel(const uint4* __restrict__ s_hi, const uint4* __restrict__ s_lo, int64_t s_img,
                               int64_t s_gp, int s_wp, int sh, int sw, uint4* d_hi, uint4* d_lo, int64_t d_img,
                               int64_t d_gp, int d_wp, int groups, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int w = 2 * sw, h = 2 * sh;
  const int x = (int)(i % w);
  int64_t t = i / w;
  const int y = (int)(t % h);
  t /= h;
  const int g = (int)(t % groups);
  const int img = (int)(t / groups);
  // Y even (2i): 0.25 row(i-1) + 0.75 row(i); odd: 0.75 row(i) + 0.25 row(i+1); edges clamp
  int ra, rb, ca, cb;
  float wa, wc;
  if (y & 1) { ra = y >> 1; rb = min(ra + 1, sh - 1); wa = 0.75f; }
  else { rb = y >> 1; ra = max(rb - 1, 0); wa = 0.25f; }
  if (x & 1) { ca = x >> 1; cb = min(ca + 1, sw - 1); wc = 0.75f; }
  else { cb = x >> 1; ca = max(cb - 1, 0); wc = 0.25f; }
  const float wb = 1.0f - wa, wd = 1.0f - wc;
  const int64_t base = img * s_img + g * s_gp;
  const int64_t r00 = base + (int64_t)(ra + 1) * s_wp + ca + kH8PadLeft;
  const int64_t r01 = base + (int64_t)(ra + 1) * s_wp + cb + kH8PadLeft;
  const int64_t r10 = base + (int64_t)(rb + 1) * s_wp + ca + kH8PadLeft;
  const int64_t r11 = base + (int64_t)(rb + 1) * s_wp + cb + kH8PadLeft;
  half8 q[4][PLANES];
  const int64_t rr[4] = {r00, r01, r10, r11};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    q[k][0] = __builtin_bit_cast(half8, s_hi[rr[k]]);
    if constexpr (PLANES == 2) q[k][1] = __builtin_bit_cast(half8, s_lo[rr[k]]);
  }
  half8 ohi, olo;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = PLANES == 2 ? join(q[k][0][e], q[k][PLANES - 1][e]) : (float)q[k][0][e];
    // horizontal first, then vertical (upsample_bilinear2d order)
    const float top = wc * v[0] + wd * v[1];
    const float bot = wc * v[2] + wd * v[3];
    const float o = wa * top + wb * bot;
    ohi[e] = (_Float16)o;
    olo[e] = lo_of(o, ohi[e]);
  }
  const int64_t drec = img * d_img + g * d_gp + (int64_t)(y + 1) * d_wp + x + kH8PadLeft;
  d_hi[drec] = __builtin_bit_cast(uint4, ohi);
  if constexpr (PLANES == 2) d_lo[drec] = __builtin_bit_cast(uint4, olo);
}

// ---- layout kernels ------------------------------------------------------------
__global__ void nchw_to_h8_kernel(const float* __restrict__ src, _Float16* hi, _Float16* lo, int64_t img_stride,
                                  int64_t gp, int wp, int ch_off, int c, int h, int w, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w);
  int64_t t = i / w;
  const int y = (int)(t % h);
  t /= h;
  const int ch = (int)(t % c);
  const int n = (int)(t / c);
  const float v = src[i];
  const int64_t k = h8_half_index(img_stride, gp, wp, n, ch_off + ch, y, x);
  const _Float16 vh = (_Float16)v;
  hi[k] = vh;
  if (lo) lo[k] = lo_of(v, vh);
}

template <int PLANES>
__global__ void pack_g16_h8_kernel(const float* __restrict__ i0, const float* __restrict__ i1, uint4* ghi,
                                   uint4* glo, int64_t img_stride, int64_t gp, int wp, int h, int w,
                                   int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w);
  const int64_t t = i / w;
  const int y = (int)(t % h);
  const int img = (int)(t / h);
  const int64_t hw = (int64_t)h * w;
  const int64_t px = (int64_t)img * 3 * hw + (int64_t)y * w + x;
  half8 hi = {}, lo = {};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float a = i0[px + c * hw], b = i1[px + c * hw];
    hi[c] = (_Float16)a;
    hi[3 + c] = (_Float16)b;
    lo[c] = lo_of(a, hi[c]);
    lo[3 + c] = lo_of(b, hi[3 + c]);
  }
  const int64_t rec = (int64_t)img * img_stride + (int64_t)(y + 1) * wp + x + kH8PadLeft;
  ghi[rec] = __builtin_bit_cast(uint4, hi);
  ghi[rec + gp] = make_uint4(0u, 0u, 0u, 0u);
  if constexpr (PLANES == 2) {
    glo[rec] = __builtin_bit_cast(uint4, lo);
    glo[rec + gp] = make_uint4(0u, 0u, 0u, 0u);
  }
}

__global__ void h8_to_nchw_kernel(const _Float16* __restrict__ hi, const _Float16* __restrict__ lo, int64_t img_stride,
                                  int64_t gp, int wp, int ch_off, float* dst, int c, int h, int w, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w);
  int64_t t = i / w;
  const int y = (int)(t % h);
  t /= h;
  const int ch = (int)(t % c);
  const int n = (int)(t / c);
  const int64_t k = h8_half_index(img_stride, gp, wp, n, ch_off + ch, y, x);
  dst[i] = lo ? join(hi[k], lo[k]) : (float)hi[k];
}

// ---- head conv (Cout <= 4) + Net glue on the H8 Net buffer --------------------
struct HeadH8Args {
  const uint4* src_hi;
  const uint4* src_lo;
  int64_t src_img, src_gp;
  int src_wp;
  _Float16* g_hi;  // g16: 2 groups
  _Float16* g_lo;
  int64_t g_img, g_gp;
  int g_wp;
  const float* w;
  const float* bias;
  const float* coef;
  float* out;
  _Float16* fr_hi;  // FLOW: raw output (1 group), nullable
  _Float16* fr_lo;
  int64_t fr_img, fr_gp;
  int fr_wp;
  int h, w_, tiles_x, tiles_y;
  uint4* g32;       // F32R: g16 as 4 records of 4 fp32 channels (g_img / g_gp / g_wp in records)
  uint4* fr32;      // F32R: raw Flow output, 1 record (nullable)
  float* raw;       // optional: head conv output before the glue, NCHW [n][COUT][h][w]
  int* status;      // optional fp16 range flag: glue stores set it, FINAL poisons on it
  uint8_t* out8;    // FINAL, optional: uint8 [n][h0][w0][3] crop (rows top .. top + h0 - 1, columns < w0)
  int h0, w0, top;
  // FINAL, optional (the YUV kernels only): the same crop as 4:2:0 planes (rrin_head_h8_desc.out_yuv)
  uint8_t* oy;
  uint8_t* ou;
  uint8_t* ov;
  int64_t o_img;
  int oy_pitch, oc_pitch, oc_step;
  rrin_yuv_coef yc;
};

// The byte of a clamped FINAL value: (uint8)(q * 255.0f) -- one fp32 multiply, truncation toward
// zero, as t.mul(255).to(torch.uint8); 0 for a poisoned pixel (fp16 range guard).
__device__ inline uint8_t final_byte(float q, bool poison) { return poison ? (uint8_t)0 : (uint8_t)(q * 255.0f); }

// FINAL with a uint8 output: the clamped pixel q of padded position (y, x) as three interleaved
// bytes (final_byte) of the crop.  Pixels of the padding (rows above top, columns from w0) are not
// written.
__device__ inline void final_store_u8(const HeadH8Args& a, int img, int y, int x, const float* q, bool poison) {
  const int yo = y - a.top;
  if (yo < 0 || yo >= a.h0 || x >= a.w0) return;
  uint8_t* o = a.out8 + (((int64_t)img * a.h0 + yo) * a.w0 + x) * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) o[ch] = final_byte(q[ch], poison);
}

// FINAL with a 4:2:0 output: a thread's two vertically adjacent pixels (rows y, y + 1, y even;
// rgb: their RGB bytes) and those of its xl ^ 1 neighbour lane are one 2x2 block of the crop,
// since top, h0 and w0 are even.  Every lane of the wave calls this (lanes outside the frame or
// the crop with any rgb): the lane exchange comes first, the stores only for pixels of the crop.
// Two luma bytes per lane; of a block's pair the even lane writes U and the odd one V.
__device__ inline void final_store_yuv(const HeadH8Args& a, int img, int y, int x, const int (*rgb)[3]) {
  int sum[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    sum[ch] = rgb[0][ch] + rgb[1][ch];
    sum[ch] += __shfl_xor(sum[ch], 1);
  }
  const int yo = y - a.top;
  if (yo < 0 || yo >= a.h0 || x >= a.w0) return;
  const int64_t base = (int64_t)img * a.o_img;
  uint8_t* py = a.oy + base + (int64_t)yo * a.oy_pitch + x;
  py[0] = (uint8_t)rgb_to_luma(a.yc, rgb[0]);
  py[a.oy_pitch] = (uint8_t)rgb_to_luma(a.yc, rgb[1]);
  const int64_t c = base + (int64_t)(yo >> 1) * a.oc_pitch + (x >> 1) * a.oc_step;
  if (x & 1)
    a.ov[c] = (uint8_t)rgb_sum_to_chroma(a.yc.vr, a.yc.vg, a.yc.vb, sum);
  else
    a.ou[c] = (uint8_t)rgb_sum_to_chroma(a.yc.ur, a.yc.ug, a.yc.ub, sum);
}

// YUV (FINAL only): the 8-bit output as 4:2:0 planes (final_store_yuv) instead of interleaved RGB
template <int COUT, int MODE, int PLANES, bool YUV = false>
__global__ void __launch_bounds__(256) head_h8_kernel(HeadH8Args a) {
  // tile 16 rows x 32 cols; thread = 2 vertically adjacent pixels (packed fp32 FMA)
  constexpr int CIN = 32, HROWS = 18, HLC = 40;
  __shared__ __attribute__((aligned(16))) float s_in[8 * HROWS * HLC];
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tx = bid % a.tiles_x;
  bid /= a.tiles_x;
  const int ty = bid % a.tiles_y;
  const int img = bid / a.tiles_y;
  const int x0 = tx * 32, y0 = ty * 16;
  const int r2 = 2 * (tid >> 5), xl = tid & 31;

  // weights are wave-uniform: scalar loads, no LDS traffic
  float2v acc2[COUT];
#pragma unroll
  for (int co = 0; co < COUT; ++co) acc2[co] = float2v{a.bias[co], a.bias[co]};
  // records of rows y0-1..y0+16, cols x0-1..x0+32 of one channel group, fetched
  // one group ahead into registers, then converted to fp32 planar LDS
  constexpr int kRec = HROWS * H8_LC, kIt = (kRec + 255) / 256;
  uint4 pre[kIt][PLANES];
  auto fetch = [&](int g) {
#pragma unroll
    for (int it = 0; it < kIt; ++it) {
      const int idx = tid + 256 * it;
      if (idx < kRec) {
        const int rr = idx / H8_LC, col = idx - rr * H8_LC;
        const int64_t rec = img * a.src_img + (int64_t)g * a.src_gp + (int64_t)(y0 + rr) * a.src_wp + x0 +
                            (kH8PadLeft - 1) + col;
        pre[it][0] = a.src_hi[rec];
        if constexpr (PLANES == 2) pre[it][1] = a.src_lo[rec];
      }
    }
  };
  fetch(0);
  for (int g = 0; g < CIN / 8; ++g) {
#pragma unroll
    for (int it = 0; it < kIt; ++it) {
      const int idx = tid + 256 * it;
      if (idx < kRec) {
        const int rr = idx / H8_LC, col = idx - rr * H8_LC;
        const half8 vh = __builtin_bit_cast(half8, pre[it][0]);
        half8 vl = {};
        if constexpr (PLANES == 2) vl = __builtin_bit_cast(half8, pre[it][PLANES - 1]);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          s_in[(e * HROWS + rr) * HLC + col + 3] = PLANES == 2 ? join(vh[e], vl[e]) : (float)vh[e];
      }
    }
    __syncthreads();
    if (g + 1 < CIN / 8) fetch(g + 1);
#pragma unroll
    for (int ci = 0; ci < 8; ++ci) {
      float rows[4][3];  // input rows r2-1 .. r2+2 (staged rows r2 .. r2+3), cols xl-1 .. xl+1
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) rows[k][kx] = s_in[(ci * HROWS + r2 + k) * HLC + xl + 3 + kx];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const float2v v = {rows[ky][kx], rows[ky + 1][kx]};
#pragma unroll
          for (int co = 0; co < COUT; ++co) {
            const float w = a.w[((co * CIN) + g * 8 + ci) * 9 + ky * 3 + kx];
            acc2[co] = __builtin_elementwise_fma(float2v{w, w}, v, acc2[co]);
          }
        }
    }
    __syncthreads();
  }

  int rgb[2][3] = {};  // YUV: the two pixels' RGB bytes
  for (int p = 0; p < 2; ++p) {
  float acc[COUT];
#pragma unroll
  for (int co = 0; co < COUT; ++co) acc[co] = acc2[co][p];
  const int y = y0 + r2 + p, x = x0 + xl;
  if (y >= a.h || x >= a.w_) continue;
  // Net buffer records of this pixel: group 0 = ch 0-7, group 1 = ch 8-15
  const int64_t rec0 = img * a.g_img + (int64_t)(y + 1) * a.g_wp + x + kH8PadLeft, rec1 = rec0 + a.g_gp;
  uint4* ghi = reinterpret_cast<uint4*>(a.g_hi);
  uint4* glo = reinterpret_cast<uint4*>(a.g_lo);
  auto load8 = [&](int64_t rec, float* v) {
    const half8 h = __builtin_bit_cast(half8, ghi[rec]);
    half8 l = {};
    if constexpr (PLANES == 2) l = __builtin_bit_cast(half8, glo[rec]);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = PLANES == 2 ? join(h[e], l[e]) : (float)h[e];
  };
  // n consecutive channels starting at half `e0` of record `rec` (one 2/4/8/16-B store per plane)
  auto store = [&](int64_t rec, int e0, const float* v, int n) {
    _Float16 hv[8], lv[8];
    for (int e = 0; e < n; ++e)
      if (a.status && !(fabsf(v[e]) <= kF16Max)) *a.status = 1;
    for (int e = 0; e < n; ++e) {
      hv[e] = (_Float16)v[e];
      lv[e] = lo_of(v[e], hv[e]);
    }
    _Float16* ph = reinterpret_cast<_Float16*>(ghi + rec) + e0;
    _Float16* pl = reinterpret_cast<_Float16*>(glo + rec) + e0;
    if (n == 8) {
      *reinterpret_cast<uint4*>(ph) = __builtin_bit_cast(uint4, hv);
      if constexpr (PLANES == 2) *reinterpret_cast<uint4*>(pl) = __builtin_bit_cast(uint4, lv);
    } else if (n == 2) {
      *reinterpret_cast<uint32_t*>(ph) = (uint32_t)__builtin_bit_cast(uint16_t, hv[0]) |
                                         ((uint32_t)__builtin_bit_cast(uint16_t, hv[1]) << 16);
      if constexpr (PLANES == 2)
        *reinterpret_cast<uint32_t*>(pl) = (uint32_t)__builtin_bit_cast(uint16_t, lv[0]) |
                                           ((uint32_t)__builtin_bit_cast(uint16_t, lv[1]) << 16);
    } else {
      for (int e = 0; e < n; ++e) {
        ph[e] = hv[e];
        if constexpr (PLANES == 2) pl[e] = lv[e];
      }
    }
  };
  const float* cf = a.coef + img * 8;
  if (a.raw)
#pragma unroll
    for (int co = 0; co < COUT; ++co) a.raw[(((int64_t)img * COUT + co) * a.h + y) * a.w_ + x] = acc[co];

  if constexpr (MODE == RRIN_HEAD_PLAIN) {
    for (int co = 0; co < COUT; ++co) {
      const int64_t k = h8_half_index(a.g_img, a.g_gp, a.g_wp, img, co, y, x);
      const _Float16 vh = (_Float16)acc[co];
      a.g_hi[k] = vh;
      if constexpr (PLANES == 2) a.g_lo[k] = lo_of(acc[co], vh);
    }
  } else if constexpr (MODE == RRIN_HEAD_FLOW) {
#pragma clang fp contract(off)
    // round the raw flow to its stored form first, so that a later t-blend of the
    // kept raw flow (skip_flow) reproduces these Ft bit for bit
    _Float16 rh[4], rl[4];
    for (int k = 0; k < 4; ++k)
      if (a.status && !(fabsf(acc[k]) <= kF16Max)) *a.status = 1;
    for (int k = 0; k < 4; ++k) {
      rh[k] = (_Float16)acc[k];
      rl[k] = lo_of(acc[k], rh[k]);
      acc[k] = PLANES == 2 ? join(rh[k], rl[k]) : (float)rh[k];
    }
    if (a.fr_hi) {
      const int64_t kk = h8_half_index(a.fr_img, a.fr_gp, a.fr_wp, img, 0, y, x);
      *reinterpret_cast<uint2*>(a.fr_hi + kk) = __builtin_bit_cast(uint2, rh);
      if constexpr (PLANES == 2) *reinterpret_cast<uint2*>(a.fr_lo + kk) = __builtin_bit_cast(uint2, rl);
    }
    float f0[2], f1[2];
    flow_blend(cf, acc, f0, f1);
    store(rec0, 6, f0, 2);
    store(rec1, 0, f1, 2);
  } else if constexpr (MODE == RRIN_HEAD_REFINE) {
#pragma clang fp contract(off)
    float g0[8], g1[8];
    load8(rec0, g0);
    load8(rec1, g1);
    const float f0[2] = {g0[6] + acc[0], g0[7] + acc[1]};
    float o1[8];
    o1[0] = g1[0] + acc[2];
    o1[1] = g1[1] + acc[3];
    const WarpTaps t0 = warp_taps(x, y, f0[0], f0[1], a.h, a.w_);
    const WarpTaps t1 = warp_taps(x, y, o1[0], o1[1], a.h, a.w_);
    // backwarp x0 (ch 0-2) with Ft0 and x1 (ch 3-5) with Ft1: one record load per tap and plane
    auto tap8 = [&](int ty, int tx, float* v) {
      load8(img * a.g_img + (int64_t)(ty + 1) * a.g_wp + tx + kH8PadLeft, v);
    };
    warp3(t0, 0, tap8, o1 + 2);
    warp3(t1, 3, tap8, o1 + 5);
    store(rec0, 6, f0, 2);
    store(rec1, 0, o1, 8);
  } else if constexpr (MODE == RRIN_HEAD_MASK) {
#pragma clang fp contract(off)
    float g1[8];
    load8(rec1, g1);
    float o[3];
    mask_blend(cf, acc[0], acc[1], g1 + 2, g1 + 5, o);
    store(rec0, 6, o, 2);
    store(rec1, 0, o + 2, 1);
  } else {  // FINAL
#pragma clang fp contract(off)
    float g0[8], g1[8];
    load8(rec0, g0);
    load8(rec1, g1);
    const float base[3] = {g0[6], g0[7], g1[0]};
    const bool poison = a.status && *a.status != 0;  // an fp16 overflow upstream (range guard)
    float q[3];
    final_clamp(acc, base, q);
    if (a.out) {
      float* o = a.out + ((int64_t)img * 3) * a.h * a.w_ + (int64_t)y * a.w_ + x;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) o[(int64_t)ch * a.h * a.w_] = poison ? __builtin_nanf("") : q[ch];
    }
    if constexpr (YUV) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) rgb[p][ch] = final_byte(q[ch], poison);
    } else if (a.out8) {
      final_store_u8(a, img, y, x, q, poison);
    }
  }
  }
  if constexpr (YUV) final_store_yuv(a, img, y0 + r2, x0 + xl, rgb);
}

template <int PLANES>
__global__ void flow_tblend_h8_kernel(const _Float16* __restrict__ fhi, const _Float16* __restrict__ flo,
                                      int64_t f_img, int64_t f_gp, int f_wp, _Float16* ghi, _Float16* glo,
                                      int64_t g_img, int64_t g_gp, int g_wp, const float* coef, int h, int w,
                                      int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w);
  const int64_t t = i / w;
  const int y = (int)(t % h);
  const int img = (int)(t / h);
  const float* cf = coef + img * 8;
  float f[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t kk = h8_half_index(f_img, f_gp, f_wp, img, k, y, x);
    f[k] = PLANES == 2 ? join(fhi[kk], flo[kk]) : (float)fhi[kk];
  }
  float o[4];
  flow_blend(cf, f, o, o + 2);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t kk = h8_half_index(g_img, g_gp, g_wp, img, 6 + k, y, x);
    const _Float16 vh = (_Float16)o[k];
    ghi[kk] = vh;
    if constexpr (PLANES == 2) glo[kk] = lo_of(o[k], vh);
  }
}

// ---- F32R (exact fp32, 4 channels per record) layout / glue kernels -----------------
__global__ void nchw_to_r32_kernel(const float* __restrict__ src, float* dst, int64_t img_stride, int64_t gp, int wp,
                                   int ch_off, int c, int h, int w, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w);
  int64_t t = i / w;
  const int y = (int)(t % h);
  t /= h;
  const int ch = (int)(t % c);
  const int n = (int)(t / c);
  dst[r32_elem_index(img_stride, gp, wp, n, ch_off + ch, y, x)] = src[i];
}

__global__ void r32_to_nchw_kernel(const float* __restrict__ src, int64_t img_stride, int64_t gp, int wp, int ch_off,
                                   float* dst, int c, int h, int w, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w);
  int64_t t = i / w;
  const int y = (int)(t % h);
  t /= h;
  const int ch = (int)(t % c);
  const int n = (int)(t / c);
  dst[i] = src[r32_elem_index(img_stride, gp, wp, n, ch_off + ch, y, x)];
}

// x = cat(x0, x1) (model.py:33) into g16: record 0 = x0 0-2, x1 0; record 1 =
// x1 1-2, 0, 0; records 2-3 zero (whole-record stores).
__global__ void pack_g16_r32_kernel(const float* __restrict__ i0, const float* __restrict__ i1, uint4* g,
                                    int64_t img_stride, int64_t gp, int wp, int h, int w, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w);
  const int64_t t = i / w;
  const int y = (int)(t % h);
  const int img = (int)(t / h);
  const int64_t hw = (int64_t)h * w;
  const int64_t px = (int64_t)img * 3 * hw + (int64_t)y * w + x;
  const float a0 = i0[px], a1 = i0[px + hw], a2 = i0[px + 2 * hw];
  const float b0 = i1[px], b1 = i1[px + hw], b2 = i1[px + 2 * hw];
  const int64_t rec = (int64_t)img * img_stride + (int64_t)(y + 1) * wp + x + kH8PadLeft;
  g[rec] = f4rec(a0, a1, a2, b0);
  g[rec + gp] = f4rec(b1, b2, 0.f, 0.f);
  g[rec + 2 * gp] = make_uint4(0u, 0u, 0u, 0u);
  g[rec + 3 * gp] = make_uint4(0u, 0u, 0u, 0u);
}

// ---- 8-bit frames straight into g16 (rrin_pack_g16_u8_h8) --------------------------
__constant__ const U8ScaleTab kU8Scale{};

// x = cat(x0, x1) from two uint8 [n][h0][w0][3] frame stacks, edge-replicated on top (`top` rows)
// and on the right to the h x w of g16: padded pixel (y, x) reads source pixel
// (max(y - top, 0), min(x, w0 - 1)).  One workgroup per row and run of 256 pixels: the run's
// 768 source bytes of each frame are loaded one byte per lane (a wave's load is 64 consecutive
// bytes, whatever the alignment of the row) into LDS, then every lane converts its pixel through
// the LDS copy of the scale table and writes the whole records pack_g16_h8_kernel /
// pack_g16_r32_kernel write.  MODE 0: fp32 records, 1: fp16, 2: split16 (hi and lo planes).
template <int MODE>
__global__ void __launch_bounds__(256) pack_g16_u8_kernel(const uint8_t* __restrict__ f0,
                                                          const uint8_t* __restrict__ f1, int64_t f_img, int w0,
                                                          int top, uint4* ghi, uint4* glo, int64_t img_stride,
                                                          int64_t gp, int wp, int w) {
  __shared__ float s_tab[256];
  __shared__ uint8_t s_px[2][768];
  const int tid = threadIdx.x;
  const int xs = blockIdx.x * 256, y = blockIdx.y, img = blockIdx.z;
  s_tab[tid] = kU8Scale.v[tid];
  const int sy = y > top ? y - top : 0;
  const int64_t row = (int64_t)img * f_img + ((int64_t)sy * w0 + xs) * 3;
  const int nb = min(256, w0 - xs) * 3;  // xs < w0: the right pad is < 16 columns, xs a multiple of 256
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int b = tid + 256 * k;
    if (b < nb) {
      s_px[0][b] = f0[row + b];
      s_px[1][b] = f1[row + b];
    }
  }
  __syncthreads();
  const int x = xs + tid;
  if (x >= w) return;
  const int c = (min(x, w0 - 1) - xs) * 3;
  float a[3], b[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a[k] = s_tab[s_px[0][c + k]];
    b[k] = s_tab[s_px[1][c + k]];
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
    for (int k = 0; k < 3; ++k) {
      hi[k] = (_Float16)a[k];
      hi[3 + k] = (_Float16)b[k];
      lo[k] = lo_of(a[k], hi[k]);
      lo[3 + k] = lo_of(b[k], hi[3 + k]);
    }
    ghi[rec] = __builtin_bit_cast(uint4, hi);
    ghi[rec + gp] = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (MODE == 2) {
      glo[rec] = __builtin_bit_cast(uint4, lo);
      glo[rec + gp] = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

// Ft0 / Ft1 (model.py:38-39) from a kept raw Flow record -> g16 channels 6-9
__global__ void flow_tblend_r32_kernel(const uint4* __restrict__ fr, int64_t f_img, int f_wp, uint4* g, int64_t g_img,
                                       int64_t g_gp, int g_wp, const float* coef, int h, int w, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w);
  const int64_t t = i / w;
  const int y = (int)(t % h);
  const int img = (int)(t / h);
  const float* cf = coef + img * 8;
  const floatx4 f = __builtin_bit_cast(floatx4, fr[(int64_t)img * f_img + (int64_t)(y + 1) * f_wp + x + kH8PadLeft]);
  const float raw[4] = {f[0], f[1], f[2], f[3]};
  float o[4];
  flow_blend(cf, raw, o, o + 2);
  const int64_t rec = (int64_t)img * g_img + (int64_t)(y + 1) * g_wp + x + kH8PadLeft;
  const floatx4 r1 = __builtin_bit_cast(floatx4, g[rec + g_gp]);
  const floatx4 r2 = __builtin_bit_cast(floatx4, g[rec + 2 * g_gp]);
  g[rec + g_gp] = f4rec(r1[0], r1[1], o[0], o[1]);
  g[rec + 2 * g_gp] = f4rec(o[2], o[3], r2[2], r2[3]);
}

// bilinear x2 (unet.py:77, align_corners=False, edge clamp) of fp32 records
__global__ void up2x_r32_kernel(const uint4* __restrict__ s, int64_t s_img, int64_t s_gp, int s_wp, int sh, int sw,
                                uint4* d, int64_t d_img, int64_t d_gp, int d_wp, int groups, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int w = 2 * sw, h = 2 * sh;
  const int x = (int)(i % w);
  int64_t t = i / w;
  const int y = (int)(t % h);
  t /= h;
  const int g = (int)(t % groups);
  const int img = (int)(t / groups);
  int ra, rb, ca, cb;
  float wa, wc;
  if (y & 1) { ra = y >> 1; rb = min(ra + 1, sh - 1); wa = 0.75f; }
  else { rb = y >> 1; ra = max(rb - 1, 0); wa = 0.25f; }
  if (x & 1) { ca = x >> 1; cb = min(ca + 1, sw - 1); wc = 0.75f; }
  else { cb = x >> 1; ca = max(cb - 1, 0); wc = 0.25f; }
  const float wb = 1.0f - wa, wd = 1.0f - wc;
  const int64_t base = img * s_img + g * s_gp + kH8PadLeft;
  const floatx4 q0 = __builtin_bit_cast(floatx4, s[base + (int64_t)(ra + 1) * s_wp + ca]);
  const floatx4 q1 = __builtin_bit_cast(floatx4, s[base + (int64_t)(ra + 1) * s_wp + cb]);
  const floatx4 q2 = __builtin_bit_cast(floatx4, s[base + (int64_t)(rb + 1) * s_wp + ca]);
  const floatx4 q3 = __builtin_bit_cast(floatx4, s[base + (int64_t)(rb + 1) * s_wp + cb]);
  float o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float top = wc * q0[e] + wd * q1[e];  // horizontal first (upsample_bilinear2d order)
    const float bot = wc * q2[e] + wd * q3[e];
    o[e] = wa * top + wb * bot;
  }
  d[img * d_img + g * d_gp + (int64_t)(y + 1) * d_wp + x + kH8PadLeft] = f4rec(o[0], o[1], o[2], o[3]);
}

// Head conv (Cout <= 4) + Net glue on fp32 records: as head_h8_kernel, with the
// 32-channel input as 8 records of 4 channels and g16 as 4 records; every g16
// update is a whole 16-B record (records the glue only partly changes are read
// first), no partial-record writes.
template <int COUT, int MODE, bool YUV = false>
__global__ void __launch_bounds__(256) head_r32_kernel(HeadH8Args a) {
  constexpr int CIN = 32, HROWS = 18, HLC = 40;
  __shared__ __attribute__((aligned(16))) float s_in[8 * HROWS * HLC];
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int tx = bid % a.tiles_x;
  bid /= a.tiles_x;
  const int ty = bid % a.tiles_y;
  const int img = bid / a.tiles_y;
  const int x0 = tx * 32, y0 = ty * 16;
  const int r2 = 2 * (tid >> 5), xl = tid & 31;

  float acc2[2][COUT];
#pragma unroll
  for (int co = 0; co < COUT; ++co) acc2[0][co] = acc2[1][co] = a.bias[co];
  // records of rows y0-1..y0+16, cols x0-1..x0+32 of 8 channels (2 record groups),
  // fetched one channel octet ahead into registers, then stored to planar LDS
  constexpr int kRec = HROWS * H8_LC, kIt = (kRec + 255) / 256;
  uint4 pre[kIt][2];
  auto fetch = [&](int g8) {
#pragma unroll
    for (int it = 0; it < kIt; ++it) {
      const int idx = tid + 256 * it;
      if (idx < kRec) {
        const int rr = idx / H8_LC, col = idx - rr * H8_LC;
        const int64_t rec = img * a.src_img + (int64_t)(2 * g8) * a.src_gp + (int64_t)(y0 + rr) * a.src_wp + x0 +
                            (kH8PadLeft - 1) + col;
        pre[it][0] = a.src_hi[rec];
        pre[it][1] = a.src_hi[rec + a.src_gp];
      }
    }
  };
  fetch(0);
  for (int g8 = 0; g8 < CIN / 8; ++g8) {
#pragma unroll
    for (int it = 0; it < kIt; ++it) {
      const int idx = tid + 256 * it;
      if (idx < kRec) {
        const int rr = idx / H8_LC, col = idx - rr * H8_LC;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          s_in[(e * HROWS + rr) * HLC + col + 3] = __builtin_bit_cast(floatx4, pre[it][e >> 2])[e & 3];
      }
    }
    __syncthreads();
    if (g8 + 1 < CIN / 8) fetch(g8 + 1);
#pragma unroll
    for (int ci = 0; ci < 8; ++ci) {
      float rows[4][3];
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) rows[k][kx] = s_in[(ci * HROWS + r2 + k) * HLC + xl + 3 + kx];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int co = 0; co < COUT; ++co) {
            const float w = a.w[((co * CIN) + g8 * 8 + ci) * 9 + ky * 3 + kx];
            acc2[0][co] = fmaf(w, rows[ky][kx], acc2[0][co]);
            acc2[1][co] = fmaf(w, rows[ky + 1][kx], acc2[1][co]);
          }
    }
    __syncthreads();
  }

  int rgb[2][3] = {};  // YUV: the two pixels' RGB bytes
  for (int p = 0; p < 2; ++p) {
    float acc[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) acc[co] = acc2[p][co];
    const int y = y0 + r2 + p, x = x0 + xl;
    if (y >= a.h || x >= a.w_) continue;
    const int64_t rec0 = img * a.g_img + (int64_t)(y + 1) * a.g_wp + x + kH8PadLeft;
    auto ld = [&](int k) { return __builtin_bit_cast(floatx4, a.g32[rec0 + k * a.g_gp]); };
    auto st = [&](int k, float v0, float v1, float v2, float v3) { a.g32[rec0 + k * a.g_gp] = f4rec(v0, v1, v2, v3); };
    const float* cf = a.coef + img * 8;
    if (a.raw)
#pragma unroll
      for (int co = 0; co < COUT; ++co) a.raw[(((int64_t)img * COUT + co) * a.h + y) * a.w_ + x] = acc[co];
    if constexpr (MODE == RRIN_HEAD_PLAIN) {
      float* gf = reinterpret_cast<float*>(a.g32);
      for (int co = 0; co < COUT; ++co) gf[r32_elem_index(a.g_img, a.g_gp, a.g_wp, img, co, y, x)] = acc[co];
    } else if constexpr (MODE == RRIN_HEAD_FLOW) {
#pragma clang fp contract(off)
      if (a.fr32) a.fr32[img * a.fr_img + (int64_t)(y + 1) * a.fr_wp + x + kH8PadLeft] = f4rec(acc[0], acc[1], acc[2], acc[3]);
      float f0[2], f1[2];
      flow_blend(cf, acc, f0, f1);
      const floatx4 r1 = ld(1), r2v = ld(2);
      st(1, r1[0], r1[1], f0[0], f0[1]);
      st(2, f1[0], f1[1], r2v[2], r2v[3]);
    } else if constexpr (MODE == RRIN_HEAD_REFINE) {
#pragma clang fp contract(off)
      const floatx4 q1 = ld(1), q2 = ld(2);
      const float f0[2] = {q1[2] + acc[0], q1[3] + acc[1]};
      float o1[8];
      o1[0] = q2[0] + acc[2];
      o1[1] = q2[1] + acc[3];
      const WarpTaps t0 = warp_taps(x, y, f0[0], f0[1], a.h, a.w_);
      const WarpTaps t1 = warp_taps(x, y, o1[0], o1[1], a.h, a.w_);
      // backwarp x0 (ch 0-2) with Ft0 and x1 (ch 3-5) with Ft1: records 0-1 per tap
      auto tap8 = [&](int ty, int tx, float* v) {
        const int64_t r = img * a.g_img + (int64_t)(ty + 1) * a.g_wp + tx + kH8PadLeft;
        const floatx4 lo = __builtin_bit_cast(floatx4, a.g32[r]);
        const floatx4 hi = __builtin_bit_cast(floatx4, a.g32[r + a.g_gp]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = lo[e];
          v[4 + e] = hi[e];
        }
      };
      warp3(t0, 0, tap8, o1 + 2);
      warp3(t1, 3, tap8, o1 + 5);
      st(1, q1[0], q1[1], f0[0], f0[1]);
      st(2, o1[0], o1[1], o1[2], o1[3]);
      st(3, o1[4], o1[5], o1[6], o1[7]);
    } else if constexpr (MODE == RRIN_HEAD_MASK) {
#pragma clang fp contract(off)
      const floatx4 r1 = ld(1), r2v = ld(2), r3 = ld(3);
      const float g1[8] = {r2v[0], r2v[1], r2v[2], r2v[3], r3[0], r3[1], r3[2], r3[3]};  // ch 8-15
      float o[3];
      mask_blend(cf, acc[0], acc[1], g1 + 2, g1 + 5, o);
      st(1, r1[0], r1[1], o[0], o[1]);
      st(2, o[2], r2v[1], r2v[2], r2v[3]);
    } else {  // FINAL
#pragma clang fp contract(off)
      const floatx4 r1 = ld(1), r2v = ld(2);
      const float base[3] = {r1[2], r1[3], r2v[0]};
      float q[3];
      final_clamp(acc, base, q);
      if (a.out) {
        float* o = a.out + ((int64_t)img * 3) * a.h * a.w_ + (int64_t)y * a.w_ + x;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[(int64_t)ch * a.h * a.w_] = q[ch];
      }
      if constexpr (YUV) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) rgb[p][ch] = final_byte(q[ch], false);
      } else if (a.out8) {
        final_store_u8(a, img, y, x, q, false);
      }
    }
  }
  if constexpr (YUV) final_store_yuv(a, img, y0 + r2, x0 + xl, rgb);
}

// zero channels [c0, c1) of every interior pixel of a record-layout view (H8 hi
// and lo planes, or R32); rrin_unet_fwd clears the channels its PLAIN head
// writes past in_ch so that the next call's first conv never stages them
__global__ void clear_channels_kernel(_Float16* hi, _Float16* lo, float* r32, int64_t img_stride, int64_t gp, int wp,
                                      int c0, int c, int h, int w, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w);
  int64_t t = i / w;
  const int y = (int)(t % h);
  t /= h;
  const int ch = c0 + (int)(t % c);
  const int n = (int)(t / c);
  if (r32) {
    r32[r32_elem_index(img_stride, gp, wp, n, ch, y, x)] = 0.f;
    return;
  }
  const int64_t k = h8_half_index(img_stride, gp, wp, n, ch, y, x);
  hi[k] = (_Float16)0.f;
  if (lo) lo[k] = (_Float16)0.f;
}

int clear_channels_h8(const rrin_h8* v, int32_t n, int32_t c0, int32_t c1, int32_t prec, hipStream_t st) {
  if (!v || n < 1 || c0 < 0 || c1 <= c0 || !rec_prec(prec) || c1 > chans_per_rec(prec) * v->groups) return RRIN_E_ARG;
  const int64_t total = (int64_t)n * (c1 - c0) * v->g.h * v->g.w;
  const int grid = (int)((total + 255) / 256);
  if (prec == RRIN_PREC_F32R) {
    hipLaunchKernelGGL(clear_channels_kernel, dim3(grid), dim3(256), 0, st, (_Float16*)nullptr, (_Float16*)nullptr,
                       static_cast<float*>(v->hi) + (int64_t)v->g_off * v->g.plane * 4, v->img_stride, v->g.plane,
                       v->g.wp, c0, c1 - c0, v->g.h, v->g.w, total);
  } else {
    const int64_t go = (int64_t)v->g_off * v->g.plane * 8;
    hipLaunchKernelGGL(clear_channels_kernel, dim3(grid), dim3(256), 0, st, static_cast<_Float16*>(v->hi) + go,
                       planes_of(prec) == 2 ? static_cast<_Float16*>(v->lo) + go : (_Float16*)nullptr,
                       (float*)nullptr, v->img_stride, v->g.plane, v->g.wp, c0, c1 - c0, v->g.h, v->g.w, total);
  }
  return hip_code(hipGetLastError());
}
}  // namespace rrin

using namespace rrin;

extern "C" int rrin_make_geom_h8(int32_t h, int32_t w, rrin_geom* g) {
  if (!g || h < 1 || w < 1) return RRIN_E_ARG;
  *g = make_geom_h8(h, w);
  return 0;
}

extern "C" int rrin_upsample2x_h8(const rrin_h8* src, const rrin_h8* dst, int32_t n, int32_t prec, void* stream) {
  if (!src || !dst || n < 1 || !rec_prec(prec)) return RRIN_E_ARG;
  if (!h8_ok(*src, prec) || !h8_ok(*dst, prec)) return RRIN_E_SHAPE;
  if (dst->g.h != 2 * src->g.h || dst->g.w != 2 * src->g.w || dst->groups < src->groups) return RRIN_E_SHAPE;
  const int64_t total = (int64_t)n * src->groups * dst->g.h * dst->g.w;
  const int grid = (int)((total + 255) / 256);
  const int64_t so = (int64_t)src->g_off * src->g.plane, dof = (int64_t)dst->g_off * dst->g.plane;
  const uint4* shi = static_cast<const uint4*>(src->hi) + so;
  uint4* dhi = static_cast<uint4*>(dst->hi) + dof;
  hipStream_t st = (hipStream_t)stream;
  if (prec == RRIN_PREC_F32R) {
    hipLaunchKernelGGL(up2x_r32_kernel, dim3(grid), dim3(256), 0, st, shi, src->img_stride, src->g.plane, src->g.wp,
                       src->g.h, src->g.w, dhi, dst->img_stride, dst->g.plane, dst->g.wp, src->groups, total);
  } else if (planes_of(prec) == 2) {
    hipLaunchKernelGGL(up2x_h8_kernel<2>, dim3(grid), dim3(256), 0, st, shi,
                       static_cast<const uint4*>(src->lo) + so, src->img_stride, src->g.plane, src->g.wp, src->g.h,
                       src->g.w, dhi, static_cast<uint4*>(dst->lo) + dof, dst->img_stride, dst->g.plane, dst->g.wp,
                       src->groups, total);
  } else {
    hipLaunchKernelGGL(up2x_h8_kernel<1>, dim3(grid), dim3(256), 0, st, shi, (const uint4*)nullptr,
                       src->img_stride, src->g.plane, src->g.wp, src->g.h, src->g.w, dhi, (uint4*)nullptr,
                       dst->img_stride, dst->g.plane, dst->g.wp, src->groups, total);
  }
  return hip_code(hipGetLastError());
}

extern "C" int rrin_nchw_to_h8(const float* src, int32_t n, int32_t c, int32_t ch_off, const rrin_h8* dst,
                               int32_t prec, void* stream) {
  if (!src || !dst || n < 1 || c < 1 || ch_off < 0 || !rec_prec(prec)) return RRIN_E_ARG;
  if (ch_off + c > chans_per_rec(prec) * dst->groups) return RRIN_E_ARG;
  if (!h8_ok(*dst, prec)) return RRIN_E_SHAPE;
  const int64_t total = (int64_t)n * c * dst->g.h * dst->g.w;
  const int grid = (int)((total + 255) / 256);
  if (prec == RRIN_PREC_F32R) {
    hipLaunchKernelGGL(nchw_to_r32_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, src,
                       static_cast<float*>(dst->hi) + (int64_t)dst->g_off * dst->g.plane * 4, dst->img_stride,
                       dst->g.plane, dst->g.wp, ch_off, c, dst->g.h, dst->g.w, total);
    return hip_code(hipGetLastError());
  }
  const int64_t go = (int64_t)dst->g_off * dst->g.plane * 8;
  hipLaunchKernelGGL(nchw_to_h8_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, src,
                     static_cast<_Float16*>(dst->hi) + go,
                     planes_of(prec) == 2 ? static_cast<_Float16*>(dst->lo) + go : (_Float16*)nullptr,
                     dst->img_stride, dst->g.plane, dst->g.wp, ch_off, c, dst->g.h, dst->g.w, total);
  return hip_code(hipGetLastError());
}

extern "C" int rrin_h8_to_nchw(const rrin_h8* src, int32_t n, int32_t c, int32_t ch_off, float* dst, int32_t prec,
                               void* stream) {
  if (!src || !dst || n < 1 || c < 1 || ch_off < 0 || !rec_prec(prec)) return RRIN_E_ARG;
  if (ch_off + c > chans_per_rec(prec) * src->groups) return RRIN_E_ARG;
  if (!h8_ok(*src, prec)) return RRIN_E_SHAPE;
  const int64_t total = (int64_t)n * c * src->g.h * src->g.w;
  const int grid = (int)((total + 255) / 256);
  if (prec == RRIN_PREC_F32R) {
    hipLaunchKernelGGL(r32_to_nchw_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const float*>(src->hi) + (int64_t)src->g_off * src->g.plane * 4, src->img_stride,
                       src->g.plane, src->g.wp, ch_off, dst, c, src->g.h, src->g.w, total);
    return hip_code(hipGetLastError());
  }
  const int64_t go = (int64_t)src->g_off * src->g.plane * 8;
  hipLaunchKernelGGL(h8_to_nchw_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                     static_cast<const _Float16*>(src->hi) + go,
                     planes_of(prec) == 2 ? static_cast<const _Float16*>(src->lo) + go : (const _Float16*)nullptr,
                     src->img_stride, src->g.plane, src->g.wp, ch_off, dst, c, src->g.h, src->g.w, total);
  return hip_code(hipGetLastError());
}

template <int COUT, int MODE, bool YUV = false>
static int head_h8_launch(const HeadH8Args& a, int planes, int grid, hipStream_t st) {
  if (planes == 0)  // F32R
    hipLaunchKernelGGL((head_r32_kernel<COUT, MODE, YUV>), dim3(grid), dim3(256), 0, st, a);
  else if (planes == 2)
    hipLaunchKernelGGL((head_h8_kernel<COUT, MODE, 2, YUV>), dim3(grid), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((head_h8_kernel<COUT, MODE, 1, YUV>), dim3(grid), dim3(256), 0, st, a);
  return hip_code(hipGetLastError());
}

// Validate a head descriptor and turn it into kernel arguments (grid: blocks).
static int head_prepare(const rrin_head_h8_desc* d, HeadH8Args& a, int& grid) {
  if (!d || !d->w || !d->bias || d->cin != 32 || d->n < 1) return RRIN_E_ARG;
  if (!rec_prec(d->prec)) return RRIN_E_ARG;
  if (!h8_ok(d->src, d->prec) || !h8_ok(d->g16, d->prec)) return RRIN_E_SHAPE;
  const int h = d->src.g.h, w = d->src.g.w;
  const int cpr = chans_per_rec(d->prec);
  if (d->g16.g.h != h || d->g16.g.w != w || d->src.groups * cpr < 32) return RRIN_E_SHAPE;
  if (d->mode != RRIN_HEAD_PLAIN) {
    if (d->g16.groups * cpr < 16 || d->g16.g_off != 0 || !d->coef) return RRIN_E_ARG;
  } else if (cpr * d->g16.groups < d->cout) {
    return RRIN_E_ARG;
  }
  const bool yuv = d->mode == RRIN_HEAD_FINAL && d->out_yuv.y;
  if (d->mode == RRIN_HEAD_FINAL && !d->out && !d->out_u8 && !yuv) return RRIN_E_ARG;
  if (yuv && d->out_u8) return RRIN_E_ARG;
  if (d->mode == RRIN_HEAD_FINAL && (d->out_u8 || yuv) &&
      (d->h0 < 1 || d->w0 < 1 || d->top < 0 || d->top + d->h0 > h || d->w0 > w))
    return RRIN_E_SHAPE;
  if (yuv) {
    if (int rc = yuv_coef_check(&d->yuv_coef)) return rc;
    if (int rc = yuv420_check(d->out_yuv, d->n, d->h0, d->w0)) return rc;
    if (d->top & 1) return RRIN_E_SHAPE;
  }
  const int planes = planes_of(d->prec);
  memset(&a, 0, sizeof(a));
  const int64_t sg = (int64_t)d->src.g_off * d->src.g.plane;
  a.src_hi = static_cast<const uint4*>(d->src.hi) + sg;
  a.src_lo = planes == 2 ? static_cast<const uint4*>(d->src.lo) + sg : nullptr;
  a.src_img = d->src.img_stride;
  a.src_gp = d->src.g.plane;
  a.src_wp = d->src.g.wp;
  const int64_t gg = (int64_t)d->g16.g_off * d->g16.g.plane * 8;
  if (d->prec == RRIN_PREC_F32R) {
    a.g32 = static_cast<uint4*>(d->g16.hi) + (int64_t)d->g16.g_off * d->g16.g.plane;
  } else {
    a.g_hi = static_cast<_Float16*>(d->g16.hi) + gg;
    a.g_lo = planes == 2 ? static_cast<_Float16*>(d->g16.lo) + gg : nullptr;
  }
  a.g_img = d->g16.img_stride;
  a.g_gp = d->g16.g.plane;
  a.g_wp = d->g16.g.wp;
  a.w = d->w;
  a.bias = d->bias;
  a.coef = d->coef;
  a.out = d->out;
  a.raw = d->raw_out;
  a.status = d->status;
  if (d->mode == RRIN_HEAD_FINAL && d->out_u8) {
    a.out8 = d->out_u8;
    a.h0 = d->h0;
    a.w0 = d->w0;
    a.top = d->top;
  }
  if (yuv) {
    a.oy = const_cast<uint8_t*>(d->out_yuv.y);
    a.ou = const_cast<uint8_t*>(d->out_yuv.u);
    a.ov = const_cast<uint8_t*>(d->out_yuv.v);
    a.o_img = d->out_yuv.img_stride;
    a.oy_pitch = d->out_yuv.y_pitch;
    a.oc_pitch = d->out_yuv.c_pitch;
    a.oc_step = d->out_yuv.c_step;
    a.yc = d->yuv_coef;
    a.h0 = d->h0;
    a.w0 = d->w0;
    a.top = d->top;
  }
  if (d->mode == RRIN_HEAD_FLOW && d->flow_raw.hi) {
    if (!h8_ok(d->flow_raw, d->prec) || d->flow_raw.g.h != h || d->flow_raw.g.w != w) return RRIN_E_SHAPE;
    const int64_t fo = (int64_t)d->flow_raw.g_off * d->flow_raw.g.plane * 8;
    if (d->prec == RRIN_PREC_F32R) {
      a.fr32 = static_cast<uint4*>(d->flow_raw.hi) + (int64_t)d->flow_raw.g_off * d->flow_raw.g.plane;
    } else {
      a.fr_hi = static_cast<_Float16*>(d->flow_raw.hi) + fo;
      a.fr_lo = planes == 2 ? static_cast<_Float16*>(d->flow_raw.lo) + fo : nullptr;
    }
    a.fr_img = d->flow_raw.img_stride;
    a.fr_gp = d->flow_raw.g.plane;
    a.fr_wp = d->flow_raw.g.wp;
  }
  a.h = h;
  a.w_ = w;
  a.tiles_x = (w + 31) / 32;
  a.tiles_y = (h + 15) / 16;
  grid = a.tiles_x * a.tiles_y * d->n;
  return 0;
}

extern "C" int rrin_head_h8_fwd(const rrin_head_h8_desc* d, void* stream) {
  HeadH8Args a;
  int grid = 0;
  const int rc = head_prepare(d, a, grid);
  if (rc) return rc;
  const int planes = d->prec == RRIN_PREC_F32R ? 0 : planes_of(d->prec);
  hipStream_t st = (hipStream_t)stream;
  switch (d->mode) {
    case RRIN_HEAD_PLAIN:
      if (d->cout == 2) return head_h8_launch<2, RRIN_HEAD_PLAIN>(a, planes, grid, st);
      if (d->cout == 3) return head_h8_launch<3, RRIN_HEAD_PLAIN>(a, planes, grid, st);
      if (d->cout == 4) return head_h8_launch<4, RRIN_HEAD_PLAIN>(a, planes, grid, st);
      return RRIN_E_ARG;
    case RRIN_HEAD_FLOW:
      return d->cout == 4 ? head_h8_launch<4, RRIN_HEAD_FLOW>(a, planes, grid, st) : RRIN_E_ARG;
    case RRIN_HEAD_REFINE:
      return d->cout == 4 ? head_h8_launch<4, RRIN_HEAD_REFINE>(a, planes, grid, st) : RRIN_E_ARG;
    case RRIN_HEAD_MASK:
      return d->cout == 2 ? head_h8_launch<2, RRIN_HEAD_MASK>(a, planes, grid, st) : RRIN_E_ARG;
    case RRIN_HEAD_FINAL:
      if (d->cout != 3) return RRIN_E_ARG;
      return a.oy ? head_h8_launch<3, RRIN_HEAD_FINAL, true>(a, planes, grid, st)
                  : head_h8_launch<3, RRIN_HEAD_FINAL>(a, planes, grid, st);
  }
  return RRIN_E_ARG;
}

extern "C" int rrin_flow_tblend_h8(const rrin_h8* fr, const rrin_h8* g16, const float* coef, int32_t n, int32_t prec,
                                   void* stream) {
  if (!fr || !g16 || !coef || n < 1 || !rec_prec(prec)) return RRIN_E_ARG;
  if (!h8_ok(*fr, prec) || !h8_ok(*g16, prec) || g16->g_off != 0 || g16->groups * chans_per_rec(prec) < 16)
    return RRIN_E_SHAPE;
  if (fr->g.h != g16->g.h || fr->g.w != g16->g.w) return RRIN_E_SHAPE;
  const int h = g16->g.h, w = g16->g.w;
  const int64_t total = (int64_t)n * h * w;
  const int grid = (int)((total + 255) / 256);
  if (prec == RRIN_PREC_F32R) {
    hipLaunchKernelGGL(flow_tblend_r32_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const uint4*>(fr->hi) + (int64_t)fr->g_off * fr->g.plane, fr->img_stride,
                       fr->g.wp, static_cast<uint4*>(g16->hi), g16->img_stride, g16->g.plane, g16->g.wp, coef, h, w,
                       total);
    return hip_code(hipGetLastError());
  }
  const int64_t fo = (int64_t)fr->g_off * fr->g.plane * 8;
  const _Float16* fhi = static_cast<const _Float16*>(fr->hi) + fo;
  hipStream_t st = (hipStream_t)stream;
  if (planes_of(prec) == 2)
    hipLaunchKernelGGL(flow_tblend_h8_kernel<2>, dim3(grid), dim3(256), 0, st, fhi,
                       static_cast<const _Float16*>(fr->lo) + fo, fr->img_stride, fr->g.plane, fr->g.wp,
                       static_cast<_Float16*>(g16->hi), static_cast<_Float16*>(g16->lo), g16->img_stride,
                       g16->g.plane, g16->g.wp, coef, h, w, total);
  else
    hipLaunchKernelGGL(flow_tblend_h8_kernel<1>, dim3(grid), dim3(256), 0, st, fhi, (const _Float16*)nullptr,
                       fr->img_stride, fr->g.plane, fr->g.wp, static_cast<_Float16*>(g16->hi), (_Float16*)nullptr,
                       g16->img_stride, g16->g.plane, g16->g.wp, coef, h, w, total);
  return hip_code(hipGetLastError());
}

extern "C" int rrin_pack_g16_h8(const float* i0, const float* i1, int32_t n, const rrin_h8* g16, int32_t prec,
                                void* stream) {
  if (!i0 || !i1 || !g16 || n < 1 || !rec_prec(prec)) return RRIN_E_ARG;
  if (!h8_ok(*g16, prec) || g16->g_off != 0 || g16->groups * chans_per_rec(prec) < 16) return RRIN_E_SHAPE;
  const int64_t total = (int64_t)n * g16->g.h * g16->g.w;
  const int grid = (int)((total + 255) / 256);
  hipStream_t st = (hipStream_t)stream;
  if (prec == RRIN_PREC_F32R)
    hipLaunchKernelGGL(pack_g16_r32_kernel, dim3(grid), dim3(256), 0, st, i0, i1, static_cast<uint4*>(g16->hi),
                       g16->img_stride, g16->g.plane, g16->g.wp, g16->g.h, g16->g.w, total);
  else if (planes_of(prec) == 2)
    hipLaunchKernelGGL(pack_g16_h8_kernel<2>, dim3(grid), dim3(256), 0, st, i0, i1, static_cast<uint4*>(g16->hi),
                       static_cast<uint4*>(g16->lo), g16->img_stride, g16->g.plane, g16->g.wp, g16->g.h, g16->g.w,
                       total);
  else
    hipLaunchKernelGGL(pack_g16_h8_kernel<1>, dim3(grid), dim3(256), 0, st, i0, i1, static_cast<uint4*>(g16->hi),
                       (uint4*)nullptr, g16->img_stride, g16->g.plane, g16->g.wp, g16->g.h, g16->g.w, total);
  return hip_code(hipGetLastError());
}

extern "C" int rrin_pack_g16_u8_h8(const uint8_t* f0, const uint8_t* f1, int64_t img_stride, int32_t n, int32_t h0,
                                   int32_t w0, const rrin_h8* g16, int32_t prec, void* stream) {
  if (!f0 || !f1 || !g16 || n < 1 || !rec_prec(prec)) return RRIN_E_ARG;
  if (!h8_ok(*g16, prec) || g16->g_off != 0 || g16->groups * chans_per_rec(prec) < 16) return RRIN_E_SHAPE;
  const int h = g16->g.h, w = g16->g.w;
  if (h0 < 1 || w0 < 1 || h != (h0 + 15) / 16 * 16 || w != (w0 + 15) / 16 * 16) return RRIN_E_SHAPE;
  if (img_stride < (int64_t)h0 * w0 * 3 && n > 1) return RRIN_E_ARG;
  if (n > 65535 || h > 65535) return RRIN_E_SHAPE;  // grid y / z
  const dim3 grid((w + 255) / 256, h, n);
  const int top = h - h0;
  hipStream_t st = (hipStream_t)stream;
  if (prec == RRIN_PREC_F32R)
    hipLaunchKernelGGL(pack_g16_u8_kernel<0>, grid, dim3(256), 0, st, f0, f1, img_stride, w0, top,
                       static_cast<uint4*>(g16->hi), (uint4*)nullptr, g16->img_stride, g16->g.plane, g16->g.wp, w);
  else if (planes_of(prec) == 2)
    hipLaunchKernelGGL(pack_g16_u8_kernel<2>, grid, dim3(256), 0, st, f0, f1, img_stride, w0, top,
                       static_cast<uint4*>(g16->hi), static_cast<uint4*>(g16->lo), g16->img_stride, g16->g.plane,
                       g16->g.wp, w);
  else
    hipLaunchKernelGGL(pack_g16_u8_kernel<1>, grid, dim3(256), 0, st, f0, f1, img_stride, w0, top,
                       static_cast<uint4*>(g16->hi), (uint4*)nullptr, g16->img_stride, g16->g.plane, g16->g.wp, w);
  return hip_code(hipGetLastError());
}
