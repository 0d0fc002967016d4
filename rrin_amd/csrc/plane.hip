// An extra single-channel plane (alpha, depth, ID) carried through a byte-frame forward by the
// picture's own motion (rrin_amd/plane.py is the definition; include/rrin_hip.h the contract):
//   rrin_plane_warp_h8   behind the REFINE head: at0 = warp(A0, Flow_t_0), at1 = warp(A1, Flow_t_1)
//                        from the refined flows in g16 channels 6-9 and the caller's byte / word
//                        planes, as fp32 into the scratch
//   rrin_plane_blend_h8  behind the MASK head: (w1 at0 + w2 at1) / (w1 + w2 + 1e-8) with the two mask
//                        logits the head left in the scratch (its raw_out), clamped, quantised,
//                        stored into the crop
// Two launches because the MASK head overwrites g16 channels 6-8 with its blend: the refined flows
// no longer exist when the mask is known, and the mask weights are never stored.
// Both are memory-bound, one padded (blend: cropped) pixel per lane with x fastest: a wave reads
// runs of consecutive 16-B records and reads / writes runs of consecutive floats and samples.  The
// warp is written once over a record format F (rec_fmt.hpp) and an element type; no LDS.
#include <type_traits>

#include "net_glue.hpp"
#include "rec_fmt.hpp"
#include "yuv.hpp"

namespace rrin {

struct PlaneIn {
  const void* a0;
  const void* a1;
  int64_t stride;  // elements between frames
  int pitch;       // elements between rows
  int h0, w0, top;
  int maxval, shift;
};

// sample (sy, sx) of a frame's plane: min(word >> shift, maxval) / maxval, the IEEE division of the
// frame packs (sample_to_float)
template <class E>
__device__ inline float plane_sample(const E* f, const PlaneIn& p, int sy, int sx) {
  const int v = (int)f[(int64_t)sy * p.pitch + sx];
  return sample_to_float(min(v >> p.shift, p.maxval), (float)p.maxval);
}

// backwarp of one plane with the taps t of the padded frame: padded pixel (ty, tx) is sample
// (max(ty - top, 0), min(tx, w0 - 1)); taps outside the padded frame read 0 (warp3's sum order)
template <class E>
__device__ inline float warp1(const WarpTaps& t, const E* f, const PlaneIn& p) {
#pragma clang fp contract(off)
  float q[4];
  const bool ok[4] = {t.vy0 && t.vx0, t.vy0 && t.vx1, t.vy1 && t.vx0, t.vy1 && t.vx1};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ty = t.y0 + (k >> 1), tx = t.x0 + (k & 1);
    q[k] = ok[k] ? plane_sample(f, p, max(ty - p.top, 0), min(tx, p.w0 - 1)) : 0.0f;
  }
  return q[0] * t.nw + q[1] * t.ne + q[2] * t.sw + q[3] * t.se;
}

// One lane per padded pixel (y, x) of image img.  at: fp32 [n][2][h][w].
template <class F, class E, bool ITEMS>
__global__ void __launch_bounds__(256) plane_warp_kernel(RecView g, PlaneIn p, float* __restrict__ at, int h, int w,
                                                         int64_t total, const int32_t* __restrict__ map, int n_pairs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w);
  const int64_t r = i / w;
  const int y = (int)(r % h);
  const int img = (int)(r / h);
  typename F::Px px{g, g.rec(img, 0, y, x), nullptr};
  px.template fetch<6, 10, 0, 0>();
  const WarpTaps t0 = warp_taps(x, y, px.c[6], px.c[7], h, w);
  const WarpTaps t1 = warp_taps(x, y, px.c[8], px.c[9], h, w);
  const int src = ITEMS ? pair_of(map, img, n_pairs) : img;
  const E* f0 = static_cast<const E*>(p.a0) + (int64_t)src * p.stride;
  const E* f1 = static_cast<const E*>(p.a1) + (int64_t)src * p.stride;
  const int64_t hw = (int64_t)h * w;
  float* o = at + (int64_t)img * 2 * hw + (int64_t)y * w + x;
  o[0] = warp1(t0, f0, p);
  o[hw] = warp1(t1, f1, p);
}

struct PlaneOut {
  void* out;
  int64_t stride;
  int pitch;
  int h0, w0, top;
  int maxval, shift;
};

// One lane per pixel (yo, x) of the crop of image img: padded pixel (top + yo, x).  at / logits:
// fp32 [n][2][h][w] each.  obey: the range flag applies (an fp16 precision), as FINAL's F::kFlag.
template <class E>
__global__ void __launch_bounds__(256) plane_blend_kernel(const float* __restrict__ at,
                                                          const float* __restrict__ logits,
                                                          const float* __restrict__ coef, PlaneOut p, int h, int w,
                                                          int64_t total, const int32_t* status, bool obey) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % p.w0);
  const int64_t r = i / p.w0;
  const int yo = (int)(r % p.h0);
  const int img = (int)(r / p.h0);
  const int64_t hw = (int64_t)h * w;
  const int64_t px = (int64_t)img * 2 * hw + (int64_t)(yo + p.top) * w + x;
  const float a0[3] = {at[px], 0.0f, 0.0f}, a1[3] = {at[px + hw], 0.0f, 0.0f};
  float o[3];
  mask_blend(coef + img * 8, logits[px], logits[px + hw], a0, a1, o);
  const float q = o[0] < 0.0f ? 0.0f : (o[0] > 1.0f ? 1.0f : o[0]);
  const bool poison = obey && status && *status != 0;  // an fp16 overflow upstream (range guard)
  // FINAL's store rule (final_byte / final_word): one fp32 multiply, truncation toward zero
  const int v = poison ? 0 : (int)(q * (float)p.maxval);
  static_cast<E*>(p.out)[(int64_t)img * p.stride + (int64_t)yo * p.pitch + x] = (E)(v << p.shift);
}

// ---- host side -----------------------------------------------------------------------
int plane_check(const rrin_aux_plane* pl, int frames, int n, int h0, int w0, int h, int w) {
  if (!pl || !pl->a0 || !pl->a1 || !pl->out || !pl->scratch) return RRIN_E_ARG;
  if (pl->depth < 8 || pl->depth > 16 || pl->shift < 0 || pl->shift > 16 - pl->depth) return RRIN_E_ARG;
  if (pl->depth == 8 && pl->shift != 0) return RRIN_E_ARG;
  if (n < 1 || frames < 1 || h0 < 1 || w0 < 1 || h0 > h || w0 > w) return RRIN_E_SHAPE;
  if (pl->depth > 8 && (((uintptr_t)pl->a0 | (uintptr_t)pl->a1 | (uintptr_t)pl->out) & 1)) return RRIN_E_ARG;
  if (pl->in_pitch < w0 || pl->out_pitch < w0) return RRIN_E_ARG;
  if (frames > 1 && pl->in_stride < (int64_t)h0 * pl->in_pitch) return RRIN_E_ARG;
  if (n > 1 && pl->out_stride < (int64_t)h0 * pl->out_pitch) return RRIN_E_ARG;
  if (((uintptr_t)pl->scratch & 3) || pl->scratch_bytes < (int64_t)n * h * w * 16) return RRIN_E_ARG;
  if (((int64_t)n * h * w + 255) / 256 > 0x7fffffff) return RRIN_E_SHAPE;
  return 0;
}

float* plane_logits(const rrin_aux_plane* pl, int n, int h, int w) {
  return static_cast<float*>(pl->scratch) + (int64_t)n * 2 * h * w;
}
}  // namespace rrin

using namespace rrin;

extern "C" int64_t rrin_plane_scratch_bytes(int32_t n, int32_t h, int32_t w) {
  if (n < 1 || h < 1 || w < 1) return RRIN_E_SHAPE;
  return (int64_t)n * h * w * 16;
}

extern "C" int rrin_plane_warp_h8(const rrin_h8* g16, const rrin_aux_plane* pl, int32_t n, int32_t h0, int32_t w0,
                                  const int32_t* pair_map, int32_t n_pairs, int32_t prec, void* stream) {
  if (!g16 || !pl || !rec_prec(prec)) return RRIN_E_ARG;
  if (n_pairs < 1 || n_pairs > n || (!pair_map && n_pairs != n)) return RRIN_E_ARG;
  if (!h8_ok(*g16, prec) || g16->g_off != 0 || g16->groups * chans_per_rec(prec) < 16) return RRIN_E_SHAPE;
  const int h = g16->g.h, w = g16->g.w;
  if (int rc = plane_check(pl, n_pairs, n, h0, w0, h, w)) return rc;
  const PlaneIn p{pl->a0, pl->a1, pl->in_stride, pl->in_pitch, h0, w0, h - h0, (1 << pl->depth) - 1, pl->shift};
  float* at = static_cast<float*>(pl->scratch);
  const int64_t total = (int64_t)n * h * w;
  const dim3 grid((unsigned)((total + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
  return with_format(prec, [&](auto f) {
    using F = decltype(f);
    auto launch = [&](auto e, auto items) {
      using E = decltype(e);
      hipLaunchKernelGGL((plane_warp_kernel<F, E, decltype(items)::value>), grid, dim3(256), 0, st, rec_view(*g16), p,
                         at, h, w, total, pair_map, n_pairs);
    };
    if (pl->depth == 8) {
      if (pair_map) launch(uint8_t{}, std::true_type{});
      else launch(uint8_t{}, std::false_type{});
    } else {
      if (pair_map) launch(uint16_t{}, std::true_type{});
      else launch(uint16_t{}, std::false_type{});
    }
    return hip_code(hipGetLastError());
  });
}

extern "C" int rrin_plane_blend_h8(const rrin_aux_plane* pl, const float* coef, int32_t n, int32_t h, int32_t w,
                                   int32_t h0, int32_t w0, int32_t prec, const int32_t* status, void* stream) {
  if (!pl || !coef || !rec_prec(prec)) return RRIN_E_ARG;
  if (h < 1 || w < 1) return RRIN_E_SHAPE;
  if (int rc = plane_check(pl, n, n, h0, w0, h, w)) return rc;
  const PlaneOut p{pl->out, pl->out_stride, pl->out_pitch, h0, w0, h - h0, (1 << pl->depth) - 1, pl->shift};
  const float* at = static_cast<const float*>(pl->scratch);
  const float* logits = plane_logits(pl, n, h, w);
  const int64_t total = (int64_t)n * h0 * w0;
  const dim3 grid((unsigned)((total + 255) / 256));
  const bool obey = prec != RRIN_PREC_F32R;
  hipStream_t st = (hipStream_t)stream;
  if (pl->depth == 8)
    hipLaunchKernelGGL(plane_blend_kernel<uint8_t>, grid, dim3(256), 0, st, at, logits, coef, p, h, w, total, status,
                       obey);
  else
    hipLaunchKernelGGL(plane_blend_kernel<uint16_t>, grid, dim3(256), 0, st, at, logits, coef, p, h, w, total, status,
                       obey);
  return hip_code(hipGetLastError());
}
