// Fine-tuning on a clip: training triplets from the frames where they live, and the loss.
// rrin_amd/finetune.py is the definition of both.
//
//   rrin_triplet_crop_u8     I0, It, I1 [K][3][ch][cw] fp32 from K items (frame0, frame_t, frame1, y0,
//   rrin_triplet_crop_u16    x0, flip) over one stack of byte / 16-bit frames given as three planes
//                            (rrin_plane: Y, U, V of any layout, or R, G, B of interleaved RGB): the
//                            crop, the integer colour conversion of yuv.hpp, value / maxval, the flip
//   rrin_tloss               sums[3] = sum sqrt(d^2 + eps), sum |d|, sum d^2 of d = out - target and
//                            grad = w_charb/N * d / sqrt(d^2 + eps) + w_l1/count * sign(d), one pass
//
// Sampler.  A gather bound by its fp32 stores: a lane owns four adjacent output pixels of one row
// of one output tensor and writes one 16-byte store per channel.  Flip 1 (left-right) is built in:
// output group g reads source group groups - 1 - g and stores its four pixels reversed; flip 2
// (top-bottom) reads row ch - 1 - r.  The four samples of a step-1 plane are one load at the
// samples' own alignment, of another step four loads; 4:2:0 / 4:2:2 chroma is two samples, each used
// twice (the crop's origin is a multiple of the chroma block, so a group starts on one).  Every
// element read lies in the crop's rows, between the crop's first and last column.  The items ride
// in the kernel's arguments (copied by the call, like the planes of the frame metrics).
//
// Loss.  The elementwise terms are fp32 with the IEEE square root and division (no contraction, no
// reciprocal); the three sums are float64: per lane, then a fixed shuffle tree, the waves in
// order, one partial per workgroup in the workspace, and a second kernel that adds the partials
// in index order.  Workgroup g takes the tiles g, g + G, ... of kTile elements, G a function of count
// alone.  No atomics: the same bits on every run.
#include <math.h>

#include "common.hpp"
#include "yuv.hpp"

namespace rrin {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// ---- triplet sampler ------------------------------------------------------------------------
constexpr int kMaxItems = RRIN_TRIPLET_MAX_ITEMS;

struct Item {
  int32_t frame[3];  // frame0, frame_t, frame1
  int32_t y0, x0, flip;
};
static_assert(sizeof(Item) == 6 * sizeof(int32_t), "an item is six int32");

struct CropArgs {
  rrin_plane p[3];
  rrin_yuv_coef k;
  int64_t frame_stride;  // elements
  float* out[3];
  int32_t yuv;           // 0: the planes are R, G, B
  int32_t by_log, bx_log;  // log2 of the chroma block (rows, columns)
  int32_t ch, cw;
  int32_t shift, maxv, mid;
  Item items[kMaxItems];
};

__device__ inline int to_sample(uint8_t v, int, int) { return (int)v; }
__device__ inline int to_sample(uint16_t v, int shift, int maxv) { return sample16(v, shift, maxv); }

// COUNT (4 or 2) adjacent samples of a plane's row, p at the first
template <int COUNT, typename T>
__device__ inline void load_samples(const T* p, int step, int shift, int maxv, int* s) {
  if (step == 1) {
    T raw[COUNT];
    __builtin_memcpy(raw, p, COUNT * sizeof(T));  // one load, at the samples' alignment
#pragma unroll
    for (int j = 0; j < COUNT; ++j) s[j] = to_sample(raw[j], shift, maxv);
  } else {
#pragma unroll
    for (int j = 0; j < COUNT; ++j) s[j] = to_sample(p[(int64_t)j * step], shift, maxv);
  }
}

template <typename T>
__device__ inline const T* sample_at(const T* frame, const rrin_plane& P, int r, int c) {
  return frame + P.off + (int64_t)r * P.pitch + (int64_t)c * P.step;
}

template <typename T>
__global__ void __launch_bounds__(kThreads) triplet_crop_kernel(const T* __restrict__ base, const CropArgs a) {
  const int groups = a.cw >> 2;
  const int t = blockIdx.x * kThreads + threadIdx.x;
  const int g = t % groups, r = t / groups;
  if (r >= a.ch) return;
  const int k = blockIdx.y / 3, f = blockIdx.y % 3;
  const Item& it = a.items[k];
  const bool lr = it.flip == 1;
  const int sy = it.y0 + (it.flip == 2 ? a.ch - 1 - r : r);
  const int sx = it.x0 + 4 * (lr ? groups - 1 - g : g);
  const T* frame = base + (int64_t)it.frame[f] * a.frame_stride;

  int rgb[4][3];
  int s0[4];
  load_samples<4>(sample_at(frame, a.p[0], sy, sx), a.p[0].step, a.shift, a.maxv, s0);
  if (!a.yuv) {
    int s1[4], s2[4];
    load_samples<4>(sample_at(frame, a.p[1], sy, sx), a.p[1].step, a.shift, a.maxv, s1);
    load_samples<4>(sample_at(frame, a.p[2], sy, sx), a.p[2].step, a.shift, a.maxv, s2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      rgb[j][0] = s0[j];
      rgb[j][1] = s1[j];
      rgb[j][2] = s2[j];
    }
  } else {
    int u[4], v[4];
    const int cy = sy >> a.by_log;
    if (a.bx_log) {  // two chroma samples, each over two pixels (sx is even)
      int u2[2], v2[2];
      load_samples<2>(sample_at(frame, a.p[1], cy, sx >> 1), a.p[1].step, a.shift, a.maxv, u2);
      load_samples<2>(sample_at(frame, a.p[2], cy, sx >> 1), a.p[2].step, a.shift, a.maxv, v2);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        u[j] = u2[j >> 1];
        v[j] = v2[j >> 1];
      }
    } else {
      load_samples<4>(sample_at(frame, a.p[1], cy, sx), a.p[1].step, a.shift, a.maxv, u);
      load_samples<4>(sample_at(frame, a.p[2], cy, sx), a.p[2].step, a.shift, a.maxv, v);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (sizeof(T) == 1)
        yuv_to_rgb(a.k, s0[j], u[j], v[j], rgb[j]);
      else
        yuv_to_rgb16(a.k, a.mid, a.maxv, s0[j], u[j], v[j], rgb[j]);
    }
  }
  const float maxf = (float)a.maxv;
  float* out = a.out[f] + (((int64_t)k * 3) * a.ch + r) * a.cw + 4 * g;
  const int64_t plane = (int64_t)a.ch * a.cw;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float4 q;
    q.x = sample_to_float(lr ? rgb[3][c] : rgb[0][c], maxf);
    q.y = sample_to_float(lr ? rgb[2][c] : rgb[1][c], maxf);
    q.z = sample_to_float(lr ? rgb[1][c] : rgb[2][c], maxf);
    q.w = sample_to_float(lr ? rgb[0][c] : rgb[3][c], maxf);
    *reinterpret_cast<float4*>(out + c * plane) = q;
  }
}

template <typename T>
int triplet_crop(const T* frames, int64_t frame_stride, int32_t n_frames, const rrin_plane* planes,
                 const int32_t* items, int32_t n_items, int32_t ch, int32_t cw, const rrin_yuv_coef* coef, int32_t depth,
                 int32_t shift, float* i0, float* it, float* i1, void* stream) {
  if (!frames || !planes || !items || !i0 || !it || !i1) return RRIN_E_ARG;
  if ((uintptr_t)frames & (sizeof(T) - 1)) return RRIN_E_ARG;
  if (((uintptr_t)i0 | (uintptr_t)it | (uintptr_t)i1) & 15) return RRIN_E_ARG;  // 16-byte stores
  if (n_frames < 1 || n_items < 1 || n_items > kMaxItems) return RRIN_E_SHAPE;
  if (ch < 16 || cw < 16 || (ch & 15) || (cw & 15)) return RRIN_E_SHAPE;
  if (coef) {
    // the integer conversion holds int32 for 8-bit bytes and for 10- and 12-bit samples (yuv.hpp)
    if (sizeof(T) == 2 && depth != 10 && depth != 12) return RRIN_E_ARG;
    const int rc = sizeof(T) == 1 ? yuv_coef_check(coef) : yuv_coef_check16(coef, depth);
    if (rc) return rc;
  }
  int64_t extent = 0;
  for (int p = 0; p < 3; ++p) {
    const rrin_plane& P = planes[p];
    if (P.step < 1 || P.step > 3 || P.off < 0) return RRIN_E_ARG;
    if (P.h < 1 || P.w < 1) return RRIN_E_SHAPE;
    if (P.pitch < (int64_t)(P.w - 1) * P.step + 1) return RRIN_E_ARG;
    const int64_t e = P.off + (int64_t)(P.h - 1) * P.pitch + (int64_t)(P.w - 1) * P.step + 1;
    if (e > extent) extent = e;
  }
  if (frame_stride < extent) return RRIN_E_ARG;
  const rrin_plane &Y = planes[0], &U = planes[1], &V = planes[2];
  if (U.h != V.h || U.w != V.w) return RRIN_E_SHAPE;
  int by_log = 0, bx_log = 0;
  if (!coef) {  // R, G, B: three planes of one size
    if (U.h != Y.h || U.w != Y.w) return RRIN_E_SHAPE;
  } else {      // the chroma block follows from the plane sizes: 4:4:4, 4:2:2 or 4:2:0
    bx_log = U.w == Y.w ? 0 : 1;
    by_log = U.h == Y.h ? 0 : 1;
    if ((int64_t)U.w << bx_log != Y.w || (int64_t)U.h << by_log != Y.h || (by_log && !bx_log)) return RRIN_E_SHAPE;
  }
  if (ch > Y.h || cw > Y.w) return RRIN_E_SHAPE;
  if ((int64_t)ch * (cw >> 2) > (1 << 30)) return RRIN_E_SHAPE;  // lanes of one output tensor of one item
  CropArgs a = {};
  for (int k = 0; k < n_items; ++k) {
    Item& q = a.items[k];
    __builtin_memcpy(&q, items + 6 * k, sizeof(Item));
    for (int f = 0; f < 3; ++f)
      if (q.frame[f] < 0 || q.frame[f] >= n_frames) return RRIN_E_ARG;
    if (q.flip < 0 || q.flip > 2) return RRIN_E_ARG;
    if (q.y0 < 0 || q.x0 < 0 || q.y0 > Y.h - ch || q.x0 > Y.w - cw) return RRIN_E_SHAPE;  // leaves the plane
    if ((q.y0 & ((1 << by_log) - 1)) || (q.x0 & ((1 << bx_log) - 1))) return RRIN_E_ARG;  // off the chroma block
  }
  for (int p = 0; p < 3; ++p) a.p[p] = planes[p];
  if (coef) a.k = *coef;
  a.frame_stride = frame_stride;
  a.out[0] = i0;
  a.out[1] = it;
  a.out[2] = i1;
  a.yuv = coef ? 1 : 0;
  a.by_log = by_log;
  a.bx_log = bx_log;
  a.ch = ch;
  a.cw = cw;
  a.shift = shift;
  a.maxv = (1 << depth) - 1;
  a.mid = 1 << (depth - 1);
  const int64_t lanes = (int64_t)ch * (cw >> 2);
  hipLaunchKernelGGL(triplet_crop_kernel<T>, dim3((unsigned)((lanes + kThreads - 1) / kThreads), 3 * n_items),
                     dim3(kThreads), 0, (hipStream_t)stream, frames, a);
  return hip_code(hipGetLastError());
}

// ---- loss -----------------------------------------------------------------------------------
constexpr int kTile = kThreads * 4 * 2;  // elements of a tile: two 16-byte groups per lane
constexpr int kMaxGroups = 1024;         // workgroups, hence partials, of a call

struct Sums3 {
  double s[3];
};

inline int64_t tloss_groups(int64_t count) {
  const int64_t tiles = (count + kTile - 1) / kTile;
  return tiles < kMaxGroups ? tiles : kMaxGroups;
}

#pragma clang fp contract(off)
// one element: its three terms into acc, its gradient returned
__device__ inline float tloss_term(float o, float t, float eps, float cw, float lw, double* acc) {
  const float d = o - t;
  const float q = d * d;
  const float s = sqrtf(q + eps);  // the correctly rounded root (__fsqrt_rn is the native one here)
  const float m = fabsf(d);
  acc[0] += (double)s;
  acc[1] += (double)m;
  acc[2] += (double)q;
  const float sign = (float)((d > 0.0f) - (d < 0.0f));
  return __fdiv_rn(cw * d, s) + lw * sign;
}
#pragma clang fp contract(on)

// VEC: out, target and grad are 16-byte aligned
template <bool VEC>
__global__ void __launch_bounds__(kThreads) tloss_kernel(const float* __restrict__ out, const float* __restrict__ target,
                                                         int64_t count, float eps, float cw, float lw,
                                                         float* __restrict__ grad, Sums3* __restrict__ part) {
  __shared__ double s_acc[kWaves][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tiles = (count + kTile - 1) / kTile;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t e = tile * kTile + (int64_t)i * (kThreads * 4) + threadIdx.x * 4;
      if (VEC && e + 4 <= count) {
        const float4 o = *reinterpret_cast<const float4*>(out + e);
        const float4 t = *reinterpret_cast<const float4*>(target + e);
        float4 g;
        g.x = tloss_term(o.x, t.x, eps, cw, lw, acc);
        g.y = tloss_term(o.y, t.y, eps, cw, lw, acc);
        g.z = tloss_term(o.z, t.z, eps, cw, lw, acc);
        g.w = tloss_term(o.w, t.w, eps, cw, lw, acc);
        if (grad) *reinterpret_cast<float4*>(grad + e) = g;
      } else {
        for (int64_t j = e; j < e + 4 && j < count; ++j) {
          const float g = tloss_term(out[j], target[j], eps, cw, lw, acc);
          if (grad) grad[j] = g;
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 64);
    if (lane == 0) s_acc[wave][c] = acc[c];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Sums3 t = {{0.0, 0.0, 0.0}};
#pragma unroll
    for (int v = 0; v < kWaves; ++v)
#pragma unroll
      for (int c = 0; c < 3; ++c) t.s[c] += s_acc[v][c];
    part[blockIdx.x] = t;
  }
}

// sums[c] = the partials' s[c], added in index order
__global__ void __launch_bounds__(64) tloss_finish_kernel(const Sums3* __restrict__ part, int groups, double* sums) {
  const int c = threadIdx.x;
  if (c >= 3) return;
  double s = 0.0;
  for (int g = 0; g < groups; ++g) s += part[g].s[c];
  sums[c] = s;
}

}  // namespace
}  // namespace rrin

using namespace rrin;

extern "C" int rrin_triplet_crop_u8(const uint8_t* frames, int64_t frame_stride, int32_t n_frames,
                                    const rrin_plane* planes, const int32_t* items, int32_t n_items, int32_t ch,
                                    int32_t cw, const rrin_yuv_coef* coef, float* i0, float* it, float* i1,
                                    void* stream) {
  return triplet_crop(frames, frame_stride, n_frames, planes, items, n_items, ch, cw, coef, 8, 0, i0, it, i1, stream);
}

extern "C" int rrin_triplet_crop_u16(const uint16_t* frames, int64_t frame_stride, int32_t n_frames,
                                     const rrin_plane* planes, const int32_t* items, int32_t n_items, int32_t ch,
                                     int32_t cw, const rrin_yuv_coef* coef, int32_t depth, int32_t shift, float* i0,
                                     float* it, float* i1, void* stream) {
  if (depth < 9 || depth > 16 || shift < 0 || shift > 16 - depth) return RRIN_E_ARG;
  return triplet_crop(frames, frame_stride, n_frames, planes, items, n_items, ch, cw, coef, depth, shift, i0, it, i1,
                      stream);
}

extern "C" int64_t rrin_tloss_workspace_bytes(int64_t count) {
  return count < 1 ? (int64_t)RRIN_E_SHAPE : tloss_groups(count) * (int64_t)sizeof(Sums3);
}

extern "C" int rrin_tloss(const float* out, const float* target, int64_t count, int32_t n, double w_charb, double w_l1,
                          float eps, double* sums, float* grad, void* workspace, int64_t workspace_bytes,
                          void* stream) {
  if (!out || !target || !sums || !workspace) return RRIN_E_ARG;
  if (((uintptr_t)out | (uintptr_t)target | (uintptr_t)grad) & 3) return RRIN_E_ARG;
  if (((uintptr_t)sums | (uintptr_t)workspace) & 7) return RRIN_E_ARG;
  if (!(eps > 0.0f) || !isfinite(eps) || !isfinite(w_charb) || !isfinite(w_l1)) return RRIN_E_ARG;
  if (count < 1 || n < 1) return RRIN_E_SHAPE;
  const int64_t groups = tloss_groups(count);
  if (workspace_bytes < groups * (int64_t)sizeof(Sums3)) return RRIN_E_WORKSPACE;
  const float cw = (float)(w_charb / (double)n), lw = (float)(w_l1 / (double)count);
  const bool vec = !(((uintptr_t)out | (uintptr_t)target | (uintptr_t)grad) & 15);
  if (vec)
    hipLaunchKernelGGL(tloss_kernel<true>, dim3((unsigned)groups), dim3(kThreads), 0, (hipStream_t)stream, out, target,
                       count, eps, cw, lw, grad, (Sums3*)workspace);
  else
    hipLaunchKernelGGL(tloss_kernel<false>, dim3((unsigned)groups), dim3(kThreads), 0, (hipStream_t)stream, out,
                       target, count, eps, cw, lw, grad, (Sums3*)workspace);
  hipLaunchKernelGGL(tloss_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const Sums3*)workspace,
                     (int)groups, sums);
  return hip_code(hipGetLastError());
}
