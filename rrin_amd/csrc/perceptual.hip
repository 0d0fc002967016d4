// The perceptual (VGG feature) term of fine-tuning: what the conv stack needs besides its convs.
// rrin_amd/perceptual.py is the definition; the convs are the training path's (rrin_tconv3x3 / the
// Winograd route of rrin_amd/autograd.py) with a linear epilogue.
//
//   rrin_trelu_fwd / _bwd      y = x < 0 ? +0 : x (torch.relu: -0 and NaN pass);  gx = y > 0 ? gy : 0
//   rrin_tmaxpool2_fwd / _bwd  MaxPool2d(2, 2) over [nc][h][w]; the backward finds the arg-max in x again
//                              (first maximum in row-major order, the last NaN if there is one) and
//                              writes all four gradients of a window: no index tensor, no atomics
//   rrin_tfeatdist             sums[0] = sum (a - b)^2 in float64, grad = (a - b) / sqrt(sums[0])
//
// All of them stream contiguous fp32 once and are bound by memory: 16-byte accesses where the
// pointers (pool: and the row length) allow, single elements otherwise and for the tail; the grid is
// a function of the shape alone (capped, the rest by stride), so a call launches the same grid every
// time.  The sum follows rrin_tloss (finetune.hip): float64 per lane, a fixed shuffle tree, the waves
// in order, one partial per workgroup in the workspace, a one-workgroup step that adds the partials
// in index order -- no atomics, the same bits on every run.  The gradient needs the finished sum, so
// it is a launch of its own that reads sums[0] from device memory.
#include <math.h>

#include "common.hpp"

namespace rrin {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxGrid = 2048;  // workgroups of an elementwise launch (256 CUs x 8)

// workgroups for `units` lanes' worth of work
inline unsigned grid_for(int64_t units) {
  const int64_t g = (units + kThreads - 1) / kThreads;
  return (unsigned)(g < 1 ? 1 : (g < kMaxGrid ? g : kMaxGrid));
}

inline bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
  return !(((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15);
}

// ---- ReLU -------------------------------------------------------------------------------------
__device__ inline float relu1(float x) { return x < 0.0f ? 0.0f : x; }
__device__ inline float relu_bwd1(float gy, float y) { return y > 0.0f ? gy : 0.0f; }

// x may be y: a lane reads its elements before it writes them, and no other lane touches them
template <bool VEC>
__global__ void __launch_bounds__(kThreads) trelu_fwd_kernel(const float* x, float* y, int64_t count) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t groups = VEC ? count >> 2 : 0;
  for (int64_t g = t; g < groups; g += stride) {
    float4 v = reinterpret_cast<const float4*>(x)[g];
    v.x = relu1(v.x);
    v.y = relu1(v.y);
    v.z = relu1(v.z);
    v.w = relu1(v.w);
    reinterpret_cast<float4*>(y)[g] = v;
  }
  for (int64_t j = groups * 4 + t; j < count; j += stride) y[j] = relu1(x[j]);
}

// gy may be gx
template <bool VEC>
__global__ void __launch_bounds__(kThreads) trelu_bwd_kernel(const float* gy, const float* __restrict__ y, float* gx,
                                                             int64_t count) {
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t groups = VEC ? count >> 2 : 0;
  for (int64_t g = t; g < groups; g += stride) {
    float4 v = reinterpret_cast<const float4*>(gy)[g];
    const float4 a = reinterpret_cast<const float4*>(y)[g];
    v.x = relu_bwd1(v.x, a.x);
    v.y = relu_bwd1(v.y, a.y);
    v.z = relu_bwd1(v.z, a.z);
    v.w = relu_bwd1(v.w, a.w);
    reinterpret_cast<float4*>(gx)[g] = v;
  }
  for (int64_t j = groups * 4 + t; j < count; j += stride) gx[j] = relu_bwd1(gy[j], y[j]);
}

// ---- 2x2 max pool -----------------------------------------------------------------------------
// The window (a b / c d) in row-major order, PyTorch's CPU scan: a later element replaces the
// maximum if it is greater or a NaN, so the first of equal maxima stays and the last NaN wins.
__device__ inline int argmax4(float a, float b, float c, float d, float* m) {
  float v = a;
  int k = 0;
  if (b > v || b != b) v = b, k = 1;
  if (c > v || c != c) v = c, k = 2;
  if (d > v || d != d) v = d, k = 3;
  *m = v;
  return k;
}

// A unit is one window, or with VEC two adjacent ones (w a multiple of 4, 16-byte aligned tensors:
// one 16-byte load per input row).  Unit u = (plane c, output row yo, unit xu of the row).
template <bool VEC>
__global__ void __launch_bounds__(kThreads) tmaxpool2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                 int w, int64_t units) {
  const int wo = w >> 1;
  const int per_row = VEC ? wo >> 1 : wo;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t u = (int64_t)blockIdx.x * kThreads + threadIdx.x; u < units; u += stride) {
    const int xu = (int)(u % per_row);
    const int64_t r = u / per_row;  // c * ho + yo: input rows 2r, 2r + 1 of the [nc * h] rows
    const float* p = x + 2 * r * w + (VEC ? 4 : 2) * xu;
    float* q = y + r * wo + (VEC ? 2 : 1) * xu;
    if (VEC) {
      const float4 t = *reinterpret_cast<const float4*>(p);
      const float4 b = *reinterpret_cast<const float4*>(p + w);
      float2 o;
      argmax4(t.x, t.y, b.x, b.y, &o.x);
      argmax4(t.z, t.w, b.z, b.w, &o.y);
      *reinterpret_cast<float2*>(q) = o;
    } else {
      float o;
      argmax4(p[0], p[1], p[w], p[w + 1], &o);
      *q = o;
    }
  }
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) tmaxpool2_bwd_kernel(const float* __restrict__ gy,
                                                                 const float* __restrict__ x, float* __restrict__ gx,
                                                                 int w, int64_t units) {
  const int wo = w >> 1;
  const int per_row = VEC ? wo >> 1 : wo;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t u = (int64_t)blockIdx.x * kThreads + threadIdx.x; u < units; u += stride) {
    const int xu = (int)(u % per_row);
    const int64_t r = u / per_row;
    const int64_t in = 2 * r * w + (VEC ? 4 : 2) * xu;
    const float* p = x + in;
    float* o = gx + in;
    const float* g = gy + r * wo + (VEC ? 2 : 1) * xu;
    float m;
    if (VEC) {
      const float4 t = *reinterpret_cast<const float4*>(p);
      const float4 b = *reinterpret_cast<const float4*>(p + w);
      const float2 gv = *reinterpret_cast<const float2*>(g);
      const int k0 = argmax4(t.x, t.y, b.x, b.y, &m);
      const int k1 = argmax4(t.z, t.w, b.z, b.w, &m);
      float4 top, bot;
      top.x = k0 == 0 ? gv.x : 0.0f;
      top.y = k0 == 1 ? gv.x : 0.0f;
      bot.x = k0 == 2 ? gv.x : 0.0f;
      bot.y = k0 == 3 ? gv.x : 0.0f;
      top.z = k1 == 0 ? gv.y : 0.0f;
      top.w = k1 == 1 ? gv.y : 0.0f;
      bot.z = k1 == 2 ? gv.y : 0.0f;
      bot.w = k1 == 3 ? gv.y : 0.0f;
      *reinterpret_cast<float4*>(o) = top;
      *reinterpret_cast<float4*>(o + w) = bot;
    } else {
      const int k = argmax4(p[0], p[1], p[w], p[w + 1], &m);
      const float gv = *g;
      o[0] = k == 0 ? gv : 0.0f;
      o[1] = k == 1 ? gv : 0.0f;
      o[w] = k == 2 ? gv : 0.0f;
      o[w + 1] = k == 3 ? gv : 0.0f;
    }
  }
}

int pool_check(const void* a, const void* b, const void* c, int32_t nc, int32_t h, int32_t w) {
  if (!a || !b || !c) return RRIN_E_ARG;
  if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 3) return RRIN_E_ARG;
  if (nc < 1 || h < 2 || w < 2 || (h & 1) || (w & 1)) return RRIN_E_SHAPE;
  return 0;
}

// ---- feature distance -------------------------------------------------------------------------
constexpr int kTile = kThreads * 4 * 2;  // elements of a tile: two 16-byte groups per lane
constexpr int kMaxGroups = 1024;         // workgroups, hence partials, of the sum

inline int64_t featdist_groups(int64_t count) {
  const int64_t tiles = (count + kTile - 1) / kTile;
  return tiles < kMaxGroups ? tiles : kMaxGroups;
}

// the difference of two floats is exact in float64, its square rounded once
__device__ inline void sq_acc(float a, float b, double& acc) {
  const double d = (double)a - (double)b;
  acc += d * d;
}

// VEC: a and b are 16-byte aligned
template <bool VEC>
__global__ void __launch_bounds__(kThreads) featdist_sum_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                int64_t count, double* __restrict__ part) {
  __shared__ double s_acc[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tiles = (count + kTile - 1) / kTile;
  double acc = 0.0;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t e = tile * kTile + (int64_t)i * (kThreads * 4) + threadIdx.x * 4;
      if (VEC && e + 4 <= count) {
        const float4 p = *reinterpret_cast<const float4*>(a + e);
        const float4 q = *reinterpret_cast<const float4*>(b + e);
        sq_acc(p.x, q.x, acc);
        sq_acc(p.y, q.y, acc);
        sq_acc(p.z, q.z, acc);
        sq_acc(p.w, q.w, acc);
      } else {
        for (int64_t j = e; j < e + 4 && j < count; ++j) sq_acc(a[j], b[j], acc);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) s_acc[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) t += s_acc[v];
    part[blockIdx.x] = t;
  }
}

// sums[0] = the partials, added in index order
__global__ void __launch_bounds__(64) featdist_finish_kernel(const double* __restrict__ part, int groups, double* sums) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int g = 0; g < groups; ++g) s += part[g];
  sums[0] = s;
}

// grad = (a - b) / sqrt(sums[0]): the exact difference divided in float64, rounded to fp32 once;
// zeros when the sum is zero (torch.norm's gradient at 0)
__device__ inline float dist_grad1(float a, float b, double norm, bool zero) {
  return zero ? 0.0f : (float)(((double)a - (double)b) / norm);
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) featdist_grad_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                 int64_t count, const double* __restrict__ sums,
                                                                 float* __restrict__ grad) {
  const double s = sums[0];
  const bool zero = s == 0.0;
  const double norm = sqrt(s);
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t groups = VEC ? count >> 2 : 0;
  for (int64_t g = t; g < groups; g += stride) {
    const float4 p = reinterpret_cast<const float4*>(a)[g];
    const float4 q = reinterpret_cast<const float4*>(b)[g];
    float4 v;
    v.x = dist_grad1(p.x, q.x, norm, zero);
    v.y = dist_grad1(p.y, q.y, norm, zero);
    v.z = dist_grad1(p.z, q.z, norm, zero);
    v.w = dist_grad1(p.w, q.w, norm, zero);
    reinterpret_cast<float4*>(grad)[g] = v;
  }
  for (int64_t j = groups * 4 + t; j < count; j += stride) grad[j] = dist_grad1(a[j], b[j], norm, zero);
}

}  // namespace
}  // namespace rrin

using namespace rrin;

extern "C" int rrin_trelu_fwd(const float* x, float* y, int64_t count, void* stream) {
  if (!x || !y) return RRIN_E_ARG;
  if (((uintptr_t)x | (uintptr_t)y) & 3) return RRIN_E_ARG;
  if (count < 1) return RRIN_E_SHAPE;
  if (aligned16(x, y))
    hipLaunchKernelGGL(trelu_fwd_kernel<true>, dim3(grid_for((count + 3) >> 2)), dim3(kThreads), 0, (hipStream_t)stream,
                       x, y, count);
  else
    hipLaunchKernelGGL(trelu_fwd_kernel<false>, dim3(grid_for(count)), dim3(kThreads), 0, (hipStream_t)stream, x, y,
                       count);
  return hip_code(hipGetLastError());
}

extern "C" int rrin_trelu_bwd(const float* gy, const float* y, float* gx, int64_t count, void* stream) {
  if (!gy || !y || !gx) return RRIN_E_ARG;
  if (((uintptr_t)gy | (uintptr_t)y | (uintptr_t)gx) & 3) return RRIN_E_ARG;
  if (count < 1) return RRIN_E_SHAPE;
  if (aligned16(gy, y, gx))
    hipLaunchKernelGGL(trelu_bwd_kernel<true>, dim3(grid_for((count + 3) >> 2)), dim3(kThreads), 0, (hipStream_t)stream,
                       gy, y, gx, count);
  else
    hipLaunchKernelGGL(trelu_bwd_kernel<false>, dim3(grid_for(count)), dim3(kThreads), 0, (hipStream_t)stream, gy, y,
                       gx, count);
  return hip_code(hipGetLastError());
}

extern "C" int rrin_tmaxpool2_fwd(const float* x, float* y, int32_t nc, int32_t h, int32_t w, void* stream) {
  const int rc = pool_check(x, y, x, nc, h, w);
  if (rc) return rc;
  const int64_t windows = (int64_t)nc * (h / 2) * (w / 2);
  if (!(w & 3) && aligned16(x, y))
    hipLaunchKernelGGL(tmaxpool2_fwd_kernel<true>, dim3(grid_for(windows / 2)), dim3(kThreads), 0, (hipStream_t)stream, x,
                       y, w, windows / 2);
  else
    hipLaunchKernelGGL(tmaxpool2_fwd_kernel<false>, dim3(grid_for(windows)), dim3(kThreads), 0, (hipStream_t)stream, x, y,
                       w, windows);
  return hip_code(hipGetLastError());
}

extern "C" int rrin_tmaxpool2_bwd(const float* gy, const float* x, float* gx, int32_t nc, int32_t h, int32_t w,
                                  void* stream) {
  const int rc = pool_check(gy, x, gx, nc, h, w);
  if (rc) return rc;
  const int64_t windows = (int64_t)nc * (h / 2) * (w / 2);
  if (!(w & 3) && aligned16(gy, x, gx))
    hipLaunchKernelGGL(tmaxpool2_bwd_kernel<true>, dim3(grid_for(windows / 2)), dim3(kThreads), 0, (hipStream_t)stream,
                       gy, x, gx, w, windows / 2);
  else
    hipLaunchKernelGGL(tmaxpool2_bwd_kernel<false>, dim3(grid_for(windows)), dim3(kThreads), 0, (hipStream_t)stream, gy,
                       x, gx, w, windows);
  return hip_code(hipGetLastError());
}

extern "C" int64_t rrin_tfeatdist_workspace_bytes(int64_t count) {
  return count < 1 ? (int64_t)RRIN_E_SHAPE : featdist_groups(count) * (int64_t)sizeof(double);
}

extern "C" int rrin_tfeatdist(const float* a, const float* b, int64_t count, double* sums, float* grad, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  if (!a || !b || !sums || !workspace) return RRIN_E_ARG;
  if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)grad) & 3) return RRIN_E_ARG;
  if (((uintptr_t)sums | (uintptr_t)workspace) & 7) return RRIN_E_ARG;
  if (count < 1) return RRIN_E_SHAPE;
  const int64_t groups = featdist_groups(count);
  if (workspace_bytes < groups * (int64_t)sizeof(double)) return RRIN_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (aligned16(a, b))
    hipLaunchKernelGGL(featdist_sum_kernel<true>, dim3((unsigned)groups), dim3(kThreads), 0, st, a, b, count,
                       (double*)workspace);
  else
    hipLaunchKernelGGL(featdist_sum_kernel<false>, dim3((unsigned)groups), dim3(kThreads), 0, st, a, b, count,
                       (double*)workspace);
  hipLaunchKernelGGL(featdist_finish_kernel, dim3(1), dim3(64), 0, st, (const double*)workspace, (int)groups, sums);
  if (grad) {
    if (aligned16(a, b, grad))
      hipLaunchKernelGGL(featdist_grad_kernel<true>, dim3(grid_for((count + 3) >> 2)), dim3(kThreads), 0, st, a, b, count,
                         (const double*)sums, grad);
    else
      hipLaunchKernelGGL(featdist_grad_kernel<false>, dim3(grid_for(count)), dim3(kThreads), 0, st, a, b, count,
                         (const double*)sums, grad);
  }
  return hip_code(hipGetLastError());
}
