// Per-plane squared error and SSIM of frame pairs, where the frames live: the byte and 16-bit
// formats the frame paths emit, read in place (rrin_amd/metrics.py is the definition).
//
//   rrin_frame_metrics_u8    sse[k][p] = sum (a - b)^2 over plane p of frame k, exact, 64 bit; with
//                            flag 1 also ssim[k][p]: the mean over the plane's windows of the 8x8 /
//                            step-4 SSIM (the form of x264 and ffmpeg's ssim filter), float64
//   rrin_frame_metrics_u16   the same over 16-bit words read as min(word >> shift, maxval)
//
// A plane is (off, step, pitch, h, w): sample (r, c) at element off + r*pitch + c*step of the
// frame, so RGB channels (step 3), interleaved chroma (step 2) and planar planes (step 1) are one
// kernel.  One pass over the two frames gives both numbers: a plane is cut into 4x4 blocks; a
// block's sums s1 = sum X, s2 = sum Y, ss = sum X^2 + Y^2, s12 = sum XY are what a window (2x2
// blocks) needs, and ss - 2*s12 is the block's squared error.
//
// Tile.  A wave takes kTileCols + 1 block columns (a lane owns one) and walks down
// kBandRows + 1 block rows: it keeps the previous block row's sums in registers, adds the
// current one (the column's two blocks of a window row) and takes its right neighbour's sum by
// a lane shuffle.  Tiles overlap by one block column and bands by one block row; the block in
// the overlap is counted for the error by the tile / band that starts there (or by the last
// one), so every sample counts once.  The samples beyond the last whole block (h % 4 rows,
// w % 4 columns) take no part in SSIM; the last band and the last tile add their error sample
// by sample.  The four waves of a workgroup take four consecutive (tile, band) units.
//
// Loads.  A lane reads a block row by row: for step-1 bytes one dword per row, for step 2 / 3 the
// two dwords at the row's first and last sample, from which v_perm_b32 picks the four bytes; for
// step-1 words two dwords, else four words.  Every byte read lies between two samples of the
// plane's row, at the samples' own alignment: nothing outside the frame is touched, whatever
// its address.  The next block row is loaded before the current one is reduced.
//
// Arithmetic.  8-bit sums stay in int32 (64*SS <= 64 * 128 * 255^2 < 2^30), 16-bit ones in int64;
// the window value is two float64 products of exact integers and one division, accumulated in
// float64 per lane.  Lanes are added by a fixed shuffle tree, waves in order, and every workgroup
// writes one partial (uint64 error, float64 window sum) to the workspace; a second kernel adds a
// plane's partials in index order and divides by the window count.  No atomics: the same bits on
// every run.
#include <math.h>

#include <type_traits>

#include "common.hpp"

namespace rrin {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTileCols = 63;  // window columns of a wave's tile: its 64 block columns less the shuffle's last
constexpr int kBandRows = 8;   // window rows of a band: kBandRows + 1 block rows

struct Planes {
  rrin_plane p[4];
};
struct Partial {
  uint64_t sse;
  double wsum;
};

// tiles across bw block columns / bands down bh block rows: each owns kTileCols / kBandRows of
// them, the last one one more; at least one (it takes the remainder samples)
__host__ __device__ inline int tiles_of(int bw) {
  const int t = (bw - 2 + kTileCols) / kTileCols;
  return t < 1 ? 1 : t;
}
__host__ __device__ inline int bands_of(int bh) {
  const int t = (bh - 2 + kBandRows) / kBandRows;
  return t < 1 ? 1 : t;
}

template <typename T>
struct Fmt;
template <>
struct Fmt<uint8_t> {
  typedef int32_t Acc;
  typedef uint32_t Row;  // four samples, one per byte
};
template <>
struct Fmt<uint16_t> {
  typedef int64_t Acc;
  typedef uint2 Row;  // four words
};

template <typename Acc>
struct Sums {
  int32_t s1, s2;
  Acc ss, s12;
};

__device__ inline uint32_t load_dword(const void* p) {  // at any alignment
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

// the four samples of a block's row, as loaded
template <int STEP>
__device__ inline uint32_t load_row(const uint8_t* p) {
  const uint32_t d0 = load_dword(p);
  if (STEP == 1) return d0;
  // bytes 0, STEP of the first dword and the two last samples of the dword that ends at sample 3
  const uint32_t d1 = load_dword(p + 3 * STEP - 3);
  return __builtin_amdgcn_perm(d1, d0, STEP == 2 ? 0x07050200u : 0x07040300u);
}
template <int STEP>
__device__ inline uint2 load_row(const uint16_t* p) {
  if (STEP == 1) return make_uint2(load_dword(p), load_dword(p + 2));
  return make_uint2((uint32_t)p[0] | ((uint32_t)p[STEP] << 16), (uint32_t)p[2 * STEP] | ((uint32_t)p[3 * STEP] << 16));
}

__device__ inline void add_row(Sums<int32_t>& s, uint32_t x, uint32_t y, int, int) {
  s.s1 = (int32_t)__builtin_amdgcn_sad_u8(x, 0u, (uint32_t)s.s1);
  s.s2 = (int32_t)__builtin_amdgcn_sad_u8(y, 0u, (uint32_t)s.s2);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int32_t a = (int32_t)((x >> (8 * k)) & 0xffu), b = (int32_t)((y >> (8 * k)) & 0xffu);
    s.ss += a * a + b * b;
    s.s12 += a * b;
  }
}
__device__ inline void add_row(Sums<int64_t>& s, uint2 x, uint2 y, int shift, int maxv) {
  const uint32_t xs[4] = {x.x & 0xffffu, x.x >> 16, x.y & 0xffffu, x.y >> 16};
  const uint32_t ys[4] = {y.x & 0xffffu, y.x >> 16, y.y & 0xffffu, y.y >> 16};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t a = (uint32_t)min((int)(xs[k] >> shift), maxv), b = (uint32_t)min((int)(ys[k] >> shift), maxv);
    s.s1 += (int32_t)a;
    s.s2 += (int32_t)b;
    s.ss += (int64_t)((uint64_t)a * a + (uint64_t)b * b);
    s.s12 += (int64_t)((uint64_t)a * b);
  }
}

__device__ inline int sample_of(const uint8_t* p, int, int) { return (int)*p; }
__device__ inline int sample_of(const uint16_t* p, int shift, int maxv) { return min((int)*p >> shift, maxv); }

template <typename T>
__device__ inline uint64_t sq_err(const T* pa, const T* pb, int shift, int maxv) {
  const int d = sample_of(pa, shift, maxv) - sample_of(pb, shift, maxv);
  return (uint64_t)((uint32_t)(d < 0 ? -d : d) * (uint32_t)(d < 0 ? -d : d));
}

template <typename Acc>
__device__ inline Sums<Acc> shfl_right(const Sums<Acc>& d) {
  Sums<Acc> r;
  r.s1 = __shfl_down(d.s1, 1, 64);
  r.s2 = __shfl_down(d.s2, 1, 64);
  r.ss = (Acc)__shfl_down(d.ss, 1, 64);
  r.s12 = (Acc)__shfl_down(d.s12, 1, 64);
  return r;
}

// One (tile, band) unit of plane P of one frame pair, by one wave: the lane's squared error and
// window sum are added to sse / wsum.
template <typename T, int STEP>
__device__ inline void unit_body(const T* fa, const T* fb, const rrin_plane& P, int unit, int lane, bool ssim,
                                 int shift, int maxv, int64_t c1, int64_t c2, uint64_t& sse, double& wsum) {
  typedef typename Fmt<T>::Acc Acc;
  typedef typename Fmt<T>::Row Row;
  const int h = P.h, w = P.w, bh = h >> 2, bw = w >> 2;
  const int tiles = tiles_of(bw), bands = bands_of(bh);
  const int tx = unit % tiles, by = unit / tiles;
  if (by >= bands) return;
  const bool last_t = tx == tiles - 1, last_b = by == bands - 1;
  const int j = tx * kTileCols + lane;  // the lane's block column
  const bool col = j < bw;
  const bool own_col = col && (lane < kTileCols || last_t);
  const int i0 = by * kBandRows, i1 = min(i0 + kBandRows + 1, bh);
  const int64_t pitch = P.pitch;
  const T* pa = fa + P.off + (int64_t)4 * j * STEP;  // the column's first sample; read only if col
  const T* pb = fb + P.off + (int64_t)4 * j * STEP;

  Row ca[4] = {}, cb[4] = {}, na[4] = {}, nb[4] = {};
  if (col && i0 < i1) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ca[r] = load_row<STEP>(pa + ((int64_t)4 * i0 + r) * pitch);
      cb[r] = load_row<STEP>(pb + ((int64_t)4 * i0 + r) * pitch);
    }
  }
  Sums<Acc> prev = {};
  for (int i = i0; i < i1; ++i) {
    if (col && i + 1 < i1) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        na[r] = load_row<STEP>(pa + ((int64_t)4 * (i + 1) + r) * pitch);
        nb[r] = load_row<STEP>(pb + ((int64_t)4 * (i + 1) + r) * pitch);
      }
    }
    Sums<Acc> s = {};
    if (col) {
#pragma unroll
      for (int r = 0; r < 4; ++r) add_row(s, ca[r], cb[r], shift, maxv);
    }
    if (own_col && (i < i0 + kBandRows || last_b)) sse += (uint64_t)(s.ss - 2 * s.s12);
    if (ssim && i > i0) {  // the window row (i - 1, i): uniform over the wave, so every lane shuffles
      const Sums<Acc> d = {prev.s1 + s.s1, prev.s2 + s.s2, prev.ss + s.ss, prev.s12 + s.s12};
      const Sums<Acc> r = shfl_right(d);
      if (lane < kTileCols && j + 1 < bw) {
        const Acc S1 = (Acc)d.s1 + r.s1, S2 = (Acc)d.s2 + r.s2, SS = d.ss + r.ss, S12 = d.s12 + r.s12;
        const Acc vars = 64 * SS - S1 * S1 - S2 * S2, covar = 64 * S12 - S1 * S2;
        const double num = (double)(2 * S1 * S2 + (Acc)c1) * (double)(2 * covar + (Acc)c2);
        const double den = (double)(S1 * S1 + S2 * S2 + (Acc)c1) * (double)(vars + (Acc)c2);
        wsum += num / den;
      }
    }
    prev = s;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ca[r] = na[r];
      cb[r] = nb[r];
    }
  }
  // the samples SSIM ignores.  Rows below the last whole block: the last band, every owned column.
  if (last_b && own_col) {
    for (int r = 4 * bh; r < h; ++r) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        sse += sq_err(pa + (int64_t)r * pitch + c * STEP, pb + (int64_t)r * pitch + c * STEP, shift, maxv);
    }
  }
  // Columns right of the last whole block: the last tile, over the band's own rows (the last
  // band's reach to h, so the corner is counted here and only here).
  if (last_t && 4 * bw < w) {
    const int r1 = last_b ? h : 4 * kBandRows * (by + 1);
    for (int r = 4 * kBandRows * by + lane; r < r1; r += 64) {
      for (int c = 4 * bw; c < w; ++c) {
        const int64_t o = P.off + (int64_t)r * pitch + (int64_t)c * STEP;
        sse += sq_err(fa + o, fb + o, shift, maxv);
      }
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(kThreads) frame_metrics_kernel(const T* __restrict__ a, int64_t a_stride,
                                                                 const T* __restrict__ b, int64_t b_stride, Planes pl,
                                                                 int n_planes, int flags, int shift, int maxv,
                                                                 int64_t c1, int64_t c2, Partial* part) {
  __shared__ uint64_t s_sse[kWaves];
  __shared__ double s_w[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = blockIdx.y, p = blockIdx.z;
  const rrin_plane P = pl.p[p];
  const T* fa = a + (int64_t)k * a_stride;
  const T* fb = b + (int64_t)k * b_stride;
  const int unit = blockIdx.x * kWaves + wave;
  const bool ssim = (flags & 1) != 0;
  uint64_t sse = 0;
  double wsum = 0.0;
  if (P.step == 1)
    unit_body<T, 1>(fa, fb, P, unit, lane, ssim, shift, maxv, c1, c2, sse, wsum);
  else if (P.step == 2)
    unit_body<T, 2>(fa, fb, P, unit, lane, ssim, shift, maxv, c1, c2, sse, wsum);
  else
    unit_body<T, 3>(fa, fb, P, unit, lane, ssim, shift, maxv, c1, c2, sse, wsum);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sse += (uint64_t)__shfl_xor((long long)sse, o, 64);
    wsum += __shfl_xor(wsum, o, 64);
  }
  if (lane == 0) {
    s_sse[wave] = sse;
    s_w[wave] = wsum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Partial t = {0, 0.0};
#pragma unroll
    for (int v = 0; v < kWaves; ++v) {
      t.sse += s_sse[v];
      t.wsum += s_w[v];
    }
    part[((int64_t)k * n_planes + p) * gridDim.x + blockIdx.x] = t;
  }
}

// sse / ssim [n][n_planes] from the partials [n][n_planes][gx], added in index order
__global__ void __launch_bounds__(kThreads) frame_metrics_finish_kernel(const Partial* __restrict__ part, int gx,
                                                                        int total, Planes pl, int n_planes, int flags,
                                                                        uint64_t* sse, double* ssim) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  uint64_t e = 0;
  double s = 0.0;
  for (int g = 0; g < gx; ++g) {
    const Partial q = part[(int64_t)t * gx + g];
    e += q.sse;
    s += q.wsum;
  }
  sse[t] = e;
  if (flags & 1) {
    const rrin_plane P = pl.p[t % n_planes];
    ssim[t] = s / (double)((int64_t)((P.h >> 2) - 1) * ((P.w >> 2) - 1));
  }
}

// The argument rules of the three entry points on the planes; gx: workgroups per frame and plane,
// extent: elements of a frame the planes reach.
int check_planes(int32_t n, const rrin_plane* planes, int32_t n_planes, int32_t flags, int64_t* gx, int64_t* extent) {
  if (!planes || n_planes < 1 || n_planes > 4 || (flags & ~1)) return RRIN_E_ARG;
  if (n < 1 || n > 65535) return RRIN_E_SHAPE;  // one frame per blockIdx.y
  int64_t g = 1, ext = 0;
  for (int p = 0; p < n_planes; ++p) {
    const rrin_plane& P = planes[p];
    if (P.step < 1 || P.step > 3 || P.off < 0) return RRIN_E_ARG;
    if (P.h < 1 || P.w < 1) return RRIN_E_SHAPE;
    if ((flags & 1) && (P.h < 8 || P.w < 8)) return RRIN_E_SHAPE;
    if (P.pitch < (int64_t)(P.w - 1) * P.step + 1) return RRIN_E_ARG;
    const int64_t units = (int64_t)tiles_of(P.w >> 2) * bands_of(P.h >> 2);
    const int64_t wg = (units + kWaves - 1) / kWaves;
    if (wg > g) g = wg;
    const int64_t e = P.off + (int64_t)(P.h - 1) * P.pitch + (int64_t)(P.w - 1) * P.step + 1;
    if (e > ext) ext = e;
  }
  if (g > 0x7fffffff) return RRIN_E_SHAPE;
  *gx = g;
  *extent = ext;
  return RRIN_OK;
}

template <typename T>
int frame_metrics(const T* a, int64_t a_stride, const T* b, int64_t b_stride, int32_t n, const rrin_plane* planes,
                  int32_t n_planes, int32_t flags, int32_t depth, int32_t shift, uint64_t* sse, double* ssim,
                  void* workspace, int64_t workspace_bytes, void* stream) {
#pragma clang fp contract(off)
  if (!a || !b || !sse || !workspace) return RRIN_E_ARG;
  if (((uintptr_t)sse & 7) || ((uintptr_t)workspace & 7)) return RRIN_E_ARG;
  if (((uintptr_t)a | (uintptr_t)b) & (sizeof(T) - 1)) return RRIN_E_ARG;
  int64_t gx = 0, extent = 0;
  const int rc = check_planes(n, planes, n_planes, flags, &gx, &extent);
  if (rc) return rc;
  if ((flags & 1) && (!ssim || ((uintptr_t)ssim & 7))) return RRIN_E_ARG;
  if (a_stride < extent || b_stride < extent) return RRIN_E_ARG;
  if (workspace_bytes < (int64_t)n * n_planes * gx * (int64_t)sizeof(Partial)) return RRIN_E_WORKSPACE;
  Planes pl = {};
  for (int p = 0; p < n_planes; ++p) pl.p[p] = planes[p];
  const int maxv = (1 << depth) - 1;
  const double m2 = (double)((int64_t)maxv * maxv);
  const int64_t c1 = (int64_t)floor(1e-4 * m2 * 64.0 + 0.5), c2 = (int64_t)floor(9e-4 * m2 * 64.0 * 63.0 + 0.5);
  hipLaunchKernelGGL(frame_metrics_kernel<T>, dim3((unsigned)gx, n, n_planes), dim3(kThreads), 0, (hipStream_t)stream, a,
                     a_stride, b, b_stride, pl, n_planes, flags, shift, maxv, c1, c2, (Partial*)workspace);
  const int total = n * n_planes;
  hipLaunchKernelGGL(frame_metrics_finish_kernel, dim3((total + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     (hipStream_t)stream, (const Partial*)workspace, (int)gx, total, pl, n_planes, flags, sse, ssim);
  return hip_code(hipGetLastError());
}

}  // namespace
}  // namespace rrin

using namespace rrin;

extern "C" int rrin_frame_metrics_tile(int32_t* tile_cols, int32_t* band_rows) {
  if (!tile_cols || !band_rows) return RRIN_E_ARG;
  *tile_cols = kTileCols;
  *band_rows = kBandRows;
  return RRIN_OK;
}

extern "C" int64_t rrin_frame_metrics_workspace_bytes(int32_t n, const rrin_plane* planes, int32_t n_planes,
                                                      int32_t flags) {
  int64_t gx = 0, extent = 0;
  const int rc = check_planes(n, planes, n_planes, flags, &gx, &extent);
  return rc ? rc : (int64_t)n * n_planes * gx * (int64_t)sizeof(Partial);
}

extern "C" int rrin_frame_metrics_u8(const uint8_t* a, int64_t a_stride, const uint8_t* b, int64_t b_stride, int32_t n,
                                     const rrin_plane* planes, int32_t n_planes, int32_t flags, uint64_t* sse,
                                     double* ssim, void* workspace, int64_t workspace_bytes, void* stream) {
  return frame_metrics(a, a_stride, b, b_stride, n, planes, n_planes, flags, 8, 0, sse, ssim, workspace,
                       workspace_bytes, stream);
}

extern "C" int rrin_frame_metrics_u16(const uint16_t* a, int64_t a_stride, const uint16_t* b, int64_t b_stride,
                                      int32_t n, const rrin_plane* planes, int32_t n_planes, int32_t flags,
                                      int32_t depth, int32_t shift, uint64_t* sse, double* ssim, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
  if (depth < 9 || depth > 16 || shift < 0 || shift > 16 - depth) return RRIN_E_ARG;
  return frame_metrics(a, a_stride, b, b_stride, n, planes, n_planes, flags, depth, shift, sse, ssim, workspace,
                       workspace_bytes, stream);
}
