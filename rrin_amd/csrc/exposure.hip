// The exposure of a synthetic shutter (rrin_amd/exposure.py is the definition; include/rrin_hip.h
// the contract): rrin_mean_frames, out[g] = the rounded mean of the frames ptr[start[g] .. start[g+1]).
//
// Memory-bound: S reads and one write per output element.  One lane owns one run of ACCESS bytes of
// one output frame (16 B where the caller's addresses allow it: a wave then reads and writes 1 KiB
// per instruction), walks that output's sources with the sums in registers, four loads in flight,
// and writes each element exactly once.  No atomics and no LDS, integer sums: the same bits on every
// run.  The sources are a table of pointers, read through the scalar cache (the index is uniform in a
// workgroup), because they are views of a frame stack and of the outputs of separate item forwards.
// blockIdx.y is the output, blockIdx.x the run; the len % (ACCESS / element) elements behind the last
// whole run belong to one more lane, which takes them one element at a time.  Nothing outside
// [frame, frame + len) is read or written.
#include "common.hpp"

namespace rrin {

// the divide by S: q = floor(n * M / 2^32) with M = floor(2^32 / S) + 1 is floor(n / S) for every
// n * e < 2^32, e = M * S - 2^32 in [1, S].  Here n <= 65535 * S + S / 2 and S <= 256, so
// n * e <= 65535.5 * 65536 < 2^32.  S == 1 has no 32-bit M and needs none.
struct MeanDiv {
  uint32_t magic, half;
  bool one;
  __device__ uint32_t operator()(uint32_t sum) const { return one ? sum : __umulhi(sum + half, magic); }
};

template <class E>
__device__ inline uint32_t mean_sample(E v, int maxval, int shift) {
  if constexpr (sizeof(E) == 1) return v;
  else return min((int)v >> shift, maxval);
}

template <class E, int ACCESS>
struct alignas(ACCESS) MeanVec {
  E e[ACCESS / sizeof(E)];
};

// A frame pointer read from the table is a generic pointer to the compiler (flat_load); the frames are
// device memory, so say so: global_load.
template <int BYTES>
struct MeanRaw;
template <>
struct MeanRaw<16> {
  typedef uint32_t type __attribute__((ext_vector_type(4)));
};
template <>
struct MeanRaw<4> {
  typedef uint32_t type;
};
template <>
struct MeanRaw<2> {
  typedef uint16_t type;
};
template <>
struct MeanRaw<1> {
  typedef uint8_t type;
};

template <class T, class E>
__device__ inline T load_global(const E* p) {
  using R = typename MeanRaw<sizeof(T)>::type;
  const R r = *(const __attribute__((address_space(1))) R*)p;
  T v;
  __builtin_memcpy(&v, &r, sizeof(T));
  return v;
}

template <class E, int ACCESS>
__global__ void __launch_bounds__(256) mean_frames_kernel(const E* const* __restrict__ ptr,
                                                          const int32_t* __restrict__ start, int k_total,
                                                          E* __restrict__ out, int64_t out_stride, int64_t len,
                                                          int maxval, int shift) {
  constexpr int V = ACCESS / sizeof(E);
  using Vec = MeanVec<E, ACCESS>;
  const int g = blockIdx.y;
  const int s0 = max(start[g], 0), s1 = min(start[g + 1], k_total);
  const int s = s1 - s0;
  if (s < 1 || s > 256) return;  // no such table comes from the Python layer; nothing is read or written
  const MeanDiv div{s > 1 ? (uint32_t)(0x100000000ull / (uint32_t)s) + 1u : 0u, (uint32_t)s >> 1, s == 1};
  const E* const* src = ptr + s0;
  E* o = out + (int64_t)g * out_stride;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t whole = len / V;
  if (i < whole) {
    const int64_t off = i * V;
    uint32_t acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0;
    int k = 0;
    for (; k + 4 <= s; k += 4) {
      Vec v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = load_global<Vec>(src[k + j] + off);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] += mean_sample(v[j].e[e], maxval, shift);
    }
    for (; k < s; ++k) {
      const Vec v = load_global<Vec>(src[k] + off);
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] += mean_sample(v.e[e], maxval, shift);
    }
    Vec r;
#pragma unroll
    for (int e = 0; e < V; ++e) r.e[e] = (E)(div(acc[e]) << shift);
    *reinterpret_cast<Vec*>(o + off) = r;
  } else if (V > 1 && i == whole) {
    for (int64_t e = whole * V; e < len; ++e) {
      uint32_t acc = 0;
      for (int k = 0; k < s; ++k) acc += mean_sample(load_global<E>(src[k] + e), maxval, shift);
      o[e] = (E)(div(acc) << shift);
    }
  }
}

template <class E, int ACCESS>
int mean_frames_launch(const void* const* ptr, const int32_t* start, int k_total, int g, void* out, int64_t out_stride,
                       int64_t len, int maxval, int shift, hipStream_t st) {
  constexpr int V = ACCESS / sizeof(E);
  const int64_t lanes = len / V + (len % V ? 1 : 0);
  const int64_t blocks = (lanes + 255) / 256;
  if (blocks > 0x7fffffff) return RRIN_E_SHAPE;
  hipLaunchKernelGGL((mean_frames_kernel<E, ACCESS>), dim3((unsigned)blocks, (unsigned)g), dim3(256), 0, st,
                     reinterpret_cast<const E* const*>(ptr), start, k_total, static_cast<E*>(out), out_stride, len,
                     maxval, shift);
  return hip_code(hipGetLastError());
}
}  // namespace rrin

using namespace rrin;

extern "C" int rrin_mean_frames(const void* const* frames, int32_t k, const int32_t* start, int32_t g, void* out,
                                int64_t out_stride, int64_t len, int32_t depth, int32_t shift, int32_t access,
                                void* stream) {
  if (!frames || !start || !out) return RRIN_E_ARG;
  if (g < 1 || len < 1) return RRIN_E_SHAPE;
  if (depth < 8 || depth > 16 || shift < 0 || shift > 16 - depth) return RRIN_E_ARG;
  if (depth == 8 && shift != 0) return RRIN_E_ARG;
  const int esize = depth == 8 ? 1 : 2;
  if (access != esize && access != 4 && access != 16) return RRIN_E_ARG;
  if (((uintptr_t)frames & 7) || ((uintptr_t)start & 3)) return RRIN_E_ARG;
  // every group has 1..256 frames
  if (k < g || (int64_t)k > (int64_t)g * 256) return RRIN_E_ARG;
  // out and, between frames, out_stride keep every access of the chosen width aligned (an odd
  // 16-bit address fails here too: access >= 2)
  if ((uintptr_t)out % (unsigned)access) return RRIN_E_ARG;
  if (g > 1 && (out_stride < len || (out_stride * esize) % access)) return RRIN_E_ARG;
  if (g > 65535) return RRIN_E_SHAPE;
  const int maxval = (1 << depth) - 1;
  hipStream_t st = (hipStream_t)stream;
  if (esize == 1) {
    if (access == 16) return mean_frames_launch<uint8_t, 16>(frames, start, k, g, out, out_stride, len, maxval, shift, st);
    if (access == 4) return mean_frames_launch<uint8_t, 4>(frames, start, k, g, out, out_stride, len, maxval, shift, st);
    return mean_frames_launch<uint8_t, 1>(frames, start, k, g, out, out_stride, len, maxval, shift, st);
  }
  if (access == 16) return mean_frames_launch<uint16_t, 16>(frames, start, k, g, out, out_stride, len, maxval, shift, st);
  if (access == 4) return mean_frames_launch<uint16_t, 4>(frames, start, k, g, out, out_stride, len, maxval, shift, st);
  return mean_frames_launch<uint16_t, 2>(frames, start, k, g, out, out_stride, len, maxval, shift, st);
}
