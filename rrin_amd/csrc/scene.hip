// Scene-cut / duplicate-frame gate of the 8-bit frame path (ABI 21): the decision is made where
// the frames live, on the forward's own stream, without a host round trip.
//
//   rrin_pair_sad_u8       sad[p] = sum |f0[p] - f1[p]| over a pair's h0*w0*3 bytes, exact, 64 bit
//   rrin_pair_sad_u16      the same over 16-bit words read as min(word >> shift, maxval) (ABI 23)
//   rrin_gate_from_sad_u8  sad -> code per pair: 1 duplicate (sad == 0), cut_code above the limit
//   rrin_gate_frames_u8    code 1 / 2: the output frame is overwritten with f0's / f1's bytes
//   rrin_*_len             the three frame entry points on blobs of any length (ABI 24): the YUV
//                          4:2:2 / 4:4:4 frames, whose size is no multiple of 3
//
// Frames are dense uint8 [h0][w0][3] at any byte address (f1 is usually f0 + one frame of one
// stack: 17 x 33 x 3 = 1683 bytes), so the two operands of a pair have no common alignment.  Both
// kernels split a frame into a head of < 16 bytes, a body of 16-byte vectors and a tail of < 16
// bytes, aligned on ONE operand (f0 for the sum, `out` for the copy: its vectors are plain
// aligned uint4 accesses); the other operand is read as whole dwords from its address rounded
// down to 4 and funnel-shifted into place.  Such a dword always holds at least one byte of the
// frame, so no read touches a page the frame does not, and no store leaves the frame.
#include "common.hpp"

namespace rrin {
namespace {

constexpr int kThreads = 256;
constexpr int kVecs = 8;                            // 16-byte vectors per lane and chunk
constexpr int64_t kChunkVecs = (int64_t)kThreads * kVecs;  // 32 KiB of a frame per workgroup step
constexpr int kMaxGridX = 4096;                     // workgroups per frame (they loop over chunks)

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// head / body / tail of `len` bytes at address `addr`: the body starts at the next multiple of 16
struct Span {
  int64_t head, vecs, tail;
};
__host__ __device__ inline Span span_of(uintptr_t addr, int64_t len) {
  Span s;
  s.head = (int64_t)((16 - (addr & 15)) & 15);
  if (s.head > len) s.head = len;
  s.vecs = (len - s.head) / 16;
  s.tail = len - s.head - 16 * s.vecs;
  return s;
}

// 16 bytes at byte address w + sh + 16 v (w dword aligned, sh = 0..3): dwords 4v .. 4v+3 of w, and
// for sh != 0 dword 4v+4 too, which then holds the last sh bytes asked for (sh == 0 reads dword
// 4v+3 again instead and shifts by nothing: no branch, and no dword past the 16 bytes)
__device__ inline uint4 load16_shifted(const uint32_t* w, uint32_t sh, int64_t v) {
  const u32x4_a4 q = *(const u32x4_a4*)(w + 4 * v);
  const uint32_t e = w[4 * v + 3 + (sh != 0)];
  const uint32_t s8 = 8 * sh;
  auto fsh = [s8](uint32_t hi, uint32_t lo) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> s8); };
  return make_uint4(fsh(q.y, q.x), fsh(q.z, q.y), fsh(q.w, q.z), fsh(e, q.w));
}

__global__ void __launch_bounds__(kThreads) zero_u64_kernel(uint64_t* p, int n) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) p[i] = 0;
}

// One pair per blockIdx.y; the workgroups of a pair walk its 32 KiB chunks.  A lane's 32-bit
// partial covers one chunk only (8 vectors x 4 dwords x at most 4 x 255: < 2^15) and is added
// to a 64-bit lane sum; workgroup 0 of the pair also takes the head and tail bytes.  One 64-bit
// atomic add per workgroup onto sad[p], which zero_u64_kernel cleared earlier on the stream.
__global__ void __launch_bounds__(kThreads) pair_sad_u8_kernel(const uint8_t* __restrict__ f0,
                                                               const uint8_t* __restrict__ f1, int64_t img_stride,
                                                               int64_t len, uint64_t* sad) {
  __shared__ uint64_t s_part[kThreads / 64];
  const int tid = threadIdx.x;
  const int p = blockIdx.y;
  const uint8_t* a = f0 + (int64_t)p * img_stride;
  const uint8_t* b = f1 + (int64_t)p * img_stride;
  const Span sp = span_of((uintptr_t)a, len);
  uint64_t sum = 0;
  if (blockIdx.x == 0 && tid < sp.head + sp.tail) {
    const int64_t i = tid < sp.head ? tid : sp.head + 16 * sp.vecs + (tid - sp.head);
    const int d = (int)a[i] - (int)b[i];
    sum = (uint64_t)(d < 0 ? -d : d);
  }
  const uint4* av = (const uint4*)(a + sp.head);
  const uint32_t sh = (uint32_t)((uintptr_t)(b + sp.head) & 3);
  const uint32_t* bw = (const uint32_t*)(b + sp.head - sh);
  const int64_t chunks = (sp.vecs + kChunkVecs - 1) / kChunkVecs;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    // a vector past the body re-reads the last one (chunks > 0: there is one) and counts nothing,
    // so the chunk's loads issue together
    uint4 x[kVecs], y[kVecs];
#pragma unroll
    for (int k = 0; k < kVecs; ++k) {
      const int64_t v = c * kChunkVecs + (int64_t)k * kThreads + tid;
      const int64_t vc = v < sp.vecs ? v : sp.vecs - 1;
      x[k] = av[vc];
      y[k] = load16_shifted(bw, sh, vc);
    }
    uint32_t part = 0;
#pragma unroll
    for (int k = 0; k < kVecs; ++k) {
      uint32_t q = __builtin_amdgcn_sad_u8(x[k].x, y[k].x, 0u);
      q = __builtin_amdgcn_sad_u8(x[k].y, y[k].y, q);
      q = __builtin_amdgcn_sad_u8(x[k].z, y[k].z, q);
      q = __builtin_amdgcn_sad_u8(x[k].w, y[k].w, q);
      part += c * kChunkVecs + (int64_t)k * kThreads + tid < sp.vecs ? q : 0u;
    }
    sum += part;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if ((tid & 63) == 0) s_part[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) {
    uint64_t t = 0;
#pragma unroll
    for (int k = 0; k < kThreads / 64; ++k) t += s_part[k];
    if (t) atomicAdd((unsigned long long*)&sad[p], (unsigned long long)t);
  }
}

// pair_sad_u8_kernel for frames of `len` 16-bit words, each read as min(word >> shift, maxv).
// Frames start at even addresses, so the body is aligned on f0's dwords (a head of 0 or 1 word, a
// tail of 0 or 1) and f1 is read as whole dwords from its address rounded down to 4, shifted by
// 0 or 16 bits into place: a dword of either always holds a word of the frame.  A lane takes
// kWords dwords per step; its 32-bit partial covers one step (16 words of at most 65535) and is
// added to the 64-bit lane sum.  The reduction and the atomic add are pair_sad_u8_kernel's.
constexpr int kWords = 8;  // dwords per lane and step

__device__ inline uint32_t absdiff16(uint32_t a, uint32_t b, int shift, int maxv) {
  const int x = min((int)(a >> shift), maxv), y = min((int)(b >> shift), maxv);
  return (uint32_t)(x > y ? x - y : y - x);
}

__global__ void __launch_bounds__(kThreads) pair_sad_u16_kernel(const uint16_t* __restrict__ f0,
                                                                const uint16_t* __restrict__ f1, int64_t img_stride,
                                                                int64_t len, int shift, int maxv, uint64_t* sad) {
  __shared__ uint64_t s_part[kThreads / 64];
  const int tid = threadIdx.x;
  const int p = blockIdx.y;
  const uint16_t* a = f0 + (int64_t)p * img_stride;
  const uint16_t* b = f1 + (int64_t)p * img_stride;
  const int64_t head = (int64_t)(((uintptr_t)a >> 1) & 1);  // len >= 1: the head word exists
  const int64_t nd = (len - head) / 2;                        // dwords of the body
  const int64_t tail = len - head - 2 * nd;
  uint64_t sum = 0;
  if (blockIdx.x == 0 && tid < head + tail) {
    const int64_t i = tid < head ? 0 : len - 1;
    sum = absdiff16(a[i], b[i], shift, maxv);
  }
  const uint32_t* aw = (const uint32_t*)(a + head);
  const uint32_t sh = (uint32_t)(((uintptr_t)(b + head) >> 1) & 1);  // b's body starts in a dword's high half
  const uint32_t* bw = (const uint32_t*)(b + head - sh);
  const int64_t step = (int64_t)kThreads * kWords;
  for (int64_t c = (int64_t)blockIdx.x * step; c < nd; c += (int64_t)gridDim.x * step) {
    uint32_t x[kWords], y[kWords];
#pragma unroll
    for (int k = 0; k < kWords; ++k) {
      // a dword past the body re-reads the last one (nd > 0 here) and counts nothing
      const int64_t v = c + (int64_t)k * kThreads + tid;
      const int64_t vc = v < nd ? v : nd - 1;
      x[k] = aw[vc];
      const uint32_t lo = bw[vc], hi = bw[vc + sh];  // sh == 0 reads the same dword twice
      y[k] = sh ? (lo >> 16) | (hi << 16) : lo;
    }
    uint32_t part = 0;
#pragma unroll
    for (int k = 0; k < kWords; ++k) {
      const uint32_t q = absdiff16(x[k] & 0xffffu, y[k] & 0xffffu, shift, maxv) +
                         absdiff16(x[k] >> 16, y[k] >> 16, shift, maxv);
      part += c + (int64_t)k * kThreads + tid < nd ? q : 0u;
    }
    sum += part;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if ((tid & 63) == 0) s_part[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) {
    uint64_t t = 0;
#pragma unroll
    for (int k = 0; k < kThreads / 64; ++k) t += s_part[k];
    if (t) atomicAdd((unsigned long long*)&sad[p], (unsigned long long)t);
  }
}

__global__ void __launch_bounds__(kThreads) gate_from_sad_kernel(const uint64_t* __restrict__ sad, int n,
                                                                 uint64_t limit, int32_t cut_code, int32_t* gate) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const uint64_t s = sad[i];
  gate[i] = s == 0 ? 1 : (s > limit ? cut_code : 0);
}

// An item's code from its pair's (ABI 25): a duplicate pair (1) gives every item the first frame,
// a cut pair (2) gives item k its own cut[k] -- the nearer frame by the item's t --, else 0.
__global__ void __launch_bounds__(kThreads) gate_items_kernel(const int32_t* __restrict__ pair_gate, int n_pairs,
                                                              const int32_t* __restrict__ map,
                                                              const int32_t* __restrict__ cut, int n, int32_t* gate) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t c = pair_gate[pair_of(map, i, n_pairs)];
  const int32_t k = cut[i];
  gate[i] = c == 1 ? 1 : (c == 2 ? (k == 1 || k == 2 ? k : 0) : 0);
}

// One pair per blockIdx.y.  A workgroup of an ungated pair leaves after reading the code; the
// others copy the chosen input frame over the output frame, aligned on the output.  ITEMS (ABI 25):
// output frame p is an item, gated from the frames of pair pair_of(map, p, n_pairs); without it map
// and n_pairs are unused.
template <bool ITEMS>
__global__ void __launch_bounds__(kThreads) gate_frames_u8_kernel(const uint8_t* __restrict__ f0,
                                                                  const uint8_t* __restrict__ f1,
                                                                  int64_t img_stride, int64_t len,
                                                                  const int32_t* __restrict__ gate, uint8_t* out,
                                                                  const int32_t* __restrict__ map, int n_pairs) {
  const int p = blockIdx.y;
  const int32_t code = gate[p];
  if (code != 1 && code != 2) return;
  const int tid = threadIdx.x;
  const int src = ITEMS ? pair_of(map, p, n_pairs) : p;
  const uint8_t* s = (code == 1 ? f0 : f1) + (int64_t)src * img_stride;
  uint8_t* d = out + (int64_t)p * len;
  const Span sp = span_of((uintptr_t)d, len);
  if (blockIdx.x == 0 && tid < sp.head + sp.tail) {
    const int64_t i = tid < sp.head ? tid : sp.head + 16 * sp.vecs + (tid - sp.head);
    d[i] = s[i];
  }
  uint4* dv = (uint4*)(d + sp.head);
  const uint32_t sh = (uint32_t)((uintptr_t)(s + sp.head) & 3);
  const uint32_t* sw = (const uint32_t*)(s + sp.head - sh);
  const int64_t chunks = (sp.vecs + kChunkVecs - 1) / kChunkVecs;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    uint4 x[kVecs];  // as in the sum: clamped loads first, then the stores of the vectors that exist
#pragma unroll
    for (int k = 0; k < kVecs; ++k) {
      const int64_t v = c * kChunkVecs + (int64_t)k * kThreads + tid;
      x[k] = load16_shifted(sw, sh, v < sp.vecs ? v : sp.vecs - 1);
    }
#pragma unroll
    for (int k = 0; k < kVecs; ++k) {
      const int64_t v = c * kChunkVecs + (int64_t)k * kThreads + tid;
      if (v < sp.vecs) dv[v] = x[k];
    }
  }
}

// shared argument rules of the frame entry points, on the frame's length
inline int frames_ok(const void* f0, const void* f1, int64_t img_stride, int32_t n, int64_t len) {
  if (!f0 || !f1) return RRIN_E_ARG;
  if (n < 1 || len < 1) return RRIN_E_SHAPE;
  if (img_stride < len) return RRIN_E_ARG;
  return RRIN_OK;
}

// the length of h0 x w0 x 3 frames; 0 (refused as a shape) unless both sizes are >= 1
inline int64_t rgb_len(int32_t h0, int32_t w0) { return h0 < 1 || w0 < 1 ? 0 : (int64_t)h0 * w0 * 3; }

// workgroups per frame: one per 32 KiB chunk of the body, at least 1 (head and tail), capped
inline int grid_x(int64_t len) {
  const int64_t chunks = (len / 16 + kChunkVecs - 1) / kChunkVecs;
  return (int)(chunks < 1 ? 1 : (chunks > kMaxGridX ? kMaxGridX : chunks));
}

}  // namespace
}  // namespace rrin

using namespace rrin;

extern "C" int rrin_pair_sad_u8(const uint8_t* f0, const uint8_t* f1, int64_t img_stride, int32_t n, int32_t h0,
                                int32_t w0, uint64_t* sad, void* stream) {
  return rrin_pair_sad_u8_len(f0, f1, img_stride, n, rgb_len(h0, w0), sad, stream);
}

extern "C" int rrin_pair_sad_u8_len(const uint8_t* f0, const uint8_t* f1, int64_t img_stride, int32_t n, int64_t len,
                                    uint64_t* sad, void* stream) {
  if (!sad || ((uintptr_t)sad & 7)) return RRIN_E_ARG;
  const int rc = frames_ok(f0, f1, img_stride, n, len);
  if (rc) return rc;
  if (n > 65535) return RRIN_E_SHAPE;  // one pair per blockIdx.y
  hipLaunchKernelGGL(zero_u64_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream,
                     sad, n);
  hipLaunchKernelGGL(pair_sad_u8_kernel, dim3(grid_x(len), n), dim3(kThreads), 0, (hipStream_t)stream, f0, f1,
                     img_stride, len, sad);
  return hip_code(hipGetLastError());
}

extern "C" int rrin_gate_from_sad_u8(const uint64_t* sad, int32_t n, uint64_t limit, int32_t cut_code,
                                     int32_t* gate, void* stream) {
  if (!sad || !gate || (cut_code != 1 && cut_code != 2)) return RRIN_E_ARG;
  if (n < 1) return RRIN_E_SHAPE;
  hipLaunchKernelGGL(gate_from_sad_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     (hipStream_t)stream, sad, n, limit, cut_code, gate);
  return hip_code(hipGetLastError());
}

extern "C" int rrin_gate_frames_u8(const uint8_t* f0, const uint8_t* f1, int64_t img_stride, int32_t n,
                                   int32_t h0, int32_t w0, const int32_t* gate, uint8_t* out, void* stream) {
  return rrin_gate_frames_u8_len(f0, f1, img_stride, n, rgb_len(h0, w0), gate, out, stream);
}

extern "C" int rrin_gate_frames_u8_len(const uint8_t* f0, const uint8_t* f1, int64_t img_stride, int32_t n,
                                       int64_t len, const int32_t* gate, uint8_t* out, void* stream) {
  if (!gate || !out) return RRIN_E_ARG;
  const int rc = frames_ok(f0, f1, img_stride, n, len);
  if (rc) return rc;
  if (n > 65535) return RRIN_E_SHAPE;  // one pair per blockIdx.y
  hipLaunchKernelGGL(gate_frames_u8_kernel<false>, dim3(grid_x(len), n), dim3(kThreads), 0, (hipStream_t)stream, f0,
                     f1, img_stride, len, gate, out, (const int32_t*)nullptr, n);
  return hip_code(hipGetLastError());
}

extern "C" int rrin_pair_sad_u16(const uint16_t* f0, const uint16_t* f1, int64_t img_stride, int32_t n, int32_t h0,
                                 int32_t w0, int32_t depth, int32_t shift, uint64_t* sad, void* stream) {
  return rrin_pair_sad_u16_len(f0, f1, img_stride, n, rgb_len(h0, w0), depth, shift, sad, stream);
}

extern "C" int rrin_pair_sad_u16_len(const uint16_t* f0, const uint16_t* f1, int64_t img_stride, int32_t n,
                                     int64_t len, int32_t depth, int32_t shift, uint64_t* sad, void* stream) {
  if (!sad || ((uintptr_t)sad & 7)) return RRIN_E_ARG;
  if (depth < 9 || depth > 16 || shift < 0 || shift > 16 - depth) return RRIN_E_ARG;
  if (((uintptr_t)f0 & 1) || ((uintptr_t)f1 & 1)) return RRIN_E_ARG;
  const int rc = frames_ok(f0, f1, img_stride, n, len);
  if (rc) return rc;
  if (n > 65535) return RRIN_E_SHAPE;  // one pair per blockIdx.y
  const int64_t steps = (len / 2 + kThreads * kWords - 1) / (kThreads * kWords);
  const int gx = (int)(steps < 1 ? 1 : (steps > kMaxGridX ? kMaxGridX : steps));
  hipLaunchKernelGGL(zero_u64_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream,
                     sad, n);
  hipLaunchKernelGGL(pair_sad_u16_kernel, dim3(gx, n), dim3(kThreads), 0, (hipStream_t)stream, f0, f1, img_stride,
                     len, shift, (1 << depth) - 1, sad);
  return hip_code(hipGetLastError());
}

extern "C" int rrin_gate_items_u8(const int32_t* pair_gate, int32_t n_pairs, const int32_t* pair_map,
                                  const int32_t* cut_codes, int32_t n, int32_t* gate, void* stream) {
  if (!pair_gate || !pair_map || !cut_codes || !gate) return RRIN_E_ARG;
  if (n_pairs < 1 || n_pairs > n) return RRIN_E_ARG;
  hipLaunchKernelGGL(gate_items_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream,
                     pair_gate, n_pairs, pair_map, cut_codes, n, gate);
  return hip_code(hipGetLastError());
}

extern "C" int rrin_gate_frames_items_u8_len(const uint8_t* f0, const uint8_t* f1, int64_t img_stride, int32_t n,
                                             int64_t len, const int32_t* gate, uint8_t* out, const int32_t* pair_map,
                                             int32_t n_pairs, void* stream) {
  if (!gate || !out || !pair_map) return RRIN_E_ARG;
  if (n_pairs < 1 || n_pairs > n) return RRIN_E_ARG;
  const int rc = frames_ok(f0, f1, img_stride, n, len);
  if (rc) return rc;
  if (n > 65535) return RRIN_E_SHAPE;  // one item per blockIdx.y
  hipLaunchKernelGGL(gate_frames_u8_kernel<true>, dim3(grid_x(len), n), dim3(kThreads), 0, (hipStream_t)stream, f0,
                     f1, img_stride, len, gate, out, pair_map, n_pairs);
  return hip_code(hipGetLastError());
}
