// The sub-pixel ring fold of the 8-wave Winograd tile (conv_winoq.hip, template parameter RF):
// the device code of the ring correction workgroups and of the hand-off between a correction
// workgroup and the conv tile that covers the same ring segment.  Included by conv_winoq.hip
// only; every function inlines into conv3x3_winoq_kernel.
//
// A sub-pixel up conv computes conv3x3(upsample_x2(x)) from phase weights over the
// edge-replicated low-res x; on the 1-pixel ring of the 2h x 2w output the true conv
// reads zero padding where the phase form read the clamped upsample, so the ring
// pixels take  y = (phase value - corr) + bias  with corr = sum over ci of the
// out-of-image taps w[c][ci][ky][kx] * up(ci, clamp(Y + ky - 1), clamp(X + kx - 1))
// (the arithmetic of edge_fix_h8_kernel, edge_fix.hip, which runs as a separate
// launch for the other configs).  Ring segment seg of (image, co block): top / bottom
// row under tile column tx (seg tx / tiles_x + tx: X in [64 tx, 64 tx + 64)), left /
// right column beside tile row ty (2 tiles_x + ty / 2 tiles_x + tiles_y + ty:
// Y in [16 ty, 16 ty + 16) within [1, H - 2]); 8 real channels (the co block).
#pragma once
#include "common.hpp"

namespace rrin {

struct RingSeg {
  int line, idx, np;  // line 0 top 1 bottom 2 left 3 right; tile column / row; pixels (64 / 16)
  int Y0, X0;         // first pixel
  int lo, hi;         // valid pixel positions [lo, hi) along the line
};
__device__ inline RingSeg ring_seg(const ConvH8Args& a, int seg) {
  RingSeg r;
  const int H = 2 * a.h, W = 2 * a.w;
  if (seg < 2 * a.tiles_x) {
    r.line = seg < a.tiles_x ? 0 : 1;
    r.idx = seg - r.line * a.tiles_x;
    r.np = 64;
    r.X0 = 64 * r.idx;
    r.Y0 = r.line == 0 ? 0 : H - 1;
    r.lo = 0;
    r.hi = min(64, W - r.X0);
  } else {
    const int t = seg - 2 * a.tiles_x;
    r.line = t < a.tiles_y ? 2 : 3;
    r.idx = t - (r.line - 2) * a.tiles_y;
    r.np = 16;
    r.Y0 = 16 * r.idx;
    r.X0 = r.line == 2 ? 0 : W - 1;
    r.lo = max(0, 1 - r.Y0);
    r.hi = max(r.lo, min(16, H - 1 - r.Y0));
  }
  return r;
}
// bilinear x2 upsample (align_corners = False, edge clamp) of channel ci of image img
// at output pixel (Y, X), in upsample_bilinear2d's order (edge_fix_h8_kernel's Up8)
__device__ inline float ring_up(const ConvH8Args& a, int img, int ci, int Y, int X) {
  int ra, rb, ca, cb;
  float wa, wc;
  if (Y & 1) { ra = Y >> 1; rb = min(ra + 1, a.h - 1); wa = 0.75f; }
  else { rb = Y >> 1; ra = max(rb - 1, 0); wa = 0.25f; }
  if (X & 1) { ca = X >> 1; cb = min(ca + 1, a.w - 1); wc = 0.75f; }
  else { cb = X >> 1; ca = max(cb - 1, 0); wc = 0.25f; }
  const float* src = reinterpret_cast<const float*>(a.src_hi + (int64_t)img * a.src_img + (int64_t)(ci >> 2) * a.src_gp +
                                                    kH8PadLeft) + (ci & 3);
  const float v0 = src[((int64_t)(ra + 1) * a.src_wp + ca) * 4], v1 = src[((int64_t)(ra + 1) * a.src_wp + cb) * 4];
  const float v2 = src[((int64_t)(rb + 1) * a.src_wp + ca) * 4], v3 = src[((int64_t)(rb + 1) * a.src_wp + cb) * 4];
  const float wb = 1.0f - wa, wd = 1.0f - wc;
  const float top = wc * v0 + wd * v1;
  const float bot = wc * v2 + wd * v3;
  return wa * top + wb * bot;
}
// segment (img, cob, seg) done by both of its writers: the later one writes its ring
// pixels, (phase value - corr) + bias, from the edge and corr scratch (after the
// caller's agent-scope acquire)
__device__ inline void ring_combine(const ConvH8Args& a, int img, int cob, int seg, int tid) {
  const RingSeg r = ring_seg(a, seg);
  const int p = tid & (r.np - 1), c = tid / r.np;
  if (c >= 8 || p < r.lo || p >= r.hi) return;
  const int H = 2 * a.h, W = 2 * a.w, creal = a.cout >> 2;
  const int Y = r.line < 2 ? r.Y0 : r.Y0 + p, X = r.line < 2 ? r.X0 + p : r.X0;
  const int ch = cob * 8 + c;
  // sc1 loads (write-through stores of other workgroups, possibly on other XCDs)
  const auto er = __builtin_amdgcn_make_buffer_rsrc(a.edge, 0, 0x7fffffff, 0x00020000);
  const float e = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
      er, (int)((((int64_t)img * creal + ch) * a.ring + ring_index(Y, X, H, W)) * 4), 0, 16));
  float* slab = a.corr + ((int64_t)(img * a.co_blocks + cob) * a.nseg + seg) * 512;
  const auto cr = __builtin_amdgcn_make_buffer_rsrc(slab, 0, 512 * 4, 0x00020000);
  const float corr = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(cr, (c * r.np + p) * 4, 0, 16));
  float* dst = reinterpret_cast<float*>(a.dst_hi);
  dst[(((int64_t)img * a.dst_img + (int64_t)(ch >> 2) * a.dst_gp + (int64_t)(Y + 1) * a.dst_wp + X + kH8PadLeft) << 2) +
      (ch & 3)] = (e - corr) + a.bias_raw[ch];
}
// one ticket of segment (img, cob, seg) by lane 0 (after every wave drained its
// write-through stores and the barrier); returns on every thread whether this
// workgroup was the segment's second writer (then after an agent-scope acquire)
__device__ inline bool ring_ticket(const ConvH8Args& a, int img, int cob, int seg, int tid, int* s_flag) {
  if (tid == 0) {
    int* cnt = a.rcnt + (img * a.co_blocks + cob) * a.nseg + seg;
    const int last = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 1;
    if (last) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // next launch
    *s_flag = last;
  }
  __syncthreads();
  const bool last = *s_flag != 0;
  __syncthreads();  // s_flag reusable
  // every load of the handed-off values is an sc1 load (ring_combine): no agent-scope
  // acquire (it would drop this CU's cached lines), only the compiler-ordering fence
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return last;
}
// correction workgroup rb (< n * co_blocks * nseg; 512 threads): corr of its segment,
// 64 input channels per LDS stage (the segment's upsampled line +-1 and the two corner
// values, the 9 taps x 8 channels of weights: 36 KB), so a stage is one round of loads
__device__ inline void ring_block(const ConvH8Args& a, int rb, float* sm) {
  const int tid = threadIdx.x;
  const int seg = rb % a.nseg, t = rb / a.nseg, cob = t % a.co_blocks, img = t / a.co_blocks;
  const RingSeg r = ring_seg(a, seg);
  if (r.lo >= r.hi) return;  // an empty column segment (its conv tile does not count it either)
  const int H = 2 * a.h, W = 2 * a.w, creal = a.cout >> 2;
  const bool row = r.line < 2;
  const int nl = r.np + 2;           // staged line: positions -1 .. np
  constexpr int RC = 64;             // input channels per LDS stage (one load round per stage)
  float* s_l = sm;                   // [RC][nl]
  float* s_e = sm + RC * 66;         // [RC][2] corner extras (row lines)
  float* s_w = s_e + RC * 2;         // [RC ci][9 taps][8 c]
  const int p = tid & (r.np - 1), c = tid / r.np;
  const bool act = c < 8 && p >= r.lo && p < r.hi;
  const int X = row ? r.X0 + p : r.X0;
  // extras: the second row in (top: 1, bottom: H - 2) at the corner columns
  const int Ye = r.line == 0 ? min(1, H - 1) : max(H - 2, 0);
  float acc = 0.f;
  for (int c0 = 0; c0 < a.cin; c0 += RC) {
    const int nc = min(RC, a.cin - c0);
    for (int i = tid; i < nc * nl; i += 512) {
      const int ci = i / nl, j = i - ci * nl;
      const int Yv = row ? r.Y0 : min(max(r.Y0 - 1 + j, 0), H - 1);
      const int Xv = row ? min(max(r.X0 - 1 + j, 0), W - 1) : r.X0;
      s_l[ci * nl + j] = ring_up(a, img, c0 + ci, Yv, Xv);
    }
    if (row && tid < 2 * nc) s_e[tid] = ring_up(a, img, c0 + (tid >> 1), Ye, (tid & 1) ? W - 1 : 0);
    for (int i = tid; i < nc * 72; i += 512) {
      const int ci = i / 72, tap = (i / 8) % 9, cc = i & 7;
      s_w[i] = cob * 8 + cc < creal ? a.wedge[((int64_t)(c0 + ci) * 9 + tap) * creal + cob * 8 + cc] : 0.f;
    }
    __syncthreads();
    if (act) {
      for (int ci = 0; ci < nc; ++ci) {
        const float* l = s_l + ci * nl;
        const float* w = s_w + ci * 72 + c;
        if (r.line == 0 || r.line == 1) {  // the outside kernel row ky (0 top, 2 bottom), then the corners
          const int ky = r.line == 0 ? 0 : 2;
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) acc = fmaf(w[(ky * 3 + kx) * 8], l[p + kx], acc);
          if (X == 0) {
            acc = fmaf(w[((r.line == 0 ? 1 : 0) * 3) * 8], r.line == 0 ? l[p] : s_e[ci * 2], acc);
            acc = fmaf(w[((r.line == 0 ? 2 : 1) * 3) * 8], r.line == 0 ? s_e[ci * 2] : l[p], acc);
          }
          if (X == W - 1) {
            acc = fmaf(w[((r.line == 0 ? 1 : 0) * 3 + 2) * 8], r.line == 0 ? l[p + 2] : s_e[ci * 2 + 1], acc);
            acc = fmaf(w[((r.line == 0 ? 2 : 1) * 3 + 2) * 8], r.line == 0 ? s_e[ci * 2 + 1] : l[p + 2], acc);
          }
        } else {  // the outside kernel column kx (0 left, 2 right)
          const int kx = r.line == 2 ? 0 : 2;
#pragma unroll
          for (int ky = 0; ky < 3; ++ky) acc = fmaf(w[(ky * 3 + kx) * 8], l[p + ky], acc);
        }
      }
    }
    __syncthreads();
  }
  if (act) {
    float* slab = a.corr + ((int64_t)(img * a.co_blocks + cob) * a.nseg + seg) * 512;
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(slab, 0, 512 * 4, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc), rsrc, (c * r.np + p) * 4, 0, 16 /* sc1 */);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (ring_ticket(a, img, cob, seg, tid, reinterpret_cast<int*>(sm + 9216))) ring_combine(a, img, cob, seg, tid);
}

}  // namespace rrin
