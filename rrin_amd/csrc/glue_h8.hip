// Every non-conv kernel of the record path (layouts in h8.hpp), each with its entry point:
// NCHW <-> records (rrin_nchw_to_h8 / rrin_h8_to_nchw), the frame pair into the Net buffer g16
// from fp32, uint8 or uint16 frames (rrin_pack_g16_h8 / rrin_pack_g16_u8_h8 / rrin_pack_g16_u16_h8), nn.Upsample(bilinear, x2)
// (unet.py:77) as its own pass (rrin_upsample2x_h8), the head convs (Cout <= 4) fused with the
// model.py glue they feed (rrin_head_h8_fwd; the arithmetic itself in net_glue.hpp; the FINAL
// head also stores 8-bit and 16-bit frames, interleaved RGB or 4:2:0 planes through yuv.hpp), and the
// t-blend of a kept raw flow (rrin_flow_tblend_h8).  Each kernel is written once over a record
// format F (rec_fmt.hpp) and instantiated for RecH8<1> (F16), RecH8<2> (F16X3) and RecR32.
#include <string.h>

#include "net_glue.hpp"
#include "rec_fmt.hpp"
#include "yuv.hpp"

namespace rrin {

// ---- bilinear x2 upsample pass (unet.py:77, align_corners=False) -------------
template <class F>
__global__ void up2x_kernel(RecView s, int sh, int sw, RecView d, int groups, int64_t total) {
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
  const int64_t rr[4] = {s.rec(img, g, ra, ca), s.rec(img, g, ra, cb), s.rec(img, g, rb, ca), s.rec(img, g, rb, cb)};
  float v[4][F::kChans];
#pragma unroll
  for (int k = 0; k < 4; ++k) F::load_rec(s, rr[k], v[k]);
  float o[F::kChans];
#pragma unroll
  for (int e = 0; e < F::kChans; ++e) {
    // horizontal first, then vertical (upsample_bilinear2d order)
    const float top = wc * v[0][e] + wd * v[1][e];
    const float bot = wc * v[2][e] + wd * v[3][e];
    o[e] = wa * top + wb * bot;
  }
  F::store_rec(d, d.rec(img, g, y, x), o);
}

// ---- layout kernels ------------------------------------------------------------
template <class F>
__global__ void nchw_to_rec_kernel(const float* __restrict__ src, RecView d, int ch_off, int c, int h, int w,
                                   int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w);
  int64_t t = i / w;
  const int y = (int)(t % h);
  t /= h;
  const int ch = (int)(t % c);
  const int n = (int)(t / c);
  F::store_elem(d, n, ch_off + ch, y, x, src[i]);
}

template <class F>
__global__ void rec_to_nchw_kernel(RecView s, int ch_off, float* dst, int c, int h, int w, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w);
  int64_t t = i / w;
  const int y = (int)(t % h);
  t /= h;
  const int ch = (int)(t % c);
  const int n = (int)(t / c);
  dst[i] = F::load_elem(s, n, ch_off + ch, y, x);
}

// zero channels [c0, c0 + c) of every interior pixel of a view; rrin_unet_fwd clears the
// channels its PLAIN head writes past in_ch so that the next call's first conv never stages them
template <class F>
__global__ void clear_channels_kernel(RecView v, int c0, int c, int h, int w, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w);
  int64_t t = i / w;
  const int y = (int)(t % h);
  t /= h;
  const int ch = c0 + (int)(t % c);
  const int n = (int)(t / c);
  F::store_elem(v, n, ch, y, x, 0.f);
}

// x = cat(x0, x1) (model.py:33) of one pixel into g16: channels 0-2 = a, 3-5 = b, 6-15 zero, as
// whole records (H8: 2 per plane, R32: 4)
template <class F>
__device__ inline void store_frame_pair(const RecView& g, int64_t rec, const float* a, const float* b) {
  const float v[16] = {a[0], a[1], a[2], b[0], b[1], b[2]};
#pragma unroll
  for (int k = 0; k < 16 / F::kChans; ++k) F::store_rec(g, rec + k * g.gp, v + k * F::kChans);
}

template <class F>
__global__ void pack_g16_kernel(const float* __restrict__ i0, const float* __restrict__ i1, RecView g, int h, int w,
                                int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w);
  const int64_t t = i / w;
  const int y = (int)(t % h);
  const int img = (int)(t / h);
  const int64_t hw = (int64_t)h * w;
  const int64_t px = (int64_t)img * 3 * hw + (int64_t)y * w + x;
  float a[3], b[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a[c] = i0[px + c * hw];
    b[c] = i1[px + c * hw];
  }
  store_frame_pair<F>(g, g.rec(img, 0, y, x), a, b);
}

// ---- 8-bit frames straight into g16 (rrin_pack_g16_u8_h8) --------------------------
__constant__ const U8ScaleTab kU8Scale{};

// x = cat(x0, x1) from two uint8 [n][h0][w0][3] frame stacks, edge-replicated on top (`top` rows)
// and on the right to the h x w of g16: padded pixel (y, x) reads source pixel
// (max(y - top, 0), min(x, w0 - 1)).  One workgroup per row and run of 256 pixels: the run's
// 768 source bytes of each frame are loaded one byte per lane (a wave's load is 64 consecutive
// bytes, whatever the alignment of the row) into LDS, then every lane converts its pixel through
// the LDS copy of the scale table and writes the whole records pack_g16_kernel writes.
// ITEMS (ABI 25): image img of g16 reads frame pair_of(map, img, n_pairs) of both stacks -- f1 is f0
// one frame on, so that is pair map[img] of one [n_pairs + 1] stack.  Without it map / n_pairs are
// unused and the kernel is, instruction for instruction, the one it was before they existed.
template <class F, bool ITEMS = false>
__global__ void __launch_bounds__(256) pack_g16_u8_kernel(const uint8_t* __restrict__ f0,
                                                          const uint8_t* __restrict__ f1, int64_t f_img, int w0,
                                                          int top, RecView g, int w,
                                                          const int32_t* __restrict__ map, int n_pairs) {
  __shared__ float s_tab[256];
  __shared__ uint8_t s_px[2][768];
  const int tid = threadIdx.x;
  const int xs = blockIdx.x * 256, y = blockIdx.y, img = blockIdx.z;
  s_tab[tid] = kU8Scale.v[tid];
  const int sy = y > top ? y - top : 0;
  const int src = ITEMS ? pair_of(map, img, n_pairs) : img;
  const int64_t row = (int64_t)src * f_img + ((int64_t)sy * w0 + xs) * 3;
  // xs < w0: w is w0 rounded up to a multiple m of 16, 32 or 64 (16 * flow_scale), so the right pad is
  // < m columns; xs < w is a multiple of 256, hence of m: xs <= w - m < w0
  const int nb = min(256, w0 - xs) * 3;
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
  store_frame_pair<F>(g, g.rec(img, 0, y, x), a, b);
}

// ---- 16-bit frames straight into g16 (rrin_pack_g16_u16_h8) ------------------------
// pack_g16_u8_kernel for uint16 [n][h0][w0][3] frames of maxval = 2^depth - 1: the run's 768
// words of each frame are loaded one per lane and step (2-byte loads: a frame of a stack starts
// at any even address; a wave's load is 128 consecutive bytes) into LDS; a pixel's samples are
// min(word, maxval) and its values sample / maxval by the IEEE division (sample_to_float): no
// table, which at 16 bits would not fit the LDS.  f_img counts words.
// ITEMS: as pack_g16_u8_kernel
template <class F, bool ITEMS = false>
__global__ void __launch_bounds__(256) pack_g16_u16_kernel(const uint16_t* __restrict__ f0,
                                                           const uint16_t* __restrict__ f1, int64_t f_img, int w0,
                                                           int top, RecView g, int w, int maxval,
                                                           const int32_t* __restrict__ map, int n_pairs) {
  __shared__ uint16_t s_px[2][768];
  const int tid = threadIdx.x;
  const int xs = blockIdx.x * 256, y = blockIdx.y, img = blockIdx.z;
  const int sy = y > top ? y - top : 0;
  const int src = ITEMS ? pair_of(map, img, n_pairs) : img;
  const int64_t row = (int64_t)src * f_img + ((int64_t)sy * w0 + xs) * 3;
  // xs < w0: w is w0 rounded up to a multiple m of 16, 32 or 64 (16 * flow_scale), so the right pad is
  // < m columns; xs < w is a multiple of 256, hence of m: xs <= w - m < w0
  const int nb = min(256, w0 - xs) * 3;
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
  const float mv = (float)maxval;
  float a[3], b[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a[k] = sample_to_float(min((int)s_px[0][c + k], maxval), mv);
    b[k] = sample_to_float(min((int)s_px[1][c + k], maxval), mv);
  }
  store_frame_pair<F>(g, g.rec(img, 0, y, x), a, b);
}

// ---- head conv (Cout <= 4) + Net glue on the record Net buffer ------------------
struct HeadH8Args {
  RecView src;      // 32 channels
  RecView g;        // g16
  RecView fr;       // FLOW: raw output (channels 0-3), hi nullable
  const float* w;
  const float* bias;
  const float* coef;
  float* out;
  int h, w_, tiles_x, tiles_y;
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
  // FINAL, the WIDE kernels only (rrin_head_h8_desc.out_u16 / out_yuv16): out8 or oy / ou / ov hold
  // uint16 pointers, o_img and the pitches count words; samples of [0, maxval], stored << shift
  int maxval, shift;
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

// FINAL with a 16-bit output: final_store_u8 with three interleaved words, each
// (uint16)(q * (float)maxval) -- one fp32 multiply, truncation, as frames_float_to_u16; 0 when poisoned
__device__ inline int final_word(float q, bool poison, float maxval) { return poison ? 0 : (int)(q * maxval); }

__device__ inline void final_store_u16(const HeadH8Args& a, int img, int y, int x, const float* q, bool poison) {
  const int yo = y - a.top;
  if (yo < 0 || yo >= a.h0 || x >= a.w0) return;
  uint16_t* o = reinterpret_cast<uint16_t*>(a.out8) + (((int64_t)img * a.h0 + yo) * a.w0 + x) * 3;
  const float mv = (float)a.maxval;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) o[ch] = (uint16_t)final_word(q[ch], poison, mv);
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

// final_store_yuv for 16-bit planes (rgb: the two pixels' samples of [0, maxval]): the same lane
// exchange and store pattern, the conversion at the planes' depth, every sample stored << shift
__device__ inline void final_store_yuv16(const HeadH8Args& a, int img, int y, int x, const int (*rgb)[3]) {
  int sum[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    sum[ch] = rgb[0][ch] + rgb[1][ch];
    sum[ch] += __shfl_xor(sum[ch], 1);
  }
  const int yo = y - a.top;
  if (yo < 0 || yo >= a.h0 || x >= a.w0) return;
  const int mid = (a.maxval + 1) >> 1;
  const int64_t base = (int64_t)img * a.o_img;
  uint16_t* py = reinterpret_cast<uint16_t*>(a.oy) + base + (int64_t)yo * a.oy_pitch + x;
  py[0] = (uint16_t)(rgb_to_luma16(a.yc, a.maxval, rgb[0]) << a.shift);
  py[a.oy_pitch] = (uint16_t)(rgb_to_luma16(a.yc, a.maxval, rgb[1]) << a.shift);
  const int64_t c = base + (int64_t)(yo >> 1) * a.oc_pitch + (x >> 1) * a.oc_step;
  if (x & 1)
    reinterpret_cast<uint16_t*>(a.ov)[c] =
        (uint16_t)(rgb_sum_to_chroma16(a.yc.vr, a.yc.vg, a.yc.vb, mid, a.maxval, sum) << a.shift);
  else
    reinterpret_cast<uint16_t*>(a.ou)[c] =
        (uint16_t)(rgb_sum_to_chroma16(a.yc.ur, a.yc.ug, a.yc.ub, mid, a.maxval, sum) << a.shift);
}

// FINAL with a 4:2:2 (CH = RRIN_CHROMA_422) or 4:4:4 output, 8-bit planes (WIDE false) or 16-bit
// words (rules of final_store_yuv16).  4:2:2: a thread's pixel of row y + p and that of its xl ^ 1
// lane are one 2x1 block (w0 is even), so each row has its own sums; the even lane writes U of
// both its rows and the odd lane V.  4:4:4: a block is a pixel, no lane exchange.  As in
// final_store_yuv every lane of the wave reaches the exchange before any return.  h0 and top may
// be odd, so each of the two rows is guarded on its own: yo may be -1 with row yo + 1 in the crop.
template <int CH, bool WIDE>
__device__ inline void final_store_yuv4xx(const HeadH8Args& a, int img, int y, int x, const int (*rgb)[3]) {
  constexpr int LOG2P = CH == RRIN_CHROMA_422 ? 1 : 0;
  int sum[2][3];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      sum[p][ch] = rgb[p][ch];
      if constexpr (CH == RRIN_CHROMA_422) sum[p][ch] += __shfl_xor(sum[p][ch], 1);
    }
  if (x >= a.w0) return;
  const int mid = (a.maxval + 1) >> 1;
  const int64_t base = (int64_t)img * a.o_img;
  const int cx = CH == RRIN_CHROMA_422 ? x >> 1 : x;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int yo = y + p - a.top;
    if (yo < 0 || yo >= a.h0) continue;
    const int64_t l = base + (int64_t)yo * a.oy_pitch + x;
    const int64_t c = base + (int64_t)yo * a.oc_pitch + (int64_t)cx * a.oc_step;
    const bool put_u = CH == RRIN_CHROMA_444 || !(x & 1), put_v = CH == RRIN_CHROMA_444 || (x & 1);
    if constexpr (WIDE) {
      reinterpret_cast<uint16_t*>(a.oy)[l] = (uint16_t)(rgb_to_luma16(a.yc, a.maxval, rgb[p]) << a.shift);
      if (put_u)
        reinterpret_cast<uint16_t*>(a.ou)[c] =
            (uint16_t)(rgb_block_to_chroma16<LOG2P>(a.yc.ur, a.yc.ug, a.yc.ub, mid, a.maxval, sum[p]) << a.shift);
      if (put_v)
        reinterpret_cast<uint16_t*>(a.ov)[c] =
            (uint16_t)(rgb_block_to_chroma16<LOG2P>(a.yc.vr, a.yc.vg, a.yc.vb, mid, a.maxval, sum[p]) << a.shift);
    } else {
      a.oy[l] = (uint8_t)rgb_to_luma(a.yc, rgb[p]);
      if (put_u) a.ou[c] = (uint8_t)rgb_block_to_chroma<LOG2P>(a.yc.ur, a.yc.ug, a.yc.ub, sum[p]);
      if (put_v) a.ov[c] = (uint8_t)rgb_block_to_chroma<LOG2P>(a.yc.vr, a.yc.vg, a.yc.vb, sum[p]);
    }
  }
}

// The glue stores whole or partial records as the format does (F::Px): RecR32 updates g16 only in
// whole 16-B records and reads first those it changes in part (FLOW records 1-2, REFINE 1-3,
// MASK 1-2); RecH8 stores 2 / 4 / 16 B per plane and sets the range flag.
// YUV (FINAL only): the 8-bit output as 4:2:0 planes (final_store_yuv) instead of interleaved RGB
// WIDE (FINAL only): the frame output in 16-bit words (final_store_u16; with YUV final_store_yuv16).
// CH (with YUV): the chroma block of the planes, rrin_chroma (4:2:2 / 4:4:4: final_store_yuv4xx).
// All are compile-time forms: the fp32 / 8-bit / 4:2:0 instantiations carry none of the other code.
template <class F, int COUT, int MODE, bool YUV = false, bool WIDE = false, int CH = RRIN_CHROMA_420>
__global__ void __launch_bounds__(256) head_kernel(HeadH8Args a) {
  // tile 16 rows x 32 cols; thread = 2 vertically adjacent pixels (one float2v per output channel;
  // the library is built without packed fp32 ops, so the FMA is two v_fma_f32)
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
  // records of rows y0-1..y0+16, cols x0-1..x0+32 of one channel octet, fetched
  // one octet ahead into registers, then converted to fp32 planar LDS
  constexpr int kRec = HROWS * H8_LC, kIt = (kRec + 255) / 256;
  uint4 pre[kIt][F::kRecs8];
  auto fetch = [&](int g8) {
#pragma unroll
    for (int it = 0; it < kIt; ++it) {
      const int idx = tid + 256 * it;
      if (idx < kRec) {
        const int rr = idx / H8_LC, col = idx - rr * H8_LC;
        F::fetch8(a.src, a.src.rec(img, g8 * (8 / F::kChans), y0 + rr - 1, x0 - 1 + col), pre[it]);
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
        float v[8];
        F::decode8(pre[it], v);
#pragma unroll
        for (int e = 0; e < 8; ++e) s_in[(e * HROWS + rr) * HLC + col + 3] = v[e];
      }
    }
    __syncthreads();
    if (g8 + 1 < CIN / 8) fetch(g8 + 1);
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
            const float w = a.w[((co * CIN) + g8 * 8 + ci) * 9 + ky * 3 + kx];
            acc2[co] = __builtin_elementwise_fma(float2v{w, w}, v, acc2[co]);
          }
        }
    }
    __syncthreads();
  }

  int rgb[2][3] = {};  // YUV: the two pixels' RGB bytes (WIDE: samples)
  for (int p = 0; p < 2; ++p) {
    float acc[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) acc[co] = acc2[co][p];
    const int y = y0 + r2 + p, x = x0 + xl;
    if (y >= a.h || x >= a.w_) continue;
    typename F::Px px{a.g, a.g.rec(img, 0, y, x), a.status};  // Net buffer channels 0-15 of this pixel
    const float* cf = a.coef + img * 8;
    if (a.raw)
#pragma unroll
      for (int co = 0; co < COUT; ++co) a.raw[(((int64_t)img * COUT + co) * a.h + y) * a.w_ + x] = acc[co];

    if constexpr (MODE == RRIN_HEAD_PLAIN) {
      for (int co = 0; co < COUT; ++co) F::store_elem(a.g, img, co, y, x, acc[co]);
    } else if constexpr (MODE == RRIN_HEAD_FLOW) {
#pragma clang fp contract(off)
      // round the raw flow to its stored form first, so that a later t-blend of the
      // kept raw flow (skip_flow) reproduces these Ft bit for bit
      for (int k = 0; k < 4; ++k) F::check_range(a.status, acc[k]);
      if (a.fr.hi) {
        typename F::Px fr{a.fr, a.fr.rec(img, 0, y, x), nullptr};
        fr.template store<0, 4>(acc);
      }
      for (int k = 0; k < 4; ++k) acc[k] = F::round_stored(acc[k]);
      float f0[2], f1[2];
      flow_blend(cf, acc, f0, f1);
      px.template fetch<0, 0, 6, 10>();
      px.template store<6, 8>(f0);
      px.template store<8, 10>(f1);
    } else if constexpr (MODE == RRIN_HEAD_REFINE) {
#pragma clang fp contract(off)
      px.template fetch<6, 10, 6, 16>();
      const float f0[2] = {px.c[6] + acc[0], px.c[7] + acc[1]};
      float o1[8];
      o1[0] = px.c[8] + acc[2];
      o1[1] = px.c[9] + acc[3];
      const WarpTaps t0 = warp_taps(x, y, f0[0], f0[1], a.h, a.w_);
      const WarpTaps t1 = warp_taps(x, y, o1[0], o1[1], a.h, a.w_);
      // backwarp x0 (ch 0-2) with Ft0 and x1 (ch 3-5) with Ft1: channels 0-7 of each tap
      auto tap8 = [&](int ty, int tx, float* v) { F::load8(a.g, a.g.rec(img, 0, ty, tx), v); };
      warp3(t0, 0, tap8, o1 + 2);
      warp3(t1, 3, tap8, o1 + 5);
      px.template store<6, 8>(f0);
      px.template store<8, 16>(o1);
    } else if constexpr (MODE == RRIN_HEAD_MASK) {
#pragma clang fp contract(off)
      px.template fetch<10, 16, 6, 9>();
      float o[3];
      mask_blend(cf, acc[0], acc[1], px.c + 10, px.c + 13, o);
      px.template store<6, 9>(o);
    } else {  // FINAL
#pragma clang fp contract(off)
      px.template fetch<6, 9, 0, 0>();
      const float base[3] = {px.c[6], px.c[7], px.c[8]};
      const bool poison = F::kFlag && a.status && *a.status != 0;  // an fp16 overflow upstream (range guard)
      float q[3];
      final_clamp(acc, base, q);
      if (a.out) {
        float* o = a.out + ((int64_t)img * 3) * a.h * a.w_ + (int64_t)y * a.w_ + x;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[(int64_t)ch * a.h * a.w_] = poison ? __builtin_nanf("") : q[ch];
      }
      if constexpr (YUV && WIDE) {
        const float mv = (float)a.maxval;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) rgb[p][ch] = final_word(q[ch], poison, mv);
      } else if constexpr (WIDE) {
        final_store_u16(a, img, y, x, q, poison);
      } else if constexpr (YUV) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) rgb[p][ch] = final_byte(q[ch], poison);
      } else if (a.out8) {
        final_store_u8(a, img, y, x, q, poison);
      }
    }
  }
  if constexpr (YUV && CH != RRIN_CHROMA_420)
    final_store_yuv4xx<CH, WIDE>(a, img, y0 + r2, x0 + xl, rgb);
  else if constexpr (YUV && WIDE)
    final_store_yuv16(a, img, y0 + r2, x0 + xl, rgb);
  else if constexpr (YUV)
    final_store_yuv(a, img, y0 + r2, x0 + xl, rgb);
}

// Ft0 / Ft1 (model.py:38-39) from a kept raw Flow record -> g16 channels 6-9.  ITEMS (ABI 25): item
// img blends the kept raw Flow of pair pair_of(map, img, n_pairs) with its own coefficients
template <class F, bool ITEMS = false>
__global__ void flow_tblend_kernel(RecView fr, RecView g, const float* coef, int h, int w, int64_t total,
                                   const int32_t* __restrict__ map, int n_pairs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w);
  const int64_t t = i / w;
  const int y = (int)(t % h);
  const int img = (int)(t / h);
  const float* cf = coef + img * 8;
  float f[F::kChans];
  const int src = ITEMS ? pair_of(map, img, n_pairs) : img;
  F::load_rec(fr, fr.rec(src, 0, y, x), f);
  float o[4];
  flow_blend(cf, f, o, o + 2);
  typename F::Px px{g, g.rec(img, 0, y, x), nullptr};
  px.template fetch<0, 0, 6, 10>();
  px.template store<6, 8>(o);
  px.template store<8, 10>(o + 2);
}

// ---- host side (with_format, rec_view: rec_fmt.hpp) ---------------------------------
int clear_channels_h8(const rrin_h8* v, int32_t n, int32_t c0, int32_t c1, int32_t prec, hipStream_t st) {
  if (!v || n < 1 || c0 < 0 || c1 <= c0 || !rec_prec(prec) || c1 > chans_per_rec(prec) * v->groups) return RRIN_E_ARG;
  const int64_t total = (int64_t)n * (c1 - c0) * v->g.h * v->g.w;
  const int grid = (int)((total + 255) / 256);
  return with_format(prec, [&](auto f) {
    hipLaunchKernelGGL(clear_channels_kernel<decltype(f)>, dim3(grid), dim3(256), 0, st, rec_view(*v), c0, c1 - c0,
                       v->g.h, v->g.w, total);
    return hip_code(hipGetLastError());
  });
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
  return with_format(prec, [&](auto f) {
    hipLaunchKernelGGL(up2x_kernel<decltype(f)>, dim3(grid), dim3(256), 0, (hipStream_t)stream, rec_view(*src),
                       src->g.h, src->g.w, rec_view(*dst), src->groups, total);
    return hip_code(hipGetLastError());
  });
}

extern "C" int rrin_nchw_to_h8(const float* src, int32_t n, int32_t c, int32_t ch_off, const rrin_h8* dst,
                               int32_t prec, void* stream) {
  if (!src || !dst || n < 1 || c < 1 || ch_off < 0 || !rec_prec(prec)) return RRIN_E_ARG;
  if (ch_off + c > chans_per_rec(prec) * dst->groups) return RRIN_E_ARG;
  if (!h8_ok(*dst, prec)) return RRIN_E_SHAPE;
  const int64_t total = (int64_t)n * c * dst->g.h * dst->g.w;
  const int grid = (int)((total + 255) / 256);
  return with_format(prec, [&](auto f) {
    hipLaunchKernelGGL(nchw_to_rec_kernel<decltype(f)>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src,
                       rec_view(*dst), ch_off, c, dst->g.h, dst->g.w, total);
    return hip_code(hipGetLastError());
  });
}

extern "C" int rrin_h8_to_nchw(const rrin_h8* src, int32_t n, int32_t c, int32_t ch_off, float* dst, int32_t prec,
                               void* stream) {
  if (!src || !dst || n < 1 || c < 1 || ch_off < 0 || !rec_prec(prec)) return RRIN_E_ARG;
  if (ch_off + c > chans_per_rec(prec) * src->groups) return RRIN_E_ARG;
  if (!h8_ok(*src, prec)) return RRIN_E_SHAPE;
  const int64_t total = (int64_t)n * c * src->g.h * src->g.w;
  const int grid = (int)((total + 255) / 256);
  return with_format(prec, [&](auto f) {
    hipLaunchKernelGGL(rec_to_nchw_kernel<decltype(f)>, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                       rec_view(*src), ch_off, dst, c, src->g.h, src->g.w, total);
    return hip_code(hipGetLastError());
  });
}

template <int COUT, int MODE, bool YUV = false, bool WIDE = false, int CH = RRIN_CHROMA_420>
static int head_launch(const HeadH8Args& a, int prec, int grid, hipStream_t st) {
  return with_format(prec, [&](auto f) {
    hipLaunchKernelGGL((head_kernel<decltype(f), COUT, MODE, YUV, WIDE, CH>), dim3(grid), dim3(256), 0, st, a);
    return hip_code(hipGetLastError());
  });
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
  const bool fin = d->mode == RRIN_HEAD_FINAL;
  const bool yuv = fin && d->out_yuv.y;
  const bool u16 = fin && d->out_u16, yuv16 = fin && d->out_yuv16.y;
  if (fin && !d->out && !d->out_u8 && !yuv && !u16 && !yuv16) return RRIN_E_ARG;
  if ((d->out_u8 != nullptr) + yuv + u16 + yuv16 > 1) return RRIN_E_ARG;
  if (u16 && (d->u16_depth < 9 || d->u16_depth > 16)) return RRIN_E_ARG;
  if (fin && (d->out_u8 || yuv || u16 || yuv16) &&
      (d->h0 < 1 || d->w0 < 1 || d->top < 0 || d->top + d->h0 > h || d->w0 > w))
    return RRIN_E_SHAPE;
  if (yuv) {
    if (int rc = yuv_coef_check(&d->yuv_coef)) return rc;
    if (int rc = yuv420_check(d->out_yuv, d->n, d->h0, d->w0)) return rc;
    if (d->out_yuv.chroma == RRIN_CHROMA_420 && (d->top & 1)) return RRIN_E_SHAPE;
  }
  if (yuv16) {
    if (int rc = yuv420_16_check(d->out_yuv16, d->n, d->h0, d->w0)) return rc;
    if (int rc = yuv_coef_check16(&d->yuv_coef, d->out_yuv16.depth)) return rc;
    if (d->out_yuv16.chroma == RRIN_CHROMA_420 && (d->top & 1)) return RRIN_E_SHAPE;
  }
  memset(&a, 0, sizeof(a));
  a.src = rec_view(d->src);
  a.g = rec_view(d->g16);
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
  if (u16) {
    a.out8 = reinterpret_cast<uint8_t*>(d->out_u16);
    a.maxval = (1 << d->u16_depth) - 1;
    a.h0 = d->h0;
    a.w0 = d->w0;
    a.top = d->top;
  }
  if (yuv16) {
    const rrin_yuv420_16& o = d->out_yuv16;
    a.oy = reinterpret_cast<uint8_t*>(const_cast<uint16_t*>(o.y));
    a.ou = reinterpret_cast<uint8_t*>(const_cast<uint16_t*>(o.u));
    a.ov = reinterpret_cast<uint8_t*>(const_cast<uint16_t*>(o.v));
    a.o_img = o.img_stride;
    a.oy_pitch = o.y_pitch;
    a.oc_pitch = o.c_pitch;
    a.oc_step = o.c_step;
    a.yc = d->yuv_coef;
    a.maxval = (1 << o.depth) - 1;
    a.shift = o.shift;
    a.h0 = d->h0;
    a.w0 = d->w0;
    a.top = d->top;
  }
  if (d->mode == RRIN_HEAD_FLOW && d->flow_raw.hi) {
    if (!h8_ok(d->flow_raw, d->prec) || d->flow_raw.g.h != h || d->flow_raw.g.w != w) return RRIN_E_SHAPE;
    a.fr = rec_view(d->flow_raw);
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
  hipStream_t st = (hipStream_t)stream;
  switch (d->mode) {
    case RRIN_HEAD_PLAIN:
      if (d->cout == 2) return head_launch<2, RRIN_HEAD_PLAIN>(a, d->prec, grid, st);
      if (d->cout == 3) return head_launch<3, RRIN_HEAD_PLAIN>(a, d->prec, grid, st);
      if (d->cout == 4) return head_launch<4, RRIN_HEAD_PLAIN>(a, d->prec, grid, st);
      return RRIN_E_ARG;
    case RRIN_HEAD_FLOW:
      return d->cout == 4 ? head_launch<4, RRIN_HEAD_FLOW>(a, d->prec, grid, st) : RRIN_E_ARG;
    case RRIN_HEAD_REFINE:
      return d->cout == 4 ? head_launch<4, RRIN_HEAD_REFINE>(a, d->prec, grid, st) : RRIN_E_ARG;
    case RRIN_HEAD_MASK:
      return d->cout == 2 ? head_launch<2, RRIN_HEAD_MASK>(a, d->prec, grid, st) : RRIN_E_ARG;
    case RRIN_HEAD_FINAL:
      if (d->cout != 3) return RRIN_E_ARG;
      if (a.maxval) {  // the 16-bit forms (head_prepare set maxval for them alone)
        if (!a.oy) return head_launch<3, RRIN_HEAD_FINAL, false, true>(a, d->prec, grid, st);
        if (d->out_yuv16.chroma == RRIN_CHROMA_422)
          return head_launch<3, RRIN_HEAD_FINAL, true, true, RRIN_CHROMA_422>(a, d->prec, grid, st);
        if (d->out_yuv16.chroma == RRIN_CHROMA_444)
          return head_launch<3, RRIN_HEAD_FINAL, true, true, RRIN_CHROMA_444>(a, d->prec, grid, st);
        return head_launch<3, RRIN_HEAD_FINAL, true, true>(a, d->prec, grid, st);
      }
      if (!a.oy) return head_launch<3, RRIN_HEAD_FINAL>(a, d->prec, grid, st);
      if (d->out_yuv.chroma == RRIN_CHROMA_422)
        return head_launch<3, RRIN_HEAD_FINAL, true, false, RRIN_CHROMA_422>(a, d->prec, grid, st);
      if (d->out_yuv.chroma == RRIN_CHROMA_444)
        return head_launch<3, RRIN_HEAD_FINAL, true, false, RRIN_CHROMA_444>(a, d->prec, grid, st);
      return head_launch<3, RRIN_HEAD_FINAL, true>(a, d->prec, grid, st);
  }
  return RRIN_E_ARG;
}

// rrin_flow_tblend_h8 (map NULL) and rrin_flow_tblend_items_h8
static int flow_tblend_launch(const rrin_h8* fr, const rrin_h8* g16, const float* coef, int32_t n, const int32_t* map,
                              int32_t n_pairs, int32_t prec, void* stream) {
  if (!fr || !g16 || !coef || n < 1 || !rec_prec(prec)) return RRIN_E_ARG;
  if (!h8_ok(*fr, prec) || !h8_ok(*g16, prec) || g16->g_off != 0 || g16->groups * chans_per_rec(prec) < 16)
    return RRIN_E_SHAPE;
  if (fr->g.h != g16->g.h || fr->g.w != g16->g.w) return RRIN_E_SHAPE;
  const int h = g16->g.h, w = g16->g.w;
  const int64_t total = (int64_t)n * h * w;
  const int grid = (int)((total + 255) / 256);
  return with_format(prec, [&](auto f) {
    if (map)
      hipLaunchKernelGGL((flow_tblend_kernel<decltype(f), true>), dim3(grid), dim3(256), 0, (hipStream_t)stream,
                         rec_view(*fr), rec_view(*g16), coef, h, w, total, map, n_pairs);
    else
      hipLaunchKernelGGL((flow_tblend_kernel<decltype(f), false>), dim3(grid), dim3(256), 0, (hipStream_t)stream,
                         rec_view(*fr), rec_view(*g16), coef, h, w, total, map, n_pairs);
    return hip_code(hipGetLastError());
  });
}

extern "C" int rrin_flow_tblend_h8(const rrin_h8* fr, const rrin_h8* g16, const float* coef, int32_t n, int32_t prec,
                                   void* stream) {
  return flow_tblend_launch(fr, g16, coef, n, nullptr, n, prec, stream);
}

extern "C" int rrin_flow_tblend_items_h8(const rrin_h8* fr, const rrin_h8* g16, const float* coef, int32_t n,
                                         const int32_t* pair_map, int32_t n_pairs, int32_t prec, void* stream) {
  if (!pair_map || n_pairs < 1 || n_pairs > n) return RRIN_E_ARG;
  return flow_tblend_launch(fr, g16, coef, n, pair_map, n_pairs, prec, stream);
}

extern "C" int rrin_pack_g16_h8(const float* i0, const float* i1, int32_t n, const rrin_h8* g16, int32_t prec,
                                void* stream) {
  if (!i0 || !i1 || !g16 || n < 1 || !rec_prec(prec)) return RRIN_E_ARG;
  if (!h8_ok(*g16, prec) || g16->g_off != 0 || g16->groups * chans_per_rec(prec) < 16) return RRIN_E_SHAPE;
  const int64_t total = (int64_t)n * g16->g.h * g16->g.w;
  const int grid = (int)((total + 255) / 256);
  return with_format(prec, [&](auto f) {
    hipLaunchKernelGGL(pack_g16_kernel<decltype(f)>, dim3(grid), dim3(256), 0, (hipStream_t)stream, i0, i1,
                       rec_view(*g16), g16->g.h, g16->g.w, total);
    return hip_code(hipGetLastError());
  });
}

namespace rrin {
// rrin_pack_g16_u8_h8 for n images that read the frames of n_pairs pairs through the device map
// (NULL: image k reads frame k, n_pairs == n); the stride rule is on the n_pairs frames of a stack
int pack_g16_u8_items(const uint8_t* f0, const uint8_t* f1, int64_t img_stride, int32_t n, int32_t h0, int32_t w0,
                      const rrin_h8* g16, int32_t prec, const int32_t* map, int32_t n_pairs, hipStream_t st,
                      int32_t mult) {
  if (!f0 || !f1 || !g16 || n < 1 || !rec_prec(prec)) return RRIN_E_ARG;
  if (n_pairs < 1 || n_pairs > n || (!map && n_pairs != n)) return RRIN_E_ARG;
  if (!h8_ok(*g16, prec) || g16->g_off != 0 || g16->groups * chans_per_rec(prec) < 16) return RRIN_E_SHAPE;
  const int h = g16->g.h, w = g16->g.w;
  if (h0 < 1 || w0 < 1 || h != pad_up(h0, mult) || w != pad_up(w0, mult)) return RRIN_E_SHAPE;
  if (img_stride < (int64_t)h0 * w0 * 3 && n_pairs > 1) return RRIN_E_ARG;
  if (n > 65535 || h > 65535) return RRIN_E_SHAPE;  // grid y / z
  const dim3 grid((w + 255) / 256, h, n);
  return with_format(prec, [&](auto f) {
    if (map)
      hipLaunchKernelGGL((pack_g16_u8_kernel<decltype(f), true>), grid, dim3(256), 0, st, f0, f1, img_stride, w0,
                         h - h0, rec_view(*g16), w, map, n_pairs);
    else
      hipLaunchKernelGGL((pack_g16_u8_kernel<decltype(f), false>), grid, dim3(256), 0, st, f0, f1, img_stride, w0,
                         h - h0, rec_view(*g16), w, map, n_pairs);
    return hip_code(hipGetLastError());
  });
}

int pack_g16_u16_items(const uint16_t* f0, const uint16_t* f1, int64_t img_stride, int32_t n, int32_t h0, int32_t w0,
                       int32_t depth, const rrin_h8* g16, int32_t prec, const int32_t* map, int32_t n_pairs,
                       hipStream_t st, int32_t mult) {
  if (!f0 || !f1 || !g16 || n < 1 || !rec_prec(prec) || depth < 9 || depth > 16) return RRIN_E_ARG;
  if (n_pairs < 1 || n_pairs > n || (!map && n_pairs != n)) return RRIN_E_ARG;
  if (!h8_ok(*g16, prec) || g16->g_off != 0 || g16->groups * chans_per_rec(prec) < 16) return RRIN_E_SHAPE;
  const int h = g16->g.h, w = g16->g.w;
  if (h0 < 1 || w0 < 1 || h != pad_up(h0, mult) || w != pad_up(w0, mult)) return RRIN_E_SHAPE;
  if (img_stride < (int64_t)h0 * w0 * 3 && n_pairs > 1) return RRIN_E_ARG;
  if (n > 65535 || h > 65535) return RRIN_E_SHAPE;  // grid y / z
  const dim3 grid((w + 255) / 256, h, n);
  return with_format(prec, [&](auto f) {
    if (map)
      hipLaunchKernelGGL((pack_g16_u16_kernel<decltype(f), true>), grid, dim3(256), 0, st, f0, f1, img_stride, w0,
                         h - h0, rec_view(*g16), w, (1 << depth) - 1, map, n_pairs);
    else
      hipLaunchKernelGGL((pack_g16_u16_kernel<decltype(f), false>), grid, dim3(256), 0, st, f0, f1, img_stride, w0,
                         h - h0, rec_view(*g16), w, (1 << depth) - 1, map, n_pairs);
    return hip_code(hipGetLastError());
  });
}
}  // namespace rrin

extern "C" int rrin_pack_g16_u8_h8(const uint8_t* f0, const uint8_t* f1, int64_t img_stride, int32_t n, int32_t h0,
                                   int32_t w0, const rrin_h8* g16, int32_t prec, void* stream) {
  return pack_g16_u8_items(f0, f1, img_stride, n, h0, w0, g16, prec, nullptr, n, (hipStream_t)stream);
}

extern "C" int rrin_pack_g16_u16_h8(const uint16_t* f0, const uint16_t* f1, int64_t img_stride, int32_t n, int32_t h0,
                                    int32_t w0, int32_t depth, const rrin_h8* g16, int32_t prec, void* stream) {
  return pack_g16_u16_items(f0, f1, img_stride, n, h0, w0, depth, g16, prec, nullptr, n, (hipStream_t)stream);
}
