// Exact-fp32 3x3 conv as Winograd F(2x2, 3x3) on fp32 records (R32) with the
// f32-input matrix cores (v_mfma_f32_32x32x2_f32): the 4-wave tile of 8 accumulators per
// wave, Winograd kind 1 (tile config 18) of the record-layout conv table
// (rrin_conv3x3_h8_fwd, precision F32R).  No conv of the default schedule runs it: it is
// selected by engine.WINO_KIND = 1 (bench.py --wino-kind) and is the reference the other
// F(2x2, 3x3) tiles are bitwise equal to.  conv_winoq.hip (kinds 3, 4) runs this tile, with
// this file's weight packing, LDS image of the raw input and arithmetic order, on twice the
// waves of 4 accumulators; conv_winoc.hip (kinds 6, 7) keeps the arithmetic with U in registers.
//
// Replaces the same reference ops as conv3x3_h8_kernel: nn.Conv2d(3, pad=1) +
// LeakyReLU(0.1) (unet.py:29,59-63), the fused avg_pool2d output (unet.py:46),
// the cat by channel offset (unet.py:93), and the sub-pixel form of Upsample +
// up conv (unet.py:77-78).
//
// Arithmetic: every operation is an IEEE fp32 operation -- no reduced-precision
// operand anywhere.  Per 2x2 output patch and input channel the 4x4 input window
// d becomes V = B^T d B (adds only), the weights U = G g G^T (host, in double,
// rounded once to fp32), and per transform point xi (16) the channel
// contraction M[xi] = sum_ci U[xi] V[xi] runs on the fp32 MFMA; the patch is
// Y = A^T M A (adds only).  16 multiplies per patch and channel pair instead of
// the direct form's 36: 2.25x fewer MFMA cycles for the same conv.
//   B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]
//   G   = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]
//   A^T = [1 1 1 0; 0 1 -1 -1]
//
// Block: 256 threads = 4 waves, tile = 32 output channels x 32 px x 8 rows =
// 64 patches (16 wide x 4 tall).  Wave (xh, ph) owns transform rows xi_y in
// {2xh, 2xh+1} (8 of the 16 points: 8 accumulators of 32 co x 32 patches, 128
// registers, so two blocks share a CU and cover each other's barriers) of the
// patch rows 2ph, 2ph+1.  K chunk = 8 channels (2 record groups): per point 4
// MFMAs (product e: lanes 0-31 channel e, lanes 32-63 channel 4+e).
// Each lane transforms exactly the B operands it feeds: the window rows of its
// patch (3 of 4: the two B^T rows of its xi_y pair), its 4 channels, straight
// from the LDS image of the raw input -- V never goes through LDS.
// Per chunk, double buffered in LDS (LDS-DMA, one chunk ahead):
//   raw input tile 2 groups x 10 rows x 34 cols (even columns, then odd, so
//                  the stride-2 window reads of 16 lanes are conflict-free)
//   U slab [xi][half][co] 16 x 2 x 32 records
// The output transform's two halves (xi_y 0-1, 2-3) meet through LDS: wave
// xh = 0 finishes output row 0 of each patch, xh = 1 row 1.
#include "wino_tile.hpp"

namespace rrin {

// raw tile records per group (10 rows) and chunk (2 groups), and the stride of a raw buffer
constexpr int kWnRawG = 10 * kWnRawCols, kWnRaw = 2 * kWnRawG, kWnRawStride = 704;
static_assert(kWinoLds == (size_t)(2 * kWnRawStride + 2 * kWnU) * 16, "LDS size");
// ABL: kernel-lab ablations only (built into librrin_lab.so under RRIN_LAB; the
// product library instantiates ABL = 0): 1 no weight DMA after chunk 1, 2 no raw
// DMA after chunk 1, 4 no MFMAs (operands kept live), 8 no transform arithmetic.
//
// Main loop: a register pipeline over half-chunks (half = one B^T row yl of the
// wave's pair = 16 MFMAs, point-major: the 4 products of point x back to back on
// accumulator 4 yl + x).  While the MFMAs of half H issue, the window reads of half
// H + 1 are in flight, and once point x's 4 MFMAs have issued its U / B registers
// take point x of half H + 1 (U read from LDS, B transformed in the MFMA shadows):
// no MFMA waits on an LDS round trip, and one operand set is live.  The chunk's
// barrier sits at the start of its second half: every read of the chunk's buffers
// has been consumed by then, so right after it those buffers take chunk c + 2's
// LDS-DMA and the reads of chunk c + 1 start.
template <int EPI, int ABL = 0>
__global__ __launch_bounds__(256, 2) void conv3x3_wino_kernel(ConvH8Args a) {
  extern __shared__ __attribute__((aligned(16))) uint4 smem4[];
  uint4* s_raw = smem4;                      // [2][kWnRawStride]: [group][row][wino_col]
  uint4* s_u = smem4 + 2 * kWnRawStride;     // [2][16][2][32]

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int xh = wv & 1, ph = wv >> 1, j = lane & 31, hh = lane >> 5;
  const int bid = wino_xcd_bid();
  const int ntiles = a.co_blocks * a.tiles_x * a.tiles_y * a.n;
  if (bid >= ntiles) return;
  const int nch = a.nchunks;

  // tile -> (channel block, column, row, image); staging bases of its raw input
  // rows y0-1..y0+8, cols x0-1..x0+32 and of its U slabs
  struct Tile {
    int cob, x0, y0, img;
  } cur;
  {
    int t = bid;
    cur.cob = t % a.co_blocks;
    t /= a.co_blocks;
    cur.x0 = (t % a.tiles_x) * 32;
    t /= a.tiles_x;
    cur.y0 = (t % a.tiles_y) * 8;
    cur.img = t / a.tiles_y;
  }
  const uint4* tsrc = a.src_hi + (int64_t)cur.img * a.src_img + (int64_t)cur.y0 * a.src_wp + cur.x0 + (kH8PadLeft - 1);
  const uint4* wsrc = a.w_hi + (int64_t)cur.cob * nch * kWnU + tid;

  // ---- staging.  Per thread and DMA piece (3): its group of the chunk, its offset
  // inside the group plane (groups past cin read the same column of the zero
  // top-padding row of group 0 instead: they meet zero weights).
  int64_t p_off[3];
  int p_g[3], p_zero[3];
#pragma unroll
  for (int it = 0; it < 3; ++it) {
    const int idx = tid + 256 * it;
    const int g = idx >= kWnRawG ? 1 : 0;
    const int rem = idx - g * kWnRawG;
    const int r = rem / kWnRawCols, pos = rem - r * kWnRawCols;
    const int col = pos < 17 ? 2 * pos : 2 * (pos - 17) + 1;
    p_g[it] = g;
    p_off[it] = (int64_t)g * a.src_gp + r * a.src_wp + col;
    p_zero[it] = col - cur.y0 * a.src_wp;
  }
  auto issue_raw = [&](int c, int buf) {
#pragma unroll
    for (int it = 0; it < 3; ++it) {
      if (it < 2 || tid + 512 < kWnRaw) {
        const int gg = 2 * c + p_g[it];
        const int64_t off = gg * 4 < a.cin ? (int64_t)(2 * c) * a.src_gp + p_off[it] : (int64_t)p_zero[it];
        dma16(tsrc + off, s_raw + buf * kWnRawStride + 256 * it + (tid & ~63));
      }
    }
  };
  auto issue_u = [&](int c, int buf) {
#pragma unroll
    for (int it = 0; it < 4; ++it) dma16(wsrc + (int64_t)c * kWnU + 256 * it, s_u + buf * kWnU + 256 * it + (tid & ~63));
  };
  auto issue = [&](int c, int buf) {
    if (!(ABL & 2) || c < 2) issue_raw(c, buf);
    if (!(ABL & 1) || c < 2) issue_u(c, buf);
  };

  // MFMA column j -> patch (row pr, column jx).  The second row's columns are
  // rotated by 12 so the window reads of the two rows (68 records apart) fall on
  // distinct banks in every ds_read_b128 lane group ({0-3,12-15,20-27}, {4-11,16-19,28-31}).
  const int pr = 2 * ph + (j >> 4), jx = (j + 12 * (j >> 4)) & 15;
  const int ra = xh ? 2 : 0, rb = xh ? 1 : 2, rd = xh ? 3 : 2;  // rc = 1
  const float sgn = xh ? -1.f : 1.f;
  // LDS addresses (records) of this lane's operands in buffer 0: U of point
  // (8 xh + 4 yl + x) at su0 + yl * 256 + x * 64; window records at rw0 + row * 34 + pc[k]
  const int su0 = 2 * kWnRawStride + (8 * xh) * 64 + hh * 32 + j;
  const int rw0 = hh * kWnRawG + (2 * pr) * kWnRawCols;
  int pc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) pc[k] = wino_col(2 * jx + k);
  const int r0a = (ra)*kWnRawCols, r0b = (rb)*kWnRawCols, r1a = kWnRawCols, r1b = (rd)*kWnRawCols;

  floatx16 acc[8];
  floatx4 u[4], v[4];  // operands of the half being issued; point x recycled after its MFMAs
  // U record of point (8 xh + 4 yl + x) of the chunk in buffer b
  auto read_u = [&](int b, int yl, int x) {
    return __builtin_bit_cast(floatx4, smem4[su0 + b * kWnU + yl * 256 + x * 64]);
  };
  // the 8 window records of B^T row yl (rows o0 / o1, 4 columns)
  auto read_raw = [&](int b, int yl, floatx4* d) {
    const uint4* rw = s_raw + b * kWnRawStride + rw0;
    const int o0 = yl ? r1a : r0a, o1 = yl ? r1b : r0b;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      d[2 * k] = __builtin_bit_cast(floatx4, rw[o0 + pc[k]]);
      d[2 * k + 1] = __builtin_bit_cast(floatx4, rw[o1 + pc[k]]);
    }
  };
  // column k of B^T row yl: t = d[ra] - d[rb] (yl 0) or d[1] + sgn d[rd] (yl 1)
  auto row_t = [&](int yl, const floatx4* d, int k) {
    if constexpr ((ABL & 8) != 0) return d[2 * k];
    floatx4 t;
    if (yl == 0) {
      t = d[2 * k] - d[2 * k + 1];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] = fmaf(sgn, d[2 * k + 1][e], d[2 * k][e]);
    }
    return t;
  };
  // the 4 MFMAs of point x of half yl (FIRST: chunk 0 starts from zero)
  auto mfma_point = [&](int yl, int x, bool first) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if constexpr ((ABL & 4) != 0) {
        asm volatile("" ::"v"(u[x][e]), "v"(v[x][e]));
      } else {
        const floatx16 c = (first && e == 0) ? floatx16{} : acc[4 * yl + x];
        acc[4 * yl + x] = __builtin_amdgcn_mfma_f32_32x32x2f32(u[x][e], v[x][e], c, 0, 0, 0);
      }
    }
  };
  // hard scheduling fence: keeps each stage's instructions between its fences, so the
  // reads stay ahead of the MFMAs
  auto fence = [&]() { __builtin_amdgcn_sched_barrier(0); };
  // one half: MFMAs of half yl (operands in u / v) while half (bn, yn) -- the next
  // one -- is read from buffer bn and transformed into u / v point by point
  auto half = [&](int yl, int bn, int yn, bool first) {
    floatx4 d[8], t[4];
    read_raw(bn, yn, d);
    fence();
    mfma_point(yl, 0, first);
    u[0] = read_u(bn, yn, 0);
    fence();
    t[0] = row_t(yn, d, 0);
    t[2] = row_t(yn, d, 2);
    mfma_point(yl, 1, first);
    v[0] = (ABL & 8) ? t[0] : t[0] - t[2];
    u[1] = read_u(bn, yn, 1);
    fence();
    t[1] = row_t(yn, d, 1);
    mfma_point(yl, 2, first);
    v[1] = (ABL & 8) ? t[1] : t[1] + t[2];
    u[2] = read_u(bn, yn, 2);
    fence();
    t[3] = row_t(yn, d, 3);
    mfma_point(yl, 3, first);
    v[2] = (ABL & 8) ? t[2] : t[2] - t[1];
    v[3] = (ABL & 8) ? t[3] : t[1] - t[3];
    u[3] = read_u(bn, yn, 3);
    fence();
  };

  // ---- prologue: chunk 0 staged, its first half's operands in u / v; chunk 1 in flight
  issue(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (nch > 1) issue(1, 1);
  {
    floatx4 d[8], t[4];
    read_raw(0, 0, d);
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = row_t(0, d, k);
    v[0] = (ABL & 8) ? t[0] : t[0] - t[2];
    v[1] = (ABL & 8) ? t[1] : t[1] + t[2];
    v[2] = (ABL & 8) ? t[2] : t[2] - t[1];
    v[3] = (ABL & 8) ? t[3] : t[1] - t[3];
#pragma unroll
    for (int x = 0; x < 4; ++x) u[x] = read_u(0, 0, x);
  }
  half(0, 0, 1, true);  // half (0, 0); reads of half (0, 1)
  // step c: half (c, 1) and half (c + 1, 0), the barrier at its top: chunk c + 1
  // landed everywhere and every read of chunk c's buffers (b) was consumed before
  // it, so b takes chunk c + 2's DMA.  No LDS read is pending across the barrier.
  auto step = [&](int c, bool first) {
    const int b = c & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (c + 2 < nch) issue(c + 2, b);
    half(1, b ^ 1, 0, first);   // half (c, 1); reads of half (c + 1, 0)
    half(0, b ^ 1, 1, false);   // half (c + 1, 0); reads of half (c + 1, 1)
  };
  if (nch > 1) step(0, true);
  for (int c = 1; c + 1 < nch; ++c) step(c, false);
  // the last chunk's second half (its "next half" reads fetch stale records)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  half(1, ((nch - 1) & 1) ^ 1, 0, nch == 1);
  // those reads complete before the epilogue reuses the LDS
  __syncthreads();

    // ---- output transform: Q[yl][c] = sum_x M[xi_y][x] A[x][c] for this wave's xi rows,
    // then Y[0][c] = Q0 + Q1 + Q2 (wave xh 0), Y[1][c] = Q1 - Q2 - Q3 (wave xh 1)
    float q[2][2][16];
#pragma unroll
    for (int yl = 0; yl < 2; ++yl)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float m0 = acc[4 * yl][i], m1 = acc[4 * yl + 1][i], m2 = acc[4 * yl + 2][i], m3 = acc[4 * yl + 3][i];
        q[yl][0][i] = (m0 + m1) + m2;
        q[yl][1][i] = (m1 - m2) - m3;
      }
    // wave xh 0 hands its Q1 (yl 1) to its partner, wave xh 1 its Q2 (yl 0): records
    // k 0-3 / 4-7 in the two U buffers (no DMA in flight and every read of them
    // consumed since the last chunk's barrier)
    floatx4* xlo = reinterpret_cast<floatx4*>(s_u);
    floatx4* xhi = reinterpret_cast<floatx4*>(s_u + kWnU);
    auto xslot = [&](int w, int k) { return (k < 4 ? xlo : xhi) + (w * 4 + (k & 3)) * 64 + lane; };
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      floatx4 g;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int v = 4 * k + e, c = v >> 4, i = v & 15;
        g[e] = xh ? q[0][c][i] : q[1][c][i];
      }
      *xslot(wv, k) = g;
    }
    __syncthreads();
    float yv[2][16];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const floatx4 pv = *xslot(wv ^ 1, k);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int v = 4 * k + e, c = v >> 4, i = v & 15;
        yv[c][i] = xh ? (pv[e] - q[0][c][i]) - q[1][c][i] : (q[0][c][i] + q[1][c][i]) + pv[e];
      }
    }

    // ---- epilogue: this lane's pixels (y, x0 + 2 jx + c), 16 channels 8 qq + 4 hh + e
    const int cob = cur.cob, x0 = cur.x0, img = cur.img;
    const int y = cur.y0 + 2 * pr + xh;
    uint4* dst = a.dst_hi + (int64_t)img * a.dst_img;
    auto store4 = [&](int64_t rec, const float* v) {
      dst[rec] = make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
    };
    if constexpr (EPI == RRIN_EPI_SUBPIXEL) {
      // rows co' = cob*32 + 8 qq + 4 hh + e: group cob of 8 real channels, phase qq = (py, px)
      const int HH = 2 * a.h, WW = 2 * a.w, creal = a.cout >> 2;
      if (cob * 32 < a.cout && y < a.h) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int x = x0 + 2 * jx + c;
          if (x >= a.w) continue;
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            const int Y = 2 * y + (qq >> 1), X = 2 * x + (qq & 1);
            const int64_t ri = ring_index(Y, X, HH, WW);
            if (ri >= 0) {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                a.edge[((int64_t)img * creal + cob * 8 + 4 * hh + e) * a.ring + ri] = yv[c][4 * qq + e];
            } else {
              float v[4];
#pragma unroll
              for (int e = 0; e < 4; ++e) v[e] = yv[c][4 * qq + e] + a.bias[cob * 32 + 8 * qq + 4 * hh + e];
              store4((int64_t)(2 * cob + hh) * a.dst_gp + (int64_t)(Y + 1) * a.dst_wp + X + kH8PadLeft, v);
            }
          }
        }
      }
    } else {
      float v[2][16];
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          float tv = yv[c][i] + a.bias[cob * 32 + 8 * (i >> 2) + 4 * hh + (i & 3)];
          if constexpr (EPI != RRIN_EPI_LINEAR) tv = leaky(tv, a.slope);
          v[c][i] = tv;
        }
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int x = x0 + 2 * jx + c;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          if (cob * 32 + 8 * qq < a.cout && y < a.h && x < a.w) {
            const int64_t rec = (int64_t)(cob * 8 + 2 * qq + hh) * a.dst_gp + (int64_t)(y + 1) * a.dst_wp + x + kH8PadLeft;
            store4(rec, &v[c][4 * qq]);
            if constexpr (EPI == RRIN_EPI_LEAKY_REP) {
              // edge replicate into the padding ring (read only by a sub-pixel up conv)
              const int dy0 = y == 0 ? -1 : 0, dy1 = y == a.h - 1 ? 1 : 0;
              const int dx0 = x == 0 ? -1 : 0, dx1 = x == a.w - 1 ? 1 : 0;
              for (int dy = dy0; dy <= dy1; ++dy)
                for (int dx = dx0; dx <= dx1; ++dx)
                  if (dy | dx) store4(rec + (int64_t)dy * a.dst_wp + dx, &v[c][4 * qq]);
            }
          }
        }
      }
      if constexpr (EPI == RRIN_EPI_LEAKY_POOL) {
        // row 1 of each patch (wave xh 1) meets row 0 (wave xh 0) in LDS, in the raw
        // buffers (idle now); avg = 0.25 ((v00 + v10) + (v01 + v11))
        floatx4* xp = reinterpret_cast<floatx4*>(s_raw);
        auto pslot = [&](int k) { return xp + (ph * 8 + k) * 64 + lane; };
        if (xh) {
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            floatx4 g;
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = v[(4 * k + e) >> 4][(4 * k + e) & 15];
            *pslot(k) = g;
          }
        }
        __syncthreads();
        if (!xh) {
          float v1[2][16];
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const floatx4 g = *pslot(k);
#pragma unroll
            for (int e = 0; e < 4; ++e) v1[(4 * k + e) >> 4][(4 * k + e) & 15] = g[e];
          }
          const int x = x0 + 2 * jx;
          uint4* pdst = a.pool_hi + (int64_t)img * a.pool_img;
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            if (cob * 32 + 8 * qq < a.cout && y < a.h && x < a.w) {
              float s4[4];
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const int i = 4 * qq + e;
                s4[e] = 0.25f * ((v[0][i] + v1[0][i]) + (v[1][i] + v1[1][i]));
              }
              const int64_t rec =
                  (int64_t)(cob * 8 + 2 * qq + hh) * a.pool_gp + (int64_t)(y / 2 + 1) * a.pool_wp + x / 2 + kH8PadLeft;
              pdst[rec] = make_uint4(__float_as_uint(s4[0]), __float_as_uint(s4[1]), __float_as_uint(s4[2]),
                                     __float_as_uint(s4[3]));
            }
          }
        }
      }
    }
}

template <int EPI, int ABL = 0>
static int launch_wino_k(const ConvH8Args& a, hipStream_t st, rrin_launch_info* info = nullptr) {
  auto k = conv3x3_wino_kernel<EPI, ABL>;
  static LdsAttr attr;
  if (int e = attr.ensure((const void*)k, (int)kWinoLds, st)) return e;
  const int64_t grid = (int64_t)a.co_blocks * a.tiles_x * a.tiles_y * a.n;
  if (info) return launch_report(info, grid, grid, 0, 0);
  hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(256), kWinoLds, st, a);
  return hip_code(hipGetLastError());
}


int launch_wino(const ConvH8Args& a, int epi, hipStream_t st, rrin_launch_info* info) {
  return wino_dispatch_epi(epi, [&](auto e) { return launch_wino_k<decltype(e)::value>(a, st, info); });
}

#ifdef RRIN_LAB
// kernel lab (librrin_lab.so only): kind 1's share of launch_wino_lab (conv_winoq.hip)
int launch_wino_lab1(const ConvH8Args& a, int abl, hipStream_t st) {
  switch (abl) {
    case 0: return launch_wino_k<RRIN_EPI_LEAKY, 0>(a, st);
    case 1: return launch_wino_k<RRIN_EPI_LEAKY, 1>(a, st);
    case 2: return launch_wino_k<RRIN_EPI_LEAKY, 2>(a, st);
    case 3: return launch_wino_k<RRIN_EPI_LEAKY, 3>(a, st);
    case 4: return launch_wino_k<RRIN_EPI_LEAKY, 4>(a, st);
    case 8: return launch_wino_k<RRIN_EPI_LEAKY, 8>(a, st);
    case 11: return launch_wino_k<RRIN_EPI_LEAKY, 11>(a, st);
    case 15: return launch_wino_k<RRIN_EPI_LEAKY, 15>(a, st);
  }
  return RRIN_E_CONFIG;
}
#endif

}  // namespace rrin
