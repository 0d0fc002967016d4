// fp16 3x3 conv as Winograd F(2x2,3x3) on H8 records (8 fp16 channels per 16-B record):
// the register-U tile of conv_winoc.hip (kind 6) with v_mfma_f32_32x32x16_f16.  Tile
// config kWinoC2Cfg at precision RRIN_PREC_F16 (BASELINE configs C3-C5).
//
// Replaces nn.Conv2d(3, pad=1) + LeakyReLU(0.1) (unet.py:29,59-63), the fused
// avg_pool2d output (unet.py:46), the cat by channel offset (unet.py:93) and the
// sub-pixel form of Upsample + up conv (unet.py:77-78), as the direct-form
// conv3x3_h8_kernel does at fp16.
//
// Arithmetic:
//   * U = G g G^T per (co, ci, point) in double on the host, times the conv's
//     power-of-two weight scale, rounded once to fp16 (rrin_pack_conv3x3_wino_h8);
//   * V = B^T d B in packed fp16 (v_pk_fma_f16 with a +-1 factor = one IEEE add per
//     element, two levels): the fp16 activations d, four at most added per V element;
//   * M[xi] = sum_ci U[xi] V[xi]: exact fp16 products, fp32 accumulation (the MFMA);
//   * the output transform, scale, bias, leaky and pool in fp32; the stores round once
//     to fp16 and flag any value fp16 cannot hold (the range guard of the H8 paths).
// |V| <= 4 max|d|: activations beyond 16376 can overflow V where the direct form would
// not; the inf / NaN then reaches the output check and the forward fails loudly.
//
// Tile (as kind 6): BM = 64 output channels (2 co tiles) x 32 px x TH = 4 NT rows.  Wave yw
// (0-3) owns B^T row yw (points 4 yw .. 4 yw + 3); lane (j, hh): patch j of the 32-patch MFMA
// tile, record group hh of the 16-channel chunk (channels 8 hh .. 8 hh + 7): the B operand
// of 32x32x16 (k = 8 (lane / 32) + e) is the transform of that lane's own records, and the A
// operand the packed U record [xi][hh][co][8].  Per wave and chunk: 8 NT MFMAs, 8 U loads
// (one 16-B record per lane each, from L2 into registers a chunk ahead), 8 NT window reads,
// 32 NT packed-f16 VALU, 2-3 LDS-DMA pieces of the raw tile (3 stages, one barrier).
#include "wino_tile.hpp"

// Ablation builds only (tools/build_wino_variant.sh, outputs wrong by design): 1 no U loads
// after the prologue, 2 no raw DMA after the prologue, 4 no transform VALU, 8 no epilogue
// stores, 16 no window reads after the prologue
#ifndef RRIN_WINOH_ABL
#define RRIN_WINOH_ABL 0
#endif

namespace rrin {

// 4 fp32 values -> 4 RNE fp16 values as one 8-B record half
__device__ inline uint2 wh_pack4(const float* v) {
  const half2v h0 = __builtin_convertvector((float2v){v[0], v[1]}, half2v);
  const half2v h1 = __builtin_convertvector((float2v){v[2], v[3]}, half2v);
  return make_uint2(__builtin_bit_cast(unsigned, h0), __builtin_bit_cast(unsigned, h1));
}

// NT 1 (kind 6 at fp16): 128 accumulator registers, two blocks per CU.  (NT 2, round 5's kind 9 --
// each U record on 2 patch tiles, one wave per SIMD -- ran 1.2-2.3x kind 6's time per conv and was
// removed in round 6 with the other rejected kinds)
struct WinoH {
  static constexpr int NT = 1;
  static constexpr int TH = 4 * NT;
  static constexpr int RG = (TH + 2) * 34;          // raw records per group
  static constexpr int RAW = 2 * RG;                // per chunk (2 groups = 16 channels)
  static constexpr int PIECES = (RAW + 255) / 256;  // DMA pieces per thread (every wave issues all)
  static constexpr int STAGE = PIECES * 256;        // records per LDS stage (the tail is a dummy)
  static constexpr int NS = 3;                      // stages: chunk c + 2 lands while c computes
  static constexpr int XREC = NT * 4 * 8 * 64;      // output-transform exchange, one co tile
  static constexpr size_t LDS = (size_t)(NS * STAGE > XREC ? NS * STAGE : XREC) * 16;
};
static_assert(WinoH::LDS == kWinoCLds1, "LDS size (common.hpp)");

template <int EPI>
__global__ __launch_bounds__(256, 2) void conv3x3_winoh_kernel(ConvH8Args a) {
  using G = WinoH;
  constexpr int NT = G::NT, CT = 2, BM = 64, TH = G::TH, RG = G::RG, STAGE = G::STAGE, P = G::PIECES;
  extern __shared__ __attribute__((aligned(16))) uint4 smem4[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int yw = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, hh = lane >> 5;
  const int bid = wino_xcd_bid();
  const int ntiles = a.co_blocks * a.tiles_x * a.tiles_y * a.n;
  if (bid >= ntiles) return;
  const int nch = a.nchunks;
  const WinoTile tp = wino_tile_pos(a, ntiles, bid, 32, TH);
  const int cob = tp.cob, x0 = tp.x0, y0 = tp.y0, img = tp.img;

  // ---- raw tile: rows y0 - 1 .. y0 + TH, cols x0 - 1 .. x0 + 32 of the chunk's two record
  // groups, by buffer_load ... lds (a lane past the tile re-reads record 0 into the dummy tail)
  const uint4* tbase = a.src_hi + (int64_t)img * a.src_img + (int64_t)y0 * a.src_wp + x0 + (kH8PadLeft - 1);
  uint32_t voff[P];
#pragma unroll
  for (int it = 0; it < P; ++it) {
    const int idx = tid + 256 * it;
    const int g = idx >= RG ? 1 : 0;
    const int rem = idx < G::RAW ? idx - g * RG : 0;
    const int r = rem / 34, pos = rem - r * 34;
    const int col = pos < 17 ? 2 * pos : 2 * (pos - 17) + 1;
    voff[it] = (uint32_t)((idx < G::RAW ? (int64_t)g * a.src_gp : 0) + (int64_t)r * a.src_wp + col) * 16u;
  }
  const int64_t chunk_stride = 2 * a.src_gp;  // records between the group pairs of consecutive chunks
  auto issue_raw_at = [&](const uint4* base, int s) {
    const auto rs = buf_rsrc(base);
#pragma unroll
    for (int it = 0; it < P; ++it) buf_dma16(rs, smem4 + s * STAGE + 256 * it + 64 * yw, voff[it]);
  };
  const uint4* raw_next = tbase + (nch > 2 ? 2 : nch - 1) * chunk_stride;

  // ---- U (A operands) straight into registers: packing [cob][chunk][xi][hh][BM co][8 halves]
  const auto ur = buf_rsrc(a.w_hi + (int64_t)cob * nch * 32 * BM);
  const uint32_t uvoff = (uint32_t)(hh * BM + j) * 16u;
  auto load_u = [&](int c, int x, int t) {
    const int soff = c * (32 * BM * 16) + (4 * yw + (x & 2)) * (2 * BM * 16);
    const int imm = (x & 1) * 2048 + t * 512;
    return __builtin_bit_cast(half8, buf_load16(ur, uvoff + imm, soff));
  };

  // ---- B operands: lane (j, hh) of N tile nt is patch (pr = 2 nt + (j >> 4), jx), the
  // second patch row's columns rotated by 12 (distinct banks per ds_read_b128 lane group)
  const int jx = (j + 12 * (j >> 4)) & 15;
  const int ra = yw == 0 ? 0 : (yw == 2 ? 2 : 1);
  const int rb = yw == 0 ? 2 : (yw == 1 ? 2 : (yw == 2 ? 1 : 3));
  const _Float16 sgh = yw == 1 ? (_Float16)1.0f : (_Float16)-1.0f;
  const half8 sg = {sgh, sgh, sgh, sgh, sgh, sgh, sgh, sgh};
  // -1 in every half, opaque to the compiler (it would turn fma(-1, b, a) back into a - b)
  unsigned m1w = 0xBC00BC00u;
  asm volatile("" : "+v"(m1w));
  const half8 m1 = __builtin_bit_cast(half8, make_uint4(m1w, m1w, m1w, m1w));
  int pcol[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) pcol[k] = hh * RG + (2 * (j >> 4)) * 34 + wino_col(2 * jx + k);
  const int oa = ra * 34, ob = rb * 34;

  floatx16 acc[CT][NT][4];
  // (set by chunk 0's first MFMA of each accumulator: C = 0, no zeroing per tile)
  half8 u[CT][4];   // U of the chunk being computed (point x reloaded after its MFMAs)
  half8 v[NT][4];   // B operands of the chunk being computed
  half8 d[NT][8];   // window records of the N tiles of the next chunk

  auto read_raw = [&](int s, int nt) {
    const uint4* rw = smem4 + s * STAGE + nt * 4 * 34;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      d[nt][2 * k] = __builtin_bit_cast(half8, rw[oa + pcol[k]]);
      d[nt][2 * k + 1] = __builtin_bit_cast(half8, rw[ob + pcol[k]]);
    }
  };
  // B^T row yw of the window, then the 4 points of that row: t_k = d[ra][k] +- d[rb][k],
  // V = (t0 - t2, t1 + t2, t2 - t1, t1 - t3); one fp16 rounding per add
  auto transform = [&](int nt) {
    if constexpr ((RRIN_WINOH_ABL & 4) != 0) {
      v[nt][0] = d[nt][0], v[nt][1] = d[nt][2], v[nt][2] = d[nt][4], v[nt][3] = d[nt][6];
      return;
    }
    half8 tr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) tr[k] = __builtin_elementwise_fma(sg, d[nt][2 * k + 1], d[nt][2 * k]);
    // a - b as fma(-1, b, a): one v_pk_fma_f16 per register (a vector subtraction is
    // split into two v_sub_f16 and a v_pack_b32_f16 by the compiler)
    v[nt][0] = __builtin_elementwise_fma(m1, tr[2], tr[0]);
    v[nt][1] = tr[1] + tr[2];
    v[nt][2] = __builtin_elementwise_fma(m1, tr[1], tr[2]);
    v[nt][3] = __builtin_elementwise_fma(m1, tr[3], tr[1]);
  };
  auto mfma_point = [&](int x, int nt, const bool first) {
#pragma unroll
    for (int t = 0; t < CT; ++t)
      acc[t][nt][x] = __builtin_amdgcn_mfma_f32_32x32x16_f16(u[t][x], v[nt][x], first ? floatx16{} : acc[t][nt][x], 0, 0,
                                                                  0);
  };
  auto reload_u = [&](int c, int x) {
#pragma unroll
    for (int t = 0; t < CT; ++t) u[t][x] = load_u(c, x, t);
  };
  // LDS-DMA of a stage is visible to the other waves after the issuing wave's vmcnt wait and
  // a barrier; the barrier is bare (a __syncthreads() would drain vmcnt to 0)
  auto bar = [&]() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
  auto fence = [&]() { __builtin_amdgcn_sched_barrier(0); };

  // Chunk c (U(c) in u, its B operands in v): the schedule of conv_winoc.hip's chunk --
  // points 0-2, each followed by its U load for chunk c + 1; the wait for raw(c + 1); the
  // barrier; raw(c + 2); per N tile chunk c + 1's window reads, point 3, its transform;
  // point 3's U load.  VMEM order per chunk: U pts 0-2, raw(c + 2), U pt 3.
  auto chunk = [&](int c, int s, const bool more, const bool first) {
#pragma unroll
    for (int x = 0; x < 3; ++x) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) mfma_point(x, nt, first);
      if (more && !(RRIN_WINOH_ABL & 1)) reload_u(c + 1, x);
      fence();
    }
    if (more) {
      RRIN_VMWAIT(0, (RRIN_WINOH_ABL & 1) ? 0 : 4 * CT);
      bar();
      if (!(RRIN_WINOH_ABL & 2)) issue_raw_at(raw_next, s == 0 ? 2 : s - 1);
      if (c + 3 < nch) raw_next += chunk_stride;
    }
    const int s1 = s == 2 ? 0 : s + 1;
    // every N tile's window reads first, then point 3's MFMAs (they cover the reads), then
    // the transforms of chunk c + 1
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      if (more && !(RRIN_WINOH_ABL & 16)) read_raw(s1, nt);
    fence();
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) mfma_point(3, nt, first);
    fence();
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      if (more) transform(nt);
    if (more && !(RRIN_WINOH_ABL & 1)) reload_u(c + 1, 3);
  };

  // prologue in the steady state's VMEM order: raw(0), U(0) pts 0-2, raw(1), U(0) pt 3
  issue_raw_at(tbase, 0);
  vm_fence();
#pragma unroll
  for (int x = 0; x < 3; ++x) reload_u(0, x);
  vm_fence();
  issue_raw_at(nch > 1 ? tbase + chunk_stride : tbase, 1);
  vm_fence();
  reload_u(0, 3);
  vm_fence();
  RRIN_VMWAIT(P, 4 * CT);
  bar();
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    read_raw(0, nt);
    transform(nt);
  }
  {
    int s = 0;
    if (nch > 1) {  // chunk 0 peeled: its MFMAs start the accumulators from C = 0
      chunk(0, s, true, true);
      s = 1;
      for (int c = 1; c + 1 < nch; ++c) {
        chunk(c, s, true, false);
        s = s == 2 ? 0 : s + 1;
      }
      chunk(nch - 1, s, false, false);
    } else {
      chunk(0, s, false, true);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the DMA past the end has landed
  // the epilogue's bias values, loaded now: their latency hides behind the exchange
  float bsv[CT][16];
#pragma unroll
  for (int t = 0; t < CT; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) bsv[t][i] = a.bias[(CT * cob + t) * 32 + 8 * (i >> 2) + 4 * hh + (i & 3)];
  __syncthreads();  // every read of the stages done before the exchange reuses the LDS

  // ---- output transform (kind 6's order): Q[c] = sum_x M[x] A[x][c] of this wave's B^T
  // row, Y[0][c] = (Q0 + Q1) + Q2, Y[1][c] = (Q1 - Q2) - Q3 over the four waves, exchanged
  // through LDS one co tile at a time; wave yw then finishes output row r = yw & 1, column
  // cc = yw >> 1 of its patches
  floatx4* X = reinterpret_cast<floatx4*>(smem4);
  const int r = yw & 1, cc = yw >> 1;
  uint4* dst = a.dst_hi + (int64_t)img * a.dst_img;
  const float isc = a.inv_wscale;
  bool bad = false;  // a stored value fp16 cannot hold (range guard)
  // 4 channels (lane half hh of an 8-channel record) -> 8-B half hh of record rec
  auto store4 = [&](uint4* base, int64_t rec, const float* vv) {
    if constexpr ((RRIN_WINOH_ABL & 8) != 0) return;
    bad |= !(fmaxf(fmaxf(fabsf(vv[0]), fabsf(vv[1])), fmaxf(fabsf(vv[2]), fabsf(vv[3]))) <= kF16Max);
    reinterpret_cast<uint2*>(base + rec)[hh] = wh_pack4(vv);
  };
#pragma unroll
  for (int t = 0; t < CT; ++t) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        floatx4 g;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int vi = 4 * k + e, c2 = vi >> 4, i = vi & 15;
          const float m0 = acc[t][nt][0][i], m1 = acc[t][nt][1][i], m2 = acc[t][nt][2][i], m3 = acc[t][nt][3][i];
          g[e] = c2 == 0 ? (m0 + m1) + m2 : (m1 - m2) - m3;
        }
        X[((nt * 4 + yw) * 8 + k) * 64 + lane] = g;
      }
    __syncthreads();
    float yv[NT][16];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4) {
        const int k = 4 * cc + k4;
        const floatx4 q0 = X[((nt * 4 + 0) * 8 + k) * 64 + lane];
        const floatx4 q1 = X[((nt * 4 + 1) * 8 + k) * 64 + lane];
        const floatx4 q2 = X[((nt * 4 + 2) * 8 + k) * 64 + lane];
        const floatx4 q3 = X[((nt * 4 + 3) * 8 + k) * 64 + lane];
#pragma unroll
        for (int e = 0; e < 4; ++e) yv[nt][4 * k4 + e] = r == 0 ? (q0[e] + q1[e]) + q2[e] : (q1[e] - q2[e]) - q3[e];
      }
    __syncthreads();  // X is rewritten by the next co tile / the pool exchange
    const int cobe = CT * cob + t;  // 32-channel block of this co tile
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int pr = 2 * nt + (j >> 4);
      const int y = y0 + 2 * pr + r, x = x0 + 2 * jx + cc;
      if constexpr (EPI == RRIN_EPI_SUBPIXEL) {
        // rows co' = (co / 8) 32 + phase 8 + co % 8: co tile cobe holds real channels
        // 8 cobe .. + 7 (one record group), i >> 2 its phase (py, px)
        const int HH = 2 * a.h, WW = 2 * a.w, creal = a.cout >> 2;
        if (cobe * 32 < a.cout && y < a.h && x < a.w) {
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            const int Y = 2 * y + (qq >> 1), XX = 2 * x + (qq & 1);
            const int64_t ri = ring_index(Y, XX, HH, WW);
            if (ri >= 0) {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                a.edge[((int64_t)img * creal + cobe * 8 + 4 * hh + e) * a.ring + ri] = yv[nt][4 * qq + e] * isc;
            } else {
              float vv[4];
#pragma unroll
              for (int e = 0; e < 4; ++e) vv[e] = yv[nt][4 * qq + e] * isc + bsv[t][4 * qq + e];
              store4(dst, (int64_t)cobe * a.dst_gp + (int64_t)(Y + 1) * a.dst_wp + XX + kH8PadLeft, vv);
            }
          }
        }
      } else {
        float vv[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          float tv = yv[nt][i] * isc + bsv[t][i];
          if constexpr (EPI != RRIN_EPI_LINEAR) tv = leaky(tv, a.slope);
          vv[i] = tv;
        }
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          if (cobe * 32 + 8 * qq < a.cout && y < a.h && x < a.w) {
            const int64_t rec = (int64_t)(cobe * 4 + qq) * a.dst_gp + (int64_t)(y + 1) * a.dst_wp + x + kH8PadLeft;
            store4(dst, rec, &vv[4 * qq]);
            if constexpr (EPI == RRIN_EPI_LEAKY_REP) {  // edge replicate into the padding ring
              const int dy0 = y == 0 ? -1 : 0, dy1 = y == a.h - 1 ? 1 : 0;
              const int dx0 = x == 0 ? -1 : 0, dx1 = x == a.w - 1 ? 1 : 0;
              for (int dy = dy0; dy <= dy1; ++dy)
                for (int dx = dx0; dx <= dx1; ++dx)
                  if (dy | dx) store4(dst, rec + (int64_t)dy * a.dst_wp + dx, &vv[4 * qq]);
            }
          }
        }
        if constexpr (EPI == RRIN_EPI_LEAKY_POOL) {
          // the patch's four outputs (yw = (r, c)) meet in LDS; wave 0 writes
          // avg = 0.25 ((Y00 + Y10) + (Y01 + Y11)), kind 6's order
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            floatx4 g;
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = vv[4 * k + e];
            X[(yw * 4 + k) * 64 + lane] = g;
          }
          __syncthreads();
          if (yw == 0) {
            const int xp = x0 + 2 * jx, yp = y0 + 2 * pr;
            uint4* pdst = a.pool_hi + (int64_t)img * a.pool_img;
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
              const floatx4 y00 = X[(0 * 4 + qq) * 64 + lane];
              const floatx4 y10 = X[(1 * 4 + qq) * 64 + lane];
              const floatx4 y01 = X[(2 * 4 + qq) * 64 + lane];
              const floatx4 y11 = X[(3 * 4 + qq) * 64 + lane];
              if (cobe * 32 + 8 * qq < a.cout && yp < a.h && xp < a.w) {
                float s4[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) s4[e] = 0.25f * ((y00[e] + y10[e]) + (y01[e] + y11[e]));
                store4(pdst, (int64_t)(cobe * 4 + qq) * a.pool_gp + (int64_t)(yp / 2 + 1) * a.pool_wp + xp / 2 +
                                 kH8PadLeft,
                       s4);
              }
            }
          }
          __syncthreads();
        }
      }
    }
  }
  if (bad && a.status) *a.status = 1;
}


template <int EPI>
static int launch_winoh_k(const ConvH8Args& a, hipStream_t st, rrin_launch_info* info) {
  auto k = conv3x3_winoh_kernel<EPI>;
  static LdsAttr attr;
  constexpr size_t lds = WinoH::LDS;
  if (int e = attr.ensure((const void*)k, (int)lds, st)) return e;
  const int64_t grid = (int64_t)a.co_blocks * a.tiles_x * a.tiles_y * a.n;
  if (info) return launch_report(info, grid, grid, 0, 0);
  hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(256), lds, st, a);
  return hip_code(hipGetLastError());
}

// co-block groups (wino_cob_group): U of a group within this many KB
#ifndef RRIN_WINOH_UGROUP_KB
#define RRIN_WINOH_UGROUP_KB 2048
#endif

int launch_winoh(const ConvH8Args& a, int epi, hipStream_t st, rrin_launch_info* info) {
  ConvH8Args b = a;
  // U of one co block: nchunks x 32 BM records
  b.cob_group = wino_cob_group(a.co_blocks, (int64_t)a.nchunks * 32 * 64 * 16, RRIN_WINOH_UGROUP_KB);
  return wino_dispatch_epi(epi, [&](auto e) { return launch_winoh_k<decltype(e)::value>(b, st, info); });
}

}  // namespace rrin
