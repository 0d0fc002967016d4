// Exact-fp32 3x3 conv as Winograd F(2x2, 3x3) on fp32 records (R32): the 4-waves-per-SIMD
// tiles, Winograd kinds 3 and 4 (tile configs 20 and 21) of the record-layout conv table
// (rrin_conv3x3_h8_fwd, precision F32R).
//
// The tile of kind 1 (conv_wino.hip: 32 output channels x 32 px, K chunks of 8 channels) with
// kind 1's weight packing, LDS image of the raw input and arithmetic order -- the outputs of
// an unsplit conv are bitwise kind 1's -- run by waves of 4 accumulators each instead of 8:
// wave (yw, pt) owns B^T row yw (transform points 4 yw .. 4 yw + 3) of patch rows 2 pt,
// 2 pt + 1, at <= 128 VGPRs, so two blocks give every SIMD four waves: more independent waves
// to keep the matrix pipe fed while others wait on LDS, barriers or their transform, instead
// of kind 1's deeper per-wave pipeline.  The four yw waves of a patch-row pair meet in the
// output transform through LDS.
//   kind 3 (PT 2): 8 waves, 8 rows per tile
//   kind 4 (PT 1): 4 waves, 4 rows per tile -- twice the tiles for the few-tile deep levels
// Per chunk, two stages of [raw input tile | U slab] in LDS (LDS-DMA, one chunk ahead), one
// barrier per chunk.
//
// On top of the tile: split-K (SK: the K slices of a tile on workgroups of their own, summed in
// slice order by the last one) and the sub-pixel ring fold (RF: the ring fix-up of a sub-pixel
// up conv inside the conv's launch; device code in winoq_ring.hpp).
//
// In the default schedule (engine.choose_cfg_h8) these kernels run, in every exact-fp32
// forward, the level-0 convs that kind 14 (conv_winoc42.hip) does not take -- wino42_ok: input
// channels no multiple of 8 or below WINO42_MIN_CIN_L0, i.e. the 9- and 10-channel first convs
// of the final and refine U-Nets (kind 3) -- and every conv whose K the geometry rule splits
// (geom_split: the deep convs of small images such as 640x368 x 1; kind 4 with SK).  The ring
// fold is off by default (engine.RING_FOLD) and kept for A/B; a forced engine.WINO_KIND = 3
// runs every body conv here.
#include "wino_tile.hpp"
#include "winoq_ring.hpp"

// Diagnostic build only (tools/clock_probe.py --kernel winoq): per-workgroup s_memtime
// stamps after chunk 0 landed, at the end of the main loop and at the end, and the
// s_memrealtime span and start
#ifndef RRIN_WINOQ_CLOCK
#define RRIN_WINOQ_CLOCK 0
#endif

namespace rrin {

#if RRIN_WINOQ_CLOCK
constexpr int kQClkSlots = 1 << 16;
__device__ unsigned long long g_winoq_clk[kQClkSlots * 6];
#endif
// two stages of the 8-wave tile: raw 2 groups x 10 rows x 34 columns + U 1024 records
static_assert(kWinoQLds == (size_t)2 * (2 * 10 * kWnRawCols + kWnU) * 16, "LDS size");
static_assert(2 * kWinoQLds <= 160 * 1024, "two blocks per CU");

// ABL (lab builds only, librrin_lab.so): 1 no U DMA after chunk 0, 2 no raw DMA
// after chunk 0, 4 no MFMAs, 8 no transform arithmetic, 16 no window reads after
// chunk 0 (registers reused), 32 no U reads after chunk 0, 64 no epilogue stores
//
// PT: patch-row pairs per tile -- 2: 8 waves, TH 8 (cfg 20); 1: 4 waves, TH 4
// (cfg 21, twice the tiles for the few-tile deep levels of small workloads).
//
// SK (split-K, a.ksplit > 1): the grid has a.ksplit blocks per tile, slice ks running
// chunks [ks * a.kper, ..).  After its output transform a slice stores its pre-bias
// outputs (16 floats per lane) to a.part and counts itself in a.cnt[tile]
// (agent-scope release / acquire: the slices may run on different XCDs); the slice that
// counts last reads the tile's slices back, sums them in slice order (so the result
// does not depend on which slice finished last), resets the counter and runs the
// epilogue.  A different association of the K sum than one slice (not bitwise equal to
// cfg 20), fixed per conv: batch and per-sample outputs stay bitwise equal.
//
// RF (EPI_SUBPIXEL, PT 2, no split): the ring fold (winoq_ring.hpp) -- the first a.nring
// workgroups of the grid are ring correction blocks (ring_block), the rest the conv tiles; a
// tile on the image border stores its ring values write-through and counts itself in the
// ticket of each ring segment it covers (ring_combine by the later writer).
template <int EPI, int ABL = 0, int PT = 2, int SK = 0, int RF = 0>
__global__ __launch_bounds__(256 * PT, 2) void conv3x3_winoq_kernel(ConvH8Args a) {
  static_assert(!RF || (EPI == RRIN_EPI_SUBPIXEL && PT == 2 && !SK), "ring fold: 8-wave sub-pixel conv");
  constexpr int NT = 256 * PT, TH = 4 * PT;
  constexpr int RG = (TH + 2) * kWnRawCols, RAW = 2 * RG, STAGE = RAW + kWnU;
  static_assert(RAW > NT && RAW <= 2 * NT && kWnU % NT == 0, "two raw pieces, whole U pieces");
  constexpr int UP = kWnU / NT;  // U pieces per thread
  extern __shared__ __attribute__((aligned(16))) uint4 smem4[];
  // two stages of [raw RAW | U 1024] records
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int yw = wv & 3, pt = wv >> 2, j = lane & 31, hh = lane >> 5;
  // RF: groups of 8 ring blocks (one per XCD) at the head of every a.rstride workgroups,
  // so the dispatcher interleaves them with the tiles; the tiles' index space skips them
  int cidx = blockIdx.x;
  if constexpr (RF) {
    const int g = blockIdx.x / a.rstride, off = blockIdx.x - g * a.rstride, ng = a.nring >> 3;
    if (g < ng && off < 8) {
      const int rb = 8 * g + off;
      if (rb < a.n * a.co_blocks * a.nseg) ring_block(a, rb, reinterpret_cast<float*>(smem4));
      return;
    }
    cidx -= 8 * min(g + 1, ng);
  }
  const int bid = wino_xcd_bid((int)gridDim.x - (RF ? a.nring : 0), cidx);
  const int ntiles = a.co_blocks * a.tiles_x * a.tiles_y * a.n;
  const int ksn = SK ? a.ksplit : 1;  // K slices per tile
  if (bid >= ntiles * ksn) return;
  const int tile = SK ? bid / ksn : bid, ks = SK ? bid - tile * ksn : 0;
#if RRIN_WINOQ_CLOCK
  const unsigned long long qc_t0 = __builtin_amdgcn_s_memtime(), qc_r0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long qc_t1 = 0;
#endif
  // this slice's chunks [c0, c0 + nch) of the conv's a.nchunks; staging below counts chunks
  // from c0 (source and weight bases moved by c0 chunks, cin_loc channels from there)
  const int c0 = SK ? ks * a.kper : 0;
  const int nch = SK ? min(a.nchunks - c0, a.kper) : a.nchunks;
  const int cin_loc = a.cin - 8 * c0;
  // co-block groups (wino_tile_pos); an XCD runs consecutive workgroups, so with groups it
  // streams one group's U
  int cob, x0, y0, img;
  {
    const WinoTile p = wino_tile_pos(a, ntiles, tile, 32, TH);
    cob = p.cob, x0 = p.x0, y0 = p.y0, img = p.img;
  }
  const uint4* tsrc =
      a.src_hi + (int64_t)img * a.src_img + (int64_t)(2 * c0) * a.src_gp + (int64_t)y0 * a.src_wp + x0 + (kH8PadLeft - 1);
  const uint4* wsrc = a.w_hi + ((int64_t)cob * a.nchunks + c0) * kWnU + tid;
  // staging: raw RAW records = NT + the rest, U 1024 = UP x NT
  int64_t p_off[2];
  int p_g[2], p_zero[2];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int idx = tid + NT * it;
    const int g = idx >= RG ? 1 : 0;
    const int rem = idx - g * RG;
    const int r = rem / kWnRawCols, pos = rem - r * kWnRawCols;
    const int col = pos < 17 ? 2 * pos : 2 * (pos - 17) + 1;
    p_g[it] = g;
    p_off[it] = (int64_t)g * a.src_gp + r * a.src_wp + col;
    p_zero[it] = col - y0 * a.src_wp;
  }
  // LDS: stages [raw | U] x 2, chunk c in stage c & 1
  auto raw_stage = [&](int c) { return smem4 + (c & 1) * STAGE; };
  auto u_stage = [&](int c) { return smem4 + (c & 1) * STAGE + RAW; };
  auto issue_raw = [&](int c) {
    uint4* base = raw_stage(c);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      if ((it == 0 || tid < RAW - NT) && !((ABL & 2) && c > 0)) {
        const int gg = 2 * c + p_g[it];
        const int64_t off = gg * 4 < cin_loc ? (int64_t)(2 * c) * a.src_gp + p_off[it] : (int64_t)p_zero[it];
        dma16(tsrc + off, base + NT * it + (tid & ~63));
      }
    }
  };
  auto issue_u = [&](int c) {
    uint4* base = u_stage(c);
#pragma unroll
    for (int it = 0; it < UP; ++it)
      if (!((ABL & 1) && c > 0)) dma16(wsrc + (int64_t)c * kWnU + NT * it, base + NT * it + (tid & ~63));
  };
  auto issue = [&](int c) {
    issue_raw(c);
    issue_u(c);
  };
  const int pr = 2 * pt + (j >> 4), jx = (j + 12 * (j >> 4)) & 15;
  const int ra = yw == 0 ? 0 : (yw == 2 ? 2 : 1);
  const int rb = yw == 0 ? 2 : (yw == 1 ? 2 : (yw == 2 ? 1 : 3));
  const float sg = yw == 1 ? 1.f : -1.f;
  const int rw0 = hh * RG + (2 * pr) * kWnRawCols;
  const int oa = ra * kWnRawCols, ob = rb * kWnRawCols;
  int pc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) pc[k] = wino_col(2 * jx + k);
  const int su0 = (4 * yw) * 64 + hh * 32 + j;  // U of point 4 yw + x: + x * 64 (layout [xi][half][32 co])

  floatx16 acc[4];
  floatx4 dk[8], uk[4];  // ABL 16 / 32: chunk 0's reads kept
  // one chunk in its stage: window reads -> B^T row -> 4 points, then per point
  // its U record and 4 MFMAs (point-major, kind 1's accumulation order)
  auto chunk = [&](bool first, int c) {
    const uint4* rw = raw_stage(c) + rw0;
    floatx4 t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      floatx4 d0, d1;
      if (!(ABL & 16) || first) {
        d0 = __builtin_bit_cast(floatx4, rw[oa + pc[k]]);
        d1 = __builtin_bit_cast(floatx4, rw[ob + pc[k]]);
        if constexpr ((ABL & 16) != 0) dk[2 * k] = d0, dk[2 * k + 1] = d1;
      } else {
        d0 = dk[2 * k];
        d1 = dk[2 * k + 1];
      }
      if constexpr ((ABL & 8) != 0) {
        t[k] = d0;
        asm volatile("" ::"v"(d1));
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) t[k][e] = fmaf(sg, d1[e], d0[e]);
      }
    }
    floatx4 v[4];
    if constexpr ((ABL & 8) != 0) {
#pragma unroll
      for (int x = 0; x < 4; ++x) v[x] = t[x];
    } else {
      v[0] = t[0] - t[2];
      v[1] = t[1] + t[2];
      v[2] = t[2] - t[1];
      v[3] = t[1] - t[3];
    }
    const uint4* su = u_stage(c) + su0;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      floatx4 u;
      if (!(ABL & 32) || first) {
        u = __builtin_bit_cast(floatx4, su[x * 64]);
        if constexpr ((ABL & 32) != 0) uk[x] = u;
      } else {
        u = uk[x];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if constexpr ((ABL & 4) != 0) {
          asm volatile("" ::"v"(u[e]), "v"(v[x][e]));
        } else {
          const floatx16 cin_acc = (first && e == 0) ? floatx16{} : acc[x];
          acc[x] = __builtin_amdgcn_mfma_f32_32x32x2f32(u[e], v[x][e], cin_acc, 0, 0, 0);
        }
      }
    }
  };
  if constexpr ((ABL & 4) != 0) {
#pragma unroll
    for (int x = 0; x < 4; ++x) acc[x] = floatx16{};
  }
  issue(0);
  for (int c = 0; c < nch; ++c) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // chunk c landed everywhere; stage (c + 1) & 1 was last read in chunk c - 1
#if RRIN_WINOQ_CLOCK
    if (c == 0) qc_t1 = __builtin_amdgcn_s_memtime();
#endif
    if (c + 1 < nch) issue(c + 1);
    chunk(c == 0, c);
  }
#if RRIN_WINOQ_CLOCK
  const unsigned long long qc_t2 = __builtin_amdgcn_s_memtime();
#endif
  // every stage DMA has landed (the last chunk waited for it): said with a wait the
  // compiler sees, so that it does not drain vmcnt at the exchange barrier below for the
  // LDS-DMA it cannot see completed -- which would wait out the bias loads too
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  // the epilogue's bias values, loaded now: their latency hides behind the exchange
  // instead of stalling the stores (the bias blob is padded to whole 32-row blocks)
  float bsv[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) bsv[i] = a.bias[cob * 32 + 8 * (i >> 2) + 4 * hh + (i & 3)];
  __syncthreads();  // every read done before the exchange reuses the LDS

  // ---- output transform (one co tile): the four yw waves of a
  // patch-row pair exchange their Q[c] = sum_x M[x] A[x][c] through LDS, one
  // column c per pass; wave (yw, pt) finishes output row r = yw & 1 of column
  // cc = yw >> 1, Y[0] = (Q0 + Q1) + Q2, Y[1] = (Q1 - Q2) - Q3 (kind 1's order)
  floatx4* X = reinterpret_cast<floatx4*>(smem4);
  const int r = yw & 1, cc = yw >> 1;
  const int y = y0 + 2 * pr + r, x = x0 + 2 * jx + cc;
  uint4* dst = a.dst_hi + (int64_t)img * a.dst_img;
  auto store4 = [&](int64_t rec, const float* vv) {
    if constexpr ((ABL & 64) != 0) {
      asm volatile("" ::"v"(vv[0]), "v"(vv[1]), "v"(vv[2]), "v"(vv[3]));
      if (vv[0] != 12345.f) return;  // keeps the values live; never stores in practice
    }
    dst[rec] = make_uint4(__float_as_uint(vv[0]), __float_as_uint(vv[1]), __float_as_uint(vv[2]), __float_as_uint(vv[3]));
  };
  // two passes (column c = 0, 1): the Q records of one column are 32 KB
  float yv[16];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
#pragma unroll
    for (int k4 = 0; k4 < 4; ++k4) {
      floatx4 g;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = 4 * k4 + e;
        const float m0 = acc[0][i], m1 = acc[1][i], m2 = acc[2][i], m3 = acc[3][i];
        g[e] = p == 0 ? (m0 + m1) + m2 : (m1 - m2) - m3;
      }
      X[((pt * 4 + yw) * 4 + k4) * 64 + lane] = g;
    }
    __syncthreads();
    if (cc == p) {
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4) {
        const floatx4 q0 = X[((pt * 4 + 0) * 4 + k4) * 64 + lane];
        const floatx4 q1 = X[((pt * 4 + 1) * 4 + k4) * 64 + lane];
        const floatx4 q2 = X[((pt * 4 + 2) * 4 + k4) * 64 + lane];
        const floatx4 q3 = X[((pt * 4 + 3) * 4 + k4) * 64 + lane];
#pragma unroll
        for (int e = 0; e < 4; ++e) yv[4 * k4 + e] = r == 0 ? (q0[e] + q1[e]) + q2[e] : (q1[e] - q2[e]) - q3[e];
      }
    }
    __syncthreads();
  }
  if constexpr (SK) {
    // slice partial: plane q of the slice = NT lanes x 4 floats (coalesced per wave).
    // Split-K seam (cdna_hip_programming.md, split-K reduction recipe, sc1 form): the slice
    // drawing ksn - 1 reduces, reading every slab with sc1 loads.  Correct for any
    // placement of a tile's slices over CUs / XCDs.
    // The slab stores are write-through (sc1), so no release fence: every wave drains, the
    // barrier, then lane 0's relaxed ticket.
    {
      float* slab = a.part + (int64_t)(tile * ksn) * 4 * NT * 4;  // block-uniform base
      const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(slab, 0, ksn * 4 * NT * 16, 0x00020000);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 v = {__float_as_uint(yv[4 * q]), __float_as_uint(yv[4 * q + 1]), __float_as_uint(yv[4 * q + 2]),
                         __float_as_uint(yv[4 * q + 3])};
        __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, ((ks * 4 + q) * NT + tid) * 16, 0, 16 /* sc1 */);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // "last slice" flag in the dynamic LDS array (right past the exchange records: 2048 of TH 8, 1024 of TH 4)
    int* s_last = reinterpret_cast<int*>(smem4 + 2048);
    if (tid == 0) {
      const int old = __hip_atomic_fetch_add(a.cnt + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = old == ksn - 1;
      if (last) __hip_atomic_store(a.cnt + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // next launch
      *s_last = last;
    }
    __syncthreads();
    if (!*s_last) return;
    // the slabs are read with sc1 loads (no agent-scope acquire, which would drop this
    // CU's cached lines); the wavefront fence only keeps the loads below the ticket
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const auto srs = __builtin_amdgcn_make_buffer_rsrc(a.part + (int64_t)(tile * ksn) * 4 * NT * 4, 0,
                                                       ksn * 4 * NT * 16, 0x00020000);
    auto ld = [&](int k, int q) {
      typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(srs, ((k * 4 + q) * NT + tid) * 16, 0, 16);
      return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
    };
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float4 sum = ld(0, q);
      for (int k = 1; k < ksn; ++k) {
        const float4 v = ld(k, q);
        sum.x += v.x;
        sum.y += v.y;
        sum.z += v.z;
        sum.w += v.w;
      }
      yv[4 * q] = sum.x;
      yv[4 * q + 1] = sum.y;
      yv[4 * q + 2] = sum.z;
      yv[4 * q + 3] = sum.w;
    }
  }
  if constexpr (EPI == RRIN_EPI_SUBPIXEL) {
    const int HH = 2 * a.h, WW = 2 * a.w, creal = a.cout >> 2;
    if (cob * 32 < a.cout && y < a.h && x < a.w) {
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const int Y = 2 * y + (qq >> 1), XX = 2 * x + (qq & 1);
        const int64_t ri = ring_index(Y, XX, HH, WW);
        if (ri >= 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int64_t k = ((int64_t)img * creal + cob * 8 + 4 * hh + e) * a.ring + ri;
            if constexpr (RF) {  // write-through: the segment's other writer may combine it
              const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(a.edge, 0, 0x7fffffff, 0x00020000);
              __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(yv[4 * qq + e]), rsrc, (int)(k * 4), 0, 16);
            } else {
              a.edge[k] = yv[4 * qq + e];
            }
          }
        } else {
          float vv[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) vv[e] = yv[4 * qq + e] + bsv[4 * qq + e];
          store4((int64_t)(2 * cob + hh) * a.dst_gp + (int64_t)(Y + 1) * a.dst_wp + XX + kH8PadLeft, vv);
        }
      }
    }
    if constexpr (RF) {
      // the ring segments this tile writes (its tile column's top / bottom row, its tile
      // row's left / right column): one ticket each, the later writer combines
      const int tx = x0 >> 5, ty = y0 / TH;
      const bool on[4] = {ty == 0, ty == a.tiles_y - 1, tx == 0, tx == a.tiles_x - 1};
      if (on[0] || on[1] || on[2] || on[3]) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int* s_flag = reinterpret_cast<int*>(smem4 + 2048);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!on[k]) continue;
          const int seg = k == 0 ? tx : k == 1 ? a.tiles_x + tx : k == 2 ? 2 * a.tiles_x + ty : 2 * a.tiles_x + a.tiles_y + ty;
          const RingSeg rs = ring_seg(a, seg);
          if (rs.lo >= rs.hi) continue;  // empty column segment: no ring block counts it either
          if (ring_ticket(a, img, cob, seg, tid, s_flag)) ring_combine(a, img, cob, seg, tid);
        }
      }
    }
  } else {
    float vv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float tv = yv[i] + bsv[i];
      if constexpr (EPI != RRIN_EPI_LINEAR) tv = leaky(tv, a.slope);
      vv[i] = tv;
    }
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      if (cob * 32 + 8 * qq < a.cout && y < a.h && x < a.w) {
        const int64_t rec = (int64_t)(cob * 8 + 2 * qq + hh) * a.dst_gp + (int64_t)(y + 1) * a.dst_wp + x + kH8PadLeft;
        store4(rec, &vv[4 * qq]);
        if constexpr (EPI == RRIN_EPI_LEAKY_REP) {
          const int dy0 = y == 0 ? -1 : 0, dy1 = y == a.h - 1 ? 1 : 0;
          const int dx0 = x == 0 ? -1 : 0, dx1 = x == a.w - 1 ? 1 : 0;
          for (int dy = dy0; dy <= dy1; ++dy)
            for (int dx = dx0; dx <= dx1; ++dx)
              if (dy | dx) store4(rec + (int64_t)dy * a.dst_wp + dx, &vv[4 * qq]);
        }
      }
    }
    if constexpr (EPI == RRIN_EPI_LEAKY_POOL) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        floatx4 g;
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = vv[4 * k + e];
        X[((pt * 4 + yw) * 4 + k) * 64 + lane] = g;
      }
      __syncthreads();
      if (yw == 0) {
        const int xp = x0 + 2 * jx, yp = y0 + 2 * pr;
        uint4* pdst = a.pool_hi + (int64_t)img * a.pool_img;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
          const floatx4 y00 = X[((pt * 4 + 0) * 4 + qq) * 64 + lane];
          const floatx4 y10 = X[((pt * 4 + 1) * 4 + qq) * 64 + lane];
          const floatx4 y01 = X[((pt * 4 + 2) * 4 + qq) * 64 + lane];
          const floatx4 y11 = X[((pt * 4 + 3) * 4 + qq) * 64 + lane];
          if (cob * 32 + 8 * qq < a.cout && yp < a.h && xp < a.w) {
            float s4[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) s4[e] = 0.25f * ((y00[e] + y10[e]) + (y01[e] + y11[e]));
            const int64_t rec =
                (int64_t)(cob * 8 + 2 * qq + hh) * a.pool_gp + (int64_t)(yp / 2 + 1) * a.pool_wp + xp / 2 + kH8PadLeft;
            pdst[rec] = make_uint4(__float_as_uint(s4[0]), __float_as_uint(s4[1]), __float_as_uint(s4[2]),
                                   __float_as_uint(s4[3]));
          }
        }
      }
    }
  }
#if RRIN_WINOQ_CLOCK
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stores done
  const unsigned long long qc_t3 = __builtin_amdgcn_s_memtime(), qc_r3 = __builtin_amdgcn_s_memrealtime();
  if (tid == 0) {
    unsigned long long* g = g_winoq_clk + (size_t)(bid % kQClkSlots) * 6;
    g[0] = qc_t1 - qc_t0;  // core clocks until chunk 0 landed
    g[1] = qc_t2 - qc_t0;  // ... until the end of the main loop
    g[2] = qc_t3 - qc_t0;  // ... until the stores completed
    g[3] = qc_r3 - qc_r0;  // 100 MHz ticks, whole workgroup
    g[4] = qc_r0;          // start (100 MHz ticks)
    g[5] = qc_r3;          // end
  }
#endif
}

template <int EPI, int ABL = 0, int PT = 2, int SK = 0, int RF = 0>
static int launch_winoq_k(const ConvH8Args& a, hipStream_t st, rrin_launch_info* info = nullptr) {
  auto k = conv3x3_winoq_kernel<EPI, ABL, PT, SK, RF>;
  static LdsAttr attr;
  constexpr size_t lds = (size_t)2 * (2 * (4 * PT + 2) * kWnRawCols + kWnU) * 16;  // two [raw | U] stages
  if (int e = attr.ensure((const void*)k, (int)lds, st)) return e;
  const int64_t tiles = (int64_t)a.co_blocks * a.tiles_x * a.tiles_y * a.n * (SK ? a.ksplit : 1);
  const int64_t nring = RF ? a.nring : 0;  // ring correction blocks at the head of the grid
  if (info) return launch_report(info, tiles, tiles, nring, 0);
  hipLaunchKernelGGL(k, dim3((unsigned)(tiles + nring)), dim3(256 * PT), lds, st, a);
  return hip_code(hipGetLastError());
}

// Workgroup order of kinds 3 / 4: co-block groups (wino_cob_group) when the co blocks' U (nchunks x
// 16 KB each) exceeds RRIN_WINOQ_UGROUP_KB -- the deep split-K convs of small images read each U
// once per XCD otherwise.  Ring-folding launches keep their own index space.
#ifndef RRIN_WINOQ_UGROUP_KB
#define RRIN_WINOQ_UGROUP_KB 2048
#endif

template <int PT, int SK>
static int launch_winoq_e(const ConvH8Args& a, int epi, hipStream_t st, rrin_launch_info* info) {
  return wino_dispatch_epi(epi, [&](auto e) { return launch_winoq_k<decltype(e)::value, 0, PT, SK>(a, st, info); });
}

int launch_winoq(const ConvH8Args& a0, int epi, int th, hipStream_t st, rrin_launch_info* info) {
  ConvH8Args a = a0;
  a.cob_group =
      a.nring > 0 ? 0 : wino_cob_group(a.co_blocks, (int64_t)a.nchunks * kWnU * 16, RRIN_WINOQ_UGROUP_KB);
  if (a.ksplit > 1) return th == 4 ? launch_winoq_e<1, 1>(a, epi, st, info) : launch_winoq_e<2, 1>(a, epi, st, info);
  if (a.nring > 0) {
    if (th != 8 || epi != RRIN_EPI_SUBPIXEL) return RRIN_E_CONFIG;
    return launch_winoq_k<RRIN_EPI_SUBPIXEL, 0, 2, 0, 1>(a, st, info);
  }
  return th == 4 ? launch_winoq_e<1, 0>(a, epi, st, info) : launch_winoq_e<2, 0>(a, epi, st, info);
}

#ifdef RRIN_LAB
// kernel lab (librrin_lab.so only): the LEAKY conv with ablation bits -- 1024 + bits: the
// 8-wave tile (cfg 20); below 1024: kind 1's bits (conv_wino.hip)
int launch_wino_lab(const ConvH8Args& a, int abl, hipStream_t st) {
  switch (abl) {
    case 1024 + 0: return launch_winoq_k<RRIN_EPI_LEAKY, 0>(a, st);
    case 1024 + 3: return launch_winoq_k<RRIN_EPI_LEAKY, 3>(a, st);
    case 1024 + 4: return launch_winoq_k<RRIN_EPI_LEAKY, 4>(a, st);
    case 1024 + 8: return launch_winoq_k<RRIN_EPI_LEAKY, 8>(a, st);
    case 1024 + 16: return launch_winoq_k<RRIN_EPI_LEAKY, 16>(a, st);
    case 1024 + 32: return launch_winoq_k<RRIN_EPI_LEAKY, 32>(a, st);
    case 1024 + 48: return launch_winoq_k<RRIN_EPI_LEAKY, 48>(a, st);
    case 1024 + 56: return launch_winoq_k<RRIN_EPI_LEAKY, 56>(a, st);
    case 1024 + 59: return launch_winoq_k<RRIN_EPI_LEAKY, 59>(a, st);
    case 1024 + 64: return launch_winoq_k<RRIN_EPI_LEAKY, 64>(a, st);
    case 1024 + 123: return launch_winoq_k<RRIN_EPI_LEAKY, 123>(a, st);
  }
  return launch_wino_lab1(a, abl, st);
}
#endif

}  // namespace rrin

using namespace rrin;

#if RRIN_WINOQ_CLOCK
// diagnostic builds only: copy n workgroup stamps (6 x u64 each) to host memory
extern "C" int rrin_winoq_clock_read(unsigned long long* host, int n) {
  if (!host || n < 1 || n > rrin::kQClkSlots) return RRIN_E_ARG;
  return rrin::hip_code(hipMemcpyFromSymbol(host, HIP_SYMBOL(rrin::g_winoq_clk), (size_t)n * 6 * 8, 0,
                                            hipMemcpyDeviceToHost));
}
#endif
