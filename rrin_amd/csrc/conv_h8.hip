// Direct-form 3x3 conv on the record layouts (h8.hpp) at all three record precisions, on the
// gfx950 matrix cores: split-fp16 ("F16X3") and fp16 ("F16") on v_mfma_f32_32x32x16_f16, exact
// fp32 ("F32R") on v_mfma_f32_32x32x2_f32, fp32 accumulate: the kernel, its launch templates and
// the host entry launch_h8.  The tiles are the direct-form rows of the config table (h8_cfg.hpp);
// descriptor validation and rrin_conv3x3_h8_fwd are in conv_rec.hip.
//
// Numerics (F16X3): every fp32 value v lives as hi = f16(v) and a pre-scaled
// lo' = f16((v - hi) * 2^11), so v = hi + lo' 2^-11 to ~2^-22 |v| and lo' stays
// a normal fp16 down to |v| ~ 1e-4.  A product a*w is computed as
// a_hi*w_hi (accumulator acc) + (a_hi*w_lo' + a_lo'*w_hi) (accumulator accx,
// scaled back by 2^-11 in the epilogue) — every term exact in fp32 — with fp32
// accumulation in the MFMA; the dropped lo*lo term is <= 2^-22 |a w|.
// Weights are pre-scaled by 2^s (exact), max |w| 2^s in [2^12, 2^13); the
// epilogue multiplies by 2^-s.  F16 keeps hi only (fp16 configs).
//
// Replaces (as conv_mfma.hip): nn.Conv2d(3,pad=1) + LeakyReLU(0.1)
// (unet.py:29,59-63,78), F.avg_pool2d (unet.py:46, fused second output), torch.cat (unet.py:93, channel-offset views).  The non-conv passes of the record
// path (upsample, layout, heads + model.py glue) are in glue_h8.hip, the host-side weight
// packing in pack_h8.hip.
#include <type_traits>

#include "edge_fix.hpp"
#include "h8_cfg.hpp"

namespace rrin {

// Schedule knobs of the kernel (template SCHED, the SCHED_* bits of h8_cfg.hpp; the cfg table picks
// them per layer, tools/conv_lab.py ablate times them).  SPREAD issues the next chunk's
// DMA pieces between the first kSpreadTaps taps of the current chunk instead
// of in one burst before it; STAGGER lets waves NW/2.. issue theirs after tap
// kStaggerTap instead (the two wave halves of a SIMD then load at different
// times); WRES keeps every weight chunk of the block's channel block resident
// in LDS, staged once per block.  Lab-only ablations (wrong outputs, they time
// what is left): NO_WDMA / NO_IDMA keep reading the chunk-0 weight slab /
// input tile instead of staging later chunks, NO_MFMA keeps the LDS operand
// reads but drops the MFMAs, NO_EPI drops the epilogue; MFMA16 issues every
// 32x32x16 product as two v_mfma_f32_16x16x32_f16 of the same FLOPs on the
// same operands (a clock/throughput probe of the other MFMA shape).
// Epilogue bias of the record kernel: 0 = each epilogue piece loads its 4 bias floats
// just before its stores (then waits out every earlier store of the tile: vmcnt counts
// stores too); 1 = every piece's bias loaded at the start of the epilogue (one wait);
// 2 = loaded at the start of the tile, landed during the chunk loop (no wait, but 16 WM
// more VGPRs live across it).  -1 (default): per tile shape, as measured at C3 fp16
// (profiles/r04/h8_bias/): 2 where the accumulators are small (WM WN <= 2: the level-0
// and level-4 tiles, 6-14 % faster per conv), 1 on the other unspread tiles (cfg 0 -8 %,
// cfg 5 -3 %), 0 on the SPREAD tiles (cfg 10 / 11, which lose 1-7 % with either).
#ifndef RRIN_H8_WIDE
#define RRIN_H8_WIDE 1
#endif
#ifndef RRIN_H8_BIAS
#define RRIN_H8_BIAS -1
#endif

constexpr int kSpreadTaps = 6, kStaggerTap = 3;

// DMA = true: stage with LDS-DMA (requires cin % 8 == 0: no partial channel
// group to mask); false: register staging with masking (first convs, cin 6/9/10).
//
// A block computes the output tiles (BM channels x TH rows x 32 columns of one
// image, channel block fastest) bid, bid + gridDim.x, ...  With a grid of every
// tile that is one tile per block; with a persistent grid (a few blocks per
// CU) chunk 0 of a block's next tile is staged while the last chunk of the
// current one computes, so only its first tile waits for staging.  WRES needs
// every tile of a block in one channel block (gridDim.x % co_blocks == 0).
//
// F32 (exact fp32, "R32" records): a record holds 4 fp32 channels, a chunk is
// 2 groups = 8 input channels, and each tap's K8 block is 4
// v_mfma_f32_32x32x2_f32 (product e: lanes 0-31 channel e, lanes 32-63 channel
// 4+e of the chunk; one ds_read_b128 per operand feeds all 4).  Same tiles,
// LDS images and DMA as the fp16 kernel; weights unscaled; whole-record stores.
template <int NW, int WM, int WN, int PLANES, int EPI, bool DMA, int SCHED = 0, bool F32 = false>
__global__ void RRIN_PK_CONV_ATTR __launch_bounds__(64 * NW) conv3x3_h8_kernel(ConvH8Args a) {
  using T = TileH8<NW, WM, WN, PLANES>;
  // EPI_SUBPIXEL with the ring from scratch in this launch: workgroups [0, nfix) run the FULL
  // fix-up -- one ring tile per 256-thread slice, one K group each (the summation order of every
  // ring_full conv whatever its tile, so the outputs do not depend on the config) -- and leave;
  // the conv tiles follow
  if constexpr (EPI == RRIN_EPI_SUBPIXEL && NW >= 4) {
    if ((int)blockIdx.x < a.nfix) {
      const int vg = threadIdx.x >> 8;
      const int r = (int)blockIdx.x * (NW / 4) + vg;
      const bool act = r < a.fix_real;
      const int rr = act ? r : 0;
      edge_fix_body<PLANES, 1, F32, true>(a.fix, rr % a.fix_gx, (rr / a.fix_gx) % a.fix_gy, rr / (a.fix_gx * a.fix_gy),
                                          vg, act);
      return;
    }
  }
  const int cgrid = (int)gridDim.x - a.nfix, cblk = (int)blockIdx.x - a.nfix;  // the conv's part of the grid
  static_assert(!F32 || PLANES == 1, "fp32 records: one plane");
  constexpr int CPR = F32 ? 4 : 8;  // channels per record
  constexpr int NT = T::NT, BM = T::BM, TH = T::TH, ROWS = T::ROWS;
  constexpr int IN_REC = T::IN_REC, W_REC = T::W_REC;
  constexpr bool kNoW = (SCHED & SCHED_NO_WDMA) != 0, kNoIn = (SCHED & SCHED_NO_IDMA) != 0;
  constexpr bool kNoMfma = (SCHED & SCHED_NO_MFMA) != 0, kNoEpi = (SCHED & SCHED_NO_EPI) != 0;
  constexpr bool kSpread = DMA && (SCHED & SCHED_SPREAD) != 0;
  constexpr bool kStagger = DMA && !kSpread && (SCHED & SCHED_STAGGER) != 0 && NW >= 2;
  constexpr bool kWRes = DMA && (SCHED & SCHED_WRES) != 0;
  constexpr bool kMfma16 = (SCHED & SCHED_MFMA16) != 0;
  constexpr int kBias = RRIN_H8_BIAS >= 0 ? RRIN_H8_BIAS : (WM * WN <= 2 ? 2 : (SCHED & SCHED_SPREAD) ? 0 : 1);
  // whole-record epilogue stores on H8 records (epi_pair; RRIN_H8_WIDE=0: per-piece half-records)
  constexpr bool kWide = RRIN_H8_WIDE && !F32 && EPI != RRIN_EPI_SUBPIXEL;
  // DMA pieces (one 16-B record per thread and plane) of one chunk: input tile, then weight slab
  constexpr int NPIECE = T::IN_IT + (kWRes ? 0 : T::W_IT);

  extern __shared__ __attribute__((aligned(16))) uint4 smem4[];
  uint4* s_in = smem4;                          // [buf][plane][IN_REC]
  uint4* s_w = smem4 + 2 * PLANES * IN_REC;     // [buf][plane][W_REC]; WRES: [chunk][plane][W_REC]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wn = tid >> 6;  // waves stacked along output rows
  const int j = lane & 31;
  const int hh = lane >> 5;

  int bid;
  {  // XCD-aware bijective remap (see conv_mfma.hip); nfix is a multiple of 8
    const int nwg = cgrid, q = nwg >> 3, r = nwg & 7;
    const int xcd = cblk & 7, slot = cblk >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
  }
  const int ntiles = a.co_blocks * a.tiles_x * a.tiles_y * a.n;
  struct TileId {
    int cob, x0, y0, img;
  };
  auto tile_id = [&](int t) {
    TileId o;
    o.cob = t % a.co_blocks;
    t /= a.co_blocks;
    o.x0 = (t % a.tiles_x) * 32;
    t /= a.tiles_x;
    o.y0 = (t % a.tiles_y) * TH;
    o.img = t / a.tiles_y;
    return o;
  };

  uint4 rin[PLANES][DMA ? 1 : T::IN_IT];
  uint4 rw[PLANES][DMA ? 1 : T::W_IT];

  // LDS-DMA staging of chunk c of tile tl: input piece `it` into buffer buf,
  // weight piece `it` into weight slot `slot` (both planes).  buffer_load ... lds from a
  // per-chunk base (scalar arithmetic) at a per-lane byte offset computed once per kernel:
  // no vector address arithmetic in the chunk loop (it cost ~80 VALU per chunk beside 36
  // MFMAs on the SPREAD tiles, each VALU stalling the MFMA pipe -- DESIGN.md §5e)
  uint32_t in_off[DMA ? T::IN_IT : 1], in_zoff[DMA ? T::IN_IT : 1];
  if constexpr (DMA) {
#pragma unroll
    for (int it = 0; it < T::IN_IT; ++it) {
      const int idx = min(tid + NT * it, IN_REC - 1);
      const int g = idx / (ROWS * H8_LC);
      const int rem = idx - g * (ROWS * H8_LC);
      const int r = rem / H8_LC;
      const int col = rem - r * H8_LC;
      in_off[it] = (uint32_t)(g * a.src_gp + r * a.src_wp + col) * 16u;
      in_zoff[it] = (uint32_t)col * 16u;  // the zero top-padding row of group 0 (groups past cin)
    }
  }
  auto dma_rs = [&](const void* base, uint32_t voff, int soff, uint4* d) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7fffffff, 0x00020000),
        (__attribute__((address_space(3))) void*)d, 16, voff, soff, 0, 0);
  };
  auto issue_in = [&](const TileId& tl, int c, int buf, int it) {
    // (a full piece needs no lane test: the condition folds for every piece but the last)
    if (NT * (it + 1) <= IN_REC || tid + NT * it < IN_REC) {
      uint4* d = s_in + buf * PLANES * IN_REC + NT * it + (tid & ~63);
      // one base per tile (scalar); the chunk's group pair and the tile row in the lane offset
      const int64_t tb = (int64_t)tl.img * a.src_img + tl.x0 + (kH8PadLeft - 1);
      const uint32_t c0 = (uint32_t)(2 * c) * (uint32_t)a.src_gp * 16u;
      uint32_t vo = in_off[it] + c0 + (uint32_t)tl.y0 * (uint32_t)a.src_wp * 16u;
      // the chunk's second group past cin: its lanes read the zero top-padding row of the
      // chunk's first group instead (uniform test; a select only in that chunk)
      if ((2 * c + 1) * CPR >= a.cin && tid + NT * it >= ROWS * H8_LC) vo = c0 + in_zoff[it];
      dma_rs(a.src_hi + tb, vo, 0, d);
      if constexpr (PLANES == 2) dma_rs(a.src_lo + tb, vo, 0, d + IN_REC);
    }
  };
  auto issue_w = [&](const TileId& tl, int c, int slot, int it) {
    if (NT * (it + 1) <= W_REC || tid + NT * it < W_REC) {
      const int64_t off = ((int64_t)tl.cob * a.nchunks + c) * W_REC;
      uint4* d = s_w + slot * PLANES * W_REC + NT * it + (tid & ~63);
      dma_rs(a.w_hi + off, (uint32_t)tid * 16u, NT * it * 16, d);
      if constexpr (PLANES == 2) dma_rs(a.w_lo + off, (uint32_t)tid * 16u, NT * it * 16, d + W_REC);
    }
  };
  auto issue_piece = [&](const TileId& tl, int c, int buf, int k) {
    if (k < T::IN_IT) {
      if constexpr (!kNoIn) issue_in(tl, c, buf, k);
    } else {
      if constexpr (!kNoW) issue_w(tl, c, buf, k - T::IN_IT);
    }
  };

  auto load_in = [&](const TileId& tl, int c) {
    const uint4* src[2] = {a.src_hi, a.src_lo};
#pragma unroll
    for (int it = 0; it < T::IN_IT; ++it) {
      const int idx = tid + NT * it;
      if (idx < IN_REC) {
        const int g = idx / (ROWS * H8_LC);
        const int rem = idx - g * (ROWS * H8_LC);
        const int r = rem / H8_LC;
        const int col = rem - r * H8_LC;
        const int gg = c * 2 + g;
        const int nval = a.cin - gg * CPR;
        const int64_t off = (int64_t)tl.img * a.src_img + (int64_t)gg * a.src_gp + (int64_t)(tl.y0 + r) * a.src_wp +
                            tl.x0 + (kH8PadLeft - 1) + col;
#pragma unroll
        for (int p = 0; p < PLANES; ++p) {
          uint4 v = make_uint4(0u, 0u, 0u, 0u);
          if (nval > 0) {
            v = src[p][off];
            if (nval < CPR) v = F32 ? mask_floats(v, nval) : mask_halves(v, nval);
          }
          rin[p][it] = v;
        }
      }
    }
  };
  auto store_in = [&](int buf) {
#pragma unroll
    for (int p = 0; p < PLANES; ++p)
#pragma unroll
      for (int it = 0; it < T::IN_IT; ++it) {
        const int idx = tid + NT * it;
        if (idx < IN_REC) s_in[(buf * PLANES + p) * IN_REC + idx] = rin[p][it];
      }
  };
  auto load_w = [&](const TileId& tl, int c) {
    const uint4* wsrc[2] = {a.w_hi, a.w_lo};
#pragma unroll
    for (int p = 0; p < PLANES; ++p)
#pragma unroll
      for (int it = 0; it < T::W_IT; ++it) {
        const int idx = tid + NT * it;
        if (idx < W_REC) rw[p][it] = wsrc[p][((int64_t)tl.cob * a.nchunks + c) * W_REC + idx];
      }
  };
  auto store_w = [&](int buf) {
#pragma unroll
    for (int p = 0; p < PLANES; ++p)
#pragma unroll
      for (int it = 0; it < T::W_IT; ++it) {
        const int idx = tid + NT * it;
        if (idx < W_REC) s_w[(buf * PLANES + p) * W_REC + idx] = rw[p][it];
      }
  };

  // acc: hi*hi products; accx (F16X3): hi*lo' + lo'*hi, 2^11 too large
  floatx16 acc[WM][WN], accx[WM][WN];
  floatx4 p16[kMfma16 ? WM : 1][kMfma16 ? WN : 1][2][PLANES];  // MFMA16 probe accumulators

  // 9 taps per chunk; one K16 block = 16 input channels at one tap (lanes
  // 0-31 carry channels 0-7 of the chunk, lanes 32-63 channels 8-15).
  // Operands of tap t+1 are read before the MFMAs of tap t issue; after_tap(t)
  // runs behind tap t's MFMAs (SPREAD / STAGGER: DMA pieces of the next chunk).
  // zc (std::true_type for the tile's first chunk): the first MFMA of each accumulator takes C = 0,
  // so a tile starts without zeroing its accumulator registers
  auto compute_f32 = [&](int buf, int wslot, auto&& after_tap, auto zc) {
    const uint4* si = s_in + (kNoIn ? 0 : buf) * IN_REC + (hh * ROWS + wn * WN) * H8_LC + j;
    const uint4* sw = s_w + (kNoW ? 0 : wslot) * W_REC + hh * BM + j;
    floatx4 av[2][WM], bv[2][WN];
    auto ld = [&](int t, int slot) {
      const int ky = t / 3, kx = t % 3;
#pragma unroll
      for (int mt = 0; mt < WM; ++mt) av[slot][mt] = __builtin_bit_cast(floatx4, sw[t * 2 * BM + mt * 32]);
#pragma unroll
      for (int nt = 0; nt < WN; ++nt) bv[slot][nt] = __builtin_bit_cast(floatx4, si[(nt + ky) * H8_LC + kx]);
    };
    ld(0, 0);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      if (t + 1 < 9) ld(t + 1, (t + 1) & 1);
      const int s = t & 1;
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int mt = 0; mt < WM; ++mt)
#pragma unroll
          for (int nt = 0; nt < WN; ++nt) {
            if constexpr (kNoMfma)
              asm volatile("" ::"v"(av[s][mt][e]), "v"(bv[s][nt][e]));
            else
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                  av[s][mt][e], bv[s][nt][e], decltype(zc)::value && t == 0 && e == 0 ? floatx16{} : acc[mt][nt], 0, 0, 0);
          }
      after_tap(t);
    }
  };
  auto compute = [&](int buf, int wslot, auto&& after_tap, auto zc) {
    if constexpr (F32) {
      compute_f32(buf, wslot, after_tap, zc);
      return;
    }
    constexpr bool kZc = decltype(zc)::value;
    const uint4* si[PLANES];
    const uint4* sw[PLANES];
#pragma unroll
    for (int p = 0; p < PLANES; ++p) {
      si[p] = s_in + ((kNoIn ? 0 : buf) * PLANES + p) * IN_REC + (hh * ROWS + wn * WN) * H8_LC + j;
      sw[p] = s_w + ((kNoW ? 0 : wslot) * PLANES + p) * W_REC + hh * BM + j;
    }
    half8 av[2][PLANES][WM], bv[2][PLANES][WN];
    auto ld = [&](int t, int slot) {
      const int ky = t / 3, kx = t % 3;
#pragma unroll
      for (int p = 0; p < PLANES; ++p) {
#pragma unroll
        for (int mt = 0; mt < WM; ++mt) av[slot][p][mt] = __builtin_bit_cast(half8, sw[p][t * 2 * BM + mt * 32]);
#pragma unroll
        for (int nt = 0; nt < WN; ++nt) bv[slot][p][nt] = __builtin_bit_cast(half8, si[p][(nt + ky) * H8_LC + kx]);
      }
    };
    ld(0, 0);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      if (t + 1 < 9) ld(t + 1, (t + 1) & 1);
      const int s = t & 1;
#pragma unroll
      for (int mt = 0; mt < WM; ++mt)
#pragma unroll
        for (int nt = 0; nt < WN; ++nt) {
          if constexpr (kNoMfma) {
            asm volatile("" ::"v"(av[s][0][mt]), "v"(bv[s][0][nt]));
            if constexpr (PLANES == 2) asm volatile("" ::"v"(av[s][1][mt]), "v"(bv[s][1][nt]));
          } else if constexpr (kMfma16) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
              if constexpr (PLANES == 2) {
                p16[mt][nt][u][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[s][1][mt], bv[s][0][nt],
                                                                           p16[mt][nt][u][1], 0, 0, 0);
                p16[mt][nt][u][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[s][0][mt], bv[s][1][nt],
                                                                           p16[mt][nt][u][1], 0, 0, 0);
              }
              p16[mt][nt][u][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[s][0][mt], bv[s][0][nt],
                                                                         p16[mt][nt][u][0], 0, 0, 0);
            }
          } else {
            if constexpr (PLANES == 2) {
              accx[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[s][1][mt], bv[s][0][nt],
                                                                   kZc && t == 0 ? floatx16{} : accx[mt][nt], 0, 0, 0);
              accx[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[s][0][mt], bv[s][1][nt], accx[mt][nt], 0, 0, 0);
            }
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[s][0][mt], bv[s][0][nt],
                                                                kZc && t == 0 ? floatx16{} : acc[mt][nt], 0, 0, 0);
          }
        }
      after_tap(t);
    }
  };

  // fp16 range guard of the stored values, accumulated per lane over the workgroup's tiles and
  // written once at its end (one conditional store instead of one per epilogue piece)
  bool bad = false;
  // ---- epilogue piece (mt, q) of tile tl: V = the combined accumulators
  // (acc + accx 2^-11, weight scale still applied): scale, bias, leaky, split,
  // 8-B half-record stores (+ pool / edge-replicate / sub-pixel ring scratch).
  // 4 consecutive channels of one pixel (lane hh's share of record co0/8, or
  // the whole fp32 record co0/4 + hh) -> record `rec` of the group plane set `d`
  auto store4 = [&](uint4* const* d, int64_t rec, const float* v) {
    if constexpr (F32) {
      d[0][rec] = make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]),
                             __float_as_uint(v[3]));
    } else {
      // fp16 range guard: a value fp16 cannot hold would become inf / NaN and
      // could end as a finite but wrong pixel (e.g. a warp of an inf flow
      // samples zeros); flag it (the FINAL head then poisons the output)
      bad |= !(fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))) <= kF16Max);
      uint2 hv, lv;
      split4(v, hv, lv);
      reinterpret_cast<uint2*>(d[0] + rec)[hh] = hv;
      if constexpr (PLANES == 2) reinterpret_cast<uint2*>(d[1] + rec)[hh] = lv;
    }
  };
  auto epi_piece = [&](const TileId& tl, const auto& V, int mt, int q, const float* bs) {
    const int cob = tl.cob, x0 = tl.x0, img = tl.img;
    const int yb = tl.y0 + wn * WN;
    const int x = x0 + j;
    uint4* dst[2] = {a.dst_hi + img * a.dst_img, PLANES == 2 ? a.dst_lo + img * a.dst_img : nullptr};
    if constexpr (EPI == RRIN_EPI_SUBPIXEL) {
      // rows co' = (co/8)*32 + phase*8 + co%8: an MFMA row block (mt) is one
      // 8-channel group, q its phase (py, px); LR pixel (y, x) -> HR (2y+py, 2x+px)
      const int HH = 2 * a.h, WW = 2 * a.w, creal = a.cout >> 2;
      const int grp = (cob * BM + mt * 32) >> 5;
      if (grp * 32 >= a.cout) return;
      const int py = q >> 1, px = q & 1;
#pragma unroll
      for (int nt = 0; nt < WN; ++nt) {
        const int y = yb + nt;
        if (y >= a.h || x >= a.w) continue;
        const int Y = 2 * y + py, X = 2 * x + px;
        float t[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = F32 ? V[mt][nt][4 * q + e] : V[mt][nt][4 * q + e] * a.inv_wscale;
        const int64_t ri = ring_index(Y, X, HH, WW);
        if (ri >= 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) a.edge[((int64_t)img * creal + grp * 8 + 4 * hh + e) * a.ring + ri] = t[e];
        } else {
          const int rg = F32 ? 2 * grp + hh : grp;  // record group of channels grp*8 + 4hh ..
          const int64_t rec = (int64_t)rg * a.dst_gp + (int64_t)(Y + 1) * a.dst_wp + X + kH8PadLeft;
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = t[e] + bs[e];
          store4(dst, rec, v);
        }
      }
    } else {
      uint4* pdst[2] = {nullptr, nullptr};
      if constexpr (EPI == RRIN_EPI_LEAKY_POOL) {
        pdst[0] = a.pool_hi + img * a.pool_img;
        if (PLANES == 2) pdst[1] = a.pool_lo + img * a.pool_img;
      }
      const int co0 = cob * BM + mt * 32 + 8 * q;  // first channel of the 8-channel block
      const int grp = F32 ? (co0 >> 2) + hh : co0 >> 3;  // record group this lane writes
      float v[WN][4];
#pragma unroll
      for (int nt = 0; nt < WN; ++nt) {
        const int y = yb + nt;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float t = V[mt][nt][4 * q + e];
          t = F32 ? t + bs[e] : t * a.inv_wscale + bs[e];
          if constexpr (EPI != RRIN_EPI_LINEAR) t = leaky(t, a.slope);
          v[nt][e] = t;
        }
        if (co0 < a.cout && y < a.h && x < a.w) {
          const int64_t rec = (int64_t)grp * a.dst_gp + (int64_t)(y + 1) * a.dst_wp + x + kH8PadLeft;
          store4(dst, rec, v[nt]);
          if constexpr (EPI == RRIN_EPI_LEAKY_REP) {
            // edge replicate into the padding ring (read only by a sub-pixel up conv)
            const int dy0 = y == 0 ? -1 : 0, dy1 = y == a.h - 1 ? 1 : 0;
            const int dx0 = x == 0 ? -1 : 0, dx1 = x == a.w - 1 ? 1 : 0;
            for (int dy = dy0; dy <= dy1; ++dy)
              for (int dx = dx0; dx <= dx1; ++dx)
                if (dy | dx) store4(dst, rec + (int64_t)dy * a.dst_wp + dx, v[nt]);
          }
        }
      }
      if constexpr (EPI == RRIN_EPI_LEAKY_POOL) {
#pragma unroll
        for (int p2 = 0; p2 < WN / 2; ++p2) {
          float s4[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float s = v[2 * p2][e] + v[2 * p2 + 1][e];
            s4[e] = 0.25f * (s + __shfl_xor(s, 1));
          }
          const int y = yb + 2 * p2;
          if (!(j & 1) && co0 < a.cout && y < a.h && x < a.w) {
            const int64_t rec = (int64_t)grp * a.pool_gp + (int64_t)(y / 2 + 1) * a.pool_wp + x / 2 + kH8PadLeft;
            store4(pdst, rec, s4);
          }
        }
      }
    }
  };
  // ---- epilogue pieces (mt, 2 qp) and (mt, 2 qp + 1) together, H8 records (kWide): each lane
  // forms its two 8-B half-records, halves_to_record (v_permlane32_swap) turns them into one whole
  // 16-B record -- lane (j, hh) stores 8-channel block 2 qp + hh of its pixel -- and the wave
  // stores whole records: half the store instructions of epi_piece, the same bytes and bits.
  // (Not the sub-pixel epilogue: its ring pixels go to the fp32 edge scratch per channel.)
  auto epi_pair = [&](const TileId& tl, const auto& V, int mt, int qp, const float* bs0, const float* bs1) {
    const int cob = tl.cob, x0 = tl.x0, img = tl.img;
    const int yb = tl.y0 + wn * WN;
    const int x = x0 + j;
    uint4* dst[2] = {a.dst_hi + img * a.dst_img, PLANES == 2 ? a.dst_lo + img * a.dst_img : nullptr};
    const int cq0 = cob * BM + mt * 32 + 16 * qp;  // first channel of block 2 qp
    const int col = cq0 + 8 * hh;                  // first channel of the block this lane stores
    float v[2][WN][4];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int nt = 0; nt < WN; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float t = V[mt][nt][4 * (2 * qp + k) + e];
          t = t * a.inv_wscale + (k ? bs1 : bs0)[e];
          if constexpr (EPI != RRIN_EPI_LINEAR) t = leaky(t, a.slope);
          v[k][nt][e] = t;
        }
    // range guard on each lane's own values (as store4: only where that block is stored)
    auto guard = [&](const float* u) {
      bad |= !(fmaxf(fmaxf(fabsf(u[0]), fabsf(u[1])), fmaxf(fabsf(u[2]), fabsf(u[3]))) <= kF16Max);
    };
    auto store_rec = [&](uint4* const* d, int64_t rec, const uint4* r) {
      d[0][rec] = r[0];
      if constexpr (PLANES == 2) d[1][rec] = r[1];
    };
    // both blocks' halves -> this lane's whole record (hi, and lo for two planes)
    auto records = [&](const float* u0, const float* u1, uint4* r) {
      uint2 h0, l0, h1, l1;
      split4(u0, h0, l0);
      split4(u1, h1, l1);
      r[0] = halves_to_record(h0, h1);
      if constexpr (PLANES == 2) r[1] = halves_to_record(l0, l1);
    };
#pragma unroll
    for (int nt = 0; nt < WN; ++nt) {
      const int y = yb + nt;
      const bool pix = y < a.h && x < a.w;
#pragma unroll
      for (int k = 0; k < 2; ++k)
        if (pix && cq0 + 8 * k < a.cout) guard(v[k][nt]);
      uint4 r[2];
      records(v[0][nt], v[1][nt], r);  // every lane: the swap reads the partner lane
      if (pix && col < a.cout) {
        const int64_t rec = (int64_t)(col >> 3) * a.dst_gp + (int64_t)(y + 1) * a.dst_wp + x + kH8PadLeft;
        store_rec(dst, rec, r);
        if constexpr (EPI == RRIN_EPI_LEAKY_REP) {
          // edge replicate into the padding ring (read only by a sub-pixel up conv)
          const int dy0 = y == 0 ? -1 : 0, dy1 = y == a.h - 1 ? 1 : 0;
          const int dx0 = x == 0 ? -1 : 0, dx1 = x == a.w - 1 ? 1 : 0;
          for (int dy = dy0; dy <= dy1; ++dy)
            for (int dx = dx0; dx <= dx1; ++dx)
              if (dy | dx) store_rec(dst, rec + (int64_t)dy * a.dst_wp + dx, r);
        }
      }
    }
    if constexpr (EPI == RRIN_EPI_LEAKY_POOL) {
      uint4* pdst[2] = {a.pool_hi + img * a.pool_img, PLANES == 2 ? a.pool_lo + img * a.pool_img : nullptr};
#pragma unroll
      for (int p2 = 0; p2 < WN / 2; ++p2) {
        float s4[2][4];
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float s = v[k][2 * p2][e] + v[k][2 * p2 + 1][e];
            s4[k][e] = 0.25f * (s + __shfl_xor(s, 1));
          }
        const int y = yb + 2 * p2;
        const bool pix = !(j & 1) && y < a.h && x < a.w;
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (pix && cq0 + 8 * k < a.cout) guard(s4[k]);
        uint4 r[2];
        records(s4[0], s4[1], r);
        if (pix && col < a.cout)
          store_rec(pdst, (int64_t)(col >> 3) * a.pool_gp + (int64_t)(y / 2 + 1) * a.pool_wp + x / 2 + kH8PadLeft, r);
      }
    }
  };
  // combined accumulators: V = acc + accx 2^-11 (F16X3), V = acc (F16)
  auto combine = [&](floatx16 (&V)[WM][WN]) {
#pragma unroll
    for (int mt = 0; mt < WM; ++mt)
#pragma unroll
      for (int nt = 0; nt < WN; ++nt)
#pragma unroll
        for (int i = 0; i < 16; ++i)
          V[mt][nt][i] = PLANES == 2 ? fmaf(accx[mt][nt][i], kLoUnscale, acc[mt][nt][i]) : acc[mt][nt][i];
  };
  constexpr int NPIECE_EPI = WM * 4;
  // bias of epilogue piece (mt, q): channels co0 + 4hh .. co0 + 4hh + 3 of lane half hh,
  // co0 = cob BM + 32 mt + 8 q (pieces past cout store nothing: their bias stays 0)
  auto load_bias_piece = [&](int cob, int mt, int q, float* bq) {
    const int co0 = cob * BM + mt * 32 + 8 * q;
#pragma unroll
    for (int e = 0; e < 4; ++e) bq[e] = co0 < a.cout ? a.bias[co0 + 4 * hh + e] : 0.f;
  };
  float bsv[kBias ? WM : 1][4][4];
  auto load_bias = [&](int cob) {
#pragma unroll
    for (int p = 0; p < NPIECE_EPI; ++p) load_bias_piece(cob, p / 4, p % 4, bsv[kBias ? p / 4 : 0][p % 4]);
  };

  int tile = bid;
  if (tile >= ntiles) return;
  TileId cur = tile_id(tile);
  // prologue: chunk 0 of the block's first tile (WRES: and every weight chunk)
  if constexpr (DMA) {
#pragma unroll
    for (int it = 0; it < T::IN_IT; ++it) issue_in(cur, 0, 0, it);
    for (int c = 0; c < (kWRes ? a.nchunks : 1); ++c)
#pragma unroll
      for (int it = 0; it < T::W_IT; ++it) issue_w(cur, c, c, it);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
    load_w(cur, 0);
    load_in(cur, 0);
    store_in(0);
    store_w(0);
  }
  __syncthreads();
  int buf = 0;
  for (;;) {
    const int ntile = tile + cgrid;
    const bool more = ntile < ntiles;
    const TileId nxt = tile_id(more ? ntile : tile);
    if constexpr (kNoMfma || kMfma16) {  // probes: the accumulators are not written by the chunk loop's MFMAs
#pragma unroll
      for (int mt = 0; mt < WM; ++mt)
#pragma unroll
        for (int nt = 0; nt < WN; ++nt)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            acc[mt][nt][i] = 0.f;
            accx[mt][nt][i] = 0.f;
            if constexpr (kMfma16) p16[mt][nt][i >> 3][(i >> 2) & (PLANES - 1)][i & 3] = 0.f;
          }
    }
    if constexpr (kBias == 2) load_bias(cur.cob);
    // chunk 0 peeled (its MFMAs start the accumulators from C = 0), then chunks 1 .. nchunks - 1
    auto chunk_iter = [&](const int c, auto zc) {
      // staged during this chunk: chunk c+1 of this tile, or chunk 0 of the next tile
      const bool last = c + 1 == a.nchunks;
      const bool pre = !last || more;
      const TileId& pt = last ? nxt : cur;
      const int pc = last ? 0 : c + 1;
      const int wslot = kWRes ? c : buf;
      if constexpr (DMA) {
        // buf^1 was last read in the previous chunk, before the barrier that ended it
        if constexpr (kSpread) {
          compute(buf, wslot, [&](int t) {
            if (t < kSpreadTaps && pre) {
              // pieces [t NPIECE / kSpreadTaps, (t + 1) NPIECE / kSpreadTaps) with tap t; the piece
              // index a compile-time constant (a runtime index put the per-piece offsets in scratch)
#pragma unroll
              for (int k = 0; k < NPIECE; ++k)
                if (t * NPIECE / kSpreadTaps <= k && k < (t + 1) * NPIECE / kSpreadTaps) issue_piece(pt, pc, buf ^ 1, k);
            }
          }, zc);
        } else if constexpr (kStagger) {
          const bool late = __builtin_amdgcn_readfirstlane(tid) >= NT / 2;
          if (pre && !late) {
#pragma unroll
            for (int k = 0; k < NPIECE; ++k) issue_piece(pt, pc, buf ^ 1, k);
          }
          compute(buf, wslot, [&](int t) {
            if (t == kStaggerTap && pre && late) {
#pragma unroll
              for (int k = 0; k < NPIECE; ++k) issue_piece(pt, pc, buf ^ 1, k);
            }
          }, zc);
        } else {
          if (pre) {
#pragma unroll
            for (int k = 0; k < NPIECE; ++k) issue_piece(pt, pc, buf ^ 1, k);
          }
          compute(buf, wslot, [](int) {}, zc);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      } else {
        if (pre) {
          load_w(pt, pc);
          load_in(pt, pc);
        }
        compute(buf, buf, [](int) {}, zc);
        if (pre) {
          store_in(buf ^ 1);
          store_w(buf ^ 1);
        }
        __syncthreads();
      }
      buf ^= 1;
    };
    chunk_iter(0, std::true_type{});
    for (int c = 1; c < a.nchunks; ++c) chunk_iter(c, std::false_type{});

    if constexpr (kMfma16) {  // probe: keep the results live (values are not the conv)
#pragma unroll
      for (int mt = 0; mt < WM; ++mt)
#pragma unroll
        for (int nt = 0; nt < WN; ++nt)
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            acc[mt][nt][i] = p16[mt][nt][i >> 2][0][i & 3];
            accx[mt][nt][i] = p16[mt][nt][i >> 2][PLANES - 1][i & 3];
          }
    }

    if constexpr (kNoEpi) {
#pragma unroll
      for (int mt = 0; mt < WM; ++mt)
#pragma unroll
        for (int nt = 0; nt < WN; ++nt)
#pragma unroll
          for (int i = 0; i < 16; ++i) asm volatile("" ::"v"(acc[mt][nt][i]), "v"(accx[mt][nt][i]));
    } else {
      floatx16 V[WM][WN];
      combine(V);
      if constexpr (kBias == 1) load_bias(cur.cob);
      // the bias has landed (mode 2: long ago, the chunk loop drained vmcnt): a wait the
      // compiler sees, so that it does not wait out each piece's stores before the next
      // piece's bias (vmcnt(0), as s_waitcnt's 16-bit immediate)
      if constexpr (kBias != 0) __builtin_amdgcn_s_waitcnt(0x0F70);
      if constexpr (kWide) {
#pragma unroll
        for (int pp = 0; pp < NPIECE_EPI / 2; ++pp) {
          const int mt = pp / 2, qp = pp % 2;
          if constexpr (kBias == 0) {
            float b0[4], b1[4];
            load_bias_piece(cur.cob, mt, 2 * qp, b0);
            load_bias_piece(cur.cob, mt, 2 * qp + 1, b1);
            epi_pair(cur, V, mt, qp, b0, b1);
          } else {
            epi_pair(cur, V, mt, qp, bsv[mt][2 * qp], bsv[mt][2 * qp + 1]);
          }
        }
      } else {
#pragma unroll
        for (int p = 0; p < NPIECE_EPI; ++p) {
          if constexpr (kBias == 0) {
            float bq[4];
            load_bias_piece(cur.cob, p / 4, p % 4, bq);
            epi_piece(cur, V, p / 4, p % 4, bq);
          } else {
            epi_piece(cur, V, p / 4, p % 4, bsv[p / 4][p % 4]);
          }
        }
      }
    }
    if (!more) break;
    tile = ntile;
    cur = nxt;
  }
  if (bad && a.status) *a.status = 1;
}

static int num_cus(int dev) {
  static std::atomic<int> n[kMaxDevices] = {};
  int v = n[dev].load(std::memory_order_relaxed);
  if (!v) {
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1) v = 256;
    n[dev].store(v, std::memory_order_relaxed);
  }
  return v;
}

template <int NW, int WM, int WN, int PLANES, int EPI, bool DMA, int SCHED, bool F32 = false>
static int launch_h8_k(const ConvH8Args& args, int persist, hipStream_t st, rrin_launch_info* info = nullptr) {
  using T = TileH8<NW, WM, WN, PLANES>;
  auto k = conv3x3_h8_kernel<NW, WM, WN, PLANES, EPI, DMA, SCHED, F32>;
  constexpr bool wres = DMA && (SCHED & SCHED_WRES) != 0;
  const size_t lds = h8_lds_bytes<NW, WM, WN, PLANES>(wres, args.nchunks);
  if (lds > kMaxLds) return RRIN_E_CONFIG;
  static LdsAttr attr;
  // resident blocks per CU, per device and LDS footprint (WRES: chunk count)
  static std::atomic<int> per_cu[kMaxDevices][40] = {};
  if (int e = attr.ensure((const void*)k, (int)kMaxLds, st)) return e;
  const int64_t ntiles = (int64_t)args.co_blocks * args.tiles_x * args.tiles_y * args.n;
  int64_t grid = ntiles;
  if (persist > 0) {
    const int dev = stream_device(st);
    std::atomic<int>& slot = per_cu[dev][wres ? (args.nchunks < 40 ? args.nchunks : 39) : 0];
    int pc = slot.load(std::memory_order_relaxed);
    if (!pc) {
      hipError_t e = on_device(dev, [&] {
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc, (const void*)k, T::NT, lds);
      });
      if (e != hipSuccess) return (int)e;
      if (pc < 1) pc = 1;
      slot.store(pc, std::memory_order_relaxed);
    }
    int64_t g = (int64_t)persist * pc * num_cus(dev);
    g -= g % args.co_blocks;  // WRES: every tile of a block in the block's channel block
    if (g < args.co_blocks) g = args.co_blocks;
    if (g < grid) grid = g;
  }
  if constexpr (EPI == RRIN_EPI_SUBPIXEL && T::NT >= 256) {
    if (args.fix_real > 0) {  // the FULL ring fix-up in workgroups [0, nfix) of this launch
      constexpr int VG = T::NT / 256;  // ring tiles per workgroup, one per 256-thread slice
      ConvH8Args b = args;
      b.nfix = ((args.fix_real + VG - 1) / VG + 7) & ~7;
      b.fix.nslices = F32 ? b.fix.cin / kFixCi : 1;  // fp32: runs of one chunk, added in run order
      b.fix.cross = 0;
      if (info) return launch_report(info, ntiles, grid, b.nfix, 0);
      const size_t flds = (size_t)VG * kFixSubFloats * sizeof(float);
      hipLaunchKernelGGL(k, dim3((unsigned)(grid + b.nfix)), dim3(T::NT), lds > flds ? lds : flds, st, b);
      return hip_code(hipGetLastError());
    }
  }
  if (info) return launch_report(info, ntiles, grid, 0, 0);
  hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(T::NT), lds, st, args);
  return hip_code(hipGetLastError());
}

template <int NW, int WM, int WN, int PLANES, int EPI, int SCHED, bool F32 = false>
static int launch_h8_t(const ConvH8Args& args, int persist, hipStream_t st, rrin_launch_info* info) {
  using T = TileH8<NW, WM, WN, PLANES>;
  if constexpr (T::LDS > kMaxLds) {
    return RRIN_E_CONFIG;
  } else {
    if (args.cin % 8 == 0 || args.tail_finite)
      return launch_h8_k<NW, WM, WN, PLANES, EPI, true, SCHED, F32>(args, persist, st, info);
    if constexpr (EPI == RRIN_EPI_LEAKY_REP || EPI == RRIN_EPI_SUBPIXEL) {
      return RRIN_E_CONFIG;  // decoder-side modes: always whole channel groups
    } else {
      return launch_h8_k<NW, WM, WN, PLANES, EPI, false, 0, F32>(args, persist, st, info);  // knobs need DMA
    }
  }
}

template <int NW, int WM, int WN, int PLANES, int SCHED, bool F32>
static int launch_h8_epi(const ConvH8Args& args, int epi, int persist, hipStream_t st, rrin_launch_info* info) {
  switch (epi) {
    case RRIN_EPI_LINEAR: return launch_h8_t<NW, WM, WN, PLANES, RRIN_EPI_LINEAR, SCHED, F32>(args, persist, st, info);
    case RRIN_EPI_LEAKY: return launch_h8_t<NW, WM, WN, PLANES, RRIN_EPI_LEAKY, SCHED, F32>(args, persist, st, info);
    case RRIN_EPI_LEAKY_POOL: return launch_h8_t<NW, WM, WN, PLANES, RRIN_EPI_LEAKY_POOL, SCHED, F32>(args, persist, st, info);
    case RRIN_EPI_LEAKY_REP: return launch_h8_t<NW, WM, WN, PLANES, RRIN_EPI_LEAKY_REP, SCHED, F32>(args, persist, st, info);
    default: return launch_h8_t<NW, WM, WN, PLANES, RRIN_EPI_SUBPIXEL, SCHED, F32>(args, persist, st, info);
  }
}

template <int NW, int WM, int WN, int SCHED>
static int launch_h8_cfg(const ConvH8Args& args, int prec, int epi, int persist, hipStream_t st,
                         rrin_launch_info* info) {
  if (prec == RRIN_PREC_F32R) return launch_h8_epi<NW, WM, WN, 1, SCHED, true>(args, epi, persist, st, info);
  if (planes_of(prec) == 2) return launch_h8_epi<NW, WM, WN, 2, SCHED, false>(args, epi, persist, st, info);
  return launch_h8_epi<NW, WM, WN, 1, SCHED, false>(args, epi, persist, st, info);
}

int launch_h8(const ConvH8Args& a, int cfg, int prec, int epi, hipStream_t st, rrin_launch_info* info) {
  switch (cfg) {
#define X(id, nw, wm, wn, sc, pe) \
  case id:                        \
    return launch_h8_cfg<nw, wm, wn, sc>(a, prec, epi, pe, st, info);
    RRIN_H8_CFGS(X)
#undef X
  }
  return RRIN_E_CONFIG;
}

#ifdef RRIN_LAB
// Kernel lab (tools/conv_lab.py ablate; built only into librrin_lab.so, `make lab`): one LEAKY
// conv of a direct-form tile with the schedule knobs `sched` (SCHED_*, ablations included) and
// grid `persist` (as PE), at F16X3 (cfg 0, 1, 6) or F32R (cfg 0, 1, 3, 4, 5, 6, 16).
template <int NW, int WM, int WN, bool F32>
static int lab_cfg(const ConvH8Args& a, int sched, int persist, hipStream_t st) {
  constexpr int P = F32 ? 1 : 2;
  switch (sched) {
#define L(v) \
  case v:    \
    return launch_h8_k<NW, WM, WN, P, RRIN_EPI_LEAKY, true, v, F32>(a, persist, st);
    L(0) L(1) L(2) L(3) L(4) L(7) L(8) L(11) L(12) L(15) L(16) L(32) L(48) L(64) L(96) L(128) L(144)
#undef L
  }
  return RRIN_E_CONFIG;
}

int launch_h8_lab(const ConvH8Args& a, int cfg, int prec, int sched, int persist, hipStream_t st) {
  if (prec == RRIN_PREC_F32R) {
    switch (cfg) {
      case 0: return lab_cfg<8, 2, 2, true>(a, sched, persist, st);
      case 1: return lab_cfg<8, 1, 2, true>(a, sched, persist, st);
      case 3: return lab_cfg<4, 1, 4, true>(a, sched, persist, st);
      case 4: return lab_cfg<4, 2, 1, true>(a, sched, persist, st);
      case 5: return lab_cfg<8, 4, 2, true>(a, sched, persist, st);
      case 6: return lab_cfg<4, 1, 2, true>(a, sched, persist, st);
      case 16: return lab_cfg<4, 1, 1, true>(a, sched, persist, st);
    }
    return RRIN_E_CONFIG;
  }
  switch (cfg) {
    case 0: return lab_cfg<8, 2, 2, false>(a, sched, persist, st);
    case 1: return lab_cfg<8, 1, 2, false>(a, sched, persist, st);
    case 6: return lab_cfg<4, 1, 2, false>(a, sched, persist, st);
  }
  return RRIN_E_CONFIG;
}
#endif

}  // namespace rrin
