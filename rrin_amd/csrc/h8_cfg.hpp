// Tile-config table of every record conv: the direct-form tiles of conv_h8.hip (TileH8, the
// RRIN_H8_CFGS list, which the kernel file instantiates) and the Winograd tiles of conv_wino*.hip.
// Plain constexpr C++; conv_rec.hip and conv_block0.hip read the table.
#pragma once
#include "h8.hpp"

namespace rrin {

template <int NW, int WM, int WN, int PLANES>
struct TileH8 {
  static constexpr int NT = 64 * NW;
  static constexpr int BM = 32 * WM;
  static constexpr int TH = WN * NW;
  static constexpr int ROWS = TH + 2;
  static constexpr int IN_REC = 2 * ROWS * H8_LC;  // per plane: 2 groups x rows x cols
  static constexpr int W_REC = 9 * 2 * BM;          // per plane: taps x halves x co
  static constexpr int IN_IT = (IN_REC + NT - 1) / NT;
  static constexpr int W_IT = (W_REC + NT - 1) / NT;
  static constexpr size_t LDS = 2 * (size_t)PLANES * (IN_REC + W_REC) * 16;
  static_assert(16 % TH == 0, "TH must divide the 16-row plane padding");
};

// Schedule knobs of the direct-form kernel (its template SCHED; see conv_h8.hip)
enum : int {
  SCHED_NO_WDMA = 1, SCHED_NO_IDMA = 2, SCHED_NO_MFMA = 4, SCHED_NO_EPI = 8,
  SCHED_SPREAD = 16, SCHED_WRES = 32, SCHED_STAGGER = 64, SCHED_MFMA16 = 128
};

// Direct-form configs: cfg -> (NW waves along rows, WM co-tiles, WN rows per wave,
// SC schedule knobs SCHED_*, PE grid: 0 = one tile per block, k = k x the
// blocks a CU holds at once, persistent).  16-17 (BM 32 x TH 4) are for the
// few-tile deep levels of small workloads (engine size classes).
#define RRIN_H8_CFGS(X)  \
  X(0, 8, 2, 2, 0, 0)    \
  X(1, 8, 1, 2, 0, 0)    \
  X(2, 4, 2, 2, 0, 0)    \
  X(3, 4, 1, 4, 0, 0)    \
  X(4, 4, 2, 1, 0, 0)    \
  X(5, 8, 4, 2, 0, 0)    \
  X(6, 4, 1, 2, 0, 0)    \
  X(7, 2, 1, 4, 0, 0)    \
  X(8, 4, 1, 2, 32, 1)   \
  X(9, 8, 1, 2, 32, 1)   \
  X(10, 8, 2, 2, 16, 1)  \
  X(11, 8, 2, 2, 16, 0)  \
  X(12, 4, 1, 2, 16, 1)  \
  X(13, 8, 1, 2, 16, 1)  \
  X(14, 4, 1, 2, 48, 1)  \
  X(15, 8, 1, 2, 48, 1)  \
  X(16, 4, 1, 1, 16, 1)  \
  X(17, 2, 1, 2, 16, 1)

// Shared memory of one block: double-buffered input tile and weight slab, or
// with WRES every chunk's weight slab resident.
template <int NW, int WM, int WN, int PLANES>
constexpr size_t h8_lds_bytes(bool wres, int nchunks) {
  using T = TileH8<NW, WM, WN, PLANES>;
  return ((size_t)2 * T::IN_REC + (size_t)(wres && nchunks > 2 ? nchunks : 2) * T::W_REC) * PLANES * 16;
}

constexpr size_t kMaxLds = 160 * 1024;
constexpr size_t kNoLds = (size_t)1 << 30;  // > kMaxLds: never usable

struct CfgH8 {
  int bm, th;
  size_t lds1, lds2;  // at two weight slabs (WRES: at <= 2 chunks); only ever compared with kMaxLds
  size_t wslab;       // bytes of one weight slab per plane (WRES: one more per chunk past 2)
  bool pool_ok;
  int sched, persist;
  int nt;  // threads per workgroup (the direct-form tiles; 0: Winograd configs)
  // as rrin_conv_h8_cfg_wino reports it.  0: direct form; Winograd tile kind: 1 (conv_wino.hip), 3, 4 (conv_winoq.hip),
  // 6, 7 (conv_winoc.hip; 6 also at fp16, conv_winoh.hip), 14 (conv_winoc42.hip); -1: a retired id
  // (rrin_conv_h8_cfg_ok 0, RRIN_E_CONFIG)
  int kind;
};
// a Winograd tile: one plane (exact fp32 records; kind 6 also fp16), never two
constexpr CfgH8 wino_cfg(int kind, int bm, int th, size_t lds) { return {bm, th, lds, kNoLds, 0, true, 0, 0, 0, kind}; }
// Round 6 removed the rejected Winograd tiles (kinds 2, 5, 8-13; DESIGN.md §5b-§5e keep their
// measurements): their ids stay reserved so that the later ids keep their meaning
constexpr CfgH8 retired_cfg(int bm, int th) { return {bm, th, kNoLds, kNoLds, 0, true, 0, 0, 0, -1}; }

inline constexpr CfgH8 kCfgH8[] = {
#define X(id, nw, wm, wn, sc, pe)                                                                               \
  {TileH8<nw, wm, wn, 1>::BM, TileH8<nw, wm, wn, 1>::TH, h8_lds_bytes<nw, wm, wn, 1>((sc & SCHED_WRES) != 0, 2), \
   h8_lds_bytes<nw, wm, wn, 2>((sc & SCHED_WRES) != 0, 2), (size_t)TileH8<nw, wm, wn, 1>::W_REC * 16,     \
   (wn % 2) == 0, sc, pe, 64 * nw, 0},
    RRIN_H8_CFGS(X)
#undef X
    wino_cfg(1, 32, 8, kWinoLds),      // 18: Winograd F(2x2,3x3) on fp32 records, BM 32 x TH 8
    retired_cfg(64, 8),                // 19: the kind-2 tile (BM 64, 8 waves, one block per CU) lost to kinds 3 and 6
    wino_cfg(3, 32, 8, kWinoQLds),     // 20: cfg 18's tile and packing, 8 waves of 4 accumulators
    wino_cfg(4, 32, 4, kWinoQLds),     // 21: the same on half-height tiles (4 waves): twice the tiles
    retired_cfg(32, 16),               // 22: Winograd F(4x4,3x3) (kind 5), 1.28-1.58x kind 3's time
    wino_cfg(6, 64, 4, kWinoCLds1),    // 23: register-U tile, 4 waves of 2 co tiles; at fp16 with f16 MFMAs
    wino_cfg(7, 32, 8, kWinoCLds2),    // 24: register-U tile, 4 waves of 2 patch tiles
    wino_cfg(14, 32, 8, kWinoC42Lds),  // 25 (round 6): register-U tile in F(4,3) x F(2,3)
};
constexpr int kNumCfgH8 = sizeof(kCfgH8) / sizeof(kCfgH8[0]);
static_assert(kNumCfgH8 == 26, "config ids (engine tables, rrin_hip.h)");

// the table row of cfg, nullptr outside [0, count)
inline const CfgH8* h8_cfg(int cfg) { return cfg >= 0 && cfg < kNumCfgH8 ? &kCfgH8[cfg] : nullptr; }

}  // namespace rrin
