// What the Winograd record-conv tiles share (conv_wino.hip: kind 1; conv_winoq.hip: kinds 3, 4;
// conv_winoc.hip: kinds 6, 7; conv_winoc42.hip: kind 14; conv_winoh.hip: kind 6 at fp16): the workgroup order (XCD
// remap, co-block groups), the LDS column swizzle and buffer-load helpers, and on the host the
// co-block group size and the per-epilogue kernel dispatch.  Every device function inlines into
// its kernel; what a kernel holds as a compile-time constant is one here.  The vector types are
// h8.hpp's.
#pragma once
#include <type_traits>
#include <utility>

#include "h8.hpp"

namespace rrin {

// The LDS-staged F(2x2,3x3) tiles (conv_wino.hip, conv_winoq.hip), per 8-channel chunk: raw
// tile rows of 34 columns (32 px + halo), one U slab [xi 16][half 2][co 32] of records
constexpr int kWnRawCols = 34;
constexpr int kWnU = 16 * 2 * 32;

// LDS position of raw column col (0..33) within its row: even columns first (the stride-2
// window reads of 16 lanes fall on distinct banks)
__device__ inline int wino_col(int col) { return (col & 1) * 17 + (col >> 1); }

// buffer_load_dwordx4 ... lds: one 16-B record per lane at byte offset voff of rsrc into
// the lane-linear LDS image at the wave-uniform base
__device__ inline void buf_dma16(__amdgpu_buffer_rsrc_t rs, uint4* lds_wave_base, uint32_t voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds_wave_base, 16, voff, 0, 0,
                                           0);
}
__device__ inline __amdgpu_buffer_rsrc_t buf_rsrc(const void* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7fffffff, 0x00020000);
}
__device__ inline floatx4 buf_load16(__amdgpu_buffer_rsrc_t rs, uint32_t voff, int soff) {
  return __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0));
}

// XCD-aware bijective remap (conv_mfma.hip): an XCD's workgroups are consecutive tiles.  Workgroup
// (xcd, slot) of a grid of 8 q + r
__device__ inline int wino_xcd_perm(int q, int r, int xcd, int slot) {
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
}
// ... workgroup idx of nwg
__device__ inline int wino_xcd_bid(int nwg, int idx) {
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = idx & 7, slot = idx >> 3;
  return wino_xcd_perm(q, r, xcd, slot);
}
// ... this workgroup
__device__ inline int wino_xcd_bid() {
  const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  return wino_xcd_perm(q, r, xcd, slot);
}
// ... past nfix (a multiple of 8: each conv workgroup keeps its XCD) ring workgroups at the head
// of the grid
__device__ inline int wino_xcd_bid(int nfix) {
  const int nwg = (int)gridDim.x - nfix, q = nwg >> 3, r = nwg & 7;
  const int cb = (int)blockIdx.x - nfix;
  const int xcd = cb & 7, slot = cb >> 3;
  return wino_xcd_perm(q, r, xcd, slot);
}

// tile (of ntiles = co blocks x positions x images) -> (co block, x0, y0, image) for TW x TH tiles: groups of a.cob_group co blocks (0: one
// group of all; wino_cob_group: U of a group fits an XCD's L2), tile positions within a group,
// the group's co blocks of a tile position on consecutive workgroups (they share its raw tile)
struct WinoTile {
  int cob, x0, y0, img;
};
__device__ inline WinoTile wino_tile_pos(const ConvH8Args& a, int ntiles, int tile, int TW, int TH) {
  const int cpg = a.cob_group > 0 ? a.cob_group : a.co_blocks;
  const int gsz = cpg * (ntiles / a.co_blocks);  // workgroups of a full group
  const int g = tile / gsz;
  const int r = tile - g * gsz;
  const int cg = min(cpg, a.co_blocks - g * cpg);  // co blocks of this group (the last may be short)
  WinoTile p;
  p.cob = g * cpg + r % cg;
  int t = r / cg;
  p.x0 = (t % a.tiles_x) * TW;
  t /= a.tiles_x;
  p.y0 = (t % a.tiles_y) * TH;
  p.img = t / a.tiles_y;
  return p;
}

// ---- host side -------------------------------------------------------------------------
// Workgroup order (XCD-aware remap: an XCD runs a contiguous range of workgroups): a workgroup
// streams its co block's whole U; when the co blocks' U does not fit an XCD's 4 MB L2, co blocks
// of one tile position that started at different times each stream U from HBM (PMC: up to 11x
// the algorithmic bytes on the deep convs).  Groups of co blocks whose U fits budget_kb put each
// XCD on one group (its U read once per XCD, L2-resident) at the price of reading each raw tile
// once per group.  Returns the largest power of two of co blocks whose U (per_cob_bytes each)
// fits, at least one; 0: one group of all (everything fits, or no budget).  The order changes
// no result.
inline int wino_cob_group(int co_blocks, int64_t per_cob_bytes, int budget_kb) {
  const int64_t cap = (int64_t)budget_kb * 1024;
  if (budget_kb <= 0 || (int64_t)co_blocks * per_cob_bytes <= cap) return 0;
  int g = 1;
  while (2 * g < co_blocks && 2 * g * per_cob_bytes <= cap) g *= 2;
  return g;
}

// f(std::integral_constant<int, EPI>) for the epilogue mode epi: one kernel instance per mode
template <class F>
inline int wino_dispatch_epi(int epi, F&& f) {
  switch (epi) {
    case RRIN_EPI_LINEAR: return f(std::integral_constant<int, RRIN_EPI_LINEAR>{});
    case RRIN_EPI_LEAKY: return f(std::integral_constant<int, RRIN_EPI_LEAKY>{});
    case RRIN_EPI_LEAKY_POOL: return f(std::integral_constant<int, RRIN_EPI_LEAKY_POOL>{});
    case RRIN_EPI_LEAKY_REP: return f(std::integral_constant<int, RRIN_EPI_LEAKY_REP>{});
    case RRIN_EPI_SUBPIXEL: return f(std::integral_constant<int, RRIN_EPI_SUBPIXEL>{});
  }
  return RRIN_E_ARG;
}

}  // namespace rrin
