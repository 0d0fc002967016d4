// The sub-pixel ring fix-up as its own launch: kernel and host side (device body: edge_fix.hpp,
// which conv tiles also run inside their own launch).  rrin_subpixel_edge_fix_h8,
// rrin_edge_fix_split_floats; edge_fix_prepare / edge_fix_run also serve conv_rec.hip's ring_full.
#include <string.h>

#include "edge_fix.hpp"
#include "h8.hpp"

namespace rrin {

template <int PLANES, int KS, bool F32 = false, bool FULL = false>
__global__ void RRIN_PK_EDGE_ATTR __launch_bounds__(256 * KS) edge_fix_h8_kernel(EdgeFixArgs a) {
  edge_fix_body<PLANES, KS, F32, FULL>(a, blockIdx.x, blockIdx.y, blockIdx.z);
}

template <int PLANES, int KS, bool F32, bool FULL>
static int edge_fix_launch_m(const EdgeFixArgs& a, dim3 grid, hipStream_t st) {
  constexpr size_t lds = (size_t)KS * kFixSubFloats * sizeof(float);
  static_assert(lds <= 160 * 1024, "edge fix LDS");
  static_assert(kFixSubFloats >= 4 * 256, "K-group sums fit a staging region");
  static LdsAttr attr;
  if (int e = attr.ensure((const void*)edge_fix_h8_kernel<PLANES, KS, F32, FULL>, (int)lds, st)) return e;
  hipLaunchKernelGGL((edge_fix_h8_kernel<PLANES, KS, F32, FULL>), grid, dim3(256 * KS), lds, st, a);
  return hip_code(hipGetLastError());
}

template <int PLANES, int KS, bool F32 = false>
static int edge_fix_launch(const EdgeFixArgs& a, dim3 grid, hipStream_t st, bool full) {
  return full ? edge_fix_launch_m<PLANES, KS, F32, true>(a, grid, st)
              : edge_fix_launch_m<PLANES, KS, F32, false>(a, grid, st);
}

// K groups and K runs of the ring fix-up, by cin and precision only (the
// summation order never depends on batch, size or scratch).  fp32 records: 2
// groups from cin 64 on, never 4 (4 x 256 threads cap a thread at 128 VGPRs and
// the fp32 kernel spills there: 31.6 vs 15.7 us per launch), runs of one chunk per
// group (cin / 64 runs).  fp16: split16 stops at 2 groups (the two-plane kernel
// spills at 4), one run.
static void edge_fix_split(int cin, int prec, int* ks, int* nsl) {
  *nsl = 1;
  if (prec == RRIN_PREC_F32R) {
    *ks = cin % (2 * kFixCi) == 0 ? 2 : 1;
    if (cin % (*ks * kFixCi) == 0) *nsl = cin / (*ks * kFixCi);
    return;
  }
  *ks = cin % (2 * kFixCi) == 0 && cin >= 4 * kFixCi ? 2 : 1;
  if (planes_of(prec) == 1 && cin % (4 * kFixCi) == 0 && cin >= 8 * kFixCi) *ks = 4;
}

// ring tiles of a line of px pixels; the fix-up's grid for an H x W output: the tiles of both
// row lines and both column lines (the corners are in the rows) x co blocks x images
static int edge_fix_tiles(int px) { return (px + kFixPx - 1) / kFixPx; }
static dim3 edge_fix_grid(int H, int W, int cout, int n) {
  return dim3((unsigned)(2 * edge_fix_tiles(W) + 2 * edge_fix_tiles(H - 2)), (unsigned)((cout + kFixCo - 1) / kFixCo),
              (unsigned)n);
}

// validate d and fill a (everything but the K split); grid: ring tiles x co blocks x images
int edge_fix_prepare(const rrin_edge_fix_desc* d, EdgeFixArgs& a, dim3& grid) {
  if (!d || (!d->edge && !d->full) || !d->wedge || !d->bias || (d->full != 0 && d->full != 1)) return RRIN_E_ARG;
  if (!rec_prec(d->prec)) return RRIN_E_ARG;
  if (d->n < 1 || d->cin < 8 || (d->cin & 7) || d->cout < 8 || (d->cout & 7)) return RRIN_E_ARG;
  if (d->epi_mode != RRIN_EPI_LINEAR && d->epi_mode != RRIN_EPI_LEAKY) return RRIN_E_ARG;
  if (!h8_ok(d->src, d->prec) || !h8_ok(d->dst, d->prec)) return RRIN_E_SHAPE;
  if (d->dst.g.h != 2 * d->src.g.h || d->dst.g.w != 2 * d->src.g.w) return RRIN_E_SHAPE;
  const int cpr = chans_per_rec(d->prec);
  if (d->cin > cpr * d->src.groups || d->cout > cpr * d->dst.groups) return RRIN_E_ARG;
  const int planes = planes_of(d->prec);
  memset(&a, 0, sizeof(a));
  const int64_t sg = (int64_t)d->src.g_off * d->src.g.plane, dg = (int64_t)d->dst.g_off * d->dst.g.plane;
  a.s_hi = static_cast<const uint4*>(d->src.hi) + sg;
  a.s_lo = planes == 2 ? static_cast<const uint4*>(d->src.lo) + sg : nullptr;
  a.s_img = d->src.img_stride;
  a.s_gp = d->src.g.plane;
  a.s_wp = d->src.g.wp;
  a.sh = d->src.g.h;
  a.sw = d->src.g.w;
  a.cin = d->cin;
  if (d->prec == RRIN_PREC_F32R) {
    a.d_f32 = static_cast<float*>(d->dst.hi) + dg * 4;
  } else {
    a.d_hi = static_cast<_Float16*>(d->dst.hi) + dg * 8;
    a.d_lo = planes == 2 ? static_cast<_Float16*>(d->dst.lo) + dg * 8 : nullptr;
  }
  a.d_img = d->dst.img_stride;
  a.d_gp = d->dst.g.plane;
  a.d_wp = d->dst.g.wp;
  a.cout = d->cout;
  a.edge = d->edge;
  a.wedge = d->wedge;
  a.bias = d->bias;
  a.ring = ring_pixels(d->dst.g.h, d->dst.g.w);
  a.slope = d->slope;
  a.leaky = d->epi_mode == RRIN_EPI_LEAKY;
  a.status = d->status;
  a.tiles_row = edge_fix_tiles(d->dst.g.w);
  a.tiles_col = edge_fix_tiles(d->dst.g.h - 2);
  grid = edge_fix_grid(d->dst.g.h, d->dst.g.w, d->cout, d->n);
  a.nslices = 1;
  a.cross = 0;
  return 0;
}

// the fix-up as its own launch: K groups / runs by edge_fix_split; the cross-workgroup K split
// where the caller passed its scratch (fp32 records)
// (one_group: one K group, fp32 runs of one chunk -- the order of the in-launch fix-up)
int edge_fix_run(EdgeFixArgs a, dim3 grid, int prec, bool full, const rrin_edge_fix_desc* d, hipStream_t st,
                 bool one_group) {
  int ks, nsl;
  edge_fix_split(a.cin, prec, &ks, &nsl);
  if (one_group) {
    ks = 1;
    // runs of whole chunks only: a cin that is no multiple of kFixCi is one run whose last chunk is
    // masked (cin / kFixCi would be no run at all below kFixCi, and runs that overlap above it)
    nsl = prec == RRIN_PREC_F32R && a.cin % kFixCi == 0 ? a.cin / kFixCi : 1;
    d = nullptr;
  }
  a.nslices = nsl;
  a.cross = 0;
  dim3 g = grid;
  const int n = (int)grid.z;
  const int64_t tiles = (int64_t)grid.x * grid.y * n;
  if (d && nsl > 1 && d->part && d->cnt && tiles * nsl * 1024 <= d->part_floats && tiles <= d->cnt_len) {
    a.cross = 1;  // one workgroup per K run (same arithmetic as the loop over runs)
    a.part = d->part;
    a.cnt = d->cnt;
    g.z = (unsigned)(n * nsl);
  }
  if (prec == RRIN_PREC_F32R) {
    return ks == 2 ? edge_fix_launch<1, 2, true>(a, g, st, full) : edge_fix_launch<1, 1, true>(a, g, st, full);
  }
  switch (planes_of(prec) * 8 + ks) {
    case 2 * 8 + 2: return edge_fix_launch<2, 2>(a, g, st, full);
    case 2 * 8 + 1: return edge_fix_launch<2, 1>(a, g, st, full);
    case 1 * 8 + 4: return edge_fix_launch<1, 4>(a, g, st, full);
    case 1 * 8 + 2: return edge_fix_launch<1, 2>(a, g, st, full);
    default: return edge_fix_launch<1, 1>(a, g, st, full);
  }
}

}  // namespace rrin

using namespace rrin;

extern "C" int rrin_subpixel_edge_fix_h8(const rrin_edge_fix_desc* d, void* stream) {
  EdgeFixArgs a;
  dim3 grid;
  if (int e = edge_fix_prepare(d, a, grid)) return e;
  return edge_fix_run(a, grid, d->prec, d->full == 1, d, (hipStream_t)stream);
}

// floats of rrin_edge_fix_desc.part and ints of .cnt for the cross-workgroup K split (0 where the
// fix-up has one K run).  A size query: it checks what it reads, less than edge_fix_prepare
extern "C" int64_t rrin_edge_fix_split_floats(const rrin_edge_fix_desc* d, int64_t* cnt) {
  if (!d || d->n < 1 || d->cin < 8 || (d->cin & 7) || d->cout < 8 || !rec_prec(d->prec)) return RRIN_E_ARG;
  int ks, nsl;
  edge_fix_split(d->cin, d->prec, &ks, &nsl);
  if (d->dst.g.h < 2 || d->dst.g.w < 1) return RRIN_E_SHAPE;
  const dim3 g = edge_fix_grid(d->dst.g.h, d->dst.g.w, d->cout, d->n);
  const int64_t tiles = (int64_t)g.x * g.y * g.z;
  if (cnt) *cnt = nsl > 1 ? tiles : 0;
  return nsl > 1 ? tiles * nsl * 1024 : 0;
}
