// Host-only front end of the record convs: the queries of the tile-config table (h8_cfg.hpp),
// descriptor validation and kernel arguments for every kernel kind (h8_prepare), the scratch-size
// queries, and rrin_conv3x3_h8_fwd's dispatch to the direct-form tiles (conv_h8.hip), the Winograd
// tiles (conv_wino*.hip) and the ring fix-up (edge_fix.hip).  No device code.
#include <string.h>

#include "h8_cfg.hpp"

namespace rrin {

static constexpr int kMaxKSplit = 16;

// Validate a conv descriptor and turn it into kernel arguments.
static int h8_prepare(const rrin_conv_h8_desc* d, ConvH8Args& a, bool need_scratch = true) {
  if (!d || !d->whi || !d->bias) return RRIN_E_ARG;
  if (!rec_prec(d->prec)) return RRIN_E_ARG;
  if (d->prec == RRIN_PREC_F16X3 && !d->wlo) return RRIN_E_ARG;
  const CfgH8* cp = h8_cfg(d->cfg);
  if (!cp || cp->kind < 0 || (planes_of(d->prec) == 2 ? cp->lds2 : cp->lds1) > kMaxLds) return RRIN_E_CONFIG;
  const CfgH8& ci = *cp;
  const bool wino = ci.kind > 0;
  if (d->n < 1 || d->cin < 1 || d->cout < 8 || (d->cout & 7)) return RRIN_E_ARG;
  if (d->epi_mode < RRIN_EPI_LINEAR || d->epi_mode > RRIN_EPI_SUBPIXEL) return RRIN_E_ARG;
  if (!h8_ok(d->src, d->prec) || !h8_ok(d->dst, d->prec)) return RRIN_E_SHAPE;
  const bool sub = d->epi_mode == RRIN_EPI_SUBPIXEL;
  const int h = d->src.g.h, w = d->src.g.w;  // the grid the conv runs on
  if (d->dst.g.h != (sub ? 2 * h : h) || d->dst.g.w != (sub ? 2 * w : w)) return RRIN_E_SHAPE;
  const int cpr = chans_per_rec(d->prec);
  if (d->cin > cpr * d->src.groups || (sub ? d->cout / 4 : d->cout) > cpr * d->dst.groups) return RRIN_E_ARG;
  if (sub && ((d->cout & 31) || !d->edge)) return RRIN_E_ARG;
  if (!(d->slope >= 0.f && d->slope <= 1.f)) return RRIN_E_ARG;  // leaky() as max(t, slope t)
  if (d->epi_mode == RRIN_EPI_LEAKY_POOL) {
    if (!ci.pool_ok) return RRIN_E_CONFIG;  // a wave must own both rows of a pool pair
    if (!h8_ok(d->pool, d->prec) || (h & 1) || (w & 1) || d->pool.g.h * 2 != h || d->pool.g.w * 2 != w ||
        d->cout > cpr * d->pool.groups)
      return RRIN_E_SHAPE;
  }
  const int planes = planes_of(d->prec);
  memset(&a, 0, sizeof(a));
  const int64_t sg = (int64_t)d->src.g_off * d->src.g.plane;
  a.src_hi = static_cast<const uint4*>(d->src.hi) + sg;
  a.src_lo = planes == 2 ? static_cast<const uint4*>(d->src.lo) + sg : nullptr;
  a.src_img = d->src.img_stride;
  a.src_gp = d->src.g.plane;
  a.src_wp = d->src.g.wp;
  a.cin = d->cin;
  a.nchunks = (d->cin + 2 * cpr - 1) / (2 * cpr);  // 2 record groups per chunk
  const int64_t dg = (int64_t)d->dst.g_off * d->dst.g.plane;
  a.dst_hi = static_cast<uint4*>(d->dst.hi) + dg;
  a.dst_lo = planes == 2 ? static_cast<uint4*>(d->dst.lo) + dg : nullptr;
  a.dst_img = d->dst.img_stride;
  a.dst_gp = d->dst.g.plane;
  a.dst_wp = d->dst.g.wp;
  a.cout = d->cout;
  if (d->epi_mode == RRIN_EPI_LEAKY_POOL) {
    const int64_t pg = (int64_t)d->pool.g_off * d->pool.g.plane;
    a.pool_hi = static_cast<uint4*>(d->pool.hi) + pg;
    a.pool_lo = planes == 2 ? static_cast<uint4*>(d->pool.lo) + pg : nullptr;
    a.pool_img = d->pool.img_stride;
    a.pool_gp = d->pool.g.plane;
    a.pool_wp = d->pool.g.wp;
  }
  a.w_hi = static_cast<const uint4*>(d->whi);
  a.w_lo = planes == 2 ? static_cast<const uint4*>(d->wlo) : nullptr;
  a.bias = d->bias;
  a.inv_wscale = d->prec == RRIN_PREC_F32R ? 1.0f : d->inv_wscale;
  a.slope = d->slope;
  a.tail_finite = d->tail_finite;
  a.status = d->status;
  a.h = h;
  a.w = w;
  if (sub) {
    a.edge = d->edge;
    a.ring = ring_pixels(2 * h, 2 * w);
  }
  a.co_blocks = (d->cout + ci.bm - 1) / ci.bm;
  a.tiles_x = (w + 31) / 32;
  a.tiles_y = (h + ci.th - 1) / ci.th;
  if (wino && d->prec == RRIN_PREC_F16) {
    // fp16 Winograd (kind 6 only): 16-channel chunks of both record groups, no split / fold
    if (ci.kind != 6 || d->ksplit > 1 || d->ring_w) return RRIN_E_CONFIG;
    if ((d->cin & 15) && !d->tail_finite) return RRIN_E_CONFIG;
  } else if (wino) {
    if (d->prec != RRIN_PREC_F32R) return RRIN_E_CONFIG;
    if ((d->cin & 3) && !d->tail_finite) return RRIN_E_CONFIG;  // stages whole records only
    // the register-U tiles (kinds 6, 7, 14) stage both record groups of every chunk: they must exist
    if (ci.kind >= 6 && (d->cin & 7) && !d->tail_finite) return RRIN_E_CONFIG;
    a.nchunks = (d->cin + 7) / 8;  // two record groups per K chunk
  }
  // the Winograd tiles stage every record group of every chunk (past cin against zero
  // weights): the source view must hold them, or the staging reads past the tensor
  if (wino && 2 * a.nchunks > d->src.groups) return RRIN_E_SHAPE;
  {
    // LDS-DMA staging addresses the source through buffer resources (num_records 2^31 - 1) with
    // 32-bit byte offsets: the direct-form tiles from one base per image (every staged record
    // group of the image), the Winograd tiles from one base per tile and chunk (two groups).  A
    // larger span would stage zeros past the range -- a wrong result with no error -- so it is
    // rejected (a 64-channel fp16 view passes 2 GB near 6144x3456).
    const bool dma = wino || d->cin % 8 == 0 || d->tail_finite;
    const int64_t span_groups = wino ? 3 : 2 * (int64_t)a.nchunks;
    if (dma && span_groups * d->src.g.plane * 16 >= ((int64_t)1 << 31)) return RRIN_E_SHAPE;
  }
  a.n = d->n;
  if ((int64_t)a.co_blocks * a.tiles_x * a.tiles_y * a.n > 0x7fffffff) return RRIN_E_SHAPE;
  a.ksplit = 1;
  if (d->ksplit > 1) {  // Winograd split-K: kinds 3 and 4 only
    if (ci.kind != 3 && ci.kind != 4) return RRIN_E_CONFIG;
    if (d->ksplit > kMaxKSplit || (need_scratch && (!d->part || !d->cnt))) return RRIN_E_ARG;
    a.kper = (a.nchunks + d->ksplit - 1) / d->ksplit;
    a.ksplit = (a.nchunks + a.kper - 1) / a.kper;  // every slice non-empty
    if ((int64_t)a.co_blocks * a.tiles_x * a.tiles_y * a.n * a.ksplit > 0x7fffffff) return RRIN_E_SHAPE;
    a.part = d->part;
    a.cnt = d->cnt;
  }
  if (d->ring_w) {  // sub-pixel ring fold (kind 3, unsplit): no separate edge fix-up launch
    if (!sub || ci.kind != 3 || a.ksplit > 1) return RRIN_E_CONFIG;
    if ((d->cin & 7) || !d->ring_bias || (need_scratch && (!d->ring_corr || !d->ring_cnt))) return RRIN_E_ARG;
    a.nseg = 2 * a.tiles_x + 2 * a.tiles_y;
    const int64_t rb = (int64_t)a.n * a.co_blocks * a.nseg;
    if (rb + (int64_t)a.co_blocks * a.tiles_x * a.tiles_y * a.n > 0x7fffffff) return RRIN_E_SHAPE;
    a.nring = (int)((rb + 7) & ~(int64_t)7);  // keeps the tiles' XCD remap aligned
    const int64_t grid = (int64_t)a.co_blocks * a.tiles_x * a.tiles_y * a.n + a.nring;
    a.rstride = 8 * (int)(grid / a.nring);    // ring groups spread over the whole grid
    a.wedge = d->ring_w;
    a.bias_raw = d->ring_bias;
    a.corr = d->ring_corr;
    a.rcnt = d->ring_cnt;
  }
  if (d->ring_full) {  // the ring from scratch with this conv (ABI 17)
    const rrin_edge_fix_desc* e = d->ring_full;
    if (!sub || d->ring_w || e->full != 1 || e->prec != d->prec || e->n != d->n || e->cout * 4 != d->cout)
      return RRIN_E_ARG;
    dim3 g;
    if (int rc = edge_fix_prepare(e, a.fix, g)) return rc;
    if (a.fix.s_hi != a.src_hi || a.fix.sh != h || a.fix.sw != w) return RRIN_E_ARG;  // this conv's input
    a.fix_gx = (int)g.x;
    a.fix_gy = (int)g.y;
    const int64_t nf = (int64_t)g.x * g.y * g.z;
    if (nf + (int64_t)a.co_blocks * a.tiles_x * a.tiles_y * a.n + 8 > 0x7fffffff) return RRIN_E_SHAPE;
    a.fix_real = (int)nf;
  }
  return 0;
}

// info (rrin_conv_h8_launch_info): the launcher reports its launch shape and launches nothing
static int conv3x3_h8_launch(const rrin_conv_h8_desc* d, const ConvH8Args& a, hipStream_t st,
                             rrin_launch_info* info) {
  switch (kCfgH8[d->cfg].kind) {  // h8_prepare passed: a live config
    case 0: return launch_h8(a, d->cfg, d->prec, d->epi_mode, st, info);
    case 1: return launch_wino(a, d->epi_mode, st, info);
    case 3: return launch_winoq(a, d->epi_mode, 8, st, info);
    case 4: return launch_winoq(a, d->epi_mode, 4, st, info);
    case 6:
      return d->prec == RRIN_PREC_F16 ? launch_winoh(a, d->epi_mode, st, info)
                                      : launch_winoc(a, d->epi_mode, 2, st, info);
    case 7: return launch_winoc(a, d->epi_mode, 1, st, info);
    case 14: return launch_winoc42(a, d->epi_mode, st, info);
  }
  return RRIN_E_CONFIG;
}

bool ring_in_launch_ok(int cfg, int cin, int prec) {
  const CfgH8* c = h8_cfg(cfg);
  if (!c || c->kind < 0 || cin % kFixCi) return false;
  if (c->kind == 6 || c->kind == 7) return prec == RRIN_PREC_F32R;  // exact fp32: 256 threads
  if (c->kind > 0) return false;                                    // kinds 1, 3, 4, 14: the fix-up as a second launch
  return c->nt >= 256;                                              // direct-form tiles of 256 / 512 threads
}

}  // namespace rrin

using namespace rrin;

extern "C" int rrin_conv_h8_cfg_count(void) { return kNumCfgH8; }
extern "C" int rrin_conv_h8_cfg_bm(int32_t cfg) { return h8_cfg(cfg) ? h8_cfg(cfg)->bm : RRIN_E_CONFIG; }
extern "C" int rrin_conv_h8_cfg_th(int32_t cfg) { return h8_cfg(cfg) ? h8_cfg(cfg)->th : RRIN_E_CONFIG; }
// CfgH8::kind (0 outside the table)
extern "C" int rrin_conv_h8_cfg_wino(int32_t cfg) { return h8_cfg(cfg) ? h8_cfg(cfg)->kind : 0; }

extern "C" int rrin_conv_h8_cfg_ok(int32_t cfg, int32_t prec) {
  const CfgH8* c = h8_cfg(cfg);
  if (!c || !rec_prec(prec) || c->kind < 0) return 0;
  // Winograd tiles: exact fp32 records; the register-U kind 6 also at fp16 (conv_winoh.hip)
  if (c->kind > 0 && (prec == RRIN_PREC_F16 ? c->kind != 6 : prec != RRIN_PREC_F32R)) return 0;
  return (planes_of(prec) == 2 ? c->lds2 : c->lds1) <= kMaxLds ? 1 : 0;
}

extern "C" int rrin_conv_h8_cfg_fits(int32_t cfg, int32_t prec, int32_t cin) {
  if (!rrin_conv_h8_cfg_ok(cfg, prec) || cin < 1) return 0;
  const CfgH8& c = kCfgH8[cfg];
  const int nch = (cin + 2 * chans_per_rec(prec) - 1) / (2 * chans_per_rec(prec));
  if (!(c.sched & SCHED_WRES) || nch <= 2) return 1;
  const int planes = planes_of(prec);
  const size_t lds = (planes == 2 ? c.lds2 : c.lds1) + (size_t)(nch - 2) * c.wslab * planes;
  return lds <= kMaxLds ? 1 : 0;
}

// floats of rrin_conv_h8_desc.ring_corr and ints of .ring_cnt a ring-folding sub-pixel conv
// needs (0 and 0 when d->ring_w is NULL)
extern "C" int64_t rrin_conv_h8_ring_floats(const rrin_conv_h8_desc* d, int64_t* cnt_ints) {
  ConvH8Args a;
  const int rc = h8_prepare(d, a, false);
  if (rc) return rc;
  const int64_t segs = a.nring > 0 ? (int64_t)a.n * a.co_blocks * a.nseg : 0;
  if (cnt_ints) *cnt_ints = segs;
  return segs * 512;
}

// floats of rrin_conv_h8_desc.part and ints of .cnt a split-K conv needs (0 without a split)
extern "C" int64_t rrin_conv_h8_split_floats(const rrin_conv_h8_desc* d, int64_t* cnt_ints) {
  ConvH8Args a;
  const int rc = h8_prepare(d, a, false);
  if (rc) return rc;
  const int64_t tiles = (int64_t)a.co_blocks * a.tiles_x * a.tiles_y * a.n;
  if (cnt_ints) *cnt_ints = a.ksplit > 1 ? tiles : 0;
  return a.ksplit > 1 ? tiles * a.ksplit * 32 * 32 * kCfgH8[d->cfg].th : 0;  // 16 floats per thread of 64 x th threads
}

// Validate and dispatch: the forward call (info null), or its launch shape alone.
static int conv3x3_h8_run(const rrin_conv_h8_desc* d, void* stream, rrin_launch_info* info) {
  ConvH8Args a;
  const int rc = h8_prepare(d, a);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (a.fix_real > 0) {
    // in the conv's launch (a tile of 256 or 512 threads); otherwise the conv, then the FULL
    // fix-up as its own launch in the same summation order
    if (!ring_in_launch_ok(d->cfg, a.fix.cin, d->prec)) {
      ConvH8Args b = a;
      b.fix_real = 0;
      if (int e = conv3x3_h8_launch(d, b, st, info)) return e;
      if (info) return 0;  // the conv part alone: the ring is a launch of its own (extra 0)
      dim3 g((unsigned)a.fix_gx, (unsigned)a.fix_gy, (unsigned)d->n);
      return edge_fix_run(a.fix, g, d->prec, true, nullptr, st, true);  // the in-launch summation order
    }
  }
  return conv3x3_h8_launch(d, a, st, info);
}

extern "C" int rrin_conv3x3_h8_fwd(const rrin_conv_h8_desc* d, void* stream) {
  return conv3x3_h8_run(d, stream, nullptr);
}

extern "C" int rrin_conv_h8_launch_info(const rrin_conv_h8_desc* d, void* stream, rrin_launch_info* out) {
  if (!out) return RRIN_E_ARG;
  return conv3x3_h8_run(d, stream, out);
}

#ifdef RRIN_LAB
// Kernel lab (tools/conv_lab.py ablate; built only into librrin_lab.so, `make lab`): one LEAKY
// conv with schedule knobs / ablation bits `sched` -- a Winograd tile (launch_wino_lab), or a
// direct-form tile at F16X3 or F32R with grid `persist` (launch_h8_lab).
extern "C" int rrin_conv3x3_h8_lab(const rrin_conv_h8_desc* d, int32_t sched, int32_t persist, void* stream) {
  const bool wino = d && h8_cfg(d->cfg) && h8_cfg(d->cfg)->kind > 0 && d->epi_mode == RRIN_EPI_LEAKY;
  if (!wino) {
    if (!d || (d->prec != RRIN_PREC_F16X3 && d->prec != RRIN_PREC_F32R) || d->epi_mode != RRIN_EPI_LEAKY ||
        (d->cin % 8))
      return RRIN_E_ARG;
    if (d->prec == RRIN_PREC_F32R && (sched & SCHED_MFMA16)) return RRIN_E_CONFIG;
  }
  ConvH8Args a;
  const int rc = h8_prepare(d, a);
  if (rc) return rc;
  return wino ? launch_wino_lab(a, sched, (hipStream_t)stream)
              : launch_h8_lab(a, d->cfg, d->prec, sched, persist, (hipStream_t)stream);
}
#endif
