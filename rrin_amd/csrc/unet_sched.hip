// The schedule of one U-Net (reference unet.py:40-51) on a workspace plan: the per-conv descriptor
// builders (conv, conv_h8, block0_h8, upconv_subpixel), the two walks -- run_unet on the planar
// fp32 layout (the first implementation, frozen) and run_unet_h8 on the record layouts --, the
// scratch layout, which is run_unet_h8 walked dry, and the U-Net's own entries (rrin_unet_*).
// Host code only: every kernel is behind an rrin_*_fwd entry of another file.  The Net's forward,
// which strings four of these walks together, is net.hip; the plan itself is net_plan.hpp.
#include "net_plan.hpp"

using namespace rrin;

namespace {

int conv(const Plan& p, const rrin_conv_weights& cw, int cin, int cout, int src_mode, int epi,
         const rrin_pp& src, const rrin_pp& dst, const rrin_pp* pool, hipStream_t st) {
  ProfScope ps(p.prof, st, RRIN_KIND_CONV, 2.0 * 9 * cin * cout * (double)dst.g.h * dst.g.w * p.n);
  rrin_conv_desc d;
  memset(&d, 0, sizeof(d));
  d.n = p.n;
  d.cin = cin;
  d.cout = cout;
  d.cfg = cw.cfg;
  d.src_mode = src_mode;
  d.epi_mode = epi;
  d.slope = 0.1f;
  d.src = src;
  d.dst = dst;
  if (pool) d.pool = *pool;
  d.wpack = cw.wpack;
  d.bias = cw.bias;
  return rrin_conv3x3_fwd(&d, st);
}

int conv_h8(const Plan& p, const rrin_conv_weights& cw, int cin, int cout, int epi, const rrin_h8& src,
            const rrin_h8& dst, const rrin_h8* pool, hipStream_t st, float* edge = nullptr, bool ring_fold = false,
            const rrin_edge_fix_desc* ring_full = nullptr) {
  // algorithmic FLOPs of the conv (a sub-pixel conv has 4 phase rows per real channel): 9
  // multiply-adds per output and input channel in the direct form, 4 in Winograd F(2x2,3x3)
  // (16 per 2x2 patch), 3 in F(4,3) x F(2,3) (kind 14: 24 per 4 x 2 patch)
  const int creal = epi == RRIN_EPI_SUBPIXEL ? cout / 4 : cout;
  const int wkind = rrin_conv_h8_cfg_wino(cw.cfg);
  const int macs = wkind == 14 ? 3 : wkind ? 4 : 9;
  ProfScope ps(p.prof, st, RRIN_KIND_CONV, 2.0 * macs * cin * creal * (double)dst.g.h * dst.g.w * p.n);
  rrin_conv_h8_desc d;
  memset(&d, 0, sizeof(d));
  d.n = p.n;
  d.cin = cin;
  d.cout = cout;
  d.cfg = cw.cfg;
  d.prec = p.prec;
  d.epi_mode = epi;
  d.slope = 0.1f;
  d.inv_wscale = cw.inv_wscale;
  d.tail_finite = 1;  // every src of the schedule: cin % 8 == 0, or g16 whose tail channels are finite
  d.src = src;
  d.dst = dst;
  if (pool) d.pool = *pool;
  d.whi = cw.whi;
  d.wlo = cw.wlo;
  d.bias = cw.bias;
  d.edge = edge;
  d.status = p.status;
  d.ring_full = ring_full;
  if (ring_fold) {
    d.ring_w = cw.wedge;
    d.ring_bias = cw.bias_raw;
    d.ring_corr = p.RCORR;
    d.ring_cnt = p.RCNT;
    int64_t cnt = 0;
    const int64_t need = rrin_conv_h8_ring_floats(&d, &cnt);
    if (need < 0) return (int)need;
    if (need > p.rcorr_floats || cnt > p.rcnt_ints) return RRIN_E_CONFIG;
  }
  if (cw.ksplit > 1 && p.prec == RRIN_PREC_F32R) {
    d.ksplit = cw.ksplit;
    d.part = p.PART;
    d.cnt = p.CNT;
    int64_t cnt = 0;
    const int64_t need = rrin_conv_h8_split_floats(&d, &cnt);
    if (need < 0) return (int)need;
    if (p.dry) {
      p.dry->add(need, cnt);
    } else if (!p.PART || need > p.part_floats || cnt > p.cnt_ints) {
      return RRIN_E_WORKSPACE;  // scratch smaller than rrin_net_scratch_bytes
    }
  }
  if (p.dry) return 0;
  return rrin_conv3x3_h8_fwd(&d, st);
}

// Fused level-0 UNetConvBlock (conv a = ca: cin -> 32, conv b = cb: 32 -> 32, + pool): one
// rrin_conv_block0_h8_fwd launch, bitwise the two conv_h8 calls it replaces
int block0_h8(const Plan& p, const rrin_conv_weights& ca, const rrin_conv_weights& cb, int cin, const rrin_h8& src,
              const rrin_h8& dst, const rrin_h8* pool, hipStream_t st) {
  ProfScope ps(p.prof, st, RRIN_KIND_CONV, 2.0 * 9 * (cin * 32 + 32 * 32) * (double)dst.g.h * dst.g.w * p.n);
  rrin_block0_h8_desc d;
  memset(&d, 0, sizeof(d));
  d.n = p.n;
  d.cin = cin;
  d.cfg_a = ca.cfg;
  d.cfg_b = cb.cfg;
  d.slope = 0.1f;
  d.inv_wscale_a = ca.inv_wscale;
  d.inv_wscale_b = cb.inv_wscale;
  d.tail_finite = 1;  // as conv_h8
  d.src = src;
  d.dst = dst;
  if (pool) d.pool = *pool;
  d.whi_a = ca.whi;
  d.bias_a = ca.bias;
  d.whi_b = cb.whi;
  d.bias_b = cb.bias;
  d.status = p.status;
  if (p.dry) return 0;
  return rrin_conv_block0_h8_fwd(&d, st);
}

// ring fix-up: cross-workgroup K split up to this many workgroups (one per CU)
constexpr int64_t kEdgeCrossMaxGroups = 256;

// up.1 conv of the up block at level L on the sub-pixel path: low-res x (2C ch,
// edge-replicated) -> CAT[L][0, C), and the ring pixels: fp16 / split16 from scratch in the conv's
// own launch (ring_full), exact fp32 by the correction of the conv's pre-bias ring values (the
// outside taps of the zero-padded upsampled image) as a second launch on the same stream.  Round 5
// measured the ring from scratch beside the conv on a side stream and after it: both lost
// (DESIGN.md §5e).
//
// fp16 / split16: the ring from scratch (ABI 17 ring_full), inside the conv's launch where the
// tile allows it (direct-form tiles of 256 / 512 threads; ring_in_launch_ok), else as a second
// launch in the same summation order: every size class gets the same ring bits.  Exact fp32 keeps
// the correction launch (its K-split form on small grids: C2 339.6-339.7 vs 334.4-334.6 pairs/s
// with the ring in the Winograd launch, headline +0.3 %; profiles/r06/ring/).
int upconv_subpixel(const Plan& p, const rrin_conv_weights& cw, int C, const rrin_h8& x, const rrin_h8& up,
                    hipStream_t st) {
  if (cw.subpixel == 2) {  // ring folded into the conv (Winograd kind 3, no split)
    if (!p.RCORR || rrin_conv_h8_cfg_wino(cw.cfg) != 3 || cw.ksplit > 1) return RRIN_E_CONFIG;
    return conv_h8(p, cw, 2 * C, 4 * C, RRIN_EPI_SUBPIXEL, x, up, nullptr, st, p.EDGE, true);
  }
  rrin_edge_fix_desc e;
  memset(&e, 0, sizeof(e));
  e.n = p.n;
  e.cin = 2 * C;
  e.cout = C;
  e.prec = p.prec;
  e.epi_mode = RRIN_EPI_LINEAR;
  e.src = x;
  e.dst = up;
  e.edge = p.EDGE;
  e.wedge = cw.wedge;
  e.bias = cw.bias_raw;
  e.status = p.status;
  e.full = 0;
  if (p.prec != RRIN_PREC_F32R && (2 * C) % kFixCi == 0) {
    // the ring from scratch (ABI 17 ring_full): where the tile allows, extra workgroups of the
    // conv's own launch -- no separate fix-up launch and no dependency step on this stream (C3:
    // the separate fix-ups cost ~3.5 %, profiles/r06/ring/)
    e.full = 1;
    return conv_h8(p, cw, 2 * C, 4 * C, RRIN_EPI_SUBPIXEL, x, up, nullptr, st, p.EDGE, false, &e);
  }
  RRIN_TRY(conv_h8(p, cw, 2 * C, 4 * C, RRIN_EPI_SUBPIXEL, x, up, nullptr, st, p.EDGE));
  // F32R plans: the cross-workgroup K split (the same result bit for bit) where the
  // split grid is at most one workgroup per CU -- the latency-bound small grids
  // (640x368 x 1: fix-up 195 -> 129 us per forward); larger grids keep one
  // workgroup per tile, whose extra workgroups only queue behind the other
  // stream's convs (720p x 4 on 2 streams: fix-up span 1.4 -> 3.5 ms per step).
  if (p.prec == RRIN_PREC_F32R) {
    int64_t tk = 0;
    const int64_t nf = rrin_edge_fix_split_floats(&e, &tk);
    if (nf > 0 && nf / 1024 <= kEdgeCrossMaxGroups) {
      if (p.dry) {
        p.dry->add(nf, tk);
      } else if (p.PART && nf <= p.part_floats && tk <= p.cnt_ints) {
        e.part = p.PART;
        e.cnt = p.CNT;
        e.part_floats = p.part_floats;
        e.cnt_len = (int32_t)p.cnt_ints;
      }
    }
  }
  if (p.dry) return 0;
  ProfScope ps(p.prof, st, RRIN_KIND_EDGE, 0.0);
  return rrin_subpixel_edge_fix_h8(&e, st);
}

// conv cw (a level-0 conv a) runs fused with the next conv: fp16, asked for by the table
bool fused_block0(const Plan& p, const rrin_conv_weights& cw) {
  return p.prec == RRIN_PREC_F16 && cw.fuse_next == 1;
}

// The checks rrin_unet_scratch_bytes and rrin_unet_fwd share once their pointers are there, in the
// order of the codes they return, and the U-Net they describe
int unet_check(const rrin_unet_desc* d, UNetSpec& u) {
  if (!padded_shape_ok(d->n, d->h, d->w)) return RRIN_E_SHAPE;
  if (d->in_ch < 1 || d->in_ch > 16 || d->out_ch < 2 || d->out_ch > 4 || d->depth < 2 || d->depth > kMaxDepth)
    return RRIN_E_ARG;
  if (!prec_ok(d->prec)) return RRIN_E_ARG;
  u = UNetSpec{d->in_ch, d->out_ch, d->depth, RRIN_HEAD_PLAIN};
  return 0;
}

}  // namespace

namespace rrin {

// One U-Net (unet.py:40-51) from g16 channels [0, in_ch) to its head.
int run_unet(const Plan& p, const UNetSpec& u, const rrin_conv_weights* cw, const rrin_head_weights& hw,
             const HeadIO& io, hipStream_t st) {
  const int D = u.depth;
  int k = 0;
  // ---- down path (unet.py:42-46)
  for (int L = 0; L < D; ++L) {
    const int C = chans(L);
    const rrin_pp in = L ? view(p.X[L], 0, chans(L - 1)) : view(p.G, 0, u.in_ch);
    const int cin = L ? chans(L - 1) : u.in_ch;
    const rrin_pp t = view(p.T[L], 0, C);
    RRIN_TRY(conv(p, cw[k++], cin, C, RRIN_SRC_DIRECT, RRIN_EPI_LEAKY, in, t, nullptr, st));
    if (L < D - 1) {
      const rrin_pp bridge = view(p.CAT[L], C, C);  // cat's second half (unet.py:93)
      const rrin_pp pooled = view(p.X[L + 1], 0, C);
      RRIN_TRY(conv(p, cw[k++], C, C, RRIN_SRC_DIRECT, RRIN_EPI_LEAKY_POOL, t, bridge, &pooled, st));
    } else {
      const Buf& bot = (L == kMaxDepth - 1) ? p.BOT : p.CAT[L];  // CAT[3] is free at depth 4
      RRIN_TRY(conv(p, cw[k++], C, C, RRIN_SRC_DIRECT, RRIN_EPI_LEAKY, t, view(bot, 0, C), nullptr, st));
      // midconv + leaky (unet.py:47) back into T[bottom]
      RRIN_TRY(conv(p, cw[k++], C, C, RRIN_SRC_DIRECT, RRIN_EPI_LEAKY, view(bot, 0, C), t, nullptr, st));
    }
  }
  // ---- up path (unet.py:48-49, 72-95)
  rrin_pp x = view(p.T[D - 1], 0, chans(D - 1));
  for (int L = D - 2; L >= 0; --L) {
    const int C = chans(L);
    const rrin_pp up = view(p.CAT[L], 0, C);
    RRIN_TRY(conv(p, cw[k++], chans(L + 1), C, RRIN_SRC_UPSAMPLE2X, RRIN_EPI_LINEAR, x, up, nullptr, st));
    const rrin_pp cat = view(p.CAT[L], 0, 2 * C);
    const rrin_pp t = view(p.T[L], 0, C);
    RRIN_TRY(conv(p, cw[k++], 2 * C, C, RRIN_SRC_DIRECT, RRIN_EPI_LEAKY, cat, t, nullptr, st));
    RRIN_TRY(conv(p, cw[k++], C, C, RRIN_SRC_DIRECT, RRIN_EPI_LEAKY, t, up, nullptr, st));  // U_L
    x = up;
  }
  // ---- last conv fused with the Net glue (unet.py:51 + model.py)
  rrin_head_desc hd;
  memset(&hd, 0, sizeof(hd));
  hd.n = p.n;
  hd.cin = 32;
  hd.cout = u.out_ch;
  hd.mode = u.head_mode;
  hd.src = x;
  hd.g16 = view(p.G, 0, 16);
  hd.w = hw.w;
  hd.bias = hw.bias;
  hd.coef = io.coef;
  hd.out = io.out;
  hd.raw_out = io.raw;
  if (u.head_mode == RRIN_HEAD_FLOW) hd.flow_raw = view(p.FLOWRAW, 0, 4);
  ProfScope ps(p.prof, st, RRIN_KIND_HEAD, 2.0 * 9 * 32 * u.out_ch * (double)x.g.h * x.g.w * p.n);
  return rrin_head_fwd(&hd, st);
}

// One U-Net on the split-fp16 path: same dataflow as run_unet.  An up conv
// either has sub-pixel weights (upsample folded into the conv; its producer then
// writes the low-res tensor into LRB with edge-replicate padding) or runs after
// an explicit upsample pass into UPT.
int run_unet_h8(const Plan& p, const UNetSpec& u, const rrin_conv_weights* cw, const rrin_head_weights& hw,
                const HeadIO& io, hipStream_t st) {
  const int D = u.depth;
  int k = 0;
  rrin_h8 x;
  for (int L = 0; L < D; ++L) {
    const int C = chans(L);
    const int cin = L ? chans(L - 1) : u.in_ch;
    // level 0 views all 16 staged channels of G (zero past in_ch): Winograd tiles read whole chunks
    const rrin_h8 in = L ? hview(p.X[L], 0, cin) : hview(p.G, 0, 16);
    const rrin_h8 t = hview(p.T[L], 0, C);
    if (L == 0 && D >= 2 && fused_block0(p, cw[k])) {  // down_path[0] in one launch
      const rrin_h8 bridge = hview(p.CAT[0], C, C);
      const rrin_h8 pooled = hview(p.X[1], 0, C);
      RRIN_TRY(block0_h8(p, cw[k], cw[k + 1], cin, in, bridge, &pooled, st));
      k += 2;
      continue;
    }
    RRIN_TRY(conv_h8(p, cw[k++], cin, C, RRIN_EPI_LEAKY, in, t, nullptr, st));
    if (L < D - 1) {
      const rrin_h8 bridge = hview(p.CAT[L], C, C);
      const rrin_h8 pooled = hview(p.X[L + 1], 0, C);
      RRIN_TRY(conv_h8(p, cw[k++], C, C, RRIN_EPI_LEAKY_POOL, t, bridge, &pooled, st));
    } else {
      const Buf& bot = (L == kMaxDepth - 1) ? p.BOT : p.CAT[L];
      RRIN_TRY(conv_h8(p, cw[k++], C, C, RRIN_EPI_LEAKY, t, hview(bot, 0, C), nullptr, st));
      // midconv; cw[k + 1] is the first up conv
      const bool sub = D >= 2 && cw[k + 1].subpixel;
      x = sub ? hview(p.LRB[L], 0, C) : t;
      RRIN_TRY(conv_h8(p, cw[k++], C, C, sub ? RRIN_EPI_LEAKY_REP : RRIN_EPI_LEAKY, hview(bot, 0, C), x, nullptr,
                       st));
    }
  }
  for (int L = D - 2; L >= 0; --L) {
    const int C = chans(L);
    const rrin_h8 up = hview(p.CAT[L], 0, C);
    const rrin_conv_weights& cu = cw[k++];
    if (cu.subpixel) {
      RRIN_TRY(upconv_subpixel(p, cu, C, x, up, st));
    } else {
      const rrin_h8 upin = hview(p.UPT[L], 0, 2 * C);
      if (!p.dry) {
        ProfScope ps(p.prof, st, RRIN_KIND_LAYOUT, 0.0);
        RRIN_TRY(rrin_upsample2x_h8(&x, &upin, p.n, p.prec, st));
      }
      RRIN_TRY(conv_h8(p, cu, 2 * C, C, RRIN_EPI_LINEAR, upin, up, nullptr, st));
    }
    const rrin_h8 cat = hview(p.CAT[L], 0, 2 * C);
    const rrin_h8 t = hview(p.T[L], 0, C);
    if (L == 0 && fused_block0(p, cw[k])) {  // the last up block's conv_block in one launch: its
      // output goes to T[0] (the launch reads all of CAT[0] while it writes)
      RRIN_TRY(block0_h8(p, cw[k], cw[k + 1], 2 * C, cat, t, nullptr, st));
      k += 2;
      x = t;
      continue;
    }
    RRIN_TRY(conv_h8(p, cw[k++], 2 * C, C, RRIN_EPI_LEAKY, cat, t, nullptr, st));
    // conv b; cw[k + 1] is the next level's up conv
    const bool sub = L > 0 && cw[k + 1].subpixel;
    const rrin_h8 out = sub ? hview(p.LRB[L], 0, C) : up;
    RRIN_TRY(conv_h8(p, cw[k++], C, C, sub ? RRIN_EPI_LEAKY_REP : RRIN_EPI_LEAKY, t, out, nullptr, st));
    x = out;
  }
  rrin_head_h8_desc hd;
  memset(&hd, 0, sizeof(hd));
  hd.n = p.n;
  hd.cin = 32;
  hd.cout = u.out_ch;
  hd.mode = u.head_mode;
  hd.prec = p.prec;
  hd.src = x;
  hd.g16 = hview(p.G, 0, 16);
  hd.w = hw.w;
  hd.bias = hw.bias;
  hd.coef = io.coef;
  hd.out = io.out;
  hd.raw_out = io.raw;
  hd.status = p.status;
  if (u.head_mode == RRIN_HEAD_FINAL && (io.out_u8 || io.out_yuv || io.out_u16 || io.out_yuv16)) {
    hd.out_u8 = io.out_u8;
    hd.out_u16 = io.out_u16;
    hd.u16_depth = io.u16_depth;
    if (io.out_yuv) {
      hd.out_yuv = *io.out_yuv;
      hd.yuv_coef = *io.yuv_coef;
    }
    if (io.out_yuv16) {
      hd.out_yuv16 = *io.out_yuv16;
      hd.yuv_coef = *io.yuv_coef;
    }
    hd.h0 = io.h0;
    hd.w0 = io.w0;
    hd.top = io.top;
  }
  if (u.head_mode == RRIN_HEAD_FLOW) hd.flow_raw = hview(p.FLOWRAW, 0, 4);
  if (p.dry) return 0;
  ProfScope ps(p.prof, st, RRIN_KIND_HEAD, 2.0 * 9 * 32 * u.out_ch * (double)x.g.h * x.g.w * p.n);
  return rrin_head_h8_fwd(&hd, st);
}

// Scratch the schedule needs (F32R: the split convs' slabs and tickets, the ring fix-up's
// cross-workgroup K split; other precisions none): the schedule walked with every launch skipped.
int scratch_layout(int n, int h, int w, int prec, const rrin_conv_weights* convs, const UNetSpec* us, int nu,
                   ScratchLayout& out) {
  out = ScratchLayout{};
  if (prec != RRIN_PREC_F32R) return 0;
  Plan p;
  // a stand-in base so the views pass the descriptor checks; never dereferenced
  make_plan(n, h, w, prec, reinterpret_cast<char*>((uintptr_t)1 << 30), p);
  ScratchNeed need;
  p.dry = &need;
  const rrin_head_weights hw{};
  int k = 0;
  for (int u = 0; u < nu; ++u) {
    RRIN_TRY(run_unet_h8(p, us[u], convs + k, hw, HeadIO{nullptr, nullptr, nullptr}, nullptr));
    k += convs_of(us[u].depth);
  }
  out.tickets = scratch_tickets(need.cnt_ints);
  if (need.part_floats || need.cnt_ints) out.bytes = out.tickets * 4 + need.part_floats * 4;
  return 0;
}

}  // namespace rrin

extern "C" int rrin_net_conv_count(void) {
  int c = 0;
  for (const auto& u : kUNets) c += convs_of(u.depth);
  return c;
}

// One U-Net alone (reference UNet.forward, unet.py:40-51): NCHW in -> NCHW out,
// the same kernels and workspace plan as the Net (input in the Net buffer's
// channels [0, in_ch), head in PLAIN mode with its raw NCHW output as y).
extern "C" int64_t rrin_unet_conv_count(int32_t depth) {
  return (depth < 2 || depth > kMaxDepth) ? RRIN_E_ARG : convs_of(depth);
}

extern "C" int64_t rrin_unet_scratch_bytes(const rrin_unet_desc* d) {
  if (!d || !d->convs) return RRIN_E_ARG;
  UNetSpec u;
  RRIN_TRY(unet_check(d, u));
  ScratchLayout s;
  RRIN_TRY(scratch_layout(d->n, d->h, d->w, d->prec, d->convs, &u, 1, s));
  return s.bytes;
}

extern "C" int rrin_unet_fwd(const rrin_unet_desc* d, void* stream) {
  if (!d || !d->x || !d->y || !d->convs || !d->head.w || !d->head.bias || !d->workspace) return RRIN_E_ARG;
  UNetSpec u;
  RRIN_TRY(unet_check(d, u));
  hipStream_t st = (hipStream_t)stream;
  Plan p;
  RRIN_TRY(begin_call(d, &u, 1, st, p));
  const HeadIO io{nullptr, nullptr, d->y};
  int rc;
  {
    ProfScope ps(p.prof, st, RRIN_KIND_LAYOUT, 0.0);
    if (d->prec == RRIN_PREC_F32) {
      const rrin_pp gx = view(p.G, 0, d->in_ch);
      rc = rrin_nchw_to_pp(d->x, d->n, d->in_ch, &gx, st);
    } else {
      const rrin_h8 gx = hview(p.G, 0, 16);
      rc = rrin_nchw_to_h8(d->x, d->n, d->in_ch, 0, &gx, d->prec, st);
      // the PLAIN head writes its out_ch channels into this buffer: past in_ch
      // they would be staged (against zero weights) by the next call's first conv
      if (!rc && d->out_ch > d->in_ch) rc = clear_channels_h8(&gx, d->n, d->in_ch, d->out_ch, d->prec, st);
    }
  }
  if (rc) return rc;
  return d->prec == RRIN_PREC_F32 ? run_unet(p, u, d->convs, d->head, io, st)
                                  : run_unet_h8(p, u, d->convs, d->head, io, st);
}
