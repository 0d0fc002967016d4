// The forward of RRIN Net (reference model.py:32-65) as a host schedule: net_forward begins a call on
// the workspace plan (net_plan.hpp), packs the frames into the 16-channel Net buffer and runs the
// four U-Nets (unet_sched.hip) on the caller's stream, each head fused with the Net glue that feeds
// the next; with the steps of an item forward, a flow_scale forward and an extra plane around them.
// Also here: the entries on fp32 NCHW frames (rrin_net_fwd, rrin_net_scaled_fwd), the Net's size
// queries, rrin_make_geom, the ABI version and the error strings.
// Not here: any kernel; the byte-frame entries and their checks (net_frames.hip); the U-Net walks
// and the scratch layout (unet_sched.hip); the profiler entries (prof.hip); the weight packers
// (pack_h8.hip, pack_wino.hip).
#include "net_plan.hpp"

using namespace rrin;

namespace {

// Debug taps (rrin_net_desc.taps): where U-Net u's raw output goes, or NULL.
float* tap_of(const rrin_net_desc* nd, const UNetSpec& u) {
  if (!nd->taps) return nullptr;
  const int64_t px = (int64_t)nd->n * nd->h * nd->w;
  int64_t off = 0;
  for (const auto& v : kUNets) {
    if (&v == &u) return nd->taps + off;
    off += v.out_ch * px;
  }
  return nullptr;
}

// rrin_net_fwd: fp32 NCHW frames d.i0 / i1 in, d.out out (the record precisions; the planar one reads
// them itself)
FrameIO frame_io(const rrin_net_desc& d) {
  FrameIO f;
  f.pack = [&d](int m, const int32_t*, int, const PackTo& to) {
    return rrin_pack_g16_h8(d.i0, d.i1, m, to.g, to.prec, to.st);
  };
  f.store.out = d.out;
  return f;
}

// The planar fp32 forward (rrin_net_fwd alone; no items, flow_scale or plane): d->i0 / i1 into g16,
// the four U-Nets by run_unet.
int planar_forward(const rrin_net_desc* d, const Plan& p, hipStream_t st) {
  // x = cat(x0, x1) into g16 channels 0-5 (model.py:33)
  const rrin_pp gx0 = view(p.G, 0, 3);
  const rrin_pp gx1 = view(p.G, 3, 3);
  int rc = 0;
  {
    ProfScope ps(p.prof, st, RRIN_KIND_LAYOUT, 0.0);
    rc = rrin_nchw_to_pp(d->i0, d->n, 3, &gx0, st);
    if (!rc) rc = rrin_nchw_to_pp(d->i1, d->n, 3, &gx1, st);
    if (!rc && d->skip_flow) {  // Flow U-Net skipped: t-blend of the kept raw Flow
      const rrin_pp fr = view(p.FLOWRAW, 0, 4);
      const rrin_pp g16 = view(p.G, 0, 16);
      rc = rrin_flow_tblend_fwd(&fr, &g16, d->coef, d->n, st);
    }
  }
  int k = 0;
  for (int u = 0; u < 4 && !rc; ++u) {
    if (!(u == 0 && d->skip_flow))
      rc = run_unet(p, kUNets[u], d->convs + k, d->heads[u], HeadIO{d->coef, d->out, tap_of(d, kUNets[u])}, st);
    k += convs_of(kUNets[u].depth);
  }
  return rc;
}

// One forward on the record layouts: what its steps share.  pack is the frame pack into the
// full-size g16 (gall), at the pad multiple of the call.
struct RecordCall {
  const rrin_net_desc* d;
  const FrameIO& f;
  const Items& items;
  const Plan& p;  // the full-size plan
  hipStream_t st;
  const rrin_h8& gall;
  PackTo to;
  int pack(int m, const int32_t* map, int np) const { return f.pack(m, map, np, to); }
  int pairs() const { return items.map ? items.n_pairs : d->n; }
};

// The Flow phase of a flow_scale forward (fs: s = 2 or 4, record layouts only; checked by
// flow_scale_check), once per pair.  The Flow U-Net runs on a second plan pl at (h / s, w / s) with
// its own workspace, conv table and scratch -- its interior writes would land in the zero halos of
// the full-size plan's buffers -- and the range flag of this call: pack into the full-size g16,
// rrin_g16_downscale_h8 into the low-res g16, the Flow U-Net there, rrin_flow_upscale_h8 of its raw
// Flow into the full-size FLOWRAW; the blend of the kept raw Flow follows as for skip_flow.  A plain
// forward's pack is not repeated.
int flow_phase_scaled(const RecordCall& c, const rrin_flow_scale* fs, Plan& pl) {
  const rrin_net_desc* d = c.d;
  const Plan& p = c.p;
  const int nf = c.pairs();
  attach_scratch(pl, fs->scratch, fs->scratch_bytes, d->n, d->h / fs->s, d->w / fs->s, fs->convs, kUNets, 4);
  pl.n = nf;
  pl.prof = p.prof;
  pl.status = p.status;
  const rrin_h8 glow = hview(pl.G, 0, 16);
  {
    ProfScope ps(p.prof, c.st, RRIN_KIND_LAYOUT, 0.0);
    RRIN_TRY(c.pack(nf, nullptr, nf));
  }
  {
    ProfScope ps(p.prof, c.st, RRIN_KIND_LAYOUT, 0.0);
    RRIN_TRY(rrin_g16_downscale_h8(&c.gall, &glow, nf, fs->s, d->prec, c.st));
  }
  // its head also blends into the low-res g16 (channels 6-9, which the next downscale zeroes)
  RRIN_TRY(run_unet_h8(pl, kUNets[0], fs->convs, d->heads[0], HeadIO{d->coef, nullptr, nullptr}, c.st));
  ProfScope ps(p.prof, c.st, RRIN_KIND_LAYOUT, 0.0);
  const rrin_h8 frl = hview(pl.FLOWRAW, 0, 4), frh = hview(p.FLOWRAW, 0, 4);
  return rrin_flow_upscale_h8(&frl, &frh, nf, fs->s, d->prec, p.status, c.st);
}

// The Flow phase of an item forward (items.map, frame forwards only): the Flow U-Net once per pair.
// One plan, sized for the d->n items, serves both phases of the call, since no buffer's image stride
// depends on the batch: this phase packs the n_pairs pairs into images [0, n_pairs) of the Net
// buffer and runs the Flow U-Net on them alone, which leaves the pairs' raw Flow in FLOWRAW.
int flow_phase_items(const RecordCall& c) {
  Plan pf = c.p;
  pf.n = c.items.n_pairs;
  {
    ProfScope ps(c.p.prof, c.st, RRIN_KIND_LAYOUT, 0.0);
    RRIN_TRY(c.pack(c.items.n_pairs, nullptr, c.items.n_pairs));
  }
  // its head also blends into the pairs' images with the first items' coefficients: the item
  // pack below overwrites those channels
  return run_unet_h8(pf, kUNets[0], c.d->convs, c.d->heads[0], HeadIO{c.d->coef, nullptr, nullptr}, c.st);
}

// Pack plus t-blend, one profiler span: the d->n images of the call into the full-size g16 unless
// they are there already (packed) -- an item forward packs item k from the frames of pair map[k]
// into image k --, then, where the Flow U-Net does not run in the loop below (blend), Ft0 / Ft1 from
// the kept raw Flow: the skip_flow path, indexed by the map for items, which blends pair map[k]'s
// raw Flow with item k's coefficients.
int pack_and_blend(const RecordCall& c, bool packed, bool blend) {
  const rrin_net_desc* d = c.d;
  ProfScope ps(c.p.prof, c.st, RRIN_KIND_LAYOUT, 0.0);
  // x0, x1 into channels 0-5; channels 6-15 zeroed, so the first convs (cin 6/9/10)
  // can stage whole records (their tail channels are finite and meet zero weights)
  if (!packed) RRIN_TRY(c.pack(d->n, c.items.map, c.pairs()));
  if (!blend) return 0;
  const rrin_h8 fr = hview(c.p.FLOWRAW, 0, 4);
  return c.items.map
             ? rrin_flow_tblend_items_h8(&fr, &c.gall, d->coef, d->n, c.items.map, c.items.n_pairs, d->prec, c.st)
             : rrin_flow_tblend_h8(&fr, &c.gall, d->coef, d->n, d->prec, c.st);
}

// The U-Nets on the d->n images: all four, or the last three after a blend.  With pa (an extra
// plane, frame forwards only; checked by plane_of) rrin_plane_warp_h8 follows the REFINE head, the
// MASK head's raw output goes into the plane's scratch and rrin_plane_blend_h8 follows that head:
// two launches and one pointer, nothing else moves.
int unet_loop(const RecordCall& c, bool blend, const rrin_aux_plane* pa) {
  const rrin_net_desc* d = c.d;
  int k = 0;
  for (int u = 0; u < 4; ++u) {
    if (!(u == 0 && blend)) {
      HeadIO io = c.f.head_io(d->coef, tap_of(d, kUNets[u]), d->h);
      const int mode = kUNets[u].head_mode;
      if (pa && mode == RRIN_HEAD_MASK) io.raw = plane_logits(pa, d->n, d->h, d->w);
      RRIN_TRY(run_unet_h8(c.p, kUNets[u], d->convs + k, d->heads[u], io, c.st));
      if (pa && (mode == RRIN_HEAD_REFINE || mode == RRIN_HEAD_MASK)) {
        ProfScope ps(c.p.prof, c.st, RRIN_KIND_LAYOUT, 0.0);
        RRIN_TRY(mode == RRIN_HEAD_REFINE
                     ? rrin_plane_warp_h8(&c.gall, pa, d->n, c.f.h0, c.f.w0, c.items.map, c.pairs(), d->prec, c.st)
                     : rrin_plane_blend_h8(pa, d->coef, d->n, d->h, d->w, c.f.h0, c.f.w0, d->prec, c.p.status,
                                           c.st));
      }
    }
    k += convs_of(kUNets[u].depth);
  }
  return 0;
}

}  // namespace

namespace rrin {

// The second plan of a flow_scale forward (RRIN_E_ARG: null members, s not 2 or 4, taps, the planar
// precision; RRIN_E_SHAPE: a padded size that is no multiple of 16 * s).
int flow_scale_check(const rrin_net_desc* nd, const rrin_flow_scale* fs) {
  if (!nd || !fs || (fs->s != 2 && fs->s != 4) || !fs->convs || !fs->workspace || nd->taps) return RRIN_E_ARG;
  if (!record_prec(nd->prec)) return RRIN_E_ARG;
  if (nd->n < 1 || nd->h < 16 * fs->s || nd->w < 16 * fs->s || nd->h % (16 * fs->s) || nd->w % (16 * fs->s))
    return RRIN_E_SHAPE;
  return 0;
}

// The schedule of the forwards: rrin_net_fwd (fp32 NCHW frames d->i0 / i1 in, d->out out),
// rrin_net_u8_fwd (8-bit RGB frames in and out), rrin_net_yuv_fwd (8-bit 4:2:0 frames in and out)
// and their 16-bit siblings rrin_net_u16_fwd / rrin_net_yuv16_fwd; the frame forwards leave d->i0 /
// i1 / out unused and run on the record layouts only.  f is the frame_io of the entry's descriptor,
// which the callers have validated with d.  With a map (items.map) the call is an item forward,
// with fs a flow_scale forward, with pa it carries an extra plane: the steps above say how.
int net_forward(const rrin_net_desc* d, const FrameIO& f, const Items& items, void* stream,
                const rrin_flow_scale* fs, const rrin_aux_plane* pa) {
  hipStream_t st = (hipStream_t)stream;
  Plan pl;  // fs: the plan of the Flow phase at (h / s, w / s), sized for the d->n images
  if (fs) {
    make_plan(d->n, d->h / fs->s, d->w / fs->s, d->prec, reinterpret_cast<char*>(fs->workspace), pl);
    if (fs->workspace_bytes < pl.bytes) return RRIN_E_WORKSPACE;
  }
  Plan p;
  RRIN_TRY(begin_call(d, kUNets, 4, st, p));
  if (!record_prec(d->prec)) return planar_forward(d, p, st);

  const rrin_h8 gall = hview(p.G, 0, 16);
  const RecordCall c{d, f, items, p, st, gall, PackTo{&gall, d->prec, st, fs ? 16 * fs->s : 16}};
  bool packed = false;  // the full-size g16 already holds the d->n images of the call
  if (fs && !d->skip_flow) {
    RRIN_TRY(flow_phase_scaled(c, fs, pl));
    packed = !items.map;
  } else if (items.map && !d->skip_flow) {
    RRIN_TRY(flow_phase_items(c));
  }
  const bool blend = d->skip_flow || items.map || fs;  // Ft0 / Ft1 from the kept raw Flow
  RRIN_TRY(pack_and_blend(c, packed, blend));
  return unet_loop(c, blend, pa);
}

}  // namespace rrin

extern "C" int rrin_net_fwd(const rrin_net_desc* d, void* stream) {
  if (!d || !d->i0 || !d->i1 || !d->out || !d->coef || !d->convs || !d->heads || !d->workspace)
    return RRIN_E_ARG;
  if (!padded_shape_ok(d->n, d->h, d->w)) return RRIN_E_SHAPE;
  if (!prec_ok(d->prec)) return RRIN_E_ARG;
  return net_forward(d, frame_io(*d), Items{}, stream);
}

extern "C" int rrin_net_scaled_fwd(const rrin_net_desc* d, const rrin_flow_scale* fs, void* stream) {
  if (int rc = flow_scale_check(d, fs)) return rc;
  if (!d->i0 || !d->i1 || !d->out || !d->coef || !d->convs || !d->heads || !d->workspace) return RRIN_E_ARG;
  return net_forward(d, frame_io(*d), Items{}, stream, fs);
}

extern "C" int64_t rrin_net_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t prec) {
  if (!padded_shape_ok(n, h, w)) return RRIN_E_SHAPE;
  if (!prec_ok(prec)) return RRIN_E_ARG;
  Plan p;
  make_plan(n, h, w, prec, nullptr, p);
  return p.bytes;
}

extern "C" int64_t rrin_net_scratch_bytes(const rrin_net_desc* d) {
  if (!d || !d->convs) return RRIN_E_ARG;
  if (!padded_shape_ok(d->n, d->h, d->w)) return RRIN_E_SHAPE;
  if (!prec_ok(d->prec)) return RRIN_E_ARG;
  ScratchLayout s;
  RRIN_TRY(scratch_layout(d->n, d->h, d->w, d->prec, d->convs, kUNets, 4, s));
  return s.bytes;
}

extern "C" int rrin_make_geom(int32_t h, int32_t w, rrin_geom* g) {
  if (!g || h < 1 || w < 1) return RRIN_E_ARG;
  *g = make_geom(h, w);
  return 0;
}

extern "C" int rrin_abi_version(void) { return RRIN_ABI_VERSION; }

extern "C" const char* rrin_strerror(int code) {
  switch (code) {
    case RRIN_OK:
      return "ok";
    case RRIN_E_SHAPE:
      return "rrin: shape precondition violated (H, W must be multiples of 16; N >= 1; views must match)";
    case RRIN_E_ARG:
      return "rrin: invalid argument (null pointer, mode or channel range)";
    case RRIN_E_WORKSPACE:
      return "rrin: workspace smaller than rrin_net_workspace_bytes() (or scratch smaller than "
             "rrin_net_scratch_bytes())";
    case RRIN_E_CONFIG:
      return "rrin: unknown conv tile config";
  }
  if (code > 0) return hipGetErrorString((hipError_t)code);
  return "rrin: unknown error";
}
