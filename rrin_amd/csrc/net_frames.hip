// The byte-frame entries of the Net forward: for each of the four frame formats (8-bit RGB, 8-bit
// YUV, 16-bit RGB, 16-bit YUV) its FrameIO -- the frame pack and the members of the FINAL store --,
// its argument checks, and its four entries rrin_net_*_fwd, _items_fwd, _scaled_fwd and _plane_fwd.
// Everything here runs before the first launch and ends in net_forward (net.hip), which holds the
// schedule; the pack and store kernels themselves are behind pack_g16_*_items (glue_h8.hip, yuv.hip)
// and the record-layout head.  The entries on fp32 NCHW frames are net.hip's.
#include "net_plan.hpp"
#include "yuv.hpp"

using namespace rrin;

namespace {

FrameIO frame_io(const rrin_net_u8_desc& d) {
  FrameIO f{d.h0, d.w0};
  f.pack = [&d](int m, const int32_t* map, int np, const PackTo& to) {
    return pack_g16_u8_items(d.f0, d.f1, d.img_stride, m, d.h0, d.w0, to.g, to.prec, map, np, to.st, to.mult);
  };
  f.store.out_u8 = d.out_u8;
  return f;
}

FrameIO frame_io(const rrin_net_yuv_desc& d) {
  FrameIO f{d.h0, d.w0};
  f.pack = [&d](int m, const int32_t* map, int np, const PackTo& to) {
    return pack_g16_yuv_items(&d.f0, &d.f1, &d.coef, m, d.h0, d.w0, to.g, to.prec, map, np, to.st, to.mult);
  };
  f.store.out_yuv = &d.out;
  f.store.yuv_coef = &d.coef;
  return f;
}

FrameIO frame_io(const rrin_net_u16_desc& d) {
  FrameIO f{d.h0, d.w0};
  f.pack = [&d](int m, const int32_t* map, int np, const PackTo& to) {
    return pack_g16_u16_items(d.f0, d.f1, d.img_stride, m, d.h0, d.w0, d.depth, to.g, to.prec, map, np, to.st,
                              to.mult);
  };
  f.store.out_u16 = d.out_u16;
  f.store.u16_depth = d.depth;
  return f;
}

FrameIO frame_io(const rrin_net_yuv16_desc& d) {
  FrameIO f{d.h0, d.w0};
  f.pack = [&d](int m, const int32_t* map, int np, const PackTo& to) {
    return pack_g16_yuv16_items(&d.f0, &d.f1, &d.coef, m, d.h0, d.w0, to.g, to.prec, map, np, to.st, to.mult);
  };
  f.store.out_yuv16 = &d.out;
  f.store.yuv_coef = &d.coef;
  return f;
}

// rrin_items of a forward of n items, checked: RRIN_E_ARG for a null descriptor, n_pairs outside
// [1, n], or no map with n_pairs != n
int items_of(const rrin_items* it, int n, Items& out) {
  if (!it || it->n_pairs < 1 || it->n_pairs > n) return RRIN_E_ARG;
  if (!it->pair_map && it->n_pairs != n) return RRIN_E_ARG;
  out.n_pairs = it->n_pairs;
  out.map = it->pair_map;
  return 0;
}

// The argument checks of the frame forwards, shared with their item forms: `frames` is the number
// of frames of f0 and of f1 -- net.n for a plain forward, the pairs of an item forward -- and the
// output always holds net.n frames.  net_check is what every format shares, in the order of the
// codes it returns: the null members of net and the record precisions (RRIN_E_ARG: the planar fp32
// path has no frame pack / store), then the format's own checks `own`, then the padded size against
// the pad multiple (RRIN_E_SHAPE).
template <class Own>
int net_check(const rrin_net_desc* nd, int h0, int w0, int mult, Own own) {
  if (!nd->coef || !nd->convs || !nd->heads || !nd->workspace) return RRIN_E_ARG;
  if (!record_prec(nd->prec)) return RRIN_E_ARG;
  if (int rc = own()) return rc;
  if (nd->h != pad_up(h0, mult) || nd->w != pad_up(w0, mult)) return RRIN_E_SHAPE;
  return 0;
}

// interleaved RGB frames (8 or 16 bit): ok = the format's pointers (and depth) are there
int net_rgb_check(bool ok, const rrin_net_desc* nd, int h0, int w0, int64_t img_stride, int frames, int mult) {
  if (!ok) return RRIN_E_ARG;
  if (int rc = net_check(nd, h0, w0, mult, [&] { return nd->n < 1 || h0 < 1 || w0 < 1 ? RRIN_E_SHAPE : 0; }))
    return rc;
  if (frames > 1 && img_stride < (int64_t)h0 * w0 * 3) return RRIN_E_ARG;
  return 0;
}

int frame_check(const rrin_net_u8_desc* d, int frames, int mult) {
  if (!d) return RRIN_E_ARG;
  return net_rgb_check(d->f0 && d->f1 && d->out_u8, &d->net, d->h0, d->w0, d->img_stride, frames, mult);
}

int frame_check(const rrin_net_u16_desc* d, int frames, int mult) {
  if (!d) return RRIN_E_ARG;
  return net_rgb_check(d->f0 && d->f1 && d->out_u16 && d->depth >= 9 && d->depth <= 16, &d->net, d->h0, d->w0,
                       d->img_stride, frames, mult);
}

int frame_check(const rrin_net_yuv_desc* d, int frames, int mult) {
  if (!d) return RRIN_E_ARG;
  return net_check(&d->net, d->h0, d->w0, mult, [&] {
    if (int rc = yuv_coef_check(&d->coef)) return rc;
    for (const rrin_yuv420* s : {&d->f0, &d->f1, &d->out}) {
      if (int rc = yuv420_check(*s, s == &d->out ? d->net.n : frames, d->h0, d->w0)) return rc;
      if (s->chroma != d->f0.chroma) return (int)RRIN_E_ARG;
    }
    return 0;
  });
}

int frame_check(const rrin_net_yuv16_desc* d, int frames, int mult) {
  if (!d) return RRIN_E_ARG;
  return net_check(&d->net, d->h0, d->w0, mult, [&] {
    for (const rrin_yuv420_16* s : {&d->f0, &d->f1, &d->out}) {
      if (int rc = yuv420_16_check(*s, s == &d->out ? d->net.n : frames, d->h0, d->w0)) return rc;
      if (s->depth != d->f0.depth || s->shift != d->f0.shift || s->chroma != d->f0.chroma) return (int)RRIN_E_ARG;
    }
    return yuv_coef_check16(&d->coef, d->f0.depth);
  });
}

// The three entries of a frame format D, rrin_net_D_fwd, _items_fwd (ABI 25: rrin_items beside the
// descriptor) and _scaled_fwd (rrin_flow_scale beside both):
//   Plain:  the descriptor's checks.
//   Items:  a null descriptor or taps (a plain forward's: an item forward refuses them), then the
//           items (RRIN_E_ARG), then the descriptor's checks with the stacks' n_pairs frames.
//   Scaled: flow_scale_check, then the items -- which may be NULL, a plain forward --, then the
//           descriptor's checks with the pad multiple 16 * s.
enum class Entry { Plain, Items, Scaled };

// bits of a sample of the frames of a descriptor: what an extra plane's depth must equal
int frame_depth(const rrin_net_u8_desc&) { return 8; }
int frame_depth(const rrin_net_yuv_desc&) { return 8; }
int frame_depth(const rrin_net_u16_desc& d) { return d.depth; }
int frame_depth(const rrin_net_yuv16_desc& d) { return d.f0.depth; }

// The extra plane of a frame forward whose own checks have passed (rrin_net_*_plane_fwd), before any
// launch: RRIN_E_ARG for taps or a depth that is not the frames', then plane_check
template <class D>
int plane_of(const D* d, const rrin_aux_plane* pa, int frames) {
  if (d->net.taps || pa->depth != frame_depth(*d)) return RRIN_E_ARG;
  return plane_check(pa, frames, d->net.n, d->h0, d->w0, d->net.h, d->net.w);
}

template <class D>
int frame_fwd(Entry e, const D* d, const rrin_items* it, const rrin_flow_scale* fs, void* stream,
              const rrin_aux_plane* pa = nullptr) {
  Items items;
  if (e == Entry::Scaled) {
    if (int rc = flow_scale_check(d ? &d->net : nullptr, fs)) return rc;
  } else if (e == Entry::Items && (!d || d->net.taps)) {
    return RRIN_E_ARG;
  }
  if (it || e == Entry::Items)
    if (int rc = items_of(it, d->net.n, items)) return rc;
  if (int rc = frame_check(d, it ? items.n_pairs : (d ? d->net.n : 0), fs ? 16 * fs->s : 16)) return rc;
  if (pa)
    if (int rc = plane_of(d, pa, it ? items.n_pairs : d->net.n)) return rc;
  return net_forward(&d->net, frame_io(*d), items, stream, fs, pa);
}

// rrin_net_*_plane_fwd: the entry that the nullable companions select, with the plane
template <class D>
int plane_fwd(const D* d, const rrin_items* it, const rrin_flow_scale* fs, const rrin_aux_plane* pa, void* stream) {
  return frame_fwd(fs ? Entry::Scaled : it ? Entry::Items : Entry::Plain, d, it, fs, stream, pa);
}

}  // namespace

extern "C" int rrin_net_u8_fwd(const rrin_net_u8_desc* d, void* stream) {
  return frame_fwd(Entry::Plain, d, nullptr, nullptr, stream);
}
extern "C" int rrin_net_yuv_fwd(const rrin_net_yuv_desc* d, void* stream) {
  return frame_fwd(Entry::Plain, d, nullptr, nullptr, stream);
}
extern "C" int rrin_net_u16_fwd(const rrin_net_u16_desc* d, void* stream) {
  return frame_fwd(Entry::Plain, d, nullptr, nullptr, stream);
}
extern "C" int rrin_net_yuv16_fwd(const rrin_net_yuv16_desc* d, void* stream) {
  return frame_fwd(Entry::Plain, d, nullptr, nullptr, stream);
}

extern "C" int rrin_net_u8_items_fwd(const rrin_net_u8_desc* d, const rrin_items* it, void* stream) {
  return frame_fwd(Entry::Items, d, it, nullptr, stream);
}
extern "C" int rrin_net_yuv_items_fwd(const rrin_net_yuv_desc* d, const rrin_items* it, void* stream) {
  return frame_fwd(Entry::Items, d, it, nullptr, stream);
}
extern "C" int rrin_net_u16_items_fwd(const rrin_net_u16_desc* d, const rrin_items* it, void* stream) {
  return frame_fwd(Entry::Items, d, it, nullptr, stream);
}
extern "C" int rrin_net_yuv16_items_fwd(const rrin_net_yuv16_desc* d, const rrin_items* it, void* stream) {
  return frame_fwd(Entry::Items, d, it, nullptr, stream);
}

extern "C" int rrin_net_u8_scaled_fwd(const rrin_net_u8_desc* d, const rrin_items* it, const rrin_flow_scale* fs,
                                      void* stream) {
  return frame_fwd(Entry::Scaled, d, it, fs, stream);
}
extern "C" int rrin_net_yuv_scaled_fwd(const rrin_net_yuv_desc* d, const rrin_items* it, const rrin_flow_scale* fs,
                                       void* stream) {
  return frame_fwd(Entry::Scaled, d, it, fs, stream);
}
extern "C" int rrin_net_u16_scaled_fwd(const rrin_net_u16_desc* d, const rrin_items* it, const rrin_flow_scale* fs,
                                       void* stream) {
  return frame_fwd(Entry::Scaled, d, it, fs, stream);
}
extern "C" int rrin_net_yuv16_scaled_fwd(const rrin_net_yuv16_desc* d, const rrin_items* it,
                                         const rrin_flow_scale* fs, void* stream) {
  return frame_fwd(Entry::Scaled, d, it, fs, stream);
}

extern "C" int rrin_net_u8_plane_fwd(const rrin_net_u8_desc* d, const rrin_items* it, const rrin_flow_scale* fs,
                                     const rrin_aux_plane* pa, void* stream) {
  return plane_fwd(d, it, fs, pa, stream);
}
extern "C" int rrin_net_u16_plane_fwd(const rrin_net_u16_desc* d, const rrin_items* it, const rrin_flow_scale* fs,
                                      const rrin_aux_plane* pa, void* stream) {
  return plane_fwd(d, it, fs, pa, stream);
}
extern "C" int rrin_net_yuv_plane_fwd(const rrin_net_yuv_desc* d, const rrin_items* it, const rrin_flow_scale* fs,
                                      const rrin_aux_plane* pa, void* stream) {
  return plane_fwd(d, it, fs, pa, stream);
}
extern "C" int rrin_net_yuv16_plane_fwd(const rrin_net_yuv16_desc* d, const rrin_items* it, const rrin_flow_scale* fs,
                                        const rrin_aux_plane* pa, void* stream) {
  return plane_fwd(d, it, fs, pa, stream);
}
