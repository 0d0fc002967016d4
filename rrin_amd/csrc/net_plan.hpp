// What the host schedule of a forward shares between its files: the four U-Nets of the Net, the
// workspace plan (one carve of the caller's workspace, identical in size query and forward), the
// caller's scratch, the buffer views, the launch profiler's state and ProfScope, the descriptor
// predicates, the step that begins a call, and the declarations of what crosses a file boundary:
//   unet_sched.hip  the U-Net walks (run_unet, run_unet_h8) and the scratch layout
//   net.hip         the Net forward driver (net_forward)
//   net_frames.hip  the byte-frame entries, which hand the driver a FrameIO
//   prof.hip        the rrin_prof_* entries
// No kernel, no launch and no extern "C" entry lives here.
#pragma once
#include <string.h>

#include <functional>
#include <vector>

#include "common.hpp"

struct rrin_prof {
  std::vector<hipEvent_t> ev;  // 2 per launch: start (recorded or shared), end
  std::vector<int32_t> start;  // per launch: index in ev of its start event
  std::vector<int32_t> kind;
  std::vector<double> flops;
  int count = 0;
  // within one rrin_net_fwd / rrin_unet_fwd call every launch on its stream is
  // bracketed, so a launch that directly follows the previous one on the same
  // stream starts at that launch's end event: one event record per launch
  bool chain = false;  // last_st / last_slot describe the call's previous launch
  hipStream_t last_st = nullptr;
  int last_slot = -1;
};

namespace rrin {

// The four U-Nets in execution order (model.py:35,42,51,62) with the input
// channel count they read from the 16-channel Net buffer g16 (starting at 0).
struct UNetSpec {
  int in_ch, out_ch, depth, head_mode;
};
inline constexpr UNetSpec kUNets[4] = {
    {6, 4, 5, RRIN_HEAD_FLOW},     // Flow        = UNet(6, 4, 5)   model.py:28
    {10, 4, 4, RRIN_HEAD_REFINE},  // refine_flow = UNet(10, 4, 4)  model.py:29
    {16, 2, 4, RRIN_HEAD_MASK},    // Mask        = UNet(16, 2, 4)  model.py:27
    {9, 3, 4, RRIN_HEAD_FINAL},    // final       = UNet(9, 3, 4)   model.py:30
};
constexpr int kMaxDepth = 5;

inline int chans(int level) { return 32 << level; }  // unet.py:26, wf=5
inline int convs_of(int depth) { return 2 * depth + 1 + 3 * (depth - 1); }

// ---- descriptor predicates: one copy of what every entry asks of n, h, w and prec
inline bool padded_shape_ok(int n, int h, int w) { return n >= 1 && h >= 16 && w >= 16 && !(h % 16) && !(w % 16); }
inline bool prec_ok(int prec) { return prec >= RRIN_PREC_F32 && prec <= RRIN_PREC_F32R; }
// the record layouts (every precision but the planar fp32 one)
inline bool record_prec(int prec) {
  return prec == RRIN_PREC_F16X3 || prec == RRIN_PREC_F16 || prec == RRIN_PREC_F32R;
}

struct Buf {
  float* base;  // F32: fp32 PP planes; F16* / F32R: (hi) records
  void* lo;     // F16X3: lo records
  int ch;
  int cpr;      // record layouts: channels per 16-B record (8: F16*, 4: F32R)
  rrin_geom g;
};

// What a schedule needs of the caller's scratch (size query, rrin_net_scratch_bytes):
// split-K slabs and tickets of the split convs, the ring fix-up's cross-workgroup K split.
struct ScratchNeed {
  int64_t part_floats = 0, cnt_ints = 0;
  void add(int64_t f, int64_t c) {
    part_floats = f > part_floats ? f : part_floats;
    cnt_ints = c > cnt_ints ? c : cnt_ints;
  }
};

// Workspace plan: offsets are identical in size query and forward.
struct Plan {
  int n, prec;
  rrin_prof* prof;        // the caller's launch profiler of this call (nullable)
  int32_t* status;        // the caller's fp16 range flag (nullable)
  rrin_geom g[kMaxDepth];
  Buf G;                  // 16 ch at level 0
  Buf X[kMaxDepth];       // level input (L >= 1): C_{L-1} ch
  Buf T[kMaxDepth];       // first conv of a block: C_L ch
  Buf CAT[kMaxDepth - 1]; // [up | bridge]: 2 C_L ch  (levels 0..3)
  Buf BOT;                // Flow bottom (level 4) conv-b output: 512 ch
  Buf UPT[kMaxDepth - 1]; // F16*: upsampled input of an up.1 conv, one per level (2 C_L ch).  Not
                          // shared across levels: another level's interior writes would land in
                          // this level's zero padding (the conv halo).
  Buf LRB[kMaxDepth];     // F16*, L >= 1: low-res input of a sub-pixel up conv (C_L ch), written with
                          // edge-replicate padding by its producer (EPI_LEAKY_REP)
  float* EDGE;            // F16*: pre-bias ring values of the current sub-pixel up conv
  Buf FLOWRAW;            // raw 4-ch Flow output, kept for reuse across t (skip_flow)
  // split-K / ring fix-up K-split scratch: the caller's (rrin_net_desc.scratch), not the
  // workspace, so a plan without splits pays nothing for it
  float* PART;            // F32R: split-K slice outputs of the current conv (part_floats)
  int32_t* CNT;           // F32R: split-K tile counters (cnt_ints; zero between convs)
  int64_t part_floats, cnt_ints;
  ScratchNeed* dry;       // non-null: size query only -- record the scratch the schedule
                          // needs, launch nothing (rrin_net_scratch_bytes)
  float* RCORR;           // F32R: ring-fold corrections of the current sub-pixel conv
  int32_t* RCNT;          // F32R: ring-fold segment tickets (zero between convs)
  int64_t rcorr_floats, rcnt_ints;
  int64_t bytes;
};

inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

inline void make_plan(int n, int h, int w, int prec, char* base, Plan& p) {
  p.n = n;
  p.prec = prec;
  p.prof = nullptr;
  p.status = nullptr;
  const bool f32 = prec == RRIN_PREC_F32;
  const int planes = prec == RRIN_PREC_F16X3 ? 2 : 1;
  const int cpr = prec == RRIN_PREC_F32R ? 4 : 8;
  int64_t off = 0;
  auto take = [&](int ch, const rrin_geom& g) {
    Buf b;
    // F32: ch fp32 planes; F16*: ch/8 record planes of 16 B (same 4 B/value with lo);
    // F32R: ch/4 record planes of 16 B
    const int64_t bytes = f32 ? (int64_t)n * ch * g.plane * 4 : (int64_t)n * ((ch + cpr - 1) / cpr) * g.plane * 16;
    b.base = base ? reinterpret_cast<float*>(base + off) : nullptr;
    off += align256(bytes);
    b.lo = nullptr;
    if (planes == 2) {
      b.lo = base ? static_cast<void*>(base + off) : nullptr;
      off += align256(bytes);
    }
    b.ch = ch;
    b.cpr = cpr;
    b.g = g;
    return b;
  };
  for (int L = 0; L < kMaxDepth; ++L) p.g[L] = f32 ? make_geom(h >> L, w >> L) : make_geom_h8(h >> L, w >> L);
  p.G = take(16, p.g[0]);
  for (int L = 0; L < kMaxDepth; ++L) {
    p.X[L] = L ? take(chans(L - 1), p.g[L]) : Buf{nullptr, nullptr, 0, cpr, p.g[0]};
    p.T[L] = take(chans(L), p.g[L]);
    if (L < kMaxDepth - 1) p.CAT[L] = take(2 * chans(L), p.g[L]);
  }
  p.BOT = take(chans(kMaxDepth - 1), p.g[kMaxDepth - 1]);
  for (int L = 0; L < kMaxDepth - 1; ++L)
    p.UPT[L] = f32 ? Buf{nullptr, nullptr, 0, cpr, p.g[L]} : take(2 * chans(L), p.g[L]);
  int64_t edge_floats = 0;
  for (int L = 0; L < kMaxDepth; ++L) {
    p.LRB[L] = (f32 || L == 0) ? Buf{nullptr, nullptr, 0, cpr, p.g[L]} : take(chans(L), p.g[L]);
    if (L < kMaxDepth - 1) {
      const int64_t hh = h >> L, ww = w >> L;
      const int64_t e = (int64_t)n * chans(L) * (2 * ww + 2 * (hh - 2));
      edge_floats = e > edge_floats ? e : edge_floats;
    }
  }
  p.EDGE = nullptr;
  if (!f32) {
    p.EDGE = base ? reinterpret_cast<float*>(base + off) : nullptr;
    off += align256(edge_floats * 4);
  }
  p.FLOWRAW = take(f32 ? 4 : cpr, p.g[0]);
  p.PART = nullptr;
  p.CNT = nullptr;
  p.RCORR = nullptr;
  p.RCNT = nullptr;
  p.rcorr_floats = p.rcnt_ints = 0;
  if (prec == RRIN_PREC_F32R) {
    // ring fold of the sub-pixel up conv into level L (runs on level L + 1's grid, 4 C_L
    // phase rows): 512 floats and one ticket per ring segment, co block and image
    for (int L = 0; L < kMaxDepth - 1; ++L) {
      const int64_t hl = h >> (L + 1), wl = w >> (L + 1);
      const int64_t segs = (int64_t)n * (4 * chans(L) / 32) * (2 * ((wl + 31) / 32) + 2 * ((hl + 7) / 8));
      p.rcnt_ints = segs > p.rcnt_ints ? segs : p.rcnt_ints;
    }
    p.rcorr_floats = 512 * p.rcnt_ints;
    p.RCORR = base ? reinterpret_cast<float*>(base + off) : nullptr;
    off += align256(p.rcorr_floats * 4);
    p.RCNT = base ? reinterpret_cast<int32_t*>(base + off) : nullptr;
    off += align256(p.rcnt_ints * 4);
  }
  p.part_floats = p.cnt_ints = 0;
  p.dry = nullptr;
  p.bytes = off;
}

// Caller-provided scratch (rrin_net_desc.scratch): [tickets | part floats].  The ticket count is
// a function of the schedule (n, h, w, the conv table): at least kScratchTickets, else the
// schedule's largest split conv's tile count rounded up to 1024 (scratch_tickets); the size
// query and the forward derive it the same way (scratch_layout), so the part slab starts at the
// same byte.
constexpr int64_t kScratchTickets = 4096;  // minimum ints at the head of the scratch (16 KB)

inline int64_t scratch_tickets(int64_t cnt_ints) {
  return cnt_ints <= kScratchTickets ? kScratchTickets : (cnt_ints + 1023) / 1024 * 1024;
}

// The scratch layout of a schedule of nu U-Nets, from one dry walk of it (unet_sched.hip): the
// tickets at its head and its size in bytes (0: the schedule needs none; every precision but
// F32R, which is not walked).  Returns the walk's error code and leaves the minimum layout.
struct ScratchLayout {
  int64_t tickets = kScratchTickets, bytes = 0;
};
int scratch_layout(int n, int h, int w, int prec, const rrin_conv_weights* convs, const UNetSpec* us, int nu,
                   ScratchLayout& out);

// The caller's scratch into the plan (F32R only; null / too small: no splits), with the ticket
// count the size query derives for this schedule of nu U-Nets at (n, h, w); a schedule the dry walk
// rejects keeps the minimum, and without a scratch nothing is walked.
inline void attach_scratch(Plan& p, void* scratch, int64_t bytes, int n, int h, int w, const rrin_conv_weights* convs,
                           const UNetSpec* us, int nu) {
  if (p.prec != RRIN_PREC_F32R || !scratch) return;
  ScratchLayout s;
  (void)scratch_layout(n, h, w, p.prec, convs, us, nu, s);
  if (bytes < s.tickets * 4) return;
  p.CNT = reinterpret_cast<int32_t*>(scratch);
  p.cnt_ints = s.tickets;
  p.PART = reinterpret_cast<float*>(reinterpret_cast<char*>(scratch) + s.tickets * 4);
  p.part_floats = (bytes - s.tickets * 4) / 4;
}

// H8 view of channels [ch_off, ch_off+channels) of a buffer, at geometry g
// (g differs from b.g only for the level-shared UPT buffer).
inline rrin_h8 hview(const Buf& b, int ch_off, int channels, const rrin_geom& g) {
  rrin_h8 v;
  v.hi = b.base;
  v.lo = b.lo;
  v.img_stride = (int64_t)((b.ch + b.cpr - 1) / b.cpr) * g.plane;
  v.g_off = ch_off / b.cpr;
  v.groups = (channels + b.cpr - 1) / b.cpr;
  v.g = g;
  return v;
}
inline rrin_h8 hview(const Buf& b, int ch_off, int channels) { return hview(b, ch_off, channels, b.g); }

inline rrin_pp view(const Buf& b, int ch_off, int channels) {
  rrin_pp v;
  v.base = b.base;
  v.img_stride = (int64_t)b.ch * b.g.plane;
  v.ch_off = ch_off;
  v.channels = channels;
  v.g = b.g;
  return v;
}

// Bracket one launch with profiler events (no-op without a profiler).
struct ProfScope {
  rrin_prof* p;
  hipStream_t st;
  int slot;
  ProfScope(rrin_prof* p_, hipStream_t s, int kind, double flops) : p(p_), st(s), slot(-1) {
    if (p && p->count < (int)p->kind.size()) {
      slot = p->count++;
      p->kind[slot] = kind;
      p->flops[slot] = flops;
      if (p->chain && slot > 0 && p->last_st == st && p->last_slot == slot - 1) {
        p->start[slot] = 2 * (slot - 1) + 1;  // the previous launch's end on this stream
      } else {
        p->start[slot] = 2 * slot;
        (void)hipEventRecord(p->ev[2 * slot], st);
      }
    }
  }
  ~ProfScope() {
    if (slot >= 0) {
      (void)hipEventRecord(p->ev[2 * slot + 1], st);
      p->chain = true;
      p->last_st = st;
      p->last_slot = slot;
    }
  }
};

#define RRIN_TRY(x)          \
  do {                       \
    int _rc = (x);           \
    if (_rc != 0) return _rc; \
  } while (0)

// Begin a call on the plan of descriptor d (rrin_net_desc / rrin_unet_desc, checked by the entry)
// whose schedule is the nu U-Nets us: carve the workspace and check its size -- the last check
// before the first HIP call --, attach the caller's scratch, take the caller's profiler and range
// flag, and clear the flag on the stream.
template <class D>
int begin_call(const D* d, const UNetSpec* us, int nu, hipStream_t st, Plan& p) {
  make_plan(d->n, d->h, d->w, d->prec, reinterpret_cast<char*>(d->workspace), p);
  if (d->workspace_bytes < p.bytes) return RRIN_E_WORKSPACE;
  attach_scratch(p, d->scratch, d->scratch_bytes, d->n, d->h, d->w, d->convs, us, nu);
  p.prof = d->prof;  // per call: concurrent calls never share launch state
  if (p.prof) p.prof->chain = false;  // the call's first launch records its own start
  if (d->status && (d->prec == RRIN_PREC_F16X3 || d->prec == RRIN_PREC_F16)) {
    p.status = d->status;  // fp16 range guard (the precisions stored as fp16)
    if (hipError_t e = hipMemsetAsync(d->status, 0, sizeof(int32_t), st)) return (int)e;
  }
  return 0;
}

// Where a U-Net's head sends its results: per-image t coefficients and the
// Net output (Net glue modes), and the optional raw conv output (NCHW).
struct HeadIO {
  const float* coef;
  float* out;
  float* raw;
  // FINAL on the record layout: the 8-bit crop (rrin_head_h8_desc.out_u8); NULL: off
  uint8_t* out_u8 = nullptr;
  int h0 = 0, w0 = 0, top = 0;
  // or the crop as 4:2:0 planes (rrin_head_h8_desc.out_yuv / yuv_coef); NULL: off
  const rrin_yuv420* out_yuv = nullptr;
  const rrin_yuv_coef* yuv_coef = nullptr;
  // or in 16-bit words (rrin_head_h8_desc.out_u16 / u16_depth, out_yuv16 with yuv_coef); NULL: off
  uint16_t* out_u16 = nullptr;
  int u16_depth = 0;
  const rrin_yuv420_16* out_yuv16 = nullptr;
};

// One U-Net (unet.py:40-51) from g16 channels [0, in_ch) to its head: on the planar fp32 layout,
// and on the record layouts (p.dry: walked with every launch skipped).  unet_sched.hip
int run_unet(const Plan& p, const UNetSpec& u, const rrin_conv_weights* cw, const rrin_head_weights& hw,
             const HeadIO& io, hipStream_t st);
int run_unet_h8(const Plan& p, const UNetSpec& u, const rrin_conv_weights* cw, const rrin_head_weights& hw,
                const HeadIO& io, hipStream_t st);

// Where a frame pack puts its images: the full-size g16 view, the precision, the stream and the pad
// multiple (16, or 16 * s of a flow_scale forward)
struct PackTo {
  const rrin_h8* g;
  int prec;
  hipStream_t st;
  int mult;
};

// The frames of a forward, whatever their format: what net_forward needs of a descriptor, filled by
// the frame_io of its type (net.hip: fp32 NCHW; net_frames.hip: the byte frames).  h0 = w0 = 0:
// rrin_net_fwd's fp32 NCHW frames.
struct FrameIO {
  int h0 = 0, w0 = 0;
  // the frame pack of m images: image k from frame k, or with a map from frame map[k] of np
  std::function<int(int m, const int32_t* map, int np, const PackTo& to)> pack;
  HeadIO store{};  // the output members of the FINAL store; coef, raw and the crop are head_io's
  HeadIO head_io(const float* coef, float* raw, int h) const {
    HeadIO io = store;
    io.coef = coef;
    io.raw = raw;
    io.h0 = h0;
    io.w0 = w0;
    io.top = h0 ? h - h0 : 0;
    return io;
  }
};

// An item forward (ABI 25): d->n items over n_pairs pairs through the device map; map NULL: a
// plain forward (every rrin_net_*_fwd)
struct Items {
  int n_pairs = 0;
  const int32_t* map = nullptr;
};

// The Net forward driver and the check of its second plan (net.hip); the callers have validated d
// and the companions they pass.
int flow_scale_check(const rrin_net_desc* nd, const rrin_flow_scale* fs);
int net_forward(const rrin_net_desc* d, const FrameIO& f, const Items& items, void* stream,
                const rrin_flow_scale* fs = nullptr, const rrin_aux_plane* pa = nullptr);

}  // namespace rrin
