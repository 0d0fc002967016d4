/*
 * rrin_hip.h — C ABI of librrin_hip.so, the MI355X (gfx950) kernels of the
 * RRIN inference hot path (reference `Net.forward`, /root/reference/model.py:59-65).
 *
 * Rules of the boundary:
 *   - plain C types only: device pointers, sizes, a hipStream_t passed as void*;
 *   - no allocation inside the library: every buffer (activations, workspace,
 *     packed weights) is owned by the caller (the Python host layer uses the
 *     PyTorch caching allocator);
 *   - every entry returns int: 0 = ok, > 0 = a hipError_t, < 0 = RRIN_E_* for a
 *     violated shape/argument precondition; rrin_strerror() decodes it;
 *   - stateless and stream-ordered: calls only enqueue work on `stream`; no
 *     call's result depends on another call.  Everything a call needs comes in
 *     its arguments (the optional launch profiler of rrin_net_fwd included);
 *     the only process-wide data are thread-safe launch caches keyed by the
 *     device of the stream a launch goes to (a kernel's dynamic-LDS attribute,
 *     resident blocks per CU), so a caller may pass any device's stream from any
 *     host thread.  One rrin_prof must not be shared by concurrent calls.
 *
 * Activation layouts between kernels:
 *   - record layout (the default, every `prec` but RRIN_PREC_F32): per image
 *     and channel group one plane of 16-byte records, hp = round_up(h,16)+2
 *     rows, wp = round_up(w,32)+16 records, pixel (y,x) at record
 *     (y+1)*wp + (x+8).  A record holds 4 fp32 channels (RRIN_PREC_F32R, exact
 *     fp32: "R32") or 8 halves (RRIN_PREC_F16X3 hi / lo planes, RRIN_PREC_F16:
 *     "H8").  rrin_geom / rrin_make_geom_h8 / rrin_h8 describe it.
 *   - padded planar ("PP", RRIN_PREC_F32 only: the round-1 fp32 path kept for
 *     A/B): per image and channel a plane of hp x wp fp32 with
 *     wp = round_up(w,32)+64, pixel (y,x) at (y+1)*wp + (x+32).
 * Padding is zero and is never written (it is the convs' zero padding).
 */
#ifndef RRIN_HIP_H
#define RRIN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RRIN_ABI_VERSION 25

#define RRIN_OK 0
#define RRIN_E_SHAPE (-1)     /* H or W not a multiple of 16, or N < 1          */
#define RRIN_E_ARG (-2)       /* null pointer / bad enum / channel range         */
#define RRIN_E_WORKSPACE (-3) /* workspace smaller than rrin_net_workspace_bytes */
#define RRIN_E_CONFIG (-4)    /* no kernel instance for the requested tile cfg   */

/* ---- Planar geometry --------------------------------------------------- */
typedef struct rrin_geom {
  int32_t h, w;      /* logical size                       */
  int32_t hp, wp;    /* padded plane size (see header)      */
  int64_t plane;     /* hp*wp (floats)                      */
} rrin_geom;

/* Fill a geometry for an h x w level. */
int rrin_make_geom(int32_t h, int32_t w, rrin_geom* g);

/* A PP tensor view: base points at channel 0 of image 0. */
typedef struct rrin_pp {
  float* base;
  int64_t img_stride; /* floats between images   */
  int32_t ch_off;     /* first channel of the view */
  int32_t channels;   /* channels in the view     */
  rrin_geom g;
} rrin_pp;

/* ---- Conv 3x3 (MFMA, exact fp32) ---------------------------------------- */
/* Replaces nn.Conv2d(k=3,pad=1)+bias (unet.py:29,59,62,78), LeakyReLU(0.1)
 * (unet.py:47,60,63), F.avg_pool2d(x,2) (unet.py:46, fused as a second output),
 * nn.Upsample(bilinear,x2) (unet.py:77, fused into the input staging) and
 * torch.cat(up,bridge) (unet.py:93, by channel-offset addressing). */
enum rrin_src_mode { RRIN_SRC_DIRECT = 0, RRIN_SRC_UPSAMPLE2X = 1 };
enum rrin_epi_mode {
  RRIN_EPI_LINEAR = 0,
  RRIN_EPI_LEAKY = 1,
  RRIN_EPI_LEAKY_POOL = 2,
  /* H8 only.  LEAKY_REP: leaky, and the image border is also written into the
   * 1-pixel padding ring (edge replicate) -- for a tensor whose only reader is
   * a sub-pixel up conv.  SUBPIXEL: the conv is the phase-combined form of
   * conv3x3(upsample_x2(src)) (rrin_subpixel_weights, cout = 4 x real cout):
   * linear, outputs pixel-shuffled into dst (2x the size of src); the outermost
   * ring of dst is not written but its pre-bias value goes to `edge` for
   * rrin_subpixel_edge_fix_h8. */
  RRIN_EPI_LEAKY_REP = 3,
  RRIN_EPI_SUBPIXEL = 4
};

typedef struct rrin_conv_desc {
  int32_t n;            /* images                                              */
  int32_t cin, cout;    /* real channel counts                                  */
  int32_t cfg;          /* tile config id (rrin_conv_cfg_bm); pack with same bm */
  int32_t src_mode;     /* rrin_src_mode; UPSAMPLE2X: src is at (h/2, w/2)      */
  int32_t epi_mode;     /* rrin_epi_mode                                        */
  float slope;          /* leaky slope (0.1)                                    */
  rrin_pp src;          /* input view (cin channels from src.ch_off)           */
  rrin_pp dst;          /* output view (cout channels from dst.ch_off), h x w  */
  rrin_pp pool;         /* EPI_LEAKY_POOL: pooled output (h/2 x w/2)           */
  const float* wpack;   /* rrin_pack_conv3x3 output for this cfg              */
  const float* bias;    /* padded bias (rrin_pack_conv3x3 output)              */
} rrin_conv_desc;

int rrin_conv_cfg_count(void);
int rrin_conv_cfg_bm(int32_t cfg);          /* output-channel tile of a config  */
int rrin_conv_cfg_th(int32_t cfg);          /* output-row tile of a config       */
int rrin_conv3x3_fwd(const rrin_conv_desc* d, void* stream);

/* Host-side weight packing (CPU memory).  w: OIHW [cout][cin][3][3] fp32,
 * b: [cout].  perm (nullable): packed input channel c reads reference channel
 * perm[c].  Output sizes from rrin_pack_conv3x3_floats(). */
int64_t rrin_pack_conv3x3_floats(int32_t cout, int32_t cin, int32_t bm);
int64_t rrin_pack_bias_floats(int32_t cout, int32_t bm);
int rrin_pack_conv3x3(const float* w, const float* b, int32_t cout, int32_t cin, int32_t bm,
                      const int32_t* perm, float* wpack, float* bpack);

/* ---- Head convs (Cout <= 4) with the fused Net glue ---------------------- */
/* One VALU conv3x3 32->{4,4,2,3} fused with the model.py glue that consumes it:
 *   FLOW   (Flow.last)        : t-blend of flows, model.py:37-39
 *   REFINE (refine_flow.last) : flow residual + two backwarps, model.py:44-48,8-21
 *   MASK   (Mask.last)        : sigmoid + weighted blend, model.py:52-55
 *   FINAL  (final.last)       : residual add + clamp to the NCHW output, model.py:62-63
 * g16 is the 16-channel Net buffer [x0(3) x1(3) Ft0(2) Ft1(2) xt1(3) xt2(3)]. */
enum rrin_head_mode { RRIN_HEAD_PLAIN = 0, RRIN_HEAD_FLOW = 1, RRIN_HEAD_REFINE = 2,
                      RRIN_HEAD_MASK = 3, RRIN_HEAD_FINAL = 4 };

typedef struct rrin_head_desc {
  int32_t n, cin, cout, mode;
  rrin_pp src;           /* cin-channel PP input                              */
  rrin_pp g16;           /* Net buffer (modes FLOW..FINAL); PLAIN: dst view    */
  const float* w;        /* OIHW [cout][cin][3][3] (unpacked)                 */
  const float* bias;     /* [cout]                                            */
  const float* coef;     /* [n][8] per-image t coefficients   */
  float* out;            /* FINAL: NCHW [n][3][h][w] contiguous               */
  rrin_pp flow_raw;      /* FLOW (optional, base NULL = skip): raw 4-ch Flow output kept
                            for reuse across t                    */
  float* raw_out;        /* optional (NULL = off): the head conv's output before any glue,
                            NCHW [n][cout][h][w] fp32 (intermediate-tap parity tests) */
} rrin_head_desc;

int rrin_head_fwd(const rrin_head_desc* d, void* stream);

/* ---- Layout kernels ------------------------------------------------------- */
/* NCHW contiguous [n][c][h][w] <-> PP view (c channels at dst.ch_off). */
int rrin_nchw_to_pp(const float* src, int32_t n, int32_t c, const rrin_pp* dst, void* stream);
int rrin_pp_to_nchw(const rrin_pp* src, int32_t n, int32_t c, float* dst, void* stream);

/* Standalone backwarp (model.py:8-21): out = grid_sample(img, grid(flow)),
 * NCHW contiguous fp32; same device code as the fused REFINE head. */
int rrin_warp_fwd(const float* img, const float* flow, float* out, int32_t n, int32_t c,
                  int32_t h, int32_t w, void* stream);

/* ---- Record-layout paths ("H8" family: 16-byte channel records) ---------- */
/* Precision of a forward / conv:
 *   F32   exact fp32 (v_mfma_f32_32x32x2_f32), PP layout above (planar, legacy);
 *   F32R  exact fp32 (v_mfma_f32_32x32x2_f32, fp32 storage) on the record layout
 *         below with 4 fp32 channels per 16-byte record ("R32"); the kernels,
 *         schedules and fusions of the fp16 paths (persistent grids, sub-pixel
 *         up convs, fused heads) -- the default fp32 path;
 *   F16X3 every fp32 value v is held as hi = f16(v), lo = f16((v - hi) * 2^11)
 *         (v = hi + lo 2^-11 to ~2^-22 |v|; lo stays normal) and every product as
 *         hi*hi + 2^-11 (hi*lo + lo*hi) in v_mfma_f32_32x32x16_f16 with fp32
 *         accumulation: fp32-class accuracy at ~5x the fp32 MFMA rate;
 *   F16   hi only (fp16 storage, fp16 products, fp32 accumulation) for the
 *         fp16 configs of BASELINE.json.
 * H8 layout: per image, per group of 8 channels, an hp x wp plane of 16-byte
 * records (8 halfs, channel-innermost); hp = round_up(h,16)+2,
 * wp = round_up(w,32)+16 records, pixel (y,x) at record (y+1)*wp + x+8.
 * F16X3 keeps two such tensors (hi, lo) with identical geometry. */
enum rrin_prec { RRIN_PREC_F32 = 0, RRIN_PREC_F16X3 = 1, RRIN_PREC_F16 = 2, RRIN_PREC_F32R = 3 };
/* In the record layout a "group" is the channels of one record: 8 (F16X3, F16)
 * or 4 (F32R); g_off / groups of an rrin_h8 view count such groups, and the
 * rrin_*_h8 entry points below accept F32R wherever they take a prec. */

int rrin_make_geom_h8(int32_t h, int32_t w, rrin_geom* g); /* plane in records */

typedef struct rrin_h8 {
  void* hi;           /* records (16 B), group 0 of image 0 of the tensor */
  void* lo;           /* same geometry; NULL for F16                     */
  int64_t img_stride; /* records between images                          */
  int32_t g_off;      /* first 8-channel group of the view               */
  int32_t groups;     /* groups in the view                              */
  rrin_geom g;
} rrin_h8;

typedef struct rrin_conv_h8_desc {
  int32_t n, cin, cout, cfg;   /* cfg: rrin_conv_h8_cfg_* */
  int32_t prec;                /* F16X3 or F16 */
  int32_t epi_mode;            /* rrin_epi_mode */
  float slope;
  float inv_wscale;            /* from rrin_pack_conv3x3_h8: weights were scaled by 1/inv_wscale */
  int32_t tail_finite;         /* 1: the channels [cin, 8*ceil(cin/8)) of src are finite (they meet
                                  zero weights), so the LDS-DMA kernel may stage whole records;
                                  0: cin % 8 != 0 uses the masking register-staged kernel */
  int32_t pad_;
  rrin_h8 src, dst, pool;      /* pool: EPI_LEAKY_POOL only */
  const void* whi;             /* packed halves (rrin_pack_conv3x3_h8) */
  const void* wlo;             /* NULL for F16 */
  const float* bias;           /* padded fp32 bias */
  float* edge;                 /* EPI_SUBPIXEL: [n][cout/4][rrin_ring_pixels(H,W)] fp32 */
  int32_t* status;             /* optional (F16X3 / F16): set to 1 when a stored value does not
                                  fit fp16 (|v| > 65504, inf or NaN) -- see rrin_net_desc.status */
  int32_t ksplit;              /* Winograd kinds 3, 4: > 1 splits the input channels into
                                  ksplit slices of whole 8-channel chunks (fewer if a slice would
                                  be empty), one workgroup per tile and slice; the last slice of a
                                  tile sums the slices' pre-bias outputs in slice order.  0 / 1:
                                  no split.  A fixed split per conv keeps batch == per-sample
                                  outputs bitwise; a different split rounds differently */
  int32_t pad2_;
  float* part;                 /* ksplit > 1: rrin_conv_h8_split_floats() floats, any contents */
  int32_t* cnt;                /* ksplit > 1: one int per tile, zero before the first call; every
                                  call leaves it zero again (one call at a time per cnt) */
  /* EPI_SUBPIXEL ring fold (Winograd kind 3, no split): with ring_w set, the launch
     also writes the 1-pixel ring of the 2h x 2w output (the work of
     rrin_subpixel_edge_fix_h8, which is then not called): correction workgroups at
     the head of the grid, one per ring segment, and the segment's conv tile meet
     through ring_cnt; edge still receives the phase values */
  const float* ring_w;         /* original weights [cin][9][cout/4] fp32 (NULL: no fold) */
  const float* ring_bias;      /* original bias [cout/4] */
  float* ring_corr;            /* rrin_conv_h8_ring_floats() floats, any contents */
  int32_t* ring_cnt;           /* rrin_conv_h8_ring_floats() ints, zero before the first call;
                                  every call leaves it zero again */
  /* ABI 17, EPI_SUBPIXEL: the ring pixels from scratch in the same call -- a rrin_edge_fix_desc
     with full = 1 for this conv's src / dst (its own weights, bias, epi_mode, status); edge is
     still written.  The direct-form tiles of 256 or 512 threads run it in extra workgroups at
     the head of the conv's grid (they read only src and write only dst's ring pixels, which the
     sub-pixel conv never writes) with threads / 256 K groups; other configs launch it after the
     conv.  NULL: the caller runs rrin_subpixel_edge_fix_h8 itself. */
  const struct rrin_edge_fix_desc* ring_full;
} rrin_conv_h8_desc;

/* Fused level-0 UNetConvBlock at fp16 (unet.py:59-63, and :46 for down_path[0]): conv a
 * (cin -> 32) + LeakyReLU, conv b (32 -> 32) + LeakyReLU, optionally the 2x2 average pool of the
 * result, in one launch; conv a's output never reaches memory (an 8 x 62 output tile's conv-a
 * values, 1-pixel halo recomputed, stay in LDS).  The weights are the two convs' own
 * rrin_pack_conv3x3_h8 packs (fp16, the bm of cfg_a / cfg_b, direct-form configs); the outputs
 * are bitwise those of the two rrin_conv3x3_h8_fwd calls (EPI_LEAKY into a 32-channel tensor,
 * then EPI_LEAKY or EPI_LEAKY_POOL) at fp16.  dst must not overlap src.  ABI 14. */
typedef struct rrin_block0_h8_desc {
  int32_t n, cin;              /* conv a: cin -> 32 (cin % 8 == 0 or tail_finite); conv b: 32 -> 32 */
  int32_t cfg_a, cfg_b;        /* rrin_conv_h8 configs the packs were made for (direct form) */
  float slope;                 /* 0 <= slope <= 1 */
  float inv_wscale_a, inv_wscale_b; /* from rrin_pack_conv3x3_h8 */
  int32_t tail_finite;         /* as rrin_conv_h8_desc.tail_finite */
  rrin_h8 src, dst, pool;      /* fp16 records; pool.hi NULL: no pool output */
  const void* whi_a;
  const float* bias_a;
  const void* whi_b;
  const float* bias_b;
  int32_t* status;             /* optional fp16 range flag, as rrin_conv_h8_desc.status */
} rrin_block0_h8_desc;
int rrin_conv_block0_h8_fwd(const rrin_block0_h8_desc* d, void* stream);

int rrin_conv_h8_cfg_count(void);
int rrin_conv_h8_cfg_bm(int32_t cfg);
int rrin_conv_h8_cfg_th(int32_t cfg);
int rrin_conv_h8_cfg_ok(int32_t cfg, int32_t prec); /* 1 if the config fits LDS at prec */
/* 1 if the config can run a conv with cin input channels (a config that keeps
 * every weight chunk resident in LDS needs them to fit) */
int rrin_conv_h8_cfg_fits(int32_t cfg, int32_t prec, int32_t cin);
int rrin_conv3x3_h8_fwd(const rrin_conv_h8_desc* d, void* stream);
/* Scratch of a split-K conv (d->ksplit > 1): returns the floats of d->part and
 * stores the ints of d->cnt (0 and 0 without a split); < 0: the error code */
int64_t rrin_conv_h8_split_floats(const rrin_conv_h8_desc* d, int64_t* cnt_ints);
/* Scratch of a ring-folding sub-pixel conv (d->ring_w set): returns the floats of
 * d->ring_corr and stores the ints of d->ring_cnt; < 0: the error code (RRIN_E_CONFIG:
 * the config cannot fold -- run rrin_subpixel_edge_fix_h8 instead) */
int64_t rrin_conv_h8_ring_floats(const rrin_conv_h8_desc* d, int64_t* cnt_ints);
/* Nonzero if cfg is a Winograd config (not packed by rrin_pack_conv3x3_r32 /
 * rrin_pack_conv3x3_h8): the tile kind.  F(2x2,3x3), packed by
 * rrin_pack_conv3x3_wino_bm with the config's BM (F32R): 1 = BM 32 x TH 8 on 4
 * waves, 3 = BM 32 x TH 8 on 8 waves of 4 accumulators (4 waves per SIMD), 4 =
 * kind 3 on TH 4 tiles (4 waves), 6 = BM 64 x TH 4 and 7 = BM 32 x TH 8 on 4 waves
 * with the U operands loaded straight into registers (cin % 8 == 0 or
 * tail_finite); all give bitwise-equal outputs.  Kinds 3 and 4 take a split-K
 * (rrin_conv_h8_desc.ksplit).  Kind 6 also runs at RRIN_PREC_F16 (packed by
 * rrin_pack_conv3x3_wino_h8; cin % 16 == 0 or tail_finite; no split-K, no ring
 * fold).  0: direct form.  -1: a retired id (19, 22: ABI 16 removed the rejected
 * kinds 2, 5 and 8-13 and their configs 25-30; rrin_conv_h8_cfg_ok reports 0 and
 * rrin_conv3x3_h8_fwd returns RRIN_E_CONFIG).  14 (ABI 18, config 25): BM 32 x TH 8 on
 * 4 waves, register U, Winograd F(4,3) x F(2,3) (patches 4 wide x 2 tall: 0.75x kind 6's
 * MFMAs; a different rounding, not bitwise the F(2x2,3x3) kinds), packed by
 * rrin_pack_conv3x3_wino42; cin % 8 == 0 or tail_finite; no split-K, no ring fold, the
 * ring_full fix-up as a second launch. */
int rrin_conv_h8_cfg_wino(int32_t cfg);
/* ABI 19: kind 14's tile geometry, process-wide: 0 (default) picks per launch the one needing
 * fewer rounds of 512 resident workgroups, and persistent workgroups for short K (<= 8 chunks)
 * on large grids; 1 always 32 px x 8 rows (persistent where eligible); 2 always 16 px x 16 rows;
 * 3 always 32 x 8, one workgroup per tile.  Every policy computes each output from the same patch
 * with the same arithmetic: the outputs are the same bits.  Returns the previous policy,
 * RRIN_E_ARG outside 0-3. */
int rrin_conv_h8_set_wino42_geom(int32_t mode);
/* The launch shape rrin_conv3x3_h8_fwd / rrin_conv_block0_h8_fwd would use for d on stream's device
 * right now (entry points only, no ABI bump): a read-only query for tests that must know which
 * branch a launcher takes -- the persistent grids depend on the device's CU count and the
 * occupancy of the tile, kind 14's geometry on the tile counts and the process-wide policy.  It
 * validates d exactly as the forward call does (same error codes, scratch pointers included),
 * runs the launcher's own grid / variant decision and launches nothing.  `tiles`: work items of
 * the conv part (co blocks x tile positions x images, x K slices for split-K; kind 14 in the
 * geometry it chose).  `grid`: workgroups launched for them; grid < tiles means workgroup b walks
 * tiles b, b + grid, ...  `extra`: workgroups at the head of the same launch that do the
 * sub-pixel ring (ring fold, or ring_full where the tile runs it in the launch), 0 when the ring
 * is a launch of its own.  `variant`: 0, or for kind 14 1 = 16 x 16 tiles, 2 = persistent 32 x 8
 * tiles. */
typedef struct rrin_launch_info {
  int64_t tiles;
  int64_t grid;
  int64_t extra;
  int32_t variant;
  int32_t pad_;
} rrin_launch_info;
int rrin_conv_h8_launch_info(const rrin_conv_h8_desc* d, void* stream, rrin_launch_info* out);
int rrin_conv_block0_h8_launch_info(const rrin_block0_h8_desc* d, void* stream, rrin_launch_info* out);

/* F32R packing: [co_block][chunk of 8 ci][tap][half][bm][4] fp32 (half hh holds
 * input channels chunk*8 + 4*hh .. +3), unscaled; pass as whi (wlo NULL,
 * inv_wscale ignored).  bpack: rrin_pack_bias_floats(cout, bm) floats. */
int64_t rrin_pack_conv3x3_r32_floats(int32_t cout, int32_t cin, int32_t bm);
int rrin_pack_conv3x3_r32(const float* w, const float* b, int32_t cout, int32_t cin, int32_t bm,
                          const int32_t* perm, float* wpack, float* bpack);

/* Winograd packing (F32R, the rrin_conv_h8_cfg_wino configs): U = G g G^T per
 * (co, ci) computed in double and rounded once to fp32, laid out
 * [co_block of bm][chunk of 8 ci][xi 16][half 2][co bm][4 ci] (xi = 4*row + col
 * of the 4x4 transform, G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]; half hh holds
 * input channels chunk*8 + 4*hh .. +3); bm = 32 or 64 (the config's BM).
 * bpack: rrin_pack_bias_floats(cout, bm) floats.  The un-suffixed pair is bm 32. */
int64_t rrin_pack_conv3x3_wino_bm_floats(int32_t cout, int32_t cin, int32_t bm);
int rrin_pack_conv3x3_wino_bm(const float* w, const float* b, int32_t cout, int32_t cin, int32_t bm,
                              const int32_t* perm, float* wpack, float* bpack);
/* Kind-14 packing (ABI 18): U(eta, xi) = sum G2[eta][ky] G4[xi][kx] g[ky][kx] in double,
 * rounded once to fp32 (G2 the F(2,3) matrix above, rows; G4 = F(4,3)'s [1/4 0 0; -1/6 -1/6
 * -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1], columns), laid out
 * [co_block of 32][chunk of 8 ci][point 6*eta + xi (24)][half 2][co 32][4 ci].  bpack:
 * rrin_pack_bias_floats(cout, 32) floats. */
int64_t rrin_pack_conv3x3_wino42_floats(int32_t cout, int32_t cin);
int rrin_pack_conv3x3_wino42(const float* w, const float* b, int32_t cout, int32_t cin, const int32_t* perm,
                             float* wpack, float* bpack);
int64_t rrin_pack_conv3x3_wino_floats(int32_t cout, int32_t cin);
int rrin_pack_conv3x3_wino(const float* w, const float* b, int32_t cout, int32_t cin, const int32_t* perm,
                           float* wpack, float* bpack);
/* fp16 Winograd packing (ABI 13; kind 6 at RRIN_PREC_F16): U = G g G^T per (co, ci)
 * in double, times a power of two that puts max|U| in [2^12, 2^13), rounded once to
 * fp16, laid out [co_block of 64][chunk of 16 ci][xi 16][half 2][co 64][8 ci] (half hh
 * holds input channels chunk*16 + 8*hh .. +7); *inv_wscale receives the exact inverse
 * scale (pass it in rrin_conv_h8_desc.inv_wscale).  bm must be 64.  bpack:
 * rrin_pack_bias_floats(cout, 64) floats. */
int64_t rrin_pack_conv3x3_wino_h8_halves(int32_t cout, int32_t cin, int32_t bm);
int rrin_pack_conv3x3_wino_h8(const float* w, const float* b, int32_t cout, int32_t cin, int32_t bm,
                              const int32_t* perm, uint16_t* whi, float* bpack, float* inv_wscale);

/* Host packing: [co_block][chunk of 16 ci][tap][half][bm][8] halves, weights
 * pre-scaled by a power of two so max|w| lands in [2^12, 2^13) (keeps lo
 * normal); *inv_wscale receives the exact inverse scale. */
int64_t rrin_pack_conv3x3_h8_halves(int32_t cout, int32_t cin, int32_t bm);
int rrin_pack_conv3x3_h8(const float* w, const float* b, int32_t cout, int32_t cin, int32_t bm,
                         const int32_t* perm, int32_t prec, uint16_t* whi, uint16_t* wlo,
                         float* bpack, float* inv_wscale);

/* ---- Sub-pixel form of the up block's upsample + conv (unet.py:77-78) ------
 * conv3x3(upsample_bilinear_x2(x)) at output pixel (2m+py, 2n+px) equals a 3x3
 * conv of x around (m, n) with phase-combined weights W'_(py,px), provided x is
 * edge-replicated by one pixel; it then equals the conv over the replicate-padded
 * upsampled image, so only the outermost output ring differs from the reference
 * (zero padding) -- by the outside taps, which rrin_subpixel_edge_fix_h8 removes.
 * rrin_subpixel_weights: w [cout][cin][3][3], b [cout] -> wsub [4*cout][cin][3][3],
 * bsub [4*cout] with row co' = (co/8)*32 + (2*py+px)*8 + co%8 (cout % 8 == 0),
 * computed in double. */
int rrin_subpixel_weights(const float* w, const float* b, int32_t cout, int32_t cin, float* wsub, float* bsub);
/* pixels on the outermost ring of an H x W image: top row, bottom row, then the
 * left and right columns without the corners (ring index order). */
int64_t rrin_ring_pixels(int32_t h, int32_t w);
typedef struct rrin_edge_fix_desc {
  int32_t n, cin, cout, prec;  /* cout: real output channels (<= 8*dst.groups), cin <= 256 */
  int32_t epi_mode;            /* LINEAR or LEAKY */
  float slope;
  rrin_h8 src;                 /* low-res input of the sub-pixel conv (h x w)   */
  rrin_h8 dst;                 /* its output (2h x 2w): ring pixels are written */
  const float* edge;           /* pre-bias ring values from the EPI_SUBPIXEL conv */
  const float* wedge;          /* original weights as [cin][9][cout] fp32       */
  const float* bias;           /* original bias [cout]                          */
  int32_t* status;             /* optional: fp16 range flag, as rrin_conv_h8_desc */
  /* ABI 11, optional (zero = one workgroup per tile loops over the K runs; the
   * result is the same bit for bit): scratch for the cross-workgroup K split of
   * fp32 records (cin / 64 runs of 64 channels, one workgroup each; the last one
   * of a tile, by a ticket in cnt, adds the runs in run order).  Used when
   * part_floats / cnt_len cover rrin_edge_fix_split_floats; cnt starts at zero
   * and is left at zero. */
  float* part;
  int32_t* cnt;
  int64_t part_floats;
  int32_t cnt_len;
  /* ABI 15: 1 = the ring value from scratch (bias + the conv's in-image taps of the
   * upsampled src, two staged lines per ring line; `edge` unused, may be NULL): it reads
   * nothing the EPI_SUBPIXEL conv writes (that conv writes ring pixels only to `edge`), so
   * the two may run concurrently (the Net measured both orders slower than the
   * correction, DESIGN.md §5e, and uses 0).  0 = the correction of the conv's `edge` values. */
  int32_t full;
} rrin_edge_fix_desc;
int rrin_subpixel_edge_fix_h8(const rrin_edge_fix_desc* d, void* stream);
/* Scratch floats (return; 0 = this cin / precision does not split) and tickets
 * (*cnt) of the ring fix-up's cross-workgroup K split for d's shapes. */
int64_t rrin_edge_fix_split_floats(const rrin_edge_fix_desc* d, int64_t* cnt);

/* nn.Upsample(bilinear, x2) (unet.py:77) of an H8 view into another H8 view. */
int rrin_upsample2x_h8(const rrin_h8* src, const rrin_h8* dst, int32_t n, int32_t prec, void* stream);
/* x = cat(x0, x1) (model.py:33) into the 16-channel H8 Net buffer: channels
 * 0-5 from the two NCHW frames, channels 6-15 zeroed (whole-record stores). */
int rrin_pack_g16_h8(const float* i0, const float* i1, int32_t n, const rrin_h8* g16, int32_t prec, void* stream);
/* ABI 20: the same from two stacks of 8-bit frames, uint8 [n][h0][w0][3] (RGB interleaved, every
 * frame dense, img_stride bytes between frames of a stack: f0 and f1 may be two views of one
 * [n+1] stack), any h0, w0 >= 1; g16 is round_up(h0,16) x round_up(w0,16) (RRIN_E_SHAPE
 * otherwise).  The frame is edge-replicated on top (h - h0 rows) and on the right (w - w0
 * columns): padded pixel (y, x) reads source pixel (max(y - (h - h0), 0), min(x, w0 - 1)); a
 * byte u becomes float(u) / 255.0f, correctly rounded (a 256-entry table).  The records are
 * bitwise those rrin_pack_g16_h8 writes from the padded fp32 NCHW frames. */
int rrin_pack_g16_u8_h8(const uint8_t* f0, const uint8_t* f1, int64_t img_stride, int32_t n, int32_t h0,
                        int32_t w0, const rrin_h8* g16, int32_t prec, void* stream);

/* ---- 8-bit YUV 4:2:0 frames (ABI 22) -------------------------------------------------------
 * One stack of 4:2:0 frames: a luma plane of h0 x w0 bytes and two chroma planes of h0/2 x w0/2
 * samples, one sample per 2x2 block of pixels.  NV12 (one interleaved UV plane): v == u + 1,
 * c_step 2; I420 (planar): c_step 1.  h0 and w0 are even.
 *
 * ABI 24: chroma (the former pad_ word, which every caller zero-filled: 4:2:0) picks the chroma
 * block.  RRIN_CHROMA_422: one U and one V sample per 2x1 block (two pixels wide, one row tall),
 * chroma planes of h0 x w0/2 samples, w0 even and >= 2, any h0 >= 1 (NV16: c_step 2; I422: 1).
 * RRIN_CHROMA_444: one per pixel, planes of h0 x w0, any h0, w0 >= 1 (c_step 1; a semi-planar
 * 4:4:4 with c_step 2 is legal here).  Another value: RRIN_E_ARG.  c_pitch >= (chroma columns) *
 * c_step.  The stacks of one call share chroma (RRIN_E_ARG otherwise). */
enum rrin_chroma { RRIN_CHROMA_420 = 0, RRIN_CHROMA_422 = 1, RRIN_CHROMA_444 = 2 };
typedef struct rrin_yuv420 {
  const uint8_t *y, *u, *v;    /* frame 0; NV12: v == u + 1 */
  int64_t img_stride;          /* bytes between frames, the same for all three pointers */
  int32_t y_pitch, c_pitch;    /* bytes between rows (>= w0, >= (w0/2)*c_step) */
  int32_t c_step, chroma;      /* bytes between chroma samples of a row: 2 NV12, 1 I420; rrin_chroma */
} rrin_yuv420;

/* The colour conversion around the 8-bit frame path, pure int32 arithmetic on Q14 coefficients
 * (>> is the arithmetic shift: floor); clip255 clamps to [0, 255].
 *   in,  per pixel, with the U, V of its 2x2 block (replicated, no interpolation),
 *        c = Y - y0, d = U - 128, e = V - 128:
 *     R = clip255((ay*c        + rv*e + 8192) >> 14)
 *     G = clip255((ay*c + gu*d + gv*e + 8192) >> 14)
 *     B = clip255((ay*c + bu*d        + 8192) >> 14)
 *   out, per pixel:  Y = clip255(y0 + ((yr*R + yg*G + yb*B + 8192) >> 14))
 *        per block, Rs / Gs / Bs the sums of its four pixels' bytes:
 *     U = clip255(128 + ((ur*Rs + ug*Gs + ub*Bs + 32768) >> 16))
 *     V = clip255(128 + ((vr*Rs + vg*Gs + vb*Bs + 32768) >> 16))
 *        ABI 24, a block of P pixels (4:2:0: 4, 4:2:2: 2, 4:4:4: 1) with sums Rs / Gs / Bs:
 *     U = clip255(128 + ((ur*Rs + ug*Gs + ub*Bs + 8192*P) >> (14 + log2 P))), V likewise
 * Any 15 values with |coefficient| < 2^16 and 0 <= y0 <= 255 may be passed (RRIN_E_ARG
 * otherwise: the sums then fit int32). */
typedef struct rrin_yuv_coef {
  int32_t y0, ay, rv, gu, gv, bu;                  /* YUV -> RGB */
  int32_t yr, yg, yb, ur, ug, ub, vr, vg, vb;      /* RGB -> YUV */
} rrin_yuv_coef;
enum rrin_yuv_standard { RRIN_YUV_BT709 = 0, RRIN_YUV_BT601 = 1 };
/* The coefficients of a standard: round(x * 2^14) of the matrix its Kr / Kb give, for limited
 * (Y 16..235, chroma 16..240) or full range; yg, ug and vg are remainders (yr + yg + yb =
 * round(2^14 * luma scale), ur + ug + ub = vr + vg + vb = 0), so grey maps to U = V = 128
 * exactly.  Host only. */
int rrin_yuv_coef_std(int32_t standard, int32_t full_range, rrin_yuv_coef* c);

/* rrin_pack_g16_u8_h8 from two stacks of 4:2:0 frames: the records are bitwise those it writes
 * from the frames converted to RGB bytes as above.  Padding is its rule applied to source
 * coordinates: padded pixel (y, x) reads source pixel (sy, sx) = (max(y - (h - h0), 0),
 * min(x, w0 - 1)), its luma and the chroma of block (sy/2, sx/2) -- (sy, sx/2) at 4:2:2, (sy, sx)
 * at 4:4:4; f0 and f1 share chroma (RRIN_E_ARG otherwise).  A frame may start at any
 * byte.  Null planes or coef, c_step not 1 or 2, a coefficient out of range: RRIN_E_ARG; odd or
 * < 2 h0 / w0, a pitch smaller than its row, frames of a stack that overlap (n > 1), a g16 that
 * is not round_up(h0,16) x round_up(w0,16): RRIN_E_SHAPE.  Validated before any HIP call. */
int rrin_pack_g16_yuv_h8(const rrin_yuv420* f0, const rrin_yuv420* f1, const rrin_yuv_coef* coef, int32_t n,
                         int32_t h0, int32_t w0, const rrin_h8* g16, int32_t prec, void* stream);

/* ---- 10- to 16-bit frames in 16-bit words (ABI 23) -------------------------------------------
 * The 8-bit frame paths with uint16 words: a sample of depth d (maxval = 2^d - 1) is
 * min(word >> shift, maxval) and becomes float(sample) / float(maxval), correctly rounded (the
 * IEEE fp32 division, no reciprocal multiply).  Strides and pitches count samples, so a frame of
 * an [n+1] stack starts at any even address.
 *
 * rrin_pack_g16_u16_h8: rrin_pack_g16_u8_h8 from uint16 [n][h0][w0][3] RGB frames of depth 9..16
 * (RRIN_E_ARG otherwise), the sample in the word's low bits; the records are bitwise those
 * rrin_pack_g16_h8 writes from the padded fp32 frames. */
int rrin_pack_g16_u16_h8(const uint16_t* f0, const uint16_t* f1, int64_t img_stride, int32_t n, int32_t h0,
                         int32_t w0, int32_t depth, const rrin_h8* g16, int32_t prec, void* stream);

/* One stack of 4:2:0 frames of 16-bit words: rrin_yuv420 with every pitch, step and stride in
 * samples.  depth is 10 or 12 (RRIN_E_ARG otherwise: with |coefficient| < 2^16 the Q14 sums stay
 * inside int32 up to 14 bits, not at 16); shift is 0 (the sample in the low bits: yuv420p10le, Y4M
 * C420p10) or 16 - depth (in the high bits: P010 / P012).  Samples are read as
 * min(word >> shift, maxval) and written as sample << shift. */
typedef struct rrin_yuv420_16 {
  const uint16_t *y, *u, *v;   /* frame 0; NV12 order: v == u + 1 */
  int64_t img_stride;          /* samples between frames, the same for all three pointers */
  int32_t y_pitch, c_pitch;    /* samples between rows */
  int32_t c_step;              /* samples between chroma samples of a row: 2 or 1 */
  int32_t depth, shift, chroma; /* chroma: rrin_chroma (ABI 24), as in rrin_yuv420 */
} rrin_yuv420_16;
/* The conversion is rrin_yuv_coef's with 128 replaced by 2^(depth-1) and clip255 by a clip to
 * [0, maxval]; the roundings stay.  Coefficients on this path: 0 <= y0 <= maxval, |ay .. bu| < 2^16,
 * |yr .. vb| < 2^15 (RRIN_E_ARG otherwise); every sum then fits int32 at depth 12, the largest
 * being a 2x2 block's chroma, 3 * (2^15 - 1) * 4 * 4095 + 2^15 < 2^31 (the blocks of 4:2:2 and
 * 4:4:4 sum fewer samples: further inside).  rrin_yuv_coef_std16 is
 * rrin_yuv_coef_std for a depth of 8..16: y0 = 16 << (depth - 8), luma scaled by
 * 219 * 2^(depth-8) / maxval and chroma by 224 * 2^(depth-8) / maxval (limited range); depth 8
 * gives rrin_yuv_coef_std's numbers.  Host only. */
int rrin_yuv_coef_std16(int32_t standard, int32_t full_range, int32_t depth, rrin_yuv_coef* c);
/* rrin_pack_g16_yuv_h8 from two rrin_yuv420_16 stacks of one depth and shift (RRIN_E_ARG
 * otherwise): bitwise the records rrin_pack_g16_u16_h8 writes from the frames converted to RGB
 * samples of that depth.  Checked as there, before any HIP call. */
int rrin_pack_g16_yuv16_h8(const rrin_yuv420_16* f0, const rrin_yuv420_16* f1, const rrin_yuv_coef* coef, int32_t n,
                           int32_t h0, int32_t w0, const rrin_h8* g16, int32_t prec, void* stream);
/* NCHW fp32 <-> H8 view (c channels starting at channel ch_off of the view).  rrin_nchw_to_h8
 * stores one element per value: the other channels of a record that [ch_off, ch_off + c) covers
 * only partly keep their contents, as do the padding and every other group. */
int rrin_nchw_to_h8(const float* src, int32_t n, int32_t c, int32_t ch_off, const rrin_h8* dst,
                    int32_t prec, void* stream);
int rrin_h8_to_nchw(const rrin_h8* src, int32_t n, int32_t c, int32_t ch_off, float* dst, int32_t prec,
                    void* stream);

typedef struct rrin_head_h8_desc {
  int32_t n, cin, cout, mode, prec, pad_;
  rrin_h8 src;           /* 32-channel input                              */
  rrin_h8 g16;           /* Net buffer (2 groups); PLAIN: dst view          */
  const float* w;        /* OIHW fp32 (unpacked)                          */
  const float* bias;
  const float* coef;
  float* out;            /* FINAL: NCHW fp32 */
  rrin_h8 flow_raw;      /* FLOW (optional, hi NULL = skip): raw 4-ch Flow output */
  float* raw_out;        /* optional: head conv output before the glue, NCHW fp32 */
  int32_t* status;       /* optional: fp16 range flag; FINAL writes NaN pixels when it is set */
  /* ABI 20, FINAL, optional (NULL: off): the output also (out set) or only (out NULL) as 8-bit
     interleaved frames [n][h0][w0][3] -- the crop rows [top, top + h0), columns [0, w0) of the
     h x w output, each value v as (uint8)(v * 255.0f) (one fp32 multiply, truncation); a pixel
     poisoned by the range flag is written as 0.  top + h0 <= h, w0 <= w. */
  uint8_t* out_u8;
  int32_t h0, w0, top, pad2_;
  /* ABI 22, FINAL, optional (out_yuv.y NULL: off), not together with out_u8 (RRIN_E_ARG); out may
     still be set: the crop's RGB bytes (those out_u8 would hold) converted to 4:2:0 with
     yuv_coef (see rrin_yuv_coef) into the planes of out_yuv, which are written through in spite
     of the const of the struct's pointers.  h0, w0 and top must be even (RRIN_E_SHAPE).  Y is
     written for the crop's pixels and U / V once per 2x2 block; pitch bytes beyond w0 and
     anything outside the crop are never written.  ABI 24, by out_yuv.chroma: at 4:2:2 only w0
     must be even (h0 and top may be odd) and U / V are written once per 2x1 block; at 4:4:4 no
     size need be even and U / V are written per pixel. */
  rrin_yuv420 out_yuv;
  rrin_yuv_coef yuv_coef;
  int32_t pad3_;
  /* ABI 23, FINAL, optional (NULL: off); at most one of out_u8 / out_yuv / out_u16 / out_yuv16
     may be set (RRIN_E_ARG otherwise), out may still be.  out_u16: the crop (h0, w0, top as for
     out_u8) as interleaved 16-bit frames [n][h0][w0][3] of depth u16_depth (9..16), each value v
     as (uint16)(v * (float)maxval), 0 when poisoned.  out_yuv16 (y NULL: off): those samples at
     out_yuv16.depth converted with yuv_coef into its 16-bit 4:2:0 planes, each written as
     sample << shift, under the rules of out_yuv. */
  uint16_t* out_u16;
  int32_t u16_depth, pad4_;
  rrin_yuv420_16 out_yuv16;
} rrin_head_h8_desc;
int rrin_head_h8_fwd(const rrin_head_h8_desc* d, void* stream);

/* Flow reuse across t: Ft0/Ft1 of model.py:38-39 recomputed
 * from a kept raw Flow (4 channels) with new per-image coefficients, written to
 * g16 channels 6-9.  The U-Net output itself does not depend on t (model.py:35). */
int rrin_flow_tblend_fwd(const rrin_pp* flow_raw, const rrin_pp* g16, const float* coef, int32_t n,
                         void* stream);
int rrin_flow_tblend_h8(const rrin_h8* flow_raw, const rrin_h8* g16, const float* coef, int32_t n,
                        int32_t prec, void* stream);
/* ABI 25: the same blend for n items over the kept raw Flow of n_pairs pairs: image k of g16 gets
 * Ft0 / Ft1 from image clamp(pair_map[k], 0, n_pairs - 1) of flow_raw with coef row k.  pair_map:
 * device int32 [n].  A null map, n_pairs < 1 or n_pairs > n: RRIN_E_ARG; the other checks are
 * rrin_flow_tblend_h8's.  With pair_map[k] == k it writes what rrin_flow_tblend_h8 writes. */
int rrin_flow_tblend_items_h8(const rrin_h8* flow_raw, const rrin_h8* g16, const float* coef, int32_t n,
                              const int32_t* pair_map, int32_t n_pairs, int32_t prec, void* stream);

/* ---- Whole forward (native schedule) ------------------------------------- */
/* Per-conv weight table entry, in Net conv order (rrin_net_conv_count). */
typedef struct rrin_conv_weights {
  const float* wpack;   /* F32: packed with bm = rrin_conv_cfg_bm(cfg)        */
  const float* bias;    /* packed bias (bm of the config of this precision)  */
  int32_t cfg;          /* F32: rrin_conv_cfg_*; F16*: rrin_conv_h8_cfg_*     */
  float inv_wscale;     /* F16*: from rrin_pack_conv3x3_h8                    */
  const void* whi;      /* F16*: packed halves                                */
  const void* wlo;      /* F16X3: packed lo halves                            */
  int32_t subpixel;     /* F16*, up convs: 1 = whi/wlo/bias hold the sub-pixel
                           weights (4*cout rows) and the upsample pass is skipped;
                           2 = the same with the ring fix-up folded into the conv
                           launch (F32R Winograd kind 3, ksplit <= 1) */
  int32_t ksplit;       /* F32R Winograd kinds 3, 4: rrin_conv_h8_desc.ksplit (0: none);
                           the forward's workspace holds the split scratch */
  const float* wedge;   /* subpixel: original weights [cin][9][cout] fp32      */
  const float* bias_raw;/* subpixel: original bias [cout]                      */
  int32_t fuse_next;    /* F16, level-0 conv a of a UNetConvBlock: 1 = run it and the next
                           conv as one rrin_conv_block0_h8_fwd launch (ABI 14) */
  int32_t pad_;
} rrin_conv_weights;

typedef struct rrin_head_weights {
  const float* w;       /* OIHW, unpacked */
  const float* bias;
} rrin_head_weights;

/* Optional launch profiler: HIP events recorded around every kernel the
 * schedule enqueues (bench.py uses it to time the MFMA conv kernels inside the
 * timed region).  Opaque; created/destroyed by the caller. */
typedef struct rrin_prof rrin_prof;
enum rrin_launch_kind { RRIN_KIND_CONV = 0, RRIN_KIND_HEAD = 1, RRIN_KIND_LAYOUT = 2, RRIN_KIND_EDGE = 3 };

int rrin_prof_create(int32_t capacity, rrin_prof** out);
int rrin_prof_destroy(rrin_prof* p);
int rrin_prof_reset(rrin_prof* p);
/* After the stream has synchronised: per recorded launch its kind, elapsed
 * milliseconds and FLOPs: 2 x the multiply-adds of the form the launch runs.  Planar fp32 convs
 * and every head: the direct form, 2*9*cin*cout per output pixel.  Record-layout convs, by the
 * tile kind of their config (rrin_conv_h8_cfg_wino): 9 multiply-adds per output and input channel
 * in the direct form (kind 0), 4 in Winograd F(2x2,3x3), 3 in F(4,3) x F(2,3) (kind 14); a
 * sub-pixel up conv counts its 4*cout phase rows on the low-res grid, a fused level-0 block both
 * convs' direct form.  So a Winograd launch reports 4/9 or 1/3 of the conv's direct-form FLOPs.
 * 0 for LAYOUT and EDGE launches.  At most the profiler's capacity of launches is recorded; the
 * rest of the call runs unrecorded. */
int rrin_prof_read(rrin_prof* p, int32_t* kinds, float* ms, double* flops, int32_t cap, int32_t* count);
/* Start / end of every recorded launch in ms after the first recorded event
 * (launches on several streams: the union of their spans is the busy time). */
int rrin_prof_read_spans(rrin_prof* p, float* t0_ms, float* t1_ms, int32_t cap, int32_t* count);

typedef struct rrin_net_desc {
  int32_t n, h, w, pad_;
  const float* i0;      /* NCHW [n][3][h][w] */
  const float* i1;
  float* out;           /* NCHW [n][3][h][w] */
  const float* coef;    /* device [n][8] t coefficients */
  /* 4 UNets in execution order Flow, refine_flow, Mask, final; convs of each
   * in UNet order (down a/b per level, mid, up/a/b per level; `last` excluded) */
  const rrin_conv_weights* convs;  /* host array, rrin_net_conv_count() entries */
  const rrin_head_weights* heads;  /* host array of 4 */
  void* workspace;      /* device, >= rrin_net_workspace_bytes, zero-filled once */
  int64_t workspace_bytes;
  int32_t skip_flow;    /* 1: the pair is the one of the previous call on this workspace:
                           reuse its raw Flow (Flow U-Net skipped, t-blend only)      */
  int32_t prec;         /* rrin_prec of the whole forward */
  rrin_prof* prof;      /* nullable: record events around every launch */
  float* taps;          /* nullable (test / debug): the four U-Nets' raw outputs (their `last`
                           conv, before the model.py glue) as NCHW fp32, concatenated:
                           Flow [n][4][h][w] | refine_flow [n][4] | Mask [n][2] | final [n][3]
                           (unet.py:51 outputs used at model.py:35,42,52,62); n*13*h*w floats */
  int32_t* status;      /* optional device int32 (F16X3 / F16 range guard): zeroed at the start
                           of the forward, set to 1 if any activation stored as fp16 overflows
                           (|v| > 65504, inf, NaN); the output is then all NaN (poisoned) instead
                           of silently wrong.  fp32 paths never set it. */
  void* scratch;        /* nullable (ABI 12): device, rrin_net_scratch_bytes(d) bytes, zero-filled
                           once (its ticket words are left zero by every call); F32R split-K
                           slabs of convs with ksplit > 1 (required for them: RRIN_E_WORKSPACE
                           without) and the ring fix-up's cross-workgroup K split (used only
                           when present; the same bits either way).  Kept out of the workspace
                           so plans without splits pay nothing for it. */
  int64_t scratch_bytes;
} rrin_net_desc;

/* Bytes of rrin_net_desc.scratch the forward of d needs with its conv table
 * (0: none; only n, h, w, prec and convs are read).  One forward at a time per scratch. */
int64_t rrin_net_scratch_bytes(const rrin_net_desc* d);

int rrin_net_conv_count(void);                 /* 77 = 81 convs - 4 heads      */

/* One U-Net alone -- the reference UNet(in_channels, n_classes, depth).forward
 * (unet.py:40-51): x NCHW [n][in_ch][h][w] -> y NCHW [n][out_ch][h][w], with
 * the Net's kernels and workspace plan (rrin_net_workspace_bytes of the same
 * n, h, w, prec); in_ch <= 16, out_ch 2..4, depth 2..5.  convs: the U-Net's
 * rrin_unet_conv_count(depth) body convs in UNet order (down a/b per level,
 * mid, up/a/b per level), packed as for rrin_net_fwd (no input permutation);
 * head: its `last` conv, OIHW.  Channels [in_ch, 16) of the workspace's input
 * buffer must be finite (a zero-filled workspace only ever used for U-Nets of
 * one in_ch keeps them zero). */
typedef struct rrin_unet_desc {
  int32_t n, h, w, in_ch, out_ch, depth, prec, pad_;
  const float* x;
  float* y;
  const rrin_conv_weights* convs;  /* host array */
  rrin_head_weights head;
  void* workspace;
  int64_t workspace_bytes;
  rrin_prof* prof;                 /* nullable */
  int32_t* status;                 /* optional device int32: the F16X3 / F16 range guard, as rrin_net_desc */
  void* scratch;                   /* nullable (ABI 12): as rrin_net_desc.scratch, rrin_unet_scratch_bytes */
  int64_t scratch_bytes;
} rrin_unet_desc;
int64_t rrin_unet_conv_count(int32_t depth);
int64_t rrin_unet_scratch_bytes(const rrin_unet_desc* d);
int rrin_unet_fwd(const rrin_unet_desc* d, void* stream);
int64_t rrin_net_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t prec);
int rrin_net_fwd(const rrin_net_desc* d, void* stream);

/* ABI 20: the forward on 8-bit frames of any size, already on the device: f0 / f1 uint8
 * [n][h0][w0][3] in, out_u8 uint8 [n][h0][w0][3] out; bit for bit the host chain "edge-pad to
 * /16 (top, right) and divide by 255 -> rrin_net_fwd -> multiply by 255, truncate, crop"
 * (rrin_pack_g16_u8_h8 in, the FINAL head's rrin_head_h8_desc.out_u8 store out: no fp32 NCHW
 * frame exists on this path).  net.n / h / w are the padded size, h == round_up(h0,16) and
 * w == round_up(w0,16) (RRIN_E_SHAPE otherwise, and for h0, w0 < 1); net.i0 / i1 / out are
 * ignored and may be NULL; every other field of net means what it means for rrin_net_fwd.  The
 * record precisions only: RRIN_PREC_F32 (planar) returns RRIN_E_ARG, as do null frames.  With
 * the range guard set (net.status) the poisoned pixels are written as 0.  Arguments are
 * validated before any HIP call. */
typedef struct rrin_net_u8_desc {
  rrin_net_desc net;
  const uint8_t* f0;    /* [n][h0][w0][3], every frame dense */
  const uint8_t* f1;
  int64_t img_stride;   /* bytes between frames of f0 and of f1 (>= h0*w0*3) */
  uint8_t* out_u8;      /* [n][h0][w0][3] contiguous */
  int32_t h0, w0;
} rrin_net_u8_desc;
int rrin_net_u8_fwd(const rrin_net_u8_desc* d, void* stream);

/* ABI 22: the same forward on 8-bit YUV 4:2:0 frames (NV12 or I420), in and out on the device:
 * by definition rgb_to_yuv420(rrin_net_u8_fwd(yuv420_to_rgb(f0), yuv420_to_rgb(f1))) with the
 * integer conversions of rrin_yuv_coef, bit for bit -- rrin_pack_g16_yuv_h8 in, the FINAL head's
 * rrin_head_h8_desc.out_yuv store out; no RGB frame exists on the device.  net as for
 * rrin_net_u8_fwd (same schedule, skip_flow, range guard -- a poisoned pixel is RGB (0,0,0)
 * before the conversion -- and record precisions only).  h0 and w0 even.  Null planes, a c_step
 * not 1 or 2: RRIN_E_ARG; odd sizes, pitches smaller than a row, overlapping frames:
 * RRIN_E_SHAPE.  Arguments are validated before any HIP call.  ABI 24: f0, f1 and out share
 * chroma (RRIN_E_ARG otherwise); at RRIN_CHROMA_422 / 444 the sizes follow rrin_yuv420's rules
 * and the definition reads rgb_to_yuv(rrin_net_u8_fwd(yuv_to_rgb(f0), yuv_to_rgb(f1))) with the
 * block of that format. */
typedef struct rrin_net_yuv_desc {
  rrin_net_desc net;
  rrin_yuv420 f0, f1;   /* n frames each; may be two views of one [n+1] stack */
  rrin_yuv420 out;      /* n frames, written through the const pointers */
  rrin_yuv_coef coef;
  int32_t h0, w0;
  int32_t pad_;
} rrin_net_yuv_desc;
int rrin_net_yuv_fwd(const rrin_net_yuv_desc* d, void* stream);

/* ABI 23: rrin_net_u8_fwd on 16-bit RGB frames of depth 9..16 (RRIN_E_ARG otherwise): bit for bit
 * "edge-pad, min(word, maxval) / maxval -> rrin_net_fwd -> multiply by maxval, truncate, crop"
 * (rrin_pack_g16_u16_h8 in, rrin_head_h8_desc.out_u16 out).  img_stride in samples
 * (>= h0*w0*3); everything else as rrin_net_u8_fwd. */
typedef struct rrin_net_u16_desc {
  rrin_net_desc net;
  const uint16_t* f0;   /* [n][h0][w0][3], every frame dense */
  const uint16_t* f1;
  int64_t img_stride;
  uint16_t* out_u16;    /* [n][h0][w0][3] contiguous */
  int32_t h0, w0, depth, pad_;
} rrin_net_u16_desc;
int rrin_net_u16_fwd(const rrin_net_u16_desc* d, void* stream);

/* ABI 23: rrin_net_yuv_fwd on 16-bit 4:2:0 frames of depth 10 or 12: by definition
 * rgb16_to_yuv420(rrin_net_u16_fwd(yuv420_to_rgb16(f0), yuv420_to_rgb16(f1))) at that depth.  f0,
 * f1 and out share depth, shift and chroma (RRIN_E_ARG otherwise); the checks of rrin_net_yuv_fwd apply,
 * with the coefficient bounds of rrin_yuv420_16. */
typedef struct rrin_net_yuv16_desc {
  rrin_net_desc net;
  rrin_yuv420_16 f0, f1;   /* n frames each; may be two views of one [n+1] stack */
  rrin_yuv420_16 out;      /* n frames, written through the const pointers */
  rrin_yuv_coef coef;
  int32_t h0, w0;
  int32_t pad_;
} rrin_net_yuv16_desc;
int rrin_net_yuv16_fwd(const rrin_net_yuv16_desc* d, void* stream);

/* ABI 25: item forwards.  A frame forward whose batch is a list of net.n ITEMS (pair index, t)
 * over n_pairs <= net.n distinct pairs: f0 / f1 hold n_pairs frames each (two views of one
 * [n_pairs + 1] stack), out holds net.n frames, net.coef has one row per item, and item k is, bit
 * for bit, the frame that the plain forward of pair pair_map[k] alone returns for coef row k.  The
 * Flow U-Net runs once over the n_pairs pairs, the other three U-Nets over the net.n items; both
 * phases share the one workspace and scratch of a plain forward of net.n (rrin_net_workspace_bytes
 * / rrin_net_scratch_bytes with n = net.n): no buffer's image stride depends on the batch, so the
 * Flow phase uses images [0, n_pairs) of the same plan.  net.skip_flow = 1 skips the Flow phase:
 * the workspace then keeps the raw Flow of the same n_pairs pairs from the previous item call.
 * pair_map: device int32 [net.n]; its values are clamped to [0, n_pairs) where they are read, so
 * no map reads outside the stacks (callers check them on the host).  Validated before any HIP
 * call: a null rrin_items, n_pairs < 1, n_pairs > net.n, a null map with n_pairs != net.n, or
 * net.taps set: RRIN_E_ARG; then the frame forward's own checks, with the stride / span rules of
 * f0 and f1 applied to n_pairs frames and those of out to net.n.  A null map with
 * n_pairs == net.n is the plain forward. */
typedef struct rrin_items {
  int32_t n_pairs;
  int32_t pad_;
  const int32_t* pair_map;
} rrin_items;
int rrin_net_u8_items_fwd(const rrin_net_u8_desc* d, const rrin_items* items, void* stream);
int rrin_net_yuv_items_fwd(const rrin_net_yuv_desc* d, const rrin_items* items, void* stream);
int rrin_net_u16_items_fwd(const rrin_net_u16_desc* d, const rrin_items* items, void* stream);
int rrin_net_yuv16_items_fwd(const rrin_net_yuv16_desc* d, const rrin_items* items, void* stream);

/* ---- Low-resolution flow estimation: flow_scale 2 and 4 (csrc/flow_scale.hip, net.hip; the byte-frame entries: net_frames.hip) ----
 * History: added after ABI 25 without a new version number -- a new struct passed to new entry
 * points only, no existing struct or entry point changes, so RRIN_ABI_VERSION stays 25; a caller
 * finds out whether a build has them by looking the symbols up.
 *
 * The forward with model.py:35, `Flow = self.Flow(x)`, replaced by
 *   Flow = s * F.interpolate(self.Flow(F.avg_pool2d(x, s)), scale_factor=s, mode="bilinear",
 *                            align_corners=False)
 * for s = 2 or 4; everything after that line runs at full size (rrin_amd/flowscale.py).  The padded
 * size is the frame size rounded up to a multiple of 16 * s.
 *
 * rrin_g16_downscale_h8: F.avg_pool2d(x, s) of channels 0-5 of n images of the full-size Net buffer
 * src (16 channels, h x w) into the Net buffer dst of a plan at exactly (h / s, w / s); channels 6-15
 * of dst are zeroed.  Per value in fp32, in raster order of the s x s block: s = 2
 * (((p00 + p01) + p10) + p11) * 0.25f; s = 4 the 16 values row by row, then * 0.0625f; stored with
 * the format's rounding.  Only interior records of dst are written (its conv halo stays zero).
 *
 * rrin_flow_upscale_h8: s * F.interpolate(flow, scale_factor=s, bilinear, align_corners=False) of
 * the 4-channel raw Flow src (a plan at (h / s, w / s)) into the raw Flow dst at h x w.  Source
 * coordinate (dst + 0.5) / s - 0.5, clamped to the image; the weights are exact dyadic numbers;
 *   v = (1-wy) * ((1-wx)*p00 + wx*p01) + wy * ((1-wx)*p10 + wx*p11)
 * with every operation rounded to fp32 (no contraction), then v * s, stored with the format's
 * rounding as a whole record (its channels past 3 zero).  status: optional fp16 range flag, set
 * where a stored value leaves the fp16 range (ignored for F32R).
 *
 * Both: a null view, s not 2 or 4, n < 1, a prec that is no record precision: RRIN_E_ARG; views
 * that fail the layout checks, g_off != 0, fewer channels than 16 (downscale) / 4 (upscale), sizes
 * that are not the exact quotient: RRIN_E_SHAPE.  Validated before any HIP call. */
int rrin_g16_downscale_h8(const rrin_h8* src, const rrin_h8* dst, int32_t n, int32_t s, int32_t prec, void* stream);
int rrin_flow_upscale_h8(const rrin_h8* src, const rrin_h8* dst, int32_t n, int32_t s, int32_t prec,
                         int32_t* status, void* stream);

/* The second plan of a flow_scale forward of net (n, h, w, prec): the Flow U-Net runs at
 * (h / s, w / s) with its own memory, because its interior writes would land in the zero halos of
 * the full-size plan.  workspace: rrin_net_workspace_bytes(n, h / s, w / s, prec) bytes, zero-filled
 * once; convs: the conv table for that size (at least the Flow U-Net's rrin_unet_conv_count(5)
 * entries, packed as for rrin_net_fwd); scratch: rrin_net_scratch_bytes of (n, h / s, w / s, prec,
 * convs), nullable when that is 0.  The range flag is net.status. */
typedef struct rrin_flow_scale {
  int32_t s;            /* 2 or 4 */
  int32_t pad_;
  const rrin_conv_weights* convs;
  void* workspace;
  int64_t workspace_bytes;
  void* scratch;
  int64_t scratch_bytes;
} rrin_flow_scale;
/* The forwards with the second plan: rrin_net_fwd (record precisions only) and the four frame
 * forwards, plain (items NULL) or as item forwards.  net.h / net.w are the frame size rounded up to
 * 16 * s (RRIN_E_SHAPE otherwise).  Order: pack into the full-size g16 (once for a plain forward;
 * an item forward packs its n_pairs pairs, then its items), downscale, the Flow U-Net on the second
 * plan, upscale into the full-size raw Flow, then the blend of the kept raw Flow and the other three
 * U-Nets as for skip_flow.  net.skip_flow = 1 skips all of the Flow phase: the workspace keeps the
 * upscaled raw Flow of the previous call, which must have been one of the same s.  A null or
 * malformed rrin_flow_scale, net.taps set, RRIN_PREC_F32: RRIN_E_ARG; a second workspace that is too
 * small: RRIN_E_WORKSPACE; then the checks of the forward itself.  Validated before any HIP call. */
int rrin_net_scaled_fwd(const rrin_net_desc* d, const rrin_flow_scale* fs, void* stream);
int rrin_net_u8_scaled_fwd(const rrin_net_u8_desc* d, const rrin_items* items, const rrin_flow_scale* fs,
                           void* stream);
int rrin_net_yuv_scaled_fwd(const rrin_net_yuv_desc* d, const rrin_items* items, const rrin_flow_scale* fs,
                            void* stream);
int rrin_net_u16_scaled_fwd(const rrin_net_u16_desc* d, const rrin_items* items, const rrin_flow_scale* fs,
                            void* stream);
int rrin_net_yuv16_scaled_fwd(const rrin_net_yuv16_desc* d, const rrin_items* items, const rrin_flow_scale* fs,
                              void* stream);

/* ---- Scene-cut / duplicate-frame gate of the 8-bit frame path (ABI 21) ------------------
 * Three small kernels for the stream of a rrin_net_u8_fwd call, so that a caller can replace the
 * interpolated frame of a pair that is a shot change or a repeated frame by one of its input
 * frames without a host round trip.  Frames as for rrin_pack_g16_u8_h8: uint8 [n][h0][w0][3],
 * every frame dense, img_stride bytes between frames of a stack (>= h0*w0*3, RRIN_E_ARG
 * otherwise); f0 and f1 may be two views of one [n+1] stack, so a frame may start at any byte
 * address.  Null pointers: RRIN_E_ARG; n, h0 or w0 < 1 (or n > 65535): RRIN_E_SHAPE.  Arguments
 * are validated before any HIP call.
 *
 * rrin_pair_sad_u8: sad[p] = sum over the h0*w0*3 bytes of pair p of |f0[p] - f1[p]|, exact (an
 * integer sum in 64 bits: the same value whatever the reduction order).  sad (8-byte aligned) is
 * overwritten: its prior contents do not matter.
 * rrin_gate_from_sad_u8: gate[p] = 1 if sad[p] == 0 (a duplicate), else cut_code if
 * sad[p] > limit (a cut), else 0; cut_code is 1 or 2 (RRIN_E_ARG otherwise).
 * rrin_gate_frames_u8: out uint8 [n][h0][w0][3] contiguous; gate[p] == 1 overwrites frame p of
 * out with f0's frame p, gate[p] == 2 with f1's; any other code leaves every byte of the frame
 * as it is (the pair's workgroups exit after reading the code). */
int rrin_pair_sad_u8(const uint8_t* f0, const uint8_t* f1, int64_t img_stride, int32_t n, int32_t h0,
                     int32_t w0, uint64_t* sad, void* stream);
int rrin_gate_from_sad_u8(const uint64_t* sad, int32_t n, uint64_t limit, int32_t cut_code, int32_t* gate,
                          void* stream);
int rrin_gate_frames_u8(const uint8_t* f0, const uint8_t* f1, int64_t img_stride, int32_t n, int32_t h0,
                        int32_t w0, const int32_t* gate, uint8_t* out, void* stream);
/* ABI 23: rrin_pair_sad_u8 on 16-bit words: sad[p] = sum over the h0*w0*3 samples of pair p of
 * |a - b| with a, b = min(word >> shift, 2^depth - 1), exact; depth 9..16 and
 * 0 <= shift <= 16 - depth (RRIN_E_ARG otherwise); img_stride in samples; a frame may start at
 * any even address.  The code and copy kernels serve 16-bit frames as they are:
 * rrin_gate_frames_u8 with w0 and img_stride doubled copies whole words. */
int rrin_pair_sad_u16(const uint16_t* f0, const uint16_t* f1, int64_t img_stride, int32_t n, int32_t h0,
                      int32_t w0, int32_t depth, int32_t shift, uint64_t* sad, void* stream);
/* ABI 24: the same three on frames that are blobs of any length (a dense 4:2:2 frame is
 * 2*h0*w0 bytes, no multiple of 3 in general): len bytes (rrin_pair_sad_u16_len: samples) per
 * frame in place of h0 and w0, img_stride >= len; len < 1: RRIN_E_SHAPE.  The same kernels, the
 * same exactness and error rules: rrin_pair_sad_u8 / _u16 / rrin_gate_frames_u8 are these with
 * len = h0*w0*3. */
int rrin_pair_sad_u8_len(const uint8_t* f0, const uint8_t* f1, int64_t img_stride, int32_t n, int64_t len,
                         uint64_t* sad, void* stream);
int rrin_pair_sad_u16_len(const uint16_t* f0, const uint16_t* f1, int64_t img_stride, int32_t n, int64_t len,
                          int32_t depth, int32_t shift, uint64_t* sad, void* stream);
int rrin_gate_frames_u8_len(const uint8_t* f0, const uint8_t* f1, int64_t img_stride, int32_t n, int64_t len,
                            const int32_t* gate, uint8_t* out, void* stream);
/* ABI 25: the gate of an item forward.  The sums and rrin_gate_from_sad_u8 (with cut_code 2) run
 * once per pair; an item inherits its pair's decision.
 * rrin_gate_items_u8: gate[k] = 1 if pair_gate[p] == 1 (a duplicate: the first frame), cut_codes[k]
 * if pair_gate[p] == 2 (a cut: the item's own nearer frame, 1 or 2; anything else gives 0), else
 * 0, with p = clamp(pair_map[k], 0, n_pairs - 1); all arrays on the device, pair_gate [n_pairs],
 * the others [n].
 * rrin_gate_frames_items_u8_len: rrin_gate_frames_u8_len for n output frames whose sources are
 * frame p (as above) of f0 / f1.  Null pointers, n_pairs < 1 or n_pairs > n: RRIN_E_ARG. */
int rrin_gate_items_u8(const int32_t* pair_gate, int32_t n_pairs, const int32_t* pair_map, const int32_t* cut_codes,
                       int32_t n, int32_t* gate, void* stream);
int rrin_gate_frames_items_u8_len(const uint8_t* f0, const uint8_t* f1, int64_t img_stride, int32_t n, int64_t len,
                                  const int32_t* gate, uint8_t* out, const int32_t* pair_map, int32_t n_pairs,
                                  void* stream);

/* ---- Frame metrics: squared error and SSIM per plane, on the device --------------------------
 * History: added after ABI 25 without a new version number -- entry points only, no struct or
 * existing entry point changes, so RRIN_ABI_VERSION stays 25; a caller finds out whether a build
 * has them by looking the symbols up.
 *
 * A plane of a frame: sample (r, c), 0 <= r < h, 0 <= c < w, is element off + r*pitch + c*step of
 * the frame (an element is a byte for rrin_frame_metrics_u8, a 16-bit word for _u16).  RGB
 * [h][w][3] is three planes of step 3 and pitch 3*w at off 0, 1, 2; interleaved chroma two of step
 * 2; a planar plane has step 1.
 *
 * rrin_frame_metrics_u8 / _u16: for frame k < n of the stacks a and b (a_stride / b_stride elements
 * between frames, each at least the planes' reach; any byte address, for _u16 any even one) and
 * plane p < n_planes (1..4; a host array, copied by the call):
 *   sse[k*n_planes + p]  = sum over the plane's h*w samples of (a - b)^2, exact;
 *   ssim[k*n_planes + p] (flags & 1) = the mean over the windows of the 8x8-window, 4-sample-step
 *     SSIM as rrin_amd/metrics.py defines it: with bh = h/4, bw = w/4 and per 4x4 block the integer
 *     sums s1 = sum a, s2 = sum b, ss = sum a^2 + b^2, s12 = sum ab, window (i, j), i < bh-1,
 *     j < bw-1, adds blocks (i..i+1, j..j+1) to S1, S2, SS, S12 and is worth
 *     ((2*S1*S2 + C1) * (2*covar + C2)) / ((S1^2 + S2^2 + C1) * (vars + C2)), vars = 64*SS - S1^2 -
 *     S2^2, covar = 64*S12 - S1*S2, C1 = floor(1e-4 * M^2 * 64 + 0.5), C2 = floor(9e-4 * M^2 * 64 * 63
 *     + 0.5), M = 2^depth - 1 (255 for _u8): the four factors exact integers, two float64
 *     products, one division; samples beyond 4*bh, 4*bw take no part.
 * _u16 reads a sample as min(word >> shift, M), depth 9..16, 0 <= shift <= 16 - depth (RRIN_E_ARG
 * otherwise).  No byte outside a plane's rows is read.  The result is the same bits on every run
 * (no floating-point atomics: per-workgroup partials in the workspace, added in index order).
 * sse, ssim and workspace are 8-byte aligned device memory; ssim may be NULL without the flag;
 * workspace_bytes >= rrin_frame_metrics_workspace_bytes(...) (RRIN_E_WORKSPACE otherwise; the query
 * returns a negative error code for arguments the call would refuse).
 * Null pointers, n_planes outside 1..4, step outside 1..3, off < 0, pitch < (w-1)*step + 1, a stride
 * below the planes' reach, flags other than 0 / 1, an odd _u16 address: RRIN_E_ARG; n, h or w < 1,
 * n > 65535, or the flag with h or w < 8 (no window): RRIN_E_SHAPE.  Validated before any launch.
 * rrin_frame_metrics_tile: the kernel's tile, for tests that want sizes around it: a wave covers
 * tile_cols window columns and band_rows window rows per step. */
typedef struct rrin_plane {
  int64_t off, pitch;
  int32_t step, h, w, pad;
} rrin_plane;
int64_t rrin_frame_metrics_workspace_bytes(int32_t n, const rrin_plane* planes, int32_t n_planes, int32_t flags);
int rrin_frame_metrics_u8(const uint8_t* a, int64_t a_stride, const uint8_t* b, int64_t b_stride, int32_t n,
                          const rrin_plane* planes, int32_t n_planes, int32_t flags, uint64_t* sse, double* ssim,
                          void* workspace, int64_t workspace_bytes, void* stream);
int rrin_frame_metrics_u16(const uint16_t* a, int64_t a_stride, const uint16_t* b, int64_t b_stride, int32_t n,
                           const rrin_plane* planes, int32_t n_planes, int32_t flags, int32_t depth, int32_t shift,
                           uint64_t* sse, double* ssim, void* workspace, int64_t workspace_bytes, void* stream);
int rrin_frame_metrics_tile(int32_t* tile_cols, int32_t* band_rows);

/* ---- Fine-tuning on a clip: triplet sampler and loss (csrc/finetune.hip) ----------------------
 * History: added after ABI 25 without a new version number -- entry points only, no struct or
 * existing entry point changes, so RRIN_ABI_VERSION stays 25; a caller finds out whether a build
 * has them by looking the symbols up.
 *
 * rrin_triplet_crop_u8 / _u16: training triplets from one stack of n_frames frames on the device
 * (frame_stride elements between frames; an element is a byte, for _u16 a 16-bit word at an even
 * address).  planes[3] describe a frame as rrin_frame_metrics_* read it: Y, U, V of any layout
 * (the chroma block -- one sample per pixel, per 2x1 or per 2x2 pixels -- follows from the plane
 * sizes), with coef the colour conversion; or, with coef NULL, R, G, B of one size (interleaved
 * RGB: step 3).  items: a host array of n_items x 6 int32 (frame0, frame_t, frame1, y0, x0, flip),
 * copied by the call, 1 <= n_items <= RRIN_TRIPLET_MAX_ITEMS.  i0, it, i1: contiguous fp32
 * [n_items][3][ch][cw] on the device, 16-byte aligned.  For item k and its frame f of the three,
 * in frame coordinates (rrin_amd/finetune.py: sample_triplets is the definition, bit for bit):
 *   rgb(y, x) = the frame's R, G, B at pixel (y0 + y, x0 + x), 0 <= y < ch, 0 <= x < cw: the
 *               planes' samples, or rrin_yuv_coef's YUV -> RGB (rrin_yuv420_16's at depth 10 / 12)
 *               of the pixel's luma and its block's chroma;
 *   value     = float(rgb) / float(maxval), the IEEE fp32 division (maxval 255, or 2^depth - 1 with
 *               a sample read as min(word >> shift, maxval));
 *   flip 0: out[k][c][y][x] = value(y, x); 1 (left-right): value(y, cw-1-x); 2 (top-bottom):
 *               value(ch-1-y, x).
 * No element outside the crops' rows is read, no float outside the three outputs written.
 * RRIN_E_ARG: a null pointer, an odd _u16 address, an output not 16-byte aligned, a plane with
 * step outside 1..3, off < 0 or pitch < (w-1)*step + 1, a frame_stride below the planes' reach, a
 * frame index outside [0, n_frames), a flip outside 0..2, an origin that is no multiple of the
 * chroma block, a coefficient out of range, _u16 with depth outside 9..16 or shift outside
 * 0..16-depth, or with coef at a depth other than 10 or 12.  RRIN_E_SHAPE: n_frames < 1, n_items
 * outside 1..RRIN_TRIPLET_MAX_ITEMS, ch or cw no positive multiple of 16, a crop that leaves
 * the luma plane (or is larger than it), chroma planes that are no 1x1, 2x1 or 2x2 reduction of the
 * luma plane (coef NULL: planes of different sizes).  Validated before any launch.
 *
 * rrin_tloss: the training loss and its gradient in one pass over out and target (contiguous
 * fp32, count = N*C*H*W >= 1 elements, 4-byte aligned; 16-byte aligned data takes 16-byte loads).
 * With d = out - target, per element in fp32 (IEEE sqrt and division, no contraction):
 *   sums[0] = sum sqrt(d*d + eps)   sums[1] = sum |d|   sums[2] = sum d*d          (float64)
 *   grad    = float(w_charb / n) * d / sqrt(d*d + eps) + float(w_l1 / count) * sign(d), sign(0) = 0
 * which is the gradient of loss = w_charb * sums[0] / n + w_l1 * sums[1] / count (the reference's
 * charbonnierLoss / 1e3 + L1Loss / 10 at w_charb 1e-3, w_l1 1e-1, eps 1e-6).  The sums are per-
 * workgroup float64 partials in the workspace, added in index order by a last step: no floating-
 * point atomics, the same bits on every run.  grad may be NULL.  sums (3 doubles) and workspace are
 * 8-byte aligned device memory, workspace_bytes >= rrin_tloss_workspace_bytes(count)
 * (RRIN_E_WORKSPACE otherwise; the query returns RRIN_E_SHAPE for count < 1).  A null required
 * pointer, a misaligned one, eps <= 0 or a weight that is not finite: RRIN_E_ARG; count < 1 or
 * n < 1: RRIN_E_SHAPE.  Validated before any launch. */
#define RRIN_TRIPLET_MAX_ITEMS 64
int rrin_triplet_crop_u8(const uint8_t* frames, int64_t frame_stride, int32_t n_frames, const rrin_plane* planes,
                         const int32_t* items, int32_t n_items, int32_t ch, int32_t cw, const rrin_yuv_coef* coef,
                         float* i0, float* it, float* i1, void* stream);
int rrin_triplet_crop_u16(const uint16_t* frames, int64_t frame_stride, int32_t n_frames, const rrin_plane* planes,
                          const int32_t* items, int32_t n_items, int32_t ch, int32_t cw, const rrin_yuv_coef* coef,
                          int32_t depth, int32_t shift, float* i0, float* it, float* i1, void* stream);
int64_t rrin_tloss_workspace_bytes(int64_t count);
int rrin_tloss(const float* out, const float* target, int64_t count, int32_t n, double w_charb, double w_l1,
               float eps, double* sums, float* grad, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- The perceptual (VGG feature) term of fine-tuning (csrc/perceptual.hip) --------------------
 * History: added after ABI 25 without a new version number -- entry points only, no struct or
 * existing entry point changes, so RRIN_ABI_VERSION stays 25; a caller finds out whether a build
 * has them by looking the symbols up.
 *
 * What torchvision's vgg19().features[:-10] needs besides its convs (those are rrin_tconv3x3 / the
 * Winograd training route with leaky = 0), and the distance of two feature tensors;
 * rrin_amd/perceptual.py is the definition.  All tensors are contiguous fp32 on the device, 4-byte
 * aligned; 16-byte aligned tensors (pool: and w a multiple of 4) take 16-byte accesses.
 *
 * rrin_trelu_fwd: y = x < 0 ? +0 : x over count elements -- torch.relu's bits: -0 and a NaN pass.
 * rrin_trelu_bwd: gx = y > 0 ? gy : 0 with y the forward's output (0 where y is a NaN).  In place is
 * allowed: x == y, gy == gx (any other overlap is not).
 *
 * rrin_tmaxpool2_fwd: MaxPool2d(2, 2) of x [nc][h][w] into y [nc][h/2][w/2].  A window is scanned in
 * row-major order and a later element replaces the maximum if it is greater or a NaN (PyTorch's CPU
 * rule): of equal maxima the first is the arg-max, with NaNs the last NaN, and y is then a NaN.
 * rrin_tmaxpool2_bwd: gx [nc][h][w] from gy [nc][h/2][w/2] and the forward's input x: the arg-max is
 * found in x again and gets the window's gy, the window's other three elements get 0 -- every element
 * of gx is written, by the one lane that owns its window; no index tensor, no atomics.
 *
 * rrin_tfeatdist: sums[0] = sum (a - b)^2 over count elements in float64 (each difference exact, each
 * square rounded once) and, unless grad is NULL, grad = (a - b) / sqrt(sums[0]) divided in float64 and
 * rounded to fp32 -- the gradient of torch.norm(a - b, 2) with respect to a; all zeros when the sum is
 * 0.  The sum is rrin_tloss's reduction: float64 per lane, a fixed shuffle tree, one partial per
 * workgroup in the workspace, added in index order by a one-workgroup step: no atomics, the same bits
 * on every run.  grad is a further launch that reads sums[0] from device memory (no host round
 * trip).  sums (1 double) and workspace are 8-byte aligned device memory, workspace_bytes >=
 * rrin_tfeatdist_workspace_bytes(count) (RRIN_E_WORKSPACE otherwise; the query returns RRIN_E_SHAPE
 * for count < 1).
 *
 * Codes, all returned before any launch: a null required pointer or a misaligned one: RRIN_E_ARG;
 * count < 1, nc < 1, h or w odd or < 2: RRIN_E_SHAPE; a workspace that is too small:
 * RRIN_E_WORKSPACE. */
int rrin_trelu_fwd(const float* x, float* y, int64_t count, void* stream);
int rrin_trelu_bwd(const float* gy, const float* y, float* gx, int64_t count, void* stream);
int rrin_tmaxpool2_fwd(const float* x, float* y, int32_t nc, int32_t h, int32_t w, void* stream);
int rrin_tmaxpool2_bwd(const float* gy, const float* x, float* gx, int32_t nc, int32_t h, int32_t w, void* stream);
int64_t rrin_tfeatdist_workspace_bytes(int64_t count);
int rrin_tfeatdist(const float* a, const float* b, int64_t count, double* sums, float* grad, void* workspace,
                   int64_t workspace_bytes, void* stream);

/* ---- An extra plane (alpha, depth, ID) through the byte-frame forwards (csrc/plane.hip, net.hip, net_frames.hip) --
 * History: added after ABI 25 without a new version number -- a new struct passed to new entry
 * points only, no existing struct or entry point changes, so RRIN_ABI_VERSION stays 25; a caller
 * finds out whether a build has them by looking the symbols up.
 *
 * One single-channel image per input frame, in the frames' element type, carried to time t by the
 * picture's own motion (rrin_amd/plane.py is the definition): with A0 / A1 the planes padded as the
 * frames are (edge replication on top and on the right) and divided by maxval,
 *   at0 = warp(A0, Flow_t_0)   at1 = warp(A1, Flow_t_1)      the refined flows (model.py:44-45)
 *   A_t = clamp((w1 at0 + w2 at1) / (w1 + w2 + 1e-8), 0, 1)   w1, w2: the picture's mask weights
 * stored as (int)(A_t * maxval), the crop only.  The final U-Net does not touch the plane.
 *
 * rrin_aux_plane (the name rrin_plane is the metrics' plane description): a0 / a1 the planes of the
 * pairs' first / second frames, [frames][h0] rows of in_pitch elements, in_stride elements between
 * frames (two views of one [frames + 1] stack are fine); out [n][h0] rows of out_pitch elements,
 * out_stride between frames.  depth 8: uint8 elements (shift 0); depth 9..16: uint16 words at even
 * addresses, a sample is min(word >> shift, 2^depth - 1) and is stored << shift,
 * 0 <= shift <= 16 - depth.  scratch: rrin_plane_scratch_bytes(n, h, w) bytes of device memory, 16 per
 * padded pixel: fp32 [n][2][h][w] at0 / at1, then fp32 [n][2][h][w] mask logits.
 *
 * rrin_plane_warp_h8: at0 / at1 of n images into the scratch, from the flows that the REFINE head
 * stored in channels 6-9 of g16 (read as the record format stores them) and the same warp_taps as
 * the picture's backwarp: bilinear, zeros outside the padded h x w = g16's size, align_corners =
 * False; padded pixel (y, x) is plane sample (max(y - top, 0), min(x, w0 - 1)), top = h - h0.
 * pair_map NULL: image k reads frame k (n_pairs == n); else frame clamp(pair_map[k], 0, n_pairs - 1).
 * rrin_plane_blend_h8: A_t of n images of padded size h x w from the scratch (at0 / at1 and the two
 * mask logits per pixel, as the MASK head's raw_out wrote them) with coef [n][8] (rrin_net_desc.coef),
 * quantised into the crop of out.  status: optional fp16 range flag; where it is set and prec is
 * F16X3 or F16 every sample is stored as 0, as the FINAL head stores its bytes.  Padding pixels and
 * elements between rows or frames of out are not written.
 * Both: a null pointer, a prec that is no record precision, depth outside 8..16 or shift outside
 * 0..16 - depth (depth 8: shift 0), an odd word address, a pitch below w0, a stride below h0 * pitch
 * with more than one frame, scratch_bytes too small, n_pairs outside [1, n] or != n without a map:
 * RRIN_E_ARG; n, h0, w0 < 1, h0 > h, w0 > w, a g16 that fails the layout checks: RRIN_E_SHAPE.
 * Validated before any launch.
 *
 * rrin_net_*_plane_fwd: the frame forwards with three nullable companions.  items NULL: a plain
 * forward, else an item forward; fs NULL: flow_scale 1, else the rrin_net_*_scaled_fwd call; plane
 * NULL: exactly those calls.  With a plane the forward launches rrin_plane_warp_h8 behind the REFINE
 * head (the MASK head overwrites g16 channels 6-8, so the refined flows are gone by the time the
 * mask is known), points the MASK head's raw_out into the scratch and launches rrin_plane_blend_h8
 * behind it; nothing else changes, the frames are the same bits.  The planes hold the frames'
 * n (items: n_pairs) and the output net.n images.  Refused with RRIN_E_ARG before any launch:
 * RRIN_PREC_F32, a plane whose depth is not the frames', net.taps, and what the kernels refuse. */
typedef struct rrin_aux_plane {
  const void* a0;
  const void* a1;
  void* out;
  int64_t in_stride, out_stride; /* elements between frames                              */
  int32_t in_pitch, out_pitch;   /* elements between rows                                */
  int32_t depth, shift;
  void* scratch;
  int64_t scratch_bytes;
} rrin_aux_plane;
int64_t rrin_plane_scratch_bytes(int32_t n, int32_t h, int32_t w);
int rrin_plane_warp_h8(const rrin_h8* g16, const rrin_aux_plane* plane, int32_t n, int32_t h0, int32_t w0,
                       const int32_t* pair_map, int32_t n_pairs, int32_t prec, void* stream);
int rrin_plane_blend_h8(const rrin_aux_plane* plane, const float* coef, int32_t n, int32_t h, int32_t w, int32_t h0,
                        int32_t w0, int32_t prec, const int32_t* status, void* stream);
int rrin_net_u8_plane_fwd(const rrin_net_u8_desc* d, const rrin_items* items, const rrin_flow_scale* fs,
                          const rrin_aux_plane* plane, void* stream);
int rrin_net_u16_plane_fwd(const rrin_net_u16_desc* d, const rrin_items* items, const rrin_flow_scale* fs,
                           const rrin_aux_plane* plane, void* stream);
int rrin_net_yuv_plane_fwd(const rrin_net_yuv_desc* d, const rrin_items* items, const rrin_flow_scale* fs,
                           const rrin_aux_plane* plane, void* stream);
int rrin_net_yuv16_plane_fwd(const rrin_net_yuv16_desc* d, const rrin_items* items, const rrin_flow_scale* fs,
                             const rrin_aux_plane* plane, void* stream);

/* ---- The exposure of a synthetic shutter: the rounded mean of byte frames ---------------------
 * History: added after ABI 25 without a new version number -- one new entry point, no struct and no
 * existing entry point changes, so RRIN_ABI_VERSION stays 25; a caller finds out whether a build
 * has it by looking the symbol up.
 *
 * rrin_mean_frames (rrin_amd/exposure.py is the definition): g output frames of len elements each,
 * frame j at out + j * out_stride (elements).  frames: a DEVICE table of k frame pointers (8-byte
 * aligned); start: a DEVICE int32 [g + 1] in CSR form, start[0] = 0 <= ... <= start[g] = k: output j is
 * the mean of the S = start[j+1] - start[j] frames frames[start[j] .. start[j+1]), 1 <= S <= 256,
 *   out[j][e] = ((sum_k s_k[e]) + S / 2) / S << shift      s_k[e] = min(word >> shift, 2^depth - 1)
 * per element e, in integers: ties round up, a sum of 256 16-bit samples is far inside 32 bits, and
 * the result is the same bits on every run (no atomics).  depth 8: uint8 elements (shift 0); depth
 * 9..16: uint16 words at even addresses, 0 <= shift <= 16 - depth, as in rrin_aux_plane.  A pointer
 * table, not base + stride, because the sources are views of a frame stack and outputs of several
 * item forwards: a source may be listed more than once, and may start at any element.  Each source
 * holds len elements; nothing outside [frame, frame + len) is read or written, and elements between
 * the frames of out are not written.  A group whose S read from start is outside 1..256 (after
 * clamping the offsets to [0, k]) is skipped: its frame is not written.
 *
 * access: the bytes one lane reads and writes at a time -- the element size, 4 or 16.  The caller,
 * who knows every address, passes the largest of them that divides every source address, out and
 * (g > 1) out_stride in bytes; the kernel takes the len % (access / element size) elements behind the
 * last whole run one at a time.  The source addresses live in device memory, so that they are
 * multiples of access is the caller's promise; everything else is checked here.
 * RRIN_E_ARG: a null pointer, a table not 8-byte or a start not 4-byte aligned, depth outside 8..16,
 * shift outside 0..16 - depth (depth 8: shift 0), access not one of the three, out (an odd word address
 * included) or out_stride not a multiple of access, g > 1 with out_stride < len, k < g or k > 256 g.
 * RRIN_E_SHAPE: g < 1, g > 65535, len < 1, more than 2^31 - 1 workgroups per frame.  Validated before
 * any launch. */
int rrin_mean_frames(const void* const* frames, int32_t k, const int32_t* start, int32_t g, void* out,
                     int64_t out_stride, int64_t len, int32_t depth, int32_t shift, int32_t access, void* stream);

/* ---- The linear-light exposure: weighted means through a transfer table ------------------------
 * History: added after ABI 25 without a new version number -- two new entry points and one new struct,
 * no existing struct or entry point changes, so RRIN_ABI_VERSION stays 25; a caller finds out whether
 * a build has them by looking the symbols up.
 *
 * rrin_amd/transfer.py and rrin_amd/exposure.py (mean_frames_linear) are the definition.  Both entries
 * take rrin_mean_frames' pointer table and CSR offsets, and beside them
 *   weights: a DEVICE int32 [k] parallel to frames, every weight in 1..65535 and the sum W of a group's
 *            weights at most 65535 (a group that breaks this is skipped like one with S outside 1..256);
 *   table:   a DEVICE int32 [2 * (maxval + 1)], 16-byte aligned, maxval = 2^depth - 1: lin[0 .. maxval],
 *            non-decreasing in [0, 2^30], then thr[0 .. maxval] with thr[c] = (lin[c-1] + lin[c] + 1) / 2
 *            for c >= 1 (thr[0] is not read).  The kernels copy it into LDS, 2 KiB at 8 bits and 32 KiB
 *            at 12, which is why depth > 12 with a table is refused.
 * With s_k = min(word >> shift, maxval) of source k and its weight w_k, in 64-bit integers (a sum stays
 * below 2^46), ties up, the same bits on every run:
 *   v = ((sum_k w_k * lin[s_k]) + W / 2) / W        enc(v) = #{c in 1..maxval : thr[c] <= v}
 *
 * rrin_mean_frames_lut: rrin_mean_frames' arguments, meaning and codes, per stored element
 *   out[j][e] = enc(v) << shift; with table == NULL at any depth 8..16 lin is the identity and enc is
 *   not applied: out[j][e] = ((sum_k w_k * s_k) + W / 2) / W << shift, which with every weight 1 is
 *   rrin_mean_frames bit for bit.  Further RRIN_E_ARG: weights null or not 4-byte aligned, a table with
 *   depth > 12 or not 16-byte aligned.  No len is too long for a grid: a workgroup walks several runs.
 *
 * rrin_mean_frames_yuv_lut: the sources and the g output frames are YUV frames of one geometry, a frame
 *   given by the address of its first luma sample (frames[] and out; output j at out + j * out_stride).
 *   rrin_yuv_planes counts in elements (bytes at depth 8, 16-bit words at depth 10 and 12): u_off / v_off
 *   from the first luma sample to the first U and V sample, the pitches, c_step, chroma, depth and shift
 *   of rrin_yuv420 / rrin_yuv420_16.  Per chroma block every source's pixels go to RGB code values by
 *   rrin_yuv_coef's way in, each R, G, B through the formula above (shift 0), and the block's RGB back
 *   by its way out: the RGB-table mean between the two conversions of the YUV forwards, bit for bit.
 *   RRIN_E_ARG: a null pointer (the table included), depth not 8, 10 or 12, shift not 0 or 16 - depth,
 *   c_step not 1 or 2, an unknown chroma, a coefficient out of range, a misaligned table, start, weights
 *   or frames, an odd out address at 16 bits, k < g or k > 256 g.  RRIN_E_SHAPE: g < 1 or > 65535, h0 /
 *   w0 not a size of the chroma format (even at 4:2:0, w0 even at 4:2:2), a pitch smaller than its row,
 *   planes that overlap (u_off inside the luma plane, v_off <= u_off, planar V inside U), output frames
 *   that overlap.  Both validate before any launch. */
typedef struct rrin_yuv_planes {
  int64_t u_off, v_off;        /* elements from a frame's first luma sample to its first U / V sample */
  int32_t y_pitch, c_pitch;    /* elements between rows */
  int32_t c_step, chroma;      /* elements between chroma samples of a row: 2 or 1; rrin_chroma */
  int32_t depth, shift;        /* 8 (bytes, shift 0), 10 or 12 (words; shift 0 or 16 - depth) */
} rrin_yuv_planes;
int rrin_mean_frames_lut(const void* const* frames, int32_t k, const int32_t* start, int32_t g, void* out,
                         int64_t out_stride, int64_t len, int32_t depth, int32_t shift, int32_t access,
                         const int32_t* weights, const int32_t* table, void* stream);
int rrin_mean_frames_yuv_lut(const void* const* frames, int32_t k, const int32_t* start, int32_t g, void* out,
                             int64_t out_stride, const rrin_yuv_planes* geom, const rrin_yuv_coef* coef, int32_t h0,
                             int32_t w0, const int32_t* weights, const int32_t* table, void* stream);

/* ---- Training path (autograd): NCHW fp32 kernels ------------------------- */
/* With autograd on (the reference trains through Net.forward, train.py:98, and
 * loss.backward(), train.py:144) rrin_amd.train wraps these in autograd
 * Functions.  All tensors are contiguous NCHW fp32.
 *   rrin_tconv3x3 FWD  : out = conv3x3(x, wt) + bias [, leaky]      (unet.py:29,38,59-63,78)
 *                 DGRAD: out = input gradient of that conv: the conv of
 *                        g' = g * leaky'(y) (leaky: y = the forward output) with
 *                        the flipped, transposed weights; x holds g [n][cout][h][w].
 *   rrin_tconv3x3_wgrad: gw = sum over images and pixels of g' (x) x shifted per
 *                        tap, gb = sum g'; deterministic split-K (work buffer of
 *                        rrin_tconv3x3_wgrad_work_floats floats).
 *   rrin_tpool2_*  : F.avg_pool2d(x, 2) (unet.py:46) and its backward; nc = n*c.
 *   rrin_tup2_*    : nn.Upsample(x2, bilinear) (unet.py:77) and its backward;
 *                    h, w = the low-resolution size.
 *   rrin_twarp_bwd : backward of warp (model.py:8-21; forward = rrin_warp_fwd):
 *                    gimg (scatter, summed exactly in 64-bit fixed point:
 *                    deterministic) and gflow; work >= rrin_twarp_bwd_work_bytes.
 * Codes, all returned before any HIP call: a null required pointer, a dimension < 1
 * (pool: h or w odd or < 2), leaky with a slope outside (0, 1] or without y, a mode other
 * than FWD / DGRAD, rrin_tpack_wino's bm not 32 or 64 or mode not 0 or 1: RRIN_E_ARG (the
 * two size queries return it as their negative value); rrin_tconv3x3 with h * w > 2^31 - 1:
 * RRIN_E_SHAPE; rrin_twarp_bwd with work_bytes too small: RRIN_E_WORKSPACE.  bias and gb
 * may be NULL. */
enum rrin_tconv_mode { RRIN_TCONV_FWD = 0, RRIN_TCONV_DGRAD = 1 };
typedef struct rrin_tconv_desc {
  int32_t n, cin, cout, h, w;
  int32_t mode;          /* rrin_tconv_mode                                    */
  int32_t leaky;         /* FWD: leaky output; DGRAD: g' = g * leaky'(y)       */
  float slope;           /* leaky slope, 0 < slope <= 1                        */
  const float* x;        /* FWD: input [n][cin][h][w]; DGRAD: g [n][cout][h][w] */
  const float* y;        /* DGRAD with leaky: forward output [n][cout][h][w]    */
  const float* wt;       /* OIHW [cout][cin][3][3]                              */
  const float* bias;     /* FWD: [cout] (nullable)                              */
  float* out;            /* FWD: [n][cout][h][w]; DGRAD: [n][cin][h][w]         */
} rrin_tconv_desc;
int rrin_tconv3x3(const rrin_tconv_desc* d, void* stream);

typedef struct rrin_twgrad_desc {
  int32_t n, cin, cout, h, w, leaky;
  float slope;
  int32_t pad_;
  const float* x;        /* forward input [n][cin][h][w]                        */
  const float* g;        /* output gradient [n][cout][h][w]                     */
  const float* y;        /* leaky: forward output [n][cout][h][w]               */
  float* gw;             /* [cout][cin][3][3]                                   */
  float* gb;             /* [cout] (nullable)                                   */
  float* work;           /* rrin_tconv3x3_wgrad_work_floats(...) floats         */
} rrin_twgrad_desc;
int64_t rrin_tconv3x3_wgrad_work_floats(int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w);
int rrin_tconv3x3_wgrad(const rrin_twgrad_desc* d, void* stream);

int rrin_tpool2_fwd(const float* x, float* y, int32_t nc, int32_t h, int32_t w, void* stream);
int rrin_tpool2_bwd(const float* gy, float* gx, int32_t nc, int32_t h, int32_t w, void* stream);
int rrin_tup2_fwd(const float* x, float* y, int32_t nc, int32_t h, int32_t w, void* stream);
int rrin_tup2_bwd(const float* gy, float* gx, int32_t nc, int32_t h, int32_t w, void* stream);
int64_t rrin_twarp_bwd_work_bytes(int32_t n, int32_t c, int32_t h, int32_t w);
/* ABI 12: the Winograd packing of rrin_pack_conv3x3_wino_bm computed on the device (the
 * training path repacks every step), bitwise the host packing.  mode 0: the conv of OIHW
 * w [cout][cin][3][3] (rows cout, channels cin); mode 1: its data-gradient conv, w
 * transposed and flipped (rows cin, channels cout).  wpack: rrin_pack_conv3x3_wino_bm_floats
 * (rows, channels, bm) floats. */
int rrin_tpack_wino(const float* w, int32_t cout, int32_t cin, int32_t bm, int32_t mode, float* wpack, void* stream);
int rrin_twarp_bwd(const float* img, const float* flow, const float* gout, float* gimg, float* gflow,
                   void* work, int64_t work_bytes, int32_t n, int32_t c, int32_t h, int32_t w, void* stream);

/* ---- Misc ---------------------------------------------------------------- */
int rrin_abi_version(void);
const char* rrin_strerror(int code);

#ifdef __cplusplus
}
#endif
#endif /* RRIN_HIP_H */
