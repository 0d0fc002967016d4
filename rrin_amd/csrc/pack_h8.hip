// Host-only side of the record convs: weight packing for the direct-form tiles (conv_h8.hip) at
// fp16 / split-fp16 (rrin_pack_conv3x3_h8) and fp32 records (rrin_pack_conv3x3_r32), the
// phase-combined weights of the sub-pixel up conv (rrin_subpixel_weights) and the size of its
// ring (rrin_ring_pixels); and the packer of the planar fp32 convs (rrin_pack_conv3x3, with the
// padded bias size every packer shares, rrin_pack_bias_floats).  No device code.
#include <math.h>
#include <string.h>

#include "h8.hpp"

using namespace rrin;

// fp32 -> fp16 bits, round to nearest even (host packing).
static uint16_t f2h_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  const uint32_t au = u & 0x7FFFFFFFu;
  if (au >= 0x7F800000u) return (uint16_t)(sign | (au > 0x7F800000u ? 0x7E00u : 0x7C00u));
  if (au >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);  // rounds to >= 65520 -> inf
  if (au < 0x38800000u) {                                     // subnormal / zero in fp16
    const float af = fabsf(f);
    const uint32_t m = (uint32_t)lrintf(af * 16777216.0f);     // units of 2^-24, RNE
    return (uint16_t)(sign | m);
  }
  const uint32_t e = ((au >> 23) - 112u) << 10;  // rebias 127 -> 15
  uint32_t m = (au >> 13) & 0x3FFu;
  const uint32_t rest = au & 0x1FFFu;
  uint32_t h = e | m;
  if (rest > 0x1000u || (rest == 0x1000u && (m & 1u))) h += 1u;
  return (uint16_t)(sign | h);
}

static float h2f(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  const uint32_t e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
  float f;
  if (e == 0) {
    f = ldexpf((float)m, -24);
  } else if (e == 31) {
    uint32_t u = sign | 0x7F800000u | (m << 13);
    memcpy(&f, &u, 4);
    return f;
  } else {
    uint32_t u = ((e + 112u) << 23) | (m << 13);
    memcpy(&f, &u, 4);
  }
  return sign ? -f : f;
}

extern "C" int64_t rrin_pack_conv3x3_h8_halves(int32_t cout, int32_t cin, int32_t bm) {
  if (cout < 1 || cin < 1 || bm < 32 || bm % 32) return RRIN_E_ARG;
  const int64_t cob = (cout + bm - 1) / bm, nch = (cin + 15) / 16;
  return cob * nch * 9 * 2 * bm * 8;
}

extern "C" int rrin_pack_conv3x3_h8(const float* w, const float* b, int32_t cout, int32_t cin, int32_t bm,
                                    const int32_t* perm, int32_t prec, uint16_t* whi, uint16_t* wlo, float* bpack,
                                    float* inv_wscale) {
  if (!w || !b || !whi || !bpack || !inv_wscale || cout < 1 || cin < 1 || bm < 32 || bm % 32) return RRIN_E_ARG;
  if (prec != RRIN_PREC_F16X3 && prec != RRIN_PREC_F16) return RRIN_E_ARG;
  if (prec == RRIN_PREC_F16X3 && !wlo) return RRIN_E_ARG;
  if (perm)
    for (int c = 0; c < cin; ++c)
      if (perm[c] < 0 || perm[c] >= cin) return RRIN_E_ARG;
  float mx = 0.f;
  const int64_t nw = (int64_t)cout * cin * 9;
  for (int64_t i = 0; i < nw; ++i) mx = fmaxf(mx, fabsf(w[i]));
  if (!(mx < INFINITY)) return RRIN_E_ARG;
  int s = 0;
  if (mx > 0.f) {
    int e;
    frexpf(mx, &e);  // mx in [2^(e-1), 2^e)
    s = 13 - e;      // scaled max in [2^12, 2^13)
  }
  const float scale = ldexpf(1.0f, s);
  *inv_wscale = ldexpf(1.0f, -s);
  const int cob_n = (cout + bm - 1) / bm, nch = (cin + 15) / 16;
  int64_t o = 0;
  for (int cob = 0; cob < cob_n; ++cob)
    for (int c = 0; c < nch; ++c)
      for (int tap = 0; tap < 9; ++tap)
        for (int hh = 0; hh < 2; ++hh)
          for (int col = 0; col < bm; ++col)
            for (int e = 0; e < 8; ++e) {
              const int co = cob * bm + col, ch = c * 16 + hh * 8 + e;
              float v = 0.f;
              if (co < cout && ch < cin) v = w[((int64_t)co * cin + (perm ? perm[ch] : ch)) * 9 + tap] * scale;
              const uint16_t hbits = f2h_rne(v);
              whi[o] = hbits;
              if (prec == RRIN_PREC_F16X3) wlo[o] = f2h_rne((v - h2f(hbits)) * 2048.0f);
              ++o;
            }
  for (int co = 0; co < cob_n * bm; ++co) bpack[co] = co < cout ? b[co] : 0.f;
  return 0;
}

extern "C" int64_t rrin_pack_conv3x3_r32_floats(int32_t cout, int32_t cin, int32_t bm) {
  if (cout < 1 || cin < 1 || bm < 32 || bm % 32) return RRIN_E_ARG;
  const int64_t cob = (cout + bm - 1) / bm, nch = (cin + 7) / 8;
  return cob * nch * 9 * 2 * bm * 4;
}

extern "C" int rrin_pack_conv3x3_r32(const float* w, const float* b, int32_t cout, int32_t cin, int32_t bm,
                                     const int32_t* perm, float* wpack, float* bpack) {
  if (!w || !b || !wpack || !bpack || cout < 1 || cin < 1 || bm < 32 || bm % 32) return RRIN_E_ARG;
  if (perm)
    for (int c = 0; c < cin; ++c)
      if (perm[c] < 0 || perm[c] >= cin) return RRIN_E_ARG;
  const int cob_n = (cout + bm - 1) / bm, nch = (cin + 7) / 8;
  int64_t o = 0;
  for (int cob = 0; cob < cob_n; ++cob)
    for (int c = 0; c < nch; ++c)
      for (int tap = 0; tap < 9; ++tap)
        for (int hh = 0; hh < 2; ++hh)
          for (int col = 0; col < bm; ++col)
            for (int e = 0; e < 4; ++e) {
              const int co = cob * bm + col, ch = c * 8 + hh * 4 + e;
              wpack[o++] = (co < cout && ch < cin) ? w[((int64_t)co * cin + (perm ? perm[ch] : ch)) * 9 + tap] : 0.f;
            }
  for (int co = 0; co < cob_n * bm; ++co) bpack[co] = co < cout ? b[co] : 0.f;
  return 0;
}

// ---- the planar fp32 convs (conv_mfma.hip) -----------------------------------------
// wpack[cob][chunk][ci8][tap][bm]: the slab a block stages per K chunk is
// contiguous; zero rows/cols pad cin to 8 and cout to bm.
extern "C" int64_t rrin_pack_conv3x3_floats(int32_t cout, int32_t cin, int32_t bm) {
  if (cout < 1 || cin < 1 || bm < 32 || bm % 32) return RRIN_E_ARG;
  const int64_t cob = (cout + bm - 1) / bm, nch = (cin + 7) / 8;
  return cob * nch * 8 * 9 * bm;
}

extern "C" int64_t rrin_pack_bias_floats(int32_t cout, int32_t bm) {
  if (cout < 1 || bm < 32 || bm % 32) return RRIN_E_ARG;
  return (int64_t)((cout + bm - 1) / bm) * bm;
}

extern "C" int rrin_pack_conv3x3(const float* w, const float* b, int32_t cout, int32_t cin, int32_t bm,
                                 const int32_t* perm, float* wpack, float* bpack) {
  if (!w || !b || !wpack || !bpack || cout < 1 || cin < 1 || bm < 32 || bm % 32) return RRIN_E_ARG;
  if (perm)
    for (int c = 0; c < cin; ++c)
      if (perm[c] < 0 || perm[c] >= cin) return RRIN_E_ARG;
  const int cob_n = (cout + bm - 1) / bm, nch = (cin + 7) / 8;
  int64_t o = 0;
  for (int cob = 0; cob < cob_n; ++cob)
    for (int c = 0; c < nch; ++c)
      for (int ci = 0; ci < 8; ++ci)
        for (int tap = 0; tap < 9; ++tap)
          for (int col = 0; col < bm; ++col) {
            const int co = cob * bm + col, ch = c * 8 + ci;
            float v = 0.f;
            if (co < cout && ch < cin) {
              const int src_ch = perm ? perm[ch] : ch;
              v = w[((int64_t)co * cin + src_ch) * 9 + tap];
            }
            wpack[o++] = v;
          }
  for (int co = 0; co < cob_n * bm; ++co) bpack[co] = co < cout ? b[co] : 0.f;
  return 0;
}

extern "C" int64_t rrin_ring_pixels(int32_t h, int32_t w) {
  if (h < 1 || w < 1) return RRIN_E_ARG;
  return ring_pixels(h, w);
}

// Phase-combined weights of conv3x3 o upsample_x2 (see rrin_hip.h).  kR[p][a][k]:
// coefficient of low-res row m+a-1 in upsampled row 2m+p+k-1 (align_corners=False).
extern "C" int rrin_subpixel_weights(const float* w, const float* b, int32_t cout, int32_t cin, float* wsub,
                                     float* bsub) {
  if (!w || !b || !wsub || !bsub || cout < 8 || (cout & 7) || cin < 1) return RRIN_E_ARG;
  static const double kR[2][3][3] = {{{0.75, 0.25, 0.0}, {0.25, 0.75, 0.75}, {0.0, 0.0, 0.25}},
                                     {{0.25, 0.0, 0.0}, {0.75, 0.75, 0.25}, {0.0, 0.25, 0.75}}};
  for (int co = 0; co < cout; ++co)
    for (int ph = 0; ph < 4; ++ph) {
      const int py = ph >> 1, px = ph & 1;
      const int64_t row = (int64_t)(co >> 3) * 32 + ph * 8 + (co & 7);
      bsub[row] = b[co];
      for (int ci = 0; ci < cin; ++ci) {
        const float* src = w + ((int64_t)co * cin + ci) * 9;
        float* dst = wsub + (row * cin + ci) * 9;
        for (int ay = 0; ay < 3; ++ay)
          for (int ax = 0; ax < 3; ++ax) {
            double acc = 0.0;
            for (int ky = 0; ky < 3; ++ky)
              for (int kx = 0; kx < 3; ++kx) acc += kR[py][ay][ky] * kR[px][ax][kx] * (double)src[ky * 3 + kx];
            dst[ay * 3 + ax] = (float)acc;
          }
      }
    }
  return 0;
}
