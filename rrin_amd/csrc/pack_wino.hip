// Host-only Winograd weight packing: U = G g G^T per (co, ci, transform point), in double, rounded
// once, in the record order each tile loads -- F(2x2,3x3) for kinds 1-7 (conv_wino.hip, conv_winoq.hip,
// conv_winoc.hip), F(4,3) x F(2,3) for kind 14 (conv_winoc42.hip), F(2x2,3x3) scaled to fp16 for
// kind 6 at fp16 (conv_winoh.hip).  No device code.
#include <math.h>

#include "common.hpp"

using namespace rrin;

extern "C" int64_t rrin_pack_conv3x3_wino_floats(int32_t cout, int32_t cin) {
  return rrin_pack_conv3x3_wino_bm_floats(cout, cin, 32);
}

extern "C" int64_t rrin_pack_conv3x3_wino_bm_floats(int32_t cout, int32_t cin, int32_t bm) {
  if (cout < 1 || cin < 1 || (bm != 32 && bm != 64)) return RRIN_E_ARG;
  const int64_t cob = (cout + bm - 1) / bm, nch = (cin + 7) / 8;
  return cob * nch * 16 * 2 * bm * 4;
}

extern "C" int rrin_pack_conv3x3_wino(const float* w, const float* b, int32_t cout, int32_t cin, const int32_t* perm,
                                      float* wpack, float* bpack) {
  return rrin_pack_conv3x3_wino_bm(w, b, cout, cin, 32, perm, wpack, bpack);
}

// [co block of bm][8-channel chunk][transform point xi][record half][bm co][4 channels]
extern "C" int rrin_pack_conv3x3_wino_bm(const float* w, const float* b, int32_t cout, int32_t cin, int32_t bm,
                                         const int32_t* perm, float* wpack, float* bpack) {
  if (!w || !b || !wpack || !bpack || cout < 1 || cin < 1 || (bm != 32 && bm != 64)) return RRIN_E_ARG;
  if (perm)
    for (int c = 0; c < cin; ++c)
      if (perm[c] < 0 || perm[c] >= cin) return RRIN_E_ARG;
  static const double G[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
  const int cob_n = (cout + bm - 1) / bm, nch = (cin + 7) / 8;
  int64_t o = 0;
  for (int cob = 0; cob < cob_n; ++cob)
    for (int c = 0; c < nch; ++c)
      for (int xi = 0; xi < 16; ++xi)
        for (int hh = 0; hh < 2; ++hh)
          for (int col = 0; col < bm; ++col)
            for (int e = 0; e < 4; ++e) {
              const int co = cob * bm + col, ch = c * 8 + hh * 4 + e;
              double u = 0.0;
              if (co < cout && ch < cin) {
                const float* g = w + ((int64_t)co * cin + (perm ? perm[ch] : ch)) * 9;
                for (int ky = 0; ky < 3; ++ky)
                  for (int kx = 0; kx < 3; ++kx) u += G[xi >> 2][ky] * G[xi & 3][kx] * (double)g[ky * 3 + kx];
              }
              wpack[o++] = (float)u;
            }
  for (int co = 0; co < cob_n * bm; ++co) bpack[co] = co < cout ? b[co] : 0.f;
  return 0;
}

// Kind-14 packing: [co block of 32][8-channel chunk][point xi = 6 eta + xi_x][record half][32 co][4 ch],
// U(eta, xi_x) = sum G2[eta][ky] G4[xi_x][kx] g[ky][kx] in double, rounded once to fp32
extern "C" int64_t rrin_pack_conv3x3_wino42_floats(int32_t cout, int32_t cin) {
  if (cout < 1 || cin < 1) return RRIN_E_ARG;
  return (int64_t)((cout + 31) / 32) * ((cin + 7) / 8) * 24 * 2 * 32 * 4;
}

extern "C" int rrin_pack_conv3x3_wino42(const float* w, const float* b, int32_t cout, int32_t cin, const int32_t* perm,
                                        float* wpack, float* bpack) {
  if (!w || !b || !wpack || !bpack || cout < 1 || cin < 1) return RRIN_E_ARG;
  if (perm)
    for (int c = 0; c < cin; ++c)
      if (perm[c] < 0 || perm[c] >= cin) return RRIN_E_ARG;
  static const double G2[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
  static const double G4[6][3] = {{0.25, 0.0, 0.0},
                                  {-1.0 / 6, -1.0 / 6, -1.0 / 6},
                                  {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                  {1.0 / 24, 1.0 / 12, 1.0 / 6},
                                  {1.0 / 24, -1.0 / 12, 1.0 / 6},
                                  {0.0, 0.0, 1.0}};
  const int cob_n = (cout + 31) / 32, nch = (cin + 7) / 8;
  int64_t o = 0;
  for (int cob = 0; cob < cob_n; ++cob)
    for (int c = 0; c < nch; ++c)
      for (int xi = 0; xi < 24; ++xi)
        for (int hh = 0; hh < 2; ++hh)
          for (int col = 0; col < 32; ++col)
            for (int e = 0; e < 4; ++e) {
              const int co = cob * 32 + col, ch = c * 8 + hh * 4 + e;
              double u = 0.0;
              if (co < cout && ch < cin) {
                const float* g = w + ((int64_t)co * cin + (perm ? perm[ch] : ch)) * 9;
                for (int ky = 0; ky < 3; ++ky)
                  for (int kx = 0; kx < 3; ++kx) u += G2[xi / 6][ky] * G4[xi % 6][kx] * (double)g[ky * 3 + kx];
              }
              wpack[o++] = (float)u;
            }
  for (int co = 0; co < cob_n * 32; ++co) bpack[co] = co < cout ? b[co] : 0.f;
  return 0;
}

// ---- packing: [co block of bm][16-channel chunk][point xi][record half][bm co][8 halves] of
// U = G g G^T (double) x 2^s, rounded once to fp16; s puts max |U| in [2^12, 2^13) as the
// direct fp16 packing does for max |g| (rrin_pack_conv3x3_h8), *inv_wscale = 2^-s
extern "C" int64_t rrin_pack_conv3x3_wino_h8_halves(int32_t cout, int32_t cin, int32_t bm) {
  if (cout < 1 || cin < 1 || bm != 64) return RRIN_E_ARG;
  const int64_t cob = (cout + bm - 1) / bm, nch = (cin + 15) / 16;
  return cob * nch * 16 * 2 * bm * 8;
}

extern "C" int rrin_pack_conv3x3_wino_h8(const float* w, const float* b, int32_t cout, int32_t cin, int32_t bm,
                                         const int32_t* perm, uint16_t* whi, float* bpack, float* inv_wscale) {
  if (!w || !b || !whi || !bpack || !inv_wscale || cout < 1 || cin < 1 || bm != 64) return RRIN_E_ARG;
  if (perm)
    for (int c = 0; c < cin; ++c)
      if (perm[c] < 0 || perm[c] >= cin) return RRIN_E_ARG;
  static const double G[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
  const int cob_n = (cout + bm - 1) / bm, nch = (cin + 15) / 16;
  auto u_of = [&](int co, int ch, int xi) {
    const float* g = w + ((int64_t)co * cin + (perm ? perm[ch] : ch)) * 9;
    double u = 0.0;
    for (int ky = 0; ky < 3; ++ky)
      for (int kx = 0; kx < 3; ++kx) u += G[xi >> 2][ky] * G[xi & 3][kx] * (double)g[ky * 3 + kx];
    return u;
  };
  double mx = 0.0;
  for (int co = 0; co < cout; ++co)
    for (int ch = 0; ch < cin; ++ch)
      for (int xi = 0; xi < 16; ++xi) mx = fmax(mx, fabs(u_of(co, ch, xi)));
  if (!(mx < INFINITY)) return RRIN_E_ARG;
  int s = 0;
  if (mx > 0.0) {
    int e;
    frexp(mx, &e);  // mx in [2^(e-1), 2^e)
    s = 13 - e;     // scaled max in [2^12, 2^13)
  }
  const double scale = ldexp(1.0, s);
  *inv_wscale = ldexpf(1.0f, -s);
  int64_t o = 0;
  for (int cob = 0; cob < cob_n; ++cob)
    for (int c = 0; c < nch; ++c)
      for (int xi = 0; xi < 16; ++xi)
        for (int hh = 0; hh < 2; ++hh)
          for (int col = 0; col < bm; ++col)
            for (int e = 0; e < 8; ++e) {
              const int co = cob * bm + col, ch = c * 16 + hh * 8 + e;
              const double u = (co < cout && ch < cin) ? u_of(co, ch, xi) * scale : 0.0;
              whi[o++] = __builtin_bit_cast(uint16_t, (_Float16)u);
            }
  for (int co = 0; co < cob_n * bm; ++co) bpack[co] = co < cout ? b[co] : 0.f;
  return 0;
}
