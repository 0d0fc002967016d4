// The record formats as the non-conv kernels of the record path (glue_h8.hip) see them: RecH8<1>
// (F16), RecH8<2> (F16X3: hi and lo' planes) and RecR32 (exact fp32), layouts in h8.hpp.  A format
// is a struct of device inline functions, chosen at compile time; each kernel there is written
// once against them.  What a format says:
//   kChans                channels of one 16-B record
//   kRecs8, fetch8 / decode8 / load8   the records that hold 8 consecutive channels of one
//                         position (from a record index of the first), raw and as 8 floats
//   load_rec / store_rec  one whole record as kChans floats
//   load_elem / store_elem one channel of one pixel
//   round_stored          a value as the format stores it
//   kFlag, check_range    whether stores can leave the range (the fp16 range flag)
//   Px                    the 16 channels of one Net-buffer (g16) pixel: fetch, then read c[] and
//                         store channel ranges
#pragma once
#include "h8.hpp"

namespace rrin {

// One record tensor: the plane pointers at the view's first group, strides in records.
struct RecView {
  uint4* hi;
  uint4* lo;  // RecH8<2> only
  int64_t img, gp;
  int wp;
  __device__ int64_t rec(int i, int g, int y, int x) const {
    return i * img + g * gp + (int64_t)(y + 1) * wp + x + kH8PadLeft;
  }
};

template <int PLANES>
struct RecH8 {
  static constexpr int kChans = 8, kRecs8 = PLANES;
  static constexpr bool kFlag = true;

  static __device__ void fetch8(const RecView& v, int64_t rec, uint4* raw) {
    raw[0] = v.hi[rec];
    if constexpr (PLANES == 2) raw[1] = v.lo[rec];
  }
  static __device__ void decode8(const uint4* raw, float* f) {
    const half8 h = __builtin_bit_cast(half8, raw[0]);
    half8 l = {};
    if constexpr (PLANES == 2) l = __builtin_bit_cast(half8, raw[PLANES - 1]);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = PLANES == 2 ? join(h[e], l[e]) : (float)h[e];
  }
  static __device__ void load8(const RecView& v, int64_t rec, float* f) {
    uint4 raw[PLANES];
    fetch8(v, rec, raw);
    decode8(raw, f);
  }
  static __device__ void load_rec(const RecView& v, int64_t rec, float* f) { load8(v, rec, f); }
  static __device__ void store_rec(const RecView& v, int64_t rec, const float* f) { put<0, 8>(v, rec, f); }

  static __device__ float load_elem(const RecView& v, int img, int ch, int y, int x) {
    const int64_t k = h8_half_index(v.img, v.gp, v.wp, img, ch, y, x);
    const _Float16 h = reinterpret_cast<const _Float16*>(v.hi)[k];
    return PLANES == 2 ? join(h, reinterpret_cast<const _Float16*>(v.lo)[k]) : (float)h;
  }
  static __device__ void store_elem(const RecView& v, int img, int ch, int y, int x, float f) {
    const int64_t k = h8_half_index(v.img, v.gp, v.wp, img, ch, y, x);
    const _Float16 h = (_Float16)f;
    reinterpret_cast<_Float16*>(v.hi)[k] = h;
    if constexpr (PLANES == 2) reinterpret_cast<_Float16*>(v.lo)[k] = lo_of(f, h);
  }

  static __device__ float round_stored(float f) {
    const _Float16 h = (_Float16)f;
    return PLANES == 2 ? join(h, lo_of(f, h)) : (float)h;
  }
  static __device__ void check_range(int* status, float f) {
    if (status && !(fabsf(f) <= kF16Max)) *status = 1;
  }

  // halves [E0, E0 + N) of one record: one 16 / 8 / 4-B store per plane for N = 8 / 4 / 2, else
  // one 2-B store per half
  template <int E0, int N>
  static __device__ void put(const RecView& v, int64_t rec, const float* f) {
    _Float16 hv[N], lv[N];
#pragma unroll
    for (int e = 0; e < N; ++e) {
      hv[e] = (_Float16)f[e];
      lv[e] = lo_of(f[e], hv[e]);
    }
    _Float16* ph = reinterpret_cast<_Float16*>(v.hi + rec) + E0;
    _Float16* pl = reinterpret_cast<_Float16*>(v.lo + rec) + E0;
    if constexpr (N == 8) {
      *reinterpret_cast<uint4*>(ph) = __builtin_bit_cast(uint4, hv);
      if constexpr (PLANES == 2) *reinterpret_cast<uint4*>(pl) = __builtin_bit_cast(uint4, lv);
    } else if constexpr (N == 4) {
      *reinterpret_cast<uint2*>(ph) = __builtin_bit_cast(uint2, hv);
      if constexpr (PLANES == 2) *reinterpret_cast<uint2*>(pl) = __builtin_bit_cast(uint2, lv);
    } else if constexpr (N == 2) {
      *reinterpret_cast<uint32_t*>(ph) = __builtin_bit_cast(uint32_t, hv);
      if constexpr (PLANES == 2) *reinterpret_cast<uint32_t*>(pl) = __builtin_bit_cast(uint32_t, lv);
    } else {
#pragma unroll
      for (int e = 0; e < N; ++e) {
        ph[e] = hv[e];
        if constexpr (PLANES == 2) pl[e] = lv[e];
      }
    }
  }

  struct Px {
    const RecView& v;
    int64_t rec0;  // the pixel's record of group 0
    int* status;   // range flag of the stores (nullable)
    float c[16];
    // before reading channels [RA, RB) of c: their records; stores are partial, so a later
    // store<WA, WB> needs nothing
    template <int RA, int RB, int WA, int WB>
    __device__ void fetch() {
#pragma unroll
      for (int k = 0; k < 2; ++k)
        if (RA < 8 * k + 8 && RB > 8 * k) load8(v, rec0 + k * v.gp, c + 8 * k);
    }
    // channels [A, B) = f[0 .. B - A), record by record, range-checked
    template <int A, int B>
    __device__ void store(const float* f) {
#pragma unroll
      for (int e = 0; e < B - A; ++e) check_range(status, f[e]);
      constexpr int A1 = A < 8 && B > 8 ? 8 : B;  // [A, A1) in A's record, [A1, B) in the next
      put<A % 8, A1 - A>(v, rec0 + (A / 8) * v.gp, f);
      if constexpr (A1 < B) put<0, B - A1>(v, rec0 + v.gp, f + (A1 - A));
    }
  };
};

struct RecR32 {
  static constexpr int kChans = 4, kRecs8 = 2;
  static constexpr bool kFlag = false;

  static __device__ void fetch8(const RecView& v, int64_t rec, uint4* raw) {
    raw[0] = v.hi[rec];
    raw[1] = v.hi[rec + v.gp];
  }
  static __device__ void decode8(const uint4* raw, float* f) {
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = __builtin_bit_cast(floatx4, raw[e >> 2])[e & 3];
  }
  static __device__ void load8(const RecView& v, int64_t rec, float* f) {
    uint4 raw[2];
    fetch8(v, rec, raw);
    decode8(raw, f);
  }
  static __device__ void load_rec(const RecView& v, int64_t rec, float* f) {
    const floatx4 q = __builtin_bit_cast(floatx4, v.hi[rec]);
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = q[e];
  }
  static __device__ void store_rec(const RecView& v, int64_t rec, const float* f) {
    v.hi[rec] = f4rec(f[0], f[1], f[2], f[3]);
  }

  static __device__ float load_elem(const RecView& v, int img, int ch, int y, int x) {
    return reinterpret_cast<const float*>(v.hi)[r32_elem_index(v.img, v.gp, v.wp, img, ch, y, x)];
  }
  static __device__ void store_elem(const RecView& v, int img, int ch, int y, int x, float f) {
    reinterpret_cast<float*>(v.hi)[r32_elem_index(v.img, v.gp, v.wp, img, ch, y, x)] = f;
  }

  static __device__ float round_stored(float f) { return f; }
  static __device__ void check_range(int*, float) {}

  struct Px {
    const RecView& v;
    int64_t rec0;
    int* status;  // unused: no range flag
    float c[16];
    // before reading channels [RA, RB) of c and storing [WA, WB): the records of [RA, RB) and
    // those [WA, WB) covers only partly -- every store is a whole record, rebuilt from c
    template <int RA, int RB, int WA, int WB>
    __device__ void fetch() {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool rd = RA < 4 * k + 4 && RB > 4 * k;
        const bool part = WA < 4 * k + 4 && WB > 4 * k && !(WA <= 4 * k && WB >= 4 * k + 4);
        if (rd || part) load_rec(v, rec0 + k * v.gp, c + 4 * k);
      }
    }
    template <int A, int B>
    __device__ void store(const float* f) {
#pragma unroll
      for (int e = A; e < B; ++e) c[e] = f[e - A];
#pragma unroll
      for (int k = A / 4; k <= (B - 1) / 4; ++k) store_rec(v, rec0 + k * v.gp, c + 4 * k);
    }
  };
};

// ---- host side ---------------------------------------------------------------------
// fn(F{}) with the record format F of a record precision (rec_prec(prec) checked by the caller)
template <class Fn>
static int with_format(int prec, Fn&& fn) {
  if (prec == RRIN_PREC_F32R) return fn(RecR32{});
  return planes_of(prec) == 2 ? fn(RecH8<2>{}) : fn(RecH8<1>{});
}

static inline RecView rec_view(const rrin_h8& v) {
  const int64_t off = (int64_t)v.g_off * v.g.plane;
  return RecView{static_cast<uint4*>(v.hi) + off, v.lo ? static_cast<uint4*>(v.lo) + off : nullptr, v.img_stride,
                 v.g.plane, v.g.wp};
}

}  // namespace rrin
