"""CPU side of the exact-value tests of the record convs (tests/test_gpu_h8_exact.py): data on
which every summation order gives the same bits, int64 references, the representability checks,
and decoders of the packed weight blobs.  No GPU call; the pack entry points are host code.

Data rules ("Exact values"):
  * x and w are +-1 / +-2 (never 0), the bias +-1..3, the leaky slope 1/4: every product, every
    partial sum in any order and the stored result are small dyadic numbers;
  * split-fp16 adds +-2^-12 to a quarter of the inputs and weights: it lands wholly in the lo
    half (hi stays the integer), and the reference is the exact sum hx*hw + hx*lw + lx*hw -- the
    lo*lo products are dropped, as the kernel drops them;
  * kind 14 (F(4,3) x F(2,3)) takes the weights times 48: G has 1/6, 1/12, 1/24, so U is integer.
References are int64 in units of a power of two (``Ref.units`` / ``Ref.scale``)."""
import functools
from dataclasses import dataclass

import numpy as np
import torch

P24 = 2 ** 24
LO = 4096            # the split-fp16 offsets are multiples of 1 / LO = 2^-12
SLOPE = 0.25


# ---- data --------------------------------------------------------------------------------------
def pm(shape, mags, seed):
    """int64 of the given magnitudes with random signs: never 0."""
    r = np.random.default_rng(seed)
    a = r.choice(np.asarray(mags, np.int64), size=shape) * r.choice(np.asarray([-1, 1], np.int64), size=shape)
    a.setflags(write=False)
    return a


def lo_units(shape, seed):
    """int64 in {-1, 0, 1}: the split-fp16 offset in units of 2^-12, non-zero for one element in four."""
    r = np.random.default_rng(seed)
    a = r.choice(np.asarray([-1, 1], np.int64), size=shape) * (r.integers(0, 4, size=shape) == 0)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def int_case(n, cin, cout, h, w, mags=(1, 2), tag=0):
    """(x [n, cin, h, w], wt [cout, cin, 3, 3], b [cout], ox, ow): integers and the lo offsets."""
    key = [n, cin, cout, h, w, len(mags), tag]
    return (pm((n, cin, h, w), mags, [1] + key), pm((cout, cin, 3, 3), mags, [2] + key), pm((cout,), (1, 2, 3), [3] + key),
            lo_units((n, cin, h, w), [4] + key), lo_units((cout, cin, 3, 3), [5] + key))


# ---- int64 references --------------------------------------------------------------------------
def conv_int(x, w, taps=None):
    """3x3 correlation, zero padding 1, int64; taps: the (ky, kx) to sum (default all nine)."""
    n, c, h, wd = x.shape
    xp = np.zeros((n, c, h + 2, wd + 2), np.int64)
    xp[:, :, 1:-1, 1:-1] = x
    y = np.zeros((n, w.shape[0], h, wd), np.int64)
    # the products summed in float64 (BLAS) where every partial sum is an integer below 2^53 -- the
    # same integers as the int64 product, many times faster at the launch-path shapes
    f64 = 9 * c * int(np.abs(x).max(initial=0)) * int(np.abs(w).max(initial=0)) < 2 ** 52
    dt = np.float64 if f64 else np.int64
    for ky in range(3):
        for kx in range(3):
            if taps is not None and (ky, kx) not in taps:
                continue
            cols = xp[:, :, ky:ky + h, kx:kx + wd].transpose(1, 0, 2, 3).reshape(c, -1).astype(dt)
            part = w[:, :, ky, kx].astype(dt) @ cols
            y += part.astype(np.int64).reshape(-1, n, h, wd).transpose(1, 0, 2, 3)
    return y


def up2_int(x):
    """Bilinear x2 (align_corners=False) of int64 x in units of 1/16: 3/4 and 1/4 along each axis."""
    def axis(a, ax):
        a = np.moveaxis(a, ax, -1)
        prev = np.concatenate([a[..., :1], a[..., :-1]], -1)
        nxt = np.concatenate([a[..., 1:], a[..., -1:]], -1)
        out = np.empty(a.shape[:-1] + (2 * a.shape[-1],), np.int64)
        out[..., 0::2] = 3 * a + prev
        out[..., 1::2] = 3 * a + nxt
        return np.moveaxis(out, -1, ax)
    return axis(axis(x.astype(np.int64), 2), 3)


@dataclass
class Ref:
    """units / scale is the exact value; scale a power of two."""
    units: np.ndarray
    scale: int

    def f64(self):
        assert int(np.abs(self.units).max()) < 2 ** 53
        return self.units.astype(np.float64) / self.scale

    def times(self, k):
        return Ref(self.units * k, self.scale * k)


def leaky(r):
    """leaky_relu, slope 1/4."""
    return Ref(np.where(r.units > 0, 4 * r.units, r.units), 4 * r.scale)


def pool(r):
    """avg_pool2d(2)."""
    u = r.units
    return Ref(u[:, :, 0::2, 0::2] + u[:, :, 0::2, 1::2] + u[:, :, 1::2, 0::2] + u[:, :, 1::2, 1::2], 4 * r.scale)


def pre_int(x, wt, b, wmul=1):
    """wmul (conv(x, wt) + b), integers: the bias is scaled with the weights, so exact zeros stay."""
    return Ref(wmul * (conv_int(x, wt) + b[None, :, None, None]), 1)


def pre_split(x, wt, b, ox, ow, zero_lo=False):
    """Split-fp16 on x + ox 2^-12, wt + ow 2^-12: hx*hw + hx*lw + lx*hw + b (no lo*lo), units 2^-12."""
    u = LO * (conv_int(x, wt) + b[None, :, None, None])
    if not zero_lo:
        u = u + conv_int(x, ow) + conv_int(ox, wt)
    return Ref(u, LO)


def pre_sub(x, wt, b, wmul=1):
    """wmul (conv(upsample_x2(x), wt) + b), units 1/16."""
    return Ref(wmul * (conv_int(up2_int(x), wt) + 16 * b[None, :, None, None]), 16)


# ---- mutations of a reference (tests/test_exact_ref.py: each must break the equality) -----------
def drop_one_tap(r, x, wt, wmul=1, at=(0, 1, 2, 3), ch=1, tap=(0, 2)):
    """r without the product of input channel ch under tap at output (image, co, y, x) = at."""
    i, co, y, xx = at
    ky, kx = tap
    yy, xq = y + ky - 1, xx + kx - 1
    assert 0 <= yy < x.shape[2] and 0 <= xq < x.shape[3]
    u = r.units.copy()
    u[i, co, y, xx] -= r.scale * wmul * int(wt[co, ch, ky, kx]) * int(x[i, ch, yy, xq])
    return Ref(u, r.scale)


def chunk_twice(r, x, wt, wmul=1, c0=8, width=8, co0=0, cob=32):
    """r with the K chunk [c0, c0 + width) added twice for the output-channel block [co0, co0 + cob)."""
    u = r.units.copy()
    u[:, co0:co0 + cob] += r.scale * wmul * conv_int(x[:, c0:c0 + width], wt[co0:co0 + cob, c0:c0 + width])
    return Ref(u, r.scale)


def swap_rows(r, y0=2):
    """r with output rows y0 and y0 + 1 exchanged (two rows of a Winograd output tile)."""
    u = r.units.copy()
    u[:, :, [y0, y0 + 1]] = u[:, :, [y0 + 1, y0]]
    return Ref(u, r.scale)


# ---- representability --------------------------------------------------------------------------
def f16_exact(v):
    t = torch.from_numpy(np.ascontiguousarray(v, np.float64))
    return bool(torch.equal(t, t.half().double()))


def f32_exact(v):
    v = np.asarray(v, np.float64)
    return bool(np.array_equal(v, v.astype(np.float32).astype(np.float64)))


def direct_sum_units(x, wt, b, wmul=1):
    """max over outputs of sum |x||w| + |b|: every partial sum of the direct form, in any order, is
    an integer (a multiple of the grid) of at most this magnitude."""
    return int((wmul * (conv_int(np.abs(x), np.abs(wt)) + np.abs(b)[None, :, None, None])).max())


BT2 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
G2 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
AT2 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)
BT4 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0],
                [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], np.float64)
G4_24 = np.array([[6, 0, 0], [-4, -4, -4], [-4, 4, -4], [1, 2, 4], [1, -2, 4], [0, 0, 24]], np.int64)  # 24 G4
AT4 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64)


def wino_u(wt, kind):
    """U[co, ci, eta, xi] = Gy g Gx^T, exact: integer numerators over 4 (F(2x2)) or 48 (kind 14)
    in int64, divided once in float64 (exact where the numerator has few bits: asserted)."""
    g2 = (2 * G2).astype(np.int64)
    gx, den = (G4_24, 48) if kind == 14 else (g2, 4)
    num = np.einsum("ak,oikl,bl->oiab", g2, wt.astype(np.int64), gx)
    u = num.astype(np.float64) / den
    assert np.array_equal(u * den, num.astype(np.float64))
    return u


def dyadic_grid(u):
    """The largest power of two (at most 1) that divides every value of u; None if u is not dyadic
    within 2^-20 (a third would not be)."""
    for k in range(0, 21):
        s = u * 2.0 ** k
        if np.array_equal(s, np.rint(s)):
            return 2.0 ** -k
    return None


def wino_worst(kind, cin, umax_pt, xmax):
    """Worst-case magnitude of any intermediate of the Winograd form, in units of the grid 1:
    for every output of a tile, sum over the transform points of |A^T| coefficients x cin x max|U|
    at the point x max|V| at the point (max|V| = xmax x the B^T row sums).  Never above the
    coarser cin * max|U| * max|V| * (row sums of A^T) and a bound on every partial sum all the same."""
    bx, ax = (BT4, AT4) if kind == 14 else (BT2, AT2)
    v = xmax * np.outer(np.abs(BT2).sum(1), np.abs(bx).sum(1))
    m = cin * umax_pt * v
    return float((np.abs(AT2) @ m @ np.abs(ax).T).max())


def wino_coarse(kind, cin, umax, xmax):
    bx, ax = (BT4, AT4) if kind == 14 else (BT2, AT2)
    return cin * umax * xmax * np.abs(BT2).sum(1).max() * np.abs(bx).sum(1).max() * np.abs(AT2).sum(1).max() * np.abs(ax).sum(1).max()


# ---- decoders of the packed blobs (layouts: pack_h8.hip, pack_wino.hip) -------------------------
def unpack_direct(blob, cout, cin, bm, cpr):
    """[cob][chunk of 2 cpr][tap][half][bm][cpr] -> [cout, cin, 9] float64 (r32: cpr 4, h8: cpr 8)."""
    cob, nch = -(-cout // bm), -(-cin // (2 * cpr))
    a = np.asarray(blob, np.float64).reshape(cob, nch, 9, 2, bm, cpr).transpose(0, 4, 1, 3, 5, 2).reshape(cob * bm, nch * 2 * cpr, 9)
    assert not a[cout:].any() and not a[:, cin:].any()
    return a[:cout, :cin]


def unpack_wino(blob, cout, cin, bm, cpr, points):
    """[cob][chunk of 2 cpr][point][half][bm][cpr] -> [cout, cin, points] float64."""
    cob, nch = -(-cout // bm), -(-cin // (2 * cpr))
    a = np.asarray(blob, np.float64).reshape(cob, nch, points, 2, bm, cpr).transpose(0, 4, 1, 3, 5, 2).reshape(cob * bm, nch * 2 * cpr, points)
    assert not a[cout:].any() and not a[:, cin:].any()
    return a[:cout, :cin]


def halves(t):
    """An int16 tensor of fp16 bits -> float64 numpy."""
    return t.cpu().view(torch.float16).double().numpy()


def records(v, prec_name, groups):
    """float64 NCHW -> the record planes of tests/record_ref.nchw_to_records (values must be fp32)."""
    from tests import record_ref as R
    assert f32_exact(v)
    return R.nchw_to_records(torch.from_numpy(np.ascontiguousarray(v)).float(), prec_name, groups, 0)



# ---- the sub-pixel up conv and the fused level-0 block -----------------------------------------
KR4 = np.array([[[3, 1, 0], [1, 3, 3], [0, 0, 1]], [[1, 0, 0], [3, 3, 1], [0, 1, 3]]], np.int64)  # 4 kR of pack_h8.hip


def subpixel_weights_int(wt):
    """rrin_subpixel_weights in units of 1/16: [4 cout, cin, 3, 3] int64, row (co >> 3) 32 + 8 phase + (co & 7)."""
    cout, cin = wt.shape[:2]
    out = np.zeros((4 * cout, cin, 3, 3), np.int64)
    for co in range(cout):
        for ph in range(4):
            out[(co >> 3) * 32 + ph * 8 + (co & 7)] = np.einsum("ak,bl,ikl->iab", KR4[ph >> 1], KR4[ph & 1], wt[co].astype(np.int64))
    return out


@functools.lru_cache(maxsize=None)
def block0_case(n, cin, h, w):
    """Data of the fused block (conv a cin -> 32, leaky, conv b 32 -> 32, leaky) whose intermediate
    and result are fp16 numbers although nothing is 0.  Random +-1 data grows like sqrt(K) per conv
    and leaves fp16's 11 bits after two convs and two slopes; here conv a's sum over the channels
    cancels by construction: x[c] = mag s[c] p, wa[co, c, tap] = s[c] t[co, c, tap] q[co, tap] with
    five +1 and three -1 among the t of every 8 channels (4 and 2 of 6), so each tap contributes
    +-2 mag per 8 channels, conv a is a multiple of 4 and its leaky an integer of at most 84.  Every
    one of the 9 cin products is +-mag: a dropped or doubled one still moves conv a by a grid step,
    and a K chunk added twice by +-2 mag per tap."""
    r = np.random.default_rng([7, n, cin, h, w])
    mag = 2 if cin < 16 else 1     # one group of 8 channels gives +-2 mag per tap: a multiple of 4 needs mag 2
    s = r.choice(np.asarray([-1, 1], np.int64), size=cin)
    p = r.choice(np.asarray([-1, 1], np.int64), size=(n, 1, h, w))
    x = mag * s[None, :, None, None] * p
    t = np.empty((32, cin, 3, 3), np.int64)
    for c0 in range(0, cin, 8):
        k = min(8, cin - c0)
        base = np.asarray([1] * (k // 2 + 1) + [-1] * (k - k // 2 - 1), np.int64)
        for co in range(32):
            for tap in range(9):
                t[co, c0:c0 + k, tap // 3, tap % 3] = r.permutation(base)
    q = r.choice(np.asarray([-1, 1], np.int64), size=(32, 1, 3, 3))
    wa = s[None, :, None, None] * t * q
    ba = 4 * pm((32,), (1, 2, 3), [8, cin])
    wb = pm((32, 32, 3, 3), (1,), [9, cin])
    bb = pm((32,), (1, 2, 3), [10, cin])
    for a in (x, wa):
        a.setflags(write=False)
    return x, wa, ba, wb, bb


def block0_ref(x, wa, ba, wb, bb):
    """(mid, out): leaky(conv a) -- integers -- and leaky(conv b(mid))."""
    ya = conv_int(x, wa) + ba[None, :, None, None]
    assert not (ya % 4).any()
    mid = np.where(ya > 0, ya, ya // 4)
    return Ref(mid, 1), leaky(Ref(conv_int(mid, wb) + bb[None, :, None, None], 1))


def wino_fits(kind, wt_units, den, cin, xmax):
    """(fits, worst, coarse, grid) of a Winograd conv of weights wt_units / den on |x| <= xmax: U
    must be dyadic and worst / grid -- wino_worst -- below 2^24."""
    u = wino_u(wt_units, kind) / den
    grid = dyadic_grid(u)
    if grid is None:
        return False, float("inf"), float("inf"), None
    upt = np.abs(u).max(axis=(0, 1)) / grid
    worst = wino_worst(kind, cin, upt, xmax)
    return worst < P24, worst, wino_coarse(kind, cin, float(upt.max()), xmax), grid


def split_case(n, cin, cout, h, w, mags=(1, 2), tag=0):
    """int_case with lo offsets that leave a handful of exact zeros before the activation at
    split-fp16 (the y > 0 boundary of the leaky mask, as _int_y of the training tests forces them):
    the output channel with the most integer zeros gets no weight offset, and the 3 x 3
    neighbourhoods of its zero pixels no input offset, so there the split sum is the integer 0."""
    x, wt, b, ox, ow = int_case(n, cin, cout, h, w, mags, tag)
    pre = conv_int(x, wt) + b[None, :, None, None]
    co = int((pre == 0).sum(axis=(0, 2, 3)).argmax())
    ox, ow = ox.copy(), ow.copy()
    ow[co] = 0
    for i, y, xx in np.argwhere(pre[:, co] == 0):
        ox[i, :, max(y - 1, 0):y + 2, max(xx - 1, 0):xx + 2] = 0
    return x, wt, b, ox, ow


def pre_sub_split(x, wt, b, ox):
    """The sub-pixel conv at split-fp16 with offsets on x alone: the phase-combined weights k / 16 w
    are fp16 numbers (lw = 0), so the three classes are hx*hw + lx*hw = conv(up(x + ox 2^-12), w),
    units 2^-16."""
    return Ref(LO * (conv_int(up2_int(x), wt) + 16 * b[None, :, None, None]) + conv_int(up2_int(ox), wt), 16 * LO)


# ---- part B: representable floats and forward bounds ----------------------------------------------
U = 2.0 ** -24   # unit roundoff of fp32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def split16_f64(v):
    """(hi, lo) as float64 with v = hi + lo where v holds its own split: hi = f16(v), lo = f16((v - hi) 2^11) 2^-11."""
    t = _t(v).float()
    hi = t.half().float()
    lo = ((t - hi) * 2048.0).half().float() / 2048.0
    return hi.double().numpy(), lo.double().numpy()


@functools.lru_cache(maxsize=None)
def float_case(n, cin, cout, h, w, prec):
    """(x, wt, b) float64 that the storage of prec ("R32", "F16", "F16X3") holds exactly: fp32
    numbers, fp16 numbers, numbers equal to their own hi + lo.  x in [-1, 1), w ~ N / (3 sqrt(cin))."""
    g = torch.Generator().manual_seed(100000 * n + 1000 * cin + 10 * h + w)
    x = torch.rand(n, cin, h, w, generator=g) * 2 - 1
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    b = torch.randn(cout, generator=g) * 0.1
    if prec == "F16":
        x, wt = x.half().float(), wt.half().float()
    elif prec == "F16X3":
        def own(v):
            hi = v.half().float()
            return (hi.double() + ((v - hi) * 2048.0).half().double() / 2048.0).float()
        x, wt = own(x), own(wt)
        for v in (x, wt):
            hi, lo = split16_f64(v.double().numpy())
            assert np.array_equal(hi + lo, v.double().numpy())
    return tuple(v.double().numpy() for v in (x, wt, b))


def conv64(x, wt, b=None):
    import torch.nn.functional as F
    return F.conv2d(_t(x), _t(wt), None if b is None else _t(b), padding=1).numpy()


def s_of(x, wt, b):
    """S = sum |x||w| + |b| per output element."""
    return conv64(np.abs(x), np.abs(wt), np.abs(b))


def leaky64(y):
    return np.where(y > 0, y, SLOPE * y)


def pool64(y):
    return (y[:, :, 0::2, 0::2] + y[:, :, 0::2, 1::2] + y[:, :, 1::2, 0::2] + y[:, :, 1::2, 1::2]) / 4


def bound(prec, k, s, ref, wino_ratio=None):
    """Per-element forward bound of |got - ref64| before pooling ("Forward bounds").

    Direct form, K = 9 cin products per output.  Every product of two fp32 (fp16) operands enters
    an fp32 accumulator with one rounding of a partial sum that is at most S in magnitude, so K
    roundings cost K u S, u = 2^-24; the bias add and the slope multiply cost one each (the slope
    1/4 of these tests is exact; the constant keeps it): (K + 2) u S.
      fp16: products of fp16 numbers are exact in fp32, the power-of-two weight scale is exact;
            the stored fp16 result adds half an ulp, 2^-11 |ref|, and 2^-25 below the normal range.
      split-fp16: three product classes, 3 K accumulations, the fma that joins the two
            accumulators and the bias: (3 K + 2) u S; the dropped lo*lo class is at most
            (2^-11)^2 |x||w| summed: 2^-22 S; the split store keeps hi + lo with lo rounded to
            fp16, half an ulp of lo, 2^-11 x 2^-11 |v|: 2^-22 |ref|.
    Winograd forms: 4 x the worst err / (u S) of the fp32 (fp16 for kind 6 at fp16) numpy emulation
    wino_emulate against float64 on the same data (wino_ratio), plus the fp16 store terms.  The
    leaky epilogue does not grow an error (|leaky(a) - leaky(b)| <= |a - b|), so the bound of the
    pre-activation holds after it."""
    if wino_ratio is not None:
        base = 4 * wino_ratio * U * s
        return base + (2.0 ** -11 * np.abs(ref) + 2.0 ** -25 if prec == "F16" else 0.0)
    if prec == "R32":
        return (k + 2) * U * s
    if prec == "F16":
        return (k + 2) * U * s + 2.0 ** -11 * np.abs(ref) + 2.0 ** -25
    return (3 * k + 2) * U * s + 2.0 ** -22 * s + 2.0 ** -22 * np.abs(ref)


def pool_bound(prec, bnd, ref, refp):
    """The pooled value is the mean of four outputs, each within bnd (whether the kernel pools
    before or after its store rounding), formed with three fp32 additions of partial sums of at
    most sum |v| (3 u mean|v|) and an exact x 1/4, then stored: fp16 2^-11 |refp| + 2^-25,
    split-fp16 2^-22 |refp|."""
    out = pool64(bnd) + 3 * U * pool64(np.abs(ref) + bnd)
    if prec == "F16":
        out = out + 2.0 ** -11 * np.abs(refp) + 2.0 ** -25
    if prec == "F16X3":
        out = out + 2.0 ** -22 * np.abs(refp)
    return out


G4 = G4_24.astype(np.float64) / 24


def wino_emulate(x, wt, b, kind, f16=False, rep=False):
    """The Winograd convs restated in numpy at the kernels' precision: U = Gy g Gx^T in double,
    rounded once (fp32; f16: x 2^s with max |U| 2^s in [2^12, 2^13), rounded to fp16); V = B^T d B
    in fp32 (f16: in fp16); M = sum over the channels in channel (= chunk) order, fp32 products
    added into an fp32 accumulator; Y = A^T M A in fp32 (f16: x 2^-s), plus the bias.  kind 14 is
    F(2,3) along y and F(4,3) along x (G4, BT4, AT4), every other kind F(2x2,3x3).  Returns the
    pre-activation as float64."""
    f = np.float32
    n, cin, h, w = x.shape
    gx, bx, ax, tw, ww = (G4, BT4, AT4, 4, 6) if kind == 14 else (G2, BT2, AT2, 2, 4)
    u = np.einsum("ak,oikl,bl->oiab", G2, wt, gx)
    inv = 1.0
    if f16:
        s = 13 - int(np.frexp(np.abs(u).max())[1])
        u, inv = (u * 2.0 ** s).astype(np.float16), 2.0 ** -s
    u = u.astype(f)
    vd = np.float16 if f16 else f
    hh, wd = -(-h // 2) * 2, -(-w // tw) * tw
    xp = np.zeros((n, cin, hh + 2, wd + 2), vd)
    xp[:, :, 1:h + 1, 1:w + 1] = x
    if rep:   # the source's edge-replicated ring (the sub-pixel conv reads it); zero beyond it
        xp[:, :, :h + 2, :w + 2] = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge")
    win = np.lib.stride_tricks.sliding_window_view(xp, (4, ww), axis=(2, 3))[:, :, ::2, ::tw]
    t = np.einsum("ab,ncpqbd->ncpqad", BT2.astype(vd), win).astype(vd)
    v = np.einsum("ncpqad,ed->ncpqae", t, bx.astype(vd)).astype(vd).astype(f)
    m = np.zeros((n, wt.shape[0]) + v.shape[2:], f)
    for c in range(cin):
        m += u[None, :, c, None, None] * v[:, None, c]
    y = np.einsum("ra,nopqab->nopqrb", AT2.astype(f), m).astype(f)
    y = np.einsum("nopqrb,sb->noprqs", y, ax.astype(f)).astype(f)
    y = y.reshape(n, wt.shape[0], hh, wd)[:, :, :h, :w]
    return ((y * f(inv)).astype(f) + b.astype(f)[None, :, None, None]).astype(np.float64)


@functools.lru_cache(maxsize=None)
def wino_ratio(n, cin, cout, h, w, prec, kind):
    """Worst err / (u S) of wino_emulate against float64 on float_case(...): the measured
    amplification of the transforms (recorded in DESIGN.md §8b; tests/test_exact_ref.py pins them)."""
    x, wt, b = float_case(n, cin, cout, h, w, prec)
    err = np.abs(wino_emulate(x, wt, b, kind, prec == "F16") - conv64(x, wt, b))
    return float((err / (U * s_of(x, wt, b))).max())


# ---- the sub-pixel up conv: more exact cases ---------------------------------------------------------
FIX_PX = FIX_CI = 32       # the ring fix-up's tile: line pixels and input channels per chunk (common.hpp)


def ring_mask(hh, ww):
    m = np.zeros((hh, ww), bool)
    m[0] = m[-1] = m[:, 0] = m[:, -1] = True
    return m


def edge_split(cin, prec, mode):
    """(K groups, K runs) of a ring pixel's sum.  "fix" / "full": the standalone fix-up
    (edge_fix.hip, edge_fix_split); "inlaunch": ring_full with the conv -- one group, fp32 records in
    runs of one chunk; "fold": one chain (winoq_ring.hpp, ring_block)."""
    if mode == "fold":
        return 1, 1
    if mode == "inlaunch":
        return 1, (cin // FIX_CI if prec == "R32" and cin % FIX_CI == 0 else 1)
    if prec == "R32":
        ks = 2 if cin % (2 * FIX_CI) == 0 else 1
        return ks, (cin // (ks * FIX_CI) if cin % (ks * FIX_CI) == 0 else 1)
    ks = 2 if cin % (2 * FIX_CI) == 0 and cin >= 4 * FIX_CI else 1
    if prec == "F16" and cin % (4 * FIX_CI) == 0 and cin >= 8 * FIX_CI:
        ks = 4
    return ks, 1


def f16_round(v):
    """float64 -> the nearest fp16 number, ties to even, as float64."""
    return np.asarray(v, np.float64).astype(np.float16).astype(np.float64)


def own_split(v):
    hi, lo = split16_f64(v)
    return bool(np.array_equal(hi + lo, np.asarray(v, np.float64)))


def seam_shift(r, left=False):
    """r with the first ring pixel of the second fix-up tile taken from its neighbour one further on:
    top row x = 32 from x = 33, or (left) the left column y = 33 from y = 34 (the columns start at y = 1)."""
    u = r.units.copy()
    if left:
        u[:, :, FIX_PX + 1, 0] = u[:, :, FIX_PX + 2, 0]
    else:
        u[:, :, 0, FIX_PX] = u[:, :, 0, FIX_PX + 1]
    return Ref(u, r.scale)


def ring_groups_miscounted(r, up, wt, wmul, ks):
    """r whose ring pixels sum ks - 1 of the ks K groups: the chunks of 32 channels the last group owns
    (chunk index = ks - 1 mod ks) are left out of every ring pixel."""
    cin = up.shape[1]
    sel = np.asarray([c for c in range(cin) if (c // FIX_CI) % ks == ks - 1])
    part = (r.scale // 16) * wmul * conv_int(up[:, sel], wt[:, sel])
    u = r.units.copy()
    m = ring_mask(*u.shape[2:])
    u[:, :, m] -= part[:, :, m]
    return Ref(u, r.scale)


# ---- the sub-pixel up conv on floats: forward bounds -----------------------------------
@functools.lru_cache(maxsize=None)
def sub_float_case(n, cin, cout, h, w, prec):
    """(x, wt, b): x and b as float_case; w = m 2^-8, |m| <= 31, so that the phase-combined weights
    (sums of k m 2^-12 with sum |k| <= 49 -- the centre tap gathers (1 + 3 + 3)^2 sixteenths -- so
    |numerator| <= 1519 < 2^11) are fp16 numbers at any
    power-of-two scale and the packs hold them exactly."""
    x, _, b = float_case(n, cin, cout, h, w, prec)
    r = np.random.default_rng([11, n, cin, cout, h, w])
    wt = r.integers(-31, 32, size=(cout, cin, 3, 3)).astype(np.float64) / 256
    return x, wt, b


def phase_weights64(wt):
    """[4, cout, cin, 3, 3]: phase 2 (Y & 1) + (X & 1) of rrin_subpixel_weights, over the low-res taps."""
    return np.stack([np.einsum("ak,bl,oikl->oiab", KR4[ph >> 1] / 4.0, KR4[ph & 1] / 4.0, wt) for ph in range(4)])


def phase_rows(wp):
    """[4, cout, cin, 3, 3] -> the [4 cout, cin, 3, 3] row order of rrin_subpixel_weights."""
    cout = wp.shape[1]
    out = np.empty((4 * cout,) + wp.shape[2:], wp.dtype)
    for co in range(cout):
        for ph in range(4):
            out[(co >> 3) * 32 + ph * 8 + (co & 7)] = wp[ph, co]
    return out


def replicate(x):
    return np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge")


def conv_valid64(xp, wt, b=None):
    import torch.nn.functional as F
    return F.conv2d(_t(xp), _t(wt), None if b is None else _t(b)).numpy()


def phase64(x, wp, b):
    """The sub-pixel form in float64: output (Y, X) is the 3 x 3 conv with phase 2 (Y & 1) + (X & 1)
    over the edge-replicated x at (Y >> 1, X >> 1), plus b.  Equal to conv(upsample(x)) off the ring."""
    n, _, h, w = x.shape
    xp = replicate(x)
    out = np.empty((n, wp.shape[1], 2 * h, 2 * w))
    for ph in range(4):
        out[:, :, ph >> 1::2, ph & 1::2] = conv_valid64(xp, wp[ph], b)
    return out


def up_emulate(x, dt=np.float32, align=False):
    """Bilinear x2 as Up8::value (edge_fix.hpp): horizontal then vertical, weights 1/4 and 3/4, edge
    clamp, every operation rounded to dt (float64: the exact upsample of fp32 data)."""
    import torch.nn.functional as F
    if align:
        return F.interpolate(_t(x), scale_factor=2, mode="bilinear", align_corners=True).numpy().astype(dt)
    x = np.asarray(x, dt)
    h, w = x.shape[2:]

    def taps(nn):
        o = np.arange(2 * nn)
        odd = (o & 1) == 1
        a = np.where(odd, o >> 1, np.maximum((o >> 1) - 1, 0))
        b_ = np.where(odd, np.minimum((o >> 1) + 1, nn - 1), o >> 1)
        return a, b_, np.where(odd, 0.75, 0.25).astype(dt)
    ra, rb, wa = taps(h)
    ca, cb, wc = taps(w)
    wb, wd = (1 - wa).astype(dt), (1 - wc).astype(dt)
    top = wc * x[:, :, ra][..., ca] + wd * x[:, :, ra][..., cb]
    bot = wc * x[:, :, rb][..., ca] + wd * x[:, :, rb][..., cb]
    out = wa[:, None] * top + wb[:, None] * bot
    assert out.dtype == dt
    return out


def _fma(acc, wv, uv):
    """acc + w u with one rounding to fp32; acc [n, cout, ...], wv [cout], uv [n, ...]."""
    wv = wv.astype(np.float64).reshape((1, -1) + (1,) * (acc.ndim - 2))
    return (acc.astype(np.float64) + wv * uv.astype(np.float64)[:, None]).astype(np.float32)


def phase_emulate(x, wp):
    """The phase convs' pre-bias value in fp32, one fma per product in channel then tap order: what the
    direct tiles leave in the edge buffer.  [n, cout, 2h, 2w] float32."""
    n, cin, h, w = x.shape
    xp = replicate(x).astype(np.float32)
    out = np.empty((n, wp.shape[1], 2 * h, 2 * w), np.float32)
    for ph in range(4):
        acc = np.zeros((n, wp.shape[1], h, w), np.float32)
        for ci in range(cin):
            for a in range(3):
                for b_ in range(3):
                    acc = _fma(acc, wp[ph][:, ci, a, b_], xp[:, ci, a:a + h, b_:b_ + w])
        out[:, :, ph >> 1::2, ph & 1::2] = acc
    return out


def edge_emulate(x, wt, b, mode, ks=1, nsl=1, pre=None, mutate=None):
    """The ring of the sub-pixel conv restated in numpy fp32 (edge_fix.hpp, edge_fix_body).

    mode "full": from scratch -- per ring pixel the in-image taps over two staged lines of U (the
    ring line and the next one inward, zero past the line's ends), slots in the order line 0 taps
    0-2, line 1 taps 0-2.  mode "corr": (pre - acc) + b with acc the outside taps over the ring line
    of U clamped at its ends, and at a corner the two further taps of the outside column, summed
    apart (accx) and added at the end of each run.  U is recomputed in fp32 (up_emulate).  The
    channels go in chunks of 32: run sl of nsl covers cin / nsl channels, in it group g of ks takes
    chunks g, g + ks, ...; the groups' sums are added in group order, the runs' in run order.
    Lines: top and bottom row with the corners, left and right column without.  Returns float32
    [n, cout, 2h, 2w], NaN off the ring.  mutate: "no_extras", "align_corners", "group_twice",
    "seam" -- the errors the bound must reject (tests/test_exact_ref.py)."""
    f = np.float32
    n, cin, h, w = x.shape
    cout, hh, ww = wt.shape[0], 2 * h, 2 * w
    u = up_emulate(x, f, align=mutate == "align_corners")
    w32, b32 = wt.astype(f), b.astype(f)
    out = np.full((n, cout, hh, ww), np.nan, f)
    csl = cin // nsl
    assert csl * nsl == cin and (nsl == 1 and ks == 1 or csl % (ks * FIX_CI) == 0)
    for line, fixed, pos in ((0, 0, np.arange(ww)), (1, hh - 1, np.arange(ww)),
                             (2, 0, np.arange(1, hh - 1)), (3, ww - 1, np.arange(1, hh - 1))):
        if not pos.size:
            continue
        row = line < 2
        full = ww if row else hh
        out_k = 0 if line in (0, 2) else 2
        inner = fixed + (1 if line in (0, 2) else -1)

        def staged(o, q):
            qc = np.clip(q, 0, full - 1)
            v = u[:, :, o, qc] if row else u[:, :, qc, o]
            return np.where((q >= 0) & (q < full), v, f(0)) if mode == "full" else v
        extras = []
        if mode == "full":
            kk = 2 if inner > fixed else 0
            slots = [((1, k) if row else (k, 1), staged(fixed, pos - 1 + k)) for k in range(3)]
            slots += [((kk, k) if row else (k, kk), staged(inner, pos - 1 + k)) for k in range(3)]
        else:
            slots = [((out_k, k) if row else (k, out_k), staged(fixed, pos - 1 + k)) for k in range(3)]
            if row and mutate != "no_extras":
                for xc, kx in ((0, 0), (ww - 1, 2)):
                    for m in range(2):
                        ky = m + (1 if out_k == 0 else 0)
                        ue = np.zeros((n, cin, pos.size), f)
                        ue[:, :, xc] = u[:, :, fixed + ky - 1, xc]
                        extras.append(((ky, kx), ue))
        corner = (pos == 0) | (pos == ww - 1) if row else np.zeros(pos.size, bool)
        tot = None
        for sl in range(nsl):
            sums = []
            for g in range(ks):
                acc = np.zeros((n, cout, pos.size), f)
                accx = np.zeros((n, cout, pos.size), f)
                for c0 in range(sl * csl + g * FIX_CI, (sl + 1) * csl, ks * FIX_CI):
                    for ci in range(c0, min(c0 + FIX_CI, cin)):
                        for (ky, kx), uv in slots:
                            acc = _fma(acc, w32[:, ci, ky, kx], uv[:, ci])
                    for ci in range(c0, min(c0 + FIX_CI, cin)):
                        for (ky, kx), uv in extras:
                            accx = _fma(accx, w32[:, ci, ky, kx], uv[:, ci])
                sums.append(np.where(corner, acc + accx, acc) if extras else acc)
            run = sums[0]
            for g in range(1, ks):
                run = run + sums[g]
            if mutate == "group_twice" and sl == 0:
                run = run + sums[-1]
            tot = run if sl == 0 else tot + run
        bb = b32[None, :, None]
        if mode == "full":
            v = tot + bb
        else:
            p = pre[:, :, fixed, pos] if row else pre[:, :, pos, fixed]
            v = (p.astype(f) - tot) + bb
        assert v.dtype == f
        if row:
            out[:, :, fixed, pos] = v
        else:
            out[:, :, pos, fixed] = v
    if mutate == "seam":
        out[:, :, 0, FIX_PX] = out[:, :, 0, FIX_PX + 1]
    return out


def store_emulate(v, prec):
    """The store of an fp32 value at prec, as float64."""
    v = np.asarray(v, np.float32)
    if prec == "F16":
        return v.astype(np.float16).astype(np.float64)
    if prec == "F16X3":
        hi, lo = split16_f64(np.nan_to_num(v.astype(np.float64)))
        return np.where(np.isnan(v), np.nan, hi + lo)
    return v.astype(np.float64)


def store_bound(prec, ref):
    """The store terms of bound(): fp16 half an ulp and the subnormal floor, split-fp16 the rounded lo."""
    if prec == "F16":
        return 2.0 ** -11 * np.abs(ref) + 2.0 ** -25
    if prec == "F16X3":
        return 2.0 ** -22 * np.abs(ref)
    return 0.0


def pre_bound(prec, k, s, wino_ratio=None):
    """Bound of the conv's pre-bias fp32 value (the edge buffer): bound()'s forms without the bias
    add, the slope multiply and the store -- K u S; split-fp16 (3 K + 1) u S + 2^-22 S; Winograd
    4 x ratio u S."""
    if wino_ratio is not None:
        return 4 * wino_ratio * U * s
    if prec == "F16X3":
        return (3 * k + 1) * U * s + 2.0 ** -22 * s
    return k * U * s


def sub_terms(x, wt, b):
    """Per output pixel of the 2h x 2w result, float64: s_phase (sum |x_rep||w_phase| + |b| of the
    pixel's phase), s_in (sum over the in-image taps of |w| x' + |b|, x' = upsample(|x|)), s_out
    (the same over the taps outside the image, x' clamped), n_in (in-image taps: 9, 6, 4)."""
    cout = wt.shape[0]
    s_phase = phase64(np.abs(x), np.abs(phase_weights64(wt)), np.abs(b))
    xa = up_emulate(np.abs(x), np.float64)
    aw = np.abs(wt)
    s_in = conv64(xa, aw, np.abs(b))
    xo = replicate(xa)
    xo[:, :, 1:-1, 1:-1] = 0
    s_out = conv_valid64(xo, aw)
    n_in = conv64(np.ones((1, 1) + xa.shape[2:]), np.ones((1, 1, 3, 3)))[0, 0]
    assert s_in.shape[1] == cout
    return s_phase, s_in, s_out, np.rint(n_in)


def ring_bound(prec, mode, cin, terms, ref, b, wino_ratio=None):
    """Per-element bound of |got - ref64| on the ring (valid on ring pixels only), u = 2^-24.

    Every staged U value is recomputed in fp32 with at most 4 roundings of numbers no larger than
    x' (§8d): within 4 u x' of exact, 4 u sum |w| x' through the taps.  A chain of T fmas rounds T
    partial sums of at most the sum of absolute values; adding G group / run sums rounds G more.
      from scratch ("full", "inlaunch"): T = n_in cin in-image taps, G = (ks - 1) + (nsl - 1), the
        bias add: (n_in cin + 4 + G + 1) u S_in, S_in = sum_in |w| x' + |b|.
      correction ("fix", "fold"): the conv's pre-bias value within pre_bound over S_phase; the outside
        taps T = (9 - n_in) cin, the U term, G and at a corner one more add (accx; none in the fold's
        single chain): ((9 - n_in) cin + 4 + G + c) u S_out; pre - acc and + bias round results of at
        most S_in: 2 u S_in.  In sums of absolute values: pre - acc cancels.
    plus the store terms of bound()."""
    s_phase, s_in, s_out, n_in = terms
    name = "fix" if mode == "full" else mode
    ks, nsl = edge_split(cin, prec, name)
    g = (ks - 1) + (nsl - 1)
    if mode in ("full", "inlaunch"):
        return (n_in * cin + 4 + g + 1) * U * s_in + store_bound(prec, ref)
    c = (n_in == 4) * (0 if mode == "fold" else 1)
    s_pre = s_phase if wino_ratio is not None else s_phase - np.abs(b)[None, :, None, None]
    return (pre_bound(prec, 9 * cin, s_pre, wino_ratio) + ((9 - n_in) * cin + 4 + g + c) * U * s_out
            + 2 * U * s_in + store_bound(prec, ref))


def sub_ref64(x, wt, b):
    return conv64(up_emulate(x, np.float64), wt, b)


@functools.lru_cache(maxsize=None)
def sub_wino_ratio(n, cin, cout, h, w, prec, kind):
    """Worst err / (u S) of wino_emulate on the phase weights over the edge-replicated source of
    sub_float_case(...) against float64 (pinned by tests/test_exact_ref.py)."""
    x, wt, b = sub_float_case(n, cin, cout, h, w, prec)
    wp = phase_weights64(wt).reshape(4 * cout, cin, 3, 3)
    b4 = np.tile(b, 4)
    got = wino_emulate(x, wp, b4, kind, prec == "F16", rep=True)
    xp = replicate(x)
    ref = conv_valid64(xp, wp, b4)
    s = conv_valid64(np.abs(xp), np.abs(wp), np.abs(b4))
    return float((np.abs(got - ref) / (U * s)).max())


# ---- launch paths (tests/test_gpu_h8_paths.py; DESIGN.md §8b, "Launch paths") ------------------------
# (n, cin, cout, h, w), cheapest first.  A test takes the first entry at which the launch-shape query
# (rrin_conv_h8_launch_info) reports the branch it wants: a walk of unequal length (grid < tiles,
# tiles % grid != 0, tiles > 2 grid) for the configs with a capped grid, grid >= 64 and grid % 8 != 0
# for the others.  Odd sizes one past a tile multiple buy the most tiles per pixel (17 x 65 is
# 3 x 3 tiles of 32 x 8); n and cout grow before the pixels do.  The last entries carry the capped
# grids of 256 to 1280 workgroups that 256 CUs give; one cin 64 entry per launch form.
LADDER = (
    (5, 16, 40, 17, 65), (5, 16, 40, 33, 65), (5, 16, 128, 33, 65), (5, 16, 256, 33, 65), (5, 64, 40, 33, 65),
    (5, 64, 128, 33, 65), (6, 16, 256, 49, 161), (6, 16, 256, 97, 161), (6, 16, 256, 113, 161), (6, 64, 256, 49, 161),
    (6, 64, 256, 97, 161),
)
# the sub-pixel up conv: (h, w) the low-res source, cout the up conv's (the conv has 4 cout phase
# channels, so 4 co blocks per 32); cin 32, the least at which ring_full runs inside the conv's launch
LADDER_SUB = ((5, 32, 32, 33, 65), (5, 32, 64, 33, 65), (6, 32, 64, 49, 161), (6, 32, 64, 97, 161), (6, 32, 64, 113, 161))
K14_TALL = [(2, 16, 32, 1, 1), (2, 16, 32, 1, 40), (2, 16, 32, 40, 1), (2, 16, 32, 17, 33), (2, 64, 40, 18, 34),
            (2, 256, 32, 17, 33)]
K14_TALL_AUTO = (4, 16, 256, 45, 80)      # co_blocks n = 32: 576 tiles of 32 x 8 (two rounds of 512), 480 of 16 x 16
K14_PERSIST = [(2, 32, 96, 1024), (2, 40, 97, 950), (3, 32, 100, 900)]   # (n, cout, h, w)
K14_PERSIST_SUB = [(2, 16, 32, 48, 512), (2, 16, 32, 49, 475), (3, 16, 32, 50, 450)]   # 768, 840, 1260 tiles
K14_PERSIST_CIN = (8, 16, 24, 64)         # nch 1, 2, > 2 and 8 chunks; 64 at the first shape only
# the co-block group walk (wino_cob_group): cin 256 puts U of 5 co blocks of 32 (3 of 64) past 2 MB;
# fp16 kind 6 halves U per channel (16-channel chunks), so cout 320
COB_SHAPE, COB_SHAPE_F16 = (3, 256, 160, 17, 65), (3, 256, 320, 17, 65)
BLOCK0_PATHS = [(3, 8, 17, 125), (3, 16, 18, 126)]   # (n, cin, h, w): 3 x 3 x 3 = 27 tiles of 62 x 8, 27 % 8 = 3


def tile_boxes(n, cout, h, w, bm, th, tw=32):
    """The (image, co0, co1, y0, y1, x0, x1) box of every tile, in the launchers' order: co block
    fastest, then x, then y, then the image (wino_tile_pos with one co-block group; conv_h8.hip)."""
    out = []
    for i in range(n):
        for y0 in range(0, h, th):
            for x0 in range(0, w, tw):
                for c0 in range(0, cout, bm):
                    out.append((i, c0, min(c0 + bm, cout), y0, min(y0 + th, h), x0, min(x0 + tw, w)))
    return out


def _box(u, b):
    i, c0, c1, y0, y1, x0, x1 = b
    return u[i, c0:c1, y0:y1, x0:x1]


def tile_from_other(r, boxes, k, j):
    """r with tile k's outputs replaced by tile j's (same box size): a workgroup that computed its
    third tile at another tile's coordinates."""
    u = r.units.copy()
    a, b_ = _box(u, boxes[k]), _box(r.units, boxes[j])
    assert a.shape == b_.shape
    a[...] = b_
    return Ref(u, r.scale)


def tile_with_previous_bias(r, boxes, k, j, b, wmul=1):
    """r (a pre-activation) with tile k carrying the bias of tile j's co block instead of its own."""
    u = r.units.copy()
    (_, c0, c1, *_), (_, d0, d1, *_) = boxes[k], boxes[j]
    assert c1 - c0 == d1 - d0
    _box(u, boxes[k])[...] += r.scale * wmul * (b[d0:d1] - b[c0:c1])[:, None, None]
    return Ref(u, r.scale)


def last_tiles_unwritten(v, boxes, grid, fill=np.nan):
    """float64 v with the last len(boxes) % grid tiles left at `fill`: a walk that stops a round early."""
    v = v.copy()
    rem = len(boxes) % grid
    assert rem
    for b in boxes[-rem:]:
        _box(v, b)[...] = fill
    return v
