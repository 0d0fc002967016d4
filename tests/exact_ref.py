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
    for ky in range(3):
        for kx in range(3):
            if taps is not None and (ky, kx) not in taps:
                continue
            cols = xp[:, :, ky:ky + h, kx:kx + wd].transpose(1, 0, 2, 3).reshape(c, -1)
            y += (w[:, :, ky, kx].astype(np.int64) @ cols).reshape(-1, n, h, wd).transpose(1, 0, 2, 3)
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
    mag = 2 if cin < 8 else 1
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


def wino_emulate(x, wt, b, kind, f16=False):
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
