"""CPU side of the planar fp32 kernel tests (tests/test_gpu_planar.py): the cases, data on which
every summation order gives the same fp32 bits, int64 references of rrin_conv3x3_fwd in both source
modes and the three epilogues, their mutations, the forward bounds on floats with an fp32 emulation
of the UPSAMPLE2X staging, the decoder of rrin_pack_conv3x3's blob, and the flow field and fp32
coordinate emulation of the rrin_warp_fwd tests.  No GPU call.

Data rules: x and w are +-1 / +-2 (never 0), the bias +-1..3, the slope 1/4.  The
bilinear x2 weights are 9/16, 3/16, 3/16, 1/16, so an upsampled input is an integer in units of 1/16
and the conv of it an int64 in that unit; LEAKY moves the grid to 1/4 of it and the 2 x 2 mean to
1/16 of it.  ``worst_steps`` bounds every partial sum in steps of the final grid; below 2^24 every
intermediate of every summation order is an fp32 number and the result has one possible value."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests import exact_ref as E

LINEAR, LEAKY, POOL = 0, 1, 2          # rrin_epi_mode
EPIS = (LINEAR, LEAKY, POOL)
N = 2                                  # images: the image stride is exercised
CHANNELS = [(1, 1), (10, 3), (16, 40), (64, 32)]
DEEP = (256, 32)                       # deep K, at 18 x 34 only
BMS = (32, 64, 128)
REFINE_PERM = (4, 5, 6, 7, 8, 9, 0, 1, 2, 3)

# output h x w -> the (upsample, epilogues) run at it; the source is half the size under UPSAMPLE2X
SHAPES = {
    (1, 1): [(False, (LINEAR, LEAKY))],
    (2, 2): [(False, EPIS), (True, EPIS)],          # pool -> 1 x 1, upsample from 1 x 1
    (1, 40): [(False, (LINEAR, LEAKY))],
    (40, 1): [(False, (LINEAR, LEAKY))],
    (2, 80): [(True, EPIS)],
    (80, 2): [(True, EPIS)],
    (18, 34): [(False, EPIS), (True, EPIS)],        # ragged in both tile directions for TH 4, 8, 16
    (17, 33): [(False, (LINEAR, LEAKY))],
}


def channel_sets(h, w):
    return CHANNELS + ([DEEP] if (h, w) == (18, 34) else [])


def combos(h, w):
    """(upsample, epi, cin, cout) of every conv case at output size h x w."""
    return [(up, epi, cin, cout) for up, epis in SHAPES[(h, w)] for epi in epis for cin, cout in channel_sets(h, w)]


# ---- integer data and references -------------------------------------------------------------------
def worst_steps(x, wt, b, up, epi):
    """max over outputs of sum |x'||w| + |b| (x' the upsampled input) in steps of the final grid:
    every partial sum of the staging, the K loop and the epilogue is a multiple of a grid at least
    as coarse and at most this large (the pool's sum of four is 4 x a mean of four)."""
    xin = E.up2_int(np.abs(x)) if up else np.abs(x)
    s = E.conv_int(xin, np.abs(wt)) + (16 if up else 1) * np.abs(b)[None, :, None, None]
    return int(s.max()) * (1, 4, 16)[epi]


@functools.lru_cache(maxsize=None)
def int_case(cin, cout, h, w, up, tag=0):
    """(x, wt, b) int64 for an output of h x w: +-1 / +-2, shrunk to +-1 where the partial sums of
    the finest grid of the source mode would leave 2^24 steps."""
    sh, sw = (h // 2, w // 2) if up else (h, w)
    for mags in ((1, 2), (1,)):
        x, wt, b, _, _ = E.int_case(N, cin, cout, sh, sw, mags, 100 + tag)
        if worst_steps(x, wt, b, up, POOL) < E.P24:
            return x, wt, b
    raise AssertionError("no data fits 2^24")


def pre_ref(x, wt, b, up):
    return E.pre_sub(x, wt, b) if up else E.pre_int(x, wt, b)


def epilogue(pre, epi):
    """(dst, pool or None) of the pre-activation."""
    r = pre if epi == LINEAR else E.leaky(pre)
    return r, (E.pool(r) if epi == POOL else None)


@functools.lru_cache(maxsize=None)
def conv_ref(cin, cout, h, w, up, epi, tag=0, perm=None):
    """(dst, pool or None) as float32 tensors, exact.  perm: packed input channel c meets the
    weights of channel perm[c] (rrin_pack_conv3x3)."""
    x, wt, b = int_case(cin, cout, h, w, up, tag=tag)
    if perm is not None:
        wt = wt[:, list(perm)]
    out = []
    for r in epilogue(pre_ref(x, wt, b, up), epi):
        if r is None:
            out.append(None)
            continue
        v = r.f64()
        assert E.f32_exact(v)
        out.append(torch.from_numpy(v.astype(np.float32)))
    return tuple(out)


# ---- mutations: each must break the equality ----------------------------------------------------------
def up2_swapped(x):
    """up2_int with the weight pair exchanged (1/4 <-> 3/4 along x) at output column 2 W - 2, the last
    one whose two taps are different source columns (column 2 W - 1 reads the clamped border twice)."""
    u = E.up2_int(x)
    xi = x.astype(np.int64)
    col = 3 * xi[..., -2] + xi[..., -1]                      # 4 x (3/4 L[W-2] + 1/4 L[W-1]), rows still source rows
    prev = np.concatenate([col[:, :, :1], col[:, :, :-1]], 2)
    nxt = np.concatenate([col[:, :, 1:], col[:, :, -1:]], 2)
    u = u.copy()
    u[:, :, 0::2, -2] = 3 * col + prev
    u[:, :, 1::2, -2] = 3 * col + nxt
    return u


def mutants(x, wt, b, up, epi, bm=32):
    """name -> (dst, pool) Refs of the mutations that apply to this data set."""
    xin = E.up2_int(x) if up else x
    pre = pre_ref(x, wt, b, up)
    n, cin, h, w = xin.shape
    m = {}
    u = pre.units.copy()                                     # a dropped tap of one channel at one pixel
    y, xx, ch, co = h - 1, w // 2, cin - 1, wt.shape[0] - 1
    u[1, co, y, xx] -= int(wt[co, ch, 1, 1]) * int(xin[1, ch, y, xx])
    m["drop_tap"] = epilogue(E.Ref(u, pre.scale), epi)
    u = pre.units.copy()                                     # the last 8-channel chunk twice for the last BM block
    c0, co0 = (cin - 1) // 8 * 8, (wt.shape[0] - 1) // bm * bm
    u[:, co0:] += E.conv_int(xin[:, c0:], wt[co0:, c0:])
    m["chunk_twice"] = epilogue(E.Ref(u, pre.scale), epi)
    if up and x.shape[3] >= 2:
        m["bilinear_swapped"] = epilogue(E.Ref(E.conv_int(up2_swapped(x), wt) + 16 * b[None, :, None, None], 16), epi)
    if h >= 2:
        m["rows_swapped"] = epilogue(E.swap_rows(pre, h - 2), epi)
    if epi == POOL and h >= 4:                               # the pool over rows (1, 2), (3, 4), ...
        r = E.leaky(pre)
        rolled = E.Ref(np.concatenate([r.units[:, :, 1:], r.units[:, :, -1:]], 2), r.scale)
        m["pool_rows"] = (r, E.pool(rolled))
    return m


# ---- rrin_pack_conv3x3 ------------------------------------------------------------------------------
def unpack_planar(blob, bias, cout, cin, bm):
    """[cob][chunk][8 ci][9 taps][bm] -> ([cout, cin, 9] float64, [cout]); the padding must be zero."""
    cob, nch = -(-cout // bm), -(-cin // 8)
    a = np.asarray(blob, np.float64).reshape(cob, nch, 8, 9, bm).transpose(0, 4, 1, 2, 3).reshape(cob * bm, nch * 8, 9)
    bias = np.asarray(bias, np.float64)
    assert a.shape[0] == bias.shape[0] and not a[cout:].any() and not a[:, cin:].any() and not bias[cout:].any()
    return a[:cout, :cin], bias[:cout]


# ---- forward bounds on floats ---------------------------------------------------------
U = E.U
NET_SLOPE = 0.1
UP_ROUNDINGS = 4   # per upsampled value: 3/4 a and the add, along x then along y (1/4 a is exact)
FLOAT_SHAPE = (16, 40, 18, 34)   # cin, cout, output h, w


@functools.lru_cache(maxsize=None)
def float_case(up):
    from rrin_amd.synthetic import keyed_tensor
    cin, cout, h, w = FLOAT_SHAPE
    sh, sw = (h // 2, w // 2) if up else (h, w)
    g = torch.Generator().manual_seed(4242 + int(up))
    x = torch.rand(N, cin, sh, sw, generator=g) * 2 - 1
    wt = keyed_tensor(f"planar.{int(up)}.w", (cout, cin, 3, 3), 9 * cin)
    b = keyed_tensor(f"planar.{int(up)}.b", (cout,), 9 * cin)
    return x, wt, b


def up64(x, align_corners=False):
    return F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=align_corners)


def leaky64(y, slope=NET_SLOPE):
    return torch.where(y > 0, y, slope * y)


def float_ref(x, wt, b, up, epi, align_corners=False):
    """(dst, pool or None, bound dst, bound pool) float64 numpy.

    DIRECT is the fp32 direct-form bound of §8b, (K + 2) u S with K = 9 cin, S = sum |x||w| + |b|.
    UPSAMPLE2X: the kernel forms each staged value as wa (1/4 l + 3/4 c) + wb (1/4 l' + 3/4 c') with
    wa, wb in {1/4, 3/4}: per axis the product with 1/4 is exact, the one with 3/4 rounds and the add
    rounds -- at most UP_ROUNDINGS = 4 roundings of numbers no larger than the same expression of |x|
    (all weights are positive), so a staged value is within 4 u x' of exact with x' = upsample(|x|),
    and through the conv that costs 4 u sum x'|w|: (K + 2 + 4) u S with S = sum x'|w| + |b|.  An fma
    in the expansion only removes roundings.  leaky does not grow an error; the pool is
    exact_ref.pool_bound."""
    xin = up64(x, align_corners) if up else x.double()
    xabs = up64(x.abs()) if up else x.double().abs()
    pre = F.conv2d(xin, wt.double(), b.double(), padding=1)
    s = F.conv2d(xabs, wt.double().abs(), b.double().abs(), padding=1).numpy()
    k = 9 * x.shape[1]
    bnd = (k + 2 + (UP_ROUNDINGS if up else 0)) * U * s
    ref = (pre if epi == LINEAR else leaky64(pre)).numpy()
    if epi != POOL:
        return ref, None, bnd, None, s
    refp = E.pool64(ref)
    return ref, refp, bnd, E.pool_bound("R32", bnd, ref, refp), s


def up_emulate(x):
    """The kernel's expansion in numpy fp32, every product and sum rounded on its own (no fma):
    horizontal first, then vertical, border by clamped reads."""
    f = np.float32
    x = x.numpy().astype(f)
    q, t = f(0.25), f(0.75)

    def axis(a, ax):
        a = np.moveaxis(a, ax, -1)
        prev = np.concatenate([a[..., :1], a[..., :-1]], -1)
        nxt = np.concatenate([a[..., 1:], a[..., -1:]], -1)
        out = np.empty(a.shape[:-1] + (2 * a.shape[-1],), f)
        out[..., 0::2] = ((q * prev).astype(f) + (t * a).astype(f)).astype(f)
        out[..., 1::2] = ((t * a).astype(f) + (q * nxt).astype(f)).astype(f)
        return np.moveaxis(out, -1, ax)
    return axis(axis(x, 3), 2)


def conv_emulate(xin, wt, b):
    """Direct form at fp32 in the kernel's K order: channel pairs, taps, one rounding per product
    entering the accumulator (the MFMA's fma chain), then the bias."""
    f = np.float32
    n, cin, h, w = xin.shape
    xp = np.zeros((n, cin, h + 2, w + 2), f)
    xp[:, :, 1:-1, 1:-1] = xin
    wn = wt.numpy().astype(f)
    acc = np.zeros((n, wn.shape[0], h, w), np.float64)
    for c in range(cin):
        for tap in range(9):
            ky, kx = divmod(tap, 3)
            prod = wn[None, :, c, ky, kx, None, None].astype(np.float64) * xp[:, None, c, ky:ky + h, kx:kx + w].astype(np.float64)
            acc = (acc + prod).astype(f).astype(np.float64)      # one rounding: fma
    return (acc.astype(f) + b.numpy().astype(f)[None, :, None, None]).astype(f).astype(np.float64)


# ---- rrin_warp_fwd --------------------------------------------------------------------------------------
# The reference's grid is 2 ((gx + u) / W - 0.5) under align_corners=False, which un-normalises to
# gx + u - 0.5: zero flow samples half a pixel up and left (four taps of weight 1/4), and the flows that
# land on one tap with weights exactly 1, 0, 0, 0 are the integers plus one half.  The kernel restates
# that arithmetic; "aligned" below means such a flow.
WARP_SIZES = [(1, 1), (1, 33), (33, 1), (16, 32), (17, 50)]
NONFINITE = (float("inf"), float("-inf"), float("nan"))
ZERO, ALIGNED, FINITE, HUGE, BAD = range(5)


def warp_flow(n, h, w):
    """One [n, 2, h, w] field holding, pixel after pixel: zero; aligned flows onto taps inside the
    frame (the shifted image) and onto taps outside it; integers, inside and pointing outside;
    flows 2^-20 on either side of a tap; flows around the four frame corners; +-1e9; +-inf and NaN
    (in u, in v, in both).  Returns (flow, kind [n, h, w])."""
    flow = torch.zeros(n, 2, h, w)
    kind = torch.zeros(n, h, w, dtype=torch.int64)
    e = 2.0 ** -20
    corners = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    k = 0
    for i in range(n):
        for y in range(h):
            for x in range(w):
                s, k = k % 23, k + 1
                if s == 0:
                    u, v, kd = 0.0, 0.0, ZERO
                elif s < 5:      # aligned, inside: tap (ty, tx)
                    tx, ty = (x * 7 + 3 * s + i) % w, (y * 5 + s) % h
                    u, v, kd = tx - x + 0.5, ty - y + 0.5, ALIGNED
                elif s < 8:      # aligned, outside: left of the frame, right of and below it, further out
                    u, v = [(-x - 0.5, 0.5), (w - x + 0.5, h - y + 0.5), (-x - 2.5, -y - 1.5)][s - 5]
                    kd = ALIGNED
                elif s < 10:     # integers: every tap has weight 1/4, some outside near the border
                    (u, v), kd = ((1.0, -2.0) if s == 8 else (float(-x), float(h - 1 - y))), FINITE
                elif s < 12:
                    (u, v), kd = ((1.5 + e, 0.5 - e) if s == 10 else (0.5 - e, -0.5 + e)), FINITE
                elif s < 16:
                    cy, cx = corners[s - 12]
                    u, v, kd = cx - x + 0.25, cy - y + 0.75, FINITE
                elif s < 18:
                    (u, v), kd = ((1e9, -1e9) if s == 16 else (-1e9, 1e9)), HUGE
                else:
                    bad = NONFINITE[(s - 18) % 3]
                    u, v = [(bad, 0.5), (0.5, bad), (bad, bad), (bad, 1.0), (1.0, bad)][s - 18]
                    kd = BAD
                flow[i, 0, y, x], flow[i, 1, y, x], kind[i, y, x] = u, v, kd
    return flow, kind


@functools.lru_cache(maxsize=None)
def warp_case(n, c, h, w):
    g = torch.Generator().manual_seed(1000 * h + 10 * w + c)
    img = torch.rand(n, c, h, w, generator=g)
    flow, kind = warp_flow(n, h, w)
    return img, flow, kind


def coord32(g, u, size):
    """ix of common.hpp warp_taps in numpy fp32, each step rounded: (2 ((g + u) / W - 0.5) + 1) (W / 2) - 0.5."""
    f = np.float32
    x = (g.astype(f) + u.astype(f)).astype(f)
    nx = (f(2) * ((x / f(size)).astype(f) - f(0.5)).astype(f)).astype(f)
    return (((nx + f(1)).astype(f) * (f(size) / f(2))).astype(f) - f(0.5)).astype(f)


def shifted(img, flow, kind):
    """(value, exact, inside).  inside: aligned flows whose tap lies in the frame; value: the image at
    that tap; exact: where also the fp32 coordinate arithmetic of warp_taps lands on the tap exactly
    (weights exactly 1, 0, 0, 0), so that the kernel's output must be the image at the tap bit for bit."""
    n, c, h, w = img.shape
    gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    u, v = flow[:, 0].numpy(), flow[:, 1].numpy()
    with np.errstate(invalid="ignore", over="ignore"):
        tx, ty = gx[None] + u - 0.5, gy[None] + v - 0.5
        inside = (kind.numpy() == ALIGNED) & (tx >= 0) & (tx <= w - 1) & (ty >= 0) & (ty <= h - 1)
        exact = (coord32(np.broadcast_to(gx[None], u.shape), u, w) == tx) & (coord32(np.broadcast_to(gy[None], v.shape), v, h) == ty)
    txi, tyi = np.where(inside, tx, 0).astype(np.int64), np.where(inside, ty, 0).astype(np.int64)
    val = img.numpy()[np.arange(n)[:, None, None, None], np.arange(c)[None, :, None, None], tyi[:, None], txi[:, None]]
    return torch.from_numpy(val), torch.from_numpy(inside & exact), torch.from_numpy(inside)
