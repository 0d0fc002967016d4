"""References for the per-kernel tests of csrc/train.hip (tests/test_gpu_train_kernels.py), in
plain numpy: no GPU, no torch operator.  tests/test_train_ref.py pins them to PyTorch-CPU
autograd in double.

Convolutions (3x3, pad 1, NCHW) come in two forms:
  * float64: the value and, next to it, the same sum over absolute values S = sum |a_i b_i|
    (+ |bias| for the forward).  An fp32 sum of K exactly formed products plus a bias is within
    (K + 2) 2^-24 S of the float64 value, whatever its order: the bound of the GPU tests.
  * exact integer (int64) for integer-valued inputs: any fp32 summation order whose partial sums
    stay below 2^24 gives these values bit for bit.
The leaky backward takes its mask from the forward output y: g' = g * (y > 0 ? 1 : slope).  In
the integer form the slope is 1 / slope_inv (a power of two keeps fp32 exact) and the result is
scaled by slope_inv, so it stays an integer.

warp_bwd is the backward of warp (grid_sample, bilinear, zeros): tap positions, validity and
weights by an fp32 twin of warp_taps (common.hpp), the flow gradient in float64 from those taps,
the image gradient as the bit-exact model of the device's 64-bit fixed-point scatter."""
import numpy as np

F32 = np.float32
SLOPE32 = F32(0.1)
U24 = 2.0 ** -24


def _shift(x, ky, kx):
    """x[..., y + ky - 1, x + kx - 1], zero outside."""
    h, w = x.shape[-2:]
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    return xp[:, :, ky:ky + h, kx:kx + w]


def _mask(g, y, slope):
    return g if y is None else g * np.where(y > 0, 1.0, float(slope))


def _imask(g, y, slope_inv):
    g = g.astype(np.int64)
    return g if y is None else g * np.where(y > 0, int(slope_inv), 1)


def _fwd(x, w, b):
    y = np.zeros((x.shape[0], w.shape[0]) + x.shape[2:], x.dtype)
    for ky in range(3):
        for kx in range(3):
            y += np.einsum("oc,nchw->nohw", w[:, :, ky, kx], _shift(x, ky, kx))
    return y if b is None else y + b[None, :, None, None]


def _dgrad(g, w):
    gx = np.zeros((g.shape[0], w.shape[1]) + g.shape[2:], g.dtype)
    for ky in range(3):
        for kx in range(3):
            gx += np.einsum("oc,nohw->nchw", w[:, :, ky, kx], _shift(g, 2 - ky, 2 - kx))
    return gx


def _wgrad(x, g):
    gw = np.zeros((g.shape[1], x.shape[1], 3, 3), g.dtype)
    for ky in range(3):
        for kx in range(3):
            gw[:, :, ky, kx] = np.einsum("nohw,nchw->oc", g, _shift(x, ky, kx))
    return gw, g.sum((0, 2, 3))


def _f64(*a):
    return [None if t is None else np.asarray(t, np.float64) for t in a]


def _i64(*a):
    out = []
    for t in a:
        if t is not None:
            t = np.asarray(t)
            assert np.array_equal(t, np.rint(t)), "integer form: integer-valued inputs only"
            t = t.astype(np.int64)
        out.append(t)
    return out


def conv_fwd(x, w, b=None):
    """(y, S) in float64, before any activation."""
    x, w, b = _f64(x, w, b)
    return _fwd(x, w, b), _fwd(np.abs(x), np.abs(w), None if b is None else np.abs(b))


def conv_fwd_int(x, w, b=None):
    return _fwd(*_i64(x, w, b))


def conv_dgrad(g, w, y=None, slope=SLOPE32):
    """(gx, S): the input gradient of conv_fwd for the output gradient g."""
    g, w = _f64(g, w)
    g = _mask(g, y, slope)
    return _dgrad(g, w), _dgrad(np.abs(g), np.abs(w))


def conv_dgrad_int(g, w, y=None, slope_inv=1):
    """slope_inv * gx, exact (slope = 1 / slope_inv)."""
    g, w = _i64(g, w)
    return _dgrad(_imask(g, y, slope_inv), w)


def conv_wgrad(x, g, y=None, slope=SLOPE32):
    """(gw, gb, S_gw, S_gb)."""
    x, g = _f64(x, g)
    g = _mask(g, y, slope)
    gw, gb = _wgrad(x, g)
    sw, sb = _wgrad(np.abs(x), np.abs(g))
    return gw, gb, sw, sb


def conv_wgrad_int(x, g, y=None, slope_inv=1):
    """(slope_inv * gw, slope_inv * gb), exact."""
    x, g = _i64(x, g)
    return _wgrad(x, _imask(g, y, slope_inv))


def leaky_f32(v, slope=SLOPE32):
    """The forward epilogue in fp32: v > 0 ? v : fl32(v * fl32(slope))."""
    v = np.asarray(v).astype(F32)
    return np.where(v > 0, v, (v * F32(slope)).astype(F32)).astype(F32)


# ---- avg_pool2d(2) and Upsample(x2, bilinear, align_corners=False) -------------------------------
def pool2_fwd(x):
    """y = 0.25 (((x00 + x01) + x10) + x11)."""
    x = np.asarray(x, np.float64)
    return (((x[..., 0::2, 0::2] + x[..., 0::2, 1::2]) + x[..., 1::2, 0::2]) + x[..., 1::2, 1::2]) * 0.25


def pool2_fwd_f32(x):
    """The same expression with every operation in fp32: the kernel's bits."""
    x = np.asarray(x, F32)
    return (((x[..., 0::2, 0::2] + x[..., 0::2, 1::2]) + x[..., 1::2, 0::2]) + x[..., 1::2, 1::2]) * F32(0.25)


def pool2_bwd(gy):
    gy = np.asarray(gy, np.float64)
    return np.repeat(np.repeat(gy, 2, -2), 2, -1) * 0.25


def up_taps(o, n):
    """Output o of a line of n inputs reads i0 = floor(s), i1 = min(i0 + 1, n - 1) with
    s = max((o + .5) / 2 - .5, 0), weights 1 - l and l = s - i0.  In fp32, exact for these
    arguments (quarters below 2^22)."""
    s = (F32(o) + F32(0.5)) * F32(0.5) - F32(0.5)
    if s < 0:
        s = F32(0)
    i0 = int(s)
    i1 = min(i0 + 1, n - 1)
    return i0, i1, float(s - F32(i0))


def up_matrix(n):
    """[2n][n]: the line operator of up_taps (both taps may be the same input at the edge)."""
    m = np.zeros((2 * n, n))
    for o in range(2 * n):
        i0, i1, l = up_taps(o, n)
        m[o, i0] += 1.0 - l
        m[o, i1] += l
    return m


def up2_fwd(x):
    x = np.asarray(x, np.float64)
    return np.einsum("oy,...yx,px->...op", up_matrix(x.shape[-2]), x, up_matrix(x.shape[-1]))


def up2_bwd(gy):
    gy = np.asarray(gy, np.float64)
    return np.einsum("oy,...op,px->...yx", up_matrix(gy.shape[-2] // 2), gy, up_matrix(gy.shape[-1] // 2))


# ---- warp backward ---------------------------------------------------------------------------
def warp_taps32(flow):
    """fp32 twin of warp_taps (common.hpp) for every pixel of flow [n][2][h][w]: the same
    operations in the same order, each rounded to fp32, nothing contracted."""
    flow = np.asarray(flow, F32)
    n, _, h, w = flow.shape
    gy, gx = np.meshgrid(np.arange(h, dtype=F32), np.arange(w, dtype=F32), indexing="ij")
    W, H = F32(w), F32(h)
    with np.errstate(over="ignore", invalid="ignore"):
        x = gx[None] + flow[:, 0]
        y = gy[None] + flow[:, 1]
        nx = F32(2) * (x / W - F32(0.5))
        ny = F32(2) * (y / H - F32(0.5))
        ix = (nx + F32(1)) * (W / F32(2)) - F32(0.5)
        iy = (ny + F32(1)) * (H / F32(2)) - F32(0.5)
        fx, fy = np.floor(ix), np.floor(iy)
        we = ix - fx
        e = F32(1) - we
        nn = iy - fy
        s = F32(1) - nn
    t = {"wx": we, "wy": nn, "e": e, "s": s, "nw": s * e, "ne": s * we, "sw": nn * e, "se": nn * we}
    assert all(v.dtype == F32 for v in t.values())
    t["vx0"] = (fx >= 0) & (fx <= F32(w - 1))
    t["vx1"] = (fx >= -1) & (fx <= F32(w - 2))
    t["vy0"] = (fy >= 0) & (fy <= F32(h - 1))
    t["vy1"] = (fy >= -1) & (fy <= F32(h - 2))
    t["x0"] = np.where(t["vx0"] | t["vx1"], fx, 0).astype(np.int64)
    t["y0"] = np.where(t["vy0"] | t["vy1"], fy, 0).astype(np.int64)
    return t


def fx_scale(gout, hw):
    """The device's fixed-point scale: 2^min(62 - hb - e, 126) with max|gout| = f 2^e,
    f in [0.5, 1), hb = ceil(log2(h w)); 1 for a zero gradient.  Returns the exponent."""
    m = F32(np.abs(np.asarray(gout, F32)).max())
    if not m > 0:
        return 0
    e = int(np.frexp(m)[1])
    hb = 0
    while (1 << hb) < hw:
        hb += 1
    return min(62 - hb - e, 126)


def warp_bwd(img, flow, gout):
    """(gimg fp32: the device's bits; gflow float64; S of gflow)."""
    img, gout = np.asarray(img, F32), np.asarray(gout, F32)
    n, c, h, w = img.shape
    t = warp_taps32(flow)
    sc = 2.0 ** fx_scale(gout, h * w)
    corners = [(0, 0, t["vy0"] & t["vx0"], t["nw"]), (0, 1, t["vy0"] & t["vx1"], t["ne"]),
               (1, 0, t["vy1"] & t["vx0"], t["sw"]), (1, 1, t["vy1"] & t["vx1"], t["se"])]
    acc = np.zeros((n, c, h, w), np.int64)
    ni, ci = np.arange(n)[:, None, None, None], np.arange(c)[None, :, None, None]
    val = []
    for dy, dx, ok, wgt in corners:
        yy, xx = (t["y0"] + dy)[:, None], (t["x0"] + dx)[:, None]
        use = np.broadcast_to((ok & (wgt != 0))[:, None], acc.shape)
        p = gout * wgt[:, None]                      # fl32(go * wgt)
        assert p.dtype == F32
        q = np.rint(p.astype(np.float64) * sc)       # exact product, ties to even
        q = np.where(use, q, 0.0).astype(np.int64)
        np.add.at(acc, (np.broadcast_to(ni, acc.shape)[use], np.broadcast_to(ci, acc.shape)[use],
                        np.broadcast_to(yy, acc.shape)[use], np.broadcast_to(xx, acc.shape)[use]), q[use])
        okc = np.broadcast_to(ok[:, None], acc.shape)
        v = np.zeros(acc.shape)
        v[okc] = img[np.broadcast_to(ni, acc.shape)[okc], np.broadcast_to(ci, acc.shape)[okc],
                     np.broadcast_to(yy, acc.shape)[okc], np.broadcast_to(xx, acc.shape)[okc]]
        val.append(v)
    gimg = (acc.astype(np.float64) / sc).astype(F32)
    a, b, cc, d = val
    go = gout.astype(np.float64)
    s_, n_, e_, w_ = (t[k].astype(np.float64)[:, None] for k in ("s", "wy", "e", "wx"))
    kx = float(F32(w) / F32(2)) * float(F32(2) / F32(w))
    ky = float(F32(h) / F32(2)) * float(F32(2) / F32(h))
    gix = (go * ((b - a) * s_ + (d - cc) * n_)).sum(1) * kx
    giy = (go * ((cc - a) * e_ + (d - b) * w_)).sum(1) * ky
    six = (np.abs(go) * (np.abs(b - a) * s_ + np.abs(d - cc) * n_)).sum(1) * kx
    siy = (np.abs(go) * (np.abs(cc - a) * e_ + np.abs(d - b) * w_)).sum(1) * ky
    return gimg, np.stack((gix, giy), 1), np.stack((six, siy), 1)
