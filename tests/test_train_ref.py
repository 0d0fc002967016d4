"""CPU: pin tests/train_ref.py (the references of tests/test_gpu_train_kernels.py) to PyTorch-CPU
autograd in double precision."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_ref as R


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _conv_case(seed, n, cin, cout, h, w, integer=False):
    r = np.random.default_rng(seed)
    if integer:
        return [r.integers(-4, 5, s).astype(np.float64) for s in
                ((n, cin, h, w), (cout, cin, 3, 3), (cout,), (n, cout, h, w))]
    return [r.standard_normal(s) for s in ((n, cin, h, w), (cout, cin, 3, 3), (cout,), (n, cout, h, w))]


@pytest.mark.parametrize("shape", [(2, 3, 5, 4, 6), (1, 1, 1, 1, 1), (2, 7, 2, 1, 9), (1, 2, 3, 6, 1)])
@pytest.mark.parametrize("leaky", [False, True])
def test_float64_convs_match_conv2d_autograd(shape, leaky):
    """conv_fwd / conv_dgrad / conv_wgrad against F.conv2d (+ leaky_relu) autograd in double.
    Both are float64 sums of the same terms in different orders: within 1e-13 of S."""
    x, w, b, g = _conv_case(sum(shape), *shape)
    xt, wt, bt = (_t(a).requires_grad_() for a in (x, w, b))
    yt = F.conv2d(xt, wt, bt, padding=1)
    pre = yt.detach().numpy()
    if leaky:
        yt = F.leaky_relu(yt, float(R.SLOPE32))
    yt.backward(_t(g))
    y, s = R.conv_fwd(x, w, b)
    assert np.all(np.abs(y - pre) <= 1e-13 * s)
    assert np.all(s >= np.abs(y) * (1 - 1e-13))
    yf = pre if leaky else None
    gx, sx = R.conv_dgrad(g, w, yf)
    assert np.all(np.abs(gx - xt.grad.numpy()) <= 1e-13 * sx + 1e-300)
    gw, gb, sw, sb = R.conv_wgrad(x, g, yf)
    assert np.all(np.abs(gw - wt.grad.numpy()) <= 1e-13 * sw + 1e-300)
    assert np.all(np.abs(gb - bt.grad.numpy()) <= 1e-13 * sb)


@pytest.mark.parametrize("shape", [(2, 3, 5, 4, 6), (1, 17, 2, 3, 3)])
def test_integer_convs_are_the_float64_convs(shape):
    """On integer data the float64 form is exact too (|sum| far below 2^53), so the two forms are
    equal; with a mask taken from the integer y (many exact zeros) and slope 1/4 the integer form
    is 4 x the float64 one."""
    x, w, b, g = _conv_case(sum(shape) + 1, *shape, integer=True)
    y = R.conv_fwd_int(x, w, b)
    assert y.dtype == np.int64 and np.array_equal(y, R.conv_fwd(x, w, b)[0])
    assert np.array_equal(R.conv_fwd_int(x, w), R.conv_fwd(x, w)[0])
    y.flat[::5] = 0      # exact zeros take the slope side of the mask
    assert np.array_equal(R.conv_dgrad_int(g, w), R.conv_dgrad(g, w)[0])
    assert np.array_equal(R.conv_dgrad_int(g, w, y, 4), 4 * R.conv_dgrad(g, w, y, 0.25)[0])
    gw, gb = R.conv_wgrad_int(x, g)
    rw, rb, _, _ = R.conv_wgrad(x, g)
    assert np.array_equal(gw, rw) and np.array_equal(gb, rb)
    gw, gb = R.conv_wgrad_int(x, g, y, 4)
    rw, rb, _, _ = R.conv_wgrad(x, g, y, 0.25)
    assert np.array_equal(gw, 4 * rw) and np.array_equal(gb, 4 * rb)
    with pytest.raises(AssertionError):
        R.conv_fwd_int(x + 0.5, w)


def test_leaky_f32():
    v = np.array([-3.0, -0.0, 0.0, 2.5, -1e-3], np.float32)
    out = R.leaky_f32(v)
    assert out.dtype == np.float32
    assert np.array_equal(out, np.array([np.float32(-3.0) * np.float32(0.1), -0.0, 0.0, 2.5,
                                         np.float32(-1e-3) * np.float32(0.1)], np.float32))
    assert np.array_equal(R.leaky_f32(torch.tensor([-3.0, 2.0]).numpy()),
                          F.leaky_relu(torch.tensor([-3.0, 2.0]), 0.1).numpy())


@pytest.mark.parametrize("shape", [(1, 2, 2), (5, 6, 10), (3, 4, 258)])
def test_pool2_matches_avg_pool2d(shape):
    r = np.random.default_rng(shape[2])
    x, gy = r.standard_normal(shape), r.standard_normal((shape[0], shape[1] // 2, shape[2] // 2))
    xt = _t(x)[None].requires_grad_()
    yt = F.avg_pool2d(xt, 2)
    yt.backward(_t(gy)[None])
    assert np.abs(R.pool2_fwd(x) - yt.detach().numpy()[0]).max() <= 1e-15
    assert np.array_equal(R.pool2_bwd(gy), xt.grad.numpy()[0])
    x32 = x.astype(np.float32)
    assert R.pool2_fwd_f32(x32).dtype == np.float32
    assert np.abs(R.pool2_fwd_f32(x32) - R.pool2_fwd(x32)).max() <= 3 * R.U24 * 4 * np.abs(x32).max()


@pytest.mark.parametrize("shape", [(1, 1, 1), (4, 1, 3), (2, 5, 7), (1, 2, 130)])
def test_up2_matches_interpolate(shape):
    r = np.random.default_rng(shape[2])
    x, gy = r.standard_normal(shape), r.standard_normal((shape[0], 2 * shape[1], 2 * shape[2]))
    xt = _t(x)[None].requires_grad_()
    yt = F.interpolate(xt, scale_factor=2, mode="bilinear", align_corners=False)
    yt.backward(_t(gy)[None])
    assert np.abs(R.up2_fwd(x) - yt.detach().numpy()[0]).max() <= 1e-14
    assert np.abs(R.up2_bwd(gy) - xt.grad.numpy()[0]).max() <= 1e-14
    m = R.up_matrix(shape[2])
    assert set(np.unique(m)) <= {0.0, 0.25, 0.75, 1.0} and np.all(m.sum(1) == 1.0)


def _ref_warp64(img, flow):  # the reference's warp (model.py:8-21) in double
    n, _, h, w = img.shape
    gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    x = gx.unsqueeze(0) + flow[:, 0]
    y = gy.unsqueeze(0) + flow[:, 1]
    grid = torch.stack((2 * (x / w - 0.5), 2 * (y / h - 0.5)), dim=3)
    return F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)


def _off_integer(flow, margin=1e-3):
    """Move every sample whose position (x + u - 0.5, y + v - 0.5) is within margin of an integer."""
    flow = flow.astype(np.float64)
    h, w = flow.shape[2:]
    gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for k, g in ((0, gx), (1, gy)):
        p = g[None] + flow[:, k] - 0.5
        near = np.abs(p - np.rint(p)) < margin
        flow[:, k] += np.where(near, 0.01, 0.0)
    return flow.astype(np.float32)


@pytest.mark.parametrize("scale", [0.3, 40.0])
def test_warp_bwd_matches_grid_sample_autograd(scale):
    """The fp32-position twin against double-precision grid_sample autograd of the reference's
    warp, on flows that keep every sample >= 1e-3 px from an integer position (there the
    derivative is one-sided by convention).

    The twin's position carries 6 fp32 roundings of values up to P + W (P = max |x + u|), so
    d = 6 * 2^-24 * (P + W) px; a tap weight moves by at most 2 d (d per axis, to first order),
    the flow gradient's weights s, n, e, w by d.  Bounds, per element, with 3 * 2^-24 for the
    image gradient's own roundings (the product, the fixed-point ulp, the final fp32):
      gimg  <= (2 d + 3 * 2^-24) * A,  A = the sum of |go| over the taps that reach the pixel
      gflow <= d * sum_ch |go| (|b - a| + |d - c|)   (resp. |c - a| + |d - b|)
    Measured max deviation on 2x3x17x23 (the largest element bound in brackets): scale 0.3:
    gimg 3.2e-6 (2.9e-4), gflow 6.0e-6 (1.1e-4); scale 40: gimg 1.1e-6 (4.3e-4), gflow 1.3e-6
    (3.4e-4)."""
    r = np.random.default_rng(int(scale * 10))
    n, c, h, w = 2, 3, 17, 23
    img = r.random((n, c, h, w)).astype(np.float32)
    flow = _off_integer((r.standard_normal((n, 2, h, w)) * scale).astype(np.float32))
    go = r.standard_normal((n, c, h, w)).astype(np.float32)
    it, ft = _t(img).requires_grad_(), _t(flow).requires_grad_()
    _ref_warp64(it, ft).backward(_t(go))
    gimg, gflow, _ = R.warp_bwd(img, flow, go)
    gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    P = max(np.abs(gx[None] + flow[:, 0]).max(), np.abs(gy[None] + flow[:, 1]).max())
    d = 6 * R.U24 * (P + max(h, w))
    assert d < 1e-3
    # A: unit-weight scatter of |go|; the flow bound: the twin on |differences| with unit weights
    t = R.warp_taps32(flow)
    A = np.zeros((n, c, h, w))
    B = np.zeros((n, 2, h, w))
    px = np.zeros((4, n, c, h, w))
    for k, (dy, dx, ok) in enumerate(((0, 0, t["vy0"] & t["vx0"]), (0, 1, t["vy0"] & t["vx1"]),
                                      (1, 0, t["vy1"] & t["vx0"]), (1, 1, t["vy1"] & t["vx1"]))):
        for i in range(n):
            for ch in range(c):
                yy, xx = t["y0"][i][ok[i]] + dy, t["x0"][i][ok[i]] + dx
                np.add.at(A[i, ch], (yy, xx), np.abs(go[i, ch][ok[i]]))
                px[k, i, ch][ok[i]] = img[i, ch][yy, xx]
    a, b, cc, dd = px
    B[:, 0] = (np.abs(go) * (np.abs(b - a) + np.abs(dd - cc))).sum(1)
    B[:, 1] = (np.abs(go) * (np.abs(cc - a) + np.abs(dd - b))).sum(1)
    ei = np.abs(gimg.astype(np.float64) - it.grad.numpy())
    ef = np.abs(gflow - ft.grad.numpy())
    print(f"scale {scale}: gimg max dev {ei.max():.2e} (bound >= {((2 * d + 3 * R.U24) * A).max():.2e}), "
          f"gflow {ef.max():.2e} ({(d * B).max():.2e})")
    assert np.all(ei <= (2 * d + 3 * R.U24) * A + 1e-30), float((ei - (2 * d + 3 * R.U24) * A).max())
    assert np.all(ef <= d * B + 1e-30), float((ef - d * B).max())


def test_warp_taps_convention_at_integer_positions():
    """At an integer sample position the twin takes floor: the whole weight on the north-west
    tap, the other three exactly zero (they then add nothing to the image gradient), and the
    flow gradient is the derivative to the right / below.  On 8 x 16 (powers of two: the
    position arithmetic is exact) with flows of k + 0.5 (the reference's warp samples pixel
    x + u - 0.5)."""
    h, w = 8, 16
    r = np.random.default_rng(0)
    k = r.integers(-3, 4, (1, 2, h, w))
    flow = (k + 0.5).astype(np.float32)
    t = R.warp_taps32(flow)
    gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    assert np.all(t["wx"] == 0) and np.all(t["wy"] == 0)
    assert np.all(t["nw"] == 1) and np.all(t["ne"] == 0) and np.all(t["sw"] == 0) and np.all(t["se"] == 0)
    inx = (gx + k[:, 0] >= 0) & (gx + k[:, 0] < w)
    iny = (gy + k[:, 1] >= 0) & (gy + k[:, 1] < h)
    assert np.array_equal(t["vx0"], inx) and np.array_equal(t["vy0"], iny)
    assert np.array_equal(t["x0"][inx], (gx + k[:, 0])[inx]) and np.array_equal(t["y0"][iny], (gy + k[:, 1])[iny])
    # gimg: go lands whole on pixel (y + ky, x + kx); gflow: the forward difference there
    img = r.integers(-4, 5, (1, 1, h, w)).astype(np.float32)
    go = np.ones((1, 1, h, w), np.float32)
    gimg, gflow, _ = R.warp_bwd(img, flow, go)
    cnt = np.zeros((h, w))
    np.add.at(cnt, ((gy + k[0, 1])[inx[0] & iny[0]], (gx + k[0, 0])[inx[0] & iny[0]]), 1.0)
    assert np.array_equal(gimg[0, 0], cnt.astype(np.float32))
    ip = np.pad(img[0, 0].astype(np.float64), ((4, 4), (4, 4)))
    yy, xx = gy + k[0, 1] + 4, gx + k[0, 0] + 4
    assert np.array_equal(gflow[0, 0], ip[yy, xx + 1] - ip[yy, xx])
    assert np.array_equal(gflow[0, 1], ip[yy + 1, xx] - ip[yy, xx])


def test_fx_scale_model():
    assert R.fx_scale(np.zeros(4, np.float32), 64) == 0
    assert R.fx_scale(np.array([0.999], np.float32), 64 * 64) == 62 - 12 - 0
    assert R.fx_scale(np.array([1.0], np.float32), 17 * 23) == 62 - 9 - 1     # ceil(log2 391) = 9
    assert R.fx_scale(np.array([2.0 ** -100], np.float32), 1) == 126          # capped
