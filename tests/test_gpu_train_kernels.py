"""The training kernels of csrc/train.hip one by one through the C ABI (tests/hip_helpers.py),
against the references of tests/train_ref.py (pinned on the CPU by tests/test_train_ref.py).

Every tolerance is equality or k * 2^-24 * S with S the sum of the absolute values of the terms
(the forward error bound of an fp32 sum of k operations); every output starts as NaN.

Integer data: x, w, b, g in [-4, 4] make every product and partial sum an exact fp32 integer
(|sum| <= 16 K < 2^24 at these shapes), so any summation order gives the int64 reference bit for
bit.  The leaky backward on integer data runs with slope 1/4 (the entry takes any slope in
(0, 1]): g' then stays a multiple of 1/4 and 4 x the result is the integer reference; slope 0.1
is covered by the random-float cases, the forward epilogue and the autograd tests."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rrin_amd import Net
from rrin_amd import autograd as ag
from rrin_amd.synthetic import keyed_state_dict, synthetic_batch
from tests import hip_helpers as H
from tests import train_ref as R

pytestmark = pytest.mark.gpu

U = R.U24


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)


def _ints(seed, *shapes):
    r = np.random.default_rng(seed)
    return [r.integers(-4, 5, s).astype(np.float32) for s in shapes]


def _int_y(x, w, b):
    """The integer forward output as the leaky mask's y, every 5th element forced to an exact 0
    (zero is on the slope side of y > 0)."""
    y = R.conv_fwd_int(x, w, b)
    y.flat[::5] = 0
    return y


def _eq(got, ref):
    got = got.cpu().numpy()
    assert got.shape == ref.shape
    bad = np.flatnonzero(~(got.astype(np.float64).ravel() == np.asarray(ref, np.float64).ravel()))
    assert bad.size == 0, (bad.size, bad[:8], got.ravel()[bad[:8]], np.asarray(ref).ravel()[bad[:8]])


def _within(got, ref, s, k, what):
    """|got - ref| <= k 2^-24 S per element; returns the largest err / (2^-24 S)."""
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), what
    err = np.abs(got - ref)
    ok = err <= k * U * s
    ratio = float((err / np.maximum(U * s, 1e-300))[s > 0].max()) if np.any(s > 0) else 0.0
    print(f"{what}: max err / (2^-24 S) = {ratio:.2f} of {k}")
    assert np.all(ok), (what, int((~ok).sum()), ratio, k)
    return ratio


# (n, cin, cout, h, w) around the 64 (M) x 64 (N) x 16 (K) tile of tconv3x3_kernel
TC_SHAPES = [(1, 1, 1, 1, 1),      # one pixel
             (2, 1, 4, 1, 7),      # K = 9 < one K step
             (1, 16, 64, 8, 8),    # K a multiple of 16, N = 64
             (3, 7, 65, 7, 9),     # K = 63, N = 63, a second M tile
             (1, 70, 130, 5, 13),  # N = 65, a third M tile
             (2, 33, 3, 1, 64)]    # a single row
TC_SHAPES_T = sorted(set(TC_SHAPES + [(n, co, ci, h, w) for n, ci, co, h, w in TC_SHAPES]))


@pytest.mark.parametrize("shape", TC_SHAPES)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("leaky", [False, True])
def test_tconv3x3_fwd_integer_exact(gpu, shape, bias, leaky):
    """(a) rrin_tconv3x3 FWD equals the int64 sum; with leaky, leaky_f32 (slope fl32(0.1)) of it."""
    n, cin, cout, h, w = shape
    x, wt, b = _ints(sum(shape), (n, cin, h, w), (cout, cin, 3, 3), (cout,))
    ref = R.conv_fwd_int(x, wt, b if bias else None)
    assert np.abs(ref).max() < 2 ** 24
    out = H.tconv(_dev(x, gpu), _dev(wt, gpu), _dev(b, gpu) if bias else None, leaky=leaky)
    _eq(out, R.leaky_f32(ref) if leaky else ref.astype(np.float32))


@pytest.mark.parametrize("shape", TC_SHAPES_T)
@pytest.mark.parametrize("leaky", [False, True])
def test_tconv3x3_dgrad_integer_exact(gpu, shape, leaky):
    """(a) rrin_tconv3x3 DGRAD (M = cin: the shapes and their cin <-> cout transposes) equals the
    int64 sum over the flipped, transposed weights; with leaky the mask comes from the integer y
    with its exact zeros, slope 1/4."""
    n, cin, cout, h, w = shape
    x, wt, b, g = _ints(sum(shape) + 1, (n, cin, h, w), (cout, cin, 3, 3), (cout,), (n, cout, h, w))
    y = _int_y(x, wt, b) if leaky else None
    ref = R.conv_dgrad_int(g, wt, y, 4)
    out = H.tconv(_dev(g, gpu), _dev(wt, gpu), dgrad=True, leaky=leaky, slope=0.25,
                  y=_dev(y, gpu) if leaky else None)
    _eq(out * (4.0 if leaky else 1.0), ref)
    if not leaky:   # without a mask the result is the plain integer sum
        _eq(out, R.conv_dgrad_int(g, wt))


@pytest.mark.parametrize("shape", [(3, 7, 65, 7, 9), (1, 70, 130, 5, 13)])
def test_tconv3x3_random_floats(gpu, shape):
    """(b) randn data: per element |out - ref64| <= (K + 2) 2^-24 S, K = 9 cin (FWD, with bias)
    resp. 9 cout (DGRAD, leaky with slope fl32(0.1) and a random y): the forward bound of an fp32
    sum of K exactly formed products plus a bias (the mask's product is one more rounding).
    Observed max err / (2^-24 S) on MI355X: FWD 3.54 (K + 2 = 65), 3.04 (632); DGRAD 3.91 (587),
    3.63 (1172)."""
    n, cin, cout, h, w = shape
    r = np.random.default_rng(cin)
    x, wt, b, g, y = (r.standard_normal(s).astype(np.float32) for s in
                      ((n, cin, h, w), (cout, cin, 3, 3), (cout,), (n, cout, h, w), (n, cout, h, w)))
    ref, s = R.conv_fwd(x, wt, b)
    _within(H.tconv(_dev(x, gpu), _dev(wt, gpu), _dev(b, gpu)), ref, s, 9 * cin + 2, f"fwd {shape}")
    ref, s = R.conv_dgrad(g, wt, y)
    out = H.tconv(_dev(g, gpu), _dev(wt, gpu), dgrad=True, leaky=True, y=_dev(y, gpu))
    _within(out, ref, s, 9 * cout + 2, f"dgrad {shape}")


def _wgrad_int(gpu, shape):
    n, cin, cout, h, w = shape
    assert 16 * n * h * w < 2 ** 24
    x, g = _ints(sum(shape) + 2, (n, cin, h, w), (n, cout, h, w))
    gw, gb = H.twgrad(_dev(x, gpu), _dev(g, gpu))
    rw, rb = R.conv_wgrad_int(x, g)
    _eq(gw, rw)
    _eq(gb, rb)


@pytest.mark.parametrize("w", [1, 3, 63, 64, 65, 68, 130])
@pytest.mark.parametrize("h", [1, 5])
def test_twgrad_widths_integer_exact(gpu, h, w):
    """(c) the 64-pixel row chunks: one partial chunk, one full, a second chunk, w % 4 != 0 (the
    scalar staging path) and w % 4 == 0 (float4)."""
    _wgrad_int(gpu, (2, 5, 7, h, w))


@pytest.mark.parametrize("cin,cout", [(1, 1), (31, 33), (32, 64), (33, 64), (65, 96), (16, 128)])
def test_twgrad_channel_edges_integer_exact(gpu, cin, cout):
    """(c) CT = 1 and CT = 2 (cout % 64 == 0), one and several ci / co tiles, zero-filled tails."""
    _wgrad_int(gpu, (2, cin, cout, 6, 12))


@pytest.mark.parametrize("shape", [(1, 65, 96, 151, 5),   # 76 slices of 2 rows, the last with 1
                                   (3, 65, 96, 50, 8)])   # 75 full slices across image boundaries
def test_twgrad_slices_integer_exact(gpu, shape):
    _wgrad_int(gpu, shape)


@pytest.mark.parametrize("shape", [(2, 33, 64, 5, 12),    # w % 4 == 0 (float4), CT = 2
                                   (2, 5, 7, 5, 13),      # w % 4 != 0 (scalar), CT = 1
                                   (1, 5, 7, 3, 68),      # w > 64, float4
                                   (1, 16, 128, 3, 70)])  # w > 64, scalar, CT = 2
def test_twgrad_fused_leaky_integer_exact(gpu, shape):
    """(c) the fused leaky backward of the weight gradient (slope 1/4, integer y with exact
    zeros): leaky=1 and leaky=0 on the test's own pre-masked g' are bitwise equal and 4 x them
    is the integer reference; gb == NULL leaves gw unchanged."""
    n, cin, cout, h, w = shape
    x, wt, b, g = _ints(sum(shape) + 3, (n, cin, h, w), (cout, cin, 3, 3), (cout,), (n, cout, h, w))
    y = _int_y(x, wt, b)
    assert (y == 0).sum() > y.size // 6
    xd, gd, yd = _dev(x, gpu), _dev(g, gpu), _dev(y, gpu)
    gw1, gb1 = H.twgrad(xd, gd, y=yd, leaky=True, slope=0.25)
    gp = torch.where(yd > 0, gd, gd * 0.25)
    gw2, gb2 = H.twgrad(xd, gp)
    gw3, gb3 = H.twgrad(xd, gd, y=yd, leaky=True, slope=0.25, bias_grad=False)
    rw, rb = R.conv_wgrad_int(x, g, y, 4)
    _eq(gw1 * 4.0, rw)
    _eq(gb1 * 4.0, rb)
    assert torch.equal(gw1, gw2) and torch.equal(gb1, gb2)
    assert gb3 is None and torch.equal(gw1, gw3)
    # the mask matters here: the unmasked gradient differs
    assert not np.array_equal(R.conv_wgrad_int(x, g)[0] * 4, rw)


def test_twgrad_random_floats(gpu):
    """(c) randn data, leaky with slope fl32(0.1) and a random y: per element within
    (n h w + 2) 2^-24 S.  Observed max err / (2^-24 S) on MI355X: gw 1.96, gb 0.56 of 132."""
    shape = n, cin, cout, h, w = 2, 33, 64, 5, 13
    r = np.random.default_rng(9)
    x, g, y = (r.standard_normal(s).astype(np.float32) for s in ((n, cin, h, w), (n, cout, h, w), (n, cout, h, w)))
    gw, gb = H.twgrad(_dev(x, gpu), _dev(g, gpu), y=_dev(y, gpu), leaky=True)
    rw, rb, sw, sb = R.conv_wgrad(x, g, y)
    _within(gw, rw, sw, n * h * w + 2, f"wgrad gw {shape}")
    _within(gb, rb, sb, n * h * w + 2, f"wgrad gb {shape}")


def _conv_module(wt, b, gpu):
    conv = torch.nn.Conv2d(wt.shape[1], wt.shape[0], 3, padding=1).to(gpu)
    conv.weight, conv.bias = torch.nn.Parameter(_dev(wt, gpu)), torch.nn.Parameter(_dev(b, gpu))
    return conv


@pytest.mark.parametrize("shape", [(2, 6, 32, 9, 13), (1, 70, 4, 7, 11)])
def test_autograd_winograd_conv_integer_exact(gpu, shape):
    """(d) ag.conv3x3 on the default path (TRAIN_WINO: exact-fp32 Winograd F(2x2,3x3) forward and
    dgrad, row-tiled wgrad) on integer data.  The transforms have only dyadic constants: the
    packed weights are multiples of 1/4, the transformed input integers, so with inputs in
    [-4, 4] and cin <= 70 every value is a multiple of 1/4 far below 2^22 and the result equals
    the integer reference exactly; the leaky forward equals leaky_f32 of it."""
    assert ag.TRAIN_WINO
    n, cin, cout, h, w = shape
    x, wt, b, g = _ints(sum(shape) + 4, (n, cin, h, w), (cout, cin, 3, 3), (cout,), (n, cout, h, w))
    conv = _conv_module(wt, b, gpu)
    xd = _dev(x, gpu).requires_grad_()
    y = ag.conv3x3(xd, conv, False)
    y.backward(_dev(g, gpu))
    _eq(y.detach(), R.conv_fwd_int(x, wt, b))
    _eq(xd.grad, R.conv_dgrad_int(g, wt))
    rw, rb = R.conv_wgrad_int(x, g)
    _eq(conv.weight.grad, rw)
    _eq(conv.bias.grad, rb)
    with torch.no_grad():
        _eq(ag.conv3x3(xd, conv, True), R.leaky_f32(R.conv_fwd_int(x, wt, b)))


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(b.abs().max(), 1e-30))


@pytest.mark.parametrize("n,cin,cout,h,w", [(2, 6, 32, 9, 13), (2, 70, 4, 7, 11)])
def test_conv3x3_autograd_implicit_gemm(gpu, monkeypatch, n, cin, cout, h, w):
    """(e) TRAIN_WINO off: _Conv3x3 runs rrin_tconv3x3 (FWD, DGRAD with the fused mask) and the
    fused-leaky weight gradient; test_gpu_train.py's comparison with float64 autograd, leaky on."""
    monkeypatch.setattr(ag, "TRAIN_WINO", False)
    g = torch.Generator().manual_seed(cin * 100 + cout)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    b = torch.randn(cout, generator=g) * 0.1
    gy = torch.randn(n, cout, h, w, generator=g)
    xr, wr, br = (t.double().requires_grad_() for t in (x, wt, b))
    yr = F.leaky_relu(F.conv2d(xr, wr, br, padding=1), 0.1)
    yr.backward(gy.double())
    conv = _conv_module(wt.numpy(), b.numpy(), gpu)
    xg = x.to(gpu).requires_grad_()
    y = ag.conv3x3(xg, conv, True)
    y.backward(gy.to(gpu))
    assert _rel(y, yr) < 1e-5
    assert _rel(xg.grad, xr.grad) < 1e-5
    assert _rel(conv.weight.grad, wr.grad) < 1e-5
    assert _rel(conv.bias.grad, br.grad) < 1e-5


def test_net_gradients_implicit_gemm(gpu, monkeypatch):
    """(e) d(sum of Net output) / d(inputs, every parameter) at 1x32x48, plain weights, with
    TRAIN_WINO off, against the oracle's autograd: 1e-4 relative per tensor (the project bound of
    test_net_gradients_match_oracle_autograd)."""
    from oracle.ref_net import net_forward
    monkeypatch.setattr(ag, "TRAIN_WINO", False)
    net = Net()
    sd = keyed_state_dict(net.state_dict())
    net.load_state_dict(sd)
    net = net.to(gpu).train()
    i0, i1 = synthetic_batch(1, 32, 48, first_index=3)
    a0, a1 = i0.to(gpu).requires_grad_(), i1.to(gpu).requires_grad_()
    out = net(a0, a1, 0.5)
    out.sum().backward()
    p = {k: v.clone().requires_grad_() for k, v in sd.items()}
    r0, r1 = i0.clone().requires_grad_(), i1.clone().requires_grad_()
    ref = net_forward(p, r0, r1, 0.5)
    ref.sum().backward()
    assert _rel(out, ref) < 1e-4
    bad = [(k, _rel(v.grad, p[k].grad)) for k, v in net.named_parameters() if not _rel(v.grad, p[k].grad) < 1e-4]
    assert not bad, bad
    assert _rel(a0.grad, r0.grad) < 1e-4 and _rel(a1.grad, r1.grad) < 1e-4


@pytest.mark.parametrize("shape", [(1, 2, 2), (5, 6, 10), (3, 4, 258)])
def test_tpool2_bitwise(gpu, shape):
    """(f) forward: the kernel's fp32 expression 0.25 (((x00 + x01) + x10) + x11) in numpy
    float32, bit for bit; backward: 0.25 gy, bit for bit."""
    nc, h, w = shape
    r = np.random.default_rng(w)
    x = r.standard_normal(shape).astype(np.float32)
    gy = r.standard_normal((nc, h // 2, w // 2)).astype(np.float32)
    _eq(H.tresample("rrin_tpool2_fwd", _dev(x, gpu), (nc, h // 2, w // 2)), R.pool2_fwd_f32(x))
    _eq(H.tresample("rrin_tpool2_bwd", _dev(gy, gpu), shape), R.pool2_bwd(gy))


@pytest.mark.parametrize("shape", [(1, 1, 1), (4, 1, 3), (2, 5, 7), (1, 2, 130)])
def test_tup2_exact_and_adjoint(gpu, shape):
    """(f) every weight is 0, 0.25, 0.75 or 1: integer data makes forward and backward exact, so
    they equal the float64 reference.  On random data <up2(x), g> = <x, up2_bwd(g)> (in float64,
    from the kernels' fp32 outputs) within 16 * 2^-24 * sum |terms| (observed: at most 0.30 of the 16)."""
    nc, h, w = shape
    up = (nc, 2 * h, 2 * w)
    x, g = _ints(w, shape, up)
    _eq(H.tresample("rrin_tup2_fwd", _dev(x, gpu), up), R.up2_fwd(x))
    _eq(H.tresample("rrin_tup2_bwd", _dev(g, gpu), shape), R.up2_bwd(g))
    r = np.random.default_rng(h)
    x, g = r.standard_normal(shape).astype(np.float32), r.standard_normal(up).astype(np.float32)
    yx = H.tresample("rrin_tup2_fwd", _dev(x, gpu), up).cpu().numpy().astype(np.float64)
    xg = H.tresample("rrin_tup2_bwd", _dev(g, gpu), shape).cpu().numpy().astype(np.float64)
    lhs, rhs = float((yx * g).sum()), float((x * xg).sum())
    terms = float((R.up2_fwd(np.abs(x)) * np.abs(g)).sum())
    print(f"adjoint {shape}: |lhs - rhs| / (2^-24 sum|terms|) = {abs(lhs - rhs) / (U * terms):.3f} of 16")
    assert abs(lhs - rhs) <= 16 * U * terms


# ---- (g) rrin_twarp_bwd ----------------------------------------------------------------------
def _gout(r, shape):
    """randn with |g| >= 2^-10: no product near the denormals."""
    g = r.standard_normal(shape)
    return (np.sign(g) * (np.abs(g) + 2.0 ** -10)).astype(np.float32)


def _img(r, shape):
    return (r.random(shape) + 0.5).astype(np.float32)


def _warp_check(gpu, img, flow, gout, what):
    """gimg bit for bit the fixed-point model; gflow per element within k 2^-24 S with
    k = 7 c + 2: per channel the kernel's gix chain is 2 differences, 2 products, 1 sum, the
    product with go and the accumulation (7 fp32 operations, fewer when contracted to FMAs), then
    the two scale factors.  Observed max err / (2^-24 S) on MI355X over all the cases below: 2.60 (c = 2, k = 16); random
    flows with c = 3: 2.21 of 23."""
    c = img.shape[1]
    gimg, gflow = H.twarp_bwd(_dev(img, gpu), _dev(flow, gpu), _dev(gout, gpu))
    ri, rf, s = R.warp_bwd(img, flow, gout)
    assert torch.equal(gimg.cpu(), torch.from_numpy(ri)), (what, int((gimg.cpu() != torch.from_numpy(ri)).sum()))
    _within(gflow, rf, s, 7 * c + 2, f"gflow {what}")
    return gimg, gflow, ri, rf


@pytest.mark.parametrize("scale", [0.3, 40.0])
def test_twarp_bwd_random_flows(gpu, scale):
    """2x3x17x23: h w = 391 is no power of two (hb = ceil(log2 391) = 9)."""
    r = np.random.default_rng(int(scale * 10))
    shape = (2, 3, 17, 23)
    flow = (r.standard_normal((2, 2, 17, 23)) * scale).astype(np.float32)
    _, _, ri, _ = _warp_check(gpu, _img(r, shape), flow, _gout(r, shape), f"scale {scale}")
    assert np.abs(ri).max() > 0


@pytest.mark.parametrize("half", [False, True])
def test_twarp_bwd_integer_and_half_pixel_flows(gpu, half):
    """8 x 16 (the position arithmetic is exact): flows k + 0.5 sample an integer position (weights
    1, 0, 0, 0: the zero-weight taps add nothing), flows k the middle of four pixels (all 0.25)
    or, with k + 0.5 in one axis only, of two (0.5, 0.5, 0, 0)."""
    r = np.random.default_rng(5)
    shape = (2, 2, 8, 16)
    k = r.integers(-3, 4, (2, 2, 8, 16)).astype(np.float32)
    flow = k.copy()
    flow[:, 0] += 0.5
    if not half:
        flow[:, 1] += 0.5
    t = R.warp_taps32(flow)
    assert set(np.unique(t["nw"])) == ({0.5} if half else {1.0}) and np.all(t["se"] == 0)
    _warp_check(gpu, _img(r, shape), flow, _gout(r, shape), f"half={half}")
    if half:
        t = R.warp_taps32(k)
        assert set(np.unique(np.stack([t[q] for q in ("nw", "ne", "sw", "se")]))) == {0.25}
        _warp_check(gpu, _img(r, shape), k, _gout(r, shape), "quarter")


@pytest.mark.parametrize("shape", [(1, 2, 5, 7), (2, 1, 8, 16)])
def test_twarp_bwd_border_straddle(gpu, shape):
    """Samples in (-1, 0) and (W - 1, W), (H - 1, H) on each side and corner: one (corner) or
    two (side) taps are valid, the others add neither to gimg nor to gflow."""
    n, c, h, w = shape
    r = np.random.default_rng(h)
    tx = np.array([-0.5, 2.3, w - 0.5, -0.25, w - 0.75])
    ty = np.array([-0.5, 1.7, h - 0.5, -0.75, h - 0.25])
    i = np.arange(n * h * w).reshape(n, h, w)
    gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    flow = np.stack((tx[i % 5] + 0.5 - gx, ty[(i // 5) % 5] + 0.5 - gy), 1).astype(np.float32)
    t = R.warp_taps32(flow)
    valid = sum((t[a] & t[b]).astype(int) for a in ("vy0", "vy1") for b in ("vx0", "vx1"))
    assert {1, 2, 4} <= set(np.unique(valid))
    _warp_check(gpu, _img(r, shape), flow, _gout(r, shape), f"border {shape}")


@pytest.mark.parametrize("far", [1e4, -1e4, 1e30, -1e30])
def test_twarp_bwd_fully_outside(gpu, far):
    r = np.random.default_rng(2)
    shape = (1, 2, 6, 9)
    flow = np.full((1, 2, 6, 9), far, np.float32)
    gimg, gflow = H.twarp_bwd(_dev(_img(r, shape), gpu), _dev(flow, gpu), _dev(_gout(r, shape), gpu))
    assert torch.equal(gimg.cpu(), torch.zeros(shape)) and torch.equal(gflow.cpu(), torch.zeros(1, 2, 6, 9))


@pytest.mark.parametrize("shape", [(2, 2, 1, 19), (2, 2, 19, 1), (1, 1, 1, 1)])
def test_twarp_bwd_single_row_and_column(gpu, shape):
    n, c, h, w = shape
    r = np.random.default_rng(w)
    flow = (r.standard_normal((n, 2, h, w)) * 1.5).astype(np.float32)
    _warp_check(gpu, _img(r, shape), flow, _gout(r, shape), f"{shape}")


def test_twarp_bwd_zero_gradient(gpu):
    """gout == 0: the scale is 1 and every output is zero."""
    r = np.random.default_rng(3)
    shape = (2, 3, 17, 23)
    flow = r.standard_normal((2, 2, 17, 23)).astype(np.float32)
    gimg, gflow = H.twarp_bwd(_dev(_img(r, shape), gpu), _dev(flow, gpu), _dev(np.zeros(shape), gpu))
    assert torch.equal(gimg.cpu(), torch.zeros(shape)) and torch.equal(gflow.cpu(), torch.zeros(2, 2, 17, 23))


@pytest.mark.parametrize("shape", [(1, 1, 64, 64), (1, 2, 17, 23)])
def test_twarp_bwd_collision_headroom(gpu, shape):
    """Every pixel's flow points at source pixel (row 5, column 7) and gout is 0.999 everywhere:
    one target receives h w taps of weight 1 (64 x 64: exactly; 17 x 23: up to the position's
    rounding, which the model follows), the worst case of fx_scale's overflow argument
    (0.999 * 2^(62 - hb) * h w < 2^63).  On 64 x 64 the target is fl32(4096 * fl32(0.999))."""
    n, c, h, w = shape
    r = np.random.default_rng(4)
    gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    flow = np.broadcast_to(np.stack((7.5 - gx, 5.5 - gy))[None], (n, 2, h, w)).astype(np.float32)
    gout = np.full(shape, 0.999, np.float32)
    gimg, _, ri, _ = _warp_check(gpu, _img(r, shape), flow, gout, f"collision {shape}")
    if shape == (1, 1, 64, 64):
        want = np.zeros(shape, np.float32)
        want[0, 0, 5, 7] = np.float32(4096.0 * float(np.float32(0.999)))
        assert np.array_equal(ri, want) and torch.equal(gimg.cpu(), torch.from_numpy(want))
    else:
        assert abs(float(ri[0, 0, 5, 7]) - 391 * 0.999) < 1e-3 * 391


def test_twarp_bwd_dynamic_range(gpu):
    """One gout element is 1.0, the rest 2^-20: the scale follows the maximum, the small ones
    keep 2^-20 * 2^(62 - 9 - 1) = 2^32 units each and are not lost."""
    r = np.random.default_rng(6)
    shape = (1, 2, 17, 23)
    gout = np.full(shape, 2.0 ** -20, np.float32)
    gout[0, 1, 8, 11] = 1.0
    flow = (r.standard_normal((1, 2, 17, 23)) * 0.3).astype(np.float32)
    gimg, _, ri, _ = _warp_check(gpu, _img(r, shape), flow, gout, "dynamic range")
    assert R.fx_scale(gout, 17 * 23) == 52
    # channel 0 holds small gradients only: its total is 2^-20 x the total valid tap weight
    t = R.warp_taps32(flow)
    total = sum(float(t[q].astype(np.float64)[t[a] & t[b]].sum())
                for q, a, b in (("nw", "vy0", "vx0"), ("ne", "vy0", "vx1"), ("sw", "vy1", "vx0"), ("se", "vy1", "vx1")))
    got = float(gimg.cpu().numpy()[0, 0].astype(np.float64).sum())
    assert total > 300 and abs(got - 2.0 ** -20 * total) <= 4 * U * 2.0 ** -20 * total


def test_twarp_bwd_deterministic_and_batch_order(gpu):
    """Two calls are bitwise equal; a batch-reversed copy of the inputs gives the batch-reversed
    gimg and gflow (the scale is the call's maximum, the sum order-free)."""
    r = np.random.default_rng(7)
    shape = (3, 3, 17, 23)
    img, gout = _dev(_img(r, shape), gpu), _dev(_gout(r, shape), gpu)
    flow = _dev((r.standard_normal((3, 2, 17, 23)) * 6).astype(np.float32), gpu)
    a, fa = H.twarp_bwd(img, flow, gout)
    b, fb = H.twarp_bwd(img, flow, gout)
    assert torch.equal(a, b) and torch.equal(fa, fb)
    c, fc = H.twarp_bwd(img.flip(0).contiguous(), flow.flip(0).contiguous(), gout.flip(0).contiguous())
    assert torch.equal(c.flip(0), a) and torch.equal(fc.flip(0), fa)
