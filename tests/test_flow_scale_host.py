"""Host side of flow_scale (rrin_amd/flowscale.py): the reference against the oracle, the NumPy
restatements of the two kernels against PyTorch, the padded-size rule, refused values, the CLI flag,
the tag rule for Flow reuse and the entry points' argument checks.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.ref_net import net_forward
from rrin_amd import _lib, flowscale
from rrin_amd.__main__ import build_parser
from tests import flow_scale_ref as FS
from tests import net_contract as NC

EPS = 2.0 ** -24  # half an ulp of an fp32 value in [1, 2): the bound of one rounded operation, relative


@pytest.mark.parametrize("tname", ["0.5", "tensor"])
def test_scaled_reference_at_1_is_the_oracle(tname):
    i0, i1 = NC.net_frames(2, 16, 32)
    t = NC.net_t(tname, 2)
    sd = NC.net_state_dict("default")
    with torch.no_grad():
        assert torch.equal(FS.net_forward_scaled(sd, i0, i1, t, 1), net_forward(sd, i0, i1, t))


def test_scaled_reference_differs_and_keeps_the_shape():
    i0, i1 = NC.net_frames(1, 32, 64)
    sd = NC.net_state_dict("default")
    with torch.no_grad():
        a, b = FS.net_forward_scaled(sd, i0, i1, 0.5, 2), net_forward(sd, i0, i1, 0.5)
    assert a.shape == b.shape and not torch.equal(a, b)


@pytest.mark.parametrize("s", [2, 4])
def test_downscale_restatement_against_avg_pool(s):
    """s*s - 1 rounded additions on either side (the scale by 1/s^2 is exact): each is off by at most
    EPS times the sum of magnitudes, so the two differ by at most 2 (s*s - 1) EPS avg(|x|) s*s."""
    x = torch.randn(3, 6, 8 * s, 12 * s, generator=torch.Generator().manual_seed(s)) * 3
    got = torch.from_numpy(FS.downscale_np(x.numpy(), s))
    ref = F.avg_pool2d(x, s)
    bound = 2 * (s * s - 1) * EPS * F.avg_pool2d(x.abs(), s) * (s * s)
    assert bool(((got - ref).abs() <= bound).all())
    exact = F.avg_pool2d(x.double(), s)
    assert float((got.double() - exact).abs().max()) <= float(bound.max())


@pytest.mark.parametrize("s", [2, 4])
def test_upscale_restatement_against_interpolate(s):
    """9 rounded operations per value on either side (6 products, 3 sums; the weights and * s are
    exact), each off by at most EPS times the interpolated magnitudes: 18 EPS s interp(|f|)."""
    f = torch.randn(2, 4, 7, 9, generator=torch.Generator().manual_seed(10 + s)) * 5
    got = torch.from_numpy(FS.upscale_np(f.numpy(), s))
    ref = s * F.interpolate(f, scale_factor=s, mode="bilinear", align_corners=False)
    mag = s * F.interpolate(f.abs(), scale_factor=s, mode="bilinear", align_corners=False)
    assert got.shape == ref.shape
    assert bool(((got - ref).abs() <= 18 * EPS * mag).all())
    exact = s * F.interpolate(f.double(), scale_factor=s, mode="bilinear", align_corners=False)
    assert bool(((got.double() - exact).abs() <= 9 * EPS * mag.double()).all())


@pytest.mark.parametrize("s", [2, 4])
def test_upscale_weights_are_dyadic_and_clamped(s):
    i0, i1, w = FS.upscale_taps(5, s)
    assert i0.min() == 0 and i1.max() == 4 and (i1 - i0).max() == 1
    assert set(np.unique(w * (2 * s))) <= set(range(2 * s))      # multiples of 1 / 2s
    src = np.maximum((np.arange(5 * s) + 0.5) / s - 0.5, 0)
    assert np.array_equal(i0 + w.astype(np.float64), src)        # exactly the clamped coordinate


def test_padded_size_rule():
    assert flowscale.padded_size(720, 1280, 1) == (720, 1280)
    assert flowscale.padded_size(720, 1280, 2) == (736, 1280)
    assert flowscale.padded_size(720, 1280, 4) == (768, 1280)
    assert flowscale.padded_size(2160, 3840, 2) == (2176, 3840)
    assert flowscale.padded_size(2160, 3840, 4) == (2176, 3840)
    assert flowscale.padded_size(37, 53, 2) == (64, 64) and flowscale.padded_size(37, 53, 1) == (48, 64)
    from rrin_amd import convert as cv
    assert cv.pad_amounts(1280, 720, 4) == (48, 0) and cv.pad_amounts(1280, 720) == (0, 0)
    f = torch.arange(2 * 5 * 7 * 3, dtype=torch.uint8).view(2, 5, 7, 3)
    x = cv.frames_u8_to_float(f, 2)
    assert tuple(x.shape) == (2, 3, 32, 32)
    assert torch.equal(x[:, :, 27:, :7], cv.frames_u8_to_float(f)[:, :, 11:, :7])   # the frame, bottom left
    assert torch.equal(x[:, :, 0, :], x[:, :, 27, :]) and torch.equal(x[:, :, :, 31], x[:, :, :, 6])


@pytest.mark.parametrize("bad", [0, 3, 8, -2, 2.0, "2", None, True])
def test_rejected_values(bad):
    with pytest.raises(ValueError, match="flow_scale"):
        flowscale.check_flow_scale(bad)
    with pytest.raises(ValueError, match="flow_scale"):
        flowscale.padded_size(32, 32, bad)


def test_net_methods_refuse_before_the_device():
    """A Net on the CPU has no engine: a bad flow_scale must raise its ValueError first."""
    from rrin_amd import Net
    net = Net()
    frames = torch.zeros(3, 16, 16, 3, dtype=torch.uint8)
    with torch.no_grad():
        with pytest.raises(ValueError, match="flow_scale"):
            net.interpolate_items_u8(frames, [0], [0.5], flow_scale=3)
        with pytest.raises(ValueError, match="flow_scale"):
            net.interpolate(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16), [0.5], flow_scale=3)


def test_cli_flag():
    p = build_parser()
    a = p.parse_args(["--model_name", "m", "convert", "--sf", "1", "--fps", "30", "--flow_scale", "2"])
    assert a.flow_scale == 2
    a = p.parse_args(["--model_name", "m", "convert", "--sf", "1", "--fps", "30"])
    assert a.flow_scale == 1
    a = p.parse_args(["--model_name", "m", "evaluate", "--y4m_in", "-", "--flow_scale", "4"])
    assert a.flow_scale == 4
    with pytest.raises(SystemExit):
        p.parse_args(["--model_name", "m", "evaluate", "--y4m_in", "-", "--flow_scale", "3"])


def test_tag_rule():
    assert flowscale.flow_tag("u8", 1) == "u8"
    tags = {flowscale.flow_tag(t, s) for t in ("f32", "u8", "u16:10", "yuv:i420:1,2") for s in (1, 2, 4)}
    assert len(tags) == 12                                        # no two (path, scale) share a tag
    assert flowscale.flow_tag("u8", 2) != flowscale.flow_tag("u8", 4)


def test_convert_functions_refuse_bad_values_first():
    """The convert functions refuse a bad flow_scale before they touch their other arguments (the
    pass-through to the model's call: tests/test_flow_scale_convert_host.py)."""
    from rrin_amd import convert as cv
    with pytest.raises(ValueError, match="flow_scale"):
        cv.retime_y4m(None, None, None, "60", flow_scale=3)
    with pytest.raises(ValueError, match="flow_scale"):
        cv.evaluate_y4m(None, None, flow_scale=3)
    with pytest.raises(ValueError, match="flow_scale"):
        cv.interpolate_y4m(None, None, None, sf=1, flow_scale=5)
    with pytest.raises(ValueError, match="flow_scale"):
        cv.interpolate_folder(None, "x", "y", 1, u8=False, flow_scale=2)


# ---- the entry points validate before any HIP call ---------------------------------------------
def h8(h, w, prec, groups, ptr=0x1000, lo=0x2000):
    v = _lib.H8()
    v.hi = ptr
    v.lo = lo if prec == _lib.PREC_F16X3 else None
    v.g = _lib.geom_h8(h, w)
    v.img_stride = groups * v.g.plane
    v.g_off, v.groups = 0, groups
    return v


@pytest.mark.parametrize("prec", _lib.RECORD_PRECS)
def test_kernel_entries_reject_before_any_launch(prec):
    L = _lib.lib()
    g16 = 16 // _lib.chans_per_record(prec)
    big, small = h8(32, 64, prec, g16), h8(16, 32, prec, g16)
    E_SHAPE, E_ARG = -1, -2
    down = lambda a, b, n=1, s=2, p=prec: L.rrin_g16_downscale_h8(a, b, n, s, p, None)
    up = lambda a, b, n=1, s=2, p=prec: L.rrin_flow_upscale_h8(a, b, n, s, p, None, None)
    for fn, src, dst in ((down, big, small), (up, small, big)):
        assert fn(None, C.byref(dst)) == E_ARG and fn(C.byref(src), None) == E_ARG
        for s in (0, 1, 3, 8):
            assert fn(C.byref(src), C.byref(dst), s=s) == E_ARG
        assert fn(C.byref(src), C.byref(dst), n=0) == E_ARG
        assert fn(C.byref(src), C.byref(dst), p=_lib.PREC_F32) == E_ARG
        assert fn(C.byref(src), C.byref(dst), s=4) == E_SHAPE          # not the exact quotient
        assert fn(C.byref(src), C.byref(src)) == E_SHAPE
    odd = h8(16, 48, prec, g16)
    assert down(C.byref(big), C.byref(odd)) == E_SHAPE and up(C.byref(odd), C.byref(big)) == E_SHAPE
    few = h8(16, 32, prec, 1)
    if _lib.chans_per_record(prec) * 1 < 16:
        assert down(C.byref(big), C.byref(few)) == E_SHAPE
    nohi = h8(16, 32, prec, g16, ptr=None)
    assert down(C.byref(big), C.byref(nohi)) == E_SHAPE


def test_scaled_forward_rejects_before_any_launch():
    L = _lib.lib()
    d = _lib.NetU8Desc()
    fs = _lib.FlowScale()
    E_SHAPE, E_ARG = -1, -2
    assert L.rrin_net_u8_scaled_fwd(C.byref(d), None, None, None) == E_ARG
    assert L.rrin_net_u8_scaled_fwd(None, None, C.byref(fs), None) == E_ARG
    table = (_lib.ConvWeights * 77)()
    heads = (_lib.HeadWeights * 4)()
    fs.s, fs.convs, fs.workspace, fs.workspace_bytes = 3, table, 0x1000, 1 << 40
    d.net.n, d.net.h, d.net.w, d.net.prec = 1, 64, 64, _lib.PREC_F32R
    d.net.coef, d.net.convs, d.net.heads, d.net.workspace, d.net.workspace_bytes = 0x1000, table, heads, 0x1000, 1 << 40
    d.f0 = d.f1 = d.out_u8 = 0x1000
    d.h0, d.w0, d.img_stride = 37, 53, 37 * 53 * 3
    assert L.rrin_net_u8_scaled_fwd(C.byref(d), None, C.byref(fs), None) == E_ARG      # s = 3
    fs.s = 2
    d.net.prec = _lib.PREC_F32
    assert L.rrin_net_u8_scaled_fwd(C.byref(d), None, C.byref(fs), None) == E_ARG      # planar
    d.net.prec = _lib.PREC_F32R
    d.net.h = 48                                                                          # round_up(37, 16)
    assert L.rrin_net_u8_scaled_fwd(C.byref(d), None, C.byref(fs), None) == E_SHAPE
    d.net.h, d.h0 = 64, 20                                                                # 20 pads to 32 at s = 2
    assert L.rrin_net_u8_scaled_fwd(C.byref(d), None, C.byref(fs), None) == E_SHAPE
    d.h0 = 37
    fs.workspace_bytes = 16
    assert L.rrin_net_u8_scaled_fwd(C.byref(d), None, C.byref(fs), None) == -3           # E_WORKSPACE
    nd = _lib.NetDesc()
    assert L.rrin_net_scaled_fwd(C.byref(nd), None, None) == E_ARG
