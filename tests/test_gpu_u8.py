"""GPU: the 8-bit frame path (rrin_pack_g16_u8_h8, the FINAL head's uint8 store, rrin_net_u8_fwd,
RRINEngine.forward_u8, Net.forward_u8 / interpolate_u8, the byte pipeline of interpolate_folder)
is bit for bit the host chain load_frame -> Net.forward -> to_uint8_image.  Every comparison is
exact equality.  Shapes: 17x33 (the largest pads: 15 rows on top, 15 columns on the right), 37x50
(medium pads), 64x96 (no padding), 16x16 (the minimum)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from PIL import Image

from rrin_amd import Net, _lib
from rrin_amd import convert as cv
from rrin_amd.pp import H8Tensor
from rrin_amd.synthetic import keyed_state_dict, synthetic_batch

from . import hip_helpers as H

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "fp32_split16", "fp16"]
SHAPES = [(17, 33), (37, 50), (64, 96), (16, 16)]
_SD = {}
_NETS = {}


def net_of(dev, precision):
    """One Net per precision for the whole module (an engine is rebuilt when the precision changes)."""
    if precision not in _NETS:
        if "sd" not in _SD:
            _SD["sd"] = keyed_state_dict(Net().state_dict(), stress=True)
        net = Net()
        net.load_state_dict(_SD["sd"], strict=True)
        net.precision = precision
        _NETS[precision] = net.to(dev).eval()
    return _NETS[precision]


def frames(n, h0, w0, seed, dev=None):
    """uint8 [n,h0,w0,3]; the first 256 bytes of every frame hold every byte value."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (n, h0, w0, 3), dtype=np.uint8)
    a.reshape(n, -1)[:, :256] = np.arange(256, dtype=np.uint8)
    t = torch.from_numpy(a)
    return t.to(dev) if dev is not None else t


def padded(f, dev):
    """The host mapping of load_frame (tests/test_u8_host.py ties the helper to it), on the device."""
    return cv.frames_u8_to_float(f.cpu()).contiguous().to(dev)


def host_u8(out, h0, w0):
    """to_uint8_image of every frame of a float [N,3,H,W] output."""
    meta = {"top": out.shape[2] - h0, "height": h0, "width": w0}
    return np.stack([cv.to_uint8_image(o, meta) for o in out.cpu()])


@pytest.mark.parametrize("shape", SHAPES[:3], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("precision", PRECISIONS)
def test_pack_u8_equals_float_pack(gpu, precision, shape):
    """rrin_pack_g16_u8_h8 writes the records rrin_pack_g16_h8 writes from the host-padded float
    frames: the whole buffers (hi and lo, padding included) are equal."""
    prec = _lib.PRECISIONS[precision]
    h0, w0 = shape
    h, w = (h0 + 15) // 16 * 16, (w0 + 15) // 16 * 16
    f0, f1 = frames(2, h0, w0, 1, gpu), frames(2, h0, w0, 2, gpu)
    got = H8Tensor(2, 16, h, w, gpu, prec)
    want = H8Tensor(2, 16, h, w, gpu, prec)
    v = got.view(0, 16)
    _lib.check(_lib.lib().rrin_pack_g16_u8_h8(f0.data_ptr(), f1.data_ptr(), h0 * w0 * 3, 2, h0, w0, C.byref(v), prec,
                                              H.stream(gpu)), "rrin_pack_g16_u8_h8")
    i0, i1 = padded(f0, gpu), padded(f1, gpu)
    v = want.view(0, 16)
    _lib.check(_lib.lib().rrin_pack_g16_h8(i0.data_ptr(), i1.data_ptr(), 2, C.byref(v), prec, H.stream(gpu)),
               "rrin_pack_g16_h8")
    torch.cuda.synchronize(gpu)
    assert want.hi.any()
    assert torch.equal(got.hi.view(torch.uint8), want.hi.view(torch.uint8))
    if want.lo is not None:
        assert torch.equal(got.lo.view(torch.uint8), want.lo.view(torch.uint8))
    # a g16 of another size is refused
    bad = H8Tensor(2, 16, h + 16, w, gpu, prec).view(0, 16)
    assert _lib.lib().rrin_pack_g16_u8_h8(f0.data_ptr(), f1.data_ptr(), h0 * w0 * 3, 2, h0, w0, C.byref(bad), prec,
                                          H.stream(gpu)) == -1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_u8_equals_host_chain(gpu, precision, shape):
    """forward_u8(f0, f1, t) == to_uint8_image(forward(padded floats, t)) for every pair: n = 1, and
    n = 3 on the default streams (parts of 1 + 2 pairs: a part's frame offset into the stacks)."""
    net = net_of(gpu, precision)
    h0, w0 = shape
    for n in (1, 3):
        f0, f1 = frames(n, h0, w0, 10 + n, gpu), frames(n, h0, w0, 20 + n, gpu)
        i0, i1 = padded(f0, gpu), padded(f1, gpu)
        for t in (0.5, 0.25):
            with torch.no_grad():
                want = host_u8(net(i0, i1, t), h0, w0)
                got = net.forward_u8(f0, f1, t)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h0, w0, 3) and got.device == f0.device
            np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"n={n} t={t}")
    net.check_range()


def test_forward_u8_on_views_of_one_stack(gpu):
    net = net_of(gpu, "fp32")
    fr = frames(4, 37, 50, 31, gpu)
    with torch.no_grad():
        got = net.forward_u8(fr[:-1], fr[1:], 0.5)
        want = net.forward_u8(fr[:-1].contiguous(), fr[1:].contiguous(), 0.5)
        # frames that are not dense are copied, not misread
        wide = torch.zeros((3, 37, 60, 3), dtype=torch.uint8, device=gpu)
        wide[:, :, :50] = fr[:-1]
        got2 = net.forward_u8(wide[:, :, :50], fr[1:], 0.5)
    assert torch.equal(got, want) and torch.equal(got2, want)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_interpolate_u8_reuses_flow_and_keeps_the_float_path_apart(gpu, precision):
    net = net_of(gpu, precision)
    f0, f1 = frames(2, 37, 50, 41, gpu), frames(2, 37, 50, 42, gpu)
    ts = [0.25, 0.5, 0.75]
    eng = net.engine()
    with torch.no_grad():
        each = [net.forward_u8(f0, f1, t) for t in ts]
        outs = net.interpolate_u8(f0, f1, ts)
        for a, b in zip(outs, each):
            assert torch.equal(a, b)
        # the workspaces now hold the raw Flow of (f0, f1): a float forward at the same padded shape
        # with other frames and reuse_flow=True must not take it for its own previous pair
        j0, j1 = padded(frames(2, 37, 50, 43), gpu), padded(frames(2, 37, 50, 44), gpu)
        got = eng.forward(j0, j1, 0.5, reuse_flow=True, streams=net.streams)
        fresh = eng.forward(j0, j1, 0.5, streams=net.streams)
        assert torch.equal(got, fresh)
        again = eng.forward(j0, j1, 0.75, reuse_flow=True, streams=net.streams)   # its own pair: reused
        assert torch.equal(again, eng.forward(j0, j1, 0.75, streams=net.streams))
        # and the other way round: forward_u8 does not reuse the float path's Flow
        eng.forward(j0, j1, 0.5, streams=net.streams)
        got8 = eng.forward_u8(f0, f1, 0.5, reuse_flow=True, streams=net.streams)
        assert torch.equal(got8, each[1])
    net.check_range()


def test_float_path_untouched_by_forward_u8(gpu):
    net = net_of(gpu, "fp32")
    i0, i1 = synthetic_batch(2, 64, 96)
    i0, i1 = i0.to(gpu), i1.to(gpu)
    with torch.no_grad():
        before = net(i0, i1, 0.5).clone()
        net.forward_u8(frames(2, 64, 96, 51, gpu), frames(2, 64, 96, 52, gpu), 0.5)
        after = net(i0, i1, 0.5)
    assert torch.equal(before.view(torch.int32), after.view(torch.int32))


def test_forward_u8_rejects_bad_inputs(gpu):
    net = net_of(gpu, "fp32")
    f = frames(1, 32, 48, 61, gpu)
    with torch.no_grad():
        with pytest.raises(TypeError):
            net.forward_u8(f.float(), f.float())
        with pytest.raises(ValueError):
            net.forward_u8(f.permute(0, 3, 1, 2).contiguous(), f.permute(0, 3, 1, 2).contiguous())   # [N,3,H,W]
        with pytest.raises(ValueError):
            net.forward_u8(f, f[:, :16])
        with pytest.raises(RuntimeError):
            net.forward_u8(f.cpu(), f.cpu())
    with pytest.raises(RuntimeError, match="inference-only"):
        net.forward_u8(f, f)                                                                 # autograd on
    planar = Net()
    planar.load_state_dict(_SD["sd"], strict=True)
    planar.precision = "fp32_planar"
    planar = planar.to(gpu).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="'fp32', 'fp32_split16' or 'fp16'"):
        planar.forward_u8(f, f)


def test_byte_pipeline_on_gpu_writes_the_float_pipelines_files(tmp_path, gpu):
    """interpolate_folder on the HIP Net with u8=True and u8=False: byte-identical PNGs (the float
    pipeline is held to the oracle by tests/test_convert.py)."""
    src = str(tmp_path / "in")
    os.makedirs(src)
    fr = frames(1, 37, 50, 71)[0].numpy()
    for k in range(5):
        Image.fromarray(np.roll(fr, 2 * k, axis=1)).save(os.path.join(src, f"{k + 1:09d}.png"))
    net = net_of(gpu, "fp32")
    a, b = str(tmp_path / "u8"), str(tmp_path / "f32")
    na = cv.interpolate_folder(net, src, a, sf=3, batch=2, device=gpu, u8=True, log=lambda *x: None)
    nb = cv.interpolate_folder(net, src, b, sf=3, batch=2, device=gpu, u8=False, log=lambda *x: None)
    assert na == nb == 17 and sorted(os.listdir(a)) == sorted(os.listdir(b))
    for name in os.listdir(b):
        assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name
    # "auto" takes the byte path for a Net on a device
    calls = []
    orig = net.interpolate_u8
    net.interpolate_u8 = lambda *x: calls.append(1) or orig(*x)
    try:
        cv.interpolate_folder(net, src, str(tmp_path / "auto"), sf=1, batch=4, device=gpu, log=lambda *x: None)
    finally:
        del net.interpolate_u8
    assert calls == [1]


def test_range_guard_writes_zeros_and_check_range_raises(gpu):
    """An fp16 overflow (the recipe of test_split16_overflow_is_loud): the float path's output is
    NaN, the byte path's is 0, and check_range raises for both."""
    from .test_gpu_configs import wide_range_sd
    net = Net()
    net.load_state_dict(wide_range_sd(1e5), strict=True)
    net.precision = "fp32_split16"
    net = net.to(gpu).eval()
    i0, i1 = synthetic_batch(1, 64, 96, first_index=2)
    f0 = i0.mul(255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(gpu)
    f1 = i1.mul(255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(gpu)
    with torch.no_grad():
        out = net(padded(f0, gpu), padded(f1, gpu), 0.5)
    assert torch.isnan(out).all()                      # these frames do overflow
    with pytest.raises(RuntimeError, match="fp16 range"):
        net.check_range()
    with torch.no_grad():
        out8 = net.forward_u8(f0, f1, 0.5)
    assert out8.dtype == torch.uint8 and not out8.any()
    with pytest.raises(RuntimeError, match="fp16 range"):
        net.check_range()
    net.precision = "fp32"                               # exact fp32 has no guard: real frames
    with torch.no_grad():
        assert net.forward_u8(f0, f1, 0.5).any()
