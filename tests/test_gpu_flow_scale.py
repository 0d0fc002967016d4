"""GPU: low-resolution flow estimation (flow_scale 2 and 4; rrin_amd/flowscale.py).

* the two kernels, bit for bit against the NumPy restatements of tests/flow_scale_ref.py with the
  format's store rounding (glue_ref.store_round), into storage that is garbage in the interior and
  zero in the halo, the whole storage compared afterwards;
* the float forward against ``net_forward_scaled`` in float64 under the gates of tests/net_contract.py;
* every frame path, the item forwards, Flow reuse and the scene gate, bit for bit against their
  definitions with the scale passed through; flow_scale=1 equals the call without the keyword.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from rrin_amd import Net, _lib
from rrin_amd import convert as cv
from rrin_amd import yuv as Y
from rrin_amd.pp import H8Tensor
from tests import flow_scale_ref as FS
from tests import glue_ref as G
from tests import hip_helpers as H
from tests import net_contract as NC
from tests import record_ref as R

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "fp32_split16", "fp16"]
NAME = {_lib.PREC_F32R: "R32", _lib.PREC_F16X3: "F16X3", _lib.PREC_F16: "F16"}
KERNEL_SIZES = [(2, 32, 32), (2, 32, 96), (2, 64, 32), (4, 64, 64), (4, 64, 128)]  # s, full H, W
_NETS = {}


def net_of(dev, precision):
    if precision not in _NETS:
        net = Net()
        net.load_state_dict(NC.net_state_dict("default"), strict=True)
        net.precision = precision
        _NETS[precision] = net.to(dev).eval()
    return _NETS[precision]


def whole_storage(t, before, enc, groups, what):
    """Every plane of the guarded tensor t equals its snapshot ``before`` with the interior of the
    record groups [0, groups) replaced by the encoded records ``enc``; the guard bands keep their bits."""
    h, w = t.h, t.w
    after = t.snapshot()
    for p, (a, b, e) in enumerate(zip(after, before, [e for e in enc if e is not None])):
        want = b.clone()
        wv = want[t.guard:t.guard + t.hi.numel()].view(t.hi.shape)
        wv[:, :groups, 1:h + 1, 8:8 + w] = e[:, :groups, 1:h + 1, 8:8 + w]
        bad = R.bits(a) != R.bits(want)
        assert not bool(bad.any()), f"{what}: plane {p}: {int(bad.sum())} elements differ, first at flat index " \
                                    f"{int(bad.nonzero()[0])} (guard {t.guard})"


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("s,h,w", KERNEL_SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_downscale_bits_and_whole_storage(gpu, precision, s, h, w, n):
    prec = _lib.PRECISIONS[precision]
    x = G.pattern((n, 16, h, w), 11 + s) * 3                    # channels 6-15 are garbage: never read
    src = H8Tensor.from_nchw(x.to(gpu), prec)
    stored = G.store_round(x[:, :6], NAME[prec]).numpy()          # what the kernel loads
    want = torch.from_numpy(FS.downscale_np(stored, s))
    lh, lw = h // s, w // s
    dst = R.GuardedH8(n, 16, lh, lw, gpu, prec, seed=31)
    dst.zero_padding()
    before = dst.snapshot()
    sv, dv = src.view(0, 16), dst.view(0, 16)
    _lib.check(_lib.lib().rrin_g16_downscale_h8(C.byref(sv), C.byref(dv), n, s, prec, H.stream(gpu)),
               "rrin_g16_downscale_h8")
    torch.cuda.synchronize(gpu)
    full = torch.cat([want, torch.zeros(n, 10, lh, lw)], 1)       # channels 6-15 zero
    enc = R.nchw_to_records(full, NAME[prec], dst.groups, 0)
    whole_storage(dst, before, enc, 16 // dst.cpr, f"downscale s={s}")
    got = dst.to_nchw(0, 6).cpu()
    assert torch.equal(R.bits(got), R.bits(G.store_round(want, NAME[prec])))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("s,h,w", KERNEL_SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_upscale_bits_and_whole_storage(gpu, precision, s, h, w, n):
    prec = _lib.PRECISIONS[precision]
    lh, lw = h // s, w // s
    cpr = _lib.chans_per_record(prec)
    f = G.pattern((n, cpr, lh, lw), 5 + s) * 9                   # flows of a few pixels; channels past 3 garbage
    src = H8Tensor.from_nchw(f.to(gpu), prec)
    stored = G.store_round(f[:, :4], NAME[prec]).numpy()
    want = torch.from_numpy(FS.upscale_np(stored, s))
    dst = R.GuardedH8(n, cpr, h, w, gpu, prec, seed=37)
    dst.zero_padding()
    before = dst.snapshot()
    status = torch.zeros(1, dtype=torch.int32, device=gpu)
    sv, dv = src.view(0, 4), dst.view(0, 4)
    _lib.check(_lib.lib().rrin_flow_upscale_h8(C.byref(sv), C.byref(dv), n, s, prec, status.data_ptr(),
                                               H.stream(gpu)), "rrin_flow_upscale_h8")
    torch.cuda.synchronize(gpu)
    assert int(status.item()) == 0
    full = torch.cat([want, torch.zeros(n, cpr - 4, h, w)], 1)    # a whole record: its other channels zero
    enc = R.nchw_to_records(full, NAME[prec], dst.groups, 0)
    whole_storage(dst, before, enc, 1, f"upscale s={s}")
    got = dst.to_nchw(0, 4).cpu()
    assert torch.equal(R.bits(got), R.bits(G.store_round(want, NAME[prec])))


@pytest.mark.parametrize("precision", ["fp32_split16", "fp16"])
def test_upscale_raises_the_range_flag(gpu, precision):
    """A low-res flow of 40000 becomes 80000 at s = 2: past fp16, the flag is set."""
    prec = _lib.PRECISIONS[precision]
    f = torch.full((1, 8, 16, 16), 40000.0)
    src = H8Tensor.from_nchw(f.to(gpu), prec)
    dst = H8Tensor(1, 8, 32, 32, gpu, prec)
    status = torch.zeros(1, dtype=torch.int32, device=gpu)
    sv, dv = src.view(0, 4), dst.view(0, 4)
    _lib.check(_lib.lib().rrin_flow_upscale_h8(C.byref(sv), C.byref(dv), 1, 2, prec, status.data_ptr(), H.stream(gpu)))
    torch.cuda.synchronize(gpu)
    assert int(status.item()) == 1


# ---- float whole forward -----------------------------------------------------------------------
FLOAT_CASES = [(2, (2, 32, 64), "0.5"), (2, (1, 64, 32), "tensor"), (4, (1, 64, 64), "0.5")]


@functools.lru_cache(maxsize=None)
def scaled_ref(s, n, h, w, tname):
    """float64 net_forward_scaled on net_contract's frames and "default" weights."""
    i0, i1 = NC.net_frames(n, h, w)
    t = NC.net_t(tname, n)
    sd = {k: v.double() for k, v in NC.net_state_dict("default").items()}
    with torch.no_grad():
        return FS.net_forward_scaled(sd, i0.double(), i1.double(), t.double() if isinstance(t, torch.Tensor) else t, s)


@pytest.mark.parametrize("s,size,tname", FLOAT_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_float_forward_against_the_scaled_reference(gpu, precision, s, size, tname):
    """engine.forward(flow_scale=s) against float64 net_forward_scaled: NET_GATE["default"] for the
    fp32-class precisions, FP16_MAXABS / FP16_PSNR for fp16 (figures printed before the asserts)."""
    n, h, w = size
    net = net_of(gpu, precision)
    i0, i1 = NC.net_frames(n, h, w)
    t = NC.net_t(tname, n)
    with torch.no_grad():
        got = net.engine().forward(i0.to(gpu), i1.to(gpu), t, flow_scale=s).cpu()
    net.check_range()
    ref = scaled_ref(s, n, h, w, tname)
    err, p = NC.maxabs(got, ref), NC.psnr(got, ref)
    print(f"flow_scale={s} {precision} {size} t={tname}: maxabs {err:.3e} psnr {p:.2f}")
    if precision == "fp16":
        assert err <= NC.FP16_MAXABS and p >= NC.FP16_PSNR, (err, p)
    else:
        assert err <= NC.NET_GATE["default"], err


# ---- frame paths -------------------------------------------------------------------------------
def frames(n, h0, w0, seed, dev, dtype=np.uint8, maxval=255):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, maxval + 1, (n, h0, w0, 3)).astype(dtype)
    return torch.from_numpy(a).to(dev)


def host_u8(net, f0, f1, t, s):
    """pad -> engine.forward(flow_scale=s) -> to_uint8_image -> crop"""
    dev = f0.device
    h0, w0 = f0.shape[1:3]
    i0 = cv.frames_u8_to_float(f0.cpu(), s).contiguous().to(dev)
    i1 = cv.frames_u8_to_float(f1.cpu(), s).contiguous().to(dev)
    out = net.engine().forward(i0, i1, t, flow_scale=s)
    meta = {"top": out.shape[2] - h0, "height": h0, "width": w0}
    return np.stack([cv.to_uint8_image(o, meta) for o in out.cpu()])


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("shape", [(37, 53), (64, 64)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_u8_equals_its_definition(gpu, precision, shape, s):
    net = net_of(gpu, precision)
    h0, w0 = shape
    f0, f1 = frames(2, h0, w0, 3, gpu), frames(2, h0, w0, 4, gpu)
    with torch.no_grad():
        want = host_u8(net, f0, f1, 0.25, s)
        got = net.forward_u8(f0, f1, 0.25, flow_scale=s)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    net.check_range()


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_yuv_equals_its_definition(gpu, precision, s):
    net = net_of(gpu, precision)
    h0, w0 = 38, 54
    rgb0, rgb1 = frames(2, h0, w0, 5, gpu), frames(2, h0, w0, 6, gpu)
    y0, y1 = Y.rgb_to_yuv(rgb0, "i420"), Y.rgb_to_yuv(rgb1, "i420")
    with torch.no_grad():
        want = Y.rgb_to_yuv(net.forward_u8(Y.yuv_to_rgb(y0, "i420"), Y.yuv_to_rgb(y1, "i420"), 0.5, flow_scale=s),
                            "i420")
        got = net.forward_yuv(y0, y1, 0.5, layout="i420", flow_scale=s)
    assert torch.equal(got, want)


def host_u16(net, f0, f1, t, depth, s):
    dev = f0.device
    h0, w0 = f0.shape[1:3]
    i0 = cv.frames_u16_to_float(f0.cpu(), depth, s).contiguous().to(dev)
    i1 = cv.frames_u16_to_float(f1.cpu(), depth, s).contiguous().to(dev)
    out = net.engine().forward(i0, i1, t, flow_scale=s)
    return cv.frames_float_to_u16(out.cpu(), h0, w0, depth)


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_u16_equals_its_definition(gpu, precision, s):
    net = net_of(gpu, precision)
    f0 = frames(2, 37, 53, 7, gpu, np.uint16, 4095)
    f1 = frames(2, 37, 53, 8, gpu, np.uint16, 4095)
    with torch.no_grad():
        want = host_u16(net, f0, f1, 0.5, 12, s)
        got = net.forward_u16(f0, f1, 0.5, depth=12, flow_scale=s)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_yuv16_equals_its_definition(gpu, precision, s):
    net = net_of(gpu, precision)
    h0, w0 = 37, 54
    rgb0 = frames(2, h0, w0, 9, gpu, np.uint16, 1023)
    rgb1 = frames(2, h0, w0, 10, gpu, np.uint16, 1023)
    y0, y1 = Y.rgb16_to_yuv(rgb0, "i422", depth=10), Y.rgb16_to_yuv(rgb1, "i422", depth=10)
    with torch.no_grad():
        mid = net.forward_u16(Y.yuv_to_rgb16(y0, "i422", depth=10), Y.yuv_to_rgb16(y1, "i422", depth=10), 0.5,
                              depth=10, flow_scale=s)
        want = Y.rgb16_to_yuv(mid, "i422", depth=10)
        got = net.forward_yuv16(y0, y1, 0.5, layout="i422", depth=10, flow_scale=s)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


# ---- items -------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_items_equal_single_forwards(gpu, precision):
    net = net_of(gpu, precision)
    stack = frames(3, 37, 53, 12, gpu)
    pair, ts = [0, 0, 1], [0.4, 0.8, 0.2]
    with torch.no_grad():
        got = net.interpolate_items_u8(stack, pair, ts, flow_scale=2)
        for k, (p, t) in enumerate(zip(pair, ts)):
            want = net.forward_u8(stack[p:p + 1], stack[p + 1:p + 2], t, flow_scale=2)[0]
            assert torch.equal(got[k], want), f"item {k}"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_interpolate_u8_equals_three_forwards(gpu, precision):
    net = net_of(gpu, precision)
    f0, f1 = frames(2, 37, 53, 13, gpu), frames(2, 37, 53, 14, gpu)
    ts = [0.25, 0.5, 0.75]
    with torch.no_grad():
        got = net.interpolate_u8(f0, f1, ts, flow_scale=2)
        for g, t in zip(got, ts):
            assert torch.equal(g, net.forward_u8(f0, f1, t, flow_scale=2)), f"t={t}"


# ---- reuse, unchanged behaviour, the gate --------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_kept_flow_is_never_reused_across_scales(gpu, precision):
    """At 64x64 the padded size is the same for every s: the two calls share a workspace."""
    net = net_of(gpu, precision)
    eng = net.engine()
    f0, f1 = frames(1, 64, 64, 15, gpu), frames(1, 64, 64, 16, gpu)
    with torch.no_grad():
        plain1, plain2 = eng.forward_u8(f0, f1, 0.5), eng.forward_u8(f0, f1, 0.5, flow_scale=2)
        assert not torch.equal(plain1, plain2)
        eng.forward_u8(f0, f1, 0.25, flow_scale=2)
        assert torch.equal(eng.forward_u8(f0, f1, 0.5, reuse_flow=True), plain1)
        assert torch.equal(eng.forward_u8(f0, f1, 0.5, flow_scale=2, reuse_flow=True), plain2)
        # the same scale does reuse, with the same bits
        eng.forward_u8(f0, f1, 0.25, flow_scale=2)
        assert torch.equal(eng.forward_u8(f0, f1, 0.5, flow_scale=2, reuse_flow=True), plain2)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_flow_scale_1_is_the_call_without_the_keyword(gpu, precision):
    net = net_of(gpu, precision)
    eng = net.engine()
    f0, f1 = frames(2, 37, 53, 17, gpu), frames(2, 37, 53, 18, gpu)
    i0, i1 = NC.net_frames(2, 32, 48)
    i0, i1 = i0.to(gpu), i1.to(gpu)
    e0, e1 = f0[:, :36, :52].contiguous(), f1[:, :36, :52].contiguous()   # even sizes for 4:2:0
    y0, y1 = Y.rgb_to_yuv(e0, "i420"), Y.rgb_to_yuv(e1, "i420")
    w0 = (f0.to(torch.int32) * 4).to(torch.int16).view(torch.uint16)
    w1 = (f1.to(torch.int32) * 4).to(torch.int16).view(torch.uint16)
    z0 = Y.rgb16_to_yuv((e0.to(torch.int32) * 4).to(torch.int16).view(torch.uint16), "i420", depth=10)
    z1 = Y.rgb16_to_yuv((e1.to(torch.int32) * 4).to(torch.int16).view(torch.uint16), "i420", depth=10)
    stack = frames(3, 37, 53, 19, gpu)
    with torch.no_grad():
        assert torch.equal(eng.forward(i0, i1, 0.5, flow_scale=1), eng.forward(i0, i1, 0.5))
        assert torch.equal(eng.forward_u8(f0, f1, 0.5, flow_scale=1), eng.forward_u8(f0, f1, 0.5))
        assert torch.equal(eng.forward_yuv(y0, y1, 0.5, layout="i420", flow_scale=1),
                           eng.forward_yuv(y0, y1, 0.5, layout="i420"))
        a, b = eng.forward_u16(w0, w1, 0.5, depth=10, flow_scale=1), eng.forward_u16(w0, w1, 0.5, depth=10)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        a = eng.forward_yuv16(z0, z1, 0.5, layout="i420", depth=10, flow_scale=1)
        b = eng.forward_yuv16(z0, z1, 0.5, layout="i420", depth=10)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        assert torch.equal(eng.interpolate_items_u8(stack, [0, 1], [0.5, 0.25], flow_scale=1),
                           eng.interpolate_items_u8(stack, [0, 1], [0.5, 0.25]))


def test_scene_gate_with_flow_scale(gpu):
    net = net_of(gpu, "fp32")
    f0, f1 = frames(3, 37, 53, 21, gpu), frames(3, 37, 53, 22, gpu)
    f1[1] = f0[1]                                   # a duplicate
    f1[2] = 255 - f0[2]                             # a cut
    f0[0] = (f0[0] // 4) + 64                       # a quiet pair
    f1[0] = f0[0] + 1
    with torch.no_grad():
        plain = net.forward_u8(f0, f1, 0.5, flow_scale=2)
        gated = net.forward_u8(f0, f1, 0.5, flow_scale=2, scene_threshold=20.0)
    assert net.last_gate.tolist() == [0, 1, 2]
    assert torch.equal(gated[0], plain[0])
    assert torch.equal(gated[1], f0[1]) and torch.equal(gated[2], f1[2])


def test_second_plans_do_not_crowd_the_workspace_cache(gpu):
    """A 4-stream flow_scale forward holds 4 parts and 4 second plans; the cache limit counts parts,
    so a 4-stream forward at another size leaves them (and their reuse_flow state) in place, and a
    shape that is evicted takes its second plans along."""
    net = Net()
    net.load_state_dict(NC.net_state_dict("default"), strict=True)
    net.precision = "fp16"
    eng = net.to(gpu).eval().engine()
    a0, a1 = frames(4, 32, 32, 27, gpu), frames(4, 32, 32, 28, gpu)
    b0, b1 = frames(4, 48, 48, 29, gpu), frames(4, 48, 48, 30, gpu)
    with torch.no_grad():
        first = eng.forward_u8(a0, a1, 0.25, streams=4, flow_scale=2)
        mine = [k for k in eng._ws if k[1:3] == (32, 32) or (isinstance(k[3], tuple) and k[3][2:4] == (32, 32))]
        assert len(mine) == 8 and eng.MAX_WORKSPACES == 8
        eng.forward_u8(b0, b1, 0.5, streams=4)
        assert all(k in eng._ws for k in mine)
        assert all(eng._flow_valid[k] == "u8|s2" for k in mine if not isinstance(k[3], tuple))
        assert torch.equal(eng.forward_u8(a0, a1, 0.25, streams=4, flow_scale=2, reuse_flow=True), first)
        eng.forward_u8(frames(4, 64, 64, 31, gpu), frames(4, 64, 64, 32, gpu), 0.5, streams=4)   # a third shape
        assert not any((isinstance(k[3], tuple) and k[3][2:4] == (48, 48)) or k[1:3] == (48, 48) for k in eng._ws)
        assert len([k for k in eng._ws if not isinstance(k[3], tuple)]) <= eng.MAX_WORKSPACES


def test_y4m_pipes_with_flow_scale(gpu):
    """interpolate_y4m and evaluate_y4m with a real Net at flow_scale=2, no scene gate: the written
    intermediate frames are forward_yuv(flow_scale=2)'s, the report records the scale and no gate."""
    import io

    from rrin_amd import y4m
    net = net_of(gpu, "fp32")
    w, h = 48, 38                                   # pads to 64 rows at s = 2, 48 at s = 1
    rgb = frames(5, h, w, 25, gpu)
    clip = Y.rgb_to_yuv(rgb, "i420")                # [5, 57, 48]
    src = io.BytesIO()
    wr = y4m.Writer(src, w, h, 24, 1)
    for f in clip.cpu().numpy():
        wr.write(f.reshape(-1))
    raw = src.getvalue()
    dst, logs = io.BytesIO(), []
    with torch.no_grad():
        assert cv.interpolate_y4m(net, io.BytesIO(raw), dst, 1, batch=2, log=logs.append, flow_scale=2) == 9
        want = net.forward_yuv(clip[:-1], clip[1:], 0.5, layout="i420", flow_scale=2).cpu().numpy()
        plain = net.forward_yuv(clip[:-1], clip[1:], 0.5, layout="i420").cpu().numpy()
    out = [np.asarray(f).reshape(-1) for f in y4m.Reader(io.BytesIO(dst.getvalue()))]
    assert len(out) == 9 and len(logs) == 1 and "scene gate" not in logs[0]
    for p in range(4):
        np.testing.assert_array_equal(out[2 * p], clip[p].cpu().numpy().reshape(-1))
        np.testing.assert_array_equal(out[2 * p + 1], want[p].reshape(-1))
    assert not np.array_equal(want, plain)
    with torch.no_grad():
        res = cv.evaluate_y4m(net, io.BytesIO(raw), hold=2, batch=2, log=logs.append, flow_scale=2)
        held = net.forward_yuv(clip[0:3:2], clip[2:5:2], 0.5, layout="i420", flow_scale=2)
        m = net.frame_metrics_yuv(held, clip[1:4:2], layout="i420")
    s = res["summary"]
    assert s["flow_scale"] == 2 and s["held_out"] == 2 and (s["cut_pairs"], s["duplicate_pairs"]) == (0, 0)
    assert [r["gate"] for r in res["rows"]] == [0, 0]
    assert [r["sse"] for r in res["rows"]] == m.sse.cpu().tolist()
    net.check_range()


def test_refusals(gpu):
    net = net_of(gpu, "fp32")
    f0 = frames(1, 32, 32, 23, gpu)
    with torch.no_grad():
        for bad in (0, 3, 8, 2.0, True, "2"):
            with pytest.raises(ValueError):
                net.forward_u8(f0, f0, 0.5, flow_scale=bad)
        x = torch.zeros(1, 3, 48, 64, device=gpu)
        with pytest.raises(RuntimeError):       # 48 is no multiple of 32
            net.engine().forward(x, x, 0.5, flow_scale=2)
        planar = Net()
        planar.load_state_dict(NC.net_state_dict("default"), strict=True)
        planar.precision = "fp32_planar"
        planar = planar.to(gpu).eval()
        x = torch.zeros(1, 3, 64, 64, device=gpu)
        with pytest.raises(RuntimeError, match="record-layout precision"):
            planar.engine().forward(x, x, 0.5, flow_scale=2)
