"""CPU: the frame-rate conversion schedule (rrin_amd.retime), the host checks of the item
forwards (engine.check_items, Net.interpolate_items_*), interpolate_y4m(fps_out=) with a host
stand-in model, and the argument validation of the ABI-25 entry points (nothing is launched)."""
import ctypes as C
import io
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

from rrin_amd import Net, _lib, retime, y4m
from rrin_amd import convert as cv
from rrin_amd.engine import check_items, item_coefficients, t_coefficients

FAKE = 1 << 30  # a fabricated non-null device pointer: never dereferenced
ALL = dict(depths=(8, 10, 12), chroma=("420", "422", "444"))
RATES = [(Fr(24), Fr(60)), (Fr(25), Fr(30)), (Fr(24000, 1001), Fr(60000, 1001)), (Fr(24), Fr(25)),
         (Fr(50), Fr(60)), (Fr(24), Fr(48))]


# ---- schedule ---------------------------------------------------------------------------------
def test_schedule_24_to_60_over_three_frames():
    # times 0, .4, .8, 1.2, 1.6, 2.0
    assert retime.schedule(3, Fr(24), Fr(60)) == [(0, Fr(0)), (0, Fr(2, 5)), (0, Fr(4, 5)), (1, Fr(1, 5)),
                                                  (1, Fr(3, 5)), (2, Fr(0))]
    assert [retime.is_passthrough(it) for it in retime.schedule(3, 24, 60)] == [True, False, False, False, False, True]


def test_schedule_25_to_30_over_26_frames():
    s = retime.schedule(26, Fr(25), Fr(30))
    assert len(s) == 31 and s[0] == (0, 0) and s[-1] == (25, 0)
    # output j at 5j/6: a pass-through every sixth output, five items per five pairs
    assert s[:7] == [(0, Fr(0)), (0, Fr(5, 6)), (1, Fr(2, 3)), (2, Fr(1, 2)), (3, Fr(1, 3)), (4, Fr(1, 6)), (5, Fr(0))]
    assert all(s[6 * k] == (5 * k, 0) for k in range(6))
    per_pair = [sum(1 for p, t in s if p == q and t != 0) for q in range(25)]
    assert per_pair == [1] * 25


def test_schedule_ntsc_film_to_5994_over_26_frames():
    s = retime.schedule(26, Fr(24000, 1001), Fr(60000, 1001))
    assert s == retime.schedule(26, Fr(24), Fr(60))  # the same ratio 2/5
    assert len(s) == 63
    per_pair = [sum(1 for p, t in s if p == q and t != 0) for q in range(25)]
    assert per_pair == [2, 2] * 12 + [2]   # 3, 2, 3, 2 outputs per pair, one of each 3 a pass-through
    assert [sum(1 for p, _ in s if p == q) for q in range(4)] == [3, 2, 3, 2]


def test_schedule_24_to_25_over_26_frames():
    s = retime.schedule(26, Fr(24), Fr(25))
    assert len(s) == 27   # floor(25 * 25 / 24) + 1
    assert s[1] == (0, Fr(24, 25)) and s[2] == (1, Fr(23, 25)) and s[25] == (24, Fr(0)) and s[26] == (24, Fr(24, 25))
    assert [sum(1 for p, t in s if p == q and t != 0) for q in range(25)] == [1] * 24 + [1]


def test_schedule_24_to_48_is_the_sf1_schedule():
    """interpolate_y4m(sf=1): per pair its first frame and one intermediate at ts = [i / (sf + 1)]."""
    sf = 1
    ts = [i / (sf + 1) for i in range(1, sf + 1)]
    s = retime.schedule(7, Fr(24), Fr(48))
    net = [(p, float(t)) for p, t in s if t != 0]
    assert net == [(p, t) for p in range(6) for t in ts]
    assert [p for p, t in s if t == 0] == list(range(7))


@pytest.mark.parametrize("fi,fo", RATES)
def test_schedule_properties(fi, fo):
    for n in range(2, 51):
        s = retime.schedule(n, fi, fo)
        assert len(s) == (n - 1) * fo // fi + 1
        times = [p + t for p, t in s]
        assert times == [j * fi / fo for j in range(len(s))]
        assert all(a < b for a, b in zip(times, times[1:]))
        assert all(a[0] <= b[0] for a, b in zip(s, s[1:]))
        assert all(0 <= t < 1 and 0 <= p <= n - 1 and (p < n - 1 or t == 0) for p, t in s)
        for q in range(n - 1):
            assert any(p == q and t != 0 for p, t in s), (n, q)


@pytest.mark.parametrize("fi,fo", RATES)
def test_stream_agrees_with_the_closed_form(fi, fo):
    st = retime.Stream(fi, fo)
    got = st.feed()
    assert got == [(0, 0)]
    for n in range(2, 51):
        new = next(st)
        got += new
        assert got == retime.schedule(n, fi, fo)
        # an item is complete when its last frame has arrived, not before
        assert all(p + (t != 0) == n - 1 for p, t in new)


def test_batches_cut_items_not_pairs():
    s = retime.schedule(6, 24, 60)   # 13 outputs, 3 pass-throughs (0, 2.0, 4.0), 10 items
    steps = list(retime.batches(s, 4))
    assert [len(b[2]) for b in steps] == [4, 4, 2]
    assert steps[0] == (0, 2, [0, 0, 1, 1], [0.4, 0.8, float(Fr(1, 5)), float(Fr(3, 5))])
    assert steps[1][:3] == (2, 4, [0, 0, 1, 1])
    assert steps[2][:3] == (4, 5, [0, 0])
    with pytest.raises(ValueError):
        list(retime.batches(s, 0))


def test_rates_and_frame_counts_are_validated():
    assert retime.as_rate("60000/1001") == Fr(60000, 1001) and retime.as_rate(" 60 ") == 60 == retime.as_rate(60)
    for bad in ("x", "1/0", "-3", 0):
        with pytest.raises(ValueError):
            retime.as_rate(bad)
    with pytest.raises(TypeError):
        retime.as_rate(59.94)
    for fo in (Fr(24), Fr(12), "24000/1001"):
        with pytest.raises(ValueError, match="decimation"):
            retime.schedule(5, Fr(24), fo)
        with pytest.raises(ValueError, match="decimation"):
            retime.Stream(Fr(24), fo)
    for n in (1, 0, -2, 2.0, True):
        with pytest.raises(ValueError, match="two frames"):
            retime.schedule(n, 24, 60)


# ---- the item batch's host checks ------------------------------------------------------------
def test_check_items():
    assert check_items([0, 0, 1, 2, 2], [0.1, 0.9, 0.5, 0.0, 0.25], 3) == ([0, 0, 1, 2, 2], [0.1, 0.9, 0.5, 0.0, 0.25])
    pl, ts = check_items(torch.tensor([0, 1], dtype=torch.int32), torch.tensor([0.5, 0.25]), 2)
    assert pl == [0, 1] and isinstance(ts, torch.Tensor) and ts.dtype == torch.float32
    for pair, t, n in [([0, 3], [0.5, 0.5], 3), ([-1, 0], [0.5, 0.5], 3), ([1, 0], [0.5, 0.5], 3),
                       ([0, 1], [0.5, 1.0], 3), ([0, 1], [-0.1, 0.5], 3), ([0, 1], [0.5, float("nan")], 3),
                       ([0, 1], [0.5], 3), ([], [], 3), ([0], [0.5], 0), ([0.0], [0.5], 3), ([True], [0.5], 3),
                       (torch.tensor([0]), [0.5], 3), ([0], torch.tensor([0.5], dtype=torch.float64), 3)]:
        with pytest.raises(ValueError):
            check_items(pair, t, n)


def test_item_coefficients_are_the_forwards_own():
    ts = [0.4, 0.8, float(Fr(1, 5)), 1 / 3]
    rows = item_coefficients(ts, 4)
    assert rows.shape == (4, 8) and rows.dtype == torch.float32
    for k, v in enumerate(ts):
        assert torch.equal(rows[k:k + 1], t_coefficients(v, 1))        # a Python float t
    tt = torch.tensor(ts, dtype=torch.float32)
    rows = item_coefficients(tt, 4)
    assert torch.equal(rows, t_coefficients(tt, 4))
    for k in range(4):
        assert torch.equal(rows[k:k + 1], t_coefficients(tt[k], 1))    # a 0-dim fp32 tensor t
    assert torch.equal(item_coefficients(tt[:1], 1), t_coefficients(tt[0], 1))


@pytest.mark.parametrize("name,shape,dtype", [("interpolate_items_u8", (4, 6, 8, 3), torch.uint8),
                                              ("interpolate_items_u16", (4, 6, 8, 3), torch.uint16),
                                              ("interpolate_items_yuv", (4, 9, 8), torch.uint8),
                                              ("interpolate_items_yuv16", (4, 9, 8), torch.uint16)])
def test_net_items_refuse_bad_batches_before_any_device_work(name, shape, dtype):
    """A Net on the host has no engine: a bad batch must raise ValueError before one is asked for."""
    net = Net().eval()
    frames = torch.zeros(shape, dtype=dtype)
    call = getattr(net, name)
    with torch.no_grad():
        for pair, t in [([0, 3], [0.5, 0.5]), ([1, 0], [0.5, 0.5]), ([0, 1], [0.5, 1.0]), ([0, 1], [-0.5, 0.5]),
                        ([0], [0.5, 0.5])]:
            with pytest.raises(ValueError):
                call(frames, pair, t)
        with pytest.raises(ValueError):
            call(frames[:1], [0], [0.5])          # one frame: no pair
        with pytest.raises(RuntimeError, match="ROCm"):
            call(frames, [0, 1], [0.5, 0.5])      # a good batch reaches the engine, which needs the device


# ---- interpolate_y4m(fps_out=) with a host model -----------------------------------------------
class HostItems(torch.nn.Module):
    """Stands in for Net: interpolate_items_yuv* is the definition -- item k is ``forward`` of its
    pair alone at its t -- over a fake forward that marks a frame with its t: f0 + round(100 t)."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    @staticmethod
    def forward_pair(f0, f1, t):
        assert f0.shape == f1.shape and f0.shape[0] == 1
        return (f0.to(torch.int32) + round(100 * t)).to(torch.int16).view(torch.uint16).to(f0.dtype)

    def _items(self, name, frames, pair, t, layout, **kw):
        check_items(pair, t, frames.shape[0] - 1)
        self.calls.append((name, tuple(frames.shape), frames.dtype, list(pair), list(t), layout, kw))
        return torch.cat([self.forward_pair(frames[p:p + 1], frames[p + 1:p + 2], v) for p, v in zip(pair, t)])

    def interpolate_items_yuv(self, frames, pair, t, layout="nv12", coef=None, **kw):
        return self._items("yuv", frames, pair, t, layout, **kw)

    def interpolate_items_yuv16(self, frames, pair, t, layout="nv12", depth=10, msb=False, coef=None, **kw):
        return self._items("yuv16", frames, pair, t, layout, depth=depth, msb=msb, **kw)


def y4m_bytes(frames, w, h, tag, fps=(24, 1)):
    src = io.BytesIO()
    wr = y4m.Writer(src, w, h, fps[0], fps[1], tag, **ALL)
    for f in frames:
        wr.write(f)
    src.seek(0)
    return src


@pytest.mark.parametrize("tag,chroma,depth", [("420", "420", 8), ("422p10", "422", 10), ("444", "444", 8)])
@pytest.mark.parametrize("fps_out,batch", [("60", 4), (Fr(60), 3), ("30000/1001", 4)])
def test_interpolate_y4m_fps_out(tag, chroma, depth, fps_out, batch):
    w, h = (6, 4) if chroma != "444" else (5, 3)
    samples = w * h * 3 // 2 if chroma == "420" else w * h * (2 if chroma == "422" else 3)
    rng = np.random.default_rng(12)
    frames = [rng.integers(0, 100, samples).astype(np.uint16 if depth > 8 else np.uint8) for _ in range(6)]
    dst = io.BytesIO()
    model = HostItems()
    logs = []
    rate = retime.as_rate(fps_out)
    sched = retime.schedule(6, Fr(24), rate)
    assert cv.interpolate_y4m(model, y4m_bytes(frames, w, h, tag), dst, fps_out=fps_out, batch=batch,
                              log=logs.append) == len(sched)
    rd = y4m.Reader(io.BytesIO(dst.getvalue()), **ALL)
    assert (rd.width, rd.height, rd.colorspace, rd.chroma, rd.bit_depth) == (w, h, tag, chroma, depth)
    assert (rd.fps_num, rd.fps_den) == (rate.numerator, rate.denominator)
    out = list(rd)
    assert len(out) == len(sched)
    for o, (p, t) in zip(out, sched):
        if t == 0:
            assert np.array_equal(o, frames[p])                         # a pass-through: the input's bytes
        else:
            assert np.array_equal(o, frames[p] + round(100 * float(t)))  # the item of pair p at t, in order
    # full batches of items until the stream ends, whatever the pairs
    n_items = sum(1 for _, t in sched if t != 0)
    assert [len(c[3]) for c in model.calls] == [batch] * (n_items // batch) + [n_items % batch] * (n_items % batch > 0)
    name = "yuv16" if depth > 8 else "yuv"
    rows = {"420": 3 * h // 2, "422": 2 * h, "444": 3 * h}[chroma]
    for c, (lo, hi, pair, ts) in zip(model.calls, retime.batches(sched, batch)):
        assert c[0] == name and c[1] == (hi - lo + 1, rows, w) and c[3] == pair and c[4] == ts and c[5] == "i" + chroma
        if depth > 8:
            assert c[6]["depth"] == depth and c[6]["msb"] is False
    assert len(logs) == 1 and "24:1 fps" in logs[0] and f"{rate.numerator}:{rate.denominator} fps" in logs[0]
    assert f"{sum(1 for _, t in sched if t == 0)} of them input frames passed through" in logs[0]


def test_interpolate_y4m_takes_exactly_one_of_sf_and_fps_out():
    frames = [np.zeros(36, np.uint8)] * 3
    for kw in ({}, {"sf": 1, "fps_out": "60"}):
        with pytest.raises(ValueError, match="exactly one"):
            cv.interpolate_y4m(HostItems(), y4m_bytes(frames, 6, 4, "420"), io.BytesIO(), log=lambda *a: None, **kw)
    with pytest.raises(ValueError, match="decimation"):
        cv.interpolate_y4m(HostItems(), y4m_bytes(frames, 6, 4, "420"), io.BytesIO(), fps_out="24", log=lambda *a: None)
    with pytest.raises(ValueError, match="two frames"):
        cv.interpolate_y4m(HostItems(), y4m_bytes(frames[:1], 6, 4, "420"), io.BytesIO(), fps_out="60",
                           log=lambda *a: None)


def test_cli_has_fps_out():
    from rrin_amd.__main__ import build_parser
    a = build_parser().parse_args(["--model_name", "M", "convert", "--sf", "0", "--fps", "0", "--y4m_in", "-",
                                   "--y4m_out", "-", "--fps_out", "60000/1001"])
    assert a.fps_out == "60000/1001" and a.sf == 0
    b = build_parser().parse_args(["--model_name", "M", "convert", "--sf", "1", "--fps", "0", "--y4m_in", "-",
                                   "--y4m_out", "-"])
    assert b.fps_out is None
    a.sf = 2
    with pytest.raises(Exception, match="--sf 0"):
        cv._convert_y4m(a)


# ---- ABI 25: validated on the host, before any HIP call --------------------------------------------
E_SHAPE, E_ARG = -1, -2


def _u8_desc(h0=38, w0=50, h=48, w=64, n=5, prec=_lib.PREC_F32R, stride=None):
    d = _lib.NetU8Desc()
    d.net.n, d.net.h, d.net.w, d.net.prec = n, h, w, prec
    d.net.coef = d.net.workspace = FAKE
    d.net.convs = C.cast(FAKE, C.POINTER(_lib.ConvWeights))
    d.net.heads = C.cast(FAKE, C.POINTER(_lib.HeadWeights))
    d.f0 = d.f1 = d.out_u8 = FAKE
    d.img_stride = h0 * w0 * 3 if stride is None else stride
    d.h0, d.w0 = h0, w0
    return d


def _items(n_pairs, mapped=True):
    return _lib.Items(n_pairs, 0, FAKE if mapped else None)


def test_abi_version_is_25():
    assert _lib.ABI_VERSION == 25 == _lib.lib().rrin_abi_version()


def test_net_u8_items_fwd_validates_before_any_launch():
    fwd = _lib.lib().rrin_net_u8_items_fwd
    assert fwd(C.byref(_u8_desc()), None, None) == E_ARG
    assert fwd(None, C.byref(_items(3)), None) == E_ARG
    assert fwd(C.byref(_u8_desc()), C.byref(_items(0)), None) == E_ARG              # n_pairs < 1
    assert fwd(C.byref(_u8_desc()), C.byref(_items(6)), None) == E_ARG              # n_pairs > n
    assert fwd(C.byref(_u8_desc()), C.byref(_items(3, mapped=False)), None) == E_ARG   # no map, n_pairs != n
    # the frame forward's own checks, the stride rule on the stacks' n_pairs frames
    assert fwd(C.byref(_u8_desc(h=32)), C.byref(_items(3)), None) == E_SHAPE
    assert fwd(C.byref(_u8_desc(h0=0, h=16)), C.byref(_items(3)), None) == E_SHAPE
    assert fwd(C.byref(_u8_desc(stride=38 * 50 * 3 - 1)), C.byref(_items(3)), None) == E_ARG
    assert fwd(C.byref(_u8_desc(prec=_lib.PREC_F32)), C.byref(_items(3)), None) == E_ARG
    d = _u8_desc()
    d.net.taps = FAKE
    assert fwd(C.byref(d), C.byref(_items(3)), None) == E_ARG
    d = _u8_desc()
    d.f1 = None
    assert fwd(C.byref(d), C.byref(_items(3)), None) == E_ARG
    # the ABI-24 entry is as it was: the stride rule on its n frames
    assert _lib.lib().rrin_net_u8_fwd(C.byref(_u8_desc(stride=38 * 50 * 3 - 1)), None) == E_ARG
    assert _lib.lib().rrin_net_u8_fwd(C.byref(_u8_desc(h=32)), None) == E_SHAPE


def _yuv_stack(h0, w0, stride=None):
    s = _lib.Yuv420()
    s.y, s.u = FAKE, FAKE + h0 * w0
    s.v, s.c_pitch, s.c_step = s.u + 1, w0, 2
    s.img_stride, s.y_pitch = (h0 * w0 * 3 // 2 if stride is None else stride), w0
    return s


def test_net_yuv_items_fwd_validates_before_any_launch():
    from rrin_amd import yuv
    fwd = _lib.lib().rrin_net_yuv_items_fwd

    def desc(h0=38, w0=50, h=48, w=64, n=5, in_stride=None, out_stride=None):
        d = _lib.NetYuvDesc()
        d.net.n, d.net.h, d.net.w, d.net.prec = n, h, w, _lib.PREC_F32R
        d.net.coef = d.net.workspace = FAKE
        d.net.convs = C.cast(FAKE, C.POINTER(_lib.ConvWeights))
        d.net.heads = C.cast(FAKE, C.POINTER(_lib.HeadWeights))
        d.f0, d.f1, d.out = _yuv_stack(h0, w0, in_stride), _yuv_stack(h0, w0, in_stride), _yuv_stack(h0, w0, out_stride)
        d.coef, d.h0, d.w0 = _lib.YuvCoef(*yuv.coefficients()), h0, w0
        return d

    assert fwd(C.byref(desc()), None, None) == E_ARG
    assert fwd(C.byref(desc()), C.byref(_items(0)), None) == E_ARG
    assert fwd(C.byref(desc()), C.byref(_items(6)), None) == E_ARG
    assert fwd(C.byref(desc()), C.byref(_items(4, mapped=False)), None) == E_ARG
    assert fwd(C.byref(desc(h0=37)), C.byref(_items(3)), None) == E_SHAPE                      # odd h0 at 4:2:0
    assert fwd(C.byref(desc(in_stride=38 * 50 - 1)), C.byref(_items(3)), None) == E_SHAPE      # input frames overlap
    assert fwd(C.byref(desc(out_stride=38 * 50 - 1)), C.byref(_items(3)), None) == E_SHAPE     # output frames overlap
    # the span rule of f0 / f1 is on n_pairs frames: one pair has no stride to check, the n outputs do
    assert fwd(C.byref(desc(out_stride=38 * 50 - 1)), C.byref(_items(1)), None) == E_SHAPE
    assert fwd(C.byref(desc(h=32)), C.byref(_items(3)), None) == E_SHAPE


def test_u16_and_yuv16_items_fwd_validate():
    L = _lib.lib()
    d = _lib.NetU16Desc()
    d.net.n, d.net.h, d.net.w, d.net.prec = 5, 48, 64, _lib.PREC_F32R
    d.net.coef = d.net.workspace = FAKE
    d.net.convs = C.cast(FAKE, C.POINTER(_lib.ConvWeights))
    d.net.heads = C.cast(FAKE, C.POINTER(_lib.HeadWeights))
    d.f0 = d.f1 = d.out_u16 = FAKE
    d.img_stride, d.h0, d.w0, d.depth = 38 * 50 * 3, 38, 50, 12
    assert L.rrin_net_u16_items_fwd(C.byref(d), None, None) == E_ARG
    assert L.rrin_net_u16_items_fwd(C.byref(d), C.byref(_items(6)), None) == E_ARG
    assert L.rrin_net_u16_items_fwd(C.byref(d), C.byref(_items(2, mapped=False)), None) == E_ARG
    d.depth = 8
    assert L.rrin_net_u16_items_fwd(C.byref(d), C.byref(_items(3)), None) == E_ARG
    d.depth, d.net.h = 12, 32
    assert L.rrin_net_u16_items_fwd(C.byref(d), C.byref(_items(3)), None) == E_SHAPE
    y = _lib.NetYuv16Desc()
    y.net.n, y.net.h, y.net.w, y.net.prec = 5, 48, 64, _lib.PREC_F32R
    assert L.rrin_net_yuv16_items_fwd(C.byref(y), None, None) == E_ARG
    assert L.rrin_net_yuv16_items_fwd(C.byref(y), C.byref(_items(0)), None) == E_ARG
    assert L.rrin_net_yuv16_items_fwd(C.byref(y), C.byref(_items(3)), None) == E_ARG   # no coef / workspace


def test_item_kernels_validate():
    L = _lib.lib()
    g = _lib.geom_h8(48, 64)
    fr = _lib.H8(FAKE, None, 1 * g.plane, 0, 1, g)
    g16 = _lib.H8(FAKE, None, 4 * g.plane, 0, 4, g)
    tb = L.rrin_flow_tblend_items_h8
    R = _lib.PREC_F32R
    assert tb(C.byref(fr), C.byref(g16), FAKE, 5, None, 3, R, None) == E_ARG          # no map
    assert tb(C.byref(fr), C.byref(g16), FAKE, 5, FAKE, 0, R, None) == E_ARG
    assert tb(C.byref(fr), C.byref(g16), FAKE, 5, FAKE, 6, R, None) == E_ARG
    assert tb(C.byref(fr), C.byref(g16), None, 5, FAKE, 3, R, None) == E_ARG
    assert tb(C.byref(fr), C.byref(g16), FAKE, 5, FAKE, 3, _lib.PREC_F32, None) == E_ARG
    small = _lib.H8(FAKE, None, 2 * g.plane, 0, 2, g)                                  # g16 of 8 channels
    assert tb(C.byref(fr), C.byref(small), FAKE, 5, FAKE, 3, R, None) == E_SHAPE
    gi = L.rrin_gate_items_u8
    assert gi(None, 3, FAKE, FAKE, 5, FAKE, None) == E_ARG
    assert gi(FAKE, 3, None, FAKE, 5, FAKE, None) == E_ARG
    assert gi(FAKE, 0, FAKE, FAKE, 5, FAKE, None) == E_ARG
    assert gi(FAKE, 6, FAKE, FAKE, 5, FAKE, None) == E_ARG
    gf = L.rrin_gate_frames_items_u8_len
    assert gf(FAKE, FAKE, 100, 5, 100, FAKE, FAKE, None, 3, None) == E_ARG
    assert gf(FAKE, FAKE, 100, 5, 100, FAKE, FAKE, FAKE, 6, None) == E_ARG
    assert gf(FAKE, FAKE, 99, 5, 100, FAKE, FAKE, FAKE, 3, None) == E_ARG
    assert gf(FAKE, FAKE, 100, 5, 0, FAKE, FAKE, FAKE, 3, None) == E_SHAPE
