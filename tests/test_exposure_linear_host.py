"""CPU: the linear-light synthetic shutter on the host -- the transfer tables and their integer encoding
(``rrin_amd.transfer``), the shutter weights and ``exposure.mean_frames_linear`` (the definition the
kernels are tested against), the keywords of ``convert.interpolate_y4m`` and the CLI, and the argument
checks of the two C entry points, which come before any launch.  No interior table value is pinned: a
table is an input of the definition, not a result."""
import io

import numpy as np
import pytest
import torch

from rrin_amd import Net, _lib, exposure, transfer, y4m, yuv
from rrin_amd import convert as cv
from rrin_amd.__main__ import build_parser
from rrin_amd.framefmt import FrameFormat

E_SHAPE, E_ARG = -1, -2
FORMATS = [(8, 0), (10, 0), (16, 0), (10, 6), (12, 4)]   # tests/test_exposure_host.py's list


def words(a, depth):
    """An integer array as a uint8 / uint16 tensor of the depth."""
    t = torch.as_tensor(np.asarray(a))
    return t.to(torch.uint8) if depth == 8 else t.to(torch.int32).to(torch.int16).view(torch.uint16)


def ints(t):
    return t.to(torch.int64) if t.dtype == torch.uint8 else (t.view(torch.int16).to(torch.int64) & 0xFFFF)


def flat_table(depth, seed):
    """A random non-decreasing table with flat runs, 0 .. 2**30."""
    rng = np.random.default_rng(seed)
    n = 1 << depth
    steps = rng.integers(0, 1 << 12, n) * (rng.random(n) < 0.6)      # about four entries in ten repeat
    lin = np.cumsum(steps)
    lin = lin * (1 << 30) // max(int(lin[-1]), 1)
    lin[0] = 0
    return torch.from_numpy(lin.astype(np.int64))


# ---- the tables ------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [8, 10, 12])
@pytest.mark.parametrize("name", transfer.NAMES)
def test_named_tables(name, depth):
    lin = transfer.table(name, depth)
    maxval = (1 << depth) - 1
    assert lin.dtype == torch.int64 and tuple(lin.shape) == (maxval + 1,)
    assert bool((lin[1:] >= lin[:-1]).all())
    assert int(lin[0]) == 0 and int(lin[maxval]) == 1 << 30
    thr = transfer.thresholds(lin)
    assert int(thr[0]) == 0 and torch.equal(thr[1:], (lin[:-1] + lin[1:] + 1) // 2)
    c = torch.arange(1, maxval)
    strict = c[(lin[c - 1] < lin[c]) & (lin[c] < lin[c + 1])]
    assert strict.numel() > maxval // 2
    assert torch.equal(transfer.encode(thr, lin[strict]), strict)
    assert torch.equal(transfer.as_table(name, depth), lin)


def test_as_table_refusals():
    good = list(range(0, 256 * 4, 4))
    assert torch.equal(transfer.as_table(good, 8), torch.tensor(good))
    assert torch.equal(transfer.as_table(torch.tensor(good, dtype=torch.int32), 8), torch.tensor(good))
    with pytest.raises(ValueError, match="one of"):
        transfer.as_table("rec709", 8)
    with pytest.raises(ValueError, match="entries"):
        transfer.as_table(good[:-1], 8)
    with pytest.raises(ValueError, match="entries"):
        transfer.as_table(torch.tensor(good), 10)
    with pytest.raises(ValueError, match="non-decreasing"):
        transfer.as_table(good[:100] + [good[99] - 1] + good[101:], 8)
    with pytest.raises(ValueError, match="2\\*\\*30"):
        transfer.as_table(good[:-1] + [(1 << 30) + 1], 8)
    with pytest.raises(ValueError, match="2\\*\\*30"):
        transfer.as_table([-1] + good[1:], 8)
    for depth in (13, 7, 16, True, 8.0):
        with pytest.raises(ValueError, match="8..12"):
            transfer.as_table("srgb", depth)
    with pytest.raises(ValueError, match="8..12"):
        transfer.table("srgb", 13)
    with pytest.raises(TypeError):
        transfer.as_table(torch.zeros(256), 8)


@pytest.mark.parametrize("depth", [8, 10, 12])
def test_encode_is_a_right_side_searchsorted(depth):
    lin = flat_table(depth, depth)
    assert bool((lin[1:] == lin[:-1]).any()) and int(lin[-1]) == 1 << 30
    lin = transfer.as_table(lin, depth)
    thr = transfer.thresholds(lin)
    rng = np.random.default_rng(depth + 1)
    v = torch.cat([torch.from_numpy(rng.integers(0, (1 << 30) + 1, 5000)), lin, thr[1:], thr[1:] - 1,
                   torch.tensor([0, 1 << 30])]).clamp_(0, 1 << 30)
    want = torch.searchsorted(thr[1:].contiguous(), v, right=True)
    assert torch.equal(transfer.encode(thr, v), want)
    count = (thr[1:][None, :] <= v[:64, None]).sum(dim=1)         # the written definition, by counting
    assert torch.equal(want[:64], count)


# ---- the weights -----------------------------------------------------------------------------------
def test_shutter_weights():
    assert exposure.shutter_weights("box", 5) == [1] * 5 == exposure.shutter_weights(None, 5)
    assert exposure.shutter_weights("triangle", 1) == [1]
    assert exposure.shutter_weights("triangle", 2) == [1, 1]
    assert exposure.shutter_weights("triangle", 5) == [1, 2, 3, 2, 1]
    assert exposure.shutter_weights("triangle", 8) == [1, 2, 3, 4, 4, 3, 2, 1]
    assert exposure.shutter_weights([3, 1, 65531], 3) == [3, 1, 65531]
    assert exposure.group_weights("triangle", [1, 3]) == [[1], [1, 2, 1]]
    with pytest.raises(ValueError, match="every"):
        exposure.group_weights([1, 2, 1], [3, 4])                 # groups of another length
    with pytest.raises(ValueError, match="above 65535"):
        exposure.shutter_weights([65535, 1], 2)
    with pytest.raises(ValueError, match="above 65535"):
        exposure.shutter_weights([32768, 32768], 2)
    assert sum(exposure.shutter_weights("triangle", 256)) == 128 * 129     # the largest named shutter: far inside
    for bad in ([0, 1], [1, 65536], [1.0, 2], [True, 1], "gauss", 3, b"box"):
        with pytest.raises(ValueError):
            exposure.shutter_weights(bad, 2)
    for s in (0, 257, True):
        with pytest.raises(ValueError):
            exposure.shutter_weights("box", s)


# ---- the definition --------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,shift", FORMATS)
@pytest.mark.parametrize("s", [1, 2, 3, 256])
def test_no_table_box_is_mean_frames(depth, shift, s):
    rng = np.random.default_rng(100 * depth + shift + s)
    frames = words(rng.integers(0, 256 if depth == 8 else 65536, (s, 5, 7)), depth)
    fmt = FrameFormat.samples(None, depth, shift)
    want = exposure.mean_frames(frames, depth, shift)
    for w in (None, "box", [1] * s):
        got = exposure.mean_frames_linear(frames, fmt, None, w)
        assert got.dtype == want.dtype and torch.equal(ints(got), ints(want))
    if depth <= 12 and s > 1:   # YUV without a table: per stored element, no colour conversion
        yf = FrameFormat.yuv("i420") if depth == 8 else FrameFormat.samples("i420", depth, shift)
        frames = words(rng.integers(0, 256 if depth == 8 else 65536, (s, 6, 4)), depth)
        assert torch.equal(ints(exposure.mean_frames_linear(frames, yf, None, None)),
                           ints(exposure.mean_frames(frames, depth, shift)))


@pytest.mark.parametrize("depth,shift", [(8, 0), (10, 0), (10, 6), (12, 4)])
@pytest.mark.parametrize("light", ["srgb", "pq", "flat"])
def test_identical_frames_come_back_where_the_table_is_strict(depth, shift, light):
    lin = flat_table(depth, 3) if light == "flat" else transfer.table(light, depth)
    maxval = (1 << depth) - 1
    rng = np.random.default_rng(depth)
    one = rng.integers(0, maxval + 1, (4, 9, 3))
    fmt = FrameFormat.samples(None, depth, shift)
    strict = torch.zeros(maxval + 1, dtype=torch.bool)
    strict[1:-1] = (lin[:-2] < lin[1:-1]) & (lin[1:-1] < lin[2:])
    for s, w in ((1, None), (3, "triangle"), (5, [7, 1, 1, 2, 9])):
        frames = words(np.stack([one << shift] * s), depth)
        got = ints(exposure.mean_frames_linear(frames, fmt, lin, w)) >> shift
        keep = strict[torch.from_numpy(one)]
        assert keep.any() and torch.equal(got[keep], torch.from_numpy(one)[keep])


def test_srgb_mean_of_black_and_white():
    frames = torch.stack([torch.zeros((4, 6, 3), dtype=torch.uint8), torch.full((4, 6, 3), 255, dtype=torch.uint8)])
    got = exposure.mean_frames_linear(frames, FrameFormat.u8(), "srgb", None)
    assert got.dtype == torch.uint8 and int(got.min()) == int(got.max()) and int(got[0, 0, 0]) in (187, 188)
    assert int(exposure.mean_frames_linear(frames, FrameFormat.u8(), None, None).unique()) == 128
    assert int(exposure.mean_frames(frames).unique()) == 128


@pytest.mark.parametrize("depth", [8, 10, 12])
def test_largest_weight_does_not_overflow(depth):
    maxval = (1 << depth) - 1
    fmt = FrameFormat.samples(None, depth, 0)
    top = words(np.full((1, 3, 5), maxval), depth)
    assert int(ints(exposure.mean_frames_linear(top, fmt, "srgb", [65535])).unique()) == maxval
    assert int(ints(exposure.mean_frames_linear(top, fmt, None, [65535])).unique()) == maxval
    many = words(np.full((255, 3, 5), maxval), depth)
    assert int(ints(exposure.mean_frames_linear(many, fmt, "pq", [257] * 255)).unique()) == maxval


def test_mean_frames_linear_refusals():
    f16 = torch.zeros((2, 4, 6, 3), dtype=torch.uint16)
    with pytest.raises(ValueError, match="LDS"):
        exposure.mean_frames_linear(f16, FrameFormat.u16(13, "t"), "srgb", None)
    with pytest.raises(ValueError, match="LDS"):
        exposure.mean_frames_linear(f16, FrameFormat.u16(16, "t"), list(range(65536)), None)
    exposure.mean_frames_linear(f16, FrameFormat.u16(16, "t"), None, "triangle")   # no table: any depth
    with pytest.raises(TypeError):
        exposure.mean_frames_linear(f16, FrameFormat.u8(), "srgb", None)
    with pytest.raises(ValueError):
        exposure.mean_frames_linear(f16, FrameFormat.u16(10, "t"), "srgb", [1, 2, 3])
    with pytest.raises(ValueError):
        exposure.mean_frames_linear(f16, FrameFormat.u16(10, "t"), "nope", None)
    with pytest.raises(ValueError, match="matrix"):
        exposure.mean_frames_linear(torch.zeros((2, 6, 4), dtype=torch.uint8), FrameFormat.samples("i420"), "srgb", None)


LAYOUT_SHAPES = {"nv12": (4, 6), "i420": (4, 6), "nv16": (3, 4), "i422": (3, 4), "i444": (3, 5)}


@pytest.mark.parametrize("layout", yuv.ALL_LAYOUTS)
@pytest.mark.parametrize("depth,msb", [(8, False), (10, False), (12, True)])
def test_yuv_definition(layout, depth, msb):
    h0, w0 = LAYOUT_SHAPES[layout]
    rows = yuv.stack_rows(h0, layout)
    fmt = FrameFormat.yuv(layout) if depth == 8 else FrameFormat.yuv16(layout, depth, msb)
    maxval, mid, shift = (1 << depth) - 1, 1 << (depth - 1), fmt.shift
    rng = np.random.default_rng(depth)
    frames = words(rng.integers(0, 256 if depth == 8 else 65536, (3, rows, w0)), depth)
    light = "srgb" if depth == 8 else "pq"
    got = exposure.mean_frames_linear(frames, fmt, light, "triangle")
    assert got.dtype == frames.dtype and tuple(got.shape) == (rows, w0)
    # by hand: RGB, the element rule at shift 0, back
    if depth == 8:
        rgb = yuv.yuv_to_rgb(frames, layout, fmt.coef)
        mean = exposure.mean_frames_linear(rgb, FrameFormat.u8(), light, "triangle")
        want = yuv.rgb_to_yuv(mean[None], layout, fmt.coef)[0]
    else:
        rgb = yuv.yuv_to_rgb16(frames, layout, fmt.coef, depth, msb)
        mean = exposure.mean_frames_linear(rgb, FrameFormat.u16(depth, "t"), light, "triangle")
        want = yuv.rgb16_to_yuv(mean[None], layout, fmt.coef, depth, msb)[0]
    assert torch.equal(ints(got), ints(want))
    # grey stays grey: U = V = mid whatever the lumas
    grey = np.full((3, rows, w0), mid << shift)
    grey[:, :h0] = rng.integers(0, maxval + 1, (3, h0, w0)) << shift
    out = ints(exposure.mean_frames_linear(words(grey, depth), fmt, light, None)) >> shift
    assert bool((out[h0:] == mid).all())
    # S = 1 under a strictly increasing table is one round trip through RGB
    lin = transfer.table("srgb", depth)
    assert bool((lin[1:] > lin[:-1]).all())
    one = exposure.mean_frames_linear(frames[:1], fmt, lin, None)
    back = (yuv.rgb_to_yuv(yuv.yuv_to_rgb(frames[:1], layout, fmt.coef), layout, fmt.coef) if depth == 8 else
            yuv.rgb16_to_yuv(yuv.yuv_to_rgb16(frames[:1], layout, fmt.coef, depth, msb), layout, fmt.coef, depth, msb))
    assert torch.equal(ints(one), ints(back[0]))


def test_expose_with_light_and_weights():
    rng = np.random.default_rng(2)
    frames = torch.from_numpy(rng.integers(0, 256, (3, 4, 5, 3), dtype=np.uint8))
    groups = [[(0, 0), (0, 0.5), (1, 0)], [(1, 0.25)], [(1, 0.5), (2, 0)]]

    def item(p, t):
        return ((frames[p].to(torch.int32) + frames[p + 1].to(torch.int32)) // 2).to(torch.uint8)

    plain = exposure.expose(frames, groups, item)
    assert torch.equal(exposure.expose(frames, groups, item, weights="box"), plain)
    got = exposure.expose(frames, groups, item, light="srgb", weights="triangle")
    for g, group in enumerate(groups):
        srcs = torch.stack([frames[p] if t == 0 else item(p, t) for p, t in group])
        assert torch.equal(got[g], exposure.mean_frames_linear(srcs, FrameFormat.u8(), "srgb", "triangle"))
    with pytest.raises(ValueError):
        exposure.expose(frames, groups, item, weights=[1, 2, 1])      # groups of 3, 1 and 2 samples
    with pytest.raises(ValueError):
        exposure.expose(frames, groups, item, light="linear")


# ---- keywords, the pipe with a host model, the CLI -------------------------------------------------
class HostLinear(torch.nn.Module):
    """Stands in for Net: expose_items_yuv* is ``exposure.expose`` over a fake item forward (the rounded mean
    of the pair's frames), with the call's ``light`` and ``weights``."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    @staticmethod
    def item(frames, p):
        return ((ints(frames[p]) + ints(frames[p + 1]) + 1) // 2).to(torch.int16).view(torch.uint16).to(frames.dtype)

    def _expose(self, fmt, frames, groups, light, weights):
        self.calls.append((light, weights))
        return exposure.expose(frames, groups, lambda p, t: self.item(frames, p), fmt.depth, fmt.shift, light=light,
                               weights=weights, fmt=fmt)

    def expose_items_yuv(self, frames, groups, chunk=4, layout="nv12", coef=None, light=None, weights=None):
        return self._expose(FrameFormat.yuv(layout, coef), frames, groups, light, weights)

    def expose_items_yuv16(self, frames, groups, chunk=4, layout="nv12", depth=10, msb=False, coef=None, light=None,
                           weights=None):
        return self._expose(FrameFormat.yuv16(layout, depth, msb, coef), frames, groups, light, weights)


def clip(n, w, h, depth, fps=60):
    rng = np.random.default_rng(n + depth)
    frames = [rng.integers(0, 1 << depth, w * h * 3 // 2).astype(np.uint16 if depth > 8 else np.uint8)
              for _ in range(n)]
    src = io.BytesIO()
    wr = y4m.Writer(src, w, h, fps, 1, "420" if depth == 8 else f"420p{depth}", depths=(8, 10, 12))
    for f in frames:
        wr.write(f)
    return frames, src


def test_y4m_keywords():
    def run(**kw):
        _, src = clip(6, 6, 4, 8)
        src.seek(0)
        return cv.interpolate_y4m(HostLinear(), src, io.BytesIO(), log=lambda m: None, **kw)

    with pytest.raises(ValueError, match="need samples"):
        run(fps_out=120, light="srgb")
    with pytest.raises(ValueError, match="need samples"):
        run(sf=1, weights="triangle")
    with pytest.raises(ValueError, match="samples > 1"):
        run(fps_out=24, samples=1, light="srgb")
    with pytest.raises(ValueError, match="samples > 1"):
        run(fps_out=120, samples=1, weights="box")
    with pytest.raises(ValueError, match="one of"):
        run(fps_out=24, samples=2, light="rec709")
    with pytest.raises(ValueError):
        run(fps_out=24, samples=2, weights=[1, 2, 3])
    with pytest.raises(ValueError, match="entries"):
        run(fps_out=24, samples=2, light=list(range(1024)))        # a 10-bit table on an 8-bit stream
    assert run(fps_out=24, samples=2, light="srgb", weights="triangle") == 2


@pytest.mark.parametrize("depth", [8, 10])
def test_expose_y4m_passes_light_and_weights(depth):
    from rrin_amd import retime
    frames, src = clip(9, 6, 4, depth)
    outs, heads, logs = {}, {}, []
    for light, weights in ((None, None), ("srgb", "triangle")):
        src.seek(0)
        dst, model = io.BytesIO(), HostLinear()
        kw = {} if light is None else {"light": light, "weights": weights}
        assert cv.expose_y4m(model, src, dst, 24, 4, batch=3, log=logs.append, **kw) == 3
        raw = dst.getvalue()
        heads[light] = raw[:raw.index(b"\n")]
        outs[light] = list(y4m.Reader(io.BytesIO(raw), depths=(8, 10, 12)))
        assert all(c == (light, weights) for c in model.calls) and model.calls
    assert heads[None] == heads["srgb"]                             # the same header with and without light
    assert any(not np.array_equal(a, b) for a, b in zip(outs[None], outs["srgb"]))
    fmt = FrameFormat.yuv("i420") if depth == 8 else FrameFormat.yuv16("i420", depth)
    stack = words(np.stack(frames).reshape(9, 6, 6), depth)
    for o, output in zip(outs["srgb"], retime.exposure_schedule(9, 60, 24, "1/2", 4)):
        srcs = torch.stack([stack[p] if t == 0 else HostLinear.item(stack, p) for p, t in output])
        want = exposure.mean_frames_linear(srcs, fmt, "srgb", "triangle")
        assert np.array_equal(o.astype(np.int64), ints(want).numpy().reshape(-1))
    assert "linear light under srgb, triangle weights" in logs[1] and "linear light" not in logs[0]


def test_cli_parses_light_and_shutter_weights():
    base = ["--model_name", "m", "convert", "--sf", "0", "--fps", "24", "--y4m_in", "-", "--y4m_out", "-",
            "--fps_out", "24", "--samples", "8"]
    args = build_parser().parse_args(base)
    assert args.light is None and args.shutter_weights is None
    for name in transfer.NAMES:
        assert build_parser().parse_args(base + ["--light", name]).light == name
    for kind in exposure.SHUTTERS:
        assert build_parser().parse_args(base + ["--shutter_weights", kind]).shutter_weights == kind
    for bad in (["--light", "rec709"], ["--light", "linear"], ["--shutter_weights", "gauss"], ["--light"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(base + bad)


@pytest.mark.parametrize("name,shape,dtype,kw", [("expose_items_u8", (4, 6, 8, 3), torch.uint8, {}),
                                                 ("expose_items_u16", (4, 6, 8, 3), torch.uint16, {"depth": 12}),
                                                 ("expose_items_yuv", (4, 9, 8), torch.uint8, {}),
                                                 ("expose_items_yuv16", (4, 9, 8), torch.uint16, {})])
def test_net_refuses_bad_light_and_weights_before_any_device_work(name, shape, dtype, kw):
    """A Net on the host has no engine: bad keywords must raise before one is asked for."""
    net = Net().eval()
    frames = torch.zeros(shape, dtype=dtype)
    call = getattr(net, name)
    groups = [[(0, 0.5), (1, 0)], [(1, 0.5), (2, 0)]]
    with torch.no_grad():
        for bad in ("rec709", [0] * 5, 7):
            with pytest.raises(ValueError):
                call(frames, groups, light=bad, **kw)
        for bad in ("gauss", [1, 2, 3], [0, 1], [65535, 1]):
            with pytest.raises(ValueError):
                call(frames, groups, weights=bad, **kw)
        with pytest.raises(RuntimeError, match="ROCm"):
            call(frames, groups, light="srgb", weights="triangle", **kw)   # good keywords reach the engine
    if name == "expose_items_u16":
        with torch.no_grad(), pytest.raises(ValueError, match="LDS"):
            call(frames, groups, light="srgb", depth=14)


# ---- the C ABI: every refusal comes before any launch ----------------------------------------------
def test_abi_version_stays_25_with_the_new_entries():
    assert _lib.ABI_VERSION == 25 == _lib.lib().rrin_abi_version()
    assert {"rrin_mean_frames_lut", "rrin_mean_frames_yuv_lut"} <= set(_lib.SIGNATURES)


def test_rrin_mean_frames_lut_argument_checks():
    """Fabricated addresses: every call below must return its code without touching them."""
    fn = _lib.lib().rrin_mean_frames_lut
    tab, st, out, wt, lut = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000

    def run(frames=tab, k=4, start=st, g=2, o=out, stride=64, length=36, depth=8, shift=0, access=4, weights=wt,
            table=lut):
        return fn(frames, k, start, g, o, stride, length, depth, shift, access, weights, table, None)

    assert run(frames=None) == E_ARG and run(start=None) == E_ARG and run(o=None) == E_ARG
    assert run(weights=None) == E_ARG and run(weights=wt + 2) == E_ARG
    assert run(g=0) == E_SHAPE and run(length=0) == E_SHAPE and run(g=65536, k=65536) == E_SHAPE
    for depth, shift in ((7, 0), (17, 0), (8, 1), (10, 7), (12, 5), (16, 1), (10, -1)):
        assert run(depth=depth, shift=shift, table=None) == E_ARG, (depth, shift)
    assert run(depth=13, access=4) == E_ARG and run(depth=16, access=4) == E_ARG    # a table above 12 bits
    assert run(table=lut + 4) == E_ARG                                              # the table is read 16 bytes wide
    assert run(depth=10, o=out + 1, access=2) == E_ARG                              # an odd 16-bit address
    assert run(depth=10, o=out + 2, access=4) == E_ARG and run(o=out + 4, access=16) == E_ARG
    assert run(stride=66, access=4) == E_ARG and run(stride=72, access=16) == E_ARG
    assert run(stride=35) == E_ARG                                                  # frames would overlap
    for access in (0, 2, 3, 8, 32, -4):
        assert run(access=access) == E_ARG, access
    assert run(frames=tab + 4) == E_ARG and run(start=st + 2) == E_ARG
    assert run(k=1) == E_ARG and run(k=513) == E_ARG


def test_rrin_mean_frames_yuv_lut_argument_checks():
    fn = _lib.lib().rrin_mean_frames_yuv_lut
    tab, st, out, wt, lut = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    coef8 = _lib.YuvCoef(*yuv.coefficients())
    coef10 = _lib.YuvCoef(*yuv.coefficients(depth=10))

    def run(frames=tab, k=4, start=st, g=2, o=out, stride=None, h0=4, w0=6, weights=wt, table=lut, layout="i420",
            depth=8, shift=0, coef=None, **over):
        from rrin_amd.framefmt import _stack_geometry
        uo, vo, c_pitch, c_step, chroma = _stack_geometry(layout, 1, h0 // 2 * 2 if layout in yuv.LAYOUTS else h0,
                                                          w0 // 2 * 2 if layout != "i444" else w0)
        geom = dict(u_off=uo, v_off=vo, y_pitch=w0, c_pitch=c_pitch, c_step=c_step, chroma=chroma, depth=depth,
                    shift=shift)
        geom.update(over)
        coef = (coef8 if depth == 8 else coef10) if coef is None else coef
        stride = 3 * h0 * w0 if stride is None else stride
        import ctypes as C
        return fn(frames, k, start, g, o, stride, C.byref(_lib.YuvPlanes(**geom)), C.byref(coef) if coef else None,
                  h0, w0, weights, table, None)

    assert run(table=None) == E_ARG                                     # the YUV entry has no table-less form
    assert run(frames=None) == E_ARG and run(start=None) == E_ARG and run(o=None) == E_ARG
    assert run(weights=None) == E_ARG and run(coef=False) == E_ARG
    assert run(table=lut + 8) == E_ARG and run(weights=wt + 1) == E_ARG and run(frames=tab + 4) == E_ARG
    for depth, shift in ((9, 0), (13, 0), (16, 0), (8, 1), (10, 5), (12, 6)):
        assert run(depth=depth, shift=shift) == E_ARG, (depth, shift)
    assert run(depth=10, o=out + 1) == E_ARG                            # an odd word address
    assert run(c_step=3) == E_ARG and run(chroma=3) == E_ARG
    bad = _lib.YuvCoef(*yuv.coefficients())
    bad.ay = 1 << 16
    assert run(coef=bad) == E_ARG
    assert run(w0=5) == E_SHAPE and run(h0=3) == E_SHAPE                # odd sizes at 4:2:0
    assert run(layout="i422", w0=5) == E_SHAPE and run(layout="i444", w0=0) == E_SHAPE
    assert run(g=0) == E_SHAPE and run(g=65536, k=65536) == E_SHAPE
    assert run(k=1) == E_ARG and run(k=513) == E_ARG
    assert run(y_pitch=5) == E_SHAPE and run(c_pitch=2) == E_SHAPE
    assert run(u_off=23) == E_SHAPE and run(v_off=24) == E_SHAPE and run(v_off=29) == E_SHAPE   # planes overlap
    assert run(stride=35) == E_SHAPE                                    # output frames overlap
