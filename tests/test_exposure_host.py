"""The synthetic shutter on the host: the schedule of any output rate with ``S`` samples per output
(``retime.exposure_schedule`` / ``ExposureStream`` / ``as_shutter``), the definition of the exposed frame
(``exposure.mean_frames``), ``convert.expose_y4m`` with a host model, the keywords and the CLI, and the
argument checks of ``rrin_mean_frames``.  No GPU."""
import io
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

from rrin_amd import Net, _lib, exposure, retime, y4m
from rrin_amd import convert as cv
from rrin_amd.__main__ import build_parser

ALL = dict(depths=(8, 10, 12), chroma=("420", "422", "444"))
E_SHAPE, E_ARG = -1, -2


# ---- the schedule --------------------------------------------------------------------------------
def test_schedule_60_to_24_half_shutter_four_samples_by_hand():
    """step = 5/2 input frames, window 5/4, sub-step 5/16: output j samples 5j/2 + k 5/16."""
    want = [[(0, Fr(0)), (0, Fr(5, 16)), (0, Fr(5, 8)), (0, Fr(15, 16))],
            [(2, Fr(1, 2)), (2, Fr(13, 16)), (3, Fr(1, 8)), (3, Fr(7, 16))],
            [(5, Fr(0)), (5, Fr(5, 16)), (5, Fr(5, 8)), (5, Fr(15, 16))]]
    assert retime.exposure_schedule(7, 60, 24, Fr(1, 2), 4) == want
    assert retime.exposure_schedule(6, 60, 24, "1/2", 4) == want[:2]   # output 2 ends at 5 + 15/16 > 5
    assert retime.exposure_schedule(4, 60, 24, "1/2", 4) == want[:1]   # output 1 ends at 3 + 7/16 > 3
    assert retime.exposure_schedule(5, 60, 24, "1/2", 4) == want[:2]
    assert retime.exposure_schedule(1, 60, 24, "1/2", 4) == []         # the first window does not fit
    assert retime.exposure_schedule(1, 60, 24, "1/2", 1) == [[(0, Fr(0))]]


@pytest.mark.parametrize("fo", [25, 30, 60, "60000/1001", Fr(48)])
@pytest.mark.parametrize("sh", [1, Fr(1, 2), "1/3"])
def test_one_sample_is_the_point_schedule(fo, sh):
    for n in (2, 3, 7, 12):
        assert retime.exposure_schedule(n, 24, fo, sh, 1) == [[it] for it in retime.schedule(n, 24, fo)]


RATES = [(60, 24, Fr(1, 2), 4), (120, 24, 1, 5), (25, 25, 1, 3), (24, 60, Fr(1, 2), 2), ("60000/1001", 50, "1/2", 8),
         (30, 25, Fr(1, 3), 7), (24, 60, 1, 1), (50, 50, "1/7", 1), (24, 1000, 1, 256)]


@pytest.mark.parametrize("fi,fo,sh,s", RATES)
def test_count_times_and_stream(fi, fo, sh, s):
    """The closed-form count, checked against the rule it is derived from; flattened times never
    decrease; every t in [0, 1); the stream, fed n frames, has returned exactly the schedule of n."""
    step = retime.as_rate(fi) / retime.as_rate(fo)
    sub = retime.as_shutter(sh) * step / s
    stream, got = retime.ExposureStream(fi, fo, sh, s), []
    for n in range(1, 14):
        sched = retime.exposure_schedule(n, fi, fo, sh, s)
        count = 0
        while count * step + (s - 1) * sub <= n - 1:   # the definition: the last sample is on the stream
            count += 1
        assert len(sched) == count == retime.exposure_count(n, fi, fo, sh, s)
        flat = [p + t for out in sched for p, t in out]
        assert all(len(out) == s for out in sched)
        assert flat == sorted(flat)
        assert flat == [j * step + k * sub for j in range(count) for k in range(s)]
        assert all(0 <= t < 1 and isinstance(p, int) and 0 <= p <= n - 1 for out in sched for p, t in out)
        assert all(p < n - 1 or t == 0 for out in sched for p, t in out)  # (n - 1, 0) is legal, nothing later
        got += stream.feed()
        assert got == sched
    assert stream.frames == 13 and stream.outputs == len(got)


def test_as_shutter():
    assert retime.as_shutter("1/2") == Fr(1, 2) == retime.as_shutter(Fr(1, 2))
    assert retime.as_shutter(1) == 1 == retime.as_shutter(" 1 ")
    for bad in (0.5, 1.0, True):
        with pytest.raises(TypeError):
            retime.as_shutter(bad)
    for bad in (0, "0", Fr(3, 2), 2, "-1/2", "half", "1/0", "", None):
        with pytest.raises(ValueError):
            retime.as_shutter(bad)
    for bad in (0, 257, True, 2.0, "4", None):
        with pytest.raises(ValueError):
            retime.exposure_schedule(5, 60, 24, "1/2", bad)
    with pytest.raises(ValueError):
        retime.exposure_schedule(0, 60, 24, "1/2", 2)
    # the point schedule's refusals are what they were
    with pytest.raises(ValueError, match="decimation is out of scope"):
        retime.schedule(5, 60, 24)
    with pytest.raises(ValueError, match="decimation is out of scope"):
        retime.Stream(24, 24)


# ---- the definition ------------------------------------------------------------------------------
def np_mean(stack: np.ndarray, depth: int, shift: int) -> np.ndarray:
    """Plain int64 arithmetic: ((sum of min(word >> shift, maxval)) + S // 2) // S << shift."""
    s = stack.shape[0]
    v = np.minimum(stack.astype(np.int64) >> shift, (1 << depth) - 1)
    return (((v.sum(axis=0) + s // 2) // s) << shift).astype(stack.dtype)


def as_torch(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(a.view(np.int16)).view(torch.uint16) if a.dtype == np.uint16 else torch.from_numpy(a)


def as_numpy(t: torch.Tensor) -> np.ndarray:
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.uint16 else t.numpy()


FORMATS = [(8, 0), (10, 0), (16, 0), (10, 6), (12, 4)]


@pytest.mark.parametrize("depth,shift", FORMATS)
@pytest.mark.parametrize("s", [1, 2, 3, 4, 7, 256])
def test_mean_frames_is_the_integer_formula(depth, shift, s):
    rng = np.random.default_rng(100 * depth + s)
    dt = np.uint8 if depth == 8 else np.uint16
    stack = rng.integers(0, 256 if depth == 8 else 65536, (s, 5, 7), dtype=np.int64).astype(dt)  # words above maxval too
    got = exposure.mean_frames(as_torch(stack), depth, shift)
    assert got.dtype == (torch.uint8 if depth == 8 else torch.uint16) and tuple(got.shape) == (5, 7)
    assert np.array_equal(as_numpy(got), np_mean(stack, depth, shift))


@pytest.mark.parametrize("depth,shift", FORMATS)
def test_mean_frames_ties_clamp_and_full_sums(depth, shift):
    dt = np.uint8 if depth == 8 else np.uint16
    maxval = (1 << depth) - 1

    def mean(rows):
        a = (np.array(rows, dtype=np.int64) << shift).astype(dt)
        return (as_numpy(exposure.mean_frames(as_torch(a), depth, shift)).astype(np.int64) >> shift).tolist()

    assert mean([[0], [1]]) == [1]                                           # 1/2 rounds up
    assert mean([[1, 1, 1], [0, 1, 1], [0, 0, 1], [0, 0, 0]]) == [0, 1, 1]   # sums 1, 2, 3 over 4: 0, 1 (tie), 1
    assert mean([[maxval]] * 256) == [maxval]                                # the largest sum there is
    assert mean([[maxval]] * 255 + [[0]]) == [maxval - (maxval + 128) // 256]
    if 8 < depth < 16:  # a word above maxval reads as maxval, whatever lies in its other bits
        over = np.full((2, 3), 0xFFFF, dtype=np.uint16)
        over[1] = np.array([0, 1, 2], dtype=np.uint16) << shift
        want = [(maxval + v + 1) // 2 << shift for v in (0, 1, 2)]
        assert as_numpy(exposure.mean_frames(as_torch(over), depth, shift)).tolist() == want


def test_mean_frames_refusals():
    with pytest.raises(ValueError):
        exposure.mean_frames(torch.zeros((257, 4), dtype=torch.uint8))
    with pytest.raises(ValueError):
        exposure.mean_frames(torch.zeros((0, 4), dtype=torch.uint8))
    with pytest.raises(TypeError):
        exposure.mean_frames(torch.zeros((2, 4), dtype=torch.uint8), 10, 0)
    with pytest.raises(ValueError):
        exposure.mean_frames(torch.zeros((2, 4), dtype=torch.uint16), 10, 7)


def test_check_groups_and_chunks():
    ok = [[(0, 0), (0, 0.25)], [(0, Fr(1, 2)), (1, 0.0)], [(2, 0.5)], [(3, 0)]]
    groups = exposure.check_groups(ok, 3)
    assert groups == [[(0, 0.0), (0, 0.25)], [(0, 0.5), (1, 0.0)], [(2, 0.5)], [(3, 0.0)]]
    assert exposure.chunks(groups, 2) == [(0, 1, [0, 0], [0.25, 0.5]), (2, 3, [0], [0.5])]
    assert exposure.chunks(groups, 5) == [(0, 3, [0, 0, 2], [0.25, 0.5, 0.5])]
    assert exposure.chunks([[(1, 0.0)]], 4) == []
    for bad in ([], [[]], [[(0, 0.5)] * 257], [[(0, 1.0)]], [[(0, -0.1)]], [[(3, 0.5)]], [[(4, 0)]], [[(-1, 0)]],
                [[(1, 0.5), (1, 0.25)]], [[(1, 0.5)], [(0, 0.75)]], [[(0.0, 0.5)]], [[(True, 0.5)]], [[(0, "0.5")]]):
        with pytest.raises(ValueError):
            exposure.check_groups(bad, 3)
    for bad in (None, 5, "ab", [5], [[5]], [[(0, 0.5, 1)]], torch.zeros(2)):
        with pytest.raises(TypeError):
            exposure.check_groups(bad, 3)
    for bad in (0, -1, True, 2.0, None):
        with pytest.raises(ValueError):
            exposure.chunks(groups, bad)


# ---- expose_y4m with a host model --------------------------------------------------------------
class HostExpose(torch.nn.Module):
    """Stands in for Net: expose_items_yuv* is the definition (``exposure.expose``) over a fake item forward
    that marks a frame with its t: f0 + round(100 t)."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    @staticmethod
    def item(frames, pair, t):
        assert 0 <= pair < frames.shape[0] - 1 and 0.0 < t < 1.0
        return (frames[pair].to(torch.int32) + round(100 * t)).to(torch.int16).view(torch.uint16).to(frames.dtype)

    def _expose(self, name, frames, groups, chunk, layout, depth=8, **kw):
        self.calls.append((name, tuple(frames.shape), frames.dtype, [list(g) for g in groups], chunk, layout, dict(kw, depth=depth)))
        return exposure.expose(frames, groups, lambda p, t: self.item(frames, p, t), depth, 0)

    def expose_items_yuv(self, frames, groups, chunk=4, layout="nv12", coef=None, **kw):
        return self._expose("yuv", frames, groups, chunk, layout, **kw)

    def expose_items_yuv16(self, frames, groups, chunk=4, layout="nv12", depth=10, msb=False, coef=None, **kw):
        assert msb is False
        return self._expose("yuv16", frames, groups, chunk, layout, depth=depth, **kw)


def y4m_bytes(frames, w, h, tag, fps):
    src = io.BytesIO()
    wr = y4m.Writer(src, w, h, fps[0], fps[1], tag, **ALL)
    for f in frames:
        wr.write(f)
    src.seek(0)
    return src


def expected_stream(frames, sched):
    """The definition applied to the schedule with HostExpose's items, in numpy."""
    out = []
    for output in sched:
        srcs = [frames[p].astype(np.int64) + (round(100 * float(t)) if t != 0 else 0) for p, t in output]
        s = len(srcs)
        out.append(((np.sum(srcs, axis=0) + s // 2) // s).astype(frames[0].dtype))
    return out


@pytest.mark.parametrize("tag,chroma,depth", [("420", "420", 8), ("422", "422", 8), ("444", "444", 8),
                                              ("420p10", "420", 10), ("444p12", "444", 12)])
@pytest.mark.parametrize("fps_in,fps_out,s,batch", [(60, 24, 4, 3), (25, 25, 3, 4), (24, 60, 2, 3), (24, 60, 1, 4),
                                                    (120, "24", 2, 1)])
def test_expose_y4m_is_the_definition_on_the_schedule(tag, chroma, depth, fps_in, fps_out, s, batch):
    w, h = (6, 4) if chroma != "444" else (5, 3)
    n = 13 if fps_in == 120 else 9
    samples = w * h * 3 // 2 if chroma == "420" else w * h * (2 if chroma == "422" else 3)
    rng = np.random.default_rng(7)
    frames = [rng.integers(0, 100, samples).astype(np.uint16 if depth > 8 else np.uint8) for _ in range(n)]
    sched = retime.exposure_schedule(n, fps_in, fps_out, "1/2", s)
    dst, model, logs = io.BytesIO(), HostExpose(), []
    kw = {} if s == 4 else {"shutter": Fr(1, 2)}   # 1/2 is the default with samples
    assert cv.interpolate_y4m(model, y4m_bytes(frames, w, h, tag, (fps_in, 1)), dst, fps_out=fps_out, samples=s,
                              batch=batch, log=logs.append, **kw) == len(sched)
    rd = y4m.Reader(io.BytesIO(dst.getvalue()), **ALL)
    rate = retime.as_rate(fps_out)
    assert (rd.width, rd.height, rd.colorspace, rd.chroma, rd.bit_depth) == (w, h, tag, chroma, depth)
    assert (rd.fps_num, rd.fps_den) == (rate.numerator, rate.denominator)      # the header carries the new rate
    out = list(rd)
    assert len(out) == len(sched) > 2
    for o, want, output in zip(out, expected_stream(frames, sched), sched):
        assert np.array_equal(o, want), output
        if s == 1 and output[0][1] == 0:
            assert np.array_equal(o, frames[output[0][0]])                      # a pass-through: the input's bytes
    # the calls: whole outputs per step, chunk = batch, the stream's layout and depth, only frames some sample reads
    name = "yuv16" if depth > 8 else "yuv"
    rows = {"420": 3 * h // 2, "422": 2 * h, "444": 3 * h}[chroma]
    sent = [g for c in model.calls for g in c[3]]
    assert len(sent) == sum(1 for output in sched if not (s == 1 and output[0][1] == 0))
    for c in model.calls:
        assert c[0] == name and c[1][1:] == (rows, w) and c[4] == batch and c[5] == "i" + chroma
        used = {p for g in c[3] for p, t in g} | {p + 1 for g in c[3] for p, t in g if t != 0}
        assert used == set(range(c[1][0]))
        if depth > 8:
            assert c[6]["depth"] == depth
    for c in model.calls[:-1]:   # a step holds at least `batch` network items, and no output more than that takes
        items = [sum(1 for _, t in g if t != 0) for g in c[3]]
        assert sum(items) >= batch > sum(items[:-1])
    if s == 1:
        assert len(sent) < len(sched)   # some outputs never reached the model
    if fps_in == 120:
        assert all(c[1][0] == 3 for c in model.calls)   # 5j, 5j+1, 5j+2 go up; 5j+3 and 5j+4 never do
    assert len(logs) == 1 and f"{n} frames of" in logs[0] and f"{len(sched)} frames at" in logs[0]
    assert f"{fps_in}:1 fps" in logs[0] and f"{rate.numerator}:{rate.denominator} fps" in logs[0]
    assert f"mean of {s} samples over a 1/2 shutter" in logs[0]


def test_expose_y4m_without_network_items():
    """120 -> 24 at shutter 1 with 5 samples: every sample is an input frame; steps are still bounded."""
    w, h, n = 6, 4, 60
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, w * h * 3 // 2).astype(np.uint8) for _ in range(n)]
    dst, model = io.BytesIO(), HostExpose()
    sched = retime.exposure_schedule(n, 120, 24, 1, 5)
    assert cv.expose_y4m(model, y4m_bytes(frames, w, h, "420", (120, 1)), dst, 24, 5, shutter=1, batch=2,
                         log=lambda m: None) == len(sched) == 12
    out = list(y4m.Reader(io.BytesIO(dst.getvalue()), **ALL))
    for j, o in enumerate(out):
        assert np.array_equal(o, ((np.sum([f.astype(np.int64) for f in frames[5 * j:5 * j + 5]], axis=0) + 2) // 5))
    assert [len(c[3]) for c in model.calls] == [8, 4]   # 4 * batch outputs a step, then the rest


# ---- keywords and the CLI ------------------------------------------------------------------------
def test_keywords():
    frames = [np.zeros(36, dtype=np.uint8) for _ in range(6)]

    def run(**kw):
        return cv.interpolate_y4m(HostExpose(), y4m_bytes(frames, 6, 4, "420", (60, 1)), io.BytesIO(),
                                  log=lambda m: None, **kw)

    with pytest.raises(ValueError, match="shutter needs samples"):
        run(fps_out=24, shutter="1/2")
    with pytest.raises(ValueError, match="shutter needs samples"):
        run(fps_out=120, shutter=Fr(1, 2))
    for bad in (0, 257, True):
        with pytest.raises(ValueError, match="samples must be an int in 1..256"):
            run(fps_out=24, samples=bad)
    with pytest.raises(ValueError, match="samples needs fps_out"):
        run(sf=1, samples=2)
    with pytest.raises(TypeError):
        run(fps_out=24, samples=2, shutter=0.5)
    with pytest.raises(ValueError):
        run(fps_out=24, samples=2, shutter="3/2")
    with pytest.raises(ValueError, match="decimation is out of scope"):   # without samples: today's refusal
        run(fps_out=24)
    with pytest.raises(ValueError, match="decimation is out of scope"):
        run(fps_out=60)
    assert run(fps_out=24, samples=2) == len(retime.exposure_schedule(6, 60, 24, "1/2", 2)) == 2
    assert run(fps_out=60, samples=3, shutter=1) == 5


def test_cli_parses_samples_and_shutter():
    base = ["--model_name", "m", "convert", "--sf", "0", "--fps", "24", "--y4m_in", "-", "--y4m_out", "-"]
    args = build_parser().parse_args(base)
    assert args.samples is None and args.shutter is None
    args = build_parser().parse_args(base + ["--fps_out", "24", "--samples", "8", "--shutter", "1/2"])
    assert args.samples == 8 and args.shutter == "1/2" and args.fps_out == "24"
    assert retime.as_shutter(args.shutter) == Fr(1, 2)


@pytest.mark.parametrize("name,shape,dtype", [("expose_items_u8", (4, 6, 8, 3), torch.uint8),
                                              ("expose_items_u16", (4, 6, 8, 3), torch.uint16),
                                              ("expose_items_yuv", (4, 9, 8), torch.uint8),
                                              ("expose_items_yuv16", (4, 9, 8), torch.uint16)])
def test_net_refuses_bad_groups_before_any_device_work(name, shape, dtype):
    """A Net on the host has no engine: bad groups must raise before one is asked for."""
    net = Net().eval()
    frames = torch.zeros(shape, dtype=dtype)
    call = getattr(net, name)
    with torch.no_grad():
        for bad in ([], [[]], [[(3, 0.5)]], [[(4, 0)]], [[(0, 1.0)]], [[(1, 0.5), (0, 0.5)]], [[(0, 0.5)] * 257]):
            with pytest.raises(ValueError):
                call(frames, bad)
        with pytest.raises(TypeError):
            call(frames, [[0.5]])
        with pytest.raises(ValueError):
            call(frames, [[(0, 0.5)]], chunk=0)
        with pytest.raises(ValueError):
            call(frames, [[(0, 0.5)]], flow_scale=3)
        with pytest.raises(RuntimeError, match="ROCm"):
            call(frames, [[(0, 0.5), (3, 0)]])      # good groups reach the engine, which needs the device
    with pytest.raises(RuntimeError, match="inference-only"):
        call(frames, [[(0, 0.5)]])


# ---- the C ABI: every refusal comes before any launch ----------------------------------------------
def test_abi_version_stays_25():
    assert _lib.ABI_VERSION == 25 == _lib.lib().rrin_abi_version()


def test_rrin_mean_frames_argument_checks():
    """Fabricated addresses: every call below must return its code without touching them."""
    fn = _lib.lib().rrin_mean_frames
    tab, st, out = 0x10000, 0x20000, 0x30000

    def run(frames=tab, k=4, start=st, g=2, o=out, stride=64, length=36, depth=8, shift=0, access=4):
        return fn(frames, k, start, g, o, stride, length, depth, shift, access, None)

    assert run(frames=None) == E_ARG and run(start=None) == E_ARG and run(o=None) == E_ARG
    assert run(g=0) == E_SHAPE and run(g=-1) == E_SHAPE
    assert run(length=0) == E_SHAPE and run(length=-5) == E_SHAPE
    assert run(g=65536, k=65536) == E_SHAPE
    for depth, shift in ((7, 0), (17, 0), (8, 1), (10, 7), (12, 5), (16, 1), (10, -1)):
        assert run(depth=depth, shift=shift) == E_ARG, (depth, shift)
    assert run(depth=10, o=out + 1, access=2) == E_ARG                 # an odd 16-bit address
    assert run(depth=10, o=out + 2, access=4) == E_ARG                 # out must keep the access aligned
    assert run(o=out + 4, access=16) == E_ARG
    assert run(stride=66, access=4) == E_ARG and run(stride=72, access=16) == E_ARG
    assert run(depth=10, stride=65, access=4) == E_ARG                 # 130 bytes between frames
    assert run(stride=35) == E_ARG                                     # frames would overlap
    for access in (0, 2, 3, 8, 32, -4):
        assert run(access=access) == E_ARG, access
    assert run(depth=10, access=1) == E_ARG
    assert run(frames=tab + 4) == E_ARG and run(start=st + 2) == E_ARG  # the table holds pointers, start int32
    assert run(k=1) == E_ARG and run(k=513) == E_ARG and run(k=0) == E_ARG  # 1..256 frames per group
    assert run(length=1 << 45, stride=1 << 45, access=1) == E_SHAPE    # more workgroups than a grid has
