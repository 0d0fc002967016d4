"""GPU: the linear-light synthetic shutter -- rrin_mean_frames_lut and rrin_mean_frames_yuv_lut against
``exposure.mean_frames_linear``, ``Net.expose_items_*`` with ``light`` / ``weights`` against ``exposure.expose``
over the same call's ``interpolate_items_*`` outputs, and ``convert.expose_y4m`` with ``light``.  Every
comparison is exact equality against the host definition; a table is an input of both sides.

Element kernel: frame lengths 1, 15, 16, 17, 36 and 256 * 16 + 5 (an empty vector part, a tail, more than
one workgroup), groups of 1, 2, 3, 5 and 256 frames in one call, source views at odd element offsets, at
4-byte and at 16-byte offsets (the three access widths), words over the whole range, a strided output
whose gaps hold a marker.  YUV kernel: every layout at every depth and alignment, the smallest frame of
each chroma format, one that is no multiple of anything, and one of more than one workgroup (18x34:
153 blocks at 4:2:0, 306 at 4:2:2; 17x33 at 4:4:4: 561)."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from rrin_amd import _lib, exposure, retime, transfer, y4m, yuv
from rrin_amd import convert as cv
from rrin_amd.engine import device_table, mean_frames, mean_frames_linear
from rrin_amd.framefmt import FrameFormat, _stack_geometry
from tests.test_gpu_items import net_of, stack_of

pytestmark = pytest.mark.gpu

E_SHAPE, E_ARG = -1, -2
SIZES = [1, 2, 3, 5, 256]
LENS = [1, 15, 16, 17, 36, 256 * 16 + 5]
FORMATS = [(8, 0), (10, 0), (10, 6), (12, 0), (12, 4)]


def np_dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def to_dev(a: np.ndarray, dev) -> torch.Tensor:
    t = torch.from_numpy(a.view(np.int16)).view(torch.uint16) if a.dtype == np.uint16 else torch.from_numpy(a)
    return t if dev is None else t.to(dev)


def to_np(t: torch.Tensor) -> np.ndarray:
    t = t.cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.uint16 else t.numpy()


def flat_table(depth, seed):
    """A random non-decreasing table with flat runs, 0 .. 2**30."""
    rng = np.random.default_rng(seed)
    n = 1 << depth
    lin = np.cumsum(rng.integers(0, 1 << 12, n) * (rng.random(n) < 0.6))
    lin = lin * (1 << 30) // max(int(lin[-1]), 1)
    lin[0] = 0
    return torch.from_numpy(lin.astype(np.int64))


def host_linear(frames, fmt, lin, weights) -> np.ndarray:
    """``exposure.mean_frames_linear`` of a list of numpy frames."""
    return to_np(exposure.mean_frames_linear(to_dev(np.stack(frames), None), fmt, lin, weights))


# ---- the element kernel ----------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["srgb", "flat", "none_triangle"])
@pytest.mark.parametrize("depth,shift", FORMATS)
def test_element_kernel_is_the_definition(gpu, depth, shift, table):
    esize = 1 if depth == 8 else 2
    fmt = FrameFormat.samples(None, depth, shift)
    lin = {"srgb": transfer.table("srgb", depth), "flat": flat_table(depth, 7), "none_triangle": None}[table]
    explicit = [3, 1, 4, 1, 5]                                  # fits the group of five only
    dev_table = None if lin is None else device_table(lin, depth, gpu)
    rng = np.random.default_rng(1000 * depth + shift)
    k = sum(SIZES)
    for mode in ("element", "four", "sixteen"):
        offs = {"element": (1, 3, 5), "four": (4 // esize, 8 // esize, 12 // esize), "sixteen": (0, 0, 0)}[mode]
        out_off = {"element": 1, "four": 4 // esize, "sixteen": 0}[mode]
        for n in LENS:
            slot = (n + 15) // 16 * 16 + 16                     # elements per source slot and per output frame
            pool = rng.integers(0, 256 ** esize, k * slot).astype(np_dtype(depth))   # words above maxval too
            pool_d = to_dev(pool, gpu)
            groups, host, i = [], [], 0
            for s in SIZES:
                lo = [(i + j) * slot + offs[(i + j) % 3] for j in range(s)]
                groups.append([pool_d[a:a + n] for a in lo])
                host.append([pool[a:a + n] for a in lo])
                i += s
            want = [host_linear(fs, fmt, lin, "triangle") for fs in host]
            # a larger buffer of 0xA5 bytes; the frames `slot` elements apart, `out_off` elements in
            g = len(SIZES)
            fill = 0xA5 if esize == 1 else 0xA5A5
            big = to_dev(np.full((g + 2) * slot, fill, dtype=np_dtype(depth)), gpu)
            out = big[slot + out_off:].as_strided((g, n), (slot, 1))
            assert mean_frames_linear(groups, fmt, dev_table, "triangle", out=out) is out
            full = np.full((g + 2) * slot, fill, dtype=np_dtype(depth))
            for j in range(g):
                full[slot + out_off + j * slot:][:n] = want[j]
            first = to_np(big)
            assert np.array_equal(first, full), (mode, n, np.nonzero(first != full)[0][:8])   # nothing else moved
            # a fresh dense output, and the same bits again
            got = mean_frames_linear(groups, fmt, dev_table, "triangle")
            assert got.shape == (g, n) and np.array_equal(to_np(got), np.stack(want)), (mode, n)
            assert np.array_equal(to_np(mean_frames_linear(groups, fmt, dev_table, "triangle")), to_np(got))
            got = mean_frames_linear([groups[3]], fmt, dev_table, explicit)
            assert np.array_equal(to_np(got)[0], host_linear(host[3], fmt, lin, explicit)), (mode, n)


@pytest.mark.parametrize("depth,shift", FORMATS + [(16, 0)])
def test_element_kernel_without_table_and_box_is_mean_frames(gpu, depth, shift):
    esize = 1 if depth == 8 else 2
    fmt = FrameFormat.samples(None, depth, shift)
    rng = np.random.default_rng(depth + shift)
    n = 256 * 16 + 5
    pool = rng.integers(0, 256 ** esize, (sum(SIZES), n + 3)).astype(np_dtype(depth))
    pool_d = to_dev(pool, gpu)
    groups, i = [], 0
    for s in SIZES:
        groups.append([pool_d[i + j, (i + j) % 3:][:n] for j in range(s)])
        i += s
    want = to_np(mean_frames(groups, depth, shift))
    for w in (None, "box"):
        assert np.array_equal(to_np(mean_frames_linear(groups, fmt, None, w)), want)


@pytest.mark.parametrize("depth,shift", FORMATS)
def test_element_kernel_largest_sum(gpu, depth, shift):
    """W = 65535 on all-maxval frames: the largest 64-bit sum there is, through the magic divide."""
    maxval = (1 << depth) - 1
    fmt = FrameFormat.samples(None, depth, shift)
    top = to_dev(np.full((3, 37), maxval << shift, dtype=np_dtype(depth)), gpu)
    zero = to_dev(np.zeros((1, 37), dtype=np_dtype(depth)), gpu)
    tab = device_table("srgb", depth, gpu)
    cases = [([top[0]], [65535]), ([top[0], top[1], top[2]], [65533, 1, 1]), ([top[0], zero[0]], [65534, 1]),
             ([top[j % 3] for j in range(255)], [257] * 255)]
    for frames, w in cases:
        host = [to_np(f) for f in frames]
        for t, lin in ((tab, "srgb"), (None, None)):
            got = to_np(mean_frames_linear([frames], fmt, t, w))[0]
            assert np.array_equal(got, host_linear(host, fmt, lin, w)), (w[:3], lin)
    assert int(to_np(mean_frames_linear([[top[0]]], fmt, tab, [65535])).min()) == maxval << shift


# ---- the YUV kernel --------------------------------------------------------------------------------
YUV_SIZES = {"420": [(2, 2), (4, 6), (18, 34)], "422": [(1, 2), (3, 4), (18, 34)], "444": [(1, 1), (3, 5), (17, 33)]}


@pytest.mark.parametrize("layout", yuv.ALL_LAYOUTS)
@pytest.mark.parametrize("depth,shift", FORMATS)
def test_yuv_kernel_is_the_definition(gpu, layout, depth, shift):
    esize = 1 if depth == 8 else 2
    light = "srgb" if depth == 8 else "pq"
    tab = device_table(light, depth, gpu)
    rng = np.random.default_rng(100 * depth + shift + len(layout))
    sizes = [1, 2, 7]
    for std, full in (("bt709", False), ("bt601", True)):
        coef = yuv.coefficients(std, full, depth)
        fmt = FrameFormat.yuv(layout, coef) if depth == 8 else FrameFormat.yuv16(layout, depth, shift != 0, coef)
        for h0, w0 in YUV_SIZES[yuv.chroma_of(layout)]:
            rows = yuv.stack_rows(h0, layout)
            n = rows * w0
            slot = (n + 15) // 16 * 16 + 16
            pool = rng.integers(0, 256 ** esize, sum(sizes) * slot).astype(np_dtype(depth))   # the whole word range
            pool_d = to_dev(pool, gpu)
            groups, host, i = [], [], 0
            for s in sizes:
                lo = [(i + j) * slot + (i + j) % 3 for j in range(s)]          # frames start at any element
                groups.append([pool_d[a:a + n].view(rows, w0) for a in lo])
                host.append([pool[a:a + n].reshape(rows, w0) for a in lo])
                i += s
            want = [host_linear(fs, fmt, light, "triangle") for fs in host]
            g = len(sizes)
            fill = 0xA5 if esize == 1 else 0xA5A5
            big = to_dev(np.full((g + 2) * slot, fill, dtype=np_dtype(depth)), gpu)
            out = big[slot + 1:].as_strided((g, rows, w0), (slot, w0, 1))
            assert mean_frames_linear(groups, fmt, tab, "triangle", out=out) is out
            full_buf = np.full((g + 2) * slot, fill, dtype=np_dtype(depth))
            for j in range(g):
                full_buf[slot + 1 + j * slot:][:n] = want[j].reshape(-1)
            first = to_np(big)
            assert np.array_equal(first, full_buf), (std, h0, w0, np.nonzero(first != full_buf)[0][:8])
            got = mean_frames_linear(groups, fmt, tab, "triangle")
            assert np.array_equal(to_np(got), np.stack(want)), (std, h0, w0)
            assert np.array_equal(to_np(mean_frames_linear(groups, fmt, tab, "triangle")), to_np(got))
            # without a table a YUV frame is averaged per stored element
            assert np.array_equal(to_np(mean_frames_linear(groups, fmt, None, "triangle")),
                                  np.stack([host_linear(fs, fmt, None, "triangle") for fs in host]))


# ---- refusals: a code, no launch -------------------------------------------------------------------
def test_entry_points_refuse_without_a_launch(gpu):
    lib = _lib.lib()
    f = torch.zeros(64, dtype=torch.uint8, device=gpu)
    out = torch.full((2, 64), 0xA5, dtype=torch.uint8, device=gpu)
    up = torch.zeros(16, dtype=torch.int64, device=gpu)
    up[:2] = f.data_ptr()
    start = torch.tensor([0, 1, 2], dtype=torch.int32, device=gpu)
    wts = torch.ones(2, dtype=torch.int32, device=gpu)
    tab8 = device_table("srgb", 8, gpu)
    tab12 = device_table("srgb", 12, gpu)
    torch.cuda.synchronize()

    def element(o=out.data_ptr(), depth=8, access=16, table=tab8.data_ptr()):
        return lib.rrin_mean_frames_lut(up.data_ptr(), 2, start.data_ptr(), 2, o, 64, 36, depth, 0, access,
                                        wts.data_ptr(), table, None)

    def planes(h0=4, w0=6, table=tab8.data_ptr(), o=out.data_ptr(), depth=8):
        uo, vo, c_pitch, c_step, chroma = _stack_geometry("i420", 1, 4, 6)
        geom = _lib.YuvPlanes(uo, vo, w0, c_pitch, c_step, chroma, depth, 0)
        coef = _lib.YuvCoef(*yuv.coefficients(depth=depth))
        return lib.rrin_mean_frames_yuv_lut(up.data_ptr(), 2, start.data_ptr(), 2, o, 64, C.byref(geom), C.byref(coef),
                                            h0, w0, wts.data_ptr(), table, None)

    assert planes(table=None) == E_ARG                               # a null table on the YUV entry
    assert element(depth=13, access=4, table=tab12.data_ptr()) == E_ARG   # depth 13 with a table
    assert planes(w0=5) == E_SHAPE                                   # odd w0 at 4:2:0
    assert element(o=out.data_ptr() + 4, access=16) == E_ARG         # out misaligned for the chosen access
    assert element(o=out.data_ptr() + 1, access=4) == E_ARG
    assert planes(o=out.data_ptr() + 1, depth=10) == E_ARG           # an odd word address
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())                                 # and nothing ran
    fmt10 = FrameFormat.samples(None, 10, 0)
    with pytest.raises(ValueError, match="device_table"):
        mean_frames_linear([[torch.zeros(8, dtype=torch.uint16, device=gpu)]], fmt10, tab8, None)
    with pytest.raises(ValueError, match="LDS"):
        mean_frames_linear([[torch.zeros(8, dtype=torch.uint16, device=gpu)]], FrameFormat.samples(None, 13, 0), tab12,
                           None)
    with pytest.raises(ValueError):
        mean_frames_linear([[f, f], [f]], FrameFormat.u8(), tab8, [1, 2])
    with pytest.raises(RuntimeError, match="ROCm"):
        mean_frames_linear([[f.cpu()]], FrameFormat.u8(), None, None)


# ---- Net.expose_items_* with light and weights -----------------------------------------------------
P = 3
GROUPS = [[(0, 0), (0, 0.4), (0, 0.8)],                      # an input frame and two items of its pair
          [(1, 0.2)],                                        # one sample
          [(1, 0.5), (2, 0), (2, 0.5), (2, 0.9375)],         # two pairs, an input frame between items
          [(2, 0.96875), (3, 0)]]                            # the last frame of the stack: (P, 0)
ITEMS = [(p, t) for g in GROUPS for p, t in g if t != 0]
PATHS = {
    "u8": dict(shape=(32, 48, 3), dtype=torch.uint8, fmt=FrameFormat.u8(), kw={}),
    "yuv": dict(shape=(48, 48), dtype=torch.uint8, fmt=FrameFormat.yuv("nv12"), kw={"layout": "nv12"}),
    "u16": dict(shape=(32, 48, 3), dtype=torch.uint16, fmt=FrameFormat.u16(12, "t"), kw={"depth": 12}),
    "yuv16": dict(shape=(48, 48), dtype=torch.uint16, fmt=FrameFormat.yuv16("i420", 10, True),
                  kw={"layout": "i420", "depth": 10, "msb": True}),
}


def defined(frames, items, fmt, light, weights, elementwise=False):
    """``exposure.expose`` over the item forward's outputs ``items`` (in ITEMS order) and the stack's frames."""
    fr, it = frames.cpu(), items.cpu()
    lookup = {pt: it[k] for k, pt in enumerate(ITEMS)}
    fmt = FrameFormat.samples(None, fmt.depth, fmt.shift) if elementwise else fmt
    return to_np(exposure.expose(fr, GROUPS, lambda p, t: lookup[(p, t)], fmt.depth, fmt.shift, light=light,
                                 weights=weights, fmt=fmt))


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_expose_items_with_light_is_the_definition(gpu, precision, path):
    cfg = PATHS[path]
    fmt = cfg["fmt"]
    net = net_of(gpu, precision)
    frames = stack_of((P + 1,) + cfg["shape"], 41, gpu, cfg["dtype"], fmt.maxval, fmt.shift)
    plane = stack_of((P + 1, 32, 48), 42, gpu, cfg["dtype"], fmt.maxval, fmt.shift)
    expose, items_fwd = getattr(net, "expose_items_" + path), getattr(net, "interpolate_items_" + path)
    pairs, ts = [p for p, _ in ITEMS], [t for _, t in ITEMS]
    with torch.no_grad():
        items, iplanes = items_fwd(frames, pairs, ts, plane=plane, **cfg["kw"])
        plain = expose(frames, GROUPS, **cfg["kw"])
        for light, weights in (("srgb", "triangle"), (None, "triangle")):
            want = defined(frames, items, fmt, light, weights)
            got = expose(frames, GROUPS, light=light, weights=weights, **cfg["kw"])
            assert got.dtype == cfg["dtype"] and tuple(got.shape) == (len(GROUPS),) + tuple(frames.shape[1:])
            assert np.array_equal(to_np(got), want), (light, weights)
            assert np.array_equal(to_np(expose(frames, GROUPS, chunk=2, light=light, weights=weights, **cfg["kw"])),
                                  want)                                  # chunk changes no bit; two runs, the same bits
            gf, gp = expose(frames, GROUPS, chunk=3, plane=plane, light=light, weights=weights, **cfg["kw"])
            assert np.array_equal(to_np(gf), want)
            # the plane has no curve: the weighted mean of its code values
            assert np.array_equal(to_np(gp), defined(plane, iplanes, fmt, None, weights, elementwise=True))
        assert not np.array_equal(to_np(plain), want)
        # without the keywords the call is what it was
        assert np.array_equal(to_np(expose(frames, GROUPS, light=None, weights=None, **cfg["kw"])), to_np(plain))
        assert np.array_equal(to_np(expose(frames, GROUPS, weights="box", **cfg["kw"])), to_np(plain))
    net.check_range()


def test_expose_items_with_light_keeps_the_gate(gpu):
    net = net_of(gpu, "fp32")
    a = stack_of((1, 32, 48, 3), 5, gpu)
    b = (a.to(torch.int16) + 3).clamp(0, 255).to(torch.uint8)
    noise = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (1, 32, 48, 3), dtype=np.uint8)).to(gpu)
    frames = torch.cat([a, a, b, noise])
    gate = torch.tensor([1, 0, 2], dtype=torch.int32, device=gpu)
    pairs, ts = [p for p, _ in ITEMS], [t for _, t in ITEMS]
    with torch.no_grad():
        items = net.interpolate_items_u8(frames, pairs, ts, gate=gate)
        net.expose_items_u8(frames, GROUPS, gate=gate)
        codes = net.last_gate.cpu().tolist()
        got = net.expose_items_u8(frames, GROUPS, gate=gate, light="srgb", weights="triangle")
        assert net.last_gate.cpu().tolist() == codes == [1, 1, 0, 0, 2, 2, 2]
        assert np.array_equal(to_np(got), defined(frames, items, FrameFormat.u8(), "srgb", "triangle"))
        sad = net.pair_stats_u8(frames[:-1], frames[1:]).tolist()
        th = (sad[1] + sad[2]) / 2 / (32 * 48 * 3)
        again = net.expose_items_u8(frames, GROUPS, scene_threshold=th, light="srgb", weights="triangle")
        assert net.last_gate.cpu().tolist() == codes and torch.equal(again, got)


def test_expose_items_refuses_bad_light_and_weights_before_device_work(gpu):
    net = net_of(gpu, "fp32")
    frames = stack_of((P + 1, 32, 48, 3), 23, gpu)
    words = stack_of((P + 1, 32, 48, 3), 23, gpu, torch.uint16, 16383)
    eng = net.engine()
    with torch.no_grad():
        for call in (net.expose_items_u8, eng.expose_items_u8):
            for bad in ("rec709", [0] * 5, list(range(255, -1, -1)), 7):
                with pytest.raises(ValueError):
                    call(frames, GROUPS, light=bad)
            for bad in ("gauss", [1, 2, 3], [65535, 1, 1]):
                with pytest.raises(ValueError):
                    call(frames, GROUPS, weights=bad)
        for call in (net.expose_items_u16, eng.expose_items_u16):
            with pytest.raises(ValueError, match="LDS"):
                call(words, GROUPS, depth=14, light="srgb")
        assert tuple(net.expose_items_u16(words, GROUPS, depth=14, weights="triangle").shape) == (4, 32, 48, 3)


# ---- the pipe --------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [8, 10])
def test_expose_y4m_with_light_on_the_device(gpu, depth):
    """9 frames of 48x32 4:2:0, 60 -> 24 with 4 samples over a 1/2 shutter under sRGB: every output frame is
    the definition over per-item forward_yuv[16] calls, and the header is that of the run without light."""
    net = net_of(gpu, "fp32")
    w0, h0, n = 48, 32, 9
    maxval = (1 << depth) - 1
    frames = stack_of((n, 3 * h0 // 2, w0), 31, None, torch.uint8 if depth == 8 else torch.uint16, maxval)
    fmt = FrameFormat.yuv("i420") if depth == 8 else FrameFormat.yuv16("i420", depth)
    kw = {} if depth == 8 else {"depth": depth}
    fwd = net.forward_yuv if depth == 8 else net.forward_yuv16
    src = io.BytesIO()
    wr = y4m.Writer(src, w0, h0, 60, 1, "420" if depth == 8 else f"420p{depth}", depths=(8, 10, 12))
    for f in frames:
        wr.write(to_np(f).reshape(-1))
    sched = retime.exposure_schedule(n, 60, 24, "1/2", 4)
    heads, logs = [], []
    for light in (None, "srgb"):
        src.seek(0)
        dst = io.BytesIO()
        assert cv.interpolate_y4m(net, src, dst, fps_out=24, samples=4, batch=3, log=logs.append, light=light) == 3
        raw = dst.getvalue()
        heads.append(raw[:raw.index(b"\n")])
    assert heads[0] == heads[1]
    out = list(y4m.Reader(io.BytesIO(raw), depths=(8, 10, 12)))
    assert len(out) == 3
    dev = frames.to(gpu)
    with torch.no_grad():
        for o, output in zip(out, sched):
            srcs = [to_np(frames[p]) if t == 0 else
                    to_np(fwd(dev[p:p + 1], dev[p + 1:p + 2], t=float(t), layout="i420", **kw)[0]) for p, t in output]
            assert np.array_equal(o, host_linear(srcs, fmt, "srgb", None).reshape(-1)), output
    assert "linear light under srgb, box weights" in logs[1] and "linear light" not in logs[0]
