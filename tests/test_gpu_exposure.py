"""GPU: the synthetic shutter -- rrin_mean_frames against ``exposure.mean_frames``, ``Net.expose_items_*``
against the definition over ``interpolate_items_*`` outputs and stack frames, and ``convert.expose_y4m`` on
the device.  Every comparison is exact equality.

Kernel shapes: ``len`` 1, 15, 16, 17, 36 and 4099 elements (below, at and above one 16-byte access, a
6x4 4:2:0 frame, more than one workgroup of 256 lanes with a tail); groups of 1, 2, 3, 7 and 256 frames
in one call; source views 0, 1 and 3 elements into their slots (the element-wide access), 0, 4 and 12
bytes (the 4-byte access) and 16-byte aligned (the 16-byte access).  Net shapes are those of
test_gpu_items.py: 40x24 (padding and crop live) and 48x32 / 48x48 (even, for 4:2:0), P = 3 pairs."""
import io

import numpy as np
import pytest
import torch

from rrin_amd import convert as cv
from rrin_amd import exposure, retime, y4m, yuv
from rrin_amd.engine import mean_frames
from tests.test_gpu_items import net_of, stack_of

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 7, 256]
LENS = [1, 15, 16, 17, 36, 4099]
FORMATS = [(8, 0), (10, 0), (12, 0), (16, 0), (10, 6), (12, 4)]
P = 3
GROUPS = [[(0, 0), (0, 0.4), (0, 0.8)],                      # an input frame and two items of its pair
          [(1, 0.2)],                                        # one sample: the item itself
          [(1, 0.5), (2, 0), (2, 0.5), (2, 0.9375)],         # two pairs, an input frame between items
          [(2, 0.96875), (3, 0)]]                            # the last frame of the stack: (P, 0)
ITEMS = [(p, t) for g in GROUPS for p, t in g if t != 0]


def np_dtype(depth):
    return np.uint8 if depth == 8 else np.uint16


def to_dev(a: np.ndarray, dev) -> torch.Tensor:
    t = torch.from_numpy(a.view(np.int16)).view(torch.uint16) if a.dtype == np.uint16 else torch.from_numpy(a)
    return t if dev is None else t.to(dev)


def to_np(t: torch.Tensor) -> np.ndarray:
    t = t.cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.uint16 else t.numpy()


def host_mean(frames, depth, shift) -> np.ndarray:
    """``exposure.mean_frames`` of a list of numpy frames."""
    return to_np(exposure.mean_frames(to_dev(np.stack(frames), None), depth, shift))


# ---- the kernel ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["element", "four", "sixteen"])
@pytest.mark.parametrize("depth,shift", FORMATS)
def test_mean_frames_kernel_is_the_definition(gpu, depth, shift, mode):
    esize = 1 if depth == 8 else 2
    offs = {"element": (0, 1, 3), "four": (0, 4 // esize, 12 // esize), "sixteen": (0, 0, 0)}[mode]
    out_off = {"element": 1, "four": 4 // esize, "sixteen": 0}[mode]
    rng = np.random.default_rng(1000 * depth + shift)
    k = sum(SIZES)
    for n in LENS:
        slot = (n + 15) // 16 * 16 + 16                     # elements per source slot and per output frame
        pool = rng.integers(0, 256 ** esize, k * slot).astype(np_dtype(depth))   # words above maxval too
        pool_d = to_dev(pool, gpu)
        assert pool_d.data_ptr() % 16 == 0
        groups, host, i = [], [], 0
        for s in SIZES:
            lo = [(i + j) * slot + offs[(i + j) % 3] for j in range(s)]
            groups.append([pool_d[a:a + n] for a in lo])
            host.append([pool[a:a + n] for a in lo])
            i += s
        want = [host_mean(fs, depth, shift) for fs in host]
        # a larger buffer of 0xA5 bytes; the frames `slot` elements apart, `out_off` elements in
        g = len(SIZES)
        fill = 0xA5 if esize == 1 else 0xA5A5
        big = to_dev(np.full((g + 2) * slot, fill, dtype=np_dtype(depth)), gpu)
        out = big[slot + out_off:].as_strided((g, n), (slot, 1))
        assert mean_frames(groups, depth, shift, out=out) is out
        full = np.full((g + 2) * slot, fill, dtype=np_dtype(depth))
        for j in range(g):
            full[slot + out_off + j * slot:][:n] = want[j]
        first = to_np(big)
        assert np.array_equal(first, full), (n, np.nonzero(first != full)[0][:8])   # and nothing else moved
        # a fresh dense output, and the same bits again
        got = mean_frames(groups, depth, shift)
        assert got.shape == (g, n) and np.array_equal(to_np(got), np.stack(want))
        assert np.array_equal(to_np(mean_frames(groups, depth, shift)), to_np(got))


def test_mean_frames_kernel_stack_views_of_36_byte_frames(gpu):
    """``stack[1:]`` of 6x4 4:2:0 frames: 36 bytes apart, so 4-byte aligned at best; one frame in two groups."""
    rng = np.random.default_rng(5)
    stack = rng.integers(0, 256, (9, 6, 6), dtype=np.uint8)
    d = to_dev(stack, gpu)[1:]
    groups = [[d[0], d[1]], [d[1], d[2], d[3]], [d[7]], [d[k] for k in range(8)]]
    want = [host_mean([stack[1 + k] for k in ks], 8, 0) for ks in ([0, 1], [1, 2, 3], [7], range(8))]
    assert np.array_equal(to_np(mean_frames(groups)), np.stack(want))
    words = rng.integers(0, 1024, (5, 36)).astype(np.uint16)
    dw = to_dev(words, gpu)[1:]
    got = mean_frames([[dw[0], dw[1], dw[2]], [dw[3], dw[0]]], 10, 0)
    assert np.array_equal(to_np(got), np.stack([host_mean(list(words[1:4]), 10, 0),
                                                host_mean([words[4], words[1]], 10, 0)]))


@pytest.mark.parametrize("depth,shift", [(8, 0), (16, 0), (10, 6)])
def test_mean_frames_kernel_every_group_size(gpu, depth, shift):
    """S = 1 .. 256 in one call (the divide by S is a multiply by a per-S constant): random frames, and
    the largest sums there are, all-maxval frames with one frame of zeros."""
    rng = np.random.default_rng(depth)
    maxval = (1 << depth) - 1
    pool = (rng.integers(0, maxval + 1, (256, 64)) << shift).astype(np_dtype(depth))
    top = np.full((2, 64), maxval << shift, dtype=np_dtype(depth))
    top[1] = 0
    pool_d, top_d = to_dev(pool, gpu), to_dev(top, gpu)
    got = to_np(mean_frames([[pool_d[j] for j in range(s)] for s in range(1, 257)], depth, shift))
    for s in range(1, 257):
        assert np.array_equal(got[s - 1], host_mean(list(pool[:s]), depth, shift)), s
    got = to_np(mean_frames([[top_d[0]] * (s - 1) + [top_d[1]] for s in range(1, 257)], depth, shift))
    for s in range(1, 257):
        assert np.array_equal(got[s - 1], host_mean([top[0]] * (s - 1) + [top[1]], depth, shift)), s


def test_mean_frames_refusals(gpu):
    f = torch.zeros(36, dtype=torch.uint8, device=gpu)
    for bad in ([], [[]], [[f] * 257], [[f, f[:35]]], [[f, f.view(6, 6)]], [[torch.zeros(72, dtype=torch.uint8, device=gpu)[::2]]],
                [[f, f.cpu()]]):
        with pytest.raises(ValueError):
            mean_frames(bad)
    with pytest.raises(TypeError):
        mean_frames([[f]], 10, 0)
    with pytest.raises(TypeError):
        mean_frames([[None]])
    with pytest.raises(ValueError):
        mean_frames([[f], [f]], out=torch.zeros((3, 36), dtype=torch.uint8, device=gpu))
    with pytest.raises(RuntimeError, match="ROCm"):
        mean_frames([[f.cpu()]])


# ---- Net.expose_items_* ----------------------------------------------------------------------------
PATHS = {
    "u8": dict(shape=(24, 40, 3), dtype=torch.uint8, depth=8, shift=0, kw={}),
    "nv12": dict(shape=(48, 48), dtype=torch.uint8, depth=8, shift=0, kw={"layout": "nv12"}, name="yuv"),
    "i422": dict(shape=(48, 40), dtype=torch.uint8, depth=8, shift=0, kw={"layout": "i422"}, name="yuv"),
    "u16": dict(shape=(24, 40, 3), dtype=torch.uint16, depth=12, shift=0, kw={"depth": 12}),
    "yuv16": dict(shape=(72, 48), dtype=torch.uint16, depth=10, shift=0, kw={"layout": "i420", "depth": 10},
                  name="yuv16"),
    "yuv16msb": dict(shape=(72, 48), dtype=torch.uint16, depth=10, shift=6,
                     kw={"layout": "i420", "depth": 10, "msb": True}, name="yuv16"),
}


def defined(frames, items, depth, shift, groups=GROUPS):
    """The definition over the item forward's outputs ``items`` (in ITEMS order) and the stack's frames."""
    fr, it = to_np(frames), to_np(items)
    out, k = [], 0
    for group in groups:
        srcs = []
        for p, t in group:
            if t == 0:
                srcs.append(fr[p])
            else:
                srcs.append(it[k])
                k += 1
        out.append(host_mean(srcs, depth, shift))
    return np.stack(out)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_expose_items_is_the_definition(gpu, precision, path):
    """Frames, chunk 1 and 5, and ``plane=``: 40x24 RGB (8 and 12 bit), 48x32 NV12, 40x24 I422, 48x48 10-bit
    I420 with the samples in the low and in the high bits."""
    cfg = PATHS[path]
    net = net_of(gpu, precision)
    name = cfg.get("name", path)
    maxval = (1 << cfg["depth"]) - 1
    frames = stack_of((P + 1,) + cfg["shape"], 21, gpu, cfg["dtype"], maxval, cfg["shift"])
    h0, w0 = (cfg["shape"][:2] if len(cfg["shape"]) == 3 else yuv.stack_size(frames, cfg["kw"]["layout"]))
    plane = stack_of((P + 1, h0, w0), 22, gpu, cfg["dtype"], maxval, cfg["shift"])
    expose, items_fwd = getattr(net, "expose_items_" + name), getattr(net, "interpolate_items_" + name)
    pairs, ts = [p for p, _ in ITEMS], [t for _, t in ITEMS]
    with torch.no_grad():
        items, iplanes = items_fwd(frames, pairs, ts, plane=plane, **cfg["kw"])
        assert torch.equal(items_fwd(frames, pairs, ts, **cfg["kw"]).view(torch.uint8), items.view(torch.uint8))
        want = defined(frames, items, cfg["depth"], cfg["shift"])
        got = expose(frames, GROUPS, **cfg["kw"])
        assert got.dtype == cfg["dtype"] and tuple(got.shape) == (len(GROUPS),) + tuple(frames.shape[1:])
        assert np.array_equal(to_np(got), want)
        assert np.array_equal(to_np(got[1]), to_np(items[2]))            # S = 1: the item, bit for bit
        for chunk in (1, 5):
            assert np.array_equal(to_np(expose(frames, GROUPS, chunk=chunk, **cfg["kw"])), want), chunk
        gf, gp = expose(frames, GROUPS, chunk=3, plane=plane, **cfg["kw"])
        assert np.array_equal(to_np(gf), want)                           # the frames do not notice the plane
        assert gp.dtype == cfg["dtype"] and tuple(gp.shape) == (len(GROUPS), h0, w0)
        assert np.array_equal(to_np(gp), defined(plane, iplanes, cfg["depth"], cfg["shift"]))
        # no network item at all: input frames only
        only = [[(0, 0), (1, 0)], [(1, 0), (2, 0), (3, 0)]]
        assert np.array_equal(to_np(expose(frames, only, **cfg["kw"])),
                              defined(frames, items[:0], cfg["depth"], cfg["shift"], only))
    net.check_range()


def test_expose_items_gate(gpu):
    """Pair 0 a duplicate, pair 2 a cut by explicit codes: the exposure averages the gated items, and
    last_gate holds the codes of the call's seven network items."""
    net = net_of(gpu, "fp32")
    a = stack_of((1, 24, 40, 3), 5, gpu)
    b = (a.to(torch.int16) + 3).clamp(0, 255).to(torch.uint8)
    noise = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (1, 24, 40, 3), dtype=np.uint8)).to(gpu)
    frames = torch.cat([a, a, b, noise])
    gate = torch.tensor([1, 0, 2], dtype=torch.int32, device=gpu)
    pairs, ts = [p for p, _ in ITEMS], [t for _, t in ITEMS]
    with torch.no_grad():
        items = net.interpolate_items_u8(frames, pairs, ts, gate=gate)
        codes = net.last_gate.cpu().tolist()
        assert codes == [1, 1, 0, 0, 2, 2, 2]      # pair 0: the first frame; pair 2 at t >= 0.5: the second
        want = defined(frames, items, 8, 0)
        for chunk in (2, 4):
            got = net.expose_items_u8(frames, GROUPS, chunk=chunk, gate=gate)
            assert net.last_gate.dtype == torch.int32 and net.last_gate.cpu().tolist() == codes
            assert np.array_equal(to_np(got), want)
        assert np.array_equal(to_np(got[0]), to_np(frames[0]))           # three times the same frame
        # the threshold form: sums on the device, the same decisions here
        sad = net.pair_stats_u8(frames[:-1], frames[1:]).tolist()
        th = (sad[1] + sad[2]) / 2 / (24 * 40 * 3)
        got = net.expose_items_u8(frames, GROUPS, chunk=3, scene_threshold=th)
        assert net.last_gate.cpu().tolist() == codes and np.array_equal(to_np(got), want)
        with pytest.raises(ValueError):
            net.expose_items_u8(frames, GROUPS, gate=gate, scene_threshold=th)
        with pytest.raises(ValueError):
            net.expose_items_u8(frames, GROUPS, gate=gate[:2])


def test_expose_items_refuses_bad_arguments_before_device_work(gpu):
    net = net_of(gpu, "fp32")
    frames = stack_of((P + 1, 24, 40, 3), 23, gpu)
    with torch.no_grad():
        for bad in ([], [[]], [[(3, 0.5)]], [[(4, 0)]], [[(0, 1.0)]], [[(1, 0.5), (0, 0.5)]], [[(0, 0.5)] * 257]):
            with pytest.raises(ValueError):
                net.expose_items_u8(frames, bad)
        with pytest.raises(TypeError):
            net.expose_items_u8(frames, [[0.5]])
        with pytest.raises(ValueError):
            net.expose_items_u8(frames, GROUPS, chunk=0)
        with pytest.raises(ValueError):
            net.expose_items_u8(frames, GROUPS, plane=torch.zeros((P + 1, 24, 39), dtype=torch.uint8, device=gpu))
        with pytest.raises(TypeError):
            net.expose_items_u8(frames, GROUPS, plane=torch.zeros((P + 1, 24, 40), dtype=torch.uint16, device=gpu))
        with pytest.raises(TypeError):
            net.expose_items_u16(frames, GROUPS)
    with pytest.raises(RuntimeError, match="inference-only"):
        net.expose_items_u8(frames, GROUPS)


# ---- the pipe --------------------------------------------------------------------------------------
def test_expose_y4m_on_the_device(gpu):
    """9 frames of 48x32 C420, 60 -> 24 with 4 samples over a 1/2 shutter in steps of 3 items: every output
    frame is the definition built from per-item forward_yuv calls."""
    net = net_of(gpu, "fp32")
    w0, h0, n = 48, 32, 9
    frames = stack_of((n, 3 * h0 // 2, w0), 31, None)
    src = io.BytesIO()
    wr = y4m.Writer(src, w0, h0, 60, 1)
    for f in frames:
        wr.write(f.numpy())
    src.seek(0)
    dst, logs = io.BytesIO(), []
    sched = retime.exposure_schedule(n, 60, 24, "1/2", 4)
    assert cv.interpolate_y4m(net, src, dst, fps_out=24, samples=4, batch=3, log=logs.append) == len(sched) == 3
    raw = dst.getvalue()
    assert raw.startswith(b"YUV4MPEG2 W48 H32 F24:1 ")
    out = list(y4m.Reader(io.BytesIO(raw)))
    assert len(out) == 3
    dev = frames.to(gpu)
    with torch.no_grad():
        for o, output in zip(out, sched):
            srcs = [frames[p].numpy() if t == 0 else
                    to_np(net.forward_yuv(dev[p:p + 1], dev[p + 1:p + 2], t=float(t), layout="i420")[0])
                    for p, t in output]
            assert np.array_equal(o, host_mean(srcs, 8, 0).reshape(-1)), output
    assert "mean of 4 samples over a 1/2 shutter" in logs[0] and "24:1 fps" in logs[0]
