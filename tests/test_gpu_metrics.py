"""GPU: rrin_frame_metrics_u8 / _u16 against the definitions of rrin_amd.metrics (the squared error
bit for bit, SSIM within the rounding of one float64 sum), Net.frame_metrics_* on every layout, and
convert.evaluate_y4m on the device against forward_yuv followed by the definition.

The SSIM bound.  Per window both sides do the same three IEEE operations on the same exact
integers, so the window values are equal; only the order in which the W values (each at most 1 in
magnitude) are added differs.  Any order of adding W such terms errs by at most (W - 1) * 2^-53 * W
on the sum, W * 2^-53 on the mean; two orders differ by at most W * 2^-52."""
import ctypes as C
import io
import json

import numpy as np
import pytest
import torch

from rrin_amd import _lib, metrics, y4m, yuv
from rrin_amd import convert as cv

from . import hip_helpers as H
from .test_gpu_items import net_of, stack_of

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A5A5A5A5A


def tile():
    tc, br = C.c_int32(), C.c_int32()
    assert _lib.lib().rrin_frame_metrics_tile(C.byref(tc), C.byref(br)) == 0
    return tc.value, br.value


def frame_planes(h, w, step):
    """Three planes of h x w in a frame of 3*h*w elements: planar (step 1), interleaved RGB (step 3), or
    two interleaved planes followed by a planar one (step 2)."""
    if step == 1:
        return [(p * h * w, 1, w, h, w) for p in range(3)]
    if step == 3:
        return metrics.planes_of("rgb", h, w)
    return [(0, 2, 2 * w, h, w), (1, 2, 2 * w, h, w), (2 * h * w, 1, w, h, w)]


def run(a, sa, b, sb, n, planes, flags, wide=None):
    """The entry point twice into guarded buffers whose payload starts as garbage: (sse list, ssim
    float64 array or None) of the first run, after checking that the second gave the same bits and
    that the guard words around both outputs are untouched."""
    dev, p = a.device, len(planes)
    lib = _lib.lib()
    arr = (_lib.Plane * p)(*[_lib.Plane(off, pitch, step, h, w, 0) for off, step, pitch, h, w in planes])
    need = lib.rrin_frame_metrics_workspace_bytes(n, arr, p, flags)
    assert need > 0
    got = []
    for _ in range(2):
        ws = torch.full((need // 8,), GUARD, dtype=torch.int64, device=dev)
        sse = torch.full((n * p + 2,), GUARD, dtype=torch.int64, device=dev)
        val = torch.full((n * p + 2,), GUARD, dtype=torch.int64, device=dev)
        common = (arr, p, flags) if wide is None else (arr, p, flags, wide[0], wide[1])
        fn = lib.rrin_frame_metrics_u8 if wide is None else lib.rrin_frame_metrics_u16
        _lib.check(fn(a.data_ptr(), sa, b.data_ptr(), sb, n, *common, sse[1:].data_ptr(),
                      val[1:].data_ptr() if flags else None, ws.data_ptr(), need, H.stream(dev)), "rrin_frame_metrics")
        torch.cuda.synchronize(dev)
        s, v = sse.cpu(), val.cpu()
        assert s[0].item() == GUARD and s[-1].item() == GUARD and v[0].item() == GUARD and v[-1].item() == GUARD
        if not flags:
            assert bool((v == GUARD).all())     # ssim is not touched without the flag
        got.append((s[1:-1].clone(), v[1:-1].clone()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])   # the same bits on every run
    return got[0][0].view(n, p), (got[0][1].view(torch.float64).view(n, p) if flags else None)


def check_against_definition(a_host, b_host, planes, flags, depth=8, shift=0, dev=None):
    """a_host / b_host: [n, frame] element stacks.  ``a`` goes up as frames 1.. of an n+1 stack (so its
    base is one odd-sized frame from an aligned address), ``b`` with 7 elements between its frames."""
    n, frame = a_host.shape
    a = torch.zeros((n + 1, frame), dtype=a_host.dtype)
    a[1:] = a_host
    b = torch.zeros((n, frame + 7), dtype=b_host.dtype)
    b[:, :frame] = b_host
    a, b = a.to(dev), b.to(dev)
    wide = None if a_host.dtype == torch.uint8 else (depth, shift)
    sse, val = run(a[1:], frame, b, frame + 7, n, planes, flags, wide)
    want_sse, want_val = metrics._host_metrics(a_host, b_host, planes, depth, shift, bool(flags))
    assert torch.equal(sse, want_sse)
    if flags:
        for p, (_, _, _, h, w) in enumerate(planes):
            windows = (h // 4 - 1) * (w // 4 - 1)
            err = (val[:, p] - want_val[:, p]).abs().max().item()
            print(f"plane {p} {h}x{w}: {windows} windows, |ssim - definition| {err:.3e} (bound {windows * 2.0 ** -52:.3e})")
            assert err <= windows * 2.0 ** -52
    return sse, val


def u8_pair(n, frame, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (n, frame), dtype=np.uint8)
    noise = rng.integers(-20, 21, (n, frame))
    b = np.clip(a.astype(np.int64) + noise, 0, 255).astype(np.uint8)
    b[1] = rng.integers(0, 256, frame, dtype=np.uint8)      # one unrelated frame: low, even negative values
    return torch.from_numpy(a), torch.from_numpy(b)


def shapes():
    tc, br = tile()
    out = [(8, 8), (9, 11), (12, 8), (8, 43), (41, 8)]
    out += [(12, 4 * (tc + 1) + k) for k in (-4, 0, 4, 5)]     # a block short of the tile, the tile, a block past it
    out += [(4 * (br + 1) + k, 12) for k in (-4, 0, 4, 5)]     # the same down a band
    out += [(4 * (2 * br + 2) + 3, 4 * (2 * tc + 3) + 3)]      # 3 bands x 3 tiles, remainders both ways
    return out


@pytest.mark.parametrize("step", [1, 2, 3])
def test_u8_equals_definition(gpu, step):
    for k, (h, w) in enumerate(shapes()):
        a, b = u8_pair(3, 3 * h * w, 100 * step + k)
        print(f"step {step} {h}x{w}")
        check_against_definition(a, b, frame_planes(h, w, step), 1, dev=gpu)


@pytest.mark.parametrize("step", [1, 2, 3])
def test_u8_equal_frames(gpu, step):
    for h, w in ((8, 8), (9, 11), (41, 261)):
        a, _ = u8_pair(3, 3 * h * w, 7)
        sse, val = check_against_definition(a, a.clone(), frame_planes(h, w, step), 1, dev=gpu)
        assert bool((sse == 0).all()) and bool((val == 1.0).all())      # exactly 1.0


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (9, 11)])
def test_sse_alone_from_1x1(gpu, shape):
    h, w = shape
    for step in (1, 2, 3):
        a, b = u8_pair(3, 3 * h * w, 11)
        a[2], b[2] = 0, 255                                              # the largest error of the shape
        sse, val = check_against_definition(a, b, frame_planes(h, w, step), 0, dev=gpu)
        assert val is None and sse[2].tolist() == [255 * 255 * h * w] * 3
    if h < 8:   # and SSIM on it is refused, in Python as a ValueError
        f = torch.zeros((1, h, w, 3), dtype=torch.uint8, device=gpu)
        with pytest.raises(ValueError, match="8x8"):
            metrics.frame_metrics_u8(f, f)


@pytest.mark.parametrize("case", ["d10", "d10msb", "d12over", "d16extreme"])
@pytest.mark.parametrize("step", [1, 2, 3])
def test_u16_equals_definition(gpu, case, step):
    tc, br = tile()
    depth, shift = {"d10": (10, 0), "d10msb": (10, 6), "d12over": (12, 0), "d16extreme": (16, 0)}[case]
    maxval = (1 << depth) - 1
    for k, (h, w) in enumerate([(8, 8), (9, 11), (4 * (br + 2) + 1, 4 * (tc + 2) + 2)]):
        frame = 3 * h * w
        rng = np.random.default_rng(1000 * step + 10 * k + depth + shift)
        if case == "d16extreme":      # the largest sums: every block sum at its bound
            av, bv = np.zeros((3, frame), np.int64), np.full((3, frame), 65535, np.int64)
            av[1], bv[1] = rng.integers(0, 65536, frame), rng.integers(0, 65536, frame)
        else:
            av = rng.integers(0, maxval + 1, (3, frame))
            bv = np.clip(av + rng.integers(-maxval // 16, maxval // 16 + 1, (3, frame)), 0, maxval)
            if case == "d12over":     # some words above maxval: read as maxval
                av[:, ::7] = rng.integers(maxval + 1, 65536, av[:, ::7].shape)
                bv[:, ::5] = 65535
            av, bv = av << shift, bv << shift
        a = torch.from_numpy(av.astype(np.uint16))
        b = torch.from_numpy(bv.astype(np.uint16))
        print(f"{case} step {step} {h}x{w}")
        sse, _ = check_against_definition(a, b, frame_planes(h, w, step), 1, depth, shift, dev=gpu)
        if case == "d16extreme":
            assert sse[0].tolist() == [65535 * 65535 * h * w] * 3


# ---- the Net level -------------------------------------------------------------------------------
def assert_metrics(m, a, b, planes, depth, shift, names):
    want_sse, want_val = metrics._host_metrics(a.cpu(), b.cpu(), planes, depth, shift, True)
    assert m.plane_names == names and m.maxval == (1 << depth) - 1 and m.count == tuple(p[3] * p[4] for p in planes)
    assert m.sse.is_cuda and m.ssim.is_cuda and m.psnr().is_cuda
    assert torch.equal(m.sse.cpu(), want_sse)
    for p, pl in enumerate(planes):
        bound = (pl[3] // 4 - 1) * (pl[4] // 4 - 1) * 2.0 ** -52
        assert (m.ssim[:, p].cpu() - want_val[:, p]).abs().max().item() <= bound
    want_psnr = torch.stack([metrics.psnr(want_sse[:, p], c, m.maxval) for p, c in enumerate(m.count)], 1)
    assert torch.allclose(m.psnr().cpu(), want_psnr, rtol=1e-14, atol=0)


@pytest.mark.parametrize("layout", yuv.ALL_LAYOUTS)
def test_net_frame_metrics_yuv(gpu, layout):
    net = net_of(gpu, "fp32")
    h0, w0 = 34, 50
    rows = yuv.stack_rows(h0, layout)
    stack = stack_of((4, rows, w0), 21, gpu)
    a, b = stack[:-1], stack[1:]                       # two views of one stack
    planes = metrics.planes_of("yuv", h0, w0, layout)
    m = net.frame_metrics_yuv(a, b, layout=layout)
    assert_metrics(m, a, b, planes, 8, 0, ("y", "u", "v"))
    # the planes the map names are the ones split_planes returns
    for p, (x, y) in enumerate(zip(yuv.split_planes(a.cpu(), layout), yuv.split_planes(b.cpu(), layout))):
        assert torch.equal(m.sse[:, p].cpu(), metrics.plane_sse(x.to(torch.int64), y.to(torch.int64)))
    # the module function on device tensors is the same call with its own workspace
    m2 = metrics.frame_metrics_yuv(a, b, layout=layout)
    assert torch.equal(m2.sse, m.sse) and torch.equal(m2.ssim, m.ssim)
    wide = stack_of((3, rows, w0), 22, gpu, torch.uint16, 1023, 6)
    m16 = net.frame_metrics_yuv16(wide[:-1], wide[1:], layout=layout, depth=10, msb=True)
    assert_metrics(m16, wide[:-1], wide[1:], planes, 10, 6, ("y", "u", "v"))


def test_net_frame_metrics_rgb(gpu):
    net = net_of(gpu, "fp32")
    s8 = stack_of((4, 37, 50, 3), 23, gpu)
    assert_metrics(net.frame_metrics_u8(s8[:-1], s8[1:]), s8[:-1], s8[1:], metrics.planes_of("rgb", 37, 50), 8, 0,
                   ("r", "g", "b"))
    s16 = stack_of((4, 37, 50, 3), 24, gpu, torch.uint16, 4095)
    # truth frames gathered on the device (as int16: the same bits)
    truth = s16.view(torch.int16).index_select(0, torch.tensor([3, 0, 2], device=gpu)).view(torch.uint16)
    assert_metrics(net.frame_metrics_u16(s16[:3], truth, depth=12), s16[:3], truth, metrics.planes_of("rgb", 37, 50),
                   12, 0, ("r", "g", "b"))
    m = net.frame_metrics_u8(s8[:1, :3, :5].contiguous(), s8[1:2, :3, :5].contiguous(), ssim=False)
    assert m.ssim is None and m.count == (15, 15, 15)
    with pytest.raises(ValueError, match="8x8"):
        net.frame_metrics_u8(s8[:, :7].contiguous(), s8[:, :7].contiguous())
    with pytest.raises(RuntimeError, match="model on"):
        net.frame_metrics_u8(s8.cpu(), s8.cpu())


# ---- evaluate_y4m on the device ------------------------------------------------------------------
def moving_pattern(n, h0, w0, layout, dtype=np.uint8, maxval=255, cut_at=None):
    """n frames of ``layout``: a smooth pattern that moves two pixels a frame (from ``cut_at`` on
    another, inverted one: a hard cut)."""
    rows = yuv.stack_rows(h0, layout)
    yy, xx = np.mgrid[0:rows, 0:w0]
    out = []
    for k in range(n):
        v = 0.5 + 0.2 * np.sin((xx + k) / 6.0) + 0.15 * np.cos((yy - k) / 9.0)
        if cut_at is not None and k >= cut_at:
            v = 1.0 - v * ((xx // 4 + yy // 4) % 2)
        out.append(np.clip(v * maxval, 0, maxval).astype(dtype))
    return out


def y4m_of(frames, w0, h0, tag):
    src = io.BytesIO()
    wr = y4m.Writer(src, w0, h0, 24, 1, tag, depths=(8, 10, 12), chroma=yuv.CHROMAS)
    for f in frames:
        wr.write(f)
    src.seek(0)
    return src


def check_rows(res, net, frames, hold, layout, depth=8, gate=None):
    """Every row: forward_yuv of the item's pair alone at its t (replaced by the gate's frame where
    ``gate`` maps frame -> code), then the definition against the held-out frame; the baseline: the
    definition on the nearer input."""
    h0, w0 = res["summary"]["height"], res["summary"]["width"]
    planes = metrics.planes_of("yuv", h0, w0, layout)
    maxval = (1 << depth) - 1
    stack = torch.from_numpy(np.stack(frames))
    items, ignored = metrics.holdout_schedule(len(frames), hold)
    assert res["summary"]["ignored"] == ignored and res["summary"]["held_out"] == len(items) == len(res["rows"])
    for row, (frame, pair, t) in zip(res["rows"], items):
        assert (row["frame"], row["pair"], row["t"]) == (frame, pair, float(t))
        f0, f1 = stack[pair * hold:pair * hold + 1], stack[(pair + 1) * hold:(pair + 1) * hold + 1]
        code = 0 if gate is None else gate.get(frame, 0)
        assert row["gate"] == code
        if code:
            out = f0 if code == 1 else f1
        else:
            with torch.no_grad():
                if depth > 8:
                    out = net.forward_yuv16(f0.to(net_dev(net)), f1.to(net_dev(net)), t=float(t), layout=layout,
                                            depth=depth).cpu()
                else:
                    out = net.forward_yuv(f0.to(net_dev(net)), f1.to(net_dev(net)), t=float(t), layout=layout).cpu()
        truth = stack[frame:frame + 1]
        for got, cand in ((row, out), (row["baseline"], f0 if metrics.nearer_input(t) == 0 else f1)):
            sse, val = metrics._host_metrics(cand, truth, planes, depth, 0, True)
            assert got["sse"] == sse[0].tolist()
            for p, pl in enumerate(planes):
                assert abs(got["ssim"][p] - val[0, p].item()) <= (pl[3] // 4 - 1) * (pl[4] // 4 - 1) * 2.0 ** -52
            psnr = [metrics.psnr(v, pl[3] * pl[4], maxval) for v, pl in zip(got["sse"], planes)]
            assert got["psnr"] == [v if np.isfinite(v) else None for v in psnr]


def net_dev(net):
    return next(net.parameters()).device


@pytest.mark.parametrize("hold,batch", [(2, 4), (3, 4)])
def test_evaluate_y4m_c420(gpu, hold, batch):
    net = net_of(gpu, "fp32")
    w0, h0 = 48, 32
    frames = moving_pattern(7, h0, w0, "i420")
    rep = io.StringIO()
    logs = []
    res = cv.evaluate_y4m(net, y4m_of(frames, w0, h0, "420"), hold=hold, batch=batch, log=logs.append, report=rep)
    assert len(res["rows"]) == {2: 3, 3: 4}[hold]
    s = res["summary"]
    assert (s["tag"], s["precision"], s["hold"], s["frames"], s["cut_pairs"], s["duplicate_pairs"]) == \
        ("C420", "fp32", hold, 7, 0, 0)
    check_rows(res, net, frames, hold, "i420")
    assert json.loads(rep.getvalue()) == res                   # the report round-trips
    assert len(logs) == 1 and "0 frames after the last input ignored" in logs[0]
    for key in ("psnr_mean", "psnr_global", "ssim_mean"):
        assert len(s[key]) == 3 and len(s["baseline"][key]) == 3


def test_evaluate_y4m_scene_gate(gpu):
    """Frames 0..4 move, 5.. are another scene; hold 3: pair 0 = frames (0, 3), pair 1 = (3, 6) holds the
    cut.  Its rows carry the nearer frame's code by t: frame 4 (t = 1/3) the first, frame 5 (2/3) the
    second, and the nearer frame's metrics."""
    net = net_of(gpu, "fp32")
    w0, h0 = 48, 32
    frames = moving_pattern(7, h0, w0, "i420", cut_at=5)
    res = cv.evaluate_y4m(net, y4m_of(frames, w0, h0, "420"), hold=3, batch=3, scene_threshold=40.0,
                          log=lambda *a: None)
    check_rows(res, net, frames, 3, "i420", gate={4: 1, 5: 2})
    assert res["summary"]["cut_pairs"] == 1 and res["summary"]["duplicate_pairs"] == 0
    assert res["summary"]["scene_threshold"] == 40.0
    for row in res["rows"][2:]:
        assert row["sse"] == row["baseline"]["sse"] and row["ssim"] == row["baseline"]["ssim"]
    # a repeated input frame: the pair is a duplicate, its rows carry code 1
    still = [frames[0]] * 3
    res = cv.evaluate_y4m(net, y4m_of(still, w0, h0, "420"), hold=2, scene_threshold=40.0, log=lambda *a: None)
    assert [r["gate"] for r in res["rows"]] == [1] and res["rows"][0]["psnr"] == [None] * 3
    assert (res["summary"]["cut_pairs"], res["summary"]["duplicate_pairs"]) == (0, 1)


@pytest.mark.parametrize("tag,layout,depth", [("420p10", "i420", 10), ("444", "i444", 8)])
def test_evaluate_y4m_other_formats(gpu, tag, layout, depth):
    net = net_of(gpu, "fp32")
    w0, h0 = 48, 32
    deep = depth > 8
    frames = moving_pattern(5, h0, w0, layout, np.uint16 if deep else np.uint8, (1 << depth) - 1)
    res = cv.evaluate_y4m(net, y4m_of([f.reshape(-1) for f in frames], w0, h0, tag), hold=2, batch=2,
                          log=lambda *a: None)
    assert res["summary"]["tag"] == "C" + tag and res["summary"]["bit_depth"] == depth
    check_rows(res, net, frames, 2, layout, depth)
