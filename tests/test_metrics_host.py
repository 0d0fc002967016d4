"""CPU: the definitions of rrin_amd.metrics (squared error, PSNR, the integer 8x8 / step-4 SSIM, the
plane maps), the hold-out schedule, the argument rules of rrin_frame_metrics_* (no launch), the
``evaluate`` subcommand's parser and evaluate_y4m end to end on a host model."""
import ctypes as C
import io
import json
import math
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

from rrin_amd import _lib, metrics, y4m, yuv
from rrin_amd import convert as cv

from .test_retime_host import HostItems, y4m_bytes

FAKE = 1 << 30
E_SHAPE, E_ARG, E_WORKSPACE = -1, -2, -3


def rand_plane(shape, maxval, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, maxval + 1, shape, dtype=np.int64))


# ---- the definitions ---------------------------------------------------------------------------
def test_constants_at_8_bits():
    assert metrics.ssim_constants(255) == (416, 235963)


@pytest.mark.parametrize("depth", [8, 10, 16])
def test_equal_frames_have_ssim_exactly_one(depth):
    maxval = (1 << depth) - 1
    x = rand_plane((2, 19, 23), maxval, depth)
    v = metrics.window_values(x, x.clone(), maxval)
    assert v.shape == (2, 3, 4) and v.dtype == torch.float64
    assert bool((v == 1.0).all())
    assert metrics.plane_ssim(x, x.clone(), maxval).tolist() == [1.0, 1.0]
    assert metrics.plane_sse(x, x.clone()).tolist() == [0, 0]


def statistical_ssim(x, y, maxval):
    """The plain form: per 8x8 window (step 4) the means, the unbiased variances (the 64/63 factor) and
    covariance of its 64 samples, in float64, with the definition's constants brought to that scale:
    c1 = C1 / 64^2 on the means, c2 = C2 / (64 * 63) on the variances."""
    x, y = x.double(), y.double()
    bh, bw = x.shape[-2] // 4, x.shape[-1] // 4
    big1, big2 = metrics.ssim_constants(maxval)
    c1, c2 = big1 / 4096.0, big2 / 4032.0
    vals = []
    for i in range(bh - 1):
        for j in range(bw - 1):
            a, b = x[4 * i:4 * i + 8, 4 * j:4 * j + 8].reshape(-1), y[4 * i:4 * i + 8, 4 * j:4 * j + 8].reshape(-1)
            ma, mb = a.mean(), b.mean()
            va, vb = ((a - ma) ** 2).mean() * (64.0 / 63.0), ((b - mb) ** 2).mean() * (64.0 / 63.0)
            cab = ((a - ma) * (b - mb)).mean() * (64.0 / 63.0)
            vals.append(((2 * ma * mb + c1) * (2 * cab + c2) / ((ma * ma + mb * mb + c1) * (va + vb + c2))).item())
    return sum(vals) / len(vals)


@pytest.mark.parametrize("depth", [8, 10, 16])
def test_definition_agrees_with_the_statistical_form(depth):
    maxval = (1 << depth) - 1
    x = rand_plane((20, 28), maxval, 10 + depth)
    y = (x + rand_plane((20, 28), maxval // 8, 20 + depth) - maxval // 16).clamp(0, maxval)
    for a, b in ((x, y), (x, rand_plane((20, 28), maxval, 30 + depth))):
        got = metrics.plane_ssim(a, b, maxval).item()
        assert abs(got - statistical_ssim(a, b, maxval)) <= 1e-12


def test_denominator_is_positive():
    for depth in (8, 16):
        maxval = (1 << depth) - 1
        x = torch.zeros((8, 8), dtype=torch.int64)
        y = torch.full((8, 8), maxval, dtype=torch.int64)
        v = metrics.window_values(x, y, maxval)
        assert torch.isfinite(v).all() and 0 < v.item() < 1e-3


def test_remainder_samples_count_for_sse_only():
    x, y = rand_plane((9, 11), 255, 1), rand_plane((9, 11), 255, 2)
    assert metrics.window_values(x, y, 255).shape == (1, 1)
    assert metrics.plane_ssim(x, y, 255).item() == metrics.plane_ssim(x[:8, :8], y[:8, :8], 255).item()
    assert metrics.plane_sse(x, y).item() == sum((int(a) - int(b)) ** 2 for a, b in zip(x.reshape(-1), y.reshape(-1)))
    assert metrics.plane_sse(x, y).item() != metrics.plane_sse(x[:8, :8], y[:8, :8]).item()
    with pytest.raises(ValueError, match="8x8"):
        metrics.window_values(x[:7], y[:7], 255)


@pytest.mark.parametrize("layout", yuv.ALL_LAYOUTS)
@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16])
def test_plane_maps_match_split_planes(layout, dtype):
    h0, w0 = 6, 10
    rows = yuv.stack_rows(h0, layout)
    vals = np.random.default_rng(5).integers(0, 250, (3, rows, w0))
    frames = torch.from_numpy(vals.astype(np.uint16 if dtype == torch.uint16 else np.uint8))
    planes = metrics.planes_of("yuv", h0, w0, layout)
    assert len(planes) == 3
    for pl, want in zip(planes, yuv.split_planes(frames, layout)):
        got = metrics.gather_plane(frames, pl)
        assert got.shape == want.shape and torch.equal(got.view(torch.uint8), want.contiguous().view(torch.uint8))


def test_plane_maps_rgb_and_y():
    rgb = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (2, 5, 7, 3), dtype=np.uint8))
    assert metrics.planes_of("rgb", 5, 7) == [(0, 3, 21, 5, 7), (1, 3, 21, 5, 7), (2, 3, 21, 5, 7)]
    for ch, pl in enumerate(metrics.planes_of("rgb", 5, 7)):
        assert torch.equal(metrics.gather_plane(rgb, pl), rgb[..., ch])
    assert metrics.planes_of("y", 5, 7) == [(0, 1, 7, 5, 7)]
    with pytest.raises(ValueError):
        metrics.planes_of("yuv", 5, 7, "nv12")
    with pytest.raises(ValueError):
        metrics.planes_of("bgr", 5, 7)


def test_samples_of_16_bit_words():
    w = torch.tensor([0, 1023, 1024, 65535, 1023 << 6, 65535], dtype=torch.int32).to(torch.int16).view(torch.uint16)
    assert metrics.samples_of(w, 10, 0).tolist() == [0, 1023, 1023, 1023, 1023, 1023]
    assert metrics.samples_of(w, 10, 6).tolist() == [0, 15, 16, 1023, 1023, 1023]


def test_psnr():
    assert metrics.psnr(0, 99, 255) == math.inf
    assert metrics.psnr(99 * 255 * 255, 99, 255) == 0.0
    assert abs(metrics.psnr(650, 100, 255) - 10 * math.log10(255 * 255 * 100 / 650)) < 1e-12
    t = metrics.psnr(torch.tensor([[0, 650]]), 100, 255)
    assert t.dtype == torch.float64 and t[0, 0].item() == math.inf
    assert t[0, 1].item() == pytest.approx(metrics.psnr(650, 100, 255), abs=1e-12)
    m = metrics.FrameMetrics(torch.tensor([[0, 650]]), None, (100, 100), 255, ("a", "b"))
    assert m.psnr().tolist() == t.tolist()


def test_public_functions_on_cpu_tensors():
    rng = np.random.default_rng(7)
    a = torch.from_numpy(rng.integers(0, 256, (2, 9, 11, 3), dtype=np.uint8))
    b = torch.from_numpy(rng.integers(0, 256, (2, 9, 11, 3), dtype=np.uint8))
    m = metrics.frame_metrics_u8(a, b)
    assert m.plane_names == ("r", "g", "b") and m.count == (99, 99, 99) and m.maxval == 255
    assert m.sse.shape == (2, 3) and m.sse.dtype == torch.int64 and m.ssim.dtype == torch.float64
    for ch in range(3):
        x, y = a[..., ch].to(torch.int64), b[..., ch].to(torch.int64)
        assert torch.equal(m.sse[:, ch], metrics.plane_sse(x, y))
        assert torch.equal(m.ssim[:, ch], metrics.plane_ssim(x, y, 255))
    assert metrics.frame_metrics_u8(a, a).ssim.tolist() == [[1.0] * 3] * 2
    small = metrics.frame_metrics_u8(a[:, :3, :5], b[:, :3, :5], ssim=False)
    assert small.ssim is None and small.count == (15, 15, 15)
    with pytest.raises(ValueError, match="8x8"):
        metrics.frame_metrics_u8(a[:, :7], b[:, :7])
    with pytest.raises(ValueError, match="8x8"):
        metrics.frame_metrics_yuv(torch.zeros(1, 12, 8, dtype=torch.uint8), torch.zeros(1, 12, 8, dtype=torch.uint8),
                                  "i420")   # 4x4 chroma planes
    with pytest.raises(TypeError):
        metrics.frame_metrics_u16(a, b)
    w = torch.from_numpy(rng.integers(0, 5000, (1, 24, 16)).astype(np.uint16))
    m16 = metrics.frame_metrics_yuv16(w, w.clone(), "i420", depth=12)
    assert m16.plane_names == ("y", "u", "v") and m16.count == (256, 64, 64) and m16.maxval == 4095
    assert m16.sse.tolist() == [[0, 0, 0]] and m16.ssim.tolist() == [[1.0, 1.0, 1.0]]


# ---- the hold-out schedule -------------------------------------------------------------------
@pytest.mark.parametrize("hold", [2, 3])
@pytest.mark.parametrize("n", [3, 4, 5, 7])
def test_holdout_schedule(hold, n):
    if n < hold + 1:
        with pytest.raises(ValueError, match="at least"):
            metrics.holdout_schedule(n, hold)
        return
    items, ignored = metrics.holdout_schedule(n, hold)
    pairs = (n - 1) // hold
    assert ignored == n - 1 - pairs * hold and 0 <= ignored < hold
    assert [f for f, _, _ in items] == [f for f in range(pairs * hold) if f % hold]   # every frame between inputs
    for frame, pair, t in items:
        assert pair == frame // hold and t == Fr(frame % hold, hold) and 0 < t < 1
    assert items == [it for p in range(pairs) for it in metrics.holdout_pair_items(p, hold)]


def test_holdout_schedule_rejects():
    for n, hold in ((2, 2), (3, 3), (1, 2)):
        with pytest.raises(ValueError):
            metrics.holdout_schedule(n, hold)
    for hold in (1, 0, 2.0, True):
        with pytest.raises(ValueError):
            metrics.holdout_schedule(9, hold)
    assert metrics.nearer_input(Fr(1, 2)) == 0 and metrics.nearer_input(Fr(1, 3)) == 0
    assert metrics.nearer_input(Fr(2, 3)) == 1


# ---- the C argument rules: refused before any launch -------------------------------------------
def plane_array(*planes):
    return (_lib.Plane * len(planes))(*[_lib.Plane(off, pitch, step, h, w, 0) for off, step, pitch, h, w in planes])


def call_u8(planes, n=1, a=FAKE, b=FAKE, stride=1 << 20, flags=1, sse=FAKE, ssim=FAKE, ws=FAKE, ws_bytes=1 << 20,
            n_planes=None):
    arr = plane_array(*planes) if planes else None
    return _lib.lib().rrin_frame_metrics_u8(a, stride, b, stride, n, arr, len(planes) if n_planes is None else n_planes,
                                            flags, sse, ssim, ws, ws_bytes, None)


def call_u16(planes, a=FAKE, b=FAKE, depth=10, shift=0, flags=1):
    return _lib.lib().rrin_frame_metrics_u16(a, 1 << 20, b, 1 << 20, 1, plane_array(*planes), len(planes), flags, depth,
                                             shift, FAKE, FAKE, FAKE, 1 << 20, None)


def test_c_argument_rules():
    lib = _lib.lib()
    good = [(0, 1, 16, 16, 16)]
    for kw in ({"a": None}, {"b": None}, {"sse": None}, {"ssim": None}, {"ws": None}):
        assert call_u8(good, **kw) == E_ARG
    assert call_u8([], n_planes=1) == E_ARG                      # no planes
    assert call_u8(good, n_planes=0) == E_ARG
    assert call_u8(good * 5) == E_ARG
    assert call_u8([(0, 4, 64, 16, 16)]) == E_ARG                # step 4
    assert call_u8([(0, 0, 16, 16, 16)]) == E_ARG
    assert call_u8([(-1, 1, 16, 16, 16)]) == E_ARG
    assert call_u8([(0, 1, 15, 16, 16)]) == E_ARG                # pitch below a row
    assert call_u8(good, stride=255) == E_ARG                    # a stride below the plane's reach
    assert call_u8(good, flags=2) == E_ARG
    assert call_u8(good, sse=FAKE + 4) == E_ARG
    assert call_u8(good, n=0) == E_SHAPE
    assert call_u8([(0, 1, 16, 0, 16)]) == E_SHAPE
    assert call_u8([(0, 1, 8, 7, 8)]) == E_SHAPE                 # SSIM on a 7x8 plane
    assert call_u8([(0, 1, 7, 8, 7)]) == E_SHAPE
    need = lib.rrin_frame_metrics_workspace_bytes(3, plane_array(*good), 1, 1)
    assert need > 0 and need % 8 == 0
    assert call_u8(good, n=3, ws_bytes=need - 1) == E_WORKSPACE  # a short workspace
    assert lib.rrin_frame_metrics_workspace_bytes(3, plane_array((0, 1, 8, 7, 8)), 1, 1) == E_SHAPE
    assert lib.rrin_frame_metrics_workspace_bytes(3, plane_array((0, 1, 8, 7, 8)), 1, 0) > 0   # SSE alone: from 1x1
    assert lib.rrin_frame_metrics_workspace_bytes(1, plane_array((0, 4, 64, 16, 16)), 1, 0) == E_ARG
    # a 1x1 plane without the flag passes every check but the workspace, which is asked for last
    assert call_u8([(0, 1, 1, 1, 1)], flags=0, ssim=None, ws_bytes=0) == E_WORKSPACE
    # 16-bit words: an odd address, the depth and shift rules of rrin_pair_sad_u16
    assert call_u16(good, a=FAKE + 1) == E_ARG and call_u16(good, b=FAKE + 1) == E_ARG
    assert call_u16(good, depth=8) == E_ARG and call_u16(good, depth=17) == E_ARG
    assert call_u16(good, depth=10, shift=7) == E_ARG and call_u16(good, shift=-1) == E_ARG
    assert call_u16([(0, 1, 8, 7, 8)]) == E_SHAPE
    tc, br = C.c_int32(), C.c_int32()
    assert lib.rrin_frame_metrics_tile(C.byref(tc), C.byref(br)) == 0 and tc.value >= 1 and br.value >= 1
    assert lib.rrin_frame_metrics_tile(None, C.byref(br)) == E_ARG


# ---- the command line --------------------------------------------------------------------------
def test_parser_accepts_evaluate_and_the_old_lines():
    from rrin_amd.__main__ import build_parser
    p = build_parser()
    a = p.parse_args(["--model_name", "M", "evaluate", "--y4m_in", "clip.y4m"])
    assert (a.mode, a.y4m_in, a.hold, a.batch, a.precision, a.scene_threshold, a.report) == \
        ("evaluate", "clip.y4m", 2, 4, "fp32", None, None)
    a = p.parse_args(["--model_name", "M", "evaluate", "--y4m_in", "-", "--hold", "3", "--batch", "2", "--precision",
                      "fp16", "--scene_threshold", "12.5", "--report", "out.json"])
    assert (a.hold, a.batch, a.precision, a.scene_threshold, a.report) == (3, 2, "fp16", 12.5, "out.json")
    with pytest.raises(SystemExit):
        p.parse_args(["--model_name", "M", "evaluate"])          # --y4m_in is required
    c = p.parse_args(["--model_name", "M", "convert", "--sf", "1", "--fps", "30", "--image_folder", "d"])
    assert c.mode == "convert" and c.sf == 1 and c.batch == 4 and c.y4m_in is None
    t = p.parse_args(["--model_name", "M", "train", "--train_folder", "d"])
    assert t.mode == "train"


# ---- evaluate_y4m on a host model ----------------------------------------------------------------
def test_evaluate_y4m_on_a_host_model():
    w, h = 48, 32
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 150, w * h * 3 // 2).astype(np.uint8) for _ in range(5)]
    model, logs, rep = HostItems(), [], io.StringIO()
    res = cv.evaluate_y4m(model, y4m_bytes(frames, w, h, "420"), hold=3, batch=4, log=logs.append, report=rep)
    # frames 0 and 3 are inputs, 1 and 2 held out, 4 comes after the last input
    rows, s = res["rows"], res["summary"]
    assert [(r["frame"], r["pair"], r["t"], r["gate"]) for r in rows] == [(1, 0, 1 / 3, 0), (2, 0, 2 / 3, 0)]
    assert (s["frames"], s["held_out"], s["ignored"], s["hold"], s["tag"]) == (5, 2, 1, 3, "C420")
    assert (s["cut_pairs"], s["duplicate_pairs"], s["planes"]) == (0, 0, ["y", "u", "v"])
    assert len(logs) == 1 and "1 frames after the last input ignored" in logs[0]
    assert [c[:2] for c in model.calls] == [("yuv", (2, 48, 48))] and model.calls[0][3:6] == ([0, 0], [1 / 3, 2 / 3], "i420")
    stack = torch.from_numpy(np.stack(frames)).view(5, 48, 48)
    for r, near in zip(rows, (0, 3)):   # the baseline: the nearer input, by hand
        want = metrics.frame_metrics_yuv(stack[near:near + 1], stack[r["frame"]:r["frame"] + 1], "i420")
        assert r["baseline"]["sse"] == want.sse[0].tolist()
        assert r["baseline"]["ssim"] == want.ssim[0].tolist()
        assert r["baseline"]["psnr"] == [metrics.psnr(v, c, 255) for v, c in zip(want.sse[0].tolist(), want.count)]
        out = HostItems.forward_pair(stack[0:1], stack[3:4], r["t"])
        got = metrics.frame_metrics_yuv(out, stack[r["frame"]:r["frame"] + 1], "i420")
        assert (r["sse"], r["ssim"]) == (got.sse[0].tolist(), got.ssim[0].tolist())
        assert r["psnr"] == [metrics.psnr(v, c, 255) for v, c in zip(r["sse"], got.count)]
    # the summary: global PSNR from the summed squared error, the mean of the rows
    for p, count in enumerate((w * h, w * h // 4, w * h // 4)):
        total = sum(r["sse"][p] for r in rows)
        assert s["psnr_global"][p] == metrics.psnr(total, 2 * count, 255)
        assert s["psnr_mean"][p] == sum(r["psnr"][p] for r in rows) / 2
        assert s["ssim_mean"][p] == sum(r["ssim"][p] for r in rows) / 2
        assert s["baseline"]["ssim_mean"][p] == sum(r["baseline"]["ssim"][p] for r in rows) / 2
    assert json.loads(rep.getvalue()) == res
    with pytest.raises(ValueError, match="at least"):
        cv.evaluate_y4m(HostItems(), y4m_bytes(frames[:3], w, h, "420"), hold=3, log=logs.append)
    with pytest.raises(ValueError):
        cv.evaluate_y4m(HostItems(), y4m_bytes(frames, w, h, "420"), hold=1, log=logs.append)


def test_evaluate_y4m_equal_frames_report_null_psnr():
    w, h = 16, 16
    frames = [np.full(w * h * 3, 7, np.uint16)] * 3
    res = cv.evaluate_y4m(HostItems(), y4m_bytes(frames, w, h, "444p10"), hold=2, log=lambda *a: None)
    (row,) = res["rows"]
    assert row["baseline"]["psnr"] == [None] * 3 and row["baseline"]["ssim"] == [1.0] * 3
    assert res["summary"]["baseline"]["psnr_mean"] == [None] * 3 and res["summary"]["bit_depth"] == 10
    json.dumps(res, allow_nan=False)
