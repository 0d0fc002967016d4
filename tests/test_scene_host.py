"""CPU: the scene gate's host side -- the integer rule of convert.scene_gate_codes / apply_gate_u8
on hand cases, interpolate_folder(scene_threshold=) with a CPU stand-in model that applies the two
reference functions, the command-line flag, and the argument validation of the three C entry
points (nothing is launched: the pointers are fabricated and this machine may have no GPU)."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from rrin_amd import _lib
from rrin_amd import convert as cv
from rrin_amd.__main__ import build_parser

FAKE = 1 << 30  # a fabricated non-null, 8-byte aligned device pointer: never dereferenced
H0, W0 = 4, 5
BYTES = H0 * W0 * 3


def pair_with_sad(sad):
    """Two uint8 [1,4,5,3] frames whose sum of absolute differences is exactly ``sad``."""
    f0 = torch.full((1, H0, W0, 3), 7, dtype=torch.uint8)
    d = torch.zeros(BYTES, dtype=torch.int64)
    q, r = divmod(sad, 248)
    assert q < BYTES
    d[:q] = 248
    d[q] = r
    return f0, (f0.view(-1).to(torch.int64) + d).to(torch.uint8).view(1, H0, W0, 3)


def test_limit_and_cut_code():
    assert cv.scene_limit(20, 37, 50) == 20 * 37 * 50 * 3
    assert cv.scene_limit(0.5, 1, 1) == 1               # floor(1.5)
    assert cv.scene_limit(0, 8, 8) == 0 and cv.scene_limit(255, 2, 2) == 255 * 12
    for bad in (-0.1, 255.5, float("nan")):
        with pytest.raises(ValueError):
            cv.scene_limit(bad, 4, 4)
    assert [cv.scene_cut_code(t) for t in (0.0, 0.25, 0.4999, 0.5, 0.75, 1.0)] == [1, 1, 1, 2, 2, 2]
    assert cv.scene_cut_code(torch.tensor(0.5)) == 2 and cv.scene_cut_code(torch.tensor([0.25])) == 1
    with pytest.raises(ValueError):
        cv.scene_cut_code(torch.tensor([0.25, 0.75]))


def test_gate_codes_on_hand_cases():
    th = 10.0
    limit = cv.scene_limit(th, H0, W0)                  # 600
    assert limit == 600
    cases = [(0, 1, 1), (1, 0, 0), (limit, 0, 0), (limit + 1, 1, 2), (248 * BYTES - 5, 1, 2)]
    for sad, at_025, at_05 in cases:                    # a pair exactly at the limit is not a cut
        f0, f1 = pair_with_sad(sad)
        assert int((f0.long() - f1.long()).abs().sum()) == sad
        assert cv.scene_gate_codes(f0, f1, th, 0.25).tolist() == [at_025], sad
        assert cv.scene_gate_codes(f0, f1, th, 0.5).tolist() == [at_05], sad
        assert cv.scene_gate_codes(f1, f0, th, 0.75).tolist() == [at_05], sad   # |a - b|: symmetric
    # a batch, and the dtype
    f0 = torch.cat([pair_with_sad(s)[0] for s, _, _ in cases])
    f1 = torch.cat([pair_with_sad(s)[1] for s, _, _ in cases])
    codes = cv.scene_gate_codes(f0, f1, th, 0.5)
    assert codes.dtype == torch.int32 and codes.tolist() == [c for _, _, c in cases]
    # threshold 0: every pair that differs at all is a cut; 255: none can be
    assert cv.scene_gate_codes(f0, f1, 0, 0.5).tolist() == [1, 2, 2, 2, 2]
    assert cv.scene_gate_codes(f0, f1, 255, 0.5).tolist() == [1, 0, 0, 0, 0]


def test_apply_gate():
    rng = np.random.default_rng(3)
    out, f0, f1 = (torch.from_numpy(rng.integers(0, 256, (5, H0, W0, 3), dtype=np.uint8)) for _ in range(3))
    keep = out.clone()
    got = cv.apply_gate_u8(out, f0, f1, torch.tensor([0, 1, 2, 7, 1], dtype=torch.int32))
    assert got.dtype == torch.uint8 and torch.equal(out, keep)          # a new tensor
    for p, want in enumerate((out, f0, f1, out, f0)):
        assert torch.equal(got[p], want[p]), p


class GatedU8Model:
    """A CPU model for the byte pipeline: the blend of the two frames, gated by the reference rule."""

    def __init__(self, accepts_threshold=True):
        self.calls = []
        self.last_gate = None
        if not accepts_threshold:
            self.interpolate_u8 = lambda f0, f1, ts: self._run(f0, f1, ts, None)

    def _run(self, f0, f1, ts, scene_threshold):
        self.calls.append(scene_threshold)
        outs = []
        for t in ts:
            o = ((1 - t) * f0.float() + t * f1.float()).to(torch.uint8)
            if scene_threshold is not None:
                self.last_gate = cv.scene_gate_codes(f0, f1, scene_threshold, t)
                o = cv.apply_gate_u8(o, f0, f1, self.last_gate)
            outs.append(o)
        return outs

    def interpolate_u8(self, f0, f1, ts, scene_threshold=None):
        return self._run(f0, f1, ts, scene_threshold)


def scene_frames(h0=37, w0=50):
    """Six frames of two shots: a smooth ramp shifted by one pixel per frame with frame 3 a repeat
    of frame 2, then the inverted, flipped ramp and its shift.  Pairs 0..4: ordinary, duplicate,
    ordinary, cut, ordinary."""
    y, x, c = np.meshgrid(np.arange(h0), np.arange(w0), np.arange(3), indexing="ij")
    ramp = ((2 * x + y + 40 * c) % 256).astype(np.uint8)
    shot2 = np.ascontiguousarray((255 - ramp)[::-1])
    return [ramp, np.roll(ramp, 1, axis=1), np.roll(ramp, 1, axis=1), np.roll(ramp, 2, axis=1), shot2,
            np.roll(shot2, 1, axis=1)]


def write_frames(folder, frames):
    os.makedirs(folder)
    for k, f in enumerate(frames):
        Image.fromarray(f).save(os.path.join(folder, f"{k + 1:09d}.png"))


def read(path):
    return np.asarray(Image.open(path).convert("RGB"))


def test_folder_run_gates_counts_and_refuses_the_float_pipeline(tmp_path):
    frames = scene_frames()
    src = str(tmp_path / "in")
    write_frames(src, frames)
    st = torch.from_numpy(np.stack(frames))
    # the margins of these inputs: ordinary pairs far below 20, the cuts far above
    mean = (st[:-1].long() - st[1:].long()).abs().reshape(5, -1).float().mean(1)
    assert mean[1] == 0 and max(mean[0], mean[2], mean[4]) < 10 and mean[3] > 40, mean
    sf = 3
    model, logs = GatedU8Model(), []
    a = str(tmp_path / "gated")
    n = cv.interpolate_folder(model, src, a, sf=sf, batch=2, device=None, u8=True, scene_threshold=20, log=logs.append)
    assert n == 1 + 5 * (sf + 1) and model.calls == [20, 20, 20]
    assert logs[-1].endswith("scene gate (threshold 20): 1 cut pairs, 1 duplicate pairs"), logs
    plain = GatedU8Model()
    b = str(tmp_path / "plain")
    logs2 = []
    cv.interpolate_folder(plain, src, b, sf=sf, batch=2, device=None, u8=True, log=logs2.append)
    assert plain.calls == [None, None, None] and "scene gate" not in logs2[-1]
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))
    for k in range(5):                                   # pair k: files base+1 .. base+sf, then frame k+1
        base = 1 + k * (sf + 1)
        for i in range(sf):
            name = f"{base + i + 1:09d}.png"
            got = read(os.path.join(a, name))
            if k == 1:                                    # the repeated frame
                np.testing.assert_array_equal(got, frames[1])
            elif k == 3:                                  # the cut: the nearer input, the second from t = 0.5
                np.testing.assert_array_equal(got, frames[k] if (i + 1) / (sf + 1) < 0.5 else frames[k + 1])
            else:
                assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name
    # a model without the keyword keeps working while the gate is off, and is refused with it
    old = GatedU8Model(accepts_threshold=False)
    cv.interpolate_folder(old, src, str(tmp_path / "old"), sf=1, batch=4, device=None, u8=True, log=lambda *x: None)
    assert old.calls == [None, None]
    with pytest.raises(TypeError):
        cv.interpolate_folder(old, src, str(tmp_path / "old2"), sf=1, device=None, u8=True, scene_threshold=20,
                              log=lambda *x: None)
    # the gate works on bytes: no float pipeline
    with pytest.raises(ValueError, match="byte pipeline"):
        cv.interpolate_folder(model, src, str(tmp_path / "f32"), sf=1, device=None, u8=False, scene_threshold=20,
                              log=lambda *x: None)
    with pytest.raises(ValueError, match="byte pipeline"):      # "auto" resolves to False on the CPU
        cv.interpolate_folder(model, src, str(tmp_path / "auto"), sf=1, device=None, scene_threshold=20,
                              log=lambda *x: None)


def test_parser_takes_scene_threshold():
    p = build_parser()
    base = ["--model_name", "M", "convert", "--sf", "1", "--fps", "30", "--image_folder", "d"]
    assert p.parse_args(base).scene_threshold is None
    assert p.parse_args(base + ["--scene_threshold", "12.5"]).scene_threshold == 12.5


def test_entry_points_validate_before_any_launch():
    L = _lib.lib()
    E_SHAPE, E_ARG = -1, -2
    frame = 17 * 33 * 3
    sad = L.rrin_pair_sad_u8
    assert sad(None, FAKE, frame, 3, 17, 33, FAKE, None) == E_ARG
    assert sad(FAKE, None, frame, 3, 17, 33, FAKE, None) == E_ARG
    assert sad(FAKE, FAKE, frame, 3, 17, 33, None, None) == E_ARG
    assert sad(FAKE, FAKE, frame, 0, 17, 33, FAKE, None) == E_SHAPE
    assert sad(FAKE, FAKE, frame, 3, 0, 33, FAKE, None) == E_SHAPE
    assert sad(FAKE, FAKE, frame, 3, 17, 0, FAKE, None) == E_SHAPE
    assert sad(FAKE, FAKE, frame - 1, 3, 17, 33, FAKE, None) == E_ARG
    gfs = L.rrin_gate_from_sad_u8
    assert gfs(None, 3, 100, 1, FAKE, None) == E_ARG
    assert gfs(FAKE, 3, 100, 1, None, None) == E_ARG
    assert gfs(FAKE, 3, 100, 0, FAKE, None) == E_ARG
    assert gfs(FAKE, 3, 100, 3, FAKE, None) == E_ARG
    assert gfs(FAKE, 0, 100, 2, FAKE, None) == E_SHAPE
    gf = L.rrin_gate_frames_u8
    assert gf(None, FAKE, frame, 3, 17, 33, FAKE, FAKE, None) == E_ARG
    assert gf(FAKE, None, frame, 3, 17, 33, FAKE, FAKE, None) == E_ARG
    assert gf(FAKE, FAKE, frame, 3, 17, 33, None, FAKE, None) == E_ARG
    assert gf(FAKE, FAKE, frame, 3, 17, 33, FAKE, None, None) == E_ARG
    assert gf(FAKE, FAKE, frame, 0, 17, 33, FAKE, FAKE, None) == E_SHAPE
    assert gf(FAKE, FAKE, frame, 3, 17, -1, FAKE, FAKE, None) == E_SHAPE
    assert gf(FAKE, FAKE, frame - 1, 3, 17, 33, FAKE, FAKE, None) == E_ARG
