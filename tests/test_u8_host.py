"""CPU: the 8-bit frame path's host side -- rrin_net_u8_fwd's argument validation (nothing is
launched), the two pure-torch helpers of convert.py against load_frame / to_uint8_image, and the
byte pipeline of interpolate_folder against the float one with a CPU stand-in model."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from PIL import Image

from rrin_amd import _lib
from rrin_amd import convert as cv

FAKE = 1 << 30  # a fabricated non-null device pointer: never dereferenced


def _u8_desc(h0, w0, h, w, prec=_lib.PREC_F32R, f0=FAKE):
    d = _lib.NetU8Desc()
    d.net.n, d.net.h, d.net.w, d.net.prec = 1, h, w, prec
    d.net.coef = d.net.workspace = FAKE
    d.net.workspace_bytes = 1 << 40
    d.net.convs = C.cast(FAKE, C.POINTER(_lib.ConvWeights))
    d.net.heads = C.cast(FAKE, C.POINTER(_lib.HeadWeights))
    d.f0, d.f1, d.out_u8 = f0, FAKE, FAKE
    d.img_stride = h0 * w0 * 3
    d.h0, d.w0 = h0, w0
    return d


def test_net_u8_fwd_validates_before_any_launch():
    """Shape and argument errors come back before any HIP call: the pointers are fabricated and
    this machine may have no GPU."""
    fwd = _lib.lib().rrin_net_u8_fwd
    E_SHAPE, E_ARG = -1, -2
    assert fwd(C.byref(_u8_desc(37, 50, 32, 64)), None) == E_SHAPE     # h != round_up(h0, 16)
    assert fwd(C.byref(_u8_desc(37, 50, 48, 48)), None) == E_SHAPE     # w != round_up(w0, 16)
    assert fwd(C.byref(_u8_desc(37, 0, 48, 16)), None) == E_SHAPE      # w0 < 1
    assert fwd(C.byref(_u8_desc(0, 50, 16, 64)), None) == E_SHAPE      # h0 < 1
    assert fwd(C.byref(_u8_desc(37, 50, 48, 64, f0=None)), None) == E_ARG
    assert fwd(C.byref(_u8_desc(37, 50, 48, 64, prec=_lib.PREC_F32)), None) == E_ARG  # planar: no byte path
    assert fwd(None, None) == E_ARG


@pytest.mark.parametrize("h,w", [(37, 50), (16, 16)])
def test_helpers_match_load_frame_and_to_uint8_image(tmp_path, h, w):
    rng = np.random.default_rng(h * 100 + w)
    arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    arr.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)  # every byte value meets the /255
    p = str(tmp_path / "f.png")
    Image.fromarray(arr).save(p)
    want, meta = cv.load_frame(p)
    raw, meta8 = cv.load_frame_u8(p)
    assert meta8 == meta and raw.dtype == torch.uint8 and tuple(raw.shape) == (h, w, 3)
    got = cv.frames_u8_to_float(raw)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(cv.frames_u8_to_float(raw[None])[0], want)      # batched form
    # the output mapping, on values that truncate either way
    t = torch.from_numpy(rng.random(tuple(want.shape), dtype=np.float32))
    t.view(-1)[:4] = torch.tensor([0.0, 1.0, 254.999 / 255, 0.5])
    back = cv.frames_float_to_u8(t, h, w)
    assert back.dtype == torch.uint8 and back.is_contiguous()
    np.testing.assert_array_equal(back.numpy(), cv.to_uint8_image(t, meta))
    np.testing.assert_array_equal(cv.frames_float_to_u8(t[None], h, w)[0].numpy(), cv.to_uint8_image(t, meta))
    np.testing.assert_array_equal(cv.frames_float_to_u8(want, h, w).numpy(), arr)  # k/255*255 truncates to k


class OracleU8Model:
    """The CPU oracle as the model, with interpolate_u8 made from the two helpers."""

    def __init__(self):
        from rrin_amd import Net
        from rrin_amd.synthetic import keyed_state_dict
        self.sd = keyed_state_dict(Net().state_dict(), stress=True)
        self.u8_calls = []

    def interpolate(self, i0, i1, ts):
        from oracle.ref_net import net_forward
        return [net_forward(self.sd, i0, i1, t) for t in ts]

    def interpolate_u8(self, f0, f1, ts):
        self.u8_calls.append((f0, f1))
        h0, w0 = f0.shape[1:3]
        outs = self.interpolate(cv.frames_u8_to_float(f0).contiguous(), cv.frames_u8_to_float(f1).contiguous(), ts)
        return [cv.frames_float_to_u8(o, h0, w0) for o in outs]


def test_byte_pipeline_writes_the_float_pipelines_files(tmp_path):
    src = str(tmp_path / "in")
    os.makedirs(src)
    rng = np.random.default_rng(7)
    base = rng.integers(0, 256, (37, 50, 3), dtype=np.uint8)
    for k in range(4):
        Image.fromarray(np.roll(base, 2 * k, axis=1)).save(os.path.join(src, f"{k + 1:09d}.png"))
    model = OracleU8Model()
    a, b = str(tmp_path / "u8"), str(tmp_path / "f32")
    na = cv.interpolate_folder(model, src, a, sf=2, batch=2, device=None, u8=True, log=lambda *x: None)
    assert len(model.u8_calls) == 2                                  # 3 pairs in batches of 2
    ncalls = len(model.u8_calls)
    nb = cv.interpolate_folder(model, src, b, sf=2, batch=2, device=None, u8=False, log=lambda *x: None)
    assert len(model.u8_calls) == ncalls                             # u8=False never takes the byte path
    assert na == nb == 10 and sorted(os.listdir(a)) == sorted(os.listdir(b))
    for name in os.listdir(b):
        assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name
    # every frame reaches the model once per step: f0 and f1 are two views of one [n+1] stack
    frame = 37 * 50 * 3
    for (f0, f1), n in zip(model.u8_calls, (2, 1)):
        assert f0.dtype == f1.dtype == torch.uint8 and tuple(f0.shape) == tuple(f1.shape) == (n, 37, 50, 3)
        assert f0.untyped_storage().data_ptr() == f1.untyped_storage().data_ptr()
        assert f0.untyped_storage().nbytes() == (n + 1) * frame
        assert f1.data_ptr() == f0.data_ptr() + frame
    # "auto" keeps today's path for a model on the CPU (device=None)
    c = str(tmp_path / "auto")
    cv.interpolate_folder(model, src, c, sf=2, batch=2, device=None, log=lambda *x: None)
    assert len(model.u8_calls) == ncalls


def test_u8_true_needs_interpolate_u8(tmp_path):
    class Blend:
        def interpolate(self, i0, i1, ts):
            return [(1 - t) * i0 + t * i1 for t in ts]

    src = str(tmp_path / "in")
    os.makedirs(src)
    for k in range(2):
        Image.fromarray(np.full((16, 16, 3), 10 * k, np.uint8)).save(os.path.join(src, f"{k + 1:09d}.png"))
    with pytest.raises(ValueError, match="interpolate_u8"):
        cv.interpolate_folder(Blend(), src, str(tmp_path / "out"), sf=1, u8=True, log=lambda *x: None)
