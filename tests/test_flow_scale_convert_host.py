"""Host: the convert functions hand ``flow_scale`` to the model's call and otherwise behave as at
scale 1 -- with and without the scene gate, whose "is it on" must not depend on the scale.  The
stand-in models are those of the Y4M, retime and evaluate host tests; the gated ones add the
``last_gate`` a Net keeps after a gated call.  No GPU."""
import io
import json
import os
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch
from PIL import Image

from rrin_amd import convert as cv
from rrin_amd import retime, y4m
from tests.test_retime_host import HostItems, y4m_bytes
from tests.test_yuv4xx_host import HostModel

ALL = dict(depths=(8, 10, 12), chroma=("420", "422", "444"))
W, H = 6, 4


class GatedModel(HostModel):
    """HostModel with the codes of a gated call: nothing gated."""
    last_gate = None

    def _run(self, name, f0, f1, ts, layout, **kw):
        self.last_gate = torch.zeros(f0.shape[0], dtype=torch.int32) if "scene_threshold" in kw else None
        return super()._run(name, f0, f1, ts, layout, **kw)


class GatedItems(HostItems):
    last_gate = None

    def _items(self, name, frames, pair, t, layout, **kw):
        self.last_gate = torch.zeros(len(pair), dtype=torch.int32) if "scene_threshold" in kw else None
        return super()._items(name, frames, pair, t, layout, **kw)


def clip(n, depth=8, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 100, W * H * 3 // 2).astype(np.uint16 if depth > 8 else np.uint8) for _ in range(n)]


def scale_of(call):
    return call[-1].get("flow_scale")


@pytest.mark.parametrize("threshold", [None, 30.0])
@pytest.mark.parametrize("tag,depth", [("420", 8), ("420p10", 10)])
def test_interpolate_y4m_passes_the_scale(tag, depth, threshold):
    frames = clip(4, depth)
    outs, calls, logs = {}, {}, {}
    for s in (1, 2):
        model, dst, logs[s] = GatedModel(), io.BytesIO(), []
        n = cv.interpolate_y4m(model, y4m_bytes(frames, W, H, tag), dst, 2, batch=2, scene_threshold=threshold,
                               log=logs[s].append, flow_scale=s)
        assert n == 10
        outs[s], calls[s] = dst.getvalue(), model.calls
    assert outs[1] == outs[2]                                    # the stand-in ignores the scale
    assert [scale_of(c) for c in calls[2]] == [2, 2]
    assert all("flow_scale" not in c[-1] for c in calls[1])      # scale 1 passes no keyword
    assert all(("scene_threshold" in c[-1]) == (threshold is not None) for c in calls[1] + calls[2])
    assert len(logs[2]) == 1 and ("scene gate" in logs[2][0]) == (threshold is not None)
    assert ("scene gate" in logs[1][0]) == (threshold is not None)


@pytest.mark.parametrize("threshold", [None, 30.0])
@pytest.mark.parametrize("tag,depth", [("420", 8), ("420p10", 10)])
def test_retime_y4m_passes_the_scale(tag, depth, threshold):
    frames = clip(6, depth)
    sched = retime.schedule(6, Fr(24), retime.as_rate("60"))
    outs = {}
    for s in (1, 2):
        model, dst, logs = GatedItems(), io.BytesIO(), []
        n = cv.interpolate_y4m(model, y4m_bytes(frames, W, H, tag), dst, fps_out="60", batch=3,
                               scene_threshold=threshold, log=logs.append, flow_scale=s)
        assert n == len(sched) and len(model.calls) >= 2
        assert [scale_of(c) for c in model.calls] == [None if s == 1 else 2] * len(model.calls)
        assert all(("scene_threshold" in c[-1]) == (threshold is not None) for c in model.calls)
        assert len(logs) == 1 and ("scene gate" in logs[0]) == (threshold is not None)
        outs[s] = dst.getvalue()
    assert outs[1] == outs[2]
    assert len(list(y4m.Reader(io.BytesIO(outs[2]), **ALL))) == len(sched)


@pytest.mark.parametrize("threshold", [None, 30.0])
def test_evaluate_y4m_passes_and_records_the_scale(threshold):
    w, h = 48, 32
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 150, w * h * 3 // 2).astype(np.uint8) for _ in range(5)]
    frames[4] = frames[3].copy()
    res = {}
    for s in (1, 2):
        model, logs, rep = GatedItems(), [], io.StringIO()
        res[s] = cv.evaluate_y4m(model, y4m_bytes(frames, w, h, "420"), hold=2, batch=4, scene_threshold=threshold,
                                 log=logs.append, report=rep, flow_scale=s)
        assert res[s]["summary"]["flow_scale"] == s
        assert json.loads(rep.getvalue()) == res[s] and len(logs) == 1
        assert [scale_of(c) for c in model.calls] == [None if s == 1 else 2] * len(model.calls)
        assert all(("scene_threshold" in c[-1]) == (threshold is not None) for c in model.calls)
    assert res[1]["rows"] == res[2]["rows"]
    a, b = dict(res[1]["summary"]), dict(res[2]["summary"])
    for d in (a, b):
        d.pop("flow_scale")
        d.pop("seconds", None)
    assert {k: v for k, v in a.items() if not isinstance(v, float)} == \
        {k: v for k, v in b.items() if not isinstance(v, float)}
    # without a gate nothing is reported as gated, whatever the scale (frames 3 and 4 are equal)
    if threshold is None:
        assert res[2]["summary"]["duplicate_pairs"] == 0 and res[2]["summary"]["cut_pairs"] == 0
        assert all(r["gate"] == 0 for r in res[2]["rows"])


class FolderModel:
    """interpolate_u8 of a byte-pipeline model: frame k of a pair is f0 + k + 1; records the keywords."""

    def __init__(self):
        self.calls, self.last_gate = [], None

    def interpolate_u8(self, f0, f1, ts, **kw):
        self.calls.append(kw)
        self.last_gate = torch.zeros(f0.shape[0], dtype=torch.int32) if "scene_threshold" in kw else None
        return [f0 + (k + 1) for k in range(len(ts))]


@pytest.mark.parametrize("threshold", [None, 30.0])
def test_interpolate_folder_passes_the_scale(tmp_path, threshold):
    src = str(tmp_path / "in")
    os.makedirs(src)
    rng = np.random.default_rng(7)
    for k in range(3):
        Image.fromarray(rng.integers(0, 200, (9, 11, 3), dtype=np.uint8)).save(os.path.join(src, f"{k + 1:09d}.png"))
    written = {}
    for s in (1, 2):
        model, logs, dest = FolderModel(), [], str(tmp_path / f"out{s}_{threshold}")
        n = cv.interpolate_folder(model, src, dest, sf=1, batch=2, device=None, u8=True, scene_threshold=threshold,
                                  log=logs.append, flow_scale=s)
        assert n == 5 and len(model.calls) == 1
        assert model.calls[0].get("flow_scale") == (None if s == 1 else 2)
        assert ("scene_threshold" in model.calls[0]) == (threshold is not None)
        assert any("scene gate" in m for m in logs) == (threshold is not None)
        written[s] = {f: open(os.path.join(dest, f), "rb").read() for f in sorted(os.listdir(dest))}
    assert written[1] == written[2] and len(written[2]) == 5
