"""CPU: the exact sequence of device work of the four Y4M stream drivers (interpolate_y4m, retime_y4m,
expose_y4m, evaluate_y4m), replayed with a recording host model against ``tests/golden/y4m_calls.json``:
every model call with its stack (shape, dtype, checksum), items and keywords, every ``check_range`` between
them, the output bytes (or the report), the return value and the log line.  The golden was recorded by
``tests/golden/gen_y4m_calls.py`` before the drivers moved to ``rrin_amd/y4mpipe.py``.  Also: what the
drivers refuse, and which streams they close."""
import hashlib
import io
import json
import os
import re
import threading
import zlib
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

from rrin_amd import convert as cv
from rrin_amd import exposure, y4m
from rrin_amd.framefmt import FrameFormat

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "y4m_calls.json")
ALL = dict(depths=(8, 10, 12), chroma=("420", "422", "444"))


def crc(t: torch.Tensor) -> int:
    return zlib.crc32(t.contiguous().view(torch.uint8).numpy().tobytes())


def ints(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.int32) & 0xFFFF if t.dtype != torch.uint16 else t.view(torch.int16).to(torch.int32) & 0xFFFF


class Recorder(torch.nn.Module):
    """Stands in for Net on the host.  An item of the pair (a, b) at t is ``(a + 2 b + round(100 t)) & maxval``;
    ``interpolate_*`` is that per pair and t, ``expose_items_*`` is ``exposure.expose`` over it.  A gated call
    leaves ``last_gate``: per item ``(sum of a + round(100 t)) % 3``.  ``log`` holds every call."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.log = []
        self.last_gate = None

    @staticmethod
    def item(a, b, t, depth):
        v = (ints(a) + 2 * ints(b) + round(100 * t)) & ((1 << depth) - 1)
        return v.to(torch.int16).view(torch.uint16).to(a.dtype)

    def record(self, name, stacks, args, kw):
        scalars = {k: v if isinstance(v, (int, float, str, bool, type(None))) else type(v).__name__
                   for k, v in sorted(kw.items())}
        self.log.append([name, [[list(s.shape), str(s.dtype), crc(s)] for s in stacks], args, scalars])

    def gate(self, kw, firsts, ts):
        self.last_gate = None
        if "scene_threshold" in kw:
            self.last_gate = torch.tensor([(int(ints(a).sum()) + round(100 * t)) % 3 for a, t in zip(firsts, ts)],
                                          dtype=torch.int32)

    def check_range(self, wait=True):
        self.log.append(["check_range", wait])

    def _pairs(self, name, f0, f1, ts, depth, kw):
        self.record(name, [f0, f1], {"ts": list(ts)}, kw)
        self.gate(kw, f0, [ts[-1]] * f0.shape[0])
        return [torch.stack([self.item(a, b, t, depth) for a, b in zip(f0, f1)]) for t in ts]

    def _items(self, name, frames, pair, t, depth, kw):
        self.record(name, [frames], {"pair": list(pair), "t": list(t)}, kw)
        self.gate(kw, [frames[p] for p in pair], t)
        return torch.stack([self.item(frames[p], frames[p + 1], v, depth) for p, v in zip(pair, t)])

    def _expose(self, name, fmt, frames, groups, kw):
        self.record(name, [frames], {"groups": [[list(s) for s in g] for g in groups]}, kw)
        net = [(p, t) for g in groups for p, t in g if t != 0]
        self.gate(kw, [frames[p] for p, _ in net], [t for _, t in net])
        return exposure.expose(frames, groups, lambda p, t: self.item(frames[p], frames[p + 1], t, fmt.depth),
                               fmt.depth, fmt.shift, light=kw.get("light"), weights=kw.get("weights"), fmt=fmt)

    def interpolate_yuv(self, f0, f1, ts, **kw):
        return self._pairs("interpolate_yuv", f0, f1, ts, 8, kw)

    def interpolate_yuv16(self, f0, f1, ts, **kw):
        return self._pairs("interpolate_yuv16", f0, f1, ts, kw["depth"], kw)

    def interpolate_items_yuv(self, frames, pair, t, **kw):
        return self._items("interpolate_items_yuv", frames, pair, t, 8, kw)

    def interpolate_items_yuv16(self, frames, pair, t, **kw):
        return self._items("interpolate_items_yuv16", frames, pair, t, kw["depth"], kw)

    def expose_items_yuv(self, frames, groups, **kw):
        return self._expose("expose_items_yuv", FrameFormat.yuv(kw["layout"], kw["coef"]), frames, groups, kw)

    def expose_items_yuv16(self, frames, groups, **kw):
        fmt = FrameFormat.yuv16(kw["layout"], kw["depth"], kw["msb"], kw["coef"])
        return self._expose("expose_items_yuv16", fmt, frames, groups, kw)


class FailsSecond(Recorder):
    """Raises in its second model call: an error in the middle of a stream."""

    def record(self, name, stacks, args, kw):
        super().record(name, stacks, args, kw)
        if len(self.log) > 1:
            raise RuntimeError("the second call fails")


def stream(n, w, h, tag, fps=24, seed=5):
    """A Y4M stream of ``n`` random frames, as bytes.  Frames 2 and 3 are equal (a duplicate pair)."""
    chroma, depth = tag[:3], int(tag[4:] or 8)
    samples = w * h * {"420": 3, "422": 4, "444": 6}[chroma] // 2
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 1 << depth, samples).astype(np.uint16 if depth > 8 else np.uint8) for _ in range(n)]
    frames[3] = frames[2].copy()
    buf = io.BytesIO()
    wr = y4m.Writer(buf, w, h, fps, 1, tag, **ALL)
    for f in frames:
        wr.write(f)
    return buf.getvalue()


# name: (driver, stream arguments, positional arguments after dst, keywords)
CASES = {
    "plain": ("interpolate_y4m", (7, 6, 4, "420"), (), dict(sf=2, batch=2)),
    "deep_gated": ("interpolate_y4m", (7, 6, 4, "422p10"), (), dict(sf=1, batch=3, scene_threshold=200.0)),
    "retime_24_60": ("retime_y4m", (6, 6, 4, "420", 24), ("60",), dict(batch=4)),
    "retime_25_30": ("retime_y4m", (8, 5, 3, "444p12", 25), (Fr(30),), dict(batch=3, scene_threshold=900.0)),
    "expose_60_24": ("expose_y4m", (13, 6, 4, "420", 60), (24, 4), dict(shutter="1/2", batch=3)),
    "expose_60_24_gated": ("expose_y4m", (13, 6, 4, "420", 60), (24, 4), dict(batch=3, scene_threshold=60.0)),
    "expose_passthrough": ("expose_y4m", (6, 6, 4, "420", 24), (48, 1), dict(batch=2)),
    "expose_linear": ("expose_y4m", (9, 6, 4, "420p10", 60), (24, 2),
                      dict(light="srgb", weights="triangle", flow_scale=2)),
    "evaluate": ("evaluate_y4m", (9, 16, 16, "420"), (), dict(hold=2, batch=3)),
    "evaluate_deep_gated": ("evaluate_y4m", (10, 16, 16, "420p10"), (), dict(hold=3, batch=2, scene_threshold=300.0)),
    "evaluate_tail": ("evaluate_y4m", (12, 16, 16, "420p10"), (), dict(hold=3, batch=2, scene_threshold=300.0)),
}


def run_case(name, src=None, dst=None):
    """One case on the current code: what the golden holds for it.  ``src`` / ``dst`` replace the in-memory
    streams (``dst``'s bytes are then the caller's to collect)."""
    fn, spec, args, kw = CASES[name]
    model, logs = Recorder(), []
    src = io.BytesIO(stream(*spec)) if src is None else src
    if fn == "evaluate_y4m":
        result = cv.evaluate_y4m(model, src, *args, log=logs.append, **kw)
        digest = hashlib.sha256(json.dumps(result, sort_keys=True).encode()).hexdigest()
        result = result["summary"]
    else:
        out = io.BytesIO() if dst is None else dst
        result = getattr(cv, fn)(model, src, out, *args, log=logs.append, **kw)
        digest = hashlib.sha256(out.getvalue()).hexdigest() if dst is None else None
    # the log line without its wall time
    logs = [re.sub(r"in \d+\.\d\d s", "in X s", m) for m in logs]
    return {"calls": model.log, "sha256": digest, "result": result, "log": logs}


def record_all():
    # through JSON, so that the golden and a replay compare as the same types
    return json.loads(json.dumps({name: run_case(name) for name in CASES}))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_has_exactly_the_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_work_is_the_recorded_sequence(golden, name):
    got = json.loads(json.dumps(run_case(name)))
    want = golden[name]
    assert len(got["calls"]) == len(want["calls"])
    for k, (a, b) in enumerate(zip(got["calls"], want["calls"])):
        assert a == b, f"call {k}"
    assert got["sha256"] == want["sha256"]
    assert got["result"] == want["result"]
    assert got["log"] == want["log"] and len(got["log"]) == 1


def test_the_cases_take_every_branch(golden):
    """The golden is only worth its cases: gaps in an exposure's stack, pass-through frames, a short last
    step, both gate codes and ignored tail frames are all in it."""
    def calls(name):
        return [c for c in golden[name]["calls"] if c[0] != "check_range"]

    assert [len(c[2]["pair"]) for c in calls("retime_24_60")] == [4, 4, 2]
    assert "3 of them input frames passed through" in golden["retime_24_60"]["log"][0]
    assert [len(c[2]["pair"]) for c in calls("retime_25_30")] == [3, 3, 1]
    assert all(c[1][0][0][0] < 13 for c in calls("expose_60_24")) and len(calls("expose_60_24")) > 1
    assert "6 of them input frames passed through" in golden["expose_passthrough"]["log"][0]
    assert all(c[3]["flow_scale"] == 2 and c[3]["light"] == "srgb" for c in calls("expose_linear"))
    assert all("flow_scale" not in c[3] and "scene_threshold" not in c[3] for c in calls("plain"))
    assert golden["evaluate_tail"]["result"]["ignored"] == 2 and golden["evaluate"]["result"]["ignored"] == 0
    assert golden["evaluate_deep_gated"]["result"]["duplicate_pairs"] + \
        golden["evaluate_deep_gated"]["result"]["cut_pairs"] > 0
    # the retire order: a step's check_range(wait=False) comes after the next step's call, the blocking one last
    for name in CASES:
        kinds = [c[0] == "check_range" for c in golden[name]["calls"]]
        n = kinds.count(False)
        assert kinds == [False] + [False, True] * (n - 1) + [True, True], name
        assert golden[name]["calls"][-1] == ["check_range", True]
        assert all(c[1] is False for c in golden[name]["calls"][:-1] if c[0] == "check_range")


def test_pipes_are_read_and_written_in_order(golden):
    """Both streams through real pipes, which cannot seek: the same calls and the same bytes."""
    data = stream(*CASES["retime_24_60"][1])
    r_src, w_src = os.pipe()
    r_dst, w_dst = os.pipe()
    got = []

    def feed():
        with os.fdopen(w_src, "wb") as f:
            f.write(data)

    def collect():
        with os.fdopen(r_dst, "rb") as f:
            got.append(f.read())

    threads = [threading.Thread(target=feed), threading.Thread(target=collect)]
    for t in threads:
        t.start()
    try:
        with os.fdopen(r_src, "rb") as src, os.fdopen(w_dst, "wb") as dst:
            assert not src.seekable() and not dst.seekable()
            res = json.loads(json.dumps(run_case("retime_24_60", src, dst)))
    finally:
        for t in threads:
            t.join()
    want = golden["retime_24_60"]
    assert res["calls"] == want["calls"] and res["result"] == want["result"]
    assert hashlib.sha256(got[0]).hexdigest() == want["sha256"]


# ---- refusals -----------------------------------------------------------------------------------
def drivers():
    """(name, call(model, src, dst, **kw)) of the four drivers with the smallest valid arguments."""
    return [("interpolate", lambda m, s, d, **kw: cv.interpolate_y4m(m, s, d, 1, log=lambda x: None, **kw)),
            ("retime", lambda m, s, d, **kw: cv.retime_y4m(m, s, d, "60", log=lambda x: None, **kw)),
            ("expose", lambda m, s, d, **kw: cv.expose_y4m(m, s, d, 24, 2, log=lambda x: None, **kw)),
            ("evaluate", lambda m, s, d, **kw: cv.evaluate_y4m(m, s, log=lambda x: None, **kw))]


@pytest.mark.parametrize("name,call", drivers())
def test_refusals(name, call, tmp_path, monkeypatch):
    data = stream(6, 16, 16, "420")
    out = tmp_path / "out.y4m"
    with pytest.raises(FileNotFoundError):
        call(Recorder(), str(tmp_path / "missing.y4m"), str(out))
    assert not out.exists()                                     # src is opened first
    one = data[:data.index(b"FRAME") + 6 + 384]
    with pytest.raises(ValueError, match="hold-out at hold=2 needs at least 3 frames" if name == "evaluate"
                       else "need at least two frames in the Y4M stream"):
        call(Recorder(), io.BytesIO(one), io.BytesIO())
    with pytest.raises(ValueError, match="batch must be an int >= 1, got 0" if name == "expose" else
                       "sf and batch must be >= 1, got 1 / 0" if name == "interpolate" else "batch must be >= 1, got 0"):
        call(Recorder(), io.BytesIO(data), io.BytesIO(), batch=0)
    monkeypatch.setenv("WORLD_SIZE", "2")
    model, dst = Recorder(), io.BytesIO()
    if name == "evaluate":                                      # reads only: not refused
        assert call(model, io.BytesIO(data), dst)["summary"]["frames"] == 6
    else:
        with pytest.raises(RuntimeError, match="runs in a single process"):
            call(model, io.BytesIO(data), dst)
        assert model.log == [] and dst.getvalue() == b""


def test_batch_rules_differ():
    """expose_y4m takes an int only; the others compare, so True counts as 1."""
    data = stream(6, 6, 4, "420", fps=60)
    with pytest.raises(ValueError, match="batch must be an int >= 1, got True"):
        cv.expose_y4m(Recorder(), io.BytesIO(data), io.BytesIO(), 24, 2, batch=True, log=lambda m: None)
    with pytest.raises(ValueError, match="batch must be an int >= 1, got 2.0"):
        cv.interpolate_y4m(Recorder(), io.BytesIO(data), io.BytesIO(), fps_out=24, samples=2, batch=2.0,
                           log=lambda m: None)
    assert cv.retime_y4m(Recorder(), io.BytesIO(data), io.BytesIO(), 120, batch=True, log=lambda m: None) == 11
    assert cv.interpolate_y4m(Recorder(), io.BytesIO(data), io.BytesIO(), 1, batch=True, log=lambda m: None) == 11


@pytest.mark.parametrize("name,call", drivers())
@pytest.mark.parametrize("fails", [False, True])
def test_only_what_was_opened_is_closed(name, call, fails, tmp_path, monkeypatch):
    data = stream(9, 16, 16, "420")
    path = tmp_path / "in.y4m"
    path.write_bytes(data)
    opened = []
    real_open = open

    def spy(*a, **kw):
        f = real_open(*a, **kw)
        opened.append(f)
        return f

    monkeypatch.setattr("builtins.open", spy)

    def run(src, dst):
        model = FailsSecond() if fails else Recorder()
        if fails:
            with pytest.raises(RuntimeError, match="the second call fails"):
                call(model, src, dst, batch=1)
        else:
            call(model, src, dst, batch=1)

    # file objects: left open
    src, dst = io.BytesIO(data), io.BytesIO()
    run(src, dst)
    assert not src.closed and not dst.closed and opened == []
    # paths: opened here, closed here
    run(str(path), str(tmp_path / "out.y4m"))
    assert len(opened) == (1 if name == "evaluate" else 2) and all(f.closed for f in opened)
    # a path in, a file object out: only the path's file is closed
    del opened[:]
    dst = io.BytesIO()
    run(path, dst)
    assert len(opened) == 1 and opened[0].closed and not dst.closed
