"""GPU: one source of Flow-reuse tags and gate-sum keys (rrin_amd.framefmt) serves every frame path, so a
wrong one would be wrong for all of them at once.  Frames of 30 x 60, one pair: they pad to 32 x 64 at
flow_scale 1 and 2, so every call of a test shares one workspace key and only the tag (or the sums' key)
keeps a call from taking the previous call's raw Flow (or sums) for its own.  Every comparison is exact.
"""
import numpy as np
import pytest
import torch

from rrin_amd import Net, yuv
from rrin_amd.synthetic import keyed_state_dict

pytestmark = pytest.mark.gpu

H0, W0 = 30, 60
BT601 = yuv.coefficients("bt601")
# (name, engine method suffix, keywords)
FORMATS = [
    ("rgb8", "u8", {}),
    ("rgb16-10", "u16", {"depth": 10}),
    ("rgb16-12", "u16", {"depth": 12}),
    ("i420", "yuv", {"layout": "i420"}),
    ("nv12", "yuv", {"layout": "nv12"}),
    ("i444", "yuv", {"layout": "i444"}),
    ("i420-bt601", "yuv", {"layout": "i420", "coef": BT601}),
    ("i420-10", "yuv16", {"layout": "i420", "depth": 10}),
    ("i420-10-msb", "yuv16", {"layout": "i420", "depth": 10, "msb": True}),
    ("i420-12", "yuv16", {"layout": "i420", "depth": 12}),
    ("i444-10", "yuv16", {"layout": "i444", "depth": 10}),
]
_NETS = {}


def net_of(dev, precision):
    if precision not in _NETS:
        if "sd" not in _NETS:
            _NETS["sd"] = keyed_state_dict(Net().state_dict(), stress=True)
        net = Net()
        net.load_state_dict(_NETS["sd"], strict=True)
        net.precision = precision
        _NETS[precision] = net.to(dev).eval()
    return _NETS[precision]


def shape_of(path, kw):
    return (1, H0, W0, 3) if path in ("u8", "u16") else (1, yuv.stack_rows(H0, kw["layout"]), W0)


def pair_of(path, kw, dev, near=False, seed=0):
    """Two random stacks of a format -- the same values for every format of one shape and sample range --
    or, ``near``, a second one that differs from the first by 1 in every sample."""
    shape = shape_of(path, kw)
    top = 1 << kw.get("depth", 8)
    rng = np.random.default_rng(1000 + seed)
    a = rng.integers(0, top, shape, dtype=np.int64)
    b = np.where(a > 0, a - 1, a + 1) if near else rng.integers(0, top, shape, dtype=np.int64)
    shift = 16 - kw["depth"] if kw.get("msb") else 0
    if top == 256:
        return tuple(torch.from_numpy(x.astype(np.uint8)).to(dev) for x in (a, b))
    return tuple(torch.from_numpy((x << shift).astype(np.uint16).view(np.int16)).view(torch.uint16).to(dev)
                 for x in (a, b))


def call(eng, path, kw, pair, t, **more):
    return getattr(eng, "forward_" + path)(pair[0], pair[1], t, streams=1, **kw, **more)


@pytest.mark.parametrize("precision", ["fp16", "fp32"])
def test_no_format_reuses_anothers_flow(gpu, precision):
    """A at t = 0.25, then B at t = 0.75 with reuse_flow=True -- B also at flow_scale 2 -- is B at 0.75 on
    a fresh engine state, for every ordered pair (A, B) of the formats, A = B included (there the reuse
    is real: same frames, same tag)."""
    eng = net_of(gpu, precision).engine()
    pairs = {name: pair_of(path, kw, gpu) for name, path, kw in FORMATS}
    with torch.no_grad():
        fresh = {}
        for name, path, kw in FORMATS:
            for s in (1, 2):
                eng._reset_caches()
                fresh[name, s] = call(eng, path, kw, pairs[name], 0.75, reuse_flow=True, flow_scale=s).clone()
        bad = []
        for na, pa, ka in FORMATS:
            for nb, pb, kb in FORMATS:
                for s in (1, 2):
                    call(eng, pa, ka, pairs[na], 0.25)
                    got = call(eng, pb, kb, pairs[nb], 0.75, reuse_flow=True, flow_scale=s)
                    if not torch.equal(got, fresh[nb, s]):
                        bad.append((na, nb, s))
        eng.check_range()
    assert not bad, f"B after A differs from B alone for (A, B, flow_scale) in {bad}"


GATE_PAIRS = [(("rgb8", "u8", {}), ("i444", "yuv", {"layout": "i444"}), 20.0),
              (("rgb16-10", "u16", {"depth": 10}), ("i444-10", "yuv16", {"layout": "i444", "depth": 10}), 80.0)]


@pytest.mark.parametrize("precision", ["fp16", "fp32"])
@pytest.mark.parametrize("case", GATE_PAIRS, ids=lambda c: c[0][0] + "+" + c[1][0])
def test_no_format_reuses_anothers_gate_sums(gpu, precision, case):
    """Two formats whose frames have the same length in elements (RGB and 4:4:4 at one depth): a gated
    call B after a gated call A, with reuse_flow=True, decides from its own sums.  One pair is two
    independent random frames (mean absolute difference about a third of the range: 85 of 255, 341 of
    1023), the other differs by 1 in every sample; ``scene_threshold`` lies between (20 and 80), so B's
    code would flip if it read A's sums."""
    fa, fb, threshold = case
    eng = net_of(gpu, precision).engine()
    with torch.no_grad():
        for (na, pa, ka), (nb, pb, kb) in ((fa, fb), (fb, fa)):
            for a_near in (False, True):
                pair_a, pair_b = pair_of(pa, ka, gpu, near=a_near), pair_of(pb, kb, gpu, near=not a_near, seed=1)
                eng._reset_caches()
                call(eng, pb, kb, pair_b, 0.75, reuse_flow=True, scene_threshold=threshold)
                alone = eng.last_gate.clone()
                assert alone.tolist() == [2 if a_near else 0]   # B is the cut (t >= 0.5: the second frame) or not
                eng._reset_caches()
                call(eng, pa, ka, pair_a, 0.25, scene_threshold=threshold)
                assert eng.last_gate.tolist() == [0 if a_near else 1]
                call(eng, pb, kb, pair_b, 0.75, reuse_flow=True, scene_threshold=threshold)
                assert torch.equal(eng.last_gate, alone), (na, nb, a_near)
        eng.check_range()
