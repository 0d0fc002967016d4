"""CPU: the engine's host-only weight packing and per-conv schedule (engine.unit_convs, h8_records,
geom_splits, h8_cfgs, pack_h8_host, h8_splits, pack_planar_host) against tests/golden/engine_schedule.json,
recorded on the device from ``RRINEngine._pack_h8`` as it was before the packing was split from the
upload: every tile config, split-K count, sub-pixel mode, fused-block mark and weight scale of every
size class at 640x368 (the geometry rule splits K) and 1280x720 (it does not), and the SHA-256 of
the packed weight and bias bytes.  No device is touched."""
import hashlib
import json
import os

import pytest

from rrin_amd import Net, _lib
from rrin_amd import engine as E
from rrin_amd.synthetic import keyed_state_dict

with open(os.path.join(os.path.dirname(__file__), "golden", "engine_schedule.json")) as _f:
    FIX = json.load(_f)


def sha(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


@pytest.fixture(scope="module")
def convs():
    """The raw convs of a CPU Net with the stress weights (the heads are not packed)."""
    net = Net()
    net.load_state_dict(keyed_state_dict(net.state_dict(), stress=True), strict=True)
    body, heads = E.unit_convs(E.net_units(net))
    assert len(heads) == 4 and len(body) == 77
    return body


@pytest.fixture(scope="module")
def records(convs):
    return E.h8_records(convs, Net().subpixel_max_level)


def host_case(records, precision, size, h, w):
    """What the recording script read from the device table and blobs, from the host functions."""
    prec = _lib.PRECISIONS[precision]
    geo = E.geom_splits(records, prec, h, w)
    cfgs = E.h8_cfgs(records, prec, size, geo)
    weights, biases, meta = E.pack_h8_host(records, cfgs, prec)
    splits = E.h8_splits(records, cfgs, geo, prec)
    assert [m.cfg for m in meta] == list(cfgs)
    assert [m.edge for m in meta] == [r[6] is not None for r in records]
    return {"size": size, "h": h, "w": w,
            "convs": [{"cfg": int(m.cfg), "ksplit": int(k), "subpixel": int(s), "fuse_next": int(m.fuse_next),
                       "inv_wscale": float(m.inv_wscale).hex()} for m, (k, s) in zip(meta, splits)],
            "weights_sha256": sha(weights), "bias_sha256": sha(biases)}


def test_fixture_header():
    assert len(FIX["recorded_from"]) == 40 and FIX["weights"] == "keyed_state_dict(stress=True)"
    assert sorted(FIX["precisions"]) == ["fp16", "fp32", "fp32_split16"]
    for cases in FIX["precisions"].values():
        assert [(c["size"], c["h"], c["w"]) for c in cases] == [
            (s, h, w) for s in ("small", "medium", "large", "xlarge", "xxlarge") for h, w in ((368, 640), (720, 1280))]
    # the geometry rule splits K at 640x368 and not at 1280x720 (exact fp32 only)
    for c in FIX["precisions"]["fp32"]:
        assert any(v["ksplit"] > 1 for v in c["convs"]) == (c["h"] == 368), (c["size"], c["h"])


@pytest.mark.parametrize("precision", ["fp32", "fp32_split16", "fp16"])
def test_h8_packing_equals_the_recorded_schedule(records, precision):
    for want in FIX["precisions"][precision]:
        got = host_case(records, precision, want["size"], want["h"], want["w"])
        for i, (g, v) in enumerate(zip(got["convs"], want["convs"])):
            assert g == v, (precision, want["size"], want["h"], i)
        assert got == want, (precision, want["size"], want["h"])


def test_planar_packing_equals_the_recorded_blob(convs):
    blob, meta = E.pack_planar_host(convs)
    assert [int(m[2]) for m in meta] == FIX["fp32_planar"]["cfgs"]
    assert sha(blob) == FIX["fp32_planar"]["blob_sha256"]


@pytest.mark.parametrize("k", range(2), ids=["FUSE_L0", "WINO42_LEVELS"])
def test_knobs_reach_the_packing(records, k, monkeypatch):
    """engine.FUSE_L0 = 0 and engine.WINO42_LEVELS = (), assigned as bench.py and the A/B tests do,
    change the schedule in the recorded way (and it differs from the default's)."""
    knob = FIX["knobs"][k]
    want = knob["case"]
    assert knob["knob"] == ("FUSE_L0", "WINO42_LEVELS")[k]
    default = next(c for c in FIX["precisions"][knob["precision"]]
                   if (c["size"], c["h"], c["w"]) == (want["size"], want["h"], want["w"]))
    assert default["convs"] != want["convs"]
    assert host_case(records, knob["precision"], want["size"], want["h"], want["w"]) == default
    value = knob["value"]
    monkeypatch.setattr(E, knob["knob"], tuple(value) if isinstance(value, list) else value)
    assert host_case(records, knob["precision"], want["size"], want["h"], want["w"]) == want
    monkeypatch.undo()
    assert host_case(records, knob["precision"], want["size"], want["h"], want["w"]) == default
