"""The host half of the record convs (config-table queries, descriptor validation, the scratch-size
queries, the ring fix-up's K split, the fused level-0 block's validation) against
tests/golden/conv_h8_host.json, recorded from the library before that code was split out of
conv_h8.hip (the recording script is the fixture's header).

Nothing is launched or dereferenced: pointers are fake (tag k stands for address k << 30), and the
three launching entries only ever see descriptors the recorded library rejected before any HIP
call -- every recorded code of theirs is an RRIN_E_* (< 0; a HIP error would be > 0).
"""
import ctypes as C
import json
import os

import pytest

from rrin_amd import _lib

with open(os.path.join(os.path.dirname(__file__), "golden", "conv_h8_host.json")) as _f:
    GOLD = json.load(_f)

SWEEP_PRECS = (0, 1, 2, 3)
SWEEP_CINS = (1, 6, 8, 16, 64, 128, 256, 512)
CNT_UNSET = -7  # *cnt before a query: a rejecting query leaves it


def _ptr(tag):
    return (tag << 30) if tag else None


def view(v):
    """{"h", "w", "groups", "hi", "lo"} (+ "hp": rows per plane, "img_stride") -> rrin_h8; None: all zero."""
    if v is None:
        return _lib.H8()
    h, w = v["h"], v["w"]
    hp, wp = v.get("hp", (h + 15) // 16 * 16 + 2), (w + 31) // 32 * 32 + 16
    g = _lib.Geom(h, w, hp, wp, hp * wp)
    return _lib.H8(_ptr(v["hi"]), _ptr(v["lo"]), v.get("img_stride", v["groups"] * hp * wp), 0, v["groups"], g)


def edge_desc(s):
    d = _lib.EdgeFixDesc()
    d.n, d.cin, d.cout, d.prec, d.epi_mode = s["n"], s["cin"], s["cout"], s["prec"], s["epi"]
    d.slope = float.fromhex(s["slope"])
    d.src, d.dst = view(s["src"]), view(s["dst"])
    d.edge, d.wedge, d.bias = _ptr(s["edge"]), _ptr(s["wedge"]), _ptr(s["bias"])
    d.part, d.cnt, d.part_floats, d.cnt_len = _ptr(s["part"]), _ptr(s["cnt"]), s["part_floats"], s["cnt_len"]
    d.full = s["full"]
    return d


def conv_desc(s):
    """-> (descriptor, objects it points to)."""
    d = _lib.ConvH8Desc()
    d.n, d.cin, d.cout, d.cfg, d.prec, d.epi_mode = s["n"], s["cin"], s["cout"], s["cfg"], s["prec"], s["epi"]
    d.slope, d.inv_wscale, d.tail_finite = float.fromhex(s["slope"]), 1.0, s["tail_finite"]
    d.src, d.dst, d.pool = view(s["src"]), view(s["dst"]), view(s["pool"])
    d.whi, d.wlo, d.bias, d.edge = _ptr(s["whi"]), _ptr(s["wlo"]), _ptr(s["bias"]), _ptr(s["edge"])
    d.ksplit, d.part, d.cnt = s["ksplit"], _ptr(s["part"]), _ptr(s["cnt"])
    d.ring_w, d.ring_bias = _ptr(s["ring_w"]), _ptr(s["ring_bias"])
    d.ring_corr, d.ring_cnt = _ptr(s["ring_corr"]), _ptr(s["ring_cnt"])
    full = edge_desc(s["ring_full"]) if s["ring_full"] else None
    if full is not None:
        d.ring_full = C.addressof(full)
    return d, full


def block0_desc(s):
    d = _lib.Block0Desc()
    d.n, d.cin, d.cfg_a, d.cfg_b, d.tail_finite = s["n"], s["cin"], s["cfg_a"], s["cfg_b"], s["tail_finite"]
    d.slope, d.inv_wscale_a, d.inv_wscale_b = float.fromhex(s["slope"]), 1.0, 1.0
    d.src, d.dst, d.pool = view(s["src"]), view(s["dst"]), view(s["pool"])
    d.whi_a, d.bias_a, d.whi_b, d.bias_b = (_ptr(s[k]) for k in ("whi_a", "bias_a", "whi_b", "bias_b"))
    return d


def _query(fn, d):
    cnt = C.c_int64(CNT_UNSET)
    return [fn(C.byref(d) if d is not None else None, C.byref(cnt)), cnt.value]


def run_table(lib):
    count = lib.rrin_conv_h8_cfg_count()
    cfgs = range(-1, count + 1)
    return {"count": count,
            "bm": [lib.rrin_conv_h8_cfg_bm(c) for c in cfgs],
            "th": [lib.rrin_conv_h8_cfg_th(c) for c in cfgs],
            "wino": [lib.rrin_conv_h8_cfg_wino(c) for c in cfgs],
            "ok": [[lib.rrin_conv_h8_cfg_ok(c, p) for p in SWEEP_PRECS] for c in cfgs],
            "fits": [[[lib.rrin_conv_h8_cfg_fits(c, p, cin) for cin in SWEEP_CINS] for p in SWEEP_PRECS]
                     for c in cfgs]}


def run_conv(lib, spec):
    """Both scratch-size queries on one conv descriptor: {"split": [ret, *cnt], "ring": [ret, *cnt]}."""
    d, keep = conv_desc(spec) if spec is not None else (None, None)
    out = {"split": _query(lib.rrin_conv_h8_split_floats, d), "ring": _query(lib.rrin_conv_h8_ring_floats, d)}
    del keep
    return out


def run_edge_split(lib, spec):
    return _query(lib.rrin_edge_fix_split_floats, edge_desc(spec) if spec is not None else None)


def run_fwd(lib, entry, spec):
    """A launching entry on a descriptor it rejects before any HIP call."""
    if entry == "conv":
        d, keep = conv_desc(spec) if spec is not None else (None, None)
        rc = lib.rrin_conv3x3_h8_fwd(C.byref(d) if d is not None else None, None)
        del keep
        return rc
    if entry == "edge":
        d = edge_desc(spec) if spec is not None else None
        return lib.rrin_subpixel_edge_fix_h8(C.byref(d) if d is not None else None, None)
    d = block0_desc(spec) if spec is not None else None
    return lib.rrin_conv_block0_h8_fwd(C.byref(d) if d is not None else None, None)


def _ids(cases):
    return [c["name"] for c in cases]


def test_fixture_covers_every_entry():
    assert len(set(_ids(GOLD["conv"]))) == len(GOLD["conv"]) >= 80
    assert len(GOLD["edge_split"]) >= 36 + 8
    assert {c["entry"] for c in GOLD["fwd"]} == {"conv", "edge", "block0"}
    # accepted and rejected descriptors both: the queries are not pinned on error paths alone
    assert any(c["split"][0] > 0 for c in GOLD["conv"]) and any(c["ring"][0] > 0 for c in GOLD["conv"])
    assert {c["split"][0] for c in GOLD["conv"] if c["split"][0] < 0} == {-1, -2, -4}


def test_cfg_table_sweep():
    got = run_table(_lib.lib())
    for key in ("count", "bm", "th", "wino", "ok", "fits"):
        assert got[key] == GOLD["table"][key], key


@pytest.mark.parametrize("case", GOLD["conv"], ids=_ids(GOLD["conv"]))
def test_conv_scratch_queries(case):
    got = run_conv(_lib.lib(), case["desc"])
    assert got["split"] == case["split"]
    assert got["ring"] == case["ring"]


@pytest.mark.parametrize("case", GOLD["edge_split"], ids=_ids(GOLD["edge_split"]))
def test_edge_fix_split_floats(case):
    assert run_edge_split(_lib.lib(), case["desc"]) == case["ret"]


@pytest.mark.parametrize("case", GOLD["fwd"], ids=[c["entry"] + "-" + c["name"] for c in GOLD["fwd"]])
def test_entries_reject_before_launch(case):
    assert case["ret"] < 0  # an RRIN_E_*: the recorded library returned before its first HIP call
    assert run_fwd(_lib.lib(), case["entry"], case["desc"]) == case["ret"]
