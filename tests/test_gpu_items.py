"""GPU: item forwards (Net.interpolate_items_*, rrin_net_*_items_fwd, ABI 25) -- a batch of
(pair index, t) items over one frame stack, the Flow U-Net once per distinct pair, the other three
U-Nets once per item.  By definition item k is forward_*(frames[pair[k]:pair[k]+1],
frames[pair[k]+1:pair[k]+2], t=t[k])[0]; every comparison here is exact equality.

Shapes: 40x24 (not a multiple of 16, W0 != H0: padding and crop live) and 48x32 (even, for 4:2:0);
P = 3 pairs (4 frames); M = 5 items over pairs [0, 0, 1, 2, 2] with five different t, one < 0.5 and
one >= 0.5 on the same pair."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

from rrin_amd import Net, _lib, retime, y4m
from rrin_amd import convert as cv
from rrin_amd.engine import t_coefficients
from rrin_amd.pp import H8Tensor
from rrin_amd.synthetic import keyed_state_dict
from tests import glue_ref as G
from tests import hip_helpers as H
from tests.test_gpu_glue import PREC, Rig, assert_only_moved, assert_same_bits, bits, snapshot
from tests.test_gpu_net_contract import expected_conv_flops, prof_read

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "fp32_split16", "fp16"]
PAIR = [0, 0, 1, 2, 2]
T = [0.4, 0.8, 0.2, 0.5, 0.9375]
P = 3
_SD = {}
_NETS = {}


def net_of(dev, precision):
    """One Net per precision for the whole module (an engine is rebuilt when the precision changes)."""
    if precision not in _NETS:
        if "sd" not in _SD:
            _SD["sd"] = keyed_state_dict(Net().state_dict(), stress=True)
        net = Net()
        net.load_state_dict(_SD["sd"], strict=True)
        net.precision = precision
        _NETS[precision] = net.to(dev).eval()
    return _NETS[precision]


def stack_of(shape, seed, dev, dtype=torch.uint8, maxval=255, shift=0):
    """A frame stack of random samples in [0, maxval] (<< shift), smoothed a little along the last
    axis so that neighbouring frames differ everywhere without being noise to the network."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, maxval + 1, shape).astype(np.int64)
    a = ((a + np.roll(a, 1, -1) + np.roll(a, 2, -1)) // 3) << shift
    t = torch.from_numpy(a.astype(np.uint16 if dtype == torch.uint16 else np.uint8))
    return t if dev is None else t.to(dev)


def by_definition(fwd, frames, pair, t, **kw):
    """The per-item calls of the definition: each pair alone, at the item's own t."""
    return torch.cat([fwd(frames[p:p + 1], frames[p + 1:p + 2], t=t[k], **kw) for k, p in enumerate(pair)])


# ---- the definition, per path -----------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_items_u8_is_the_definition(gpu, precision):
    net = net_of(gpu, precision)
    frames = stack_of((P + 1, 24, 40, 3), 1, gpu)
    with torch.no_grad():
        want = by_definition(net.forward_u8, frames, PAIR, T)
        got = net.interpolate_items_u8(frames, PAIR, T)
        assert got.shape == (5, 24, 40, 3) and got.dtype == torch.uint8
        assert torch.equal(got, want)
        assert not torch.equal(got[0], got[1]) and not torch.equal(got[3], got[4])   # t is live
        # tensors for pair and t: the definition with fp32 tensor t
        tt = torch.tensor(T, dtype=torch.float32, device=gpu)
        want_t = by_definition(net.forward_u8, frames, PAIR, tt)
        got_t = net.interpolate_items_u8(frames, torch.tensor(PAIR, dtype=torch.int32, device=gpu), tt)
        assert torch.equal(got_t, want_t)
        # M = 1, and an item on the last pair only (its frames are a view into the stack)
        assert torch.equal(net.interpolate_items_u8(frames, [2], [0.3]), net.forward_u8(frames[2:3], frames[3:4], t=0.3))
        # M = P over every pair once: the plain batched forward with a t tensor
        t3 = torch.tensor([0.25, 0.5, 0.75], dtype=torch.float32)
        assert torch.equal(net.interpolate_items_u8(frames, [0, 1, 2], t3),
                           net.forward_u8(frames[:-1], frames[1:], t=t3))
        # pairs that skip one (gathered frames), one stream or two
        for streams in (1, 2):
            net.streams = streams
            try:
                assert torch.equal(net.interpolate_items_u8(frames, [0, 0, 2], [0.1, 0.6, 0.7]),
                                   by_definition(net.forward_u8, frames, [0, 0, 2], [0.1, 0.6, 0.7]))
                assert torch.equal(net.interpolate_items_u8(frames, PAIR, T), want)
            finally:
                net.streams = None
    net.check_range()


@pytest.mark.parametrize("layout,shape", [("nv12", (32, 48)), ("i422", (24, 40))])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_items_yuv_is_the_definition(gpu, precision, layout, shape):
    from rrin_amd import yuv
    net = net_of(gpu, precision)
    h0, w0 = shape
    frames = stack_of((P + 1, yuv.stack_rows(h0, layout), w0), 2, gpu)
    coef = yuv.coefficients("bt601", True)
    with torch.no_grad():
        for kw in ({"layout": layout}, {"layout": layout, "coef": coef}):
            got = net.interpolate_items_yuv(frames, PAIR, T, **kw)
            assert got.shape == (5,) + tuple(frames.shape[1:])
            assert torch.equal(got, by_definition(net.forward_yuv, frames, PAIR, T, **kw))
    net.check_range()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_items_u16_is_the_definition(gpu, precision):
    net = net_of(gpu, precision)
    frames = stack_of((P + 1, 24, 40, 3), 3, gpu, torch.uint16, 4095)
    with torch.no_grad():
        got = net.interpolate_items_u16(frames, PAIR, T, depth=12)
        assert got.dtype == torch.uint16
        assert torch.equal(got, by_definition(net.forward_u16, frames, PAIR, T, depth=12))
    net.check_range()


@pytest.mark.parametrize("msb", [False, True])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_items_yuv16_is_the_definition(gpu, precision, msb):
    net = net_of(gpu, precision)
    frames = stack_of((P + 1, 48, 48), 4, gpu, torch.uint16, 1023, 6 if msb else 0)
    kw = dict(layout="i420", depth=10, msb=msb)
    with torch.no_grad():
        got = net.interpolate_items_yuv16(frames, PAIR, T, **kw)
        assert torch.equal(got, by_definition(net.forward_yuv16, frames, PAIR, T, **kw))
    net.check_range()


# ---- the launch structure ------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_flow_runs_once_per_pair(gpu, precision):
    """The launches of one interpolate_items_u8 call, from the engine's launch profiler: every conv
    and the head of the Flow U-Net carry batch P = 3, those of the other three U-Nets M = 5.  A
    loop over the existing calls cannot give this list."""
    lib = _lib.lib()
    net = net_of(gpu, precision)
    eng = net.engine()
    frames = stack_of((P + 1, 24, 40, 3), 1, gpu)
    m, h, w = len(PAIR), 32, 48
    prof = C.c_void_p()
    _lib.check(lib.rrin_prof_create(4096, C.byref(prof)), "rrin_prof_create")
    try:
        with torch.no_grad():
            plain = eng.interpolate_items_u8(frames, PAIR, T, streams=1)
            got = eng.interpolate_items_u8(frames, PAIR, T, streams=1, prof=prof)
        torch.cuda.synchronize(gpu)
        assert torch.equal(got, plain)
        launches = prof_read(prof)
    finally:
        lib.rrin_prof_destroy(prof)
    per_item, fused = expected_conv_flops(eng, 1, h, w)
    table_m, _ = expected_conv_flops(eng, m, h, w)
    assert [f * m for f in per_item] == table_m   # one tile-table class at this size: FLOPs are per image
    unet, i, heads = 0, 0, []
    for kind, flops in launches:
        if kind == _lib.KIND_CONV:
            batch = P if unet == 0 else m
            assert flops == per_item[i] * batch, f"{precision}: conv launch {i} (U-Net {unet}) is not batch {batch}"
            i += 1
        elif kind == _lib.KIND_HEAD:
            heads.append(flops)
            unet += 1
    assert i == len(per_item) == 77 - fused and unet == 4
    assert heads == [2.0 * 9 * 32 * co * h * w * n for co, n in ((4, P), (4, m), (2, m), (3, m))]
    assert launches[0][0] == _lib.KIND_LAYOUT and launches[-1][0] == _lib.KIND_HEAD


# ---- dirty state -----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_no_stale_flow_after_other_calls(gpu, precision):
    """One process, one engine: an items call, a plain forward_u8 of the same part shape on other
    frames (it overwrites the kept raw Flow of the shared workspace), the items call again -- and
    a forward_u8(reuse_flow=True) after an items call must not take the items' Flow for its own."""
    net = net_of(gpu, precision)
    eng = net.engine()
    frames = stack_of((P + 1, 24, 40, 3), 1, gpu)
    other = stack_of((6, 24, 40, 3), 9, gpu)
    with torch.no_grad():
        want = by_definition(net.forward_u8, frames, PAIR, T)
        first = eng.interpolate_items_u8(frames, PAIR, T, streams=1)
        mid = eng.forward_u8(other[:-1], other[1:], 0.3, streams=1)       # 5 pairs: the items' workspace
        again = eng.interpolate_items_u8(frames, PAIR, T, streams=1)
        assert torch.equal(first, want) and torch.equal(again, want)
        reused = eng.forward_u8(other[:-1], other[1:], 0.3, reuse_flow=True, streams=1)
        assert torch.equal(reused, mid)
    net.check_range()


# ---- the scene gate ----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_gate_per_item(gpu, precision):
    """Pair 0 a duplicate, pair 1 ordinary, pair 2 unrelated noise, and a threshold between the last
    two: the duplicate's items are the first frame, the cut's the nearer frame by their own t."""
    net = net_of(gpu, precision)
    a = stack_of((1, 24, 40, 3), 5, gpu)
    b = (a.to(torch.int16) + 3).clamp(0, 255).to(torch.uint8)
    noise = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (1, 24, 40, 3), dtype=np.uint8)).to(gpu)
    frames = torch.cat([a, a, b, noise])
    sad = net.pair_stats_u8(frames[:-1], frames[1:]).tolist()
    assert sad[0] == 0 < sad[1] < sad[2]
    th = (sad[1] + sad[2]) / 2 / (24 * 40 * 3)
    f0 = frames[PAIR]
    f1 = frames[[p + 1 for p in PAIR]]
    pair_code = [1, 0, 2]
    codes = torch.tensor([0 if pair_code[p] == 0 else 1 if pair_code[p] == 1 else cv.scene_cut_code(T[k])
                          for k, p in enumerate(PAIR)], dtype=torch.int32)
    assert codes.tolist() == [1, 1, 0, 2, 2]
    with torch.no_grad():
        plain = net.interpolate_items_u8(frames, PAIR, T)
        want = cv.apply_gate_u8(plain, f0, f1, codes)
        got = net.interpolate_items_u8(frames, PAIR, T, scene_threshold=th)
        assert net.last_gate.shape == (5,) and net.last_gate.cpu().tolist() == codes.tolist()
        assert torch.equal(got, want)
        # a cut item below 0.5 takes the first frame
        t2 = [0.4, 0.8, 0.2, 0.25, 0.75]
        got = net.interpolate_items_u8(frames, PAIR, t2, scene_threshold=th)
        assert net.last_gate.cpu().tolist() == [1, 1, 0, 1, 2]
        assert torch.equal(got[3], frames[2]) and torch.equal(got[4], frames[3])
        # explicit codes per pair are honoured the same way
        gate = torch.tensor([0, 2, 1], dtype=torch.int32, device=gpu)
        got = net.interpolate_items_u8(frames, PAIR, T, gate=gate)
        assert net.last_gate.cpu().tolist() == [0, 0, 1, 1, 1]
        want = cv.apply_gate_u8(plain, f0, f1, torch.tensor([0, 0, 1, 1, 1], dtype=torch.int32))
        assert torch.equal(got, want)
        with pytest.raises(ValueError):
            net.interpolate_items_u8(frames, PAIR, T, gate=gate, scene_threshold=th)
        with pytest.raises(ValueError):
            net.interpolate_items_u8(frames, PAIR, T, gate=gate[:2])


def test_gate_per_item_yuv16(gpu):
    """The 16-bit gate copies whole words and sums samples: a duplicate and a cut on 10-bit 4:2:0."""
    net = net_of(gpu, "fp32")
    a = stack_of((1, 48, 48), 7, gpu, torch.uint16, 1023)
    noise = torch.from_numpy(np.random.default_rng(8).integers(0, 1024, (1, 48, 48)).astype(np.uint16)).to(gpu)
    frames = torch.cat([a, a, noise])
    kw = dict(layout="i420", depth=10)
    with torch.no_grad():
        got = net.interpolate_items_yuv16(frames, [0, 1, 1], [0.5, 0.25, 0.5], scene_threshold=20.0, **kw)
    assert net.last_gate.cpu().tolist() == [1, 1, 2]
    assert torch.equal(got[0], frames[0]) and torch.equal(got[1], frames[1]) and torch.equal(got[2], frames[2])


# ---- the indexed t-blend entry -------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["R32", "F16"])
def test_tblend_items_h8(gpu, prec):
    """rrin_flow_tblend_items_h8 of 3 kept raw flows for 5 items into a pattern-filled g16: channels
    6-9 are bit for bit the unindexed entry's on the gathered raw flows, fp32 records also exactly
    glue_ref's fp32 t-blend of them; nothing else moves, and a map outside [0, n_pairs) is clamped."""
    lib = _lib.lib()
    h, w = 24, 40
    m = len(PAIR)
    src = Rig(gpu, prec, P, h, w, t=[0.3, 0.3, 0.3])
    fr = H8Tensor(P, 4, h, w, gpu, src.prec)
    src.head("flow", src.g16(), 300.0, flow_raw=fr)
    coef = t_coefficients(torch.tensor(T), m)
    coef_d = coef.to(gpu)

    def g16(seed):
        g = H8Tensor(m, G.G16_CHANNELS, h, w, gpu, src.prec)
        for k, a in enumerate([g.hi] + ([g.lo] if g.lo is not None else [])):
            a.copy_(G.pattern(a.shape, seed + k, a.dtype))
        return g

    for pairs, clamped in ((PAIR, PAIR), ([-7, 0, 1, 2, 99], [0, 0, 1, 2, 2])):
        maps = torch.tensor(pairs, dtype=torch.int32, device=gpu)
        gb = g16(5)
        snap = snapshot(gb)
        frv, gv = fr.view(0, 4), gb.view(0, gb.c)
        assert lib.rrin_flow_tblend_items_h8(C.byref(frv), C.byref(gv), coef_d.data_ptr(), m, maps.data_ptr(), P,
                                             src.prec, H.stream(gpu)) == 0
        torch.cuda.synchronize()
        assert_only_moved(gb, snap, range(6, 10), "indexed t-blend g16")
        assert not torch.equal(bits(gb.hi), bits(snap[0]))
        # the unindexed entry on the gathered raw flows
        gathered = H8Tensor(m, 4, h, w, gpu, src.prec)
        gathered.hi.copy_(fr.hi[clamped])
        gc = g16(5)
        gfv, gcv = gathered.view(0, 4), gc.view(0, gc.c)
        assert lib.rrin_flow_tblend_h8(C.byref(gfv), C.byref(gcv), coef_d.data_ptr(), m, src.prec, H.stream(gpu)) == 0
        torch.cuda.synchronize()
        assert_same_bits(gb, gc, "indexed t-blend vs unindexed on gathered flows")
        raw = fr.to_nchw(0, 4).cpu()[clamped]
        ft = torch.cat(G.flow_blend32(coef, raw), 1)
        assert torch.equal(gb.to_nchw(6, 4).cpu(), G.store_round(ft, prec))
    assert PREC[prec] == src.prec


# ---- the pipe ------------------------------------------------------------------------------------------
def test_interpolate_y4m_fps_out(gpu):
    """24 -> 60 on a 4-frame C420 stream of 48x32: the pass-through bytes and the interpolate_items_yuv
    results laid out by retime.schedule; the header says F60:1."""
    net = net_of(gpu, "fp32")
    w0, h0 = 48, 32
    frames = stack_of((4, 3 * h0 // 2, w0), 11, None)
    src = io.BytesIO()
    wr = y4m.Writer(src, w0, h0, 24, 1)
    for f in frames:
        wr.write(f.numpy())
    src.seek(0)
    dst = io.BytesIO()
    logs = []
    sched = retime.schedule(4, 24, 60)
    assert cv.interpolate_y4m(net, src, dst, fps_out="60", batch=4, log=logs.append) == len(sched) == 8
    raw = dst.getvalue()
    assert raw.startswith(b"YUV4MPEG2 W48 H32 F60:1 ")
    out = list(y4m.Reader(io.BytesIO(raw)))
    assert len(out) == 8
    items = [(p, float(t)) for p, t in sched if t != 0]
    with torch.no_grad():
        want = net.interpolate_items_yuv(frames.to(gpu), [p for p, _ in items], [t for _, t in items],
                                         layout="i420").cpu()
    k = 0
    for o, (p, t) in zip(out, sched):
        if t == 0:
            assert np.array_equal(o, frames[p].numpy().reshape(-1))
        else:
            assert np.array_equal(o, want[k].numpy().reshape(-1))
            k += 1
    # times 0, .4, ..., 2.8: frames 0 and 2 pass through, six items in steps of 4 and 2
    assert k == 6 and "2 of them input frames passed through" in logs[0] and "60:1 fps" in logs[0]
