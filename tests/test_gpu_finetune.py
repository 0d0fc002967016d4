"""GPU: the fine-tuning kernels (csrc/finetune.hip) against their definitions in
rrin_amd/finetune.py -- the triplet sampler bit for bit, the fused loss within a few fp32
roundings, the autograd Function -- and the loop on the device."""
import ctypes as C
import io

import pytest
import torch

from rrin_amd import Net, _lib, autograd, metrics, yuv
from rrin_amd import finetune as ft
from tests.finetune_clip import DESCENT, clip_bytes, keyed_net

pytestmark = pytest.mark.gpu

E_SHAPE, E_ARG, E_WORKSPACE = -1, -2, -3
NAN_BITS = 0x7FC0BEEF   # the pattern around and in the outputs before a call
GUARD = 64              # floats between the outputs (keeps them 16-byte aligned)

# name -> (layout, depth, msb, H0, W0)
CASES = {
    "nv12": ("nv12", 8, False, 40, 48), "i420": ("i420", 8, False, 40, 48),
    "nv16": ("nv16", 8, False, 37, 48), "i422": ("i422", 8, False, 37, 48),
    "i444": ("i444", 8, False, 40, 48),
    "i420p10": ("i420", 10, False, 40, 48), "i420p10msb": ("i420", 10, True, 40, 48),
    "i444p12": ("i444", 12, False, 40, 48),
    "rgb8": ("rgb", 8, False, 40, 48), "rgb12": ("rgb", 12, False, 40, 48),
}
N_FRAMES = 4


def host_stack(layout, depth, msb, h, w, seed):
    """N_FRAMES frames of random samples (16-bit: a few words above maxval, which read as maxval)."""
    g = torch.Generator().manual_seed(seed)
    shape = (N_FRAMES, h, w, 3) if layout == "rgb" else (N_FRAMES, yuv.stack_rows(h, layout), w)
    if depth == 8:
        return torch.randint(0, 256, shape, generator=g, dtype=torch.int32).to(torch.uint8)
    v = torch.randint(0, (1 << depth) + (0 if msb else 37), shape, generator=g, dtype=torch.int32)
    return yuv.int_to_words(v << (16 - depth) if msb else v)


def device_slice(host, gpu):
    """The stack as a slice of a larger device buffer full of a poison value: a read outside the
    stack meets bytes the host copy does not have."""
    flat = host.reshape(-1)
    pad = 4096
    if host.dtype == torch.uint8:
        big = torch.full((flat.numel() + 2 * pad,), 0xA5, dtype=torch.uint8, device=gpu)
        big[pad:pad + flat.numel()] = flat.to(gpu)
        return big[pad:pad + flat.numel()].view(host.shape)
    big = torch.full((flat.numel() + 2 * pad,), 0x5A5A, dtype=torch.int16, device=gpu)
    big[pad:pad + flat.numel()] = flat.view(torch.int16).to(gpu)
    return big[pad:pad + flat.numel()].view(torch.uint16).view(host.shape)


class Outputs:
    """Three [K,3,ch,cw] outputs inside one buffer of NAN_BITS, GUARD floats around each."""

    def __init__(self, k, ch, cw, gpu):
        self.n = k * 3 * ch * cw
        self.shape = (k, 3, ch, cw)
        self.buf = torch.full((3 * self.n + 4 * GUARD,), NAN_BITS, dtype=torch.int32, device=gpu)
        self.offs = [GUARD + j * (self.n + GUARD) for j in range(3)]

    def ptrs(self):
        return [self.buf.data_ptr() + 4 * o for o in self.offs]

    def tensors(self):
        return [self.buf[o:o + self.n].view(torch.float32).view(self.shape) for o in self.offs]

    def guards_untouched(self):
        keep = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        for o in self.offs:
            keep[o:o + self.n] = False
        return bool((self.buf[keep] == NAN_BITS).all())

    def untouched(self):
        return bool((self.buf == NAN_BITS).all())


def crop_call(dev_frames, items, ch, cw, layout, depth, msb, outs, h, w, *, n_frames=None, planes=None, k=None,
              null=None, shift=None, depth_arg=None, base_off=0, with_coef=None):
    """rrin_triplet_crop_u8 / _u16 with the arguments a test may bend; returns the code."""
    lib = _lib.lib()
    if planes is None:
        planes = metrics.planes_of("rgb", h, w) if layout == "rgb" else metrics.planes_of("yuv", h, w, layout)
    arr = (_lib.Plane * 3)(*[_lib.Plane(off, pitch, step, ph, pw, 0) for off, step, pitch, ph, pw in planes])
    flat = (C.c_int32 * (6 * len(items)))(*[int(v) for it in items for v in it])
    use_coef = (layout != "rgb") if with_coef is None else with_coef
    kc = C.byref(_lib.YuvCoef(*yuv.as_coef(None, depth if depth in (8, 10, 12) else 10))) if use_coef else None
    args = {"frames": dev_frames.data_ptr() + base_off, "planes": arr, "items": flat}
    p = outs.ptrs()
    args.update({"i0": p[0], "it": p[1], "i1": p[2]})
    if null:
        args[null] = None
    st = C.c_void_p(torch.cuda.current_stream(dev_frames.device).cuda_stream)
    head = (args["frames"], dev_frames.stride(0), dev_frames.shape[0] if n_frames is None else n_frames, args["planes"],
            args["items"], len(items) if k is None else k, ch, cw, kc)
    if dev_frames.dtype == torch.uint8:
        return lib.rrin_triplet_crop_u8(*head, args["i0"], args["it"], args["i1"], st)
    sh = (16 - depth if msb else 0) if shift is None else shift
    return lib.rrin_triplet_crop_u16(*head, depth if depth_arg is None else depth_arg, sh, args["i0"], args["it"],
                                     args["i1"], st)


@pytest.fixture(scope="module")
def stacks(gpu):
    out = {}
    for seed, (name, (layout, depth, msb, h, w)) in enumerate(CASES.items()):
        host = host_stack(layout, depth, msb, h, w, 100 + seed)
        out[name] = (host, device_slice(host, gpu))
    return out


def item_sets(layout, h, w, ch, cw):
    """K = 5 (repeated frames, every origin and flip) and three K = 1 calls."""
    by, bx = (1, 1) if layout == "rgb" else yuv.block_of(yuv.chroma_of(layout))
    last = (h - ch, w - cw)                  # the last position that fits (on the block for every case here)
    mid = (5, 7) if (by, bx) == (1, 1) else (3 * by, 5 * bx)   # odd for one-pixel blocks
    assert last[0] % by == 0 and last[1] % bx == 0 and mid[0] <= last[0] and mid[1] <= last[1]
    five = [(0, 1, 2, 0, 0, 0), (3, 3, 0, *last, 1), (1, 1, 1, *mid, 2), (2, 0, 3, *last, 2), (0, 2, 0, *mid, 1)]
    return [five, [(1, 2, 3, *last, 0)], [(3, 2, 1, *mid, 1)], [(0, 3, 1, 0, 0, 2)]]


@pytest.mark.parametrize("name", list(CASES))
def test_sampler_is_the_definition_bit_for_bit(stacks, gpu, name):
    layout, depth, msb, h, w = CASES[name]
    host, dev = stacks[name]
    for ch, cw in ((16, 16), (16, 32), (32, 16)):
        for items in item_sets(layout, h, w, ch, cw):
            want = ft.sample_triplets(host, items, (ch, cw), layout, None, depth, msb)
            outs = Outputs(len(items), ch, cw, gpu)
            assert crop_call(dev, items, ch, cw, layout, depth, msb, outs, h, w) == 0
            got = outs.tensors()
            for j in range(3):
                assert torch.equal(got[j].cpu().view(torch.int32), want[j].view(torch.int32)), (name, ch, cw, items, j)
            assert outs.guards_untouched(), (name, ch, cw, items)
    # the public function on the device: the same kernel
    items = item_sets(layout, h, w, 16, 32)[0]
    got = ft.sample_triplets(dev, items, (16, 32), layout, None, depth, msb)
    want = ft.sample_triplets(host, items, (16, 32), layout, None, depth, msb)
    assert all(g.is_cuda and torch.equal(g.cpu(), x) for g, x in zip(got, want))


def test_sampler_refusals_leave_the_outputs_alone(stacks, gpu):
    host, dev = stacks["i420"]
    host16, dev16 = stacks["i420p10"]
    h, w = 40, 48
    ok = [(0, 1, 2, 0, 0, 0)]
    outs = Outputs(1, 16, 16, gpu)

    def call(items=ok, ch=16, cw=16, d=dev, layout="i420", depth=8, **kw):
        return crop_call(d, items, ch, cw, layout, depth, False, outs, h, w, **kw)

    def call16(**kw):
        return call(d=dev16, depth=10, **kw)

    many = [(0, 1, 2, 0, 0, 0)] * (ft.MAX_ITEMS + 1)
    luma = metrics.planes_of("yuv", h, w, "i420")[0]
    lopsided = [luma, (h * w, 1, w, h // 2, w), (h * w, 1, w, h // 2, w)]   # chroma halved in rows only: no format
    cases = [
        (E_ARG, call(null="frames")), (E_ARG, call(null="planes")), (E_ARG, call(null="items")),
        (E_ARG, call(null="i0")), (E_ARG, call(null="it")), (E_ARG, call(null="i1")),
        (E_SHAPE, call(k=0)), (E_SHAPE, call(items=many)),
        (E_SHAPE, call(ch=0)), (E_SHAPE, call(ch=8)), (E_SHAPE, call(ch=24)), (E_SHAPE, call(cw=40)),
        (E_SHAPE, call(cw=-16)),
        (E_SHAPE, call(items=[(0, 1, 2, h - 16 + 2, 0, 0)])), (E_SHAPE, call(items=[(0, 1, 2, 0, w - 16 + 2, 0)])),
        (E_SHAPE, call(items=[(0, 1, 2, -2, 0, 0)])), (E_SHAPE, call(ch=48)), (E_SHAPE, call(cw=64)),
        (E_ARG, call(items=[(0, 1, 2, 1, 0, 0)])), (E_ARG, call(items=[(0, 1, 2, 0, 1, 0)])),
        (E_ARG, call(items=[(-1, 1, 2, 0, 0, 0)])), (E_ARG, call(items=[(0, N_FRAMES, 2, 0, 0, 0)])),
        (E_ARG, call(items=[(0, 1, N_FRAMES, 0, 0, 0)])), (E_ARG, call(items=[(0, 1, 3, 0, 0, 0)], n_frames=3)),
        (E_SHAPE, call(n_frames=0)),
        (E_ARG, call(items=[(0, 1, 2, 0, 0, 3)])), (E_ARG, call(items=[(0, 1, 2, 0, 0, -1)])),
        (E_SHAPE, call(planes=lopsided)),
        (E_ARG, call16(base_off=1)),
        (E_ARG, call16(depth_arg=8)), (E_ARG, call16(depth_arg=17)), (E_ARG, call16(shift=-1)),
        (E_ARG, call16(shift=7)), (E_ARG, call16(depth_arg=11)),   # YUV conversion: depth 10 or 12 only
    ]
    torch.cuda.synchronize(gpu)
    for n, (want, got) in enumerate(cases):
        assert got == want, (n, want, got)
    assert outs.untouched()
    # and the calls next to them are taken: the last origin, RGB words at depth 11 and 16
    assert call(items=[(0, 1, 2, h - 16, w - 16, 2)]) == 0
    assert call16(items=[(3, 3, 3, 24, 32, 1)]) == 0
    _, rgb16 = stacks["rgb12"]
    for depth in (11, 16):
        assert crop_call(rgb16, ok, 16, 16, "rgb", depth, False, outs, h, w) == 0
    torch.cuda.synchronize(gpu)
    assert outs.guards_untouched()


# ---- loss --------------------------------------------------------------------------------------------
U = 2.0 ** -24
SHAPES = [(1, 3, 16, 16), (3, 3, 24, 40), (1, 3, 5, 7), (2, 3, 64, 64)]


def tloss(out, tgt, n, grad=True, short=0, w_charb=ft.W_CHARB, w_l1=ft.W_L1, eps=ft.EPS):
    """rrin_tloss on flat device tensors: (code, sums [3] float64, grad or None)."""
    lib = _lib.lib()
    count = out.numel()
    need = lib.rrin_tloss_workspace_bytes(count)
    assert need > 0 and need % 24 == 0
    ws = torch.zeros(need // 8, dtype=torch.float64, device=out.device)
    sums = torch.full((3,), -1.0, dtype=torch.float64, device=out.device)
    g = torch.full_like(out, float("nan")) if grad else None
    rc = lib.rrin_tloss(out.data_ptr(), tgt.data_ptr(), count, n, w_charb, w_l1, eps, sums.data_ptr(),
                        g.data_ptr() if grad else None, ws.data_ptr(), need - short,
                        C.c_void_p(torch.cuda.current_stream(out.device).cuda_stream))
    return rc, sums, g


def pair(shape, gpu, seed, offset=0):
    g = torch.Generator().manual_seed(seed)
    n = 1
    for s in shape:
        n *= s
    o, t = torch.rand(n + offset, generator=g), torch.rand(n + offset, generator=g)
    return o.to(gpu)[offset:], t.to(gpu)[offset:]


@pytest.mark.parametrize("shape,offset", [(s, 0) for s in SHAPES] + [((1, 3, 5, 7), 1), ((3, 3, 24, 40), 3)])
def test_loss_sums_and_gradient(gpu, shape, offset):
    """Each term is a few correctly rounded fp32 operations on d and float64 accumulation adds
    nothing visible at these sizes: 4 * 2^-24 relative on each sum and on each gradient element
    (offset: data that is not 16-byte aligned takes the kernel's scalar path)."""
    o, t = pair(shape, gpu, 11 + offset, offset)
    rc, sums, grad = tloss(o, t, shape[0])
    assert rc == 0
    rs, rg = ft.frame_loss_parts_ref(o.view(shape), t.view(shape))
    sums, rs = sums.cpu(), rs.cpu()
    rel = ((sums - rs).abs() / rs).tolist()
    print("shape", shape, "offset", offset, "sums rel err / 2^-24:", [r / U for r in rel])
    assert all(r <= 4 * U for r in rel), rel
    err = (grad.double() - rg.reshape(-1)).abs()
    bound = 4 * U * rg.reshape(-1).abs() + 2.0 ** -40
    print("grad max err / bound:", (err / bound).max().item())
    assert bool((err <= bound).all())


def test_loss_special_cases(gpu):
    shape = (3, 3, 24, 40)
    o, t = pair(shape, gpu, 5)
    count = o.numel()
    rc, sums, grad = tloss(o, o.clone(), shape[0])   # out == target
    assert rc == 0
    want = count * (1e-6 ** 0.5)
    assert abs(sums[0].item() - want) <= 4 * U * want
    assert sums[1].item() == 0.0 and sums[2].item() == 0.0
    assert bool((grad == 0).all())
    rc, sums, grad = tloss(o, t, shape[0])
    rc2, sums2, none = tloss(o, t, shape[0], grad=False)   # grad = NULL: the same sums
    rc3, sums3, grad3 = tloss(o, t, shape[0])              # and the same bits on every run
    assert (rc, rc2, rc3) == (0, 0, 0) and none is None
    assert torch.equal(sums.view(torch.int64), sums2.view(torch.int64))
    assert torch.equal(sums.view(torch.int64), sums3.view(torch.int64))
    assert torch.equal(grad.view(torch.int32), grad3.view(torch.int32))
    rc, sums, grad = tloss(o, t, shape[0], short=1)        # a workspace one byte short
    assert rc == E_WORKSPACE and bool((sums == -1.0).all()) and bool(torch.isnan(grad).all())
    lib = _lib.lib()
    assert lib.rrin_tloss_workspace_bytes(0) == E_SHAPE
    assert tloss(o, t, 0)[0] == E_SHAPE
    assert tloss(o, t, 3, eps=0.0)[0] == E_ARG and tloss(o, t, 3, eps=-1e-6)[0] == E_ARG
    st = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    ws = torch.zeros(lib.rrin_tloss_workspace_bytes(count) // 8, dtype=torch.float64, device=gpu)
    s = torch.zeros(3, dtype=torch.float64, device=gpu)
    for a in ((None, t.data_ptr(), s.data_ptr(), ws.data_ptr()), (o.data_ptr(), None, s.data_ptr(), ws.data_ptr()),
              (o.data_ptr(), t.data_ptr(), None, ws.data_ptr()), (o.data_ptr(), t.data_ptr(), s.data_ptr(), None)):
        assert lib.rrin_tloss(a[0], a[1], count, 3, 1e-3, 1e-1, 1e-6, a[2], None, a[3], ws.numel() * 8, st) == E_ARG
    assert lib.rrin_tloss(o.data_ptr(), t.data_ptr(), 0, 3, 1e-3, 1e-1, 1e-6, s.data_ptr(), None, ws.data_ptr(),
                          ws.numel() * 8, st) == E_SHAPE


def test_frame_loss_autograd(gpu):
    shape = (2, 3, 24, 40)
    o, t = pair(shape, gpu, 8)
    o, t = o.view(shape), t.view(shape)
    rc, sums, grad = tloss(o.reshape(-1), t.reshape(-1), shape[0])
    assert rc == 0
    x = o.clone().requires_grad_()
    loss, got = autograd.frame_loss(x, t, return_sums=True)
    assert loss.dim() == 0 and loss.dtype == torch.float64 and not got.requires_grad
    assert torch.equal(got, sums)
    want = ft.W_CHARB * sums[0].item() / shape[0] + ft.W_L1 * sums[1].item() / o.numel()
    assert abs(loss.item() - want) <= 1e-15 * want * 4
    (loss * 2.5).backward()
    assert torch.equal(x.grad, grad.view(shape) * 2.5)
    ref = ft.frame_loss_ref(o, t).item()
    assert abs(loss.item() - ref) <= 4 * U * ref
    with torch.no_grad():   # validation only: no gradient is kept
        assert autograd.frame_loss(o, t).item() == loss.item()


# ---- the loop on the device --------------------------------------------------------------------------
LOOP = {"steps": 3, "batch": 2, "crop": 32, "seed": 7}


@pytest.fixture(scope="module")
def gpu_runs(gpu, tmp_path_factory):
    raw = clip_bytes(64, 48, 13)
    out = []
    for k in range(2):
        path = tmp_path_factory.mktemp("ftgpu") / f"M{k}.pth"
        res = ft.finetune_y4m(keyed_net(gpu), io.BytesIO(raw), **LOOP, save=str(path), log=lambda *a: None)
        out.append((res, path))
    return raw, out


def test_gpu_loop_result_and_schedule(gpu_runs):
    res = gpu_runs[1][0][0]
    assert len(res["losses"]) == 3 and all(torch.isfinite(torch.tensor(res["losses"])))
    assert (res["frames"], res["train_frames"], res["val_frames"]) == (13, 10, 3)
    sched = ft.triplet_schedule(10, (48, 64), (2, 2), (2,), 3, 2, 32, 7)
    assert res["schedule"][0].items == sched[0].items and res["schedule"] == sched
    assert res["val_before"]["frames"] == [11]


def test_gpu_loop_is_reproducible(gpu_runs):
    a = torch.load(gpu_runs[1][0][1], map_location="cpu", weights_only=True)["model"]
    b = torch.load(gpu_runs[1][1][1], map_location="cpu", weights_only=True)["model"]
    assert len(a) == 162
    assert all(a[k].numpy().tobytes() == b[k].numpy().tobytes() for k in a)
    assert gpu_runs[1][0][0]["losses"] == gpu_runs[1][1][0]["losses"]


def test_val_after_uses_the_updated_weights(gpu_runs, gpu):
    """The packed inference weights are rebuilt after the optimiser has stepped
    (Net._weights_fingerprint): val_after is what a fresh Net loaded from the checkpoint measures."""
    raw, runs = gpu_runs
    res, path = runs[0]
    fresh = Net()
    fresh.load_state_dict(torch.load(path, map_location="cpu", weights_only=True)["model"], strict=True)
    fresh = fresh.to(gpu).eval()
    clip = ft.read_clip(io.BytesIO(raw), gpu)
    again = ft.validate(fresh, clip, res["train_frames"], 2)
    assert again["sse"] == res["val_after"]["sse"] and again["frames"] == res["val_after"]["frames"]
    assert res["val_after"]["sse"] != res["val_before"]["sse"]


def test_gpu_fixed_batch_descends(gpu):
    res = ft.finetune_y4m(keyed_net(gpu), io.BytesIO(clip_bytes(32, 32, 3)), **DESCENT, log=lambda *a: None)
    assert all(s.items == [ft.Item(0, 1, 2, 0, 0, 0)] for s in res["schedule"]) and len(res["losses"]) == 8
    print("GPU fixed-batch losses:", res["losses"])
    assert res["losses"][7] < res["losses"][0]
