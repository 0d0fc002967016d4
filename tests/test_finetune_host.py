"""CPU: the fine-tuning path's host code and definitions (rrin_amd/finetune.py) -- the triplet
schedule, the sampler's definition, the loss against the reference's expressions, the command
line, and the whole loop on a tiny clip with PyTorch operators."""
import io
from fractions import Fraction

import pytest
import torch

from rrin_amd import Net, convert, yuv
from rrin_amd import finetune as ft
from rrin_amd.__main__ import build_parser, main
from tests.finetune_clip import DESCENT, clip_bytes, keyed_net

GOLDEN_KEYS = "tests/golden/state_dict_keys.txt"


# ---- schedule ------------------------------------------------------------------------------------
def _schedule(**kw):
    args = dict(n_frames=20, size=(48, 64), block=(2, 2), spans=(2,), steps=40, batch=3, crop=(16, 32), seed=5)
    args.update(kw)
    return ft.triplet_schedule(**args)


def test_schedule_is_a_function_of_its_seed():
    assert _schedule() == _schedule()
    assert _schedule() != _schedule(seed=6)


@pytest.mark.parametrize("block,size", [((2, 2), (48, 64)), ((1, 2), (37, 48)), ((1, 1), (33, 47))])
def test_schedule_items_in_bounds_on_block_in_range(block, size):
    steps = _schedule(block=block, size=size, spans=(2, 3), n_frames=9, steps=100)
    assert len(steps) == 100 and all(len(s.items) == 3 for s in steps)
    seen_flip, seen_y, seen_x = set(), set(), set()
    for s in steps:
        for it in s.items:
            assert all(0 <= f < 9 for f in it[:3])
            assert 0 <= it.y0 <= size[0] - 16 and 0 <= it.x0 <= size[1] - 32
            assert it.y0 % block[0] == 0 and it.x0 % block[1] == 0
            lo, hi = min(it.frame0, it.frame1), max(it.frame0, it.frame1)
            assert hi - lo == s.span and lo < it.frame_t < hi
            seen_flip.add(it.flip), seen_y.add(it.y0), seen_x.add(it.x0)
    assert seen_flip == {0, 1, 2}
    assert max(seen_y) == (size[0] - 16) // block[0] * block[0] and min(seen_y) == 0
    assert max(seen_x) == (size[1] - 32) // block[1] * block[1] and min(seen_x) == 0


def test_schedule_avoids_cut_pairs():
    cuts = (3, 4, 11)
    for s in _schedule(spans=(2, 3), cut_pairs=cuts, steps=200):
        for it in s.items:
            lo, hi = min(it.frame0, it.frame1), max(it.frame0, it.frame1)
            assert not any(lo <= p < hi for p in cuts)
    # a clip cut everywhere has no triplet
    with pytest.raises(ValueError):
        _schedule(n_frames=5, cut_pairs=(0, 1, 2, 3))


def test_schedule_spans_and_shared_t():
    steps = _schedule(spans=(2, 3), steps=200)
    assert {(s.span, s.j) for s in steps} == {(2, 1), (3, 1), (3, 2)}
    assert {s.reversed for s in steps} == {False, True}
    for s in steps:
        fwd = Fraction(s.j, s.span)
        assert s.t == (1 - fwd if s.reversed else fwd)
        for it in s.items:   # one t for the step: every item has the same j and direction
            a = min(it.frame0, it.frame1)
            assert it.frame_t == a + s.j
            assert (it.frame0 > it.frame1) == s.reversed


def test_schedule_without_augment():
    for s in _schedule(augment=False, spans=(2, 3)):
        assert not s.reversed and s.t == Fraction(s.j, s.span)
        for it in s.items:
            assert (it.y0, it.x0, it.flip) == (0, 0, 0) and it.frame0 < it.frame_t < it.frame1


@pytest.mark.parametrize("kw", [{"n_frames": 2}, {"n_frames": 3, "spans": (2, 3)}, {"crop": (64, 32)},
                                {"crop": (16, 80)}, {"crop": 24}, {"crop": (16, 40)}, {"crop": 0}])
def test_schedule_value_errors(kw):
    with pytest.raises(ValueError):
        _schedule(**kw)


# ---- the sampler's definition ------------------------------------------------------------------------
def _rgb(n, h, w, depth, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 1 << depth, (n, h, w, 3), generator=g, dtype=torch.int32)
    return x.to(torch.uint8) if depth == 8 else yuv.int_to_words(x)


def _written_definition(frames, it, ch, cw, layout, depth, top):
    """Section 1a of the issue, restated: the whole frame through the input mapping, the crop (the
    mapping pads ``top`` rows above the frame), the flip."""
    out = []
    for f in it[:3]:
        fr = frames[f:f + 1]
        if depth == 8:
            x = convert.frames_u8_to_float(yuv.yuv_to_rgb(fr, layout, None))
        else:
            x = convert.frames_u16_to_float(yuv.yuv_to_rgb16(fr, layout, None, depth, False), depth)
        x = x[:, :, top + it[3]:top + it[3] + ch, it[4]:it[4] + cw]
        out.append(x.flip(3) if it[5] == 1 else x.flip(2) if it[5] == 2 else x)
    return out


@pytest.mark.parametrize("layout,depth,h,w", [("i420", 8, 40, 48), ("i422", 10, 37, 48)])
def test_sample_triplets_cpu_is_the_definition(layout, depth, h, w):
    rgb = _rgb(4, h, w, depth, 3)
    frames = yuv.rgb_to_yuv(rgb, layout) if depth == 8 else yuv.rgb16_to_yuv(rgb, layout, None, depth, False)
    by = yuv.block_of(yuv.chroma_of(layout))[0]
    items = [(0, 1, 2, 0, 0, 0), (3, 2, 1, (h - 16) // by * by, w - 32, 1), (1, 2, 3, by, 2, 2)]
    got = ft.sample_triplets(frames, items, (16, 32), layout, None, depth)
    top = (16 - h % 16) % 16
    for k, it in enumerate(items):
        want = _written_definition(frames, it, 16, 32, layout, depth, top)
        for j in range(3):
            assert got[j].dtype == torch.float32 and got[j].shape == (3, 3, 16, 32)
            assert torch.equal(got[j][k:k + 1], want[j])
    for bad in [(0, 1, 4, 0, 0, 0), (0, 1, 2, h - 15, 0, 0), (0, 1, 2, 0, 1, 0), (0, 1, 2, 0, 0, 3)]:
        with pytest.raises(ValueError):
            ft.sample_triplets(frames, [bad], (16, 32), layout, None, depth)


# ---- the loss ----------------------------------------------------------------------------------------
def test_frame_loss_ref_is_the_references_expressions():
    g = torch.Generator().manual_seed(1)
    o = torch.rand((3, 3, 8, 10), generator=g, dtype=torch.float64).requires_grad_()
    t = torch.rand((3, 3, 8, 10), generator=g, dtype=torch.float64)
    t[0, 0, 0, :3] = o.detach()[0, 0, 0, :3]   # d == 0: sign(0) = 0
    ref = torch.sum(torch.sqrt((o - t).pow(2) + 1e-6)) / 3 / 1e3 + (o - t).abs().mean() / 10   # losses.py:39-42, train.py:105
    gref, = torch.autograd.grad(ref, o)
    o2 = o.detach().clone().requires_grad_()
    loss = ft.frame_loss_ref(o2, t)
    assert loss.dtype == torch.float64
    assert abs(loss.item() - ref.item()) <= 1e-15 * abs(ref.item()) * 10
    loss.backward()
    assert torch.allclose(o2.grad, gref, rtol=1e-13, atol=0)
    sums, grad = ft.frame_loss_parts_ref(o.detach(), t)
    assert torch.allclose(grad, gref, rtol=1e-13, atol=0)
    assert abs(1e-3 * sums[0].item() / 3 + 1e-1 * sums[1].item() / o.numel() - ref.item()) <= 1e-14 * ref.item()
    assert abs(sums[2].item() - (o - t).pow(2).sum().item()) <= 1e-14 * sums[2].item()
    # fp32 inputs: the loss and its gradient go through float64
    o3 = o.detach().float().requires_grad_()
    ft.frame_loss_ref(o3, t.float()).backward()
    assert o3.grad.dtype == torch.float32 and torch.allclose(o3.grad.double(), gref, rtol=1e-4, atol=1e-9)


# ---- command line ----------------------------------------------------------------------------------
def test_cli_finetune_parses_and_train_is_still_refused():
    a = build_parser().parse_args(["--model_name", "M", "finetune", "--y4m_in", "clip.y4m", "--steps", "7", "--batch", "3",
                                   "--crop", "128", "--spans", "2,3,4", "--lr", "3e-5", "--seed", "9",
                                   "--scene_threshold", "30", "--val_fraction", "0.2", "--no_augment", "--report",
                                   "r.json"])
    assert (a.mode, a.y4m_in, a.steps, a.batch, a.crop, a.spans) == ("finetune", "clip.y4m", 7, 3, 128, (2, 3, 4))
    assert (a.lr, a.seed, a.scene_threshold, a.val_fraction, a.no_augment, a.report) == (3e-5, 9, 30.0, 0.2, True,
                                                                                        "r.json")
    d = build_parser().parse_args(["--model_name", "M", "finetune", "--y4m_in", "-", "--steps", "1"])
    assert (d.batch, d.crop, d.spans, d.lr, d.seed, d.scene_threshold, d.val_fraction, d.no_augment, d.report) == \
        (2, 256, (2,), 1e-4, 0, None, 0.1, False, None)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--model_name", "M", "finetune", "--y4m_in", "-", "--steps", "1", "--spans", "1,2"])
    with pytest.raises(SystemExit) as e:
        main(["--model_name", "M", "train", "--train_folder", "x"])
    assert str(e.value) == ("rrin_amd does not ship the training loop (AdamW, VGG19 perceptual loss: out of "
                            "scope, SURVEY §2 rows 11-12); Net.forward / backward run on the HIP training "
                            "kernels under autograd, so drive them from your own loop or the reference train.py")


# ---- the loop on the CPU -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_runs(tmp_path_factory):
    raw = clip_bytes(32, 32, 11)
    out = []
    for k in range(2):
        path = tmp_path_factory.mktemp("ft") / f"M{k}.pth"
        res = ft.finetune_y4m(keyed_net(), io.BytesIO(raw), 2, batch=1, crop=32, augment=False, val_fraction=0.3,
                              save=str(path), log=lambda *a: None)
        out.append((res, path))
    return out


def test_cpu_loop_result_and_checkpoint(cpu_runs):
    res, path = cpu_runs[0]
    assert len(res["losses"]) == 2 and all(torch.isfinite(torch.tensor(res["losses"])))
    assert (res["frames"], res["train_frames"], res["val_frames"]) == (11, 7, 4)
    assert res["logged"][-1]["step"] == 2 and len(res["logged"][-1]["sums"]) == 3
    assert res["val_before"]["frames"] == [8] == res["val_after"]["frames"]   # inputs 7 and 9; frame 10 ignored
    assert res["val_before"]["sse"] != res["val_after"]["sse"]
    assert all(max(it[:3]) < 7 for s in res["schedule"] for it in s.items)   # the validation frames are never sampled
    state = torch.load(path, map_location="cpu", weights_only=True)
    assert set(state) == {"model", "optim", "epoch"} and state["epoch"] == 1
    keys = open(GOLDEN_KEYS).read().split()
    assert list(state["model"]) == keys and len(keys) == 162
    fresh = Net()
    fresh.load_state_dict(state["model"], strict=True)
    start = keyed_net().state_dict()
    assert all(not torch.equal(state["model"][k], start[k]) for k in keys)
    torch.optim.AdamW(fresh.parameters(), lr=1e-4).load_state_dict(state["optim"])   # what a --resume does


def test_cpu_loop_is_reproducible(cpu_runs):
    a = torch.load(cpu_runs[0][1], map_location="cpu", weights_only=True)["model"]
    b = torch.load(cpu_runs[1][1], map_location="cpu", weights_only=True)["model"]
    assert all(a[k].numpy().tobytes() == b[k].numpy().tobytes() for k in a)
    assert cpu_runs[0][0]["losses"] == cpu_runs[1][0]["losses"]


def test_cpu_fixed_batch_descends():
    res = ft.finetune_y4m(keyed_net(), io.BytesIO(clip_bytes(32, 32, 3)), **DESCENT, log=lambda *a: None)
    items = [s.items for s in res["schedule"]]
    assert all(i == [ft.Item(0, 1, 2, 0, 0, 0)] for i in items) and len(items) == 8
    print("CPU fixed-batch losses:", res["losses"])
    assert res["losses"][7] < res["losses"][0]
