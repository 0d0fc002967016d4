"""GPU: the perceptual term through rrin_amd.autograd -- the frozen VGG convs on the training route,
ReLU, max pool and the feature distance -- against the CPU definition (rrin_amd/perceptual.py).

Tolerance.  The definition runs twice on the CPU, in fp32 and in float64, on the same inputs.  The
GPU path may differ from float64 by at most 4 x the larger of (a) the fp32 CPU run's own error and (b)
1e-5 per conv, the bound tests/test_gpu_train.py applies to one training conv (max-abs error over
max-abs value), compounded over the stack's 12 convs: 1.2e-4.  Nothing of the bound comes from the
GPU result.  Errors are max-abs over max-abs, as in test_gpu_train.py."""
import pytest
import torch

from rrin_amd import autograd as ag
from rrin_amd import perceptual as pc

pytestmark = pytest.mark.gpu

SMALL = (4, 4, "M", 8, 8, "M", 8, 8, 8, 8, "M", 16, 16, 16, 16)
PER_CONV, CONVS = 1e-5, 12
CASES = {"small16": (SMALL, 2, 16, 16), "small24": (SMALL, 2, 16, 24), "vgg19": (pc.VGG19_RELU4_4, 1, 16, 16)}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(b.abs().max(), 1e-30))


def double_of(vgg):
    v = pc.VggFeatures(vgg.cfg, vgg.weights, vgg.biases)
    v.weights, v.biases = [w.double() for w in vgg.weights], [b.double() for b in vgg.biases]
    return v


@pytest.fixture(scope="module")
def refs():
    """Per case: the VggFeatures, the frames and the CPU definition's loss and gradient in fp32 and float64
    (computed once, shared, left unchanged)."""
    out = {}
    for name, (cfg, n, h, w) in CASES.items():
        vgg = pc.VggFeatures.synthetic(cfg)
        g = torch.Generator().manual_seed(len(name))
        o, t = torch.rand(n, 3, h, w, generator=g), torch.rand(n, 3, h, w, generator=g)
        a = o.clone().requires_grad_()
        l32 = pc.perceptual_loss(a, t, vgg)
        l32.backward()
        b = o.double().requires_grad_()
        l64 = pc.perceptual_loss(b, t.double(), double_of(vgg))
        l64.backward()
        out[name] = (vgg, o, t, l32.detach(), a.grad, l64.detach(), b.grad)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_loss_and_gradient_match_the_definition(gpu, refs, name):
    vgg, o, t, l32, g32, l64, g64 = refs[name]
    cpu_loss_err, cpu_grad_err = rel(l32, l64), rel(g32, g64)
    loss_bound = 4 * max(cpu_loss_err, PER_CONV * CONVS)
    grad_bound = 4 * max(cpu_grad_err, PER_CONV * CONVS)
    x = o.to(gpu).requires_grad_()
    tt = t.to(gpu).requires_grad_()
    loss = ag.perceptual_loss(x, tt, vgg)
    assert loss.dim() == 0 and loss.dtype == torch.float64 and loss.is_cuda
    loss.backward()
    le, ge = rel(loss, l64), rel(x.grad, g64)
    print(f"{name}: fp32 CPU vs float64: loss {cpu_loss_err:.3e} grad {cpu_grad_err:.3e}; GPU vs float64: loss {le:.3e} "
          f"grad {ge:.3e}; bounds {loss_bound:.3e} / {grad_bound:.3e}")
    assert le <= loss_bound and ge <= grad_bound
    assert tt.grad is None   # the gradient flows to out only
    # the same bits on every run
    x2 = o.to(gpu).requires_grad_()
    loss2 = ag.perceptual_loss(x2, t.to(gpu), vgg)
    loss2.backward()
    assert torch.equal(loss, loss2) and torch.equal(x.grad, x2.grad)


def test_equal_frames_give_zero(gpu, refs):
    vgg, o = refs["small16"][0], refs["small16"][1]
    x = o.to(gpu).requires_grad_()
    loss = ag.perceptual_loss(x, o.to(gpu), vgg)
    loss.backward()
    assert loss.item() == 0.0 and bool((x.grad == 0).all())


def saved_of(loss):
    """{data_ptr: bytes} of every tensor the graph of ``loss`` keeps for its backward."""
    seen, todo, kept = set(), [loss.grad_fn], {}
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        for t in getattr(fn, "saved_tensors", ()):
            if t is not None:
                kept[t.data_ptr()] = t.numel() * t.element_size()
        todo.extend(f for f, _ in fn.next_functions)
    return kept


def test_no_wgrad_and_nothing_of_the_target_branch_is_kept(gpu, refs):
    vgg, o, t = refs["small24"][:3]
    n, _, h, w = o.shape
    x = o.to(gpu).requires_grad_()
    ag.PROF = []
    try:
        loss = ag.perceptual_loss(x, t.to(gpu), vgg)
        kept = saved_of(loss)
        loss.backward()
        torch.cuda.synchronize(gpu)
        kinds = [k for _, _, _, k in ag.PROF]
    finally:
        ag.PROF = None
    # two branches of 12 forward convs, one backward of 12 data-gradient convs, no weight gradient
    assert kinds.count("fwd") == 24 and kinds.count("dgrad") == 12 and "wgrad" not in kinds
    assert kinds.count("vgg_conv") == 36 and kinds.count("vgg_relu") == 36 and kinds.count("vgg_pool") == 9
    assert kinds.count("vgg_dist") == 1
    assert set(kinds) == {"fwd", "dgrad", "vgg_conv", "vgg_relu", "vgg_pool", "vgg_dist"}
    # kept for the backward: the output branch's 12 ReLU outputs (a pool reads the one before it) and the
    # distance's gradient -- one branch's activations, not two
    acts, hh, ww = 0, h, w
    for v in vgg.cfg:
        if v == "M":
            hh, ww = hh // 2, ww // 2
        else:
            acts += 4 * n * v * hh * ww
    feat = 4 * n * vgg.cfg[-1] * hh * ww
    assert sum(kept.values()) == acts + feat and len(kept) == 13
    assert all(p.grad is None for p in vgg.weights + vgg.biases)


def test_packs_are_built_once_per_vgg_and_device(gpu, refs):
    _, o, t = refs["small16"][:3]
    vgg = pc.VggFeatures.synthetic(SMALL, seed=9)   # a fresh one: no packs yet
    before = ag.VGG_PACKS
    x = o.to(gpu).requires_grad_()
    ag.perceptual_loss(x, t.to(gpu), vgg).backward()
    first = ag.VGG_PACKS - before
    assert first == (24 if ag.TRAIN_WINO else 0)   # forward and data-gradient pack of each conv
    x2 = o.to(gpu).requires_grad_()
    ag.perceptual_loss(x2, t.to(gpu), vgg).backward()
    assert ag.VGG_PACKS - before == first and torch.equal(x.grad, x2.grad)


def test_functions_alone(gpu):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 3, 6, 8, generator=g)
    gy = torch.randn(2, 3, 3, 4, generator=g)
    xr = x.clone().requires_grad_()
    torch.nn.functional.max_pool2d(torch.relu(xr), 2, 2).backward(gy)
    xg = x.to(gpu).requires_grad_()
    y = ag.max_pool2(ag.relu(xg))
    y.backward(gy.to(gpu))
    assert torch.equal(y.cpu(), torch.nn.functional.max_pool2d(torch.relu(x), 2, 2)) and torch.equal(xg.grad.cpu(), xr.grad)
    a, b = x.to(gpu).requires_grad_(), (x + 1).to(gpu)
    d = ag.feature_distance(a, b)
    d.backward()
    assert abs(d.item() - x.numel() ** 0.5) <= 1e-6 * x.numel() ** 0.5
    with pytest.raises(ValueError):
        ag.perceptual_loss(torch.zeros(1, 3, 12, 16, device=gpu), torch.zeros(1, 3, 12, 16, device=gpu),
                           pc.VggFeatures.synthetic(SMALL))
