"""GPU: the kernels of csrc/perceptual.hip, each alone against the definition -- ReLU and the 2x2
max pool bit for bit against PyTorch's CPU operators and their autograd, the feature distance against
float64 -- with guard words around every output and every refusal code."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from rrin_amd import _lib

pytestmark = pytest.mark.gpu

E_SHAPE, E_ARG, E_WORKSPACE = -1, -2, -3
NAN_BITS = 0x7FC0BEEF   # the pattern in and around the outputs before a call
GUARD = 64              # floats on either side of a tensor (a multiple of 4: offset 0 stays 16-byte aligned)
U = 2.0 ** -24
# the elementwise grids are capped at 2048 workgroups of 256 lanes; past that a lane strides on
GRID_LANES = 2048 * 256


def stream(gpu):
    return C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)


class Guarded:
    """``count`` floats inside a buffer of NAN_BITS, GUARD floats on either side; ``offset`` floats more in
    front move the tensor off 16-byte alignment (the kernels' single-element path)."""

    def __init__(self, count, gpu, offset=0, fill=None):
        self.lo = GUARD + offset
        self.count = count
        self.buf = torch.full((self.lo + count + GUARD,), NAN_BITS, dtype=torch.int32, device=gpu)
        if fill is not None:
            self.t.copy_(fill.reshape(-1))

    @property
    def t(self):
        return self.buf[self.lo:self.lo + self.count].view(torch.float32)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.lo

    def guards_ok(self):
        return bool((self.buf[:self.lo] == NAN_BITS).all()) and bool((self.buf[self.lo + self.count:] == NAN_BITS).all())

    def untouched(self):
        return bool((self.buf == NAN_BITS).all())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- ReLU ---------------------------------------------------------------------------------------------
RELU_COUNTS = [1, 3, 4, 5, 2047, 2048, 2049, 4 * GRID_LANES + 1029]


def relu_input(count, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(count, generator=g)
    gy = torch.randn(count, generator=g)
    for j, v in enumerate((-0.0, 0.0, float("nan"), -1.5, 2.5, -0.0)):   # spread over a 16-byte group and the tail
        if j < count:
            x[(count - 1 - j * 5) % count] = v
    return x, gy


def relu_bwd_ref(gy, y):
    """The kernel's contract: gx = y > 0 ? gy : 0 (the gradient of a NaN is 0; PyTorch passes gy there)."""
    return torch.where(y > 0, gy, torch.zeros_like(gy))


@pytest.mark.parametrize("count", RELU_COUNTS)
@pytest.mark.parametrize("offset", [0, 1])
def test_relu_bit_for_bit(gpu, count, offset):
    lib = _lib.lib()
    x, gy = relu_input(count, count + offset)
    xr = x.clone().requires_grad_()
    want = torch.relu(xr)
    want.backward(gy)
    gx_want = relu_bwd_ref(gy, want.detach())
    finite = ~torch.isnan(x)
    assert torch.equal(gx_want[finite], xr.grad[finite])   # the contract is PyTorch's autograd away from NaNs
    # out of place
    xd, yd = Guarded(count, gpu, offset, x), Guarded(count, gpu, offset)
    assert lib.rrin_trelu_fwd(xd.ptr, yd.ptr, count, stream(gpu)) == 0
    assert torch.equal(bits(yd.t), bits(want)) and yd.guards_ok()
    assert torch.equal(bits(xd.t), bits(x))
    gyd, gxd = Guarded(count, gpu, offset, gy), Guarded(count, gpu, offset)
    assert lib.rrin_trelu_bwd(gyd.ptr, yd.ptr, gxd.ptr, count, stream(gpu)) == 0
    assert torch.equal(bits(gxd.t), bits(gx_want)) and gxd.guards_ok()
    # in place: x == y, gy == gx
    assert lib.rrin_trelu_fwd(xd.ptr, xd.ptr, count, stream(gpu)) == 0
    assert torch.equal(bits(xd.t), bits(want)) and xd.guards_ok()
    assert lib.rrin_trelu_bwd(gyd.ptr, xd.ptr, gyd.ptr, count, stream(gpu)) == 0
    assert torch.equal(bits(gyd.t), bits(gx_want)) and gyd.guards_ok()


@pytest.mark.parametrize("value", [-0.0, 0.0, float("nan"), -3.0, 3.0, float("-inf"), float("inf")])
def test_relu_single_values(gpu, value):
    lib = _lib.lib()
    x = torch.tensor([value])
    xd, yd = Guarded(1, gpu, 0, x), Guarded(1, gpu)
    assert lib.rrin_trelu_fwd(xd.ptr, yd.ptr, 1, stream(gpu)) == 0
    assert torch.equal(bits(yd.t), bits(torch.relu(x))) and yd.guards_ok()


# ---- 2x2 max pool -------------------------------------------------------------------------------------
# the shapes the issue names take the one-window-per-lane path (w no multiple of 4); (2,4,8), (3,6,12) and
# (4,16,40) take the two-window 16-byte path, (4,16,40) and (5,18,34) more than one workgroup on either
POOL_SHAPES = [(1, 2, 2), (3, 6, 10), (2, 4, 34), (1, 2, 66), (2, 4, 8), (3, 6, 12), (4, 16, 40), (5, 18, 34)]
POOL_KINDS = ["random", "equal", "zero", "nan"]


def pool_input(shape, kind, seed):
    nc, h, w = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, nc, h, w, generator=g)
    gy = torch.randn(1, nc, h // 2, w // 2, generator=g)
    last = x[0, nc - 1, h - 2:, w - 2:]   # the last window: the one a lane past the end would own
    first = x[0, 0, :2, :2]
    if kind == "equal":       # all-equal positive windows: the first element is the arg-max
        first[:] = 3.0
        last[:] = 0.5
    elif kind == "zero":      # all-zero windows, and a mix of the two zeros
        first[:] = 0.0
        last[:] = torch.tensor([[0.0, -0.0], [-0.0, 0.0]])
    elif kind == "nan":       # the last NaN of a window is the arg-max
        first[:] = torch.tensor([[1.0, float("nan")], [float("nan"), 3.0]])
        last[:] = torch.tensor([[float("nan"), 2.0], [1.0, 0.5]])
    return x, gy


@pytest.mark.parametrize("shape", POOL_SHAPES)
@pytest.mark.parametrize("kind", POOL_KINDS)
@pytest.mark.parametrize("offset", [0, 1])
def test_max_pool_bit_for_bit(gpu, shape, kind, offset):
    lib = _lib.lib()
    nc, h, w = shape
    x, gy = pool_input(shape, kind, nc * 1000 + h * 10 + w)
    xr = x.clone().requires_grad_()
    want = F.max_pool2d(xr, 2, 2)
    want.backward(gy)
    xd = Guarded(x.numel(), gpu, offset, x)
    yd = Guarded(want.numel(), gpu, offset)
    assert lib.rrin_tmaxpool2_fwd(xd.ptr, yd.ptr, nc, h, w, stream(gpu)) == 0
    assert torch.equal(bits(yd.t), bits(want).reshape(-1)) and yd.guards_ok()
    gyd = Guarded(gy.numel(), gpu, offset, gy)
    gxd = Guarded(x.numel(), gpu, offset)   # NaN before the call: every element must be written
    assert lib.rrin_tmaxpool2_bwd(gyd.ptr, xd.ptr, gxd.ptr, nc, h, w, stream(gpu)) == 0
    got = gxd.t.cpu()
    assert not bool(torch.isnan(got).any())
    assert torch.equal(bits(got), bits(xr.grad).reshape(-1)) and gxd.guards_ok()
    assert torch.equal(bits(xd.t), bits(x).reshape(-1))


def test_max_pool_first_maximum_rule(gpu):
    """Spelled out, not only inherited from the CPU operator: equal maxima -> the first in row-major order."""
    lib = _lib.lib()
    x = torch.tensor([[[1.0, 4.0, 0.0, 0.0], [4.0, 4.0, 0.0, 0.0]]])   # windows (1 4 / 4 4) and all zeros
    gy = torch.tensor([[[7.0, 9.0]]])
    xd, gyd, gxd = Guarded(8, gpu, 0, x), Guarded(2, gpu, 0, gy), Guarded(8, gpu)
    assert lib.rrin_tmaxpool2_bwd(gyd.ptr, xd.ptr, gxd.ptr, 1, 2, 4, stream(gpu)) == 0
    assert gxd.t.cpu().tolist() == [0.0, 7.0, 9.0, 0.0, 0.0, 0.0, 0.0, 0.0]


# ---- feature distance -----------------------------------------------------------------------------------
# 1024 partials of 2048-element tiles: past 1024 * 2048 elements a workgroup takes a second tile
DIST_COUNTS = [1, 2047, 2048, 2049, 3 * 2048 + 5, 1024 * 2048 + 3 * 2048 + 5]


def featdist(a, b, gpu, offset=0, grad=True, short=0):
    """rrin_tfeatdist on host tensors: (code, sum, Guarded grad or None)."""
    lib = _lib.lib()
    count = a.numel()
    need = lib.rrin_tfeatdist_workspace_bytes(count)
    assert need > 0 and need % 8 == 0
    ws = torch.zeros(need // 8, dtype=torch.float64, device=gpu)
    sums = torch.full((1,), -1.0, dtype=torch.float64, device=gpu)
    ad, bd = Guarded(count, gpu, offset, a), Guarded(count, gpu, offset, b)
    g = Guarded(count, gpu, offset) if grad else None
    rc = lib.rrin_tfeatdist(ad.ptr, bd.ptr, count, sums.data_ptr(), g.ptr if grad else None, ws.data_ptr(),
                            need - short, stream(gpu))
    return rc, sums.cpu(), g


def dist_pair(count, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(count, generator=g), torch.randn(count, generator=g)


@pytest.mark.parametrize("count", DIST_COUNTS)
@pytest.mark.parametrize("offset", [0, 1])
def test_feature_distance(gpu, count, offset):
    """Differences are exact in float64 and each square is rounded once, so the sum and the gradient sit
    far inside rrin_tloss's bound for the same reduction: 4 * 2^-24 relative."""
    a, b = dist_pair(count, 17 + count + offset)
    rc, sums, g = featdist(a, b, gpu, offset)
    assert rc == 0
    d = a.double() - b.double()
    ref = (d * d).sum()
    rel = abs(sums[0].item() - ref.item()) / ref.item()
    print("count", count, "offset", offset, "sum rel err / 2^-24:", rel / U)
    assert rel <= 4 * U
    rg = d / torch.sqrt(ref)
    err = (g.t.cpu().double() - rg).abs()
    bound = 4 * U * rg.abs() + 2.0 ** -40
    print("grad max err / bound:", (err / bound).max().item())
    assert bool((err <= bound).all()) and g.guards_ok()
    rc2, sums2, g2 = featdist(a, b, gpu, offset)                 # the same bits on every run
    rc3, sums3, none = featdist(a, b, gpu, offset, grad=False)   # and without a gradient
    assert (rc2, rc3) == (0, 0) and none is None
    assert torch.equal(sums.view(torch.int64), sums2.view(torch.int64))
    assert torch.equal(sums.view(torch.int64), sums3.view(torch.int64))
    assert torch.equal(bits(g.t), bits(g2.t))


@pytest.mark.parametrize("count", [1, 2049])
def test_feature_distance_of_equal_tensors(gpu, count):
    a, _ = dist_pair(count, 3)
    rc, sums, g = featdist(a, a.clone(), gpu)
    assert rc == 0 and sums[0].item() == 0.0
    assert torch.equal(bits(g.t), torch.zeros(count, dtype=torch.int32)) and g.guards_ok()   # +0: no NaN


# ---- refusals -------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(gpu):
    lib = _lib.lib()
    st = stream(gpu)
    x = Guarded(64, gpu, 0, torch.ones(64))
    y, z = Guarded(64, gpu), Guarded(64, gpu)
    sums = torch.full((1,), -1.0, dtype=torch.float64, device=gpu)
    need = lib.rrin_tfeatdist_workspace_bytes(64)
    ws = torch.zeros(need // 8 + 1, dtype=torch.float64, device=gpu)
    cases = [
        (E_ARG, lib.rrin_trelu_fwd(None, y.ptr, 64, st)), (E_ARG, lib.rrin_trelu_fwd(x.ptr, None, 64, st)),
        (E_ARG, lib.rrin_trelu_fwd(x.ptr + 2, y.ptr, 60, st)), (E_ARG, lib.rrin_trelu_fwd(x.ptr, y.ptr + 1, 60, st)),
        (E_SHAPE, lib.rrin_trelu_fwd(x.ptr, y.ptr, 0, st)), (E_SHAPE, lib.rrin_trelu_fwd(x.ptr, y.ptr, -4, st)),
        (E_ARG, lib.rrin_trelu_bwd(None, x.ptr, y.ptr, 64, st)), (E_ARG, lib.rrin_trelu_bwd(x.ptr, None, y.ptr, 64, st)),
        (E_ARG, lib.rrin_trelu_bwd(x.ptr, x.ptr, None, 64, st)),
        (E_ARG, lib.rrin_trelu_bwd(x.ptr, x.ptr, y.ptr + 3, 60, st)),
        (E_SHAPE, lib.rrin_trelu_bwd(x.ptr, x.ptr, y.ptr, 0, st)),
        (E_ARG, lib.rrin_tmaxpool2_fwd(None, y.ptr, 1, 8, 8, st)), (E_ARG, lib.rrin_tmaxpool2_fwd(x.ptr, None, 1, 8, 8, st)),
        (E_ARG, lib.rrin_tmaxpool2_fwd(x.ptr, y.ptr + 2, 1, 8, 6, st)),
        (E_SHAPE, lib.rrin_tmaxpool2_fwd(x.ptr, y.ptr, 0, 8, 8, st)),
        (E_SHAPE, lib.rrin_tmaxpool2_fwd(x.ptr, y.ptr, 1, 7, 8, st)),
        (E_SHAPE, lib.rrin_tmaxpool2_fwd(x.ptr, y.ptr, 1, 8, 7, st)),
        (E_SHAPE, lib.rrin_tmaxpool2_fwd(x.ptr, y.ptr, 1, 0, 8, st)),
        (E_SHAPE, lib.rrin_tmaxpool2_fwd(x.ptr, y.ptr, 1, 8, 0, st)),
        (E_ARG, lib.rrin_tmaxpool2_bwd(None, x.ptr, y.ptr, 1, 8, 8, st)),
        (E_ARG, lib.rrin_tmaxpool2_bwd(x.ptr, None, y.ptr, 1, 8, 8, st)),
        (E_ARG, lib.rrin_tmaxpool2_bwd(x.ptr, x.ptr, None, 1, 8, 8, st)),
        (E_ARG, lib.rrin_tmaxpool2_bwd(x.ptr, x.ptr, y.ptr + 1, 1, 8, 6, st)),
        (E_SHAPE, lib.rrin_tmaxpool2_bwd(x.ptr, x.ptr, y.ptr, -1, 8, 8, st)),
        (E_SHAPE, lib.rrin_tmaxpool2_bwd(x.ptr, x.ptr, y.ptr, 1, 9, 8, st)),
        (E_SHAPE, lib.rrin_tmaxpool2_bwd(x.ptr, x.ptr, y.ptr, 1, 8, 1, st)),
        (E_ARG, lib.rrin_tfeatdist(None, x.ptr, 64, sums.data_ptr(), y.ptr, ws.data_ptr(), need, st)),
        (E_ARG, lib.rrin_tfeatdist(x.ptr, None, 64, sums.data_ptr(), y.ptr, ws.data_ptr(), need, st)),
        (E_ARG, lib.rrin_tfeatdist(x.ptr, x.ptr, 64, None, y.ptr, ws.data_ptr(), need, st)),
        (E_ARG, lib.rrin_tfeatdist(x.ptr, x.ptr, 64, sums.data_ptr(), y.ptr, None, need, st)),
        (E_ARG, lib.rrin_tfeatdist(x.ptr, x.ptr, 60, sums.data_ptr(), y.ptr + 2, ws.data_ptr(), need, st)),
        (E_ARG, lib.rrin_tfeatdist(x.ptr, x.ptr, 64, sums.data_ptr(), y.ptr, ws.data_ptr() + 4, need, st)),
        (E_SHAPE, lib.rrin_tfeatdist(x.ptr, x.ptr, 0, sums.data_ptr(), y.ptr, ws.data_ptr(), need, st)),
        (E_WORKSPACE, lib.rrin_tfeatdist(x.ptr, x.ptr, 64, sums.data_ptr(), y.ptr, ws.data_ptr(), need - 1, st)),
        (E_SHAPE, lib.rrin_tfeatdist_workspace_bytes(0)), (E_SHAPE, lib.rrin_tfeatdist_workspace_bytes(-5)),
    ]
    torch.cuda.synchronize(gpu)
    for n, (want, got) in enumerate(cases):
        assert got == want, (n, want, got)
    assert y.untouched() and z.untouched() and sums.item() == -1.0
    assert bool((x.t == 1).all())
    # and the calls next to them are taken
    assert lib.rrin_trelu_fwd(x.ptr, y.ptr, 64, st) == 0
    assert lib.rrin_tmaxpool2_fwd(x.ptr, z.ptr, 1, 8, 8, st) == 0
    torch.cuda.synchronize(gpu)
    assert y.guards_ok() and z.buf[GUARD + 16:].eq(NAN_BITS).all()
