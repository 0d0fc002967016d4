"""Case tables and float64 references of the whole-forward contract tests (no GPU):
tests/test_net_contract_ref.py checks them on the CPU, tests/test_gpu_net_contract.py runs the
library against them.

* U-Net over the contract of ``rrin_unet_fwd`` (in_ch 1..16, out_ch 2..4, depth 2..5): the table
  UNET_CASES, key-seeded weights whose ``last`` conv is scaled by LAST_SCALE so that max|ref| lies
  in [0.5, 2] (the keyed outputs are 0.07-0.09, where a tolerance relative to max(1, max|ref|)
  would be 10x slack), the oracle's ``unet_forward`` in float64.
* Net on its smallest frames and at the ends of t: NET_SIZES x NET_T, the oracle's ``net_forward``
  with the state dict and the frames cast to float64.

Every reference is computed once per process (lru_cache) and returned to all callers: treat the
tensors as read-only."""
from functools import lru_cache

import torch

from oracle.ref_net import net_forward, unet_forward
from rrin_amd import Net, UNet
from rrin_amd.synthetic import keyed_state_dict, synthetic_batch

PRECISIONS = ("fp32", "fp32_planar", "fp32_split16", "fp16")
RECORD_PRECISIONS = ("fp32", "fp32_split16", "fp16")

# ---- A: one U-Net ---------------------------------------------------------------------------
# tolerance of test_unet_alone_golden (tests/test_gpu_configs.py): factor x max(1, max|ref|)
UNET_TOL = {"fp32": 1e-5, "fp32_planar": 1e-5, "fp32_split16": 1e-4, "fp16": 3e-2}
UNET_SIZES = ((1, 16, 16), (3, 16, 48), (2, 48, 32))  # n, h, w
UNET_IN_CH = (1, 3, 4, 5, 8, 12, 16)
# (in_ch, out_ch, depth): every listed in_ch at depths 2 and 5, every depth with every out_ch
UNET_CASES = (
    (1, 2, 2), (3, 3, 2), (4, 4, 2), (5, 2, 2), (8, 3, 2), (12, 4, 2), (16, 2, 2),
    (1, 2, 3), (5, 3, 3), (12, 4, 3),
    (3, 4, 4), (8, 2, 4), (16, 3, 4),
    (1, 3, 5), (3, 4, 5), (4, 2, 5), (5, 3, 5), (8, 4, 5), (12, 2, 5), (16, 4, 5),
)
LAST_SCALE = 12.0
PREFIX = "u"


def unet_state_dict(ci: int, co: int, d: int):
    """Key-seeded weights of UNet(ci, co, d), ``last`` scaled by LAST_SCALE (fp32, module keys)."""
    sd = keyed_state_dict(UNet(ci, co, d).state_dict())
    sd["last.weight"] = sd["last.weight"] * LAST_SCALE
    sd["last.bias"] = sd["last.bias"] * LAST_SCALE
    return sd


def make_unet(ci: int, co: int, d: int) -> UNet:
    u = UNet(ci, co, d)
    u.load_state_dict(unet_state_dict(ci, co, d), strict=True)
    return u.eval()


def unet_input(ci: int, n: int, h: int, w: int, which: int = 0) -> torch.Tensor:
    """Input ``which`` (0, 1: two different tensors) of a case: uniform in [-1, 1)."""
    g = torch.Generator().manual_seed(1000003 * which + 10007 * ci + 101 * n + 7 * h + w)
    return torch.rand(n, ci, h, w, generator=g) * 2 - 1


def _prefixed(sd, dtype):
    return {f"{PREFIX}.{k}": v.to(dtype) for k, v in sd.items()}


@lru_cache(maxsize=None)
def unet_ref(ci: int, co: int, d: int, n: int, h: int, w: int, which: int = 0) -> torch.Tensor:
    """float64 reference of the case's U-Net on unet_input(ci, n, h, w, which)."""
    with torch.no_grad():
        return unet_forward(_prefixed(unet_state_dict(ci, co, d), torch.float64), PREFIX,
                            unet_input(ci, n, h, w, which).double())


def unet_oracle32(ci: int, co: int, d: int, n: int, h: int, w: int, which: int = 0) -> torch.Tensor:
    """The fp32 oracle on the same case (reference sanity)."""
    with torch.no_grad():
        return unet_forward(_prefixed(unet_state_dict(ci, co, d), torch.float32), PREFIX,
                            unet_input(ci, n, h, w, which))


# ---- B: the Net -----------------------------------------------------------------------------
NET_SIZES = ((1, 16, 16), (2, 16, 64), (2, 64, 16), (3, 32, 48))  # n, h, w
NET_WEIGHTS = ("default", "stress")
NET_T = ("0", "1", "0.5", "tensor")
NET_FIRST_INDEX = 70
# project gates: the fp32-class precisions by weights, fp16 max-abs and PSNR
NET_GATE = {"default": 1e-4, "stress": 1e-3}
FP16_MAXABS, FP16_PSNR = 1e-2, 45.0
# fp16 only: cases whose max-abs misses 1e-2 through rounding, not a defect.  With the
# stress weights at t = 1 the refine_flow output reaches 20 px (6 px at t = 0 and 0.5) and its fp16
# error is the same 8e-4 relative: 1.6e-2 px against 4.8e-3 px.  A float64 model of the oracle that
# only rounds every conv's input, weights and output to fp16 gives 1.23e-2 (16x64) and 1.44e-2
# (32x48) for the frame; the library measured 1.23e-2 and 1.18e-2.  Their PSNR gate stays.
FP16_ROUNDING = {("stress", (2, 16, 64), "1"), ("stress", (2, 16, 64), "tensor"),
                 ("stress", (3, 32, 48), "1"), ("stress", (3, 32, 48), "tensor")}
TAP_TOL = 1e-4  # test_unet_taps_golden: x max(1, max|want|), the fp32-class precisions
# engine.forward(taps=...) name -> the oracle's taps key
TAP_KEYS = {"Flow": "Flow", "refine_flow": "refine", "Mask": "mask_logits", "final": "final_unet"}


def net_t(name: str, n: int):
    """The t of case ``name`` for a batch of n: a Python float, or for "tensor" a per-sample fp32
    tensor [n,1,1,1] cycling 0, 1, 0.5 (n = 1: the one-element tensor 0, the tensor-arithmetic
    branch of the coefficient table)."""
    if name == "tensor":
        return torch.tensor(([0.0, 1.0, 0.5] * n)[:n]).view(n, 1, 1, 1)
    return float(name)


@lru_cache(maxsize=None)
def net_state_dict(which: str):
    return keyed_state_dict(Net().state_dict(), stress=which == "stress")


def net_frames(n: int, h: int, w: int, first_index: int = NET_FIRST_INDEX):
    return synthetic_batch(n, h, w, first_index=first_index)


@lru_cache(maxsize=None)
def _sd64(which: str):
    return {k: v.double() for k, v in net_state_dict(which).items()}


@lru_cache(maxsize=None)
def net_ref(which: str, n: int, h: int, w: int, tname: str, first_index: int = NET_FIRST_INDEX):
    """(float64 output, taps dict) of the oracle with state dict and frames cast to float64."""
    i0, i1 = net_frames(n, h, w, first_index)
    t = net_t(tname, n)
    taps = {}
    with torch.no_grad():
        out = net_forward(_sd64(which), i0.double(), i1.double(), t.double() if isinstance(t, torch.Tensor) else t,
                          taps=taps)
    return out, taps


def net_oracle32(which: str, n: int, h: int, w: int, tname: str, first_index: int = NET_FIRST_INDEX):
    i0, i1 = net_frames(n, h, w, first_index)
    with torch.no_grad():
        return net_forward(net_state_dict(which), i0, i1, net_t(tname, n))


def maxabs(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.double() - b.double()).abs().max())


def psnr(a: torch.Tensor, b: torch.Tensor) -> float:
    """PSNR (peak 1) over the whole batch; inf for equal tensors."""
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float("inf") if mse == 0 else 10 * float(torch.log10(torch.tensor(1.0 / mse, dtype=torch.float64)))
