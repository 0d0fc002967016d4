"""The reference's VGG19 perceptual term, from a weights file the user already has.

The reference trains on ``CombinedLoss / 10 + charbonnierLoss / 1e3`` (train.py:103-105) with
``CombinedLoss = VggLoss + L1Loss`` and ``VggLoss = torch.norm(f(out) - f(gt), 2)`` over ``f`` =
torchvision's ``vgg19().features[:-10]``, the stack up to relu4_4 (losses.py:6-36).  This module is
the *definition* of that term in PyTorch operators, on any device; ``rrin_amd.autograd.perceptual_loss``
computes the same on a ROCm device with the HIP training kernels (``csrc/perceptual.hip`` and the
training convs).

The weights are read from a ``vgg19-*.pth`` state dict on disk (:meth:`VggFeatures.load`) and are
never fetched: nothing here imports torchvision or knows where such a file comes from.
"""
from __future__ import annotations

import math
import os
import zlib

import torch
import torch.nn.functional as F

# torchvision's vgg19().features[:-10] (modules 0..26): a number is Conv2d(3x3, padding 1) + ReLU of
# that many output channels, "M" is MaxPool2d(2, 2)
VGG19_RELU4_4 = (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512)
FRAME_MULTIPLE = 8   # three 2x2 pools


def conv_layout(cfg=VGG19_RELU4_4, in_ch=3):
    """[(index in ``features``, cin, cout)] of the convs of ``cfg``: a conv and its ReLU take two
    indices, a pool one (0, 2, 5, 7, 10, ... for VGG19)."""
    out, idx, cin = [], 0, in_ch
    for v in cfg:
        if v == "M":
            idx += 1
            continue
        v = int(v)
        if v < 1:
            raise ValueError(f"a conv of {v} channels in {cfg!r}")
        out.append((idx, cin, v))
        cin = v
        idx += 2
    if not out:
        raise ValueError(f"no conv in {cfg!r}")
    return out


class VggFeatures:
    """Frozen fp32 weights of the conv stack ``cfg``: ``weights[k]``, ``biases[k]`` of conv k
    (``[cout,cin,3,3]`` / ``[cout]``, no gradient), ``name`` the file name or ``"synthetic"``."""

    def __init__(self, cfg=VGG19_RELU4_4, weights=None, biases=None, name="synthetic"):
        self.cfg = tuple(cfg)
        self.layout = conv_layout(self.cfg)
        if weights is None and biases is None:   # empty, as a module is before its state dict is loaded
            weights = [torch.zeros(cout, cin, 3, 3) for _, cin, cout in self.layout]
            biases = [torch.zeros(cout) for _, _, cout in self.layout]
        if weights is None or biases is None or len(weights) != len(self.layout) or len(biases) != len(self.layout):
            raise ValueError(f"{len(self.layout)} weight and bias tensors are needed for {self.cfg!r}")
        self.weights, self.biases = [], []
        for (idx, cin, cout), w, b in zip(self.layout, weights, biases):
            _check_shape(f"{idx}.weight", w, (cout, cin, 3, 3))
            _check_shape(f"{idx}.bias", b, (cout,))
            self.weights.append(w.detach().to(torch.float32).contiguous().requires_grad_(False))
            self.biases.append(b.detach().to(torch.float32).contiguous().requires_grad_(False))
        self.name = name
        self._device = {}   # device -> what rrin_amd.autograd keeps there (weights, Winograd packs)

    @property
    def device(self):
        return self.weights[0].device

    def to(self, device):
        """The same weights on ``device`` (this object if they are there already)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self.device:
            return self
        return VggFeatures(self.cfg, [w.to(device) for w in self.weights], [b.to(device) for b in self.biases],
                           self.name)

    def state_dict(self, prefix="features."):
        """``{prefix + "N.weight" / "N.bias"}``, N the convs' indices in ``features``."""
        out = {}
        for (idx, _, _), w, b in zip(self.layout, self.weights, self.biases):
            out[f"{prefix}{idx}.weight"] = w
            out[f"{prefix}{idx}.bias"] = b
        return out

    @classmethod
    def from_state_dict(cls, state, cfg=VGG19_RELU4_4, name="state_dict"):
        """From a state dict with keys ``features.N.weight/bias`` (a whole torchvision model: its other
        keys are ignored) or ``N.weight/bias``.  ValueError names the missing or mis-shaped key."""
        if not isinstance(state, dict):
            raise ValueError(f"a VGG weights file holds a state dict, got {type(state).__name__}")
        layout = conv_layout(cfg)
        prefix = "features." if any(str(k).startswith("features.") for k in state) else ""
        ws, bs = [], []
        for idx, cin, cout in layout:
            for kind, shape, dest in (("weight", (cout, cin, 3, 3), ws), ("bias", (cout,), bs)):
                key = f"{prefix}{idx}.{kind}"
                if key not in state:
                    raise ValueError(f"the VGG state dict has no key {key!r}")
                _check_shape(key, state[key], shape)
                dest.append(state[key])
        return cls(cfg, ws, bs, name)

    @classmethod
    def load(cls, path, cfg=VGG19_RELU4_4):
        """The stack of ``cfg`` from the state dict file ``path`` (``torch.load(path, weights_only=True)``),
        on the CPU.  The file must exist: it is never downloaded."""
        path = os.fspath(path)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"no VGG weights file {path!r} (the file is never fetched: pass one that is on disk)")
        state = torch.load(path, map_location="cpu", weights_only=True)
        return cls.from_state_dict(state, cfg, os.path.basename(path))

    @classmethod
    def synthetic(cls, cfg=VGG19_RELU4_4, seed=0):
        """Keyed weights for tests and benchmarks, the recipe of :mod:`rrin_amd.synthetic`: for key ``k``
        (``features.N.weight`` / ``.bias``) a generator seeded ``crc32(k) + seed``; weights uniform in
        ``+-sqrt(6 / fan_in)`` (He: the activations keep their scale through the ReLUs), biases uniform
        in ``+-1 / sqrt(fan_in)``, ``fan_in = 9 cin``."""
        ws, bs = [], []
        for idx, cin, cout in conv_layout(cfg):
            fan = 9 * cin
            for kind, shape, bound, dest in (("weight", (cout, cin, 3, 3), math.sqrt(6.0 / fan), ws),
                                             ("bias", (cout,), 1.0 / math.sqrt(fan), bs)):
                g = torch.Generator().manual_seed(zlib.crc32(f"features.{idx}.{kind}".encode()) + int(seed))
                dest.append((torch.rand(shape, generator=g) * 2 - 1) * bound)
        return cls(cfg, ws, bs, "synthetic")

    def features(self, x):
        """``features[:-10](x)`` with PyTorch operators (differentiable through ``x``)."""
        k = 0
        for v in self.cfg:
            if v == "M":
                x = F.max_pool2d(x, 2, 2)
            else:
                x = torch.relu(F.conv2d(x, self.weights[k], self.biases[k], padding=1))
                k += 1
        return x


def _check_shape(key, t, shape):
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or not t.is_floating_point():
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"VGG weights: {key!r} is {got}, expected a float tensor of shape {tuple(shape)}")


def check_frames(out, target, vgg):
    """ValueError unless ``out`` and ``target`` are two ``[N,C,H,W]`` tensors of one shape that the stack takes:
    C the first conv's input channels, H and W multiples of 8."""
    if out.dim() != 4 or out.shape != target.shape:
        raise ValueError(f"perceptual_loss takes two [N,C,H,W] tensors of one shape, got {tuple(out.shape)} / "
                         f"{tuple(target.shape)}")
    n, c, h, w = out.shape
    if n < 1 or c != vgg.layout[0][1]:
        raise ValueError(f"perceptual_loss takes {vgg.layout[0][1]}-channel frames, got {tuple(out.shape)}")
    if h < FRAME_MULTIPLE or w < FRAME_MULTIPLE or h % FRAME_MULTIPLE or w % FRAME_MULTIPLE:
        raise ValueError(f"H and W must be positive multiples of {FRAME_MULTIPLE}, got {h}x{w}")


def perceptual_loss(out, target, vgg):
    """``torch.norm(features(out) - features(target), 2)``: one scalar over the whole batch (the reference's
    ``VggLoss``, losses.py:20-26).  ``out`` and ``target`` are the network's [0,1] RGB ``[N,3,H,W]`` with no
    ImageNet normalisation, exactly as the reference feeds them; H and W are multiples of 8 (ValueError
    otherwise).  The gradient flows to ``out`` only: the target branch runs without autograd.

    Two tie rules fix the gradient where the function has a kink (PyTorch's CPU rules; the HIP kernels
    follow them):

    * max-pool backward sends the gradient to the first maximum of the 2x2 window in row-major order;
    * the norm's gradient is ``d / norm``, and it is 0 where ``norm == 0``.
    """
    check_frames(out, target, vgg)
    with torch.no_grad():
        ft = vgg.features(target.detach())
    return torch.norm(vgg.features(out) - ft, 2)
