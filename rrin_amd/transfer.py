"""Transfer tables of the linear-light synthetic shutter: code value -> light and back, in integers.

A shutter integrates light, not code values.  :mod:`rrin_amd.exposure` therefore takes its weighted mean
through a table ``lin`` of ``maxval + 1`` integers, ``maxval = 2**depth - 1``, ``depth`` in 8..12:

    lin[c] = floor(f(c / maxval) * 2**30 + 0.5)                 (float64)

``f`` is the decoding curve of the material, normalised so that ``f(0) = 0`` and ``f(1) = 1`` (every curve
below is divided by its own value at 1).  RGB code values on the byte paths are full scale after the
project's matrix, so ``c / maxval`` is the signal, and one table per depth serves limited and full range.

The curves (``x`` the signal in [0, 1]):

* ``"srgb"``     IEC 61966-2-1: ``x / 12.92`` for ``x <= 0.04045``, else ``((x + 0.055) / 1.055) ** 2.4``
* ``"bt1886"``   ``x ** 2.4``
* ``"gamma22"``  ``x ** 2.2``
* ``"pq"``       SMPTE ST 2084 EOTF: with ``p = x ** (1 / m2)``, ``(max(p - c1, 0) / (c2 - c3 * p)) ** (1 / m1)``,
  ``m1 = 2610 / 16384``, ``m2 = 2523 / 4096 * 128``, ``c1 = 3424 / 4096``, ``c2 = 2413 / 4096 * 32``,
  ``c3 = 2392 / 4096 * 32``
* ``"hlg"``      the inverse of the ARIB STD-B67 OETF, scene light, no OOTF: ``x * x / 3`` for ``x <= 1/2``,
  else ``(exp((x - c) / a) + b) / 12``, ``a = 0.17883277``, ``b = 1 - 4 a = 0.28466892``,
  ``c = 0.5 - a ln(4 a) = 0.55991073``

A caller may pass its own table instead of a name: any sequence or integer tensor of ``maxval + 1`` values,
non-decreasing, in ``[0, 2**30]`` (:func:`as_table`).

**Encoding** is "nearest in linear light", without floating point:

    thr[c] = (lin[c-1] + lin[c] + 1) // 2          for c in 1..maxval          (:func:`thresholds`)
    enc(v) = the number of c in 1..maxval with thr[c] <= v                     (:func:`encode`)

a right-side ``searchsorted``.  Where the table is strictly increasing around ``c``, ``enc(lin[c]) == c``.
The table is an input of the definition and of the kernels alike: a last-bit difference between two
machines' ``pow`` changes a table entry, never the agreement of the two.

Host only: plain torch and Python.
"""
from __future__ import annotations

import functools
import math

import torch

ONE = 1 << 30          # lin of full scale
DEPTHS = (8, 9, 10, 11, 12)
NAMES = ("srgb", "bt1886", "gamma22", "pq", "hlg")

_PQ_M1, _PQ_M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
_PQ_C1, _PQ_C2, _PQ_C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
_HLG_A, _HLG_B, _HLG_C = 0.17883277, 0.28466892, 0.55991073


def _srgb(x: float) -> float:
    return x / 12.92 if x <= 0.04045 else ((x + 0.055) / 1.055) ** 2.4


def _pq(x: float) -> float:
    p = x ** (1.0 / _PQ_M2)
    return (max(p - _PQ_C1, 0.0) / (_PQ_C2 - _PQ_C3 * p)) ** (1.0 / _PQ_M1)


def _hlg(x: float) -> float:
    return x * x / 3.0 if x <= 0.5 else (math.exp((x - _HLG_C) / _HLG_A) + _HLG_B) / 12.0


CURVES = {"srgb": _srgb, "bt1886": lambda x: x ** 2.4, "gamma22": lambda x: x ** 2.2, "pq": _pq, "hlg": _hlg}


def check_depth(depth) -> int:
    """``depth`` if it is an int in 8..12 (a table of more bits does not fit beside the kernels' other
    use of LDS), else ValueError."""
    if isinstance(depth, bool) or not isinstance(depth, int) or depth not in DEPTHS:
        raise ValueError(f"a transfer table has a depth of 8..12 bits (2**depth entries, held in LDS on the device), "
                         f"got {depth!r}")
    return depth


@functools.lru_cache(maxsize=32)
def _named(name: str, depth: int) -> tuple:
    f = CURVES[name]
    maxval, top = (1 << depth) - 1, f(1.0)
    return tuple(int(math.floor(f(c / maxval) / top * ONE + 0.5)) for c in range(maxval + 1))


def table(name: str, depth: int) -> torch.Tensor:
    """The int64 table ``lin`` ``[maxval + 1]`` of a named curve at ``depth`` 8..12 (module docstring)."""
    depth = check_depth(depth)
    if not isinstance(name, str) or name not in CURVES:
        raise ValueError(f"light must be one of {NAMES} or a table, got {name!r}")
    return torch.tensor(_named(name, depth), dtype=torch.int64)


def as_table(light, depth: int) -> torch.Tensor:
    """A name of :data:`NAMES` or a caller's table -> the validated int64 ``lin`` ``[maxval + 1]``.
    ValueError for an unknown name, a wrong length, a decreasing table, an entry outside ``[0, 2**30]``
    or a depth outside 8..12; TypeError for a table that is not made of integers."""
    depth = check_depth(depth)
    if isinstance(light, str):
        return table(light, depth)
    if light is None or isinstance(light, (bytes, bool, int, float)):
        raise ValueError(f"light must be one of {NAMES} or a table, got {light!r}")
    n = 1 << depth
    if isinstance(light, torch.Tensor):
        if light.dtype.is_floating_point or light.dtype.is_complex or light.dtype == torch.bool:
            raise TypeError(f"a transfer table holds integers, got {light.dtype}")
        if light.dim() != 1 or light.numel() != n:
            raise ValueError(f"a transfer table at depth {depth} has {n} entries, got {tuple(light.shape)}")
        lin = light.detach().cpu()
        lin = (lin.view(torch.int16).to(torch.int64) & 0xFFFF) if lin.dtype == torch.uint16 else lin.to(torch.int64)
    else:
        vals = list(light)
        if len(vals) != n:
            raise ValueError(f"a transfer table at depth {depth} has {n} entries, got {len(vals)}")
        if any(isinstance(v, bool) or not isinstance(v, int) for v in vals):
            raise TypeError("a transfer table holds integers")
        if any(not 0 <= v <= ONE for v in vals):
            raise ValueError("a transfer table's entries lie in [0, 2**30]")
        lin = torch.tensor(vals, dtype=torch.int64)
    if int(lin.min()) < 0 or int(lin.max()) > ONE:
        raise ValueError("a transfer table's entries lie in [0, 2**30]")
    if bool((lin[1:] < lin[:-1]).any()):
        raise ValueError("a transfer table is non-decreasing")
    return lin


def table_key(light, depth: int):
    """What names a validated table in a cache: ``(name, depth)``, a custom table by its bytes."""
    depth = check_depth(depth)
    if isinstance(light, str):
        if light not in CURVES:
            raise ValueError(f"light must be one of {NAMES} or a table, got {light!r}")
        return (light, depth)
    return (as_table(light, depth).numpy().tobytes(), depth)


def thresholds(lin: torch.Tensor) -> torch.Tensor:
    """``thr`` ``[maxval + 1]`` int64 of a table: ``thr[c] = (lin[c-1] + lin[c] + 1) // 2``; ``thr[0]`` is unused
    and stored as 0."""
    lin = lin.to(torch.int64)
    thr = torch.zeros_like(lin)
    thr[1:] = (lin[:-1] + lin[1:] + 1) // 2
    return thr


def encode(thr: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """``enc(v)`` per element of the integer tensor ``v``: the number of ``c`` in ``1..maxval`` with ``thr[c] <=
    v``, int64.  Written as the device computes it, a binary search of ``depth`` steps over the
    non-decreasing ``thr``: ``pos + step`` never passes ``maxval``."""
    n = thr.numel()
    if n < 2 or n & (n - 1):
        raise ValueError(f"thr has 2**depth entries, got {n}")
    thr = thr.to(torch.int64)
    v = v.to(torch.int64)
    pos = torch.zeros_like(v)
    step = n >> 1
    while step:
        pos = pos + (thr[pos + step] <= v).to(torch.int64) * step
        step >>= 1
    return pos


def device_words(lin: torch.Tensor) -> torch.Tensor:
    """The int32 ``[2 * (maxval + 1)]`` that the library takes: ``lin``, then ``thr`` (host tensor)."""
    return torch.cat((lin, thresholds(lin))).to(torch.int32)
