"""The residual blocks of the Cheng20 transforms (src/models/layer/cheng_resblock.py:20-107) with the reference's
constructor arguments, defaults and state-dict keys (`conv1`, `conv2`, `actv2.*`, `shortcut` / `c1.{0,3,4}`, `shortcut.0`).

What runs where (all exact -- LeakyReLU commutes with the pixel-shuffle permutation):
  * conv1 carries its activation in the conv epilogue; in UpResBlock it sits in front of the shuffle;
  * actv2 in lrelu / relu / None: conv2 carries the activation; the shortcut and a following InterpChAtt (`affine`) are ONE launch behind it
    (functional.add_affine).  The conv epilogue has LRELU, RES and AFFINE in the block's order, but its backward refuses an activation
    with RES / AFFINE behind it: the activation's mask cannot be recovered from the saved output;
  * actv2 in gdn / igdn: conv2 is a plain conv and the block ends in GDN(conv2, res=shortcut), one launch (crdr_gdn_res_fwd); a following
    `affine` is then the stand-alone functional.affine."""
from __future__ import annotations

from typing import Optional

import torch.nn as nn

from crdr_amd.hip import functional as HF

from .gdn import GDN
from .hip_layers import HipConv2d

_CONV_ACTS = ("relu", "lrelu")
_GDN_ACTS = ("gdn", "igdn")


def _check_actv(actv: Optional[str], actv2: Optional[str]) -> None:
    if actv is not None and actv not in _CONV_ACTS:
        raise NotImplementedError(f"actv={actv!r}: the first activation is a conv epilogue, one of {_CONV_ACTS} or None")
    if actv2 is not None and actv2 not in _CONV_ACTS + _GDN_ACTS:
        raise KeyError(actv2)


def _refuse_padding_mode(padding_mode: str) -> None:
    if padding_mode != "zeros":
        raise NotImplementedError(f"padding_mode={padding_mode!r}: the HIP convs pad with zeros only")


def _tail(conv2: HipConv2d, gdn: Optional[GDN], actv2: Optional[str], y, shortcut, affine):
    """What both blocks end in: conv2, the second activation, the shortcut, the InterpChAtt that may follow"""
    if gdn is None:
        return HF.add_affine(conv2(y, act=actv2), shortcut, affine)
    out = gdn(conv2(y), res=shortcut)
    return out if affine is None else HF.affine(out, affine[0], affine[1])


class ResBlock(nn.Module):
    def __init__(self, in_channel: int, out_channel: int, bn: bool = False, actv: Optional[str] = "relu", actv2: Optional[str] = None,
                 downscale: bool = False, kernel_size: int = 3, padding_mode: str = "zeros"):
        super().__init__()
        if bn:
            raise NotImplementedError("bn=True: BatchNorm2d has no HIP kernel here (no shipped Cheng20 transform uses it)")
        _refuse_padding_mode(padding_mode)
        _check_actv(actv, actv2)
        stride = 2 if downscale else 1
        pad = (kernel_size - 1) // 2
        self.conv1 = HipConv2d(in_channel, out_channel, kernel_size, stride=stride, padding=pad)
        self.conv2 = HipConv2d(out_channel, out_channel, kernel_size, stride=1, padding=pad)
        self.actv, self.actv2_name, self.bn = actv, actv2, False
        self.actv2 = GDN(out_channel, inverse=(actv2 == "igdn")) if actv2 in _GDN_ACTS else None
        # cheng_resblock.py:44-47: a 1x1 conv of the block's stride wherever the shapes differ
        self.shortcut = HipConv2d(in_channel, out_channel, 1, stride=stride) if (downscale or in_channel != out_channel) else None

    def forward(self, x, affine=None):
        shortcut = x if self.shortcut is None else self.shortcut(x)
        y = self.conv1(x, act=self.actv)
        return _tail(self.conv2, self.actv2, self.actv2_name, y, shortcut, affine)


class _Slots(nn.Module):
    """Children under the reference's nn.Sequential indices (the parameter-free entries in between are not modules here)"""

    def __init__(self, **children):
        super().__init__()
        for idx, m in children.items():
            if m is not None:
                self.add_module(idx.lstrip("_"), m)


class UpResBlock(nn.Module):
    def __init__(self, in_channel: int, out_channel: int, kernel_size: int = 3, actv: Optional[str] = "relu", actv2: Optional[str] = None,
                 up_type: str = "pixelshuffle", padding_mode: str = "zeros"):
        super().__init__()
        if up_type == "interpolate":
            raise NotImplementedError("up_type='interpolate': nearest up-sampling has no HIP kernel here; the transforms use 'pixelshuffle'")
        if up_type != "pixelshuffle":
            raise ValueError(f"Invalid up_mode: {up_type}")
        _refuse_padding_mode(padding_mode)
        _check_actv(actv, actv2)
        pad = (kernel_size - 1) // 2
        # c1 = [conv -> 4 out, PixelShuffle(2), actv, conv, actv2 or Identity]; shortcut = [1x1 conv -> 4 out, PixelShuffle(2)]
        self.c1 = _Slots(_0=HipConv2d(in_channel, out_channel * 4, kernel_size, padding=pad),
                         _3=HipConv2d(out_channel, out_channel, kernel_size, padding=pad),
                         _4=GDN(out_channel, inverse=(actv2 == "igdn")) if actv2 in _GDN_ACTS else None)
        self.shortcut = _Slots(_0=HipConv2d(in_channel, out_channel * 4, 1))
        self.actv, self.actv2_name = actv, actv2

    def forward(self, x, affine=None):
        shortcut = HF.pixel_shuffle(getattr(self.shortcut, "0")(x))
        y = HF.pixel_shuffle(getattr(self.c1, "0")(x, act=self.actv))   # the activation in front of the permutation: the same values
        return _tail(getattr(self.c1, "3"), getattr(self.c1, "4", None), self.actv2_name, y, shortcut, affine)
