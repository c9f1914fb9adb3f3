"""ChannelNorm2D with the parameters and state-dict keys of the reference's (src/models/layer/hific_norm.py:18-59: per-pixel
moments over the channel axis, unbiased variance as `torch.var` gives it, eps 1e-3, `gamma` / `beta` of shape (1, C, 1, 1)), and
NHWC reflection padding (`nn.ReflectionPad2d`, src/models/subnet/autoencoder/hific_autoencoder.py:57-59,148,219-221).

    z = gamma (x - mu) rsqrt(var + eps) + beta ;   y = act(z)   or   y = z + res

The activation that follows the norm in the HiFiC transforms and in the CN discriminator, or the residual block's `res + identity`, is
fused into the one pass over the tensor (crdr_channel_norm_fwd / _bwd, csrc/chnorm.hip).  Train and eval are identical: there are no
running statistics.  Not on the CRDR hot path: optional registered ops."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch
import torch.nn as nn

from crdr_amd.hip import functional as HF
from crdr_amd.hip import lib as L
from crdr_amd.hip import ops

_ACTS = {None: 0, "relu": 1, "lrelu": 2}


def _desc(m: int, c: int, ldx: int, ldy: int, ldres: int, act, slope: float, eps: float) -> "L.ChannelNormDesc":
    if act not in _ACTS:
        raise ValueError(f"ChannelNorm2D: act must be None, 'relu' or 'lrelu' (got {act!r})")
    return L.ChannelNormDesc(M=m, C=c, ldx=ldx, ldy=ldy, ldres=ldres, act=_ACTS[act], slope=slope, eps=eps)


def channel_norm_fwd(x, gamma, beta, *, eps: float = 1e-3, act: Optional[str] = None, slope: float = 0.2, res=None, out=None):
    """One forward launch, no autograd.  `x`, `res` and `out` may be channel slices of wider NHWC tensors; `out` is written in place.
    Returns (y, stats, x as launched, pixel stride of x); stats holds (mu, rstd) per pixel for channel_norm_bwd."""
    lib = L.load()
    x, ldx = ops.nhwc(x)
    n, c, h, w = x.shape
    y = ops.empty_nhwc(n, c, h, w, x.device) if out is None else out
    y_l, ldy = ops.nhwc(y)
    if out is not None and y_l.data_ptr() != out.data_ptr():
        raise L.CrdrHipError("channel_norm: `out` must be NHWC memory (a channel slice of an NHWC tensor is fine)")
    ldres = 0
    if res is not None:
        res, ldres = ops.nhwc(res)
    stats = torch.empty(2 * n * h * w, dtype=torch.float32, device=x.device)
    d = _desc(n * h * w, c, ldx, ldy, ldres, act, slope, eps)
    L.check(lib.crdr_channel_norm_fwd(C.byref(d), x.data_ptr(), ops._p(gamma), ops._p(beta), ops._p(res), y.data_ptr(), stats.data_ptr(),
                                      ops._stream()), "channel_norm_fwd")
    return y, stats, x, ldx


def channel_norm_bwd(x, ldx, gamma, beta, stats, dy, *, eps, act, slope, dgamma=None, dbeta=None):
    """One backward launch (+ the finish launch of the parameter gradients, which are ACCUMULATED into dgamma / dbeta); returns dx."""
    lib = L.load()
    dy, lddy = ops.nhwc(dy)
    n, c, h, w = x.shape
    dx = ops.empty_nhwc(n, c, h, w, x.device)
    d = _desc(n * h * w, c, ldx, ops.ld_for(c), 0, act, slope, eps)
    nb = p = 0
    if dgamma is not None or dbeta is not None:
        nb = lib.crdr_channel_norm_workspace(C.byref(d))
        ws = torch.empty(nb + 256, dtype=torch.uint8, device=x.device)
        p = (ws.data_ptr() + 255) // 256 * 256
    L.check(lib.crdr_channel_norm_bwd(C.byref(d), x.data_ptr(), ops._p(gamma), ops._p(beta), stats.data_ptr(), dy.data_ptr(), lddy,
                                      dx.data_ptr(), ops.ld_for(c), ops._p(dgamma), ops._p(dbeta), p, nb, ops._stream()), "channel_norm_bwd")
    return dx


def _aligned(t):
    """`t`, or a copy of it where `t` does not start on a 16-byte boundary: a parameter that an optimiser laid out in its flat buffer
    behind one with an odd element count (the RGB bias of a decoder's last conv) -- the kernels load gamma / beta four at a time"""
    return t if t is None or t.data_ptr() % 16 == 0 else t.detach().clone()


class _ChannelNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, res, eps: float, act, slope: float):
        y, stats, x, ldx = channel_norm_fwd(x, _aligned(gamma), _aligned(beta), eps=eps, act=act, slope=slope, res=res)
        ctx.save_for_backward(x, gamma, beta, stats)
        ctx.cfg = (ldx, eps, act, slope, res is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, stats = ctx.saved_tensors
        ldx, eps, act, slope, has_res = ctx.cfg
        needs = ctx.needs_input_grad
        gg = HF.grad_slot(gamma) if (gamma is not None and needs[1]) else None
        gb = HF.grad_slot(beta) if (beta is not None and needs[2]) else None
        # (a gradient slot off the 16-byte grid -- see _aligned -- is accumulated into through a zeroed, aligned stand-in)
        sg, sb = (None if g is None or g.data_ptr() % 16 == 0 else torch.zeros(g.shape, dtype=g.dtype, device=g.device) for g in (gg, gb))
        dx = channel_norm_bwd(x, ldx, _aligned(gamma), _aligned(beta), stats, dy, eps=eps, act=act, slope=slope,
                              dgamma=gg if sg is None else sg, dbeta=gb if sb is None else sb)
        for slot, stand_in in ((gg, sg), (gb, sb)):
            if stand_in is not None:
                slot.add_(stand_in)
        return dx, None, None, (dy if has_res else None), None, None, None


class ChannelNorm2D(nn.Module):
    def __init__(self, input_channels: int, momentum: float = 0.1, eps: float = 1e-3, affine: bool = True, **kwargs):
        super().__init__()
        assert input_channels % 4 == 0, "ChannelNorm2D on the HIP path needs a channel count that is a multiple of 4"
        self.momentum, self.eps, self.affine = momentum, float(eps), affine
        if affine:
            self.gamma = nn.Parameter(torch.ones(1, input_channels, 1, 1))
            self.beta = nn.Parameter(torch.zeros(1, input_channels, 1, 1))

    def forward(self, x, *, act: Optional[str] = None, slope: float = 0.2, res=None):
        gamma, beta = (self.gamma, self.beta) if self.affine else (None, None)
        return _ChannelNormFn.apply(x, gamma, beta, res, self.eps, act, float(slope))


def ChannelNorm2D_wrap(input_channels, momentum=0.1, affine=True, track_running_stats=False, **kwargs):
    return ChannelNorm2D(input_channels, momentum=momentum, affine=affine, track_running_stats=track_running_stats)


def _pad_launch(fn, what: str, src, n, h, w, c, pad: Tuple[int, int, int, int], dst):
    src, lds = ops.nhwc(src)
    _, ldd = ops.nhwc(dst)
    l, r, t, b = pad
    L.check(fn(src.data_ptr(), n, h, w, c, lds, l, r, t, b, dst.data_ptr(), ldd, ops._stream()), what)
    return dst


class _ReflectPadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pad):
        n, c, h, w = x.shape
        l, r, t, b = pad
        ctx.cfg = (n, c, h, w, pad)
        y = ops.empty_nhwc(n, c, h + t + b, w + l + r, x.device)
        return _pad_launch(L.load().crdr_reflect_pad_fwd, "reflect_pad_fwd", x, n, h, w, c, pad, y)

    @staticmethod
    def backward(ctx, dy):
        n, c, h, w, pad = ctx.cfg
        dx = ops.empty_nhwc(n, c, h, w, dy.device)
        return _pad_launch(L.load().crdr_reflect_pad_bwd, "reflect_pad_bwd", dy, n, h, w, c, pad, dx), None


def reflect_pad(x, pad: Tuple[int, int, int, int]):
    """`F.pad(x, (l, r, t, b), mode="reflect")` on NHWC memory (never leaves the layout)."""
    pad = tuple(int(v) for v in pad)
    assert len(pad) == 4, "reflect_pad takes (left, right, top, bottom)"
    return _ReflectPadFn.apply(x, pad)
