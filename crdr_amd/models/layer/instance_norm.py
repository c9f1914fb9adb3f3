"""InstanceNorm2D: `nn.InstanceNorm2d` without running statistics (what the reference's rate-aware discriminators build with
`norm_type: IN`, src/models/discriminator/multirate_clic21_gvae_discriminator.py:12-24) on NHWC memory.

    mu, var = moments of x over H x W per (image, channel), var biased ;   z = weight (x - mu) rsqrt(var + eps) + bias ;   y = act(z)

The activation that follows the norm is fused into the apply pass (crdr_instance_norm_fwd / _bwd, csrc/instnorm.hip).  Train and eval are
identical.  With `affine=True` the parameters are `weight` / `bias` of shape [C], torch's keys.  Not on the CRDR hot path: an optional
registered op."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
import torch.nn as nn

from crdr_amd.hip import functional as HF
from crdr_amd.hip import lib as L
from crdr_amd.hip import ops
from crdr_amd.models.layer.hific_norm import _aligned

_ACTS = {None: 0, "relu": 1, "lrelu": 2}


def _desc(n: int, hw: int, c: int, ldx: int, ldy: int, act, slope: float, eps: float) -> "L.InstanceNormDesc":
    if act not in _ACTS:
        raise ValueError(f"InstanceNorm2D: act must be None, 'relu' or 'lrelu' (got {act!r})")
    return L.InstanceNormDesc(HW=hw, N=n, C=c, ldx=ldx, ldy=ldy, act=_ACTS[act], slope=slope, eps=eps)


def _workspace(lib, d, device):
    """(keep-alive tensor, 256-byte aligned address, bytes) of the slab partials"""
    nb = lib.crdr_instance_norm_workspace(C.byref(d))
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=device)
    return ws, (ws.data_ptr() + 255) // 256 * 256, nb


def instance_norm_fwd(x, weight=None, bias=None, *, eps: float = 1e-5, act: Optional[str] = None, slope: float = 0.2, out=None):
    """The forward launches, no autograd.  `x` and `out` may be channel slices of wider NHWC tensors; `out` is written in place.
    Returns (y, stats, x as launched, pixel stride of x); stats holds [n][0][c] = mu, [n][1][c] = rstd for instance_norm_bwd."""
    lib = L.load()
    x, ldx = ops.nhwc(x)
    n, c, h, w = x.shape
    y = ops.empty_nhwc(n, c, h, w, x.device) if out is None else out
    y_l, ldy = ops.nhwc(y)
    if out is not None and y_l.data_ptr() != out.data_ptr():
        raise L.CrdrHipError("instance_norm: `out` must be NHWC memory (a channel slice of an NHWC tensor is fine)")
    stats = torch.empty(2 * n * c, dtype=torch.float32, device=x.device)
    d = _desc(n, h * w, c, ldx, ldy, act, slope, eps)
    ws, p, nb = _workspace(lib, d, x.device)
    L.check(lib.crdr_instance_norm_fwd(C.byref(d), x.data_ptr(), ops._p(weight), ops._p(bias), y.data_ptr(), stats.data_ptr(), p, nb,
                                       ops._stream()), "instance_norm_fwd")
    return y, stats, x, ldx


def instance_norm_bwd(x, ldx, weight, bias, stats, dy, *, eps, act, slope, dweight=None, dbias=None):
    """The backward launches; the parameter gradients are ACCUMULATED into dweight / dbias (either may be None); returns dx."""
    lib = L.load()
    dy, lddy = ops.nhwc(dy)
    n, c, h, w = x.shape
    dx = ops.empty_nhwc(n, c, h, w, x.device)
    d = _desc(n, h * w, c, ldx, ops.ld_for(c), act, slope, eps)
    ws, p, nb = _workspace(lib, d, x.device)
    L.check(lib.crdr_instance_norm_bwd(C.byref(d), x.data_ptr(), ops._p(weight), ops._p(bias), stats.data_ptr(), dy.data_ptr(), lddy,
                                       dx.data_ptr(), ops.ld_for(c), ops._p(dweight), ops._p(dbias), p, nb, ops._stream()), "instance_norm_bwd")
    return dx


class _InstanceNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps: float, act, slope: float):
        y, stats, x, ldx = instance_norm_fwd(x, _aligned(weight), _aligned(bias), eps=eps, act=act, slope=slope)
        ctx.save_for_backward(x, weight, bias, stats)
        ctx.cfg = (ldx, eps, act, slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias, stats = ctx.saved_tensors
        ldx, eps, act, slope = ctx.cfg
        needs = ctx.needs_input_grad
        # (the gradient slots are read and written one float at a time: they need no 16-byte alignment, unlike weight / bias)
        gw = HF.grad_slot(weight) if (weight is not None and needs[1]) else None
        gb = HF.grad_slot(bias) if (bias is not None and needs[2]) else None
        dx = instance_norm_bwd(x, ldx, _aligned(weight), _aligned(bias), stats, dy, eps=eps, act=act, slope=slope, dweight=gw, dbias=gb)
        return dx, None, None, None, None, None


class InstanceNorm2D(nn.Module):
    def __init__(self, num_features: int, eps: float = 1e-5, affine: bool = False):
        super().__init__()
        assert num_features % 4 == 0, "InstanceNorm2D on the HIP path needs a channel count that is a multiple of 4"
        self.num_features, self.eps, self.affine = num_features, float(eps), affine
        if affine:
            self.weight = nn.Parameter(torch.ones(num_features))
            self.bias = nn.Parameter(torch.zeros(num_features))

    def forward(self, x, *, act: Optional[str] = None, slope: float = 0.2):
        weight, bias = (self.weight, self.bias) if self.affine else (None, None)
        return _InstanceNormFn.apply(x, weight, bias, self.eps, act, float(slope))
