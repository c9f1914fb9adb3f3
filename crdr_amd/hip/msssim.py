"""MS-SSIM on the HIP kernels of msssim.hip (pytorch_msssim 1.0.0 `ms_ssim(X, Y, data_range, size_average=True)`, the
library behind src/losses/distortion_loss.py:61-70 and src/utils/img_utils.py:135-162; it is third-party and not
pinned here, see tests/msssim_ref.py for the restated algorithm).

`ms_ssim(x, y, data_range)` takes [N, C <= 4, H, W] fp32 images on the device: NCHW-contiguous tensors (copied once into
padded NHWC) or NHWC views with a pixel stride of 4 (what the decoder emits, taken as they are).  Gradients flow to
whichever of x and y require them; the per-pixel maps the backward needs are kept by the forward (crdr_hip.h)."""
from __future__ import annotations

import torch

from . import lib as L
from . import ops

WIN_SIZE = 11
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MIN_SIDE = (WIN_SIZE - 1) * 2 ** (len(WEIGHTS) - 1)   # 160: the reference asserts min(H, W) > this
QUANT_NONE, QUANT_TRUNC, QUANT_255 = 0, 1, 2


def check_size(h: int, w: int) -> None:
    """pytorch_msssim's assertion, raised on the host before anything is launched."""
    assert min(h, w) > MIN_SIDE, "Image size should be larger than %d due to the 4 downsamplings in ms-ssim" % MIN_SIDE


def _image(t: torch.Tensor) -> torch.Tensor:
    if t.dim() != 4:
        raise L.CrdrHipError(f"ms_ssim: expected [N, C, H, W] images, got {tuple(t.shape)}")
    t, ld = ops.nhwc(t)
    if ld != 4:
        raise L.CrdrHipError(f"ms_ssim: images of at most 4 channels (got {t.shape[1]})")
    return t


class _MsSsim(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, data_range: float, quant: int, keep_maps: bool):
        lib = L.load()
        xs, ys = _image(x), _image(y)
        n, c, h, w = xs.shape
        state = torch.empty(lib.crdr_msssim_workspace(n, h, w, int(keep_maps)) // 4, dtype=torch.float32, device=xs.device)
        out = torch.empty(1, dtype=torch.float32, device=xs.device)
        L.check(lib.crdr_msssim_fwd(xs.data_ptr(), 4, ys.data_ptr(), 4, n, h, w, c, float(data_range), quant, state.data_ptr(),
                                    state.numel() * 4, int(keep_maps), out.data_ptr(), ops._stream()), "msssim_fwd")
        ctx.keep_maps = keep_maps
        ctx.save_for_backward(xs, ys, state)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        xs, ys, state = ctx.saved_tensors
        if not ctx.keep_maps:
            raise L.CrdrHipError("ms_ssim: the forward ran without gradients (grad mode off, or a quantised metric)")
        lib = L.load()
        n, c, h, w = xs.shape
        dx = ops.empty_nhwc(n, c, h, w, xs.device, ld=4) if ctx.needs_input_grad[0] else None
        dy = ops.empty_nhwc(n, c, h, w, xs.device, ld=4) if ctx.needs_input_grad[1] else None
        ws, wsn = ops.workspace(lib.crdr_msssim_workspace(n, h, w, 2), xs.device)
        L.check(lib.crdr_msssim_bwd(xs.data_ptr(), 4, ys.data_ptr(), 4, n, h, w, c, state.data_ptr(), g.reshape(1).contiguous().data_ptr(),
                                    ops._p(dx), 4, ops._p(dy), 4, ws, wsn, ops._stream()), "msssim_bwd")
        return dx, dy, None, None, None


def _ms_ssim(x: torch.Tensor, y: torch.Tensor, data_range: float, quant: int) -> torch.Tensor:
    if x.shape != y.shape:
        raise L.CrdrHipError(f"ms_ssim: shapes differ: {tuple(x.shape)} vs {tuple(y.shape)}")
    check_size(x.shape[-2], x.shape[-1])
    ops._require_gpu(x)
    ops._require_gpu(y)
    keep_maps = quant == QUANT_NONE and torch.is_grad_enabled() and (x.requires_grad or y.requires_grad)
    return _MsSsim.apply(x, y, float(data_range), quant, keep_maps)


def ms_ssim(x: torch.Tensor, y: torch.Tensor, data_range: float, quantize_255: bool = False) -> torch.Tensor:
    """Scalar MS-SSIM of x against y (mean over images and channels).  quantize_255: map both images by
    (v + 1) / 2 * 255 and truncate toward zero on the load (the validation metric's conversion; no gradient)."""
    return _ms_ssim(x, y, data_range, QUANT_255 if quantize_255 else QUANT_NONE)
