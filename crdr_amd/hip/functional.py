"""torch.autograd plumbing around the HIP kernels.

Each Function's forward/backward is one or a few C-ABI launches; torch only owns the graph, the memory and the
stream.  Parameter gradients of conv layers are accumulated by the kernels straight into `param.grad` (so the
trainer can keep all gradients in one flat buffer for a single RCCL all-reduce).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import lib as L
from . import ops, packs

def grad_slot(p: torch.Tensor) -> torch.Tensor:
    if p.grad is None:
        p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
    return p.grad


class ConvSpec:
    """Static description of one conv layer + its two persistent weight packs (forward / input-gradient operand)."""

    def __init__(self, in_ch, out_ch, k, stride, pad, transposed=False, out_pad=0):
        self.in_ch, self.out_ch, self.k = in_ch, out_ch, (k, k) if isinstance(k, int) else tuple(k)
        self.stride, self.pad, self.transposed, self.out_pad = stride, pad, transposed, out_pad
        self._packs = {}
        self.smallc = (not transposed) and in_ch <= 4  # RGB-input convs use the tap-major forward pack
        # ... and so does the input-gradient of an RGB-output ConvTranspose2d (a regular conv that reduces over <= 4 channels)
        self.smallc_dgrad = transposed and out_ch <= 4

    def out_hw(self, h, w):
        return (ops.conv_out_size(h, self.k[0], self.stride, self.pad, self.transposed, self.out_pad),
                ops.conv_out_size(w, self.k[1], self.stride, self.pad, self.transposed, self.out_pad))

    def pack(self, weight: torch.Tensor, for_dgrad: bool) -> torch.Tensor:
        # forward pack has rows = out channels: Conv2d weight [O][I] -> no transpose; ConvT weight [I][O] -> transpose
        transpose = (self.transposed != for_dgrad)
        tapmajor = (self.smallc and not for_dgrad) or (self.smallc_dgrad and for_dgrad)
        return self._pack(weight, transpose, 2 if tapmajor else int(transpose))

    def mark_stale(self) -> None:
        """The weight buffer was rewritten in place by a kernel (spectral norm): refill the packs on next use."""
        for ent in self._packs.values():
            ent.key = None

    def pack_scatter(self, weight: torch.Tensor) -> torch.Tensor:
        """[4 T][first weight dim] pack of an RGB-output transposed op done as GEMM + col2im (crdr_col2im_rgb)."""
        return self._pack(weight, "scatter", 3)

    def _pack(self, weight: torch.Tensor, slot, mode: int) -> torch.Tensor:
        ent = self._packs.get(slot)
        if ent is None or ent.weight.data_ptr() != weight.data_ptr() or ent.weight.shape != weight.shape:
            I, J, r = weight.shape[0], weight.shape[1], ops.round32
            T = weight.shape[2] * weight.shape[3] if weight.dim() == 4 else 1
            shape = {0: (T, r(I), r(J)), 1: (T, r(J), r(I)), 2: (1, r(I), r(4 * T)), 3: (1, r(4 * T), r(I))}[mode]   # (modes: crdr_pack_item)
            ent = self._packs[slot] = packs._PackEntry(weight, torch.empty(shape, dtype=torch.float32, device=weight.device), mode, shape[1], shape[2])
        packs.ensure_fresh((ent,), log=True)
        return ent.dst


def scatter_conv(u: torch.Tensor, weight: torch.Tensor, bias, spec: "ConvSpec", out_hw) -> torch.Tensor:
    """RGB-output transposed op (ConvTranspose2d C -> <=4, or the input gradient of a Conv2d <=4 -> C) as ONE 1x1 GEMM
    with 4 T output columns + a gather, instead of per-tap / per-phase GEMMs padded from 3 to 32 output columns."""
    lib = L.load()
    n, _, h, w = u.shape
    T = spec.k[0] * spec.k[1]
    pk = spec.pack_scatter(weight)
    cols = ops.conv2d_raw(u, pk, 4 * T, (1, 1), 1, 0, False, (h, w))
    c = weight.shape[1]
    out = ops.empty_nhwc(n, c, out_hw[0], out_hw[1], u.device)
    L.check(lib.crdr_col2im_rgb(cols.data_ptr(), 4 * T, n, h, w, spec.k[0], spec.k[1], spec.stride, spec.pad,
                                None if bias is None else bias.data_ptr(), out.data_ptr(), ops.ld_for(c), out_hw[0], out_hw[1], c,
                                ops._stream()), "col2im_rgb")
    return out


def _flags(bias, act, vec2, res, gate, affine) -> int:
    f = 0
    if bias is not None:
        f |= L.EPI_BIAS
    if act == "relu":
        f |= L.EPI_RELU
    elif act == "lrelu":
        f |= L.EPI_LRELU
    elif act is not None:
        raise ValueError(act)
    if vec2 is not None:
        f |= L.EPI_VEC2
    if res is not None:
        f |= L.EPI_RES
    if gate:
        f |= L.EPI_GATE
    if affine:
        f |= L.EPI_AFFINE
    return f


class _FusedConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, vec2, res, scale, shift, gx, gt, spec: ConvSpec, act, return_wgrad=False):
        ctx.return_wgrad = return_wgrad
        flags = _flags(bias, act, vec2, res, gx is not None, scale is not None)
        n, _, h, w = x.shape
        oh, ow = spec.out_hw(h, w)
        sig = ops.empty_nhwc(n, spec.out_ch, oh, ow, x.device) if gx is not None else None
        if spec.transposed and spec.out_ch <= 4 and not (flags & ~L.EPI_BIAS) and spec.k[0] * spec.k[1] > 1:
            out = scatter_conv(x, weight, bias, spec, (oh, ow))
        else:
            out = ops.conv2d_raw(x, spec.pack(weight, False), spec.out_ch, spec.k, spec.stride, spec.pad, spec.transposed,
                                 (oh, ow), bias=bias, flags=flags, vec2=vec2, res=res, scale=scale, shift=shift,
                                 gate_x=gx, gate_t=gt, sig_out=sig, wlayout=1 if spec.smallc else 0)
        ctx.spec, ctx.flags, ctx.in_hw = spec, flags, (h, w)
        if ops.RELU_MASK_SINK is not None and act == "relu" and vec2 is None and res is None and scale is None and gx is None and any(ctx.needs_input_grad):   # (a no-grad pass -- the high-rate reconstruction -- has no backward to take masks for)
            ops.RELU_MASK_SINK(weight, out, None)
        ctx.has = (bias is not None, vec2 is not None, res is not None, scale is not None, gx is not None)
        need_out = flags & (L.EPI_RELU | L.EPI_LRELU | L.EPI_AFFINE)
        ctx.save_for_backward(x, weight, bias, vec2, scale, shift, gt, sig, out if need_out else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, bias, vec2, scale, shift, gt, sig, out = ctx.saved_tensors
        spec, flags = ctx.spec, ctx.flags
        has_bias, has_vec2, has_res, has_aff, has_gate = ctx.has
        needs = ctx.needs_input_grad
        dout, _ = ops.nhwc(dout)
        heavy = flags & (L.EPI_RELU | L.EPI_LRELU | L.EPI_AFFINE | L.EPI_GATE)
        gres = dgt = dscale = dshift = dvec2 = None
        if heavy or has_vec2:
            dz, gres, dgt, cs = ops.epilogue_bwd(dout, out, flags, vec2=vec2, scale=scale, shift=shift, gate_t=gt, sig=sig,
                                                 need_dz=bool(heavy),
                                                 dbias_accum=grad_slot(bias) if (has_bias and needs[2]) else None)
            if dz is None:
                dz = dout
            if has_vec2:
                dvec2 = cs[1]
            if has_aff:
                dscale, dshift = cs[2], cs[3]
        else:
            dz = dout
            if has_bias and needs[2]:
                ops.colsum(dz, grad_slot(bias), accumulate=True)
        if gres is None and (has_res or has_gate):
            gres = dout  # no affine in front: the residual branch sees dout itself
        dx = None
        if needs[0]:
            if (not spec.transposed) and spec.in_ch <= 4 and spec.k[0] * spec.k[1] > 1:
                dx = scatter_conv(dz, weight, None, spec, ctx.in_hw)  # RGB image gradient: one GEMM + gather
            else:
                dx = ops.conv2d_raw(dz, spec.pack(weight, True), x.shape[1], spec.k, spec.stride, spec.pad,
                                    not spec.transposed, ctx.in_hw, wlayout=1 if spec.smallc_dgrad else 0)
        dw = None
        if needs[1]:
            # a parameter's gradient is accumulated straight into its (flat) slot; a derived weight (spectral norm) gets
            # its gradient returned through autograd instead, reduced immediately
            g = torch.empty_like(weight) if ctx.return_wgrad else grad_slot(weight)
            g4 = g if g.dim() == 4 else g.view(g.shape[0], g.shape[1], 1, 1)
            kw = dict(accumulate=not ctx.return_wgrad, defer=not ctx.return_wgrad)
            if spec.transposed:
                ops.conv2d_wgrad_raw(x, dz, g4, spec.k, spec.stride, spec.pad, **kw)
            else:
                ops.conv2d_wgrad_raw(dz, x, g4, spec.k, spec.stride, spec.pad, **kw)
            dw = g if ctx.return_wgrad else None
        return (dx, dw, None, dvec2, gres if has_res else None, dscale, dshift, gres if has_gate else None,
                dgt, None, None, None)


class _SmallLinear(torch.autograd.Function):
    """1x1 conv over <= 16 single-pixel rows (conditioning MLP / projections): GEMV kernels on the raw parameter."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu: bool):
        lib = L.load()
        ops._require_gpu(x)
        m, i, o = x.shape[0], x.shape[1], weight.shape[0]
        x2 = x.reshape(m, i).contiguous()
        y = torch.empty((m, o), dtype=torch.float32, device=x.device)
        L.check(lib.crdr_linear_fwd(x2.data_ptr(), m, i, i, weight.data_ptr(), None if bias is None else bias.data_ptr(),
                                    y.data_ptr(), o, o, int(relu), ops._stream()), "linear_fwd")
        ctx.relu = relu
        ctx.save_for_backward(x2, weight, bias, y if relu else None)
        return y.view(m, o, 1, 1)

    @staticmethod
    def backward(ctx, dy):
        x2, weight, bias, y = ctx.saved_tensors
        lib = L.load()
        m, i, o = x2.shape[0], x2.shape[1], weight.shape[0]
        dy2 = dy.reshape(m, o).contiguous()
        needs = ctx.needs_input_grad
        dx = torch.empty((m, i), dtype=torch.float32, device=dy.device) if needs[0] else None
        dw = grad_slot(weight) if needs[1] else None
        db = grad_slot(bias) if (bias is not None and needs[2]) else None
        L.check(lib.crdr_linear_bwd(x2.data_ptr(), m, i, i, weight.data_ptr(), dy2.data_ptr(), o, None if y is None else y.data_ptr(),
                                    o, o, None if dx is None else dx.data_ptr(), i, None if dw is None else dw.data_ptr(),
                                    None if db is None else db.data_ptr(), ops._stream()), "linear_bwd")
        return (None if dx is None else dx.view(m, i, 1, 1)), None, None, None


class _LinearGroup(torch.autograd.Function):
    """Several linear layers of ONE input (the nine beta projections of a bottleneck stack read the same [1, 512] vector):
    one launch forward, two backward; the input gradient is summed over the layers inside the kernel (fixed order), so
    autograd sees a single consumer of the input.  apply(x, n, w_0 .. w_{n-1}, b_0 .. b_{n-1}) -> n outputs [M, O_g]."""

    @staticmethod
    def forward(ctx, x, n: int, *wb):
        lib = L.load()
        ops._require_gpu(x)
        ws, bs = wb[:n], wb[n:]
        m, i = x.shape[0], x.shape[1]
        x2 = x.reshape(m, i).contiguous()
        g = L.LinearGroup()
        ys = []
        for k in range(n):
            o = ws[k].shape[0]
            assert ws[k].is_contiguous() and ws[k].numel() == o * i
            y = torch.empty((m, o), dtype=torch.float32, device=x.device)
            g.w[k], g.y[k], g.O[k] = ws[k].data_ptr(), y.data_ptr(), o
            g.b[k] = None if bs[k] is None else bs[k].data_ptr()
            ys.append(y)
        L.check(lib.crdr_linear_group_fwd(x2.data_ptr(), m, i, i, C.byref(g), n, ops._stream()), "linear_group_fwd")
        ctx.n = n
        ctx.x_shape = tuple(x.shape)
        ctx.has_b = [b is not None for b in bs]
        ctx.save_for_backward(x2, *ws, *[b for b in bs if b is not None])
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        n = ctx.n
        saved = ctx.saved_tensors
        x2, ws, rest = saved[0], saved[1:1 + n], list(saved[1 + n:])
        lib = L.load()
        m, i = x2.shape
        needs = ctx.needs_input_grad
        g = L.LinearGroup()
        keep = []
        for k in range(n):
            o = ws[k].shape[0]
            dy = dys[k]
            dy = torch.zeros((m, o), dtype=torch.float32, device=x2.device) if dy is None else dy.reshape(m, o).contiguous()
            keep.append(dy)
            b = rest.pop(0) if ctx.has_b[k] else None
            g.w[k], g.dy[k], g.O[k] = ws[k].data_ptr(), dy.data_ptr(), o
            g.dw[k] = grad_slot(ws[k]).data_ptr() if needs[2 + k] else None
            g.db[k] = grad_slot(b).data_ptr() if (b is not None and needs[2 + n + k]) else None
        dx = torch.empty((m, i), dtype=torch.float32, device=x2.device) if needs[0] else None
        L.check(lib.crdr_linear_group_bwd(x2.data_ptr(), m, i, i, C.byref(g), n, None if dx is None else dx.data_ptr(), i,
                                          ops._stream()), "linear_group_bwd")
        return (None if dx is None else dx.view(ctx.x_shape), None) + (None,) * (2 * n)


def linear_group(x, layers):
    """y_g = layer_g(x) for 1x1 conv / linear layers (weight [O, I(, 1, 1)], optional bias) sharing the input x [M <= 16, I(, 1, 1)]:
    one grouped launch per direction.  Returns a list of [M, O_g] tensors."""
    outs = []
    for c0 in range(0, len(layers), L.MAX_GROUP):
        chunk = layers[c0:c0 + L.MAX_GROUP]
        ws = [ly.weight for ly in chunk]  # the parameters themselves ([O, I] or [O, I, 1, 1]): their .grad slots are written
        bs = [ly.bias for ly in chunk]
        outs += list(_LinearGroup.apply(x, len(chunk), *ws, *bs))
    return outs


def fused_conv(x, weight, bias, spec: ConvSpec, *, act: Optional[str] = None, vec2=None, res=None,
               affine: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
               gate: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, return_wgrad: bool = False):
    if (not return_wgrad and spec.k == (1, 1) and spec.stride == 1 and spec.pad == 0 and not spec.transposed and x.dim() == 4 and x.shape[2] == 1
            and x.shape[3] == 1 and x.shape[0] <= 16 and vec2 is None and res is None and affine is None and gate is None
            and act in (None, "relu") and weight.is_contiguous()):
        return _SmallLinear.apply(x, weight, bias, act == "relu")
    scale, shift = affine if affine is not None else (None, None)
    gx, gt = gate if gate is not None else (None, None)
    return _FusedConv.apply(x, weight, bias, vec2, res, scale, shift, gx, gt, spec, act, return_wgrad)


class _SpectralNorm(torch.autograd.Function):
    """weight_orig -> weight_orig / sigma with torch.nn.utils.spectral_norm's semantics (one power iteration per
    training-mode call, u / v updated in place and treated as constants by the backward)."""

    @staticmethod
    def forward(ctx, w_orig, u, v, training: bool, out_buf: torch.Tensor, eps: float):
        lib = L.load()
        ops._require_gpu(w_orig)
        o, k = w_orig.shape[0], w_orig.numel() // w_orig.shape[0]
        sigma = torch.empty(1, dtype=torch.float32, device=w_orig.device)
        ws, wsn = ops.workspace((o + k + 2) * 4, w_orig.device)
        L.check(lib.crdr_spectral_norm_fwd(w_orig.data_ptr(), o, k, u.data_ptr(), v.data_ptr(), int(training), float(eps),
                                           out_buf.data_ptr(), sigma.data_ptr(), ws, wsn, ops._stream()), "spectral_norm_fwd")
        ctx.save_for_backward(w_orig, u.clone() if training else u, v.clone() if training else v, sigma)
        return out_buf.detach()  # a fresh alias of the persistent buffer (stable address for the weight packs)

    @staticmethod
    def backward(ctx, dw_sn):
        w_orig, u, v, sigma = ctx.saved_tensors
        lib = L.load()
        o, k = w_orig.shape[0], w_orig.numel() // w_orig.shape[0]
        g = grad_slot(w_orig)
        nb = lib.crdr_reduce_workspace(o * k) + 16
        ws, wsn = ops.workspace(nb, w_orig.device)
        L.check(lib.crdr_spectral_norm_bwd(dw_sn.contiguous().data_ptr(), w_orig.data_ptr(), u.data_ptr(), v.data_ptr(),
                                           sigma.data_ptr(), o, k, g.data_ptr(), ws, wsn, ops._stream()), "spectral_norm_bwd")
        return None, None, None, None, None, None


def spectral_norm_weight(w_orig, u, v, training: bool, out_buf: torch.Tensor, eps: float = 1e-12):
    return _SpectralNorm.apply(w_orig, u, v, training, out_buf, eps)


class _InterpCaVectors(torch.autograd.Function):
    @staticmethod
    def forward(ctx, W, B, q: float):
        lib = L.load()
        Lv, Cc = W.shape[0], W.shape[2]
        scale = torch.empty(Cc, dtype=torch.float32, device=W.device)
        shift = torch.empty(Cc, dtype=torch.float32, device=W.device)
        L.check(lib.crdr_interp_ca_params(W.data_ptr(), None if B is None else B.data_ptr(), Lv, Cc, float(q),
                                          scale.data_ptr(), shift.data_ptr(), ops._stream()), "interp_ca_params")
        ctx.q, ctx.has_b = float(q), B is not None
        ctx.B = B  # (a parameter: only its .grad slot is touched in backward)
        ctx.save_for_backward(W)
        return scale, shift

    @staticmethod
    def backward(ctx, dscale, dshift):
        (W,) = ctx.saved_tensors
        lib = L.load()
        Lv, Cc = W.shape[0], W.shape[2]
        # the kernel accumulates: leaf parameters get their rows added straight into .grad (the flat gradient buffer), like
        # the bias gradients of the conv layers -- no zero-filled temporary, no autograd add per module
        direct = W.is_leaf and (ctx.B is None or ctx.B.is_leaf)
        if direct:
            dW = grad_slot(W) if ctx.needs_input_grad[0] else None
            dB = grad_slot(ctx.B) if (ctx.has_b and ctx.needs_input_grad[1]) else None
        else:
            dW = torch.zeros_like(W)
            dB = torch.zeros_like(W) if ctx.has_b else None
        if dW is not None or dB is not None:
            scratch = None
            if dW is None:  # (scale frozen, bias trained: the kernel still wants a destination)
                scratch = dW = torch.zeros_like(W)
            L.check(lib.crdr_interp_ca_params_bwd(W.data_ptr(), Lv, Cc, ctx.q, dscale.contiguous().data_ptr(),
                                                  dshift.contiguous().data_ptr(), dW.data_ptr(),
                                                  None if dB is None else dB.data_ptr(), ops._stream()), "interp_ca_params_bwd")
            if scratch is not None:
                dW = None
        if direct:
            return None, None, None
        return dW, dB, None


def interp_ca_vectors(W, B, q: float):
    return _InterpCaVectors.apply(W, B, float(q))


class _Affine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, shift):
        lib = L.load()
        x, ld = ops.nhwc(x)
        n, c, h, w = x.shape
        y = ops.empty_nhwc(n, c, h, w, x.device)
        L.check(lib.crdr_affine(x.data_ptr(), ld, scale.data_ptr(), shift.data_ptr(), y.data_ptr(), ops.ld_for(c), n * h * w, c,
                                ops._stream()), "affine")
        ctx.save_for_backward(y, scale, shift)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, scale, shift = ctx.saved_tensors
        dz, _, _, cs = ops.epilogue_bwd(dy, y, L.EPI_AFFINE, scale=scale, shift=shift)
        return dz, cs[2], cs[3]


def affine(x, scale, shift):
    return _Affine.apply(x, scale, shift)


class _AddAffine(torch.autograd.Function):
    """(a, r, scale?, shift?) -> (a + r) [* scale + shift] in one launch (crdr_add_affine).  Both addends get dy (* scale); the affine's own
    gradients come from crdr_epilogue_bwd on the saved output, as in _Affine."""

    @staticmethod
    def forward(ctx, a, r, scale, shift):
        lib = L.load()
        a, lda = ops.nhwc(a)
        r, ldr = ops.nhwc(r)
        if a.shape != r.shape:
            raise L.CrdrHipError(f"add_affine: operands of shapes {tuple(a.shape)} and {tuple(r.shape)}")
        n, c, h, w = a.shape
        y = ops.empty_nhwc(n, c, h, w, a.device)
        L.check(lib.crdr_add_affine(a.data_ptr(), lda, r.data_ptr(), ldr, ops._p(scale), ops._p(shift), y.data_ptr(), ops.ld_for(c), n * h * w, c,
                                    ops._stream()), "add_affine")
        ctx.save_for_backward(*((y, scale, shift) if scale is not None else ()))
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.saved_tensors:
            return dy, dy, None, None
        y, scale, shift = ctx.saved_tensors
        dz, _, _, cs = ops.epilogue_bwd(dy, y, L.EPI_AFFINE, scale=scale, shift=shift)
        return dz, dz, cs[2], cs[3]


def add_affine(a, r, affine: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """a + r, then the (scale, shift) of an InterpChAtt where one follows"""
    scale, shift = affine if affine is not None else (None, None)
    return _AddAffine.apply(a, r, scale, shift)


class _PixelShuffle(torch.autograd.Function):
    """nn.PixelShuffle(2) on NHWC memory: [N, 4C, H, W] -> [N, C, 2H, 2W] (crdr_pixel_shuffle_fwd / _bwd).  Nothing is saved: the
    backward is the inverse permutation of the cotangent, one launch."""

    @staticmethod
    def forward(ctx, x):
        lib = L.load()
        x, ldx = ops.nhwc(x)
        n, c4, h, w = x.shape
        if c4 % 4 != 0:
            raise L.CrdrHipError(f"pixel_shuffle: {c4} input channels are not a multiple of 4")
        c = c4 // 4
        y = ops.empty_nhwc(n, c, 2 * h, 2 * w, x.device)
        L.check(lib.crdr_pixel_shuffle_fwd(x.data_ptr(), ldx, n, h, w, c, y.data_ptr(), ops.ld_for(c), ops._stream()), "pixel_shuffle_fwd")
        ctx.in_shape = (n, c4, h, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = L.load()
        n, c4, h, w = ctx.in_shape
        dy, lddy = ops.nhwc(dy)
        dx = ops.empty_nhwc(n, c4, h, w, dy.device)
        L.check(lib.crdr_pixel_shuffle_bwd(dy.data_ptr(), lddy, n, h, w, c4 // 4, dx.data_ptr(), c4, ops._stream()), "pixel_shuffle_bwd")
        return dx


def pixel_shuffle(x):
    """F.pixel_shuffle(x, 2) for NHWC tensors; 12 -> 3 channels yields the image layout (pixel stride 4, zero fourth lane)."""
    return _PixelShuffle.apply(x)


UPSAMPLE16_MODES = {"nearest": 0, "bilinear": 1, "bicubic": 2}   # crdr_upsample16_desc.mode


class _Upsample16Cat(torch.autograd.Function):
    """(img [N,3,16h,16w], cond [N,Cc,h,w]) -> torch.cat((img, F.interpolate(cond, scale_factor=16, mode)), dim=1) in dense NHWC memory of
    pixel stride Cc + 4, pad lane zero (crdr_upsample16_cat_fwd / _bwd).  Nothing is saved: the backward is linear in the cotangent.  An
    input that needs no gradient gets a null pointer, and the kernels skip its share of the work."""

    @staticmethod
    def forward(ctx, img, cond, mode: int):
        lib = L.load()
        img, ldi = ops.nhwc(img)
        cond, ldc = ops.nhwc(cond)
        n, cc, h, w = cond.shape
        if tuple(img.shape) != (n, 3, 16 * h, 16 * w):
            raise L.CrdrHipError(f"upsample16_cat: image of shape {tuple(img.shape)} for a condition of shape {tuple(cond.shape)}")
        ldo = ops.ld_for(3 + cc)
        buf = torch.empty((n, 16 * h, 16 * w, ldo), dtype=torch.float32, device=img.device)   # every lane is written, the pad lanes as zeros
        d = L.Upsample16Desc(N=n, h=h, w=w, Cc=cc, ldi=ldi, ldc=ldc, ldo=ldo, mode=mode)
        L.check(lib.crdr_upsample16_cat_fwd(C.byref(d), img.data_ptr(), cond.data_ptr(), buf.data_ptr(), ops._stream()), "upsample16_cat_fwd")
        ctx.geom = (n, cc, h, w, mode)
        return buf.permute(0, 3, 1, 2)[:, :3 + cc]

    @staticmethod
    def backward(ctx, dout):
        lib = L.load()
        n, cc, h, w, mode = ctx.geom
        dout, ldo = ops.nhwc(dout)
        dev = dout.device
        dimg = torch.empty((n, 16 * h, 16 * w, 4), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        dcond = torch.empty((n, h, w, cc), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        d = L.Upsample16Desc(N=n, h=h, w=w, Cc=cc, ldi=4, ldc=cc, ldo=ldo, mode=mode)
        ws, wsn = ops.workspace(lib.crdr_upsample16_cat_workspace(C.byref(d)), dev) if dcond is not None else (None, 0)
        L.check(lib.crdr_upsample16_cat_bwd(C.byref(d), dout.data_ptr(), ops._p(dimg), ops._p(dcond), ws, wsn, ops._stream()), "upsample16_cat_bwd")
        return (None if dimg is None else dimg.permute(0, 3, 1, 2)[:, :3], None if dcond is None else dcond.permute(0, 3, 1, 2), None)


def upsample16_cat(img, cond, mode="bilinear"):
    """torch.cat((img, F.interpolate(cond, scale_factor=16, mode=mode, align_corners=False)), dim=1) for a 3-channel image and a condition
    of Cc % 4 == 0 channels: the NCHW view [:, :3 + Cc] of a dense NHWC buffer, the form HipConv2d takes a channel count that is no
    multiple of 4 in.  `mode` is 'nearest', 'bilinear' or 'bicubic' (or the descriptor's number)."""
    if isinstance(mode, str):
        if mode not in UPSAMPLE16_MODES:
            raise L.CrdrHipError(f"upsample16_cat: mode {mode!r} (one of {sorted(UPSAMPLE16_MODES)})")
        mode = UPSAMPLE16_MODES[mode]
    return _Upsample16Cat.apply(img, cond, int(mode))


class _Lrp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, z):
        lib = L.load()
        a, lda = ops.nhwc(a)
        z, ldz = ops.nhwc(z)
        n, c, h, w = a.shape
        y = ops.empty_nhwc(n, c, h, w, a.device)
        L.check(lib.crdr_lrp(a.data_ptr(), lda, z.data_ptr(), ldz, y.data_ptr(), ops.ld_for(c), n * h * w, c, ops._stream()), "lrp")
        ctx.save_for_backward(z)
        return y

    @staticmethod
    def backward(ctx, dy):
        (z,) = ctx.saved_tensors
        lib = L.load()
        dy, lddy = ops.nhwc(dy)
        z, ldz = ops.nhwc(z)
        n, c, h, w = z.shape
        dz = ops.empty_nhwc(n, c, h, w, z.device)
        L.check(lib.crdr_lrp_bwd(dy.data_ptr(), lddy, z.data_ptr(), ldz, dz.data_ptr(), ops.ld_for(c), n * h * w, c, ops._stream()),
                "lrp_bwd")
        return dy, dz


def lrp(a, z):
    """a + 0.5 * tanh(z)"""
    return _Lrp.apply(a, z)


class _Tanh(torch.autograd.Function):
    """torch.tanh on NHWC memory (crdr_tanh_fwd / _bwd); the output is saved, the backward is dy (1 - y^2).  A 3-channel tensor keeps the
    image layout: pixel stride 4, fourth lane written as zero in both directions."""

    @staticmethod
    def forward(ctx, x):
        lib = L.load()
        x, ldx = ops.nhwc(x)
        n, c, h, w = x.shape
        y = ops.empty_nhwc(n, c, h, w, x.device)
        L.check(lib.crdr_tanh_fwd(x.data_ptr(), ldx, n * h * w, c, y.data_ptr(), ops.ld_for(c), ops._stream()), "tanh_fwd")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        lib = L.load()
        dy, lddy = ops.nhwc(dy)
        n, c, h, w = y.shape
        dx = ops.empty_nhwc(n, c, h, w, y.device)
        L.check(lib.crdr_tanh_bwd(y.data_ptr(), ops.ld_for(c), dy.data_ptr(), lddy, n * h * w, c, dx.data_ptr(), ops.ld_for(c),
                                  ops._stream()), "tanh_bwd")
        return dx


def tanh(x):
    """torch.tanh(x) for NHWC tensors (the Cheng20 decoders' output non-linearity)"""
    return _Tanh.apply(x)


def gauss_cond_fwd2(d, io, device) -> None:
    """crdr_gauss_cond_fwd2 with the scratch for its per-block partial bit sums attached (fixed-order finishing pass)."""
    lib = L.load()
    io.ws, io.ws_bytes = ops.workspace(lib.crdr_gauss_cond_fwd_workspace(C.byref(d)), device)
    L.check(lib.crdr_gauss_cond_fwd2(C.byref(d), C.byref(io), ops._stream()), "gauss_cond_fwd2")


def _gc_operands(y, mu, sigma, noise, ph, bounds):
    """What the forward and the backward of gauss_cond tell the kernels alike: the three operands as ops.nhwc hands them over with their
    pixel strides, N / HW / C, the two bounds and the noise source -- the given samples with their pixel stride, or the (seed, offset) pair
    `ph` the kernel draws them from (the tensor is the whole latent: Ctot = C, c0 = 0; with given samples the two stay at the library's
    defaults).  -> (descriptor, io, (y, mu, sigma, noise) as passed); each direction adds its own fields."""
    y, ldy = ops.nhwc(y)
    mu, ldmu = ops.nhwc(mu)
    sigma, ldsg = ops.nhwc(sigma)
    n, c, h, w = y.shape
    d = L.GcDesc2(N=n, HW=h * w, C=c, ldy=ldy, ldmu=ldmu, ldsigma=ldsg, scale_bound=bounds[0], likelihood_bound=bounds[1])
    io = L.GcIO(y=y.data_ptr(), mu=mu.data_ptr(), sigma=sigma.data_ptr())
    if ph is not None:
        d.Ctot, d.c0, io.philox = c, 0, ph.data_ptr()
    elif noise is not None:
        noise, d.ldnoise = ops.nhwc(noise)
        io.noise = noise.data_ptr()
    return d, io, (y, mu, sigma, noise)


class _GaussCond(torch.autograd.Function):
    """(y, mu, sigma, noise, philox_state) -> (y_hat, bits_noisy[N], bits_quant[N], lik_noisy?, lik_quant?).  `noise` given: those samples.
    Else `philox_state`, the device (seed, offset) pair of the caller's generator, given: the noise is drawn in the kernel; the forward forks
    its own pair off the state (crdr_philox_fork, so a captured graph draws fresh noise at every replay) and the backward regenerates the
    same samples from that pair -- nothing is stored.  Neither: the quantised outputs only, and no backward."""

    @staticmethod
    def forward(ctx, y, mu, sigma, noise, philox_state, scale_bound, lik_bound, want_lik):
        lib = L.load()
        dev = y.device
        ph = None
        if noise is None and philox_state is not None:
            ph = torch.empty(2, dtype=torch.int64, device=dev)
            L.check(lib.crdr_philox_fork(philox_state.data_ptr(), ph.data_ptr(), (y.numel() + 3) // 4 + 1, ops._stream()), "philox_fork")
        d, io, (y, mu, sigma, noise) = _gc_operands(y, mu, sigma, noise, ph, (scale_bound, lik_bound))
        n, c, h, w = y.shape
        src = noise if ph is None else ph
        yhat = ops.empty_nhwc(n, c, h, w, dev)
        bits_n = torch.zeros(n, dtype=torch.float32, device=dev)
        bits_q = torch.zeros(n, dtype=torch.float32, device=dev)
        lik_n = ops.empty_nhwc(n, c, h, w, dev) if (want_lik and src is not None) else None
        lik_q = ops.empty_nhwc(n, c, h, w, dev) if want_lik else None
        d.ldyhat = d.ldlik = ops.ld_for(c)   # the pixel stride of every buffer empty_nhwc made above
        io.yhat, io.lik_noisy, io.lik_quant = yhat.data_ptr(), ops._p(lik_n), ops._p(lik_q)
        io.bits_noisy, io.bits_quant = bits_n.data_ptr(), bits_q.data_ptr()
        gauss_cond_fwd2(d, io, dev)
        ctx.bounds, ctx.in_kernel = (scale_bound, lik_bound), ph is not None
        ctx.save_for_backward(y, mu, sigma, src)   # the samples or the forked pair, never both
        ctx.mark_non_differentiable(bits_q)
        for t in (lik_n, lik_q):
            if t is not None:
                ctx.mark_non_differentiable(t)
        return yhat, bits_n, bits_q, lik_n, lik_q

    @staticmethod
    def backward(ctx, dyhat, dbits_n, _dq, _dln, _dlq):
        y, mu, sigma, src = ctx.saved_tensors
        if src is None:
            raise L.CrdrHipError("gauss_cond: backward needs the noisy (training) forward")
        lib = L.load()
        noise, ph = (None, src) if ctx.in_kernel else (src, None)
        d, io, (y, mu, sigma, noise) = _gc_operands(y, mu, sigma, noise, ph, ctx.bounds)
        n, c, h, w = y.shape
        dev = y.device
        if dbits_n is None:
            dbits_n = torch.zeros(n, dtype=torch.float32, device=dev)
        dbits_n = dbits_n.contiguous()
        if dyhat is not None:
            dyhat, d.lddyhat = ops.nhwc(dyhat)
        dy, dmu, dsg = (ops.empty_nhwc(n, c, h, w, dev) for _ in range(3))
        d.ldgrad = ops.ld_for(c)
        io.gbits, io.dyhat = dbits_n.data_ptr(), ops._p(dyhat)
        io.dy, io.dmu, io.dsigma = dy.data_ptr(), dmu.data_ptr(), dsg.data_ptr()
        L.check(lib.crdr_gauss_cond_bwd2(C.byref(d), C.byref(io), ops._stream()), "gauss_cond_bwd2")
        return dy, dmu, dsg, None, None, None, None, None


def gauss_cond(y, mu, sigma, noise, scale_bound=0.11, lik_bound=1e-9, want_lik=False, philox_state=None):
    """noise given: those samples; noise None and `philox_state` (device int64 [seed, offset]) given: in-kernel Philox noise; both
    None: the quantised (eval) outputs only."""
    return _GaussCond.apply(y, mu, sigma, noise, philox_state, float(scale_bound), float(lik_bound), bool(want_lik))


class _EntropyBottleneck(torch.autograd.Function):
    """(z, params[C,58], medians[C], noise) -> (z_hat, lik, bits[N])"""

    @staticmethod
    def forward(ctx, z, params, medians, noise, lik_bound):
        lib = L.load()
        z = ops.dense_nhwc(z)   # the kernels index element e of channel c at e * C + c: dense rows in, dense rows out
        n, c, h, w = z.shape
        if noise is not None:
            noise = ops.dense_nhwc(noise)
        dev = z.device
        zhat, lik = ops.empty_nhwc(n, c, h, w, dev, ld=c), ops.empty_nhwc(n, c, h, w, dev, ld=c)
        bits = torch.zeros(n, dtype=torch.float32, device=dev)
        params = params.contiguous()
        medians = medians.contiguous()
        L.check(lib.crdr_entropy_bottleneck_fwd(z.data_ptr(), ops._p(noise), params.data_ptr(), medians.data_ptr(), n, h * w,
                                                c, lik_bound, zhat.data_ptr(), lik.data_ptr(), bits.data_ptr(), ops._stream()),
                "entropy_bottleneck_fwd")
        ctx.lik_bound = lik_bound
        ctx.save_for_backward(z, params, noise)
        ctx.mark_non_differentiable(lik)
        return zhat, lik, bits

    @staticmethod
    def backward(ctx, dzhat, _dlik, dbits):
        z, params, noise = ctx.saved_tensors
        if noise is None:
            raise L.CrdrHipError("entropy_bottleneck: backward needs the noisy (training) forward")
        lib = L.load()
        n, c, h, w = z.shape
        dev = z.device
        if dbits is None:
            dbits = torch.zeros(n, dtype=torch.float32, device=dev)
        if dzhat is not None:
            dzhat = ops.dense_nhwc(dzhat)
        dz = ops.empty_nhwc(n, c, h, w, dev, ld=c)
        dparams = torch.empty_like(params)
        L.check(lib.crdr_entropy_bottleneck_bwd(z.data_ptr(), noise.data_ptr(), params.data_ptr(), n, h * w, c, ctx.lik_bound,
                                                dbits.contiguous().data_ptr(), ops._p(dzhat), dz.data_ptr(),
                                                dparams.data_ptr(), ops._stream()), "entropy_bottleneck_bwd")
        # z_hat = ste_round(z - median) + median: no gradient reaches the medians through it
        return dz, dparams, None, None, None


def entropy_bottleneck(z, params, medians, noise, lik_bound=1e-9):
    return _EntropyBottleneck.apply(z, params, medians, noise, float(lik_bound))


# ---------------------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------------------
def _loss_nhwc(t: torch.Tensor) -> torch.Tensor:
    """A [N,C,H,W] loss operand in the library's own layout: NHWC memory whose pixel stride is ld_for(C), padding lanes zero.  A tensor
    that already has that pixel stride is taken as it is -- its padding lanes are the library's (ops.nhwc / ops.empty_nhwc make them
    zero); anything else (NCHW memory, a channel slice of a wider buffer at any offset, a view that does not own its last padding
    lanes) is copied, so that no foreign channel enters the sum."""
    t2, ld = ops.nhwc(t)
    n, c, h, w = t2.shape
    if ld == ops.ld_for(c) and t2.storage_offset() + n * h * w * ld <= t2.untyped_storage().nbytes() // t2.element_size():
        return t2
    buf = ops.empty_nhwc(n, c, h, w, t2.device, zero=True)
    buf.copy_(t2)
    return buf


def _same_layout(a, b):
    """-> (flat a, flat b, geometry): the two operands of a difference as flat contiguous buffers in ONE element order.  Two contiguous
    tensors (1-D, [n,1,1,1], NCHW, ...) of one element count are flattened as they are (geometry None); otherwise both must have one
    shape, and two [N,C,H,W] tensors are both brought to padded NHWC order (_loss_nhwc; geometry (n, c, h, w, ld)), whatever memory
    each one came in.  The decision is made on the layouts, never on the element counts alone."""
    ops._require_gpu(a)
    ops._require_gpu(b)
    if a.is_contiguous() and b.is_contiguous() and a.numel() == b.numel():
        return a.reshape(-1), b.reshape(-1), None
    if a.shape != b.shape:
        raise L.CrdrHipError(f"loss operands of different shapes {tuple(a.shape)} and {tuple(b.shape)}")
    if a.dim() != 4:
        return a.contiguous().reshape(-1), b.contiguous().reshape(-1), None
    a2, b2 = _loss_nhwc(a), _loss_nhwc(b)
    n, c, h, w = a2.shape
    ld = ops.ld_for(c)
    return (torch.as_strided(a2, (n * h * w * ld,), (1,), a2.storage_offset()),
            torch.as_strided(b2, (n * h * w * ld,), (1,), b2.storage_offset()), (n, c, h, w, ld))


def _unflat(flat, shape, geom):
    """A gradient computed on a flat buffer of _same_layout, as a tensor of the operand's shape (NHWC memory when `geom` is set: autograd
    takes a gradient in any strides)."""
    if flat is None:
        return None
    if geom is None:
        return flat.view(shape)
    n, c, h, w, ld = geom
    return flat.view(n, h, w, ld).permute(0, 3, 1, 2)[:, :c]


# public name -> (sum entry, backward entry, takes a target) of the crdr_* ABI
_PAIR_SUMS = {"sqdiff_sum": ("sqdiff_sum", "sqdiff_bwd", False),
              "l1_sum": ("l1_sum", "l1_bwd", False),           # sum |a - b| (nn.L1Loss before its mean); gradient sign(a - b), sign(0) = 0
              "bce_diff_sum": ("bce_diff_sum", "bce_diff_bwd", True)}   # sum BCEWithLogits(a - b, target)


class _PairSum(torch.autograd.Function):
    """(a, b) -> one float: a sum over the elements of a pair, by the _PAIR_SUMS entry `name`."""

    @staticmethod
    def forward(ctx, a, b, name, target):
        lib = L.load()
        entry, _, has_target = _PAIR_SUMS[name]
        if has_target:   # (the older rule: each operand flattened in its own contiguous order)
            fa, fb, ctx.geom = a.contiguous().reshape(-1), b.contiguous().reshape(-1), None
        else:
            fa, fb, ctx.geom = _same_layout(a, b)
        ctx.name, ctx.targs = name, ((target,) if has_target else ())
        out = torch.empty(1, dtype=torch.float32, device=a.device)
        ws, wsn = ops.workspace(lib.crdr_reduce_workspace(fa.numel()), a.device)
        L.check(getattr(lib, "crdr_" + entry)(fa.data_ptr(), fb.data_ptr(), fa.numel(), *ctx.targs, out.data_ptr(), ws, wsn, ops._stream()),
                entry)
        ctx.shapes = (a.shape, b.shape)
        ctx.save_for_backward(fa, fb)   # (views of a, b wherever those already had the common layout)
        return out

    @staticmethod
    def backward(ctx, g):
        fa, fb = ctx.saved_tensors
        lib = L.load()
        entry = _PAIR_SUMS[ctx.name][1]
        da = torch.empty_like(fa) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(fb) if ctx.needs_input_grad[1] else None
        L.check(getattr(lib, "crdr_" + entry)(fa.data_ptr(), fb.data_ptr(), fa.numel(), *ctx.targs, g.contiguous().data_ptr(), 1.0,
                                              ops._p(da), ops._p(db), ops._stream()), entry)
        return _unflat(da, ctx.shapes[0], ctx.geom), _unflat(db, ctx.shapes[1], ctx.geom), None, None


def sqdiff_sum(a, b):
    return _PairSum.apply(a, b, "sqdiff_sum", None)


def l1_sum(a, b):
    return _PairSum.apply(a, b, "l1_sum", None)


def bce_diff_sum(p, q, target: float):
    return _PairSum.apply(p, q, "bce_diff_sum", float(target))


GAN_BCE, GAN_HINGE_D, GAN_HINGE_G = 0, 1, 2   # crdr_gan_loss_desc.kind


class _GanLossSum(torch.autograd.Function):
    """(p, q, mask) -> one float: sum_i mask_i l(p_i - r_i) of crdr_gan_loss_fwd, r = q (paired), mean(q) (centred) or 0 (q is None).
    Operands are flattened like _PairSum's bce_diff_sum: each in its own contiguous order.  The mask gets no gradient."""

    @staticmethod
    def forward(ctx, p, q, mask, kind, target, sgn, center):
        lib = L.load()
        fp = p.contiguous().reshape(-1)
        fq = None if q is None else q.contiguous().reshape(-1)
        fm = None if mask is None else mask.expand_as(p).contiguous().reshape(-1)
        if fq is not None and not center and fq.numel() != fp.numel():
            raise ValueError(f"gan_loss_sum: paired operands of {fp.numel()} and {fq.numel()} elements")
        if center and fq is None:
            raise ValueError("gan_loss_sum: center=True needs q")
        for t in (fp, fq, fm):
            if t is not None and (t.dtype != torch.float32 or t.device != p.device or not t.is_cuda):
                raise ValueError("gan_loss_sum: operands are float32 tensors on one GPU")
        d = L.GanLossDesc(n=fp.numel(), nq=0 if fq is None else fq.numel(), kind=int(kind), center=int(bool(center)),
                          target=float(target), sgn=float(sgn))
        out = torch.empty(1, dtype=torch.float32, device=p.device)
        stats = torch.empty(2, dtype=torch.float32, device=p.device)
        ws, wsn = ops.workspace(lib.crdr_gan_loss_workspace(d.n, d.nq), p.device)
        L.check(lib.crdr_gan_loss_fwd(C.byref(d), fp.data_ptr(), ops._p(fq), ops._p(fm), out.data_ptr(), stats.data_ptr(), ws, wsn,
                                      ops._stream()), "gan_loss_fwd")
        ctx.desc, ctx.has_q, ctx.has_mask = d, fq is not None, fm is not None
        ctx.shapes = (p.shape, None if q is None else q.shape)
        ctx.save_for_backward(fp, stats, *([fq] if fq is not None else []), *([fm] if fm is not None else []))
        return out

    @staticmethod
    def backward(ctx, g):
        lib = L.load()
        fp, stats, *rest = ctx.saved_tensors
        fq = rest.pop(0) if ctx.has_q else None
        fm = rest.pop(0) if ctx.has_mask else None
        d = ctx.desc
        dp = torch.empty_like(fp) if ctx.needs_input_grad[0] else None
        dq = torch.empty_like(fq) if (fq is not None and ctx.needs_input_grad[1]) else None
        ws, wsn = ops.workspace(lib.crdr_gan_loss_workspace(d.n, d.nq), fp.device)
        L.check(lib.crdr_gan_loss_bwd(C.byref(d), fp.data_ptr(), ops._p(fq), ops._p(fm), stats.data_ptr(), g.contiguous().data_ptr(), 1.0,
                                      ops._p(dp), ops._p(dq), ws, wsn, ops._stream()), "gan_loss_bwd")
        return (_unflat(dp, ctx.shapes[0], None), _unflat(dq, ctx.shapes[1], None), None, None, None, None, None)


def gan_loss_sum(p, q=None, *, kind: int, target: float = 0.0, sgn: float = 1.0, center: bool = False, mask=None):
    """sum_i mask_i l(p_i - r_i): kind GAN_BCE (BCEWithLogits against `target`), GAN_HINGE_D (max(1 - sgn x, 0)) or GAN_HINGE_G (-x);
    r = q elementwise, mean(q) with center=True (q of any size), 0 without q.  Gradients flow to p and to q."""
    return _GanLossSum.apply(p, q, mask, int(kind), float(target), float(sgn), bool(center))


class _MaxPool3s2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        lib = L.load()
        x = ops.dense_nhwc(x)
        n, c, h, w = x.shape
        oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        y = ops.empty_nhwc(n, c, oh, ow, x.device, ld=c)   # the kernel takes no stride: dense rows in, dense rows out
        L.check(lib.crdr_maxpool3s2_fwd(x.data_ptr(), y.data_ptr(), n, h, w, c, ops._stream()), "maxpool_fwd")
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        lib = L.load()
        n, c, h, w = x.shape
        dy = ops.dense_nhwc(dy)
        dx = ops.empty_nhwc(n, c, h, w, x.device, ld=c)
        L.check(lib.crdr_maxpool3s2_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), n, h, w, c, ops._stream()), "maxpool_bwd")
        return dx


def maxpool3s2(x):
    return _MaxPool3s2.apply(x)


class _MaxPool2s2(torch.autograd.Function):
    """F.max_pool2d(x, 2, 2) on NHWC memory (crdr_maxpool2s2_fwd / _bwd): channel slices of wider tensors go in as they are.  x is saved;
    the backward recomputes the argmax from it (first maximum in row-major order, torch's rule) and writes every element of dx once."""

    @staticmethod
    def forward(ctx, x):
        lib = L.load()
        x, ldx = ops.nhwc(x)
        n, c, h, w = x.shape
        if c % 4 != 0:
            raise L.CrdrHipError(f"maxpool2s2: {c} channels are not a multiple of 4")
        y = ops.empty_nhwc(n, c, h // 2, w // 2, x.device)
        L.check(lib.crdr_maxpool2s2_fwd(x.data_ptr(), ldx, n, h, w, c, y.data_ptr(), c, ops._stream()), "maxpool2s2_fwd")
        ctx.save_for_backward(x)
        ctx.ldx = ldx
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        lib = L.load()
        n, c, h, w = x.shape
        dy, lddy = ops.nhwc(dy)
        dx = ops.empty_nhwc(n, c, h, w, x.device)
        L.check(lib.crdr_maxpool2s2_bwd(x.data_ptr(), ctx.ldx, dy.data_ptr(), lddy, n, h, w, c, dx.data_ptr(), c, ops._stream()),
                "maxpool2s2_bwd")
        return dx


def maxpool2s2(x):
    """F.max_pool2d(x, 2, 2) for NHWC tensors with C % 4 == 0, H >= 2 and W >= 2; autograd routes as torch does."""
    return _MaxPool2s2.apply(x)


class _LpipsLayer(torch.autograd.Function):
    """(f_real, f_fake, lin[C]) -> per-image distance [N]; gradient flows to f_fake only."""

    @staticmethod
    def forward(ctx, f0, f1, lin):
        lib = L.load()
        f0, f1 = ops.dense_nhwc(f0), ops.dense_nhwc(f1)
        n, c, h, w = f0.shape
        out = torch.zeros(n, dtype=torch.float32, device=f0.device)
        ws, wsn = ops.workspace(n * 64 * 4, f0.device)
        L.check(lib.crdr_lpips_layer_fwd(f0.data_ptr(), f1.data_ptr(), lin.data_ptr(), n, h * w, c, out.data_ptr(), ws, wsn,
                                         ops._stream()), "lpips_layer_fwd")
        ctx.save_for_backward(f0, f1, lin)
        return out

    @staticmethod
    def backward(ctx, g):
        f0, f1, lin = ctx.saved_tensors
        lib = L.load()
        n, c, h, w = f0.shape
        df1 = ops.empty_nhwc(n, c, h, w, f0.device, ld=c)   # dense, like the f0 / f1 the forward saved
        L.check(lib.crdr_lpips_layer_bwd(f0.data_ptr(), f1.data_ptr(), lin.data_ptr(), n, h * w, c, g.contiguous().data_ptr(),
                                         df1.data_ptr(), ops._stream()), "lpips_layer_bwd")
        return None, df1, None


def lpips_layer(f_real, f_fake, lin):
    return _LpipsLayer.apply(f_real, f_fake, lin)
