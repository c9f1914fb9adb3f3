"""Hand-scheduled forward / backward of conv chains (residual bottleneck stacks, NLAM branches, discriminator trunks).

The reference builds these from nn.Sequential pieces (src/models/layer/elic_layers.py:23-53, cheng_nlam.py:31-46,
elic_interpca_beta_cond_autoencoder.py:42-84, clic21_gvae_discriminator.py:12-50) and lets autograd walk them op by op.
Here a *chain* -- a list of units, each a list of conv layers with an optional residual from the unit's input to its
output -- is ONE autograd node whose backward is written out:

 * the ReLU / LeakyReLU backward of layer l rides in the epilogue of the input-gradient conv of layer l+1
   (CRDR_EPI_RELUMASK / LRELUMASK on the saved activation, CRDR_EPI_MASKOFF when a beta vector was added after the ReLU),
   so no elementwise pass re-reads the activation and its gradient;
 * bias and beta-vector gradients are column sums produced by the same epilogue (CRDR_EPI_COLSUM) and finished by one
   batched launch per chain (ops.ColsumQueue);
 * the residual gradient is the RES operand of the unit's first input-gradient conv: no separate accumulation kernel;
 * G parallel chains of one geometry (the trunk and attention branches of an NLAM) run as grouped launches.
The forward issues exactly the launches the per-layer path issued (same kernels, same packs), so values are unchanged."""
from __future__ import annotations

import itertools
from typing import List, Sequence

import torch

from . import functional as HF
from . import lib as L
from . import ops
from .ops import V


class Layer:
    """One conv of a chain: `conv` is a HipConv2d / HipConvTranspose2d (weight, bias, spec); act in (None, 'relu', 'lrelu');
    vec_index: index into the chain's beta vectors added AFTER the activation (or None)."""
    __slots__ = ("conv", "act", "vec_index")

    def __init__(self, conv, act=None, vec_index=None):
        self.conv, self.act, self.vec_index = conv, act, vec_index


class Unit:
    __slots__ = ("layers", "residual")

    def __init__(self, layers: Sequence[Layer], residual: bool):
        self.layers, self.residual = list(layers), residual


_chain_sites = itertools.count()


class ChainSpec:
    """Static description: `groups` parallel chains (lists of units) of identical geometry; `affine` = the last conv of
    group 0's last unit carries a per-channel scale + shift epilogue (InterpChAtt); nvec = number of beta vectors."""

    def __init__(self, groups: Sequence[Sequence[Unit]], affine: bool = False, nvec: int = 0, name: str = "chain"):
        self.groups = [list(g) for g in groups]
        self.G = len(self.groups)
        self.U = len(self.groups[0])
        assert all(len(g) == self.U for g in self.groups)
        self.affine, self.nvec, self.name = affine, nvec, name
        assert not (affine and self.G > 1)
        self._dv = None
        # the flush site of this chain's column sums: never reused, unlike id(self) -- the tables of a site that a HIP graph captured stay
        # frozen (hip/batched.py), and a later chain must not inherit those of a dead one
        self.site = ("chain", next(_chain_sites))

    def unit(self, g, u) -> Unit:
        return self.groups[g][u]

    def layers(self, u, li) -> List[Layer]:
        """layer li of unit u in each of the G chains"""
        return [grp[u].layers[li] for grp in self.groups]

    def parameters(self):
        out = []
        for grp in self.groups:
            for un in grp:
                for lay in un.layers:
                    out.append(lay.conv.weight)
                    if lay.conv.bias is not None:
                        out.append(lay.conv.bias)
        return out

    def dv_buffers(self, sizes, device):
        """persistent gradient buffers of the beta vectors (stable addresses for the column-sum job tables)"""
        if self._dv is None or [t.numel() for t in self._dv[1]] != list(sizes) or self._dv[0].device != device:
            flat = torch.zeros(sum((s + 3) // 4 * 4 for s in sizes), dtype=torch.float32, device=device)
            vs, off = [], 0
            for s in sizes:
                vs.append(flat[off:off + s])
                off += (s + 3) // 4 * 4
            self._dv = (flat, vs)
        return self._dv


def _flags(act):
    return L.EPI_RELU if act == "relu" else L.EPI_LRELU if act == "lrelu" else 0


class Acts:
    """One tensor of each of the G parallel chains -- a layer's outputs, or their gradients -- in fresh dense [M][c'] buffers of one pixel
    stride (c' = c rounded up to 4, padding lanes zeroed)."""
    __slots__ = ("bufs", "cp", "c", "n", "h", "w")

    def __init__(self, g, n, h, w, c, device):
        self.cp, self.c, self.n, self.h, self.w = (c + 3) // 4 * 4, c, n, h, w
        mk = torch.zeros if self.cp != c else torch.empty
        self.bufs = [mk((n * h * w, self.cp), dtype=torch.float32, device=device) for _ in range(g)]

    def vs(self) -> List[V]:
        return [V(b.data_ptr(), self.cp, self.c) for b in self.bufs]

    def nchw(self) -> List[torch.Tensor]:
        return [b.view(self.n, self.h, self.w, self.cp).permute(0, 3, 1, 2)[:, :self.c] for b in self.bufs]


# A forward pass kept for a SECOND backward (round 6).  The stage-3 step evaluates the discriminator on the reconstruction twice with unchanged
# weights: in the generator phase (D frozen, the adversarial term's gradient flows to the image) and in the discriminator phase (image detached,
# the gradient flows to D's weights) -- the reference even does it three times (multirate_hr_rgan_beta_cond_rate_distortion_trainer.py:52, 92,
# 98).  Same input, same weights, same launches: the activations of the first pass ARE those of the second.  With KEEP_HANDLES a list, every
# chain forward appends a handle (spec, saved activations, geometry, input); run_chain_reuse(handle) is then an autograd node whose
# forward launches nothing and whose backward is _ChainFn.backward on the kept activations.
KEEP_HANDLES = None


class ChainHandle:
    __slots__ = ("spec", "saved", "geom", "x")

    def __init__(self, spec, saved, geom, x):
        self.spec, self.saved, self.geom, self.x = spec, saved, geom, x


class _KeptCtx:
    """what _ChainFn.backward reads of its ctx, for a backward on kept activations: the chain input counts as detached
    (needs_input_grad[0]), there are no beta vectors ([5 + i])"""
    needs_input_grad = (False,) * 8

    def __init__(self, ctx):
        self.spec, self.saved_acts, self.geom, self.nrest, self.saved_tensors = ctx.spec, ctx.saved_acts, ctx.geom, ctx.nrest, ctx.saved_tensors


def _bias_slot(cv):
    return HF.grad_slot(cv.bias) if (cv.bias is not None and cv.bias.requires_grad) else None


def _colsum_targets(layers: Sequence[Layer], dvs):
    """Where the column sums of the gradient of `layers`' outputs go, per chain: (address for the pre-mask sum = the beta vector added
    after the activation, address for the post-mask sum = the bias)"""
    slots = [_bias_slot(b.conv) for b in layers]
    return [(None if b.vec_index is None else dvs[b.vec_index].data_ptr(), None if s is None else s.data_ptr()) for b, s in zip(layers, slots)]


def _layer_input(saved, xin, u, li):
    """What layer li of unit u read, as (Vs, (h, w), channels): the layer below it, the previous unit's output, or the chain input `xin`"""
    if u == 0 and li == 0:
        return xin
    a = saved[u][li - 1] if li else saved[u - 1][-1]
    return a.vs(), (a.h, a.w), a.c


def _output_grad(spec: ChainSpec, out: Acts, douts, scale, shift, dvs, device):
    """The gradient at the chain output(s) -> (Vs, tensors, d scale, d shift), with the bias / beta-vector gradients of the last layers taken.
    An affine epilogue on the last conv (InterpChAtt) is undone by the fused elementwise pass, which also yields d scale / d shift and the
    column sums of the pre-affine gradient."""
    last = spec.layers(spec.U - 1, -1)
    if spec.affine:
        lay = last[0]
        _, gres, _, cs = ops.epilogue_bwd(douts[0], out.nchw()[0], L.EPI_AFFINE | L.EPI_RES, scale=scale, shift=shift, need_dz=False,
                                         dbias_accum=_bias_slot(lay.conv))
        gres, ldg = ops.nhwc(gres)
        if lay.vec_index is not None:
            dvs[lay.vec_index].add_(cs[0])
        return [V(gres.data_ptr(), ldg, out.c)], [gres], cs[2], cs[3]
    ts = [d if d is not None else torch.zeros_like(o) for d, o in zip(douts, out.nchw())]
    pairs = [ops.nhwc(t) for t in ts]
    if len({ld for _, ld in pairs}) > 1:   # a grouped launch needs one pixel stride: repack densely
        dense = Acts(spec.G, out.n, out.h, out.w, out.c, device)
        dz_v, dz_t = dense.vs(), dense.nchw()
        for d, t in zip(dz_t, ts):
            d.copy_(t)
    else:
        dz_t = [t for t, _ in pairs]
        dz_v = [V(t.data_ptr(), ld, out.c) for t, ld in pairs]
    for lay, t in zip(last, dz_t):   # bias / beta-vector gradient of the chain's last layer: a plain column sum
        tgt = _bias_slot(lay.conv)
        if tgt is not None:
            ops.colsum(t, tgt, accumulate=True)
        if lay.vec_index is not None:
            ops.colsum(t, dvs[lay.vec_index], accumulate=True)
    return dz_v, dz_t, None, None


class _ChainFn(torch.autograd.Function):
    """(x, spec, scale, shift, nvec, *vecs, *params) -> tuple of G outputs (NCHW views).  The parameters are passed only so
    that autograd sees the node as differentiable when x is detached (discriminator phase); their gradients are
    accumulated straight into the (flat) .grad slots by the kernels, the node returns None for them."""

    @staticmethod
    def forward(ctx, x, spec: ChainSpec, scale, shift, nvec, *rest):
        vecs = rest[:nvec]
        ctx.nrest = len(rest)
        x, ldx = ops.nhwc(x)
        n, c, h, w = x.shape
        dev = x.device
        G = spec.G
        cur, cur_hw = [V(x.data_ptr(), ldx, c)] * G, (h, w)
        saved = []   # per unit: the Acts of every layer's output
        for u in range(spec.U):
            unit_in = cur
            acts = []
            nl = len(spec.unit(0, u).layers)
            for li in range(nl):
                lay0 = spec.unit(0, u).layers[li]
                convs = [lay.conv for lay in spec.layers(u, li)]
                sp = convs[0].spec
                ih, iw = cur_hw
                oh, ow = sp.out_hw(ih, iw)
                out = Acts(G, n, oh, ow, sp.out_ch, dev)
                ys = out.vs()
                last = li == nl - 1
                ress = unit_in if (last and spec.unit(0, u).residual) else None
                aff = spec.affine and last and u == spec.U - 1
                packs = [cv.spec.pack(cv.weight, False) for cv in convs]
                ops.conv_multi(n, ih, iw, oh, ow, cur, [pk.data_ptr() for pk in packs], ys, sp.out_ch, sp.k, sp.stride, sp.pad,
                               sp.transposed, wrows=packs[0].shape[1], wcols=packs[0].shape[2],
                               biases=[cv.bias.data_ptr() for cv in convs] if convs[0].bias is not None else None,
                               ress=ress, vec2=None if lay0.vec_index is None else vecs[lay0.vec_index].data_ptr(),
                               scale=scale.data_ptr() if aff else None, shift=shift.data_ptr() if aff else None,
                               flags=_flags(lay0.act) | (L.EPI_VEC2 if lay0.vec_index is not None else 0),
                               wlayout=1 if sp.smallc else 0, device=dev, label=spec.name)
                acts.append(out)
                if ops.RELU_MASK_SINK is not None and lay0.act == "relu" and any(ctx.needs_input_grad):   # (a no-grad pass -- the high-rate reconstruction -- has no backward to take masks for)
                    for cv, t in zip(convs, out.nchw()):   # (test hook: the activations this node's backward takes its ReLU masks from)
                        ops.RELU_MASK_SINK(cv.weight, t, None if lay0.vec_index is None else vecs[lay0.vec_index])
                cur, cur_hw = ys, (oh, ow)
            saved.append(acts)
        ctx.spec, ctx.saved_acts, ctx.geom = spec, saved, (n, c, h, w, ldx)
        ctx.save_for_backward(x, scale, shift, *vecs)
        if KEEP_HANDLES is not None and not vecs and scale is None:
            KEEP_HANDLES.append(ChainHandle(spec, saved, ctx.geom, x))
        return tuple(saved[-1][-1].nchw())

    @staticmethod
    def backward(ctx, *douts):
        spec: ChainSpec = ctx.spec
        x, scale, shift, *vecs = ctx.saved_tensors
        n, c, h, w, ldx = ctx.geom
        dev = x.device
        G = spec.G
        saved = ctx.saved_acts
        xin = ([V(x.data_ptr(), ldx, c)] * G, (h, w), c)
        q = ops.colsum_queue(dev)
        dvs = []
        if vecs:
            flat, dvs = spec.dv_buffers([v.numel() for v in vecs], dev)
            flat.zero_()
        try:
            with ops.local_wgrad_defer(dev, ("chain-local", dev.index)):
                dz_v, dz_t, dscale, dshift = _output_grad(spec, saved[-1][-1], douts, scale, shift, dvs, dev)
                dz_hw = (saved[-1][-1].h, saved[-1][-1].w)
                dx_out = None
                # ---- units in reverse
                for u in reversed(range(spec.U)):
                    layers0 = spec.unit(0, u).layers
                    g_unit, g_unit_keep = dz_v, dz_t   # gradient wrt the unit output (kept alive: the residual operand of the
                    # unit's first input-gradient conv reads it after the per-layer gradients have been replaced)
                    assert layers0[-1].act is None, "the last layer of a unit carries no activation"
                    for li in reversed(range(len(layers0))):
                        convs = [lay.conv for lay in spec.layers(u, li)]
                        sp = convs[0].spec
                        lin, (ih, iw), lin_c = _layer_input(saved, xin, u, li)
                        oh_, ow_ = dz_hw
                        wts = [cv.weight for cv in convs]
                        if wts[0].requires_grad:   # weight gradient: (dz, layer input)
                            gp = [HF.grad_slot(wt).data_ptr() for wt in wts]
                            if sp.transposed:
                                ops.wgrad_multi(n, ih, iw, oh_, ow_, lin, dz_v, gp, wts[0].shape[0], wts[0].shape[1], sp.k, sp.stride, sp.pad,
                                                device=dev, label=spec.name)
                            else:
                                ops.wgrad_multi(n, oh_, ow_, ih, iw, dz_v, lin, gp, wts[0].shape[0], wts[0].shape[1], sp.k, sp.stride, sp.pad,
                                                device=dev, label=spec.name)
                        first = li == 0
                        if first and u == 0 and not ctx.needs_input_grad[0]:
                            break
                        if first and u == 0 and (not sp.transposed) and sp.in_ch <= 4 and sp.k[0] * sp.k[1] > 1:
                            assert G == 1   # RGB image gradient: GEMM + gather path (nothing to fuse at the chain input)
                            dx_out = [HF.scatter_conv(dz_t[0], convs[0].weight, None, sp, (ih, iw))]
                            break
                        # input gradient, with the backward of the layers that produced this input fused in: the layer below, or (first
                        # layer of a unit) the last layer of the unit before, which carries no activation -- and the residual's
                        dgrad = Acts(G, n, ih, iw, lin_c, dev)
                        ys, yts = dgrad.vs(), dgrad.nchw()
                        flags, masks, vec2 = 0, None, None
                        targets = [(None, None)] * G
                        if not (first and u == 0):
                            below = spec.layers(u, li - 1) if not first else spec.layers(u - 1, -1)
                            targets = _colsum_targets(below, dvs)
                            b0 = below[0]
                            if b0.act is not None:
                                flags |= L.EPI_RELUMASK if b0.act == "relu" else L.EPI_LRELUMASK
                                masks = lin
                                if b0.vec_index is not None:
                                    flags |= L.EPI_MASKOFF
                                    vec2 = vecs[b0.vec_index].data_ptr()
                        ress = g_unit if (first and spec.unit(0, u).residual) else None
                        want_cs = any(a is not None or b is not None for a, b in targets)
                        packs = [cv.spec.pack(cv.weight, True) for cv in convs]
                        cs = ops.conv_multi(n, oh_, ow_, ih, iw, dz_v, [pk.data_ptr() for pk in packs], ys, lin_c, sp.k, sp.stride, sp.pad,
                                            not sp.transposed, wrows=packs[0].shape[1], wcols=packs[0].shape[2], masks=masks, ress=ress,
                                            vec2=vec2, flags=flags, colsum=want_cs, wlayout=1 if sp.smallc_dgrad else 0, device=dev,
                                            label=spec.name + ".bwd")
                        if want_cs:
                            for (ptr, rows, ld), (pre, post) in zip(cs, targets):
                                q.add(ptr, rows, ld, lin_c, pre, post, True)
                        dz_v, dz_t, dz_hw = ys, yts, (ih, iw)
                    if u == 0 and dx_out is None and ctx.needs_input_grad[0]:
                        dx_out = dz_t
                q.flush(spec.site)
        except BaseException:
            q.drop()   # (like the scope's weight-gradient jobs: the next backward on this device must not finish stale column sums)
            raise
        dx = None
        if dx_out is not None:
            dx = dx_out[0]
            for g in range(1, len(dx_out)):
                dx = dx + dx_out[g]
        # the beta-vector gradients live in the chain's persistent buffer, which the next backward of this spec zeroes.  Under
        # graph capture the fixed address is the point (the projections' backward consumes them inside the same captured
        # pass); eagerly autograd gets copies, so a second backward of the same chain (retain_graph, the chain used twice in
        # one graph) cannot clobber gradients the engine still holds
        keep = torch.cuda.is_current_stream_capturing()
        return (dx, None, dscale, dshift, None) + tuple((dvs[i] if keep else dvs[i].clone()) if ctx.needs_input_grad[5 + i] else None
                                                        for i in range(len(vecs))) \
            + (None,) * (ctx.nrest - len(vecs))


def run_chain(x, spec: ChainSpec, scale=None, shift=None, vecs=()):
    return _ChainFn.apply(x, spec, scale, shift, len(vecs), *vecs, *spec.parameters())


class _ChainReuseFn(torch.autograd.Function):
    """(handle, *params) -> the kept forward's outputs; backward = _ChainFn.backward on the kept activations (weight and bias gradients into the
    flat .grad slots; no gradient for the chain input: it was produced by another graph and is treated as detached)"""

    @staticmethod
    def forward(ctx, handle: ChainHandle, *params):
        ctx.spec, ctx.saved_acts, ctx.geom = handle.spec, handle.saved, handle.geom
        ctx.nrest = len(params)
        ctx.save_for_backward(handle.x, None, None)
        return tuple(handle.saved[-1][-1].nchw())

    @staticmethod
    def backward(ctx, *douts):
        _ChainFn.backward(_KeptCtx(ctx), *douts)
        return (None,) * (1 + ctx.nrest)


def run_chain_reuse(handle: ChainHandle):
    """The outputs of a chain forward kept by KEEP_HANDLES, as a differentiable function of the chain's parameters (see above)."""
    return _ChainReuseFn.apply(handle, *handle.spec.parameters())
