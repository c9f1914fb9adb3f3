"""PatchGAN-like discriminator used per rate level in stage 3
(src/models/discriminator/clic21_gvae_discriminator.py:12-50, `norm_type: none`): conv3 s1, [conv3 s2, conv3 s1]x3,
conv3 s2, conv3 head; LeakyReLU(0.2) fused into every conv but the head.  Parameter keys `model.{0,2,...,16}`.

`norm_type: CN` (clic21_gvae_discriminator.py:18-19) puts a ChannelNorm2D between conv and LeakyReLU on every block but the first:
the conv runs without activation and the norm carries the fused LeakyReLU(0.2).  Keys as the reference's nn.Sequential numbers them:
`model.0`, `model.2`, `model.3.{gamma,beta}`, `model.5`, `model.6.{gamma,beta}`, ..., `model.21.{gamma,beta}`, head `model.23`.

CLIC21GVAELatentConditionalDiscriminator (clic21_gvae_discriminator.py:53-68) is the same trunk behind a condition on the quantised latent:
`latent_conv.0` (1x1 conv + LeakyReLU(0.2) of y_hat.detach()), up-sampled x16 (bilinear, bicubic or nearest) and concatenated behind the
image by one kernel (hip/functional.py upsample16_cat), so the trunk's first conv reads 3 + latent_nc channels."""
from __future__ import annotations

import torch.nn as nn

from crdr_amd.hip import chain as CH
from crdr_amd.hip import functional as HF
from crdr_amd.models.layer.hific_norm import ChannelNorm2D
from crdr_amd.models.layer.hip_layers import HipConv2d, to_image_nhwc
from crdr_amd.utils.registry import DISCRIMINATOR_REGISTRY

from .base_discriminator import BaseDiscriminator


class _Blocks(nn.Module):
    def __init__(self, in_ch, main_ch, out_ch, kw, num_downscale, head=True):
        super().__init__()
        plan = [(in_ch, main_ch, 1), (main_ch, main_ch, 2)]
        c = main_ch
        for _ in range(num_downscale - 1):
            o = min(c * 2, main_ch * 8)
            plan += [(c, o, 1), (o, o, 2)]
            c = o
        self.n_act = len(plan)
        for i, (ci, co, s) in enumerate(plan):
            self.add_module(str(2 * i), HipConv2d(ci, co, kw, stride=s, padding=kw // 2))
        self.head = head
        if head:
            self.add_module(str(2 * self.n_act), HipConv2d(c, out_ch, 3, stride=1, padding=1))

    def _chain(self) -> "CH.ChainSpec":
        """the conv trunk as one hand-scheduled autograd node: LeakyReLU backward fused into the input-gradient convs,
        bias gradients from their epilogues (crdr_amd/hip/chain.py)"""
        sp = self.__dict__.get("_chain_spec")
        if sp is None:
            layers = [CH.Layer(getattr(self, str(2 * i)), "lrelu") for i in range(self.n_act)]
            if self.head:
                layers.append(CH.Layer(getattr(self, str(2 * self.n_act)), None))
            else:
                layers[-1] = CH.Layer(layers[-1].conv, None)
            sp = CH.ChainSpec([[CH.Unit(layers, residual=False)]], name="disc")
            self.__dict__["_chain_spec"] = sp
        return sp

    def forward(self, x):
        if self.head:
            return CH.run_chain(x, self._chain())[0]
        for i in range(self.n_act):
            x = getattr(self, str(2 * i))(x, act="lrelu")
        return x


class _BlocksCN(nn.Module):
    """the same trunk with ChannelNorm2D after every conv but the first (and the head)"""

    def __init__(self, in_ch, main_ch, out_ch, kw, num_downscale):
        super().__init__()
        plan = [(in_ch, main_ch, 1), (main_ch, main_ch, 2)]
        c = main_ch
        for _ in range(num_downscale - 1):
            o = min(c * 2, main_ch * 8)
            plan += [(c, o, 1), (o, o, 2)]
            c = o
        self.steps = []   # (conv index, norm index or None)
        idx = 0
        for i, (ci, co, s) in enumerate(plan):
            self.add_module(str(idx), HipConv2d(ci, co, kw, stride=s, padding=kw // 2))
            if i == 0:
                self.steps.append((idx, None))
                idx += 2   # conv, LeakyReLU
            else:
                self.add_module(str(idx + 1), ChannelNorm2D(co))
                self.steps.append((idx, idx + 1))
                idx += 3   # conv, norm, LeakyReLU
        self.head_idx = idx
        self.add_module(str(idx), HipConv2d(c, out_ch, 3, stride=1, padding=1))

    def forward(self, x):
        for ci, ni in self.steps:
            conv = getattr(self, str(ci))
            x = conv(x, act="lrelu") if ni is None else getattr(self, str(ni))(conv(x), act="lrelu", slope=0.2)
        return getattr(self, str(self.head_idx))(x)


def _trunk(in_ch, main_ch, out_ch, norm_type: str, num_downscale: int) -> nn.Module:
    if norm_type == "CN":
        return _BlocksCN(in_ch, main_ch, out_ch, 3, num_downscale)
    if norm_type != "none":
        raise NotImplementedError(f"norm_type {norm_type!r}: only 'none' (CRDR, config/crdr_stage_3.yaml:23) and 'CN' (ChannelNorm2D) "
                                  "are built; 'BN' and 'IN' are not")
    return _Blocks(in_ch, main_ch, out_ch, 3, num_downscale)


@DISCRIMINATOR_REGISTRY.register()
class CLIC21GVAEDiscriminator(BaseDiscriminator):
    def __init__(self, in_ch=3, out_ch=1, main_ch=64, norm_type: str = "BN", num_downscale: int = 4):
        super().__init__()
        self.model = _trunk(in_ch, main_ch, out_ch, norm_type, num_downscale)

    def forward(self, input, **kwargs):
        return self.model(to_image_nhwc(input))


@DISCRIMINATOR_REGISTRY.register()
class CLIC21GVAELatentConditionalDiscriminator(BaseDiscriminator):
    BATCH_INPUTS = ("y_hat",)   # per-sample keyword inputs: a trainer that stacks [x_hat; x] along the batch stacks these as well

    def __init__(self, in_ch=3, out_ch=1, y_ch=192, latent_nc=12, main_ch=64, norm_type: str = "BN", latent_interp_mode: str = "bilinear"):
        super().__init__()
        assert latent_interp_mode in ["bilinear", "bicubic", "nearest"]
        if in_ch != 3:
            raise NotImplementedError(f"in_ch {in_ch}: the fused up-sample + concat kernel takes a 3-channel image")
        if latent_nc % 4 != 0 or not 4 <= latent_nc <= 64:
            raise NotImplementedError(f"latent_nc {latent_nc}: the fused up-sample + concat kernel takes a multiple of 4 in [4, 64]")
        self.latent_conv = nn.Sequential()
        self.latent_conv.add_module("0", HipConv2d(y_ch, latent_nc, 1))
        self.model = _trunk(in_ch + latent_nc, main_ch, out_ch, norm_type, 4)
        self.latent_interp_mode = latent_interp_mode

    def forward(self, input, y_hat, **kwargs):
        cond = getattr(self.latent_conv, "0")(y_hat.detach(), act="lrelu")
        x = HF.upsample16_cat(to_image_nhwc(input), cond, self.latent_interp_mode)
        # The trunk's input depends on a trainable layer (latent_conv), and a kept chain handle gives no gradient to the chain's input
        # (chain.run_chain_reuse): reused in the discriminator phase it would drop latent_conv's gradient from the D(x_hat) term.  So this
        # class hands out no handle, and the trainers take their one-pass [x_hat; x] path.
        keep, CH.KEEP_HANDLES = CH.KEEP_HANDLES, None
        try:
            return self.model(x)
        finally:
            CH.KEEP_HANDLES = keep
