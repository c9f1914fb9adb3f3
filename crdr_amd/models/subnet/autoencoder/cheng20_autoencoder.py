"""Cheng et al. (CVPR 2020) transforms: residual blocks with GDN / inverse GDN at the resolution changes, simplified attention
(src/models/subnet/autoencoder/cheng20_autoencoder.py:12-106; an ablation baseline of the reference and the backbone of its
variable-rate baseline, cheng20_interpca_autoencoder.py).  Same constructor arguments, defaults and state-dict keys.  Every stage takes
`affine`, the (scale, shift) of an InterpChAtt that follows it, and applies it in its last launch where that launch is a conv."""
from __future__ import annotations

import torch.nn as nn

from crdr_amd.hip import functional as HF
from crdr_amd.models.layer.cheng_nlam import ChengNLAM
from crdr_amd.models.layer.cheng_resblock import ResBlock, UpResBlock
from crdr_amd.models.layer.hip_layers import HipConv2d, to_image_nhwc
from crdr_amd.utils.registry import DECODER_REGISTRY, ENCODER_REGISTRY

from .base_autoencoder import BaseDecoder, BaseEncoder


@ENCODER_REGISTRY.register()
class Cheng20Encoder(BaseEncoder):
    stage_names = ("block1", "block2", "block3", "nlam1", "block4", "block5", "block6", "conv7", "nlam2")

    def __init__(self, in_ch: int = 3, out_ch: int = 192, main_ch: int = 192, padding_mode: str = "zeros", **kwargs):
        super().__init__()
        down = dict(actv="lrelu", actv2="gdn", downscale=True, padding_mode=padding_mode)
        normal = dict(actv="lrelu", actv2="lrelu", downscale=False, padding_mode=padding_mode)
        self.block1 = ResBlock(in_ch, main_ch, **down)        # (H, W) -> (H/2, W/2)
        self.block2 = ResBlock(main_ch, main_ch, **normal)
        self.block3 = ResBlock(main_ch, main_ch, **down)      # -> (H/4, W/4)
        self.nlam1 = ChengNLAM(main_ch, padding_mode=padding_mode)
        self.block4 = ResBlock(main_ch, main_ch, **normal)
        self.block5 = ResBlock(main_ch, main_ch, **down)      # -> (H/8, W/8)
        self.block6 = ResBlock(main_ch, main_ch, **normal)
        self.conv7 = HipConv2d(main_ch, out_ch, 3, stride=2, padding=1)   # -> (H/16, W/16)
        self.nlam2 = ChengNLAM(out_ch, padding_mode=padding_mode)
        self.num_downscale = 4
        self.latent_ch = out_ch

    def forward(self, x):
        x = to_image_nhwc(x)
        for name in self.stage_names:
            x = getattr(self, name)(x)
        return x


class _Up3(nn.Module):
    """conv -> 4 out_ch, PixelShuffle(2): the reference's `up3` Sequential (key `up3.0`); 12 -> 3 channels gives the image layout"""

    def __init__(self, in_ch: int, out_ch: int):
        super().__init__()
        self.add_module("0", HipConv2d(in_ch, out_ch * 4, 3, padding=1))

    def forward(self, x, affine=None):
        assert affine is None, "nothing follows up3"
        return HF.pixel_shuffle(getattr(self, "0")(x))


@DECODER_REGISTRY.register()
class Cheng20Decoder(BaseDecoder):
    stage_names = ("nlam0", "block0", "up0", "block1", "up1", "nlam2", "block2", "up2", "block3", "up3")

    def __init__(self, in_ch: int = 192, out_ch: int = 3, main_ch: int = 192, use_tanh: bool = True, padding_mode: str = "zeros", **kwargs):
        super().__init__()
        up = dict(actv="lrelu", actv2="igdn", padding_mode=padding_mode)
        normal = dict(actv="lrelu", actv2="lrelu", padding_mode=padding_mode)
        self.nlam0 = ChengNLAM(in_ch, padding_mode=padding_mode)
        self.block0 = ResBlock(in_ch, main_ch, **normal)
        self.up0 = UpResBlock(main_ch, main_ch, **up)         # (H/16, W/16) -> (H/8, W/8)
        self.block1 = ResBlock(main_ch, main_ch, **normal)
        self.up1 = UpResBlock(main_ch, main_ch, **up)         # -> (H/4, W/4)
        self.nlam2 = ChengNLAM(main_ch, padding_mode=padding_mode)
        self.block2 = ResBlock(main_ch, main_ch, **normal)
        self.up2 = UpResBlock(main_ch, main_ch, **up)         # -> (H/2, W/2)
        self.block3 = ResBlock(main_ch, main_ch, **normal)
        self.up3 = _Up3(main_ch, out_ch)                      # -> (H, W)
        self.use_tanh = use_tanh

    def finish(self, x):
        return HF.tanh(x) if self.use_tanh else x

    def forward(self, x):
        for name in self.stage_names:
            x = getattr(self, name)(x)
        return self.finish(x)
