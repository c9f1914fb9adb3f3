"""Cheng20 transforms with interpolation channel attention (Sun et al., ACM MM 2022; src/models/subnet/autoencoder/
cheng20_interpca_autoencoder.py:16-74).  Encoder: InterpChAtt AFTER each of the nine stages; decoder: BEFORE each of the ten.  As in
elic_interpca_autoencoder.py the per-channel scale + shift rides in the epilogue of the launch that produces the tensor where that
launch is a conv (ResBlock ending in LeakyReLU, the NLAM gate, conv7); behind a block that ends in GDN / IGDN it is one affine launch."""
from __future__ import annotations

from typing import Dict

import torch.nn as nn

from crdr_amd.models.layer.hip_layers import to_image_nhwc
from crdr_amd.models.layer.interp_channel_attention import InterpChAtt
from crdr_amd.utils.registry import DECODER_REGISTRY, ENCODER_REGISTRY

from .cheng20_autoencoder import Cheng20Decoder, Cheng20Encoder


@ENCODER_REGISTRY.register()
class Cheng20InterpCaEncoder(Cheng20Encoder):
    def __init__(self, rate_level: int, in_ch: int = 3, out_ch: int = 192, main_ch: int = 192, padding_mode: str = "zeros",
                 ca_kwargs: Dict = {}, **kwargs):
        super().__init__(in_ch=in_ch, out_ch=out_ch, main_ch=main_ch, padding_mode=padding_mode)
        # cheng20_interpca_autoencoder.py:32-34 builds ALL nine with main_ch, the two behind conv7 and nlam2 (out_ch channels) included
        assert out_ch == main_ch, (f"Cheng20InterpCaEncoder: out_ch ({out_ch}) must equal main_ch ({main_ch}) -- the reference sizes the "
                                   "channel attention behind conv7 and nlam2 with main_ch")
        self.layer_list = list(self.stage_names)
        self.interp_ca_list = nn.ModuleList(InterpChAtt(main_ch, rate_level, **ca_kwargs) for _ in self.layer_list)

    def forward(self, x, rate_ind):
        x = to_image_nhwc(x)
        for name, ca in zip(self.layer_list, self.interp_ca_list):
            x = getattr(self, name)(x, affine=ca.vectors(rate_ind))   # layer -> interp_ca
        return x


@DECODER_REGISTRY.register()
class Cheng20InterpCaDecoder(Cheng20Decoder):
    def __init__(self, rate_level: int, in_ch: int = 192, out_ch: int = 3, main_ch: int = 192, use_tanh: bool = True,
                 padding_mode: str = "zeros", ca_kwargs: Dict = {}, **kwargs):
        super().__init__(in_ch=in_ch, out_ch=out_ch, main_ch=main_ch, use_tanh=use_tanh, padding_mode=padding_mode)
        self.layer_list = list(self.stage_names)
        chans = [in_ch] * 2 + [main_ch] * (len(self.layer_list) - 2)   # (cheng20_interpca_autoencoder.py:63-65)
        self.interp_ca_list = nn.ModuleList(InterpChAtt(c, rate_level, **ca_kwargs) for c in chans)

    def forward(self, x, rate_ind):
        # interp_ca_i -> layer_i: the first is a stand-alone affine on y_hat, every later one the epilogue of layer_{i-1}
        cas = list(self.interp_ca_list)
        x = cas[0](x, rate_ind)
        for i, name in enumerate(self.layer_list):
            nxt = cas[i + 1].vectors(rate_ind) if i + 1 < len(cas) else None
            x = getattr(self, name)(x, affine=nxt)
        return self.finish(x)
