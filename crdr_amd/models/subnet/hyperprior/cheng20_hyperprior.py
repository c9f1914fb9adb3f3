"""Hyper analysis / synthesis of Cheng et al. (CVPR 2020) as the reference's hyperprior-only models use them
(src/models/subnet/hyperprior/cheng20_hyperprior.py:22-59): five 3x3 layers with LeakyReLU(0.2) after the first four.
Encoder: c3 and c5 have stride 2.  Decoder: c2 and c4 are ConvTranspose2d(k=4, s=2, p=1), c5 a plain 3x3 conv whose
output is (mean | scale) along the channels.  Keys `c1.0`, `c2.0`, `c3.0`, `c4.0`, `c5` (index 1 of each nn.Sequential
is its activation); the LeakyReLU rides in the conv epilogue."""
from __future__ import annotations

import torch.nn as nn

from crdr_amd.models.layer.hip_layers import HipConv2d, HipConvTranspose2d
from crdr_amd.utils.registry import HYPERDECODER_REGISTRY, HYPERENCODER_REGISTRY


class _Act(nn.Module):
    """a conv under index 0 of the reference's nn.Sequential(conv, LeakyReLU(0.2))"""

    def __init__(self, conv: nn.Module):
        super().__init__()
        self.add_module("0", conv)

    def __getitem__(self, i):
        return getattr(self, str(i))

    def forward(self, x):
        return self[0](x, act="lrelu")


def conv_lrelu(in_ch: int, out_ch: int, stride: int = 1) -> _Act:
    return _Act(HipConv2d(in_ch, out_ch, 3, stride=stride, padding=1))


def up_conv(in_ch: int, out_ch: int) -> _Act:
    return _Act(HipConvTranspose2d(in_ch, out_ch, 4, stride=2, padding=1))


@HYPERENCODER_REGISTRY.register()
class Cheng20HyperEncoder(nn.Module):
    def __init__(self, in_ch: int = 192, out_ch: int = 192, main_ch: int = 192, **kwargs):
        super().__init__()
        self.c1 = conv_lrelu(in_ch, main_ch)
        self.c2 = conv_lrelu(main_ch, main_ch)
        self.c3 = conv_lrelu(main_ch, main_ch, stride=2)
        self.c4 = conv_lrelu(main_ch, main_ch)
        self.c5 = HipConv2d(main_ch, out_ch, 3, stride=2, padding=1)
        self.num_downscale = 2
        self.latent_ch = out_ch

    def forward(self, x):
        return self.c5(self.c4(self.c3(self.c2(self.c1(x)))))


@HYPERDECODER_REGISTRY.register()
class Cheng20HyperDecoder(nn.Module):
    def __init__(self, in_ch: int = 192, out_ch: int = 384, main_ch: int = 192, **kwargs):
        super().__init__()
        assert out_ch % 2 == 0
        self.c1 = conv_lrelu(in_ch, main_ch)
        self.c2 = up_conv(main_ch, main_ch)
        self.c3 = conv_lrelu(main_ch, main_ch)
        self.c4 = up_conv(main_ch, main_ch)
        self.c5 = HipConv2d(main_ch, out_ch, 3, stride=1, padding=1)
        self.mean_ch = out_ch // 2

    def forward(self, x):
        return self.c5(self.c4(self.c3(self.c2(self.c1(x)))))

    def hd_mu(self, z_hat):
        """The mean half of forward(): one trunk feeds both halves, so the whole decoder runs and the first out_ch / 2 channels come back
        as a view -- bit-identical to forward(z_hat)[:, :out_ch / 2]."""
        return self.forward(z_hat)[:, :self.mean_ch]
