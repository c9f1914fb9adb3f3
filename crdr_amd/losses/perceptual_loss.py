"""LPIPS perceptual loss on the HIP kernels (src/losses/perceptual_loss.py:11-30 wraps lpips==0.1.4, which is third-party and not
installed here), for the two backbones a training config names:

  net: alex  scaling layer -> AlexNet conv1..5 (ReLU fused, max-pool 3/2 before conv2 and conv3), taps = the five conv outputs
  net: vgg   scaling layer -> the thirteen 3x3 convs of VGG16 (ReLU fused, max-pool 2/2 between the five groups; torchvision's fifth
             pool is not part of LPIPS), taps = relu1_2, relu2_2, relu3_3, relu4_3, relu5_3

-> per tap: unit-normalise over channels, squared difference, 1x1 `lin` weights, spatial mean; summed over the five taps.  The network
is frozen; gradients flow to the reconstructed image only.  `range_norm: true` (images in [0, 1] instead of [-1, 1], reference :26-28)
is folded into the scaling layer's constants and costs no launch.

Weights: torchvision's backbone + lpips' linear heads cannot be downloaded here, so they are supplied as ONE file,
`torch.save({"alexnet_features": torchvision.models.alexnet(weights=...).features.state_dict(),
             "lpips_lin": {k: v for k, v in lpips.LPIPS(net="alex").state_dict().items() if k.startswith("lin")}}, path)`
(for `net: vgg`: "vgg16_features" from torchvision.models.vgg16(weights=...).features and the lin entries of lpips.LPIPS(net="vgg")),
named by the loss option `weights:` (YAML / CLI overlay `loss.perceptual_loss.weights=...`) or the environment variable
CRDR_LPIPS_WEIGHTS.  Without it LPIPSLoss refuses to be built -- a random-feature distance is not LPIPS -- unless
`allow_random_weights: true` / CRDR_ALLOW_RANDOM_LPIPS=1 is set explicitly (throughput benchmark, tests)."""
from __future__ import annotations

import logging
import os
from typing import Dict, Optional

import torch
import torch.nn as nn

from crdr_amd.hip import functional as HF
from crdr_amd.hip import ops
from crdr_amd.models.layer.hip_layers import HipConv2d
from crdr_amd.utils.registry import LOSS_REGISTRY

ALEX_CFG = ((3, 64, 11, 4, 2), (64, 192, 5, 1, 2), (192, 384, 3, 1, 1), (384, 256, 3, 1, 1), (256, 256, 3, 1, 1))
LPIPS_SHIFT = (-0.030, -0.088, -0.188)
LPIPS_SCALE = (0.458, 0.448, 0.450)
_TV_IDX = (0, 3, 6, 8, 10)  # torchvision alexnet.features indices of the convs

# VGG16: (in, out) of the 3x3 / padding 1 convs, group by group; a 2/2 max-pool in front of the first conv of groups 2..5
VGG_GROUPS = (((3, 64), (64, 64)), ((64, 128), (128, 128)), ((128, 256), (256, 256), (256, 256)),
              ((256, 512), (512, 512), (512, 512)), ((512, 512), (512, 512), (512, 512)))
VGG_CFG = tuple(io for grp in VGG_GROUPS for io in grp)
VGG_TV_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)   # torchvision vgg16.features indices of the convs
VGG_POOL_BEFORE = (2, 4, 7, 10)    # convs (in VGG_CFG order) that read a pooled map
VGG_TAPS = (1, 3, 6, 9, 12)        # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
VGG_MIN_SIDE = 16                  # four pools: below 16 the last one has no output


def scaling_constants(range_norm: bool = False):
    """(scale, shift) of the scaling layer as one affine map: (x - SHIFT) / SCALE, and with range_norm the same applied to
    (x - 0.5) * 2:  scale' = 2 scale, shift' = shift - scale."""
    if not range_norm:
        return 1.0 / torch.tensor(LPIPS_SCALE), -torch.tensor(LPIPS_SHIFT) / torch.tensor(LPIPS_SCALE)
    shift, scale = torch.tensor(LPIPS_SHIFT, dtype=torch.float64), torch.tensor(LPIPS_SCALE, dtype=torch.float64)
    in_scale, in_shift = 1.0 / scale, -shift / scale   # folded in float64, rounded once
    return (2.0 * in_scale).float(), (in_shift - in_scale).float()


class _LpipsNet(nn.Module):
    """What the two backbones share: the frozen parameters `net.{i}` / `lin.{i}`, the scaling layer, the weights file, the distance."""
    FEATURES_KEY = ""    # the backbone's entry of the weights file
    TV_IDX = ()          # torchvision `features` index of conv i

    def _finish(self, lin_widths, range_norm: bool) -> None:
        self.lin = nn.ParameterList(nn.Parameter(torch.rand(co) * 0.1) for co in lin_widths)
        in_scale, in_shift = scaling_constants(range_norm)
        self.register_buffer("in_scale", in_scale)
        self.register_buffer("in_shift", in_shift)
        for p in self.parameters():
            p.requires_grad_(False)

    def load_lpips_weights(self, features_sd: Dict[str, torch.Tensor], lpips_lin_sd: Dict[str, torch.Tensor]) -> None:
        for i, j in enumerate(self.TV_IDX):
            self.net[i].weight.data.copy_(features_sd[f"{j}.weight"])
            self.net[i].bias.data.copy_(features_sd[f"{j}.bias"])
        for i in range(len(self.lin)):
            self.lin[i].data.copy_(lpips_lin_sd[f"lin{i}.model.1.weight"].reshape(-1))

    def load_lpips_file(self, path: str) -> None:
        """One file holding {FEATURES_KEY: state dict of the torchvision backbone's `features`,
        "lpips_lin": lpips.LPIPS(net=...) state dict (its lin{i}.model.1.weight entries)}."""
        blob = torch.load(path, map_location="cpu")
        if not (isinstance(blob, dict) and self.FEATURES_KEY in blob and "lpips_lin" in blob):
            raise ValueError(f"{path}: expected a dict with the keys '{self.FEATURES_KEY}' and 'lpips_lin' (see crdr_amd/losses/"
                             "perceptual_loss.py)")
        self.load_lpips_weights(blob[self.FEATURES_KEY], blob["lpips_lin"])

    def forward(self, real, fake):
        with torch.no_grad():
            f_real = self.features(real.detach())
        f_fake = self.features(fake)
        total = None
        for a, b, lin in zip(f_real, f_fake, self.lin):
            d = HF.lpips_layer(a, b, lin)
            total = d if total is None else total + d
        return total  # [N]


class LpipsAlex(_LpipsNet):
    FEATURES_KEY = "alexnet_features"
    TV_IDX = _TV_IDX

    def __init__(self, range_norm: bool = False):
        super().__init__()
        self.net = nn.ModuleList(HipConv2d(ci, co, k, stride=s, padding=p) for ci, co, k, s, p in ALEX_CFG)
        self._finish([co for _, co, _, _, _ in ALEX_CFG], range_norm)

    def features(self, x):
        x, _ = ops.nhwc(x)
        x = HF.affine(x, self.in_scale, self.in_shift)
        feats = []
        for i, conv in enumerate(self.net):
            if i in (1, 2):
                x = HF.maxpool3s2(x)
            x = conv(x, act="relu")
            feats.append(x)
        return feats


class LpipsVgg(_LpipsNet):
    FEATURES_KEY = "vgg16_features"
    TV_IDX = VGG_TV_IDX

    def __init__(self, range_norm: bool = False):
        super().__init__()
        self.net = nn.ModuleList(HipConv2d(ci, co, 3, padding=1) for ci, co in VGG_CFG)
        self._finish([VGG_CFG[i][1] for i in VGG_TAPS], range_norm)

    def features(self, x, all_layers: bool = False):
        """The five taps, or with all_layers the thirteen post-ReLU maps in conv order."""
        if min(x.shape[2], x.shape[3]) < VGG_MIN_SIDE:
            raise ValueError(f"LPIPS-VGG needs images of at least {VGG_MIN_SIDE} x {VGG_MIN_SIDE} pixels (four 2/2 max-pools), got "
                             f"{x.shape[2]} x {x.shape[3]}")
        x, _ = ops.nhwc(x)
        x = HF.affine(x, self.in_scale, self.in_shift)
        feats = []
        for i, conv in enumerate(self.net):
            if i in VGG_POOL_BEFORE:
                x = HF.maxpool2s2(x)
            x = conv(x, act="relu")
            if all_layers or i in VGG_TAPS:
                feats.append(x)
        return feats


LPIPS_NETS = {"alex": LpipsAlex, "vgg": LpipsVgg}


@LOSS_REGISTRY.register()
class LPIPSLoss(nn.Module):
    def __init__(self, loss_weight: float, range_norm: bool = False, net: str = "alex", weights: Optional[str] = None,
                 allow_random_weights: bool = False):
        super().__init__()
        if net not in LPIPS_NETS:
            raise NotImplementedError(f"LPIPSLoss: net={net!r} is not available (net is one of {sorted(LPIPS_NETS)})")
        self.lamb_lpips = loss_weight
        self.lpips = LPIPS_NETS[net](range_norm=bool(range_norm))
        weights = weights or os.environ.get("CRDR_LPIPS_WEIGHTS")
        if weights:
            self.lpips.load_lpips_file(weights)
            self.pretrained = True
        elif allow_random_weights or os.environ.get("CRDR_ALLOW_RANDOM_LPIPS") == "1":
            logging.getLogger("crdr").warning(
                "LPIPSLoss: NO pretrained weights given -- the perceptual term is a random-feature distance, not LPIPS "
                "(fine for throughput measurements and plumbing tests, wrong for training)")
            self.pretrained = False
        else:
            raise RuntimeError(
                "LPIPSLoss needs the pretrained backbone (AlexNet or VGG16) + LPIPS linear-head weights (the reference gets them from the "
                "`lpips` package, src/losses/perceptual_loss.py:23): pass `weights: <file>` in loss.perceptual_loss or set "
                "CRDR_LPIPS_WEIGHTS (file layout: crdr_amd/losses/perceptual_loss.py); to run on random features on purpose "
                "set allow_random_weights: true or CRDR_ALLOW_RANDOM_LPIPS=1")

    def forward(self, real_images, fake_images):
        return self.lamb_lpips * self.lpips(real_images, fake_images).mean()
