"""The four rate-aware CLIC21 discriminators the paper weighs against "one discriminator per rate"
(src/models/discriminator/multirate_clic21_gvae_discriminator.py:12-283), with the reference's constructor arguments, defaults and
state-dict keys:

    SharedBackboneClic21GvaeDiscriminator            one backbone, one head per rate            backbone.*, head_list.{i}.*
    SharedHeadClic21GvaeDiscriminator                one backbone per rate, one head            backbone_list.{i}.*, head.*
    MultirateSeparateClic21GvaeDiscriminator         one whole discriminator per rate           discriminator_list.{i}.*
    MultirateSharedRateCondClic21GvaeDiscriminator   one discriminator, one-hot rate planes     net.*

A block (`b{res}`, :77-101) is conv3 s1 -> [IN] -> LeakyReLU(0.2), conv3 s2 -> [IN] -> LeakyReLU(0.2), its convs under `b{res}.{0,1}.0`;
a head (:104-119) is blocks under `block.` and `last_conv`.  `norm_type: none` rides the activation in the conv's epilogue; with `IN` the
conv runs bare and InstanceNorm2D (affine=False: no keys) carries the fused LeakyReLU.  `BN` is not built: it needs batch statistics and
running buffers, and would break the trainer's one discriminator pass over [x_hat; x].

The one-hot condition (:68-74) is `rate_level` constant planes behind the image (SharedBackbone, SharedRateCond) or behind the backbone's
features (SharedHead); it is laid out by ATen -- off the hot path -- straight into dense NHWC memory whose pixel stride is the channel
count rounded up to 4, the pad lanes zero, which is the form HipConv2d takes an input width that is no multiple of 4 in (the image's own
3 + 1).  The gradient flows to the image / feature channels only.

`partition_modules()` / `partitions_for(q)` tell the stage-3 trainer which contiguous parameter ranges rate q trains, so that the flat
Adam leaves the others' moments and step counts alone, as torch.optim.Adam does for parameters whose .grad is None."""
from __future__ import annotations

from typing import Dict, List, Tuple, Union

import torch
import torch.nn as nn

from crdr_amd.hip import ops
from crdr_amd.models.layer.hip_layers import HipConv2d, to_image_nhwc
from crdr_amd.models.layer.instance_norm import InstanceNorm2D
from crdr_amd.utils.registry import DISCRIMINATOR_REGISTRY

from .base_discriminator import BaseDiscriminator

NORM_TYPES = ("none", "IN")


def _check_norm(norm_type: str) -> None:
    if norm_type not in NORM_TYPES:
        raise NotImplementedError(f"norm_type {norm_type!r}: only 'none' and 'IN' (InstanceNorm2D) are built; 'BN' needs batch statistics "
                                  "and running buffers")


def build_channel_dict(img_size: int, in_ch: int, main_ch: int, max_ch: int) -> Dict[int, int]:
    """{img_size: in_ch, img_size / 2: main_ch, img_size / 4: min(2 main_ch, max_ch), ...} down to resolution 8 (:27-56)"""
    levels = img_size.bit_length() - 1
    assert img_size > 0 and (1 << levels) == img_size, f"invalid img_size: {img_size}"
    chans = {img_size: in_ch}
    ch = main_ch
    for k in range(1, levels - 1):
        chans[img_size >> k] = ch
        ch = min(2 * ch, max_ch)
    return chans


def as_list(val: Union[int, List, Tuple], length: int):
    """an int repeated `length` times, or the list / tuple itself if it has that length (:59-65)"""
    if isinstance(val, (list, tuple)):
        assert len(val) == length, f"len(val) must be {length}, but got {len(val)}"
        return val
    if isinstance(val, int):
        return [val] * length
    raise TypeError(f"val must be int, list, or tuple, but got {type(val)}")


def _rate_index(rate_ind) -> int:
    if isinstance(rate_ind, torch.Tensor):
        assert rate_ind.numel() == 1
        rate_ind = rate_ind.item()
    return int(rate_ind)


def cat_onehot_nhwc(x: torch.Tensor, rate_ind: int, rate_level: int) -> torch.Tensor:
    """[x; one_hot(rate_ind) as constant planes] along the channels, in dense NHWC memory with the pixel stride rounded up to 4 (pad
    lanes zero).  x is copied in through autograd; the planes are constants."""
    n, c, h, w = x.shape
    buf = torch.zeros((n, h, w, ops.ld_for(c + rate_level)), dtype=x.dtype, device=x.device)
    buf[..., c + rate_ind] = 1.0
    buf[..., :c] = x.permute(0, 2, 3, 1)
    return buf.permute(0, 3, 1, 2)[:, :c + rate_level]


class _ConvNormLrelu(nn.Module):
    """conv `0`, norm `1` (without keys), LeakyReLU(0.2) (:12-24)"""

    def __init__(self, in_ch: int, out_ch: int, stride: int, norm_type: str):
        super().__init__()
        self.add_module("0", HipConv2d(in_ch, out_ch, 3, stride=stride, padding=1))
        if norm_type == "IN":
            self.add_module("1", InstanceNorm2D(out_ch))
        self.normed = norm_type == "IN"

    def forward(self, x):
        conv = getattr(self, "0")
        return getattr(self, "1")(conv(x), act="lrelu", slope=0.2) if self.normed else conv(x, act="lrelu")


class _Pair(nn.Module):
    def __init__(self, in_ch: int, out_ch: int, norm_type: str):
        super().__init__()
        self.add_module("0", _ConvNormLrelu(in_ch, out_ch, 1, norm_type))
        self.add_module("1", _ConvNormLrelu(out_ch, out_ch, 2, norm_type))

    def forward(self, x):
        return getattr(self, "1")(getattr(self, "0")(x))


class DiscriminatorBlock(nn.Module):
    def __init__(self, channel_dict: Dict[int, int], input_res: int, num_depth: int, norm_type: str):
        super().__init__()
        self.block_resolutions = [input_res >> i for i in range(num_depth)]
        for res in self.block_resolutions:
            self.add_module(f"b{res}", _Pair(channel_dict[res], channel_dict[res // 2], norm_type))

    def forward(self, x):
        for res in self.block_resolutions:
            x = getattr(self, f"b{res}")(x)
        return x


class DiscriminatorHead(nn.Module):
    def __init__(self, out_ch: int, channel_dict: Dict[int, int], input_res: int, num_depth: int, norm_type: str):
        super().__init__()
        self.block = DiscriminatorBlock(channel_dict, input_res, num_depth, norm_type)
        self.last_conv = HipConv2d(channel_dict[input_res >> num_depth], out_ch, 3, stride=1, padding=1)

    def forward(self, x):
        return self.last_conv(self.block(x))


@DISCRIMINATOR_REGISTRY.register()
class SharedBackboneClic21GvaeDiscriminator(BaseDiscriminator):
    """Shared backbone + one head per rate"""

    def __init__(self, num_head: int, in_ch: int = 3, out_ch: int = 1, main_ch: int = 64, img_size: int = 256, norm_type: str = "none",
                 backbone_depth: int = 2, head_depth: int = 2, use_rate_ind_cond: bool = False):
        super().__init__()
        _check_norm(norm_type)
        chans = build_channel_dict(img_size, in_ch, main_ch, main_ch * 8)
        self.use_rate_ind_cond, self.rate_level = use_rate_ind_cond, num_head
        if use_rate_ind_cond:
            chans[img_size] += num_head
        self.backbone = DiscriminatorBlock(chans, img_size, backbone_depth, norm_type)
        self.head_list = nn.ModuleList(DiscriminatorHead(out_ch, chans, img_size >> backbone_depth, head_depth, norm_type)
                                       for _ in range(num_head))

    def forward(self, input, rate_ind, **kwargs):
        q = _rate_index(rate_ind)
        x = to_image_nhwc(input)
        if self.use_rate_ind_cond:
            x = cat_onehot_nhwc(x, q, self.rate_level)
        return self.head_list[q](self.backbone(x))

    def partition_modules(self):
        return [self.backbone, *self.head_list]

    def partitions_for(self, q):
        return [0, 1 + _rate_index(q)]


@DISCRIMINATOR_REGISTRY.register()
class SharedHeadClic21GvaeDiscriminator(BaseDiscriminator):
    """One backbone per rate + shared head"""

    def __init__(self, num_backbone: int, in_ch: int = 3, out_ch: int = 1, main_ch: int = 64, img_size: int = 256, norm_type: str = "none",
                 backbone_depth: int = 2, head_depth: int = 2, use_rate_ind_cond: bool = False):
        super().__init__()
        _check_norm(norm_type)
        chans = build_channel_dict(img_size, in_ch, main_ch, main_ch * 8)
        feat_size = img_size >> backbone_depth
        self.backbone_list = nn.ModuleList(DiscriminatorBlock(chans, img_size, backbone_depth, norm_type) for _ in range(num_backbone))
        self.use_rate_ind_cond, self.rate_level = use_rate_ind_cond, num_backbone
        if use_rate_ind_cond:
            chans[feat_size] += num_backbone
        self.head = DiscriminatorHead(out_ch, chans, feat_size, head_depth, norm_type)

    def forward(self, input, rate_ind, **kwargs):
        q = _rate_index(rate_ind)
        feat = self.backbone_list[q](to_image_nhwc(input))
        if self.use_rate_ind_cond:
            feat = cat_onehot_nhwc(feat, q, self.rate_level)
        return self.head(feat)

    def partition_modules(self):
        return [*self.backbone_list, self.head]

    def partitions_for(self, q):
        return [_rate_index(q), len(self.backbone_list)]


@DISCRIMINATOR_REGISTRY.register()
class MultirateSeparateClic21GvaeDiscriminator(BaseDiscriminator):
    """One whole discriminator per rate (widths and depths may differ per rate)"""

    def __init__(self, rate_level: int, in_ch: int = 3, out_ch: int = 1, main_ch: Union[int, List[int]] = 64, img_size: int = 256,
                 norm_type: str = "none", depth: Union[int, List[int]] = 4):
        super().__init__()
        _check_norm(norm_type)
        widths, depths = as_list(main_ch, rate_level), as_list(depth, rate_level)
        self.discriminator_list = nn.ModuleList(
            DiscriminatorHead(out_ch, build_channel_dict(img_size, in_ch, ch, ch * 8), img_size, depths[i], norm_type)
            for i, ch in enumerate(widths))

    def forward(self, input, rate_ind, **kwargs):
        return self.discriminator_list[_rate_index(rate_ind)](to_image_nhwc(input))

    def partition_modules(self):
        return list(self.discriminator_list)

    def partitions_for(self, q):
        return [_rate_index(q)]


@DISCRIMINATOR_REGISTRY.register()
class MultirateSharedRateCondClic21GvaeDiscriminator(BaseDiscriminator):
    """One discriminator that reads the rate as one-hot planes behind the image"""

    def __init__(self, rate_level: int, in_ch: int = 3, out_ch: int = 1, main_ch: int = 64, img_size: int = 256, norm_type: str = "none",
                 depth: int = 4, rate_cond_policy: str = "onehot"):
        super().__init__()
        _check_norm(norm_type)
        assert rate_cond_policy in ["onehot"]
        self.rate_cond_policy, self.rate_level = rate_cond_policy, rate_level
        self.net = DiscriminatorHead(out_ch, build_channel_dict(img_size, in_ch + rate_level, main_ch, main_ch * 8), img_size, depth, norm_type)

    def forward(self, input, rate_ind, **kwargs):
        return self.net(cat_onehot_nhwc(to_image_nhwc(input), _rate_index(rate_ind), self.rate_level))

    def partition_modules(self):
        return [self.net]

    def partitions_for(self, q):
        return [0]
