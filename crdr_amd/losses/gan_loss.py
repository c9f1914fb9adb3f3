"""GAN losses on discriminator logits (src/losses/gan_loss.py:10-112).

VanillaGANLoss: non-saturating loss, BCE-with-logits against a constant label, mean over logits; the generator-side value carries the
loss weight (:10-31).  `forward_diff(p, q, ...)` evaluates the loss of the logit difference p - q (the relativistic form) in one fused
reduction, `forward_centered(p, q, ...)` that of p - mean(q) (the relativistic-average form).
MaskedVanillaGANLoss (:34-53): the per-logit loss times a mask before the mean; the mask must broadcast to the logits' shape.  MultiscaleVanillaGANLoss (:57-81): a list of logit
maps, the mean over scales.  HingeGANLoss (:84-103): relu(1 -/+ x) for the discriminator, -mean(x) for the generator.
MultiscaleHingeGANLoss (:106-112): the sum over scales.  The four added classes run on crdr_gan_loss_fwd / _bwd (hip.functional.gan_loss_sum)."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from crdr_amd.hip import functional as HF
from crdr_amd.utils.registry import LOSS_REGISTRY


def _mean(total: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    return (total / x.numel()).reshape(())


@LOSS_REGISTRY.register()
class VanillaGANLoss(nn.Module):
    def __init__(self, loss_weight: float, real_label: float = 1.0, fake_label: float = 0.0, loss_reduction: str = "mean"):
        super().__init__()
        assert loss_reduction == "mean"
        self.lamb_gan = loss_weight
        self.real_label_val, self.fake_label_val = real_label, fake_label

    def forward_diff(self, p, q, is_real: bool, is_disc: bool = False):
        target = self.real_label_val if is_real else self.fake_label_val
        loss = (HF.bce_diff_sum(p, q, target) / p.numel()).reshape(())
        return loss if is_disc else self.lamb_gan * loss

    def forward_centered(self, p, q, is_real: bool, is_disc: bool = False):
        """The loss of p - mean(q) (ragan_rate_distortion_trainer.py:35-36, 72-77); q may carry a gradient and may differ from p in size."""
        target = self.real_label_val if is_real else self.fake_label_val
        loss = _mean(HF.gan_loss_sum(p, q, kind=HF.GAN_BCE, target=target, center=True), p)
        return loss if is_disc else self.lamb_gan * loss

    def forward(self, x, is_real: bool, is_disc: bool = False, **kwargs):
        return self.forward_diff(x, torch.zeros_like(x), is_real, is_disc)


@LOSS_REGISTRY.register()
class MaskedVanillaGANLoss(VanillaGANLoss):
    def __init__(self, loss_weight: float, real_label: float = 1.0, fake_label: float = 0.0):
        super().__init__(loss_weight, real_label, fake_label)

    def forward(self, x: torch.Tensor, is_real: bool, mask: Optional[torch.Tensor] = None, is_disc: bool = False, **kwargs):
        target = self.real_label_val if is_real else self.fake_label_val
        mask = mask if isinstance(mask, torch.Tensor) else None
        if mask is not None and torch.broadcast_shapes(mask.shape, x.shape) != x.shape:
            # (the reference's `loss * mask` would grow to the mask's shape and average over that)
            raise ValueError(f"MaskedVanillaGANLoss: a mask of shape {tuple(mask.shape)} does not broadcast to the logits' {tuple(x.shape)}")
        loss = _mean(HF.gan_loss_sum(x, kind=HF.GAN_BCE, target=target, mask=mask), x)
        return loss if is_disc else self.lamb_gan * loss


@LOSS_REGISTRY.register()
class MultiscaleVanillaGANLoss(nn.Module):
    def __init__(self, loss_weight: float):
        super().__init__()
        self.lamb_gan = loss_weight

    def forward(self, x, is_real: bool, is_disc: bool = False, **kwargs):
        assert isinstance(x, list)
        loss = 0.
        for feat in x:
            loss = loss + _mean(HF.gan_loss_sum(feat, kind=HF.GAN_BCE, target=1.0 if is_real else 0.0), feat)
        loss = loss / len(x)
        return loss if is_disc else self.lamb_gan * loss


@LOSS_REGISTRY.register()
class HingeGANLoss(nn.Module):
    def __init__(self, loss_weight: float) -> None:
        super().__init__()
        self.lamb_gan = loss_weight

    def forward_diff(self, p, q, is_real: bool, is_disc: bool = False):
        """The hinge loss of the logit difference p - q (q = None: of p)."""
        if is_disc:
            return _mean(HF.gan_loss_sum(p, q, kind=HF.GAN_HINGE_D, sgn=1.0 if is_real else -1.0), p)
        assert is_real, 'For G loss `is_real` should be True'
        return self.lamb_gan * _mean(HF.gan_loss_sum(p, q, kind=HF.GAN_HINGE_G), p)

    def forward_centered(self, p, q, is_real: bool, is_disc: bool = False):
        """The hinge loss of p - mean(q)."""
        if is_disc:
            return _mean(HF.gan_loss_sum(p, q, kind=HF.GAN_HINGE_D, sgn=1.0 if is_real else -1.0, center=True), p)
        assert is_real, 'For G loss `is_real` should be True'
        return self.lamb_gan * _mean(HF.gan_loss_sum(p, q, kind=HF.GAN_HINGE_G, center=True), p)

    def forward(self, x, is_real: bool, is_disc: bool = False, **kwargs):
        return self.forward_diff(x, None, is_real, is_disc)


@LOSS_REGISTRY.register()
class MultiscaleHingeGANLoss(HingeGANLoss):
    def forward(self, x, is_real: bool, is_disc: bool = False, **kwargs):
        return sum(super(MultiscaleHingeGANLoss, self).forward(feat, is_real=is_real, is_disc=is_disc) for feat in x)
