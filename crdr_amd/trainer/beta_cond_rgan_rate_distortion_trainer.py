"""Relativistic GAN step of a beta-conditioned multi-rate model against ONE discriminator
(src/trainer/beta_cond_rgan_rate_distortion_trainer.py:10-98): the RGAN terms, weighted like stage 3,
  L = distortion + rate + beta (adv + perceptual)                                                            (:48)
with (q, beta) drawn once per batch; the perceptual loss is required (:35).  The draw and the device buffers beta enters through are
the stage-3 trainer's (beta_conditions.py: the graph key is the rate index; beta is data).
Segments, graph capture, `reuse_d_forward` and the spectral-norm counts: gan_rate_distortion_trainer.py."""
from __future__ import annotations

from typing import Dict

from crdr_amd.utils.registry import TRAINER_REGISTRY

from .beta_conditions import BetaConditions
from .rgan_rate_distortion_trainer import RGANRateDistortionTrainer


@TRAINER_REGISTRY.register()
class BetaCondRGANRateDistortionTrainer(BetaConditions, RGANRateDistortionTrainer):
    def __init__(self, opt, **kwargs) -> None:
        super().__init__(opt, **kwargs)
        assert self.perceptual_loss is not None, "BetaCondRGANRateDistortionTrainer needs loss.perceptual_loss"
        self._init_conditions(opt)

    def _conditions(self, data_dict: Dict):
        cond, key = super()._conditions(data_dict)
        return {"rate_ind": float(cond["rate_ind"]), "beta": cond["beta"]}, key

    def run_comp_model(self, data_dict: Dict):
        real, fake, bpp, other = super().run_comp_model(data_dict)
        other.pop("beta")   # (:25) the weight enters the total through the device scalar _beta_t
        return real, fake, bpp, other

    def _total_loss(self, terms: Dict, rate):
        return terms["distortion"] + rate + self._beta_t * (terms["adv"] + terms["perceptual"])
