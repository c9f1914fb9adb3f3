"""Multi-rate "high-rate relativistic GAN" trainer base: the relative score image is the no-grad reconstruction
one rate level up (src/trainer/multirate_hr_rgan_rate_distortion_trainer.py:11-14).

Only the beta-conditioned subclass (stage 3) has a step here.  The reference's step of THIS class -- the high-rate relativistic objective of
a multi-rate model without beta -- is not built, so the class refuses to train instead of running the vanilla step it would inherit
from GANRateDistortionTrainer under another objective's name."""
from __future__ import annotations

from crdr_amd.utils.registry import TRAINER_REGISTRY

from .gan_rate_distortion_trainer import GANRateDistortionTrainer


@TRAINER_REGISTRY.register()
class MultirateHighRateRGANRateDistortionTrainer(GANRateDistortionTrainer):
    def __init__(self, opt, relative_score_rate_delta=1) -> None:
        super().__init__(opt)
        self.rate_level = self.comp_model.rate_level
        self.relative_score_rate_delta = relative_score_rate_delta

    def _optimize_parameters(self, current_iter: int, data_dict):
        raise NotImplementedError(
            f"{type(self).__name__}: the high-rate relativistic step without beta conditioning is not built; use "
            "MultirateBetaCondHrrGanRateDistortionTrainer (stage 3), or RGANRateDistortionTrainer for a relativistic step against the real image")
