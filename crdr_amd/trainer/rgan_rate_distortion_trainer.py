"""Relativistic GAN step (src/trainer/rgan_rate_distortion_trainer.py:10-91): the losses are taken of logit differences.
  G: adv = [gan_loss(D(x)^ - D(x_hat), fake) + gan_loss(D(x_hat) - D(x)^, real)] / 2                     (:34-39), ^ = detached
  D: l_d_real = 1/2 gan_loss(D(x) - D(x_hat)^, real, disc),  l_d_fake = 1/2 gan_loss(D(x_hat) - D(x)^, fake, disc)   (:69-77)
The reference back-propagates the two discriminator terms one after the other; their gradients add up to those of the sum taken here.
Segments, graph capture, `reuse_d_forward` and the spectral-norm counts: gan_rate_distortion_trainer.py."""
from __future__ import annotations

from crdr_amd.utils.registry import TRAINER_REGISTRY

from .gan_rate_distortion_trainer import GANRateDistortionTrainer


@TRAINER_REGISTRY.register()
class RGANRateDistortionTrainer(GANRateDistortionTrainer):
    REAL_IN_G = True

    def _adv_generator(self, real_d, fake_g):
        gl = self.gan_loss
        return (gl.forward_diff(real_d, fake_g, is_real=False, is_disc=False) + gl.forward_diff(fake_g, real_d, is_real=True, is_disc=False)) / 2

    def _adv_discriminator(self, real_d, fake_d):
        gl = self.gan_loss
        return (gl.forward_diff(real_d, fake_d.detach(), is_real=True, is_disc=True) * 0.5,
                gl.forward_diff(fake_d, real_d.detach(), is_real=False, is_disc=True) * 0.5)
