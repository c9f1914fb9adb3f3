"""Relativistic-average GAN step (src/trainer/ragan_rate_distortion_trainer.py:11-92): each logit against the MEAN of the other side.
  G: adv = [gan_loss(D(x)^ - mean D(x_hat), fake) + gan_loss(D(x_hat) - mean D(x)^, real)] / 2           (:32-37), ^ = detached
  D: l_d_real = 1/2 gan_loss(D(x) - mean D(x_hat)^, real, disc),  l_d_fake = 1/2 gan_loss(D(x_hat) - mean D(x)^, fake, disc)   (:70-78)
In the generator phase the centred operand of the first term carries the gradient: crdr_gan_loss_bwd spreads -(sum dp) / n over it.
The mean stays on the device (crdr_gan_loss_fwd's stats), so the step captures into HIP graphs like the others.
Segments, graph capture, `reuse_d_forward` and the spectral-norm counts: gan_rate_distortion_trainer.py."""
from __future__ import annotations

from crdr_amd.utils.registry import TRAINER_REGISTRY

from .gan_rate_distortion_trainer import GANRateDistortionTrainer


@TRAINER_REGISTRY.register()
class RaGANRateDistortionTrainer(GANRateDistortionTrainer):
    REAL_IN_G = True

    def _adv_generator(self, real_d, fake_g):
        gl = self.gan_loss
        return (gl.forward_centered(real_d, fake_g, is_real=False, is_disc=False)
                + gl.forward_centered(fake_g, real_d, is_real=True, is_disc=False)) / 2

    def _adv_discriminator(self, real_d, fake_d):
        gl = self.gan_loss
        return (gl.forward_centered(real_d, fake_d.detach(), is_real=True, is_disc=True) * 0.5,
                gl.forward_centered(fake_d, real_d.detach(), is_real=False, is_disc=True) * 0.5)
