"""Single-rate adversarial training: the discriminator, its optimiser, the GAN loss, and the vanilla step
(src/trainer/gan_rate_distortion_trainer.py:17-227; the step is :46-119).

Per iteration:
  G: x_hat = G(x);  L = distortion + rate (+ perceptual) + adv,  adv = gan_loss(D(x_hat), real)   (D frozen);  clip, Adam; aux Adam.
  D: L_D = 1/2 gan_loss(D(x), real, disc) + 1/2 gan_loss(D(x_hat)^, fake, disc),  ^ = detached;  Adam.
The relativistic subclasses (rgan_ / ragan_ / beta_cond_rgan_rate_distortion_trainer.py) replace two hooks -- `_adv_generator`, the
generator's term from (D(x) without grad, D(x_hat)), and `_adv_discriminator`, the two discriminator terms from (D(x), D(x_hat)^) -- and,
for the beta-conditioned one, the weighting of the total.  Everything else is shared.

Segments (each one HIP graph per condition key, like the stage-3 trainer): `g` generator forward, losses, backward; `dfb` discriminator
forward + backward, run BEFORE the generator update (D reads x and x_hat^ only, not G's parameters: the same computation as the
reference's order, see the stage-3 trainer's _seg_dfwdbwd); `u` generator + aux update; `d` discriminator update.  A NaN / Inf / huge
generator loss sets the device-side flag that makes all three optimisers skip (the reference returns before any update).

`reuse_d_forward` (default on; opt key, or CRDR_REUSE_D_FORWARD=0): the discriminator weights do not change between the two phases,
so a chain-built discriminator (CLIC21GVAEDiscriminator, norm_type none) keeps the generator phase's forward(s) and the discriminator
phase back-propagates through them; any other discriminator runs the discriminator phase as one pass over [x_hat; x] (none of the
discriminators here has batch statistics).  Off: two separate passes, D(x) then D(x_hat), as the reference orders them.
With a spectral-norm discriminator (HiFiCDiscriminator, use_sn -- NOT chain-built, so "reuse on" is the one pass over [x_hat; x])
every training-mode forward runs one power iteration, so the number of u / v updates per step differs from the reference's:
                                                                  reference   reuse on   reuse off
    vanilla (G: D(x_hat);  D: D(x), D(x_hat))                          3          2           3
    relativistic (G: D(x), D(x_hat);  D: D(x_hat), D(x), D(x_hat))     5          3           4
(same fixed point).  Data parallel: the AsyncGradSync calls of the stage-3 trainer on its non-staged path; no machine with more than
one rank has run these four trainers."""
from __future__ import annotations

import os
from copy import deepcopy
from typing import Dict, Optional

import torch

from crdr_amd.hip import chain as _chain
from crdr_amd.losses import build_loss
from crdr_amd.models.discriminator import build_discriminator
from crdr_amd.utils.path import PathHandler
from crdr_amd.utils.registry import TRAINER_REGISTRY

from . import dist as D
from .optimizer import build_optimizer, build_scheduler
from .rate_distortion_trainer import RateDistortionTrainer


@TRAINER_REGISTRY.register()
class GANRateDistortionTrainer(RateDistortionTrainer):
    REAL_IN_G = False   # whether the generator's adversarial term reads D(x)

    def __init__(self, opt, **kwargs) -> None:
        super().__init__(opt, **kwargs)
        self.reuse_d_forward = bool(opt.get("reuse_d_forward", os.environ.get("CRDR_REUSE_D_FORWARD", "1") != "0"))

    def _set_models(self) -> None:
        super()._set_models()
        self.discriminator = build_discriminator(self.opt.discriminator).to(self.device)
        D.broadcast_module_(self.discriminator)
        self.discriminator.train()

    def _set_losses(self) -> None:
        super()._set_losses()
        self.gan_loss = build_loss(deepcopy(self.opt.loss).gan_loss, loss_name="gan_loss")

    def _set_optimizer_scheduler(self) -> None:
        super()._set_optimizer_scheduler()
        oo = deepcopy(self.opt.optim)
        self.d_optimizer = build_optimizer(dict(self.discriminator.named_parameters()), oo.d_optimizer)
        if hasattr(self.discriminator, "partition_modules") and len(self.d_optimizer.param_groups) == 1:
            # a rate-aware discriminator names its own partitions (shared backbone + heads, ...) and, per rate, the ones a step trains
            # (partitions_for): multirate_clic21_gvae_discriminator.py
            self.d_optimizer.set_partitions(self.discriminator.partition_modules())
        elif hasattr(self.discriminator, "subD_list") and len(self.d_optimizer.param_groups) == 1:
            # one partition per sub-discriminator: only the one a step ran is zeroed / all-reduced / updated, like
            # torch.optim.Adam skipping the parameters whose .grad is None (module_list_discriminator.py:26-30)
            self.d_optimizer.set_partitions(self.discriminator.subD_list)
        self.d_scheduler = build_scheduler(self.d_optimizer, oo.d_scheduler) if oo.get("d_scheduler") else None

    # ------------------------------------------------------------------ the two hooks
    def _adv_generator(self, real_d, fake_g):
        """The generator's adversarial term; real_d = D(x) without grad (None unless REAL_IN_G)."""
        return self.gan_loss(fake_g, is_real=True, is_disc=False)

    def _adv_discriminator(self, real_d, fake_d):
        """-> (l_d_real, l_d_fake), each with its factor 1/2."""
        return (self.gan_loss(real_d, is_real=True, is_disc=True) * 0.5, self.gan_loss(fake_d, is_real=False, is_disc=True) * 0.5)

    def _total_loss(self, terms: Dict, rate):
        return sum(terms.values()) + rate

    # ------------------------------------------------------------------ G phase: forward, losses, backward
    def _d_keep(self, img, d_kwargs: Dict, on: bool):
        """-> (D(img), the chain handle of that pass or None): with `on`, a chain-built discriminator keeps its activations for a later
        backward (hip/chain.py KEEP_HANDLES)"""
        if on:
            _chain.KEEP_HANDLES = []
        try:
            out = self.discriminator(img, **d_kwargs)
        finally:
            handles, _chain.KEEP_HANDLES = _chain.KEEP_HANDLES, None
        return out, (handles[0] if (on and handles is not None and len(handles) == 1) else None)

    def _g_forward(self, real, cond: Dict, noise, current_iter: int) -> Dict:
        self.discriminator.requires_grad_(False)
        self.g_optimizer.zero_grad()
        if self.aux_optimizer:
            self.aux_optimizer.zero_grad()
        data = {"real_images": real, **cond}
        if noise is not None:
            data["noise"] = noise
        real_p, fake, bpp, other = self.run_comp_model(data)
        terms = {"distortion": self.distortion_loss(real_p, fake, **other)}
        if self.perceptual_loss:
            terms["perceptual"] = self.perceptual_loss(real_p, fake)
        keep = self.reuse_d_forward
        real_d, d_real_handle = None, None
        if self.REAL_IN_G:
            with torch.no_grad():
                real_d, d_real_handle = self._d_keep(real_p, other, keep)
        fake_g, d_handle = self._d_keep(fake, other, keep)
        terms["adv"] = self._adv_generator(real_d, fake_g)
        d_kwargs = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in other.items()}
        return {"bpp": bpp, "other": other, "terms": terms,
                "extra": {"real": real_p, "fake": fake.detach(), "d_kwargs": d_kwargs, "d_handle": d_handle, "d_real_handle": d_real_handle}}

    def _seg_generator(self, real, cond: Dict, noise, current_iter: int) -> Dict:
        f = self._g_forward(real, cond, noise, current_iter)
        other = f["other"]
        rate = self.rate_loss(f["bpp"], **other, **self._rate_kwargs(other), current_iter=current_iter)
        l_total = self._total_loss(f["terms"], rate)
        l_total.backward()
        self._flush_wgrads("g")
        return {"losses": {**f["terms"], "rate": rate}, "bad": self._bad_flag(l_total), "qbpp": other.get("qbpp", None), **f["extra"]}

    # ------------------------------------------------------------------ D forward + backward (needs only x and x_hat)
    D_BATCH_KEYS = ("y_hat",)   # per-sample tensors among the discriminator's keyword inputs (HiFiCConditionalDiscriminator)

    def _seg_dfwdbwd(self, ctx: Dict) -> Dict:
        kw = ctx["d_kwargs"]
        self.discriminator.requires_grad_(True)
        self.d_optimizer.zero_grad()
        if ctx.get("d_handle") is not None:
            # D(x_hat): the generator phase's forward (same weights, same input) -- nothing is launched, the backward runs on its activations
            fake_d = _chain.run_chain_reuse(ctx["d_handle"])[0]
            real_d = (_chain.run_chain_reuse(ctx["d_real_handle"])[0] if ctx.get("d_real_handle") is not None
                      else self.discriminator(ctx["real"], **kw))
        elif self.reuse_d_forward:
            both_kw = {k: (torch.cat([v, v], dim=0) if k in self.D_BATCH_KEYS else v) for k, v in kw.items()}
            both = self.discriminator(torch.cat([ctx["fake"], ctx["real"]], dim=0), **both_kw)
            fake_d, real_d = both[: both.shape[0] // 2], both[both.shape[0] // 2:]
        else:
            real_d = self.discriminator(ctx["real"], **kw)
            fake_d = self.discriminator(ctx["fake"], **kw)
        l_d_real, l_d_fake = self._adv_discriminator(real_d, fake_d)
        (l_d_real + l_d_fake).backward()
        self._flush_wgrads("d")
        return {"d_real": l_d_real, "d_fake": l_d_fake, "d_total": l_d_real + l_d_fake,
                "out_d_real": real_d.detach().mean(), "out_d_fake": fake_d.detach().mean()}

    def _seg_dstep(self, ctx: Dict) -> Dict:
        self.d_optimizer.step(skip=ctx["bad"])
        return {}

    def _optimize_parameters(self, current_iter: int, data_dict: Dict):
        data_dict = dict(data_dict)
        noise = data_dict.pop("noise", None)
        real = self._stage_input(data_dict["real_images"])
        cond, key = self._conditions(data_dict)
        scheduled = bool(getattr(self.rate_loss, "lambda_schedule", None) or getattr(self.rate_loss, "target_rate_schedule", None))
        run = self._runner(("gan", key), allow_graph=not scheduled)  # explicit noise tensors must be persistent device buffers
        self.g_optimizer.sync_lr_to_device()
        self.d_optimizer.sync_lr_to_device()
        ctx = run("g", lambda: self._seg_generator(real, cond, noise, current_iter))
        g_sync = D.AsyncGradSync(self.g_optimizer.flat_grads(), [ctx["bad"]], label="g.all")   # overlaps the D forward/backward
        ctx_d = run("dfb", lambda: self._seg_dfwdbwd(ctx))
        d_sync = D.AsyncGradSync(self.d_optimizer.flat_grads(), label="d")   # overlaps the G update
        g_sync.wait()
        ctx2 = run("u", lambda: self._seg_update(ctx))
        d_sync.wait()
        run("d", lambda: self._seg_dstep(ctx))
        log = {"qbpp": ctx["qbpp"] if ctx["qbpp"] is not None else -1, **ctx["losses"], **ctx2, **ctx_d, "_bad": ctx["bad"]}
        return self._finish_step(current_iter, log)

    def _finish_step(self, current_iter: int, log):
        vals = super()._finish_step(current_iter, log)
        if vals is not None and self.d_scheduler:
            self.d_scheduler.step()
        return vals

    def _training_state(self) -> Dict:
        st = super()._training_state()
        st["d_optimizer"] = self.d_optimizer
        if self.d_scheduler:
            st["d_scheduler"] = self.d_scheduler
        return st

    def save(self, current_iter: int) -> None:
        self.model_saver.save({"comp_model": self.comp_model}, "comp_model", current_iter, keep=True)
        self.model_saver.save({"discriminator": self.discriminator}, "discriminator", current_iter, keep=self.opt.get("keep_discriminator", False))
        self.model_saver.save(self._training_state(), "training_state", current_iter, keep=self.opt.get("keep_training_state", False))

    def _load_checkpoint(self, exp: str, itr: int, load_optimizer: bool = True, load_discriminator: bool = True,
                         load_scheduler: bool = True, new_g_lr: Optional[float] = None, new_d_lr: Optional[float] = None,
                         strict: bool = True, **kwargs) -> None:
        super()._load_checkpoint(exp, itr, load_optimizer=load_optimizer, load_scheduler=load_scheduler, new_g_lr=new_g_lr, strict=strict)
        if not load_discriminator:
            return
        ph = PathHandler(self.opt.path.ckpt_root, exp)
        self.discriminator.load_state_dict(torch.load(ph.get_ckpt_path("discriminator", itr), map_location="cpu")["discriminator"], strict=strict)
        if load_optimizer:
            st = torch.load(ph.get_ckpt_path("training_state", itr), map_location="cpu")
            self.d_optimizer.load_state_dict(st["d_optimizer"])
            if new_d_lr is not None:
                self.update_learning_rate(self.d_optimizer, new_d_lr)
            if self.d_scheduler and load_scheduler:
                self.d_scheduler.load_state_dict(st["d_scheduler"])
