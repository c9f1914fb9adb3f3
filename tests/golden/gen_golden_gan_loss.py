"""Golden vectors of the reference's GAN losses and of the loss algebra of its four single-rate adversarial steps, same rules as
gen_golden_channel_norm.py: the reference's own classes (src/losses/gan_loss.py:10-112) are run under install_stubs() on seeded logits,
in float64 on the CPU; only inputs, values and logit gradients are stored, plus the argument names (and defaults) of each class's constructor and call.

  loss.<Class>.<side>.*   one call per (is_real, is_disc) the class accepts: x (a list x0, x1 for the multiscale classes; mask for the
                          masked one), value, dx
  form.<form>.<side>.*    VanillaGANLoss on a - b (`paired`) and a - mean(b) (`centred`, b of another size) as the relativistic trainers
                          call it, and on a alone (`plain`): a, b, value, da, db
  step.<step>.*           the reference trainer modules DO import under the stubs, so each optimize_parameters
                          (src/trainer/{gan,rgan,ragan,beta_cond_rgan}_rate_distortion_trainer.py) also runs once on a stub `self` with tiny
                          float64 torch stand-ins for the model and the discriminator: the discriminator's logits D(x), D(x_hat) (the same
                          in both phases: its weights change only at the very end), every logged term, the total the step handed
                          its NaN check, and beta.

    python tests/golden/gen_golden_gan_loss.py      # needs the reference checkout gen_golden.REF names; writes tests/golden/reference_gan_loss.npz
"""
import inspect
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from seeded_weights import fill_module_, seeded_input  # noqa: E402

LOSS_WEIGHT = 0.37
SIDES = {"d_real": (True, True), "d_fake": (False, True), "g_real": (True, False), "g_fake": (False, False)}
CTOR = {"VanillaGANLoss": dict(loss_weight=LOSS_WEIGHT, real_label=0.9, fake_label=0.1), "MaskedVanillaGANLoss": dict(loss_weight=LOSS_WEIGHT),
        "MultiscaleVanillaGANLoss": dict(loss_weight=LOSS_WEIGHT), "HingeGANLoss": dict(loss_weight=LOSS_WEIGHT),
        "MultiscaleHingeGANLoss": dict(loss_weight=LOSS_WEIGHT)}
BETA = 1.28


def f64(t):
    return torch.as_tensor(t).detach().cpu().numpy().astype(np.float64)


def leaf(tag, shape, scale=3.0):
    return seeded_input("ganloss.gold." + tag, shape, scale).double().requires_grad_(True)


def arg_names(fn):
    """the argument names of fn, `name=default` where there is a default, `**name` for the catch-all: a list of names"""
    ps = [p for n, p in inspect.signature(fn).parameters.items() if n != "self"]
    return np.array([("**" + p.name) if p.kind is p.VAR_KEYWORD else p.name if p.default is p.empty else f"{p.name}={p.default!r}" for p in ps])


class _AttrDict(dict):
    __getattr__ = dict.__getitem__


class _G(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 3, 3, padding=1)

    def forward(self, x):
        return self.conv(x)


class _D(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1, self.conv2 = nn.Conv2d(3, 4, 3, stride=2, padding=1), nn.Conv2d(4, 1, 3, padding=1)
        self.calls = []

    def forward(self, x, **kwargs):
        o = self.conv2(nn.functional.leaky_relu(self.conv1(x), 0.2))
        self.calls.append(o.detach().clone())
        return o


def run_step(cls, gan_loss, beta_cond):
    """one optimize_parameters of the reference trainer class `cls` on a stub self -> (log dict, l_total, D calls)"""
    G, D = _G(), _D()
    fill_module_(G, "ganloss.gold.G.")
    fill_module_(D, "ganloss.gold.D.")
    G.double()
    D.double()
    seen = {}

    def run_comp_model(data):
        real = data["real_images"]
        fake = G(real)
        bpp = fake.square().mean(dim=(1, 2, 3)) + 0.5
        other = {"qbpp": bpp.detach() * 0.9}
        if beta_cond:
            other["beta"] = BETA
        return real, fake, bpp, other

    def check(l_total):
        seen["l_total"] = l_total.detach().clone()
        return False

    stub = types.SimpleNamespace(
        discriminator=D, comp_model=G, g_optimizer=torch.optim.Adam(G.parameters(), lr=1e-4), d_optimizer=torch.optim.Adam(D.parameters(), lr=1e-4),
        aux_optimizer=None, g_scheduler=None, d_scheduler=None, run_comp_model=run_comp_model,
        distortion_loss=lambda r, f, **kw: 150 * (r - f).square().mean(), rate_loss=lambda bpp, **kw: 0.1 * bpp.mean(),
        perceptual_loss=lambda r, f: 0.39 * (r - f).abs().mean(), gan_loss=gan_loss, check_loss_nan_inf=check,
        logger=types.SimpleNamespace(warning=print), opt=_AttrDict(optim=_AttrDict(clip_max_norm=1.0)),
        calc_avg_d_score_for_log=cls.calc_avg_d_score_for_log)
    x = seeded_input("ganloss.gold.image", (2, 3, 8, 8)).double()
    log = cls.optimize_parameters(stub, 1, {"real_images": x})
    assert log is not None
    return log, seen["l_total"], D.calls


def main():
    from gen_golden import REF, install_stubs
    install_stubs()
    sys.path.insert(0, REF)
    import logging
    logging.disable(logging.CRITICAL)
    from src.losses import gan_loss as RL
    out = {}

    # (i) the five classes
    for name, kw in CTOR.items():
        cls = getattr(RL, name)
        out[f"meta.ctor.{name}"], out[f"meta.forward.{name}"] = arg_names(cls.__init__), arg_names(cls.forward)
        multi = name.startswith("Multiscale")
        for side, (is_real, is_disc) in SIDES.items():
            if "Hinge" in name and not is_disc and not is_real:
                continue   # refused by the class's assert
            m = cls(**kw)
            xs = [leaf(f"{name}.{side}.x{i}", s) for i, s in enumerate(((2, 1, 5, 7), (2, 1, 3, 4)))] if multi else [leaf(f"{name}.{side}.x", (2, 1, 5, 7))]
            extra = {}
            if name == "MaskedVanillaGANLoss":
                extra["mask"] = (seeded_input(f"ganloss.gold.{side}.mask", (2, 1, 5, 7)) > 0).double() * 1.5
                out[f"loss.{name}.{side}.mask"] = f64(extra["mask"])
            v = m(xs if multi else xs[0], is_real=is_real, is_disc=is_disc, **extra)
            v.backward()
            out[f"loss.{name}.{side}.value"] = f64(v)
            for i, x in enumerate(xs):
                sfx = str(i) if multi else ""
                out[f"loss.{name}.{side}.x{sfx}"], out[f"loss.{name}.{side}.dx{sfx}"] = f64(x), f64(x.grad)
    out["meta.ctor_kwargs"] = np.array(repr(CTOR))

    # (ii) the forms the four trainers hand VanillaGANLoss
    for form in ("plain", "paired", "centred"):
        for side, (is_real, is_disc) in SIDES.items():
            m = RL.VanillaGANLoss(loss_weight=LOSS_WEIGHT)
            a = leaf(f"form.{form}.{side}.a", (2, 1, 5, 7))
            b = None if form == "plain" else leaf(f"form.{form}.{side}.b", (2, 1, 5, 7) if form == "paired" else (3, 1, 4, 4), 2.0)
            arg = a if form == "plain" else a - b if form == "paired" else a - torch.mean(b)
            v = m(arg, is_real=is_real, is_disc=is_disc)
            v.backward()
            out[f"form.{form}.{side}.a"], out[f"form.{form}.{side}.da"], out[f"form.{form}.{side}.value"] = f64(a), f64(a.grad), f64(v)
            if b is not None:
                out[f"form.{form}.{side}.b"], out[f"form.{form}.{side}.db"] = f64(b), f64(b.grad)

    # (iii) the four steps
    from src.trainer.beta_cond_rgan_rate_distortion_trainer import BetaCondRGANRateDistortionTrainer
    from src.trainer.gan_rate_distortion_trainer import GANRateDistortionTrainer
    from src.trainer.ragan_rate_distortion_trainer import RaGANRateDistortionTrainer
    from src.trainer.rgan_rate_distortion_trainer import RGANRateDistortionTrainer
    for step, cls in (("gan", GANRateDistortionTrainer), ("rgan", RGANRateDistortionTrainer), ("ragan", RaGANRateDistortionTrainer),
                      ("beta_cond_rgan", BetaCondRGANRateDistortionTrainer)):
        log, l_total, calls = run_step(cls, RL.VanillaGANLoss(loss_weight=LOSS_WEIGHT), step == "beta_cond_rgan")
        if step == "gan":   # G: D(x_hat);  D: D(x), D(x_hat)
            assert len(calls) == 3 and torch.equal(calls[0], calls[2])
            real_d, fake_d = calls[1], calls[2]
        else:               # G: D(x), D(x_hat);  D: D(x_hat), D(x), D(x_hat)
            assert len(calls) == 5 and torch.equal(calls[0], calls[3]) and torch.equal(calls[1], calls[2]) and torch.equal(calls[1], calls[4])
            real_d, fake_d = calls[3], calls[4]
        out[f"step.{step}.real_d"], out[f"step.{step}.fake_d"], out[f"step.{step}.l_total"] = f64(real_d), f64(fake_d), f64(l_total)
        out[f"step.{step}.power_iterations"] = np.array(len(calls))   # discriminator forwards per step
        for k, v in log.items():
            out[f"step.{step}.log.{k}"] = f64(v).mean()
    out["meta.loss_weight"], out["meta.beta"] = np.array(LOSS_WEIGHT), np.array(BETA)

    path = os.path.join(HERE, "reference_gan_loss.npz")
    np.savez_compressed(path, **out)
    print(sorted(k for k in out if k.startswith("step.")))
    print({k: str(v) for k, v in out.items() if k.startswith("meta.")})
    print(len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
