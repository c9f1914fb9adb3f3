"""CPU-side checks of the GAN objectives (no GPU): the float64 restatement tests/gan_loss_ref.py -- which the GPU tests hold the kernels
and the trainers to -- equals the reference's own classes and steps as recorded in tests/golden/reference_gan_loss.npz to 1e-12, and
torch's BCEWithLogitsLoss / relu compositions; the five loss classes and the four trainers are registered, with the reference's
constructor and call arguments."""
import ast
import inspect
import os

import numpy as np
import pytest
import torch

from tests import gan_loss_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-12
SIDES = {"d_real": (True, True), "d_fake": (False, True), "g_real": (True, False), "g_fake": (False, False)}
LOSS_NAMES = ("VanillaGANLoss", "MaskedVanillaGANLoss", "MultiscaleVanillaGANLoss", "HingeGANLoss", "MultiscaleHingeGANLoss")
TRAINER_NAMES = ("GANRateDistortionTrainer", "RGANRateDistortionTrainer", "BetaCondRGANRateDistortionTrainer", "RaGANRateDistortionTrainer")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "reference_gan_loss.npz"))


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def near(what, got, ref):
    got, ref = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(ref, dtype=torch.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    e = (got - ref).abs().max().item()
    assert e <= TOL * max(1.0, ref.abs().max().item()), (what, e)


def _ctor_kwargs(gold):
    return ast.literal_eval(str(gold["meta.ctor_kwargs"]))   # a dict literal of numbers


@pytest.mark.parametrize("name", LOSS_NAMES)
def test_restated_classes_equal_the_reference(gold, name):
    kw = _ctor_kwargs(gold)[name]
    multi = name.startswith("Multiscale")
    seen = 0
    for side, (is_real, is_disc) in SIDES.items():
        key = f"loss.{name}.{side}"
        if key + ".value" not in gold.files:
            assert "Hinge" in name and side == "g_fake"   # the class refuses it
            continue
        xs = [t64(gold[f"{key}.x{i}"]).requires_grad_(True) for i in range(2)] if multi else [t64(gold[key + ".x"]).requires_grad_(True)]
        extra = {"mask": t64(gold[key + ".mask"])} if name == "MaskedVanillaGANLoss" else {}
        v = R.LOSSES[name](xs if multi else xs[0], is_real, is_disc, **kw, **extra)
        v.backward()
        near(key + " value", v.detach(), t64(gold[key + ".value"]))
        for i, x in enumerate(xs):
            near(f"{key} dx{i}", x.grad, t64(gold[f"{key}.dx{i}" if multi else key + ".dx"]))
        seen += 1
    assert seen >= 3


@pytest.mark.parametrize("form", ["plain", "paired", "centred"])
def test_restated_kernel_formulas_equal_the_reference_forms(gold, form):
    """sum / n and the closed-form dp, dq of the kernel contract against VanillaGANLoss on a, a - b and a - mean(b)"""
    w = float(gold["meta.loss_weight"])
    for side, (is_real, is_disc) in SIDES.items():
        key = f"form.{form}.{side}"
        a = t64(gold[key + ".a"])
        b = None if form == "plain" else t64(gold[key + ".b"])
        scale = (1.0 if is_disc else w) / a.numel()
        kw = dict(kind=R.BCE, target=1.0 if is_real else 0.0, center=form == "centred")
        near(key + " value", R.gan_loss_sum(a, b, **kw) * scale, t64(gold[key + ".value"]))
        dp, dq = R.gan_loss_grads(a, b, g=scale, **kw)
        near(key + " da", dp, t64(gold[key + ".da"]))
        if b is not None:
            near(key + " db", dq, t64(gold[key + ".db"]))


@pytest.mark.parametrize("step", R.STEPS)
def test_restated_step_algebra_equals_the_reference_trainers(gold, step):
    """from the recorded logits D(x), D(x_hat): the generator's adversarial term, the total it back-propagated, the discriminator's terms"""
    w, beta = float(gold["meta.loss_weight"]), float(gold["meta.beta"])
    loss = lambda x, is_real, is_disc: R.vanilla(x, is_real, is_disc, loss_weight=w)   # noqa: E731
    real_d, fake_d = t64(gold[f"step.{step}.real_d"]), t64(gold[f"step.{step}.fake_d"])
    log = {k[len(f"step.{step}.log."):]: t64(gold[k]) for k in gold.files if k.startswith(f"step.{step}.log.")}
    assert set(log) == {"qbpp", "distortion", "rate", "perceptual", "adv", "d_real", "d_fake", "d_total", "out_d_real", "out_d_fake"}
    adv = R.step_adv(step, loss, real_d, fake_d)
    near(f"{step} adv", adv, log["adv"])
    terms = {"distortion": log["distortion"], "adv": adv, "rate": log["rate"], "perceptual": log["perceptual"]}
    near(f"{step} total", R.step_total(step, terms, beta), t64(gold[f"step.{step}.l_total"]))
    for k, v in R.step_d(step, loss, real_d, fake_d).items():
        near(f"{step} {k}", v, log[k])
    assert int(gold[f"step.{step}.power_iterations"]) == (3 if step == "gan" else 5)   # the counts the trainers' docstring states


def test_restatement_equals_torch_compositions():
    x = R.logits("host.x", 301).double()
    y = R.logits("host.y", 301, 2.0).double()
    m = (R.logits("host.m", 301) > 0).double() * 0.5
    for t in (0.0, 1.0, 0.9, 0.1):
        bce = torch.nn.BCEWithLogitsLoss(reduction="none")
        near(f"bce terms t={t}", R.terms(x, R.BCE, t), bce(x, torch.full_like(x, t)))
        near(f"bce paired t={t}", R.gan_loss_sum(x, y, kind=R.BCE, target=t), bce(x - y, torch.full_like(x, t)).sum())
        near(f"bce centred t={t}", R.gan_loss_sum(x, y[:77], kind=R.BCE, target=t, center=True), bce(x - y[:77].mean(), torch.full_like(x, t)).sum())
        near(f"bce masked t={t}", R.gan_loss_sum(x, kind=R.BCE, target=t, mask=m), (bce(x, torch.full_like(x, t)) * m).sum())
        xg = x.clone().requires_grad_(True)
        bce(xg, torch.full_like(x, t)).sum().backward()
        near(f"bce slope t={t}", R.slope(x, R.BCE, t), xg.grad)
    for sgn in (1.0, -1.0):
        near(f"hinge terms {sgn}", R.terms(x, R.HINGE_D, sgn=sgn), torch.relu(1 - sgn * x))
        xg = x.clone().requires_grad_(True)
        torch.relu(1 - sgn * xg).sum().backward()
        near(f"hinge slope {sgn}", R.slope(x, R.HINGE_D, sgn=sgn), xg.grad)
    near("hinge at the kink", R.slope(torch.tensor([1.0], dtype=torch.float64), R.HINGE_D, sgn=1.0), torch.zeros(1, dtype=torch.float64))
    near("hinge G", R.gan_loss_sum(x, y, kind=R.HINGE_G), -(x - y).sum())
    # closed-form gradients against autograd, centred form with a mask
    xg, yg = x.clone().requires_grad_(True), y[:77].clone().requires_grad_(True)
    (0.37 * R.gan_loss_sum(xg, yg, kind=R.BCE, target=0.9, center=True, mask=m)).backward()
    dp, dq = R.gan_loss_grads(x, y[:77], kind=R.BCE, target=0.9, center=True, mask=m, g=0.37)
    near("closed-form dp", dp, xg.grad)
    near("closed-form dq", dq, yg.grad)


def test_seeded_cases_stay_off_the_hinge_kinks():
    for n in (1, 63, 257, 4099):
        for form, nq in (("none", None), ("paired", None), ("centred", 1), ("centred", 300)):
            p, q, _ = R.case(n, form, nq)
            x = R.argument(p.double(), None if q is None else q.double(), form == "centred")
            assert R.kink_count(x) == 0, (n, form, nq)


def test_losses_and_trainers_are_registered():
    """fails before this change: four of the five losses and three of the four trainers did not exist"""
    from crdr_amd.losses import build_loss  # noqa: F401  (imports every *_loss.py)
    from crdr_amd.trainer import build_trainer  # noqa: F401
    from crdr_amd.utils.registry import LOSS_REGISTRY, TRAINER_REGISTRY
    for n in LOSS_NAMES:
        assert LOSS_REGISTRY.get(n).__name__ == n
    for n in TRAINER_NAMES:
        assert TRAINER_REGISTRY.get(n).__name__ == n
    from crdr_amd.trainer.gan_rate_distortion_trainer import GANRateDistortionTrainer
    from crdr_amd.trainer.rate_distortion_trainer import RateDistortionTrainer
    assert GANRateDistortionTrainer._optimize_parameters is not RateDistortionTrainer._optimize_parameters, \
        "GANRateDistortionTrainer still runs the plain rate-distortion step"
    from crdr_amd.trainer.multirate_hr_rgan_beta_cond_rate_distortion_trainer import MultirateBetaCondHrrGanRateDistortionTrainer as S3
    for m in ("_g_forward", "_seg_generator", "_seg_dfwdbwd", "_seg_dstep", "_optimize_parameters", "_conditions"):
        owner = next(c for c in S3.__mro__ if m in vars(c))
        assert owner not in (GANRateDistortionTrainer, RateDistortionTrainer), f"the stage-3 trainer would take {m} from the single-rate step"


def test_the_multirate_trainer_without_a_step_refuses_to_train():
    """MultirateHighRateRGANRateDistortionTrainer is registered (the stage-3 trainer's base) but its own step -- the high-rate relativistic
    objective without beta -- is not built: it must not run the vanilla step it inherits under that name"""
    from crdr_amd.trainer.gan_rate_distortion_trainer import GANRateDistortionTrainer
    from crdr_amd.trainer.multirate_hr_rgan_rate_distortion_trainer import MultirateHighRateRGANRateDistortionTrainer as M
    assert M._optimize_parameters is not GANRateDistortionTrainer._optimize_parameters
    with pytest.raises(NotImplementedError, match="not built"):
        M._optimize_parameters(object.__new__(M), 1, {})


def test_masked_loss_refuses_a_mask_that_does_not_broadcast_to_the_logits():
    from crdr_amd.losses.gan_loss import MaskedVanillaGANLoss
    with pytest.raises(ValueError, match="does not broadcast"):
        MaskedVanillaGANLoss(loss_weight=1.0)(torch.zeros(2, 1, 3, 3), is_real=True, mask=torch.ones(2, 4, 3, 3))


def _arg_names(fn):
    ps = [p for n, p in inspect.signature(fn).parameters.items() if n != "self"]
    return [("**" + p.name) if p.kind is p.VAR_KEYWORD else p.name if p.default is p.empty else f"{p.name}={p.default!r}" for p in ps]


@pytest.mark.parametrize("name", LOSS_NAMES)
def test_constructor_and_call_arguments_match_the_reference(gold, name):
    from crdr_amd.losses import build_loss
    from crdr_amd.utils.registry import LOSS_REGISTRY
    cls = LOSS_REGISTRY.get(name)
    assert _arg_names(cls.__init__) == [str(s) for s in gold[f"meta.ctor.{name}"]]
    assert _arg_names(cls.forward) == [str(s) for s in gold[f"meta.forward.{name}"]]
    m = build_loss({"type": name, **_ctor_kwargs(gold)[name]})
    assert m.lamb_gan == float(gold["meta.loss_weight"])
    if "Hinge" in name:
        with pytest.raises(AssertionError):   # the generator side is defined for is_real only
            m([torch.zeros(1)] if name.startswith("Multiscale") else torch.zeros(1), is_real=False, is_disc=False)
