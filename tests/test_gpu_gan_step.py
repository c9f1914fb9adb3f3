"""One step of each single-rate adversarial trainer (bs 2, 64 x 64, seeded parameters, explicit noise) against the step written out
literally below in the reference's order: GANRateDistortionTrainer, RGANRateDistortionTrainer and RaGANRateDistortionTrainer on the stage-1
config + CLIC21GVAEDiscriminator (norm_type none) + VanillaGANLoss; BetaCondRGANRateDistortionTrainer on the stage-3 config with that single
discriminator; GANRateDistortionTrainer on the hyperprior-only model with small HificEncoder / HificDecoder, HiFiCConditionalDiscriminator
(use_sn False) and HingeGANLoss (the HiFiC recipe).

The comparison side runs on deep copies of the trainer's own modules (taken before any forward), so both sides launch the same conv
kernels; its GAN loss is torch's (binary_cross_entropy_with_logits / relu / mean on the device, `a - b` and `a - torch.mean(b)` as the
reference forms them), its backward() calls are the reference's (one per discriminator term in the relativistic steps), its optimisers
are torch.optim.Adam and clip_grad_norm_.  The two sides can differ only in the loss arithmetic and in accumulation order, so every
logged term, every generator / discriminator gradient before the optimiser and every parameter after it is held to the project's conv
gate, 2e-5 of the tensor's scale (README): max |a - b| <= 2e-5 max |b|.

The discriminator's head bias is under the same gate as every other tensor, gradient and parameter.  Its gradient is the plain sum of
the logit gradients and cancels analytically in the paired relativistic steps and in the hinge step with as many real as fake terms
active; measured, both sides hold the same bits there (profiles/gan_step_test_margins.txt).  One place has no scale to take 2e-5 of: in
the reuse on / off test of the HiFiC case the two-pass path's head-bias gradient is EXACTLY 0 (162 terms of -1/324 against 162 of
+1/324, summed pass by pass) where the one-pass path leaves the rounding residue of summing all 324 in one column sum.  A tensor
that is exactly 0 on the reference side is held to 2e-5 of the sum of the magnitudes of the terms that cancelled, sum_i |dL/dlogit_i|
<= 1 (|l'| <= 1, two factors 1/2) -- stated here and in DESIGN 13, applied to that one tensor of that one test, and printed.

The HiFiC case runs with `reuse_d_forward: false`.  Its discriminator is not chain-built, so with the option on the discriminator
phase is ONE pass over [x_hat; x] -- launches the literal step does not share (batch 4 against two passes of batch 2), which breaks the
premise of the gate.  Measured on an MI355X with the option on: every logged term and gradient still within the cap (D gradients
1.8e-6 of scale: accumulation order), but `model.6.bias` after the update at 1.4e-4 of its scale: element 111 has gradient exactly 0
in the literal step and 3.0e-9 here (3e-7 of that tensor's largest), and Adam's first step turns that residue into lr x 3.0e-9 /
(3.0e-9 + 1e-8) = 2.3e-5 against max |p| = 0.17.  That is Adam's normalisation of a gradient below the rounding noise, not a property of
the step; the one-pass path is held to the two-pass path on gradients by test_reuse_d_forward_on_and_off_give_the_same_gradients.

Each comparison prints its figure before it asserts (profiles/gan_step_test_margins.txt)."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

from tests.golden.seeded_weights import seeded_input
from tests.test_gpu_model import dev
from tests.test_gpu_step import _opt, _seed_params

pytestmark = pytest.mark.gpu
CAP = 2e-5
GAN_WEIGHT = 0.05
HEAD_BIAS = {"CLIC21GVAEDiscriminator": "model.16.bias", "HiFiCConditionalDiscriminator": "model.8.bias"}   # the last conv of each

CASES = {"gan": ("GANRateDistortionTrainer", 1, "gan"), "rgan": ("RGANRateDistortionTrainer", 1, "rgan"),
         "ragan": ("RaGANRateDistortionTrainer", 1, "ragan"), "beta_cond_rgan": ("BetaCondRGANRateDistortionTrainer", 3, "rgan"),
         "hific": ("GANRateDistortionTrainer", 1, "gan")}


def _gan_opt(case, **extra):
    trainer, stage, _ = CASES[case]
    opt = _opt(stage, 2, 64)
    opt["trainer"] = {"type": trainer}
    opt["discriminator"] = {"type": "CLIC21GVAEDiscriminator", "in_ch": 3, "out_ch": 1, "main_ch": 64, "norm_type": "none"}
    opt["loss"]["gan_loss"] = {"type": "VanillaGANLoss", "loss_weight": GAN_WEIGHT}
    opt["optim"]["d_optimizer"] = {"type": "Adam", "lr": 1e-4}
    opt["optim"].pop("d_scheduler", None)
    if case == "hific":
        from crdr_amd.utils.options import BaseConfig
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        model, _, _ = BaseConfig._file2dict_yaml(os.path.join(root, "config", "_base_", "model", "elic_hyperprior.yaml"))
        model["subnet"]["encoder"] = {"type": "HificEncoder", "in_ch": 3, "bottleneck_y": 320, "filters": [8, 12, 16, 20, 24]}
        model["subnet"]["decoder"] = {"type": "HificDecoder", "bottleneck_y": 320, "n_residual_blocks": 2, "filters": [24, 20, 16, 12, 8]}
        opt["model_type"], opt["subnet"] = model["model_type"], model["subnet"]
        opt["discriminator"] = {"type": "HiFiCConditionalDiscriminator", "in_ch": 3, "out_ch": 1, "main_ch": 16, "y_ch": 320, "latent_nc": 12,
                                "use_sn": False}
        opt["loss"]["gan_loss"] = {"type": "HingeGANLoss", "loss_weight": GAN_WEIGHT}
        opt["reuse_d_forward"] = False   # (module docstring: this discriminator is not chain-built)
    for k, v in extra.items():
        opt[k] = v
    return opt


def _build(case, **extra):
    """-> (trainer, deep copies of (comp_model, discriminator) taken before any forward)"""
    from crdr_amd.trainer import build_trainer
    tr = build_trainer(_gan_opt(case, **extra))
    _seed_params(tr.comp_model, "")
    _seed_params(tr.discriminator, "gan.D.")
    if case == "hific":
        from tests.channel_norm_ref import recentre_gammas_
        recentre_gammas_(tr.comp_model)
    _seed_params(tr.perceptual_loss.lpips, "lpips.")
    tr.loss_huge_threshold = float("inf")   # seeded random weights give a loss > 1e4, which the trainer would skip
    return tr, (copy.deepcopy(tr.comp_model), copy.deepcopy(tr.discriminator))


def _data(case):
    x = seeded_input("image", (2, 3, 64, 64)).to(dev())
    noise = {"y": seeded_input("noise.y", (2, 320, 4, 4), 0.5).to(dev()), "z": seeded_input("noise.z", (2, 192, 1, 1), 0.5).to(dev())}
    data = {"real_images": x, "noise": noise}
    if case == "beta_cond_rgan":
        data.update(rate_ind=torch.tensor([2]), beta=2.56)
    return data


def _capture(tr):
    """the trainer's gradients as each optimiser finds them"""
    captured = {}

    def cap(name, module, fn):
        def wrapped(*a, **k):
            captured[name] = {n: p.grad.detach().clone() for n, p in module.named_parameters() if p.grad is not None}
            return fn(*a, **k)
        return wrapped
    tr.g_optimizer.step = cap("g", tr.comp_model, tr.g_optimizer.step)
    tr.d_optimizer.step = cap("d", tr.discriminator, tr.d_optimizer.step)
    return captured


def _torch_gan_loss(tr):
    """the trainer's gan_loss configuration as torch ops: loss(x, is_real, is_disc)"""
    w = tr.gan_loss.lamb_gan
    if type(tr.gan_loss).__name__ == "HingeGANLoss":
        def loss(x, is_real, is_disc):
            if is_disc:
                return torch.mean(torch.relu(1 - x) if is_real else torch.relu(1 + x))
            assert is_real
            return w * -torch.mean(x)
        return loss
    rl, fl = tr.gan_loss.real_label_val, tr.gan_loss.fake_label_val

    def loss(x, is_real, is_disc):
        v = F.binary_cross_entropy_with_logits(x, torch.full_like(x, rl if is_real else fl))
        return v if is_disc else w * v
    return loss


def _literal_step(tr, G, D, data, step):
    """gan_rate_distortion_trainer.py:46-119, rgan_...:11-91, ragan_...:12-92, beta_cond_rgan_...:11-98 on the copies G, D.
    -> (log, G gradients before the clip, D gradients)"""
    loss = _torch_gan_loss(tr)
    main, aux = G.separate_aux_parameters()
    g_opt = torch.optim.Adam(list(main.values()), lr=1e-4)
    aux_opt = torch.optim.Adam(list(aux.values()), lr=1e-3)
    d_opt = torch.optim.Adam(list(D.parameters()), lr=1e-4)
    log = {}
    # ---- G
    D.requires_grad_(False)
    g_opt.zero_grad(set_to_none=True)
    aux_opt.zero_grad(set_to_none=True)
    out = G.run_model(**{k: (float(v.item()) if k == "rate_ind" else v) for k, v in data.items()})
    real, fake, bpp = out.pop("real_images"), out.pop("fake_images"), out.pop("bpp")
    other = out
    log["qbpp"] = other["qbpp"].detach().mean()
    beta = other.pop("beta") if tr.__class__.__name__.startswith("BetaCond") else None
    t = {"distortion": tr.distortion_loss(real, fake, **other)}
    if step == "gan":
        g_fake = D(fake, **other)
        t["adv"] = loss(g_fake, True, False)
        t["rate"] = tr.rate_loss(bpp, **other, current_iter=1)
        t["perceptual"] = tr.perceptual_loss(real, fake)
    else:
        t["rate"] = tr.rate_loss(bpp, **other, current_iter=1)
        t["perceptual"] = tr.perceptual_loss(real, fake)
        real_d = D(real, **other).detach()
        fake_g = D(fake, **other)
        if step == "rgan":
            l_g_real, l_g_fake = loss(real_d - fake_g, False, False), loss(fake_g - real_d, True, False)
        else:
            l_g_real, l_g_fake = loss(real_d - torch.mean(fake_g), False, False), loss(fake_g - torch.mean(real_d), True, False)
        t["adv"] = (l_g_real + l_g_fake) / 2
    l_total = sum(t.values()) if beta is None else t["distortion"] + t["rate"] + beta * (t["adv"] + t["perceptual"])
    l_total.backward()
    g_grads = {n: p.grad.detach().clone() for n, p in G.named_parameters() if p.grad is not None}
    torch.nn.utils.clip_grad_norm_(G.parameters(), 1.0)
    g_opt.step()
    log.update({k: v.detach() for k, v in t.items()})
    aux_opt.zero_grad(set_to_none=True)
    a = G.aux_loss()
    a.backward()
    aux_opt.step()
    log["aux"] = a.detach()
    # ---- D
    D.requires_grad_(True)
    d_opt.zero_grad(set_to_none=True)
    if step == "gan":
        d_real = D(real, **other)
        d_fake = D(fake.detach(), **other)
        l_d_real, l_d_fake = loss(d_real, True, True) * 0.5, loss(d_fake, False, True) * 0.5
        (l_d_real + l_d_fake).backward()
    else:
        centre = (lambda v: v) if step == "rgan" else torch.mean
        fake_d = D(fake, **other).detach()
        d_real = D(real, **other)
        l_d_real = loss(d_real - centre(fake_d), True, True) * 0.5
        l_d_real.backward()
        d_fake = D(fake.detach(), **other)
        l_d_fake = loss(d_fake - centre(d_real.detach()), False, True) * 0.5
        l_d_fake.backward()
    log.update(d_real=l_d_real.detach(), d_fake=l_d_fake.detach(), d_total=(l_d_real + l_d_fake).detach(),
               out_d_real=torch.mean(d_real.detach()), out_d_fake=torch.mean(d_fake.detach()))
    d_grads = {n: p.grad.detach().clone() for n, p in D.named_parameters() if p.grad is not None}
    d_opt.step()
    return {k: float(v) for k, v in log.items()}, g_grads, d_grads


def _fig(what, got, ref, worst):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = ref.abs().max().item()
    e = (got - ref).abs().max().item()
    r = e / scale if scale > 0 else (0.0 if e == 0 else float("inf"))
    if r > worst[0]:
        worst[0], worst[1] = r, what
    return r


def _compare_tensors(what, got: dict, ref: dict, zero_scale=None):
    """every tensor of `ref` against `got` at CAP of its scale; prints the worst figure, then asserts on all.  `zero_scale` {name: scale}:
    the scale of a tensor that is EXACTLY zero in `ref` (module docstring); it is used for nothing else."""
    worst, bad = [0.0, None], []
    assert set(ref) <= set(got), (what, sorted(set(ref) - set(got))[:4])
    for n, r in ref.items():
        if zero_scale and n in zero_scale and float(r.abs().max()) == 0.0:
            f = got[n].detach().abs().max().item() / zero_scale[n]
            print(f"{what} {n}: reference exactly 0, here {got[n].detach().abs().max().item():.3e} against the scale {zero_scale[n]:g} of the "
                  f"terms that cancel: {f:.3e} (gate {CAP:.0e})")
            worst[:] = [f, n] if f > worst[0] else worst
        else:
            f = _fig(n, got[n], r, worst)
        if not f <= CAP:
            bad.append((n, f))
    print(f"{what}: worst {worst[0]:.3e} at {worst[1]} over {len(ref)} tensors (gate {CAP:.0e})")
    assert not bad, (what, bad[:6], len(bad))


@pytest.mark.parametrize("case", list(CASES))
def test_step_equals_the_literal_reference_step(case):
    _, _, step = CASES[case]
    tr, (G, D) = _build(case)
    captured = _capture(tr)
    before_g = {n: p.detach().clone() for n, p in tr.comp_model.named_parameters()}
    before_d = {n: p.detach().clone() for n, p in tr.discriminator.named_parameters()}
    data = _data(case)
    log = tr.optimize_parameters(1, dict(data))
    assert log is not None
    ref_log, g_grads, d_grads = _literal_step(tr, G, D, data, step)
    torch.cuda.synchronize()
    # logged terms
    assert set(ref_log) == set(log), (sorted(ref_log), sorted(log))
    for k, r in ref_log.items():
        f = abs(log[k] - r) / abs(r) if r != 0 else abs(log[k])
        print(f"{case} log {k}: {log[k]:.9e} against {r:.9e}: {f:.3e} (gate {CAP:.0e})")
        assert f <= CAP, (case, k, log[k], r)
    # gradients before the optimisers, parameters after them: every tensor, the discriminator's head bias included
    _compare_tensors(f"{case} G gradients", captured["g"], g_grads)
    _compare_tensors(f"{case} D gradients", captured["d"], d_grads)
    _compare_tensors(f"{case} G parameters", dict(tr.comp_model.named_parameters()), dict(G.named_parameters()))
    _compare_tensors(f"{case} D parameters", dict(tr.discriminator.named_parameters()), dict(D.named_parameters()))
    head = HEAD_BIAS[type(tr.discriminator).__name__]
    print(f"{case} D head bias {head}: gradient {captured['d'][head].item():.9e} against {d_grads[head].item():.9e}, parameter "
          f"{dict(tr.discriminator.named_parameters())[head].item():.9e} against {dict(D.named_parameters())[head].item():.9e} (in the gates above)")
    # the discriminator trained (before this change a config naming GANRateDistortionTrainer ran a plain rate-distortion step), and so did G
    moved_d = max((p.detach() - before_d[n]).abs().max().item() for n, p in tr.discriminator.named_parameters())
    moved_g = max((p.detach() - before_g[n]).abs().max().item() for n, p in tr.comp_model.named_parameters())
    print(f"{case}: largest parameter move D {moved_d:.3e}, G {moved_g:.3e}")
    assert 0 < moved_d <= 1e-4 * (1 + 1e-3) and 0 < moved_g
    assert {"adv", "d_real", "d_fake", "d_total", "out_d_real", "out_d_fake"} <= set(log)


@pytest.mark.parametrize("case", ["rgan", "hific"])
def test_reuse_d_forward_on_and_off_give_the_same_step(case):
    """rgan: the chain-built discriminator back-propagates through the generator phase's two forwards; hific: one pass over [x_hat; x] --
    the DEFAULT path of the HiFiC recipe; off: D(x), D(x_hat) evaluated again one after the other, the path the literal comparison above
    runs for hific.  Every logged term and every gradient of the default path against the other's at the cap."""
    grads, logs = {}, {}
    for reuse in (True, False):
        tr, _ = _build(case, reuse_d_forward=reuse)
        assert tr.reuse_d_forward is reuse
        captured = _capture(tr)
        logs[reuse] = tr.optimize_parameters(1, _data(case))
        assert logs[reuse] is not None
        grads[reuse] = captured
        del tr
    assert set(logs[True]) == set(logs[False])
    for k, r in logs[False].items():
        f = abs(logs[True][k] - r) / abs(r) if r != 0 else abs(logs[True][k])
        print(f"{case} reuse on/off log {k}: {logs[True][k]:.9e} against {r:.9e}: {f:.3e} (gate {CAP:.0e})")
        assert f <= CAP, (case, k, logs[True][k], r)
    head = HEAD_BIAS["CLIC21GVAEDiscriminator" if case == "rgan" else "HiFiCConditionalDiscriminator"]
    _compare_tensors(f"{case} reuse on/off G gradients", grads[True]["g"], grads[False]["g"])
    _compare_tensors(f"{case} reuse on/off D gradients", grads[True]["d"], grads[False]["d"], zero_scale={head: 1.0} if case == "hific" else None)


def test_graph_replayed_steps_equal_eager_steps_bit_for_bit():
    """RaGAN (its centred loss keeps mean(q) in device memory): four iterations, the last two replayed from the captured g / dfb / u / d
    graphs after the two eager warm-up iterations, against four eager ones; the batch changes every iteration"""
    logs, params = {}, {}
    for graphs in (False, True):
        tr, _ = _build("ragan", hip_graphs=graphs)
        out = []
        base = _data("ragan")   # (the explicit noise tensors are persistent device buffers: a captured graph reads their addresses)
        for it in range(1, 5):
            data = dict(base, real_images=torch.roll(base["real_images"], it, dims=3) * (1 - 0.05 * it))
            out.append(tr.optimize_parameters(it, data))
        if graphs:
            assert len(tr.graphs) == 4, "segments were not captured"
        logs[graphs] = out
        params[graphs] = {"G." + k: p.detach().clone() for k, p in tr.comp_model.named_parameters()}
        params[graphs].update({"D." + k: p.detach().clone() for k, p in tr.discriminator.named_parameters()})
        del tr
    for a, b in zip(logs[False], logs[True]):
        assert a is not None and b is not None and a.keys() == b.keys()
        for k in a:
            assert a[k] == b[k], (k, a[k], b[k])
    for k in params[False]:
        assert torch.equal(params[False][k], params[True][k]), k


def test_nan_loss_leaves_parameters_and_moments_unchanged():
    tr, _ = _build("gan")
    assert tr.optimize_parameters(1, _data("gan")) is not None   # moments are non-zero from here on
    opts = {"g": tr.g_optimizer, "d": tr.d_optimizer, "aux": tr.aux_optimizer}

    def state():
        s = {"G." + n: p.detach().clone() for n, p in tr.comp_model.named_parameters()}
        s.update({"D." + n: p.detach().clone() for n, p in tr.discriminator.named_parameters()})
        for name, o in opts.items():
            for i, g in enumerate(o.param_groups):
                if g["flat"] is not None:
                    s[f"{name}.{i}.m"], s[f"{name}.{i}.v"] = g["m"].clone(), g["v"].clone()
        return s
    before = state()
    assert any(float(v.abs().max()) > 0 for k, v in before.items() if k.endswith(".m"))
    mse = tr.distortion_loss
    tr.distortion_loss = lambda *a, **k: mse(*a, **k) * float("nan")
    assert tr.optimize_parameters(2, _data("gan")) is None
    after = state()
    for k, v in before.items():
        assert torch.equal(v, after[k]), k


@pytest.mark.parametrize("case,reuse,count", [("gan", True, 2), ("gan", False, 3), ("rgan", True, 3), ("rgan", False, 4)])
def test_spectral_norm_discriminator_step_advances_u_v_by_the_documented_count(case, reuse, count):
    """HiFiCDiscriminator(use_sn=True), which is not chain-built.  Vanilla: D(x_hat) in the generator phase, then one pass over [x_hat; x]
    (reuse on: 2 power iterations) or D(x), D(x_hat) (off: 3; the reference: 3).  Relativistic: D(x), D(x_hat) in the generator phase,
    then one pass (3) or two (4; the reference: 5).  The iteration depends on the weights alone, which change only at the end of the
    step: a copy of the discriminator run forward k times in training mode holds the trainer's u / v exactly for k = count and for no
    other k <= 5."""
    from crdr_amd.trainer import build_trainer
    opt = _gan_opt(case, reuse_d_forward=reuse)
    opt["discriminator"] = {"type": "HiFiCDiscriminator", "in_ch": 3, "out_ch": 1, "main_ch": 16, "use_sn": True}
    tr = build_trainer(opt)
    _seed_params(tr.comp_model, "")
    _seed_params(tr.discriminator, "gan.sn.")
    _seed_params(tr.perceptual_loss.lpips, "lpips.")
    tr.loss_huge_threshold = float("inf")
    D0 = copy.deepcopy(tr.discriminator)
    log = tr.optimize_parameters(1, _data(case))
    assert log is not None and all(v == v and abs(v) != float("inf") for v in log.values()), log
    for n, p in list(tr.discriminator.named_parameters()) + list(tr.discriminator.named_buffers()):
        assert bool(torch.isfinite(p).all()), n
    uv = {n: b.detach().clone() for n, b in tr.discriminator.named_buffers() if n.endswith("weight_u") or n.endswith("weight_v")}
    assert len(uv) == 10
    x = _data(case)["real_images"]
    match = []
    for k in range(1, 6):
        with torch.no_grad():
            D0(x)
        same = all(torch.equal(b, uv[n]) for n, b in D0.named_buffers() if n in uv)
        print(f"{case} reuse {reuse}: u / v after {k} training-mode forwards equal the trainer's: {same}")
        match.append(same)
    assert match == [k == count for k in range(1, 6)], match


def test_channel_norm_takes_parameters_off_the_16_byte_grid():
    """An optimiser's flat buffer puts gamma / beta wherever the parameters before them end (the decoder's 3-element RGB bias): ChannelNorm2D
    with gamma, beta and their gradient slots 4 and 8 bytes off the grid gives the bits of the aligned module -- y, dx, dgamma, dbeta, the
    latter accumulated onto what the slots held"""
    from crdr_amd.models.layer.hific_norm import ChannelNorm2D
    c = 12
    x = seeded_input("cn.unaligned.x", (2, c, 5, 7), 2.0).to(dev())
    cot = seeded_input("cn.unaligned.cot", (2, c, 5, 7)).to(dev())
    gamma, beta = seeded_input("cn.unaligned.gamma", (1, c, 1, 1)) + 1.5, seeded_input("cn.unaligned.beta", (1, c, 1, 1))
    held = seeded_input("cn.unaligned.held", (2, 1, c, 1, 1))
    out = {}
    for off in (0, 1):
        m = ChannelNorm2D(c).to(dev())
        flat, gflat = torch.zeros(2 * c + 8, device=dev()), torch.zeros(2 * c + 8, device=dev())
        for i, (p, v) in enumerate(((m.gamma, gamma), (m.beta, beta))):
            lo = off * (i + 1) + i * (c + 4)
            p.data = flat[lo:lo + c].view(1, c, 1, 1)
            p.data.copy_(v)
            p.grad = gflat[lo:lo + c].view(1, c, 1, 1)
            p.grad.copy_(held[i])
            assert p.data_ptr() % 16 == 4 * off * (i + 1) and p.grad.data_ptr() % 16 == 4 * off * (i + 1)
        xd = x.clone().requires_grad_(True)
        y = m(xd, act="lrelu")
        y.backward(cot)
        out[off] = (y.detach().clone(), xd.grad.clone(), m.gamma.grad.clone(), m.beta.grad.clone())
    for name, a, b in zip(("y", "dx", "dgamma", "dbeta"), out[1], out[0]):
        assert torch.equal(a, b), name
    assert not torch.equal(out[1][2].cpu(), held[0]), "dgamma was not accumulated"
