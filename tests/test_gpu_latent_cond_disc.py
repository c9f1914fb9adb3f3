"""GPU parity of CLIC21GVAELatentConditionalDiscriminator (crdr_amd/models/discriminator/clic21_gvae_discriminator.py) and of the trainers
that feed it.

1. The module against the recorded float64 results of the reference's own class (tests/golden/reference_latent_cond.npz, written by
   tests/golden/gen_golden_latent_cond.py): output, dx and the recorded parameter gradients within 2e-5 of the scale of the reference tensor.
2. RGANRateDistortionTrainer, one step (bs 2, 64 x 64, stage-1 model) against the literal step of tests/test_gpu_gan_step.py on deep copies:
   every logged term, every G and D gradient and every updated parameter within 2e-5 of scale, `latent_conv.0.weight` included, with
   `reuse_d_forward` off (D(x), D(x_hat) one after the other, the literal step's launches) and on (the default: one pass over
   [x_hat; x], since this class hands out no chain handle), and the two settings against each other.  A discriminator that handed out a
   chain handle would lose latent_conv's gradient from the D(x_hat) term with the option on (chain.run_chain_reuse gives no gradient to
   the chain's input): that is what the on / off comparison catches.
3. MultirateBetaCondHrrGanRateDistortionTrainer with a ModuleListDiscriminator of five such sub-discriminators, one step at q = 2 and one
   at q = 4, against the reference's step (...beta_cond...trainer.py:25-110) written out below on deep copies: torch ops for the loss,
   torch.optim.Adam, clip_grad_norm_.  Same gate; the sub-discriminators other than q stay bit-identical and without optimiser state.
4. Three steps of that trainer with `hip_graphs` on and off: the logged losses are bit-identical.

The head bias on the one-pass path.  Its gradient is the plain sum of the logit gradients and cancels analytically in the paired
relativistic step.  The literal step sums the two halves in two backward passes and holds an EXACT 0; one pass over [x_hat; x] sums all
rows in one column sum and keeps the rounding residue (measured on an MI355X: 4.66e-9 RGAN, 3.73e-9 stage 3; exactly 0 with the option
off).  A tensor that is exactly 0 on the reference side has no scale to take 2e-5 of, so two bounds that follow from the arithmetic
stand in, for this one tensor and only where the reference gradient IS exactly 0 (checked):
  gradient   2e-5 of the sum of the magnitudes of the terms that cancel, <= 1 (|l'| <= 1, two factors 1/2): the rule of
             tests/test_gpu_gan_step.py and DESIGN 13;
  parameter  the literal step's does not move, and Adam's first step moves a parameter by lr |g| / (|g| + eps) < lr whatever g is, so
             |p_here - p_literal| <= lr = 1e-4 (absolute; with the 1e-3 slack tests/test_gpu_gan_step.py gives the same quantity).  Measured:
             residue 3.7e-9 -> 2.7e-5.  A relative gate cannot hold here: Adam normalises a gradient below the rounding noise.
Every other tensor, and this one wherever the reference is not exactly 0, is under the 2e-5 gate.

Each comparison prints its figure before it asserts (profiles/upsample16_test_margins.txt)."""
import copy
import os

import numpy as np
import pytest
import torch

from tests.golden.gen_golden_latent_cond import cases
from tests.golden.seeded_weights import seeded_input, seeded_tensor
from tests.test_gpu_gan_step import CAP, _capture, _compare_tensors, _data, _gan_opt, _literal_step, _torch_gan_loss
from tests.test_gpu_instance_norm import gate
from tests.test_gpu_model import dev
from tests.test_gpu_step import _opt, _seed_params

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_latent_cond.npz")
CASES = cases()
SUB_D = {"in_ch": 3, "out_ch": 1, "y_ch": 320, "latent_nc": 12, "main_ch": 16, "norm_type": "none", "latent_interp_mode": "bilinear"}
NAME = "CLIC21GVAELatentConditionalDiscriminator"
HEAD_BIAS = "model.16.bias"   # the trunk's last conv (norm_type none)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ---- 1. the module against the recorded reference -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,kw,grads", CASES, ids=[c[0] for c in CASES])
def test_discriminator_matches_the_recorded_reference(gold, tag, kw, grads):
    from crdr_amd.utils.registry import DISCRIMINATOR_REGISTRY
    import crdr_amd.models.discriminator  # noqa: F401
    D = DISCRIMINATOR_REGISTRY.get(NAME)(**kw)
    shapes = {k: v.shape for k, v in D.state_dict().items()}
    D.load_state_dict({str(k): seeded_tensor(f"lcd.{tag}." + str(k), shapes[str(k)]) for k in gold[f"{tag}.keys"]}, strict=True)
    D.to(dev())
    x = torch.from_numpy(gold["x"]).to(dev()).requires_grad_(True)
    y = torch.from_numpy(gold["y"]).to(dev()).requires_grad_(True)
    out = D(x, y_hat=y)
    out.backward(torch.from_numpy(gold["cot"]).float().to(dev()))
    gate(f"{tag} out", out, torch.from_numpy(gold[f"{tag}.out"]), 2e-5)
    assert tuple(x.grad.shape) == (2, 3, 32, 48)
    gate(f"{tag} dx", x.grad, torch.from_numpy(gold[f"{tag}.dx"]), 2e-5)
    assert y.grad is None, "the latent enters detached"
    params = dict(D.named_parameters())
    for k in grads:
        gate(f"{tag} grad {k}", params[k].grad, torch.from_numpy(gold[f"{tag}.grad.{k}"]).view_as(params[k].grad), 2e-5)
    for k, p in params.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k


def test_no_chain_handle_leaves_the_module():
    """with chain.KEEP_HANDLES set, as the trainers set it around D(x_hat), the trunk keeps no handle -- and the caller's list is put back"""
    from crdr_amd.hip import chain
    from crdr_amd.utils.registry import DISCRIMINATOR_REGISTRY
    import crdr_amd.models.discriminator  # noqa: F401
    D = DISCRIMINATOR_REGISTRY.get(NAME)(**CASES[0][1]).to(dev())
    plain = DISCRIMINATOR_REGISTRY.get("CLIC21GVAEDiscriminator")(in_ch=3, out_ch=1, main_ch=16, norm_type="none").to(dev())
    x = seeded_input("lcd.handle.x", (2, 3, 32, 48)).to(dev())
    y = seeded_input("lcd.handle.y", (2, 24, 2, 3)).to(dev())
    mine = chain.KEEP_HANDLES = []
    try:
        D(x, y_hat=y)
        assert chain.KEEP_HANDLES is mine and mine == []
        plain(x)
        assert len(mine) == 1, "the unconditional sibling still hands out its handle"
    finally:
        chain.KEEP_HANDLES = None


# ---- 2. RGANRateDistortionTrainer ----------------------------------------------------------------------------------------------------------

def _rgan_build(reuse):
    from crdr_amd.trainer import build_trainer
    tr = build_trainer(_gan_opt("rgan", discriminator={"type": NAME, **SUB_D}, reuse_d_forward=reuse))
    _seed_params(tr.comp_model, "")
    _seed_params(tr.discriminator, "lcd.rgan.D.")
    _seed_params(tr.perceptual_loss.lpips, "lpips.")
    tr.loss_huge_threshold = float("inf")
    return tr, (copy.deepcopy(tr.comp_model), copy.deepcopy(tr.discriminator))


@pytest.fixture(scope="module")
def rgan_runs():
    """{reuse: (log, captured gradients, parameters after the step)} of the trainer, and the literal step's (log, G gradients, D gradients,
    G parameters, D parameters), each computed once"""
    runs, literal = {}, None
    for reuse in (True, False):
        tr, (G, D) = _rgan_build(reuse)
        assert tr.reuse_d_forward is reuse
        captured = _capture(tr)
        data = _data("rgan")
        log = tr.optimize_parameters(1, dict(data))
        assert log is not None
        if literal is None:
            ref_log, g_grads, d_grads = _literal_step(tr, G, D, data, "rgan")
            literal = (ref_log, g_grads, d_grads, {n: p.detach().clone() for n, p in G.named_parameters()},
                       {n: p.detach().clone() for n, p in D.named_parameters()})
        torch.cuda.synchronize()
        runs[reuse] = (log, captured, {n: p.detach().clone() for n, p in tr.comp_model.named_parameters()},
                       {n: p.detach().clone() for n, p in tr.discriminator.named_parameters()})
        del tr, G, D
    return runs, literal


def _compare_logs(what, log, ref_log):
    assert set(ref_log) <= set(log), (sorted(ref_log), sorted(log))
    for k, r in ref_log.items():
        f = abs(log[k] - r) / abs(r) if r != 0 else abs(log[k])
        print(f"{what} log {k}: {log[k]:.9e} against {r:.9e}: {f:.3e} (gate {CAP:.0e})")
        assert f <= CAP, (what, k, log[k], r)


LR_D = 1e-4   # the discriminator's Adam step size in every config of this file


def _compare_d_parameters(what, got, ref, ref_grads, head):
    """every updated discriminator parameter at the gate; the head bias by the module docstring's bound where, and only where, the literal
    step's gradient of it is exactly 0"""
    if float(ref_grads[head].abs().max()) != 0.0:
        _compare_tensors(what, got, ref)
        return
    rest = {n: p for n, p in ref.items() if n != head}
    _compare_tensors(f"{what} (all but {head})", {n: got[n] for n in rest}, rest)
    moved = float((got[head].detach() - ref[head].detach()).abs().max())
    print(f"{what} {head}: literal gradient exactly 0, |p - p_literal| {moved:.3e} against Adam's largest first step {LR_D:g} "
          f"({moved / float(ref[head].abs().max()):.3e} of scale)")
    assert moved <= LR_D * (1 + 1e-3), (what, head, moved)


def test_rgan_step_equals_the_literal_reference_step(rgan_runs):
    """`reuse_d_forward: false`: D(x), D(x_hat) one after the other, the launches of the literal step"""
    runs, (ref_log, g_grads, d_grads, g_params, d_params) = rgan_runs
    log, captured, g_after, d_after = runs[False]
    what = "rgan latent-cond"
    _compare_logs(what, log, ref_log)
    assert "latent_conv.0.weight" in d_grads and float(d_grads["latent_conv.0.weight"].abs().max()) > 0
    _compare_tensors(f"{what} G gradients", captured["g"], g_grads)
    _compare_tensors(f"{what} D gradients", captured["d"], d_grads)
    _compare_tensors(f"{what} G parameters", g_after, g_params)
    _compare_tensors(f"{what} D parameters", d_after, d_params)


def test_rgan_reuse_d_forward_on_and_off_give_the_same_gradients(rgan_runs):
    """the default setting (one pass over [x_hat; x]) against the other and against the literal step; the head bias: module docstring"""
    runs, (ref_log, g_grads, d_grads, g_params, d_params) = rgan_runs
    _compare_logs("rgan latent-cond reuse on/off", runs[True][0], runs[False][0])
    _compare_tensors("rgan latent-cond reuse on/off G gradients", runs[True][1]["g"], runs[False][1]["g"])
    _compare_tensors("rgan latent-cond reuse on/off D gradients", runs[True][1]["d"], runs[False][1]["d"], zero_scale={HEAD_BIAS: 1.0})
    on, off = runs[True][1]["d"]["latent_conv.0.weight"], runs[False][1]["d"]["latent_conv.0.weight"]
    print(f"latent_conv.0.weight gradient: max |on| {float(on.abs().max()):.6e}, max |off| {float(off.abs().max()):.6e}")
    assert float(on.abs().max()) > 0
    log, captured, g_after, d_after = runs[True]
    what = "rgan latent-cond reuse on against the literal step"
    _compare_logs(what, log, ref_log)
    _compare_tensors(f"{what} G gradients", captured["g"], g_grads)
    _compare_tensors(f"{what} D gradients", captured["d"], d_grads, zero_scale={HEAD_BIAS: 1.0})
    _compare_tensors(f"{what} G parameters", g_after, g_params)
    _compare_d_parameters(f"{what} D parameters", d_after, d_params, d_grads, HEAD_BIAS)


# ---- 3. the stage-3 trainer with one such discriminator per rate level ----------------------------------------------------------------

def _stage3_build(**extra):
    from crdr_amd.trainer import build_trainer
    opt = _opt(3, 2, 64)
    opt["discriminator"] = {"type": "ModuleListDiscriminator", "_subd_type": NAME, "_num_subd": 5, **SUB_D}
    for k, v in extra.items():
        opt[k] = v
    tr = build_trainer(opt)
    _seed_params(tr.comp_model, "")
    init = _seed_params(tr.discriminator, "lcd.s3.D.")
    _seed_params(tr.perceptual_loss.lpips, "lpips.")
    tr.loss_huge_threshold = float("inf")   # seeded random weights give a loss > 1e4, which the trainer would skip
    return tr, init


def _stage3_data(q, beta=2.56):
    return dict(_data("rgan"), rate_ind=torch.tensor([q]), beta=beta)


def _literal_stage3_step(tr, G, D, data, q):
    """...beta_cond...trainer.py:25-110 on the copies G, D -> (log, G gradients before the clip, D gradients)"""
    loss = _torch_gan_loss(tr)
    main, aux = G.separate_aux_parameters()
    g_opt = torch.optim.Adam(list(main.values()), lr=1e-4)
    aux_opt = torch.optim.Adam(list(aux.values()), lr=1e-3)
    d_opt = torch.optim.Adam(list(D.parameters()), lr=1e-4)
    log = {}
    # ---- G (:19-83)
    D.requires_grad_(False)
    g_opt.zero_grad(set_to_none=True)
    aux_opt.zero_grad(set_to_none=True)
    call = {k: (float(v.item()) if k == "rate_ind" else v) for k, v in data.items()}
    out = G.run_model(**call)
    real, fake, bpp = out.pop("real_images"), out.pop("fake_images"), out.pop("bpp")
    other = out
    other["rate_ind"] = q
    beta = other["beta"]
    log["qbpp"] = other["qbpp"].detach().mean()
    if q + 1 > tr.rate_level - 1:
        relative = real
    else:
        with torch.no_grad():   # (:36-39) the whole model once more at the next rate level; only its image is kept
            relative = G.run_model(**dict(call, rate_ind=float(q + 1)))["fake_images"]
    t = {"distortion": tr.distortion_loss(real, fake, **other)}
    t["rate"] = tr.rate_loss(bpp, **other, current_iter=1)
    t["perceptual"] = tr.perceptual_loss(real, fake)
    real_d = D(relative.detach(), **other).detach()   # (:56) with the LOW-rate pass's y_hat
    fake_g = D(fake, **other)
    t["adv"] = (loss(real_d - fake_g, False, False) + loss(fake_g - real_d, True, False)) / 2
    l_total = t["distortion"] + t["rate"] + beta * (t["perceptual"] + t["adv"])
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
    # ---- D (:88-110)
    D.requires_grad_(True)
    d_opt.zero_grad(set_to_none=True)
    fake_d = D(fake.detach(), **other).detach()
    d_real = D(real, **other)
    l_d_real = loss(d_real - fake_d, True, True) * 0.5
    l_d_real.backward()
    d_fake = D(fake.detach(), **other)
    l_d_fake = loss(d_fake - d_real.detach(), False, True) * 0.5
    l_d_fake.backward()
    log.update(d_real=l_d_real.detach(), d_fake=l_d_fake.detach(), d_total=(l_d_real + l_d_fake).detach(),
               out_d_real=torch.mean(d_real.detach()), out_d_fake=torch.mean(d_fake.detach()))
    d_grads = {n: p.grad.detach().clone() for n, p in D.named_parameters() if p.grad is not None}
    d_opt.step()
    return {k: float(v) for k, v in log.items()}, g_grads, d_grads


_STAGE3 = {}


def _stage3_run(q):
    """one trainer step and the literal step at rate level q, computed once: everything the test below compares, as clones"""
    if q in _STAGE3:
        return _STAGE3[q]
    tr, init = _stage3_build()
    assert tr.d_batch_inputs == ("y_hat",)
    G, D = copy.deepcopy(tr.comp_model), copy.deepcopy(tr.discriminator)
    captured = _capture(tr)
    data = _stage3_data(q)
    log = tr.optimize_parameters(1, dict(data))
    assert log is not None
    ref_log, g_grads, d_grads = _literal_stage3_step(tr, G, D, data, q)
    torch.cuda.synchronize()
    tr.d_optimizer.host_step_counts()
    g0 = tr.d_optimizer.param_groups[0]
    parts = g0["parts"]
    clone = lambda m: {n: p.detach().clone() for n, p in m.named_parameters()}   # noqa: E731
    _STAGE3[q] = dict(log=log, ref_log=ref_log, captured=captured, g_grads=g_grads, d_grads=d_grads, g_after=clone(tr.comp_model), g_ref=clone(G),
                      d_after=clone(tr.discriminator), d_ref=clone(D), init=init, steps=[pt["step"] for pt in parts],
                      moments_moved=[bool(g0["m"][pt["lo"]:pt["hi"]].any()) or bool(g0["v"][pt["lo"]:pt["hi"]].any()) for pt in parts])
    return _STAGE3[q]


@pytest.mark.parametrize("q", [2, 4], ids=["q2", "q4"])
def test_stage3_step_equals_the_literal_reference_step(q):
    """the trainer's one pass over [x_hat; x], y_hat stacked along the batch, against the reference's three evaluations"""
    r = _stage3_run(q)
    what = f"stage 3 latent-cond q{q}"
    head = f"subD_list.{q}.{HEAD_BIAS}"
    _compare_logs(what, r["log"], r["ref_log"])
    assert set(r["d_grads"]) == {n for n in r["d_ref"] if n.startswith(f"subD_list.{q}.")}
    assert float(r["d_grads"][f"subD_list.{q}.latent_conv.0.weight"].abs().max()) > 0
    _compare_tensors(f"{what} G gradients", r["captured"]["g"], r["g_grads"])
    _compare_tensors(f"{what} D gradients", r["captured"]["d"], r["d_grads"], zero_scale={head: 1.0})
    _compare_tensors(f"{what} G parameters", r["g_after"], r["g_ref"])
    _compare_d_parameters(f"{what} D parameters", r["d_after"], r["d_ref"], r["d_grads"], head)
    # the sub-discriminators that did not run: bit-identical to their initial state, no optimiser state
    assert r["steps"] == [int(k == q) for k in range(5)], r["steps"]
    for n, p in r["d_after"].items():
        if int(n.split(".")[1]) != q:
            assert torch.equal(p.cpu(), r["init"]["lcd.s3.D." + n]), f"{n}: a sub-discriminator that did not run was touched"
    assert r["moments_moved"] == [k == q for k in range(5)], r["moments_moved"]


def test_stage3_graph_replayed_steps_equal_eager_steps_bit_for_bit():
    logs = {}
    for graphs in (False, True):
        tr, _ = _stage3_build(hip_graphs=graphs)
        base = _stage3_data(2)   # (the explicit noise tensors are persistent device buffers: a captured graph reads their addresses)
        out = []
        for it in range(1, 4):
            out.append(tr.optimize_parameters(it, dict(base, real_images=torch.roll(base["real_images"], it, dims=3) * (1 - 0.05 * it))))
        if graphs:
            assert len(tr.graphs) > 0, "segments were not captured"
        logs[graphs] = out
        del tr
    for it, (a, b) in enumerate(zip(logs[False], logs[True]), start=1):
        assert a is not None and b is not None and a.keys() == b.keys()
        for k in a:
            print(f"stage 3 latent-cond iteration {it} {k}: eager {a[k]!r} graph {b[k]!r}")
            assert a[k] == b[k], (it, k, a[k], b[k])
