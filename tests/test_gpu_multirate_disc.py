"""GPU parity of the four rate-aware discriminators (crdr_amd/models/discriminator/multirate_clic21_gvae_discriminator.py) against the
recorded float64 outputs of the reference's own classes (tests/golden/reference_multirate_disc.npz, written by
tests/golden/gen_golden_multirate_disc.py), the one-hot condition, and the stage-3 trainer's optimiser partitions with them.

Gates as in tests/test_gpu_hific.py: outputs and input gradients within 2e-5 of the scale of the reference tensor, parameter gradients
within 5e-5.  Every comparison prints its figure before it asserts."""
import os

import numpy as np
import pytest
import torch

from tests.golden.gen_golden_multirate_disc import RATES, cases
from tests.golden.seeded_weights import seeded_input, seeded_tensor
from tests.test_gpu_instance_norm import gate
from tests.test_gpu_model import dev
from tests.test_gpu_step import _opt, _seed_params

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_multirate_disc.npz")
CASES = cases()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def build(tag, cls, kw, gold):
    """the class on the device, weights from seeded_weights by (the generator's prefix + key, shape): a strict load of the recorded keys"""
    from crdr_amd.utils.registry import DISCRIMINATOR_REGISTRY
    import crdr_amd.models.discriminator  # noqa: F401
    D = DISCRIMINATOR_REGISTRY.get(cls)(**kw)
    shapes = {k: v.shape for k, v in D.state_dict().items()}
    D.load_state_dict({str(k): seeded_tensor(f"mrd.{tag}." + str(k), shapes[str(k)]) for k in gold[f"{tag}.keys"]}, strict=True)
    return D.to(dev())


# ---- 6. the recorded cases ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,cls,kw,grads", CASES, ids=[c[0] for c in CASES])
def test_discriminator_matches_the_recorded_reference(gold, tag, cls, kw, grads):
    D = build(tag, cls, kw, gold)
    cot = torch.from_numpy(gold["cot"]).float().to(dev())
    for q in RATES:
        D.zero_grad(set_to_none=True)
        x = torch.from_numpy(gold["x"]).float().to(dev()).requires_grad_(True)
        out = D(x, rate_ind=torch.tensor([float(q)]))
        out.backward(cot)
        gate(f"{tag} q{q} out", out, torch.from_numpy(gold[f"{tag}.q{q}.out"]), 2e-5)
        assert tuple(x.grad.shape) == (2, 3, 32, 48)
        gate(f"{tag} q{q} dx", x.grad, torch.from_numpy(gold[f"{tag}.q{q}.dx"]), 2e-5)
        params = dict(D.named_parameters())
        names = [k[len(f"{tag}.q{q}.grad."):] for k in gold.files if k.startswith(f"{tag}.q{q}.grad.")]
        assert len(names) == 3, names
        for k in names:
            gate(f"{tag} q{q} grad {k}", params[k].grad, torch.from_numpy(gold[f"{tag}.q{q}.grad.{k}"]), 5e-5)
        for k, p in params.items():
            assert p.grad is None or bool(torch.isfinite(p.grad).all()), k


# ---- 7. the one-hot condition ---------------------------------------------------------------------------------------------------------------

def test_onehot_planes_are_dense_nhwc_constants():
    from crdr_amd.models.discriminator.multirate_clic21_gvae_discriminator import cat_onehot_nhwc
    from crdr_amd.models.layer.hip_layers import to_image_nhwc
    img = seeded_input("mrd.onehot.x", (2, 3, 8, 12)).to(dev()).requires_grad_(True)
    cat = cat_onehot_nhwc(to_image_nhwc(img), 2, 3)
    assert tuple(cat.shape) == (2, 6, 8, 12) and cat.stride(1) == 1 and cat.stride(3) == 8, "3 + 3 channels in NHWC rows of 8 floats"
    assert torch.equal(cat[:, :3], img.detach())
    want = torch.tensor([0.0, 0.0, 1.0], device=dev()).view(1, 3, 1, 1).expand(2, 3, 8, 12)
    assert torch.equal(cat[:, 3:].detach(), want)
    full = torch.as_strided(cat.detach(), (2, 8, 8, 12), (8 * 12 * 8, 1, 12 * 8, 8))
    assert bool((full[:, 6:] == 0).all()), "pad lanes must be zero"
    cot = seeded_input("mrd.onehot.cot", (2, 6, 8, 12)).to(dev())
    cat.backward(cot)
    assert tuple(img.grad.shape) == (2, 3, 8, 12) and torch.equal(img.grad, cot[:, :3])


@pytest.mark.parametrize("tag", ["sb.IN.c1", "sh.none.c1", "src.IN"])
def test_onehot_condition_reaches_the_output_and_not_the_gradient_shape(gold, tag):
    """dx has the image's shape and is what the conv's input gradient gives on the image channels, whatever stands in the planes: the
    same network run on an input whose planes are built by hand, with a gradient slot on them, returns the same dx on the image channels
    (finite-difference free).  With the weights fixed the output changes with rate_ind."""
    from crdr_amd.models.discriminator import multirate_clic21_gvae_discriminator as M
    _, cls, kw, _ = next(c for c in CASES if c[0] == tag)
    D = build(tag, cls, kw, gold)
    cot = torch.from_numpy(gold["cot"]).float().to(dev())
    x = torch.from_numpy(gold["x"]).float().to(dev()).requires_grad_(True)
    out = D(x, rate_ind=2.0)
    out.backward(cot)
    assert tuple(x.grad.shape) == tuple(x.shape)
    # the planes as an ordinary input that wants a gradient: same dx on the image, and a gradient on the planes that D itself never returns
    seen = {}
    real_cat = M.cat_onehot_nhwc

    def spy(t, rate_ind, rate_level):
        n, c, h, w = t.shape
        planes = torch.zeros(n, rate_level, h, w, device=t.device)
        planes[:, rate_ind] = 1.0
        seen["planes"] = planes.requires_grad_(True)
        buf = torch.zeros((n, h, w, (c + rate_level + 3) // 4 * 4), device=t.device)
        buf[..., :c] = t.permute(0, 2, 3, 1)
        buf[..., c:c + rate_level] = seen["planes"].permute(0, 2, 3, 1)
        return buf.permute(0, 3, 1, 2)[:, :c + rate_level]
    M.cat_onehot_nhwc = spy
    try:
        D.zero_grad(set_to_none=True)
        x2 = x.detach().clone().requires_grad_(True)
        out2 = D(x2, rate_ind=2.0)
        out2.backward(cot)
    finally:
        M.cat_onehot_nhwc = real_cat
    assert torch.equal(out2, out) and torch.equal(x2.grad, x.grad)
    assert seen["planes"].grad is not None and float(seen["planes"].grad.abs().max()) > 0
    with torch.no_grad():
        other = D(x.detach(), rate_ind=torch.tensor([0.0]))
    assert not torch.equal(other, out.detach())
    if tag.startswith("src"):   # one net for every rate: only the planes can have changed the output
        print(f"{tag}: max |D(x, 0) - D(x, 2)| = {float((other - out.detach()).abs().max()):.3e}")
        assert float((other - out.detach()).abs().max()) > 1e-4 * float(out.detach().abs().max())


# ---- 8. stage-3 partitions ----------------------------------------------------------------------------------------------------------------------

def _stage3(disc_opt):
    from crdr_amd.trainer import build_trainer
    opt = _opt(3, 2, 64)
    opt["discriminator"] = disc_opt
    tr = build_trainer(opt)
    _seed_params(tr.comp_model, "")
    init = _seed_params(tr.discriminator, "mrd.step.")
    _seed_params(tr.perceptual_loss.lpips, "lpips.")
    tr.loss_huge_threshold = float("inf")   # seeded random weights give a loss > 1e4, which the trainer would skip
    return tr, init


def _two_iterations(tr):
    x = seeded_input("image", (2, 3, 64, 64))
    for it, q in enumerate((0, 2), start=1):
        log = tr.optimize_parameters(it, {"real_images": x.to(dev()), "rate_ind": torch.tensor([q]), "beta": 2.56})
        assert log is not None
        for k, v in log.items():
            assert np.isfinite(float(v)), (it, k, v)
    torch.cuda.synchronize()
    tr.d_optimizer.host_step_counts()
    g = tr.d_optimizer.param_groups[0]
    return g, g["parts"]


def _untouched(tr, g, part, prefix, init):
    assert part["step"] == 0, (prefix, part["step"])
    assert not bool(g["m"][part["lo"]:part["hi"]].any()) and not bool(g["v"][part["lo"]:part["hi"]].any()), f"{prefix}: Adam moments moved"
    names = [n for n, _ in tr.discriminator.named_parameters() if n.startswith(prefix)]
    assert names
    for n, p in tr.discriminator.named_parameters():
        if n.startswith(prefix):
            assert torch.equal(p.detach().cpu(), init["mrd.step." + n]), f"{n}: a part that did not run was touched"


def test_stage3_shared_backbone_partitions():
    tr, init = _stage3({"type": "SharedBackboneClic21GvaeDiscriminator", "num_head": 5, "in_ch": 3, "out_ch": 1, "main_ch": 16, "img_size": 64,
                        "norm_type": "IN", "backbone_depth": 2, "head_depth": 2})
    assert len(tr.d_optimizer.param_groups[0]["parts"]) == 6   # backbone, five heads
    assert tr._d_parts(0) == [0, 1] and tr._d_parts(torch.tensor([2])) == [0, 3]
    g, parts = _two_iterations(tr)
    assert [pt["step"] for pt in parts] == [2, 1, 0, 1, 0, 0], [pt["step"] for pt in parts]
    for h in (1, 3, 4):
        _untouched(tr, g, parts[1 + h], f"head_list.{h}.", init)
    moved = {n for n, p in tr.discriminator.named_parameters() if not torch.equal(p.detach().cpu(), init["mrd.step." + n])}
    assert any(n.startswith("backbone.") for n in moved) and any(n.startswith("head_list.0.") for n in moved) \
        and any(n.startswith("head_list.2.") for n in moved), sorted(moved)


def test_stage3_separate_discriminators_partitions():
    tr, init = _stage3({"type": "MultirateSeparateClic21GvaeDiscriminator", "rate_level": 5, "in_ch": 3, "out_ch": 1, "main_ch": 16, "img_size": 64,
                        "norm_type": "IN", "depth": 4})
    assert len(tr.d_optimizer.param_groups[0]["parts"]) == 5
    g, parts = _two_iterations(tr)
    assert [pt["step"] for pt in parts] == [1, 0, 1, 0, 0], [pt["step"] for pt in parts]
    for k in (1, 3, 4):
        _untouched(tr, g, parts[k], f"discriminator_list.{k}.", init)
