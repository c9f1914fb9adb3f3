"""LPIPS-VGG on the device: LpipsVgg against the float64 restatement of tests/lpips_vgg_ref.py under the decision budget (the device's
ReLU masks and pool indices are imposed on the restatement; at most 8 may differ from its own, each where float64 itself is within
1e-4 of undecided), the folded range_norm, the unchanged default path, and graph replay of a stage-1 step with `net: vgg`.

Gates against float64: 2e-5, as max|d| / max|ref| for the value and relative L2 for the image gradient -- the project's gate for conv
outputs and norm ops; torch's CPU float32 sits at 7e-8 and 2e-6 on the 2 x 3 x 35 x 45 input (tests/test_lpips_vgg_host.py).  Every
comparison prints its figure before it asserts; profiles/lpips_vgg_test_margins.txt keeps a run's figures.

Measured on an MI355X (profiles/lpips_vgg_test_margins.txt): 2 x 3 x 35 x 45: 1 of 888 320 decisions differs, none outside the window,
value 9.7e-8, gradient 2.4e-6;  1 x 3 x 16 x 16: none of 76 800 differs, value 7.7e-8, gradient 1.6e-6;  range_norm: value 1.7e-7 (alex) /
1.0e-7 (vgg), gradient 7.3e-7 / 4.6e-7."""
import pytest
import torch

from tests import lpips_vgg_ref as R
from tests.golden.seeded_weights import seeded_input
from tests.test_gpu_model import dev
from tests.test_gpu_step import _opt, _seed_params

pytestmark = pytest.mark.gpu
GATE = 2e-5


def _seeded_vgg_module():
    from crdr_amd.losses.perceptual_loss import LpipsVgg
    sd, lin = R.seeded_vgg()
    m = LpipsVgg()
    with torch.no_grad():
        for j in range(len(R.CFG)):
            m.net[j].weight.copy_(sd[f"net.{j}.weight"])
            m.net[j].bias.copy_(sd[f"net.{j}.bias"])
        for i in range(5):
            m.lin[i].copy_(lin[i])
    return m.to(dev()), sd, lin


@pytest.mark.parametrize("shape", [(2, 3, 35, 45), (1, 3, 16, 16)], ids=lambda s: "x".join(map(str, s)))
def test_lpips_vgg_matches_float64_under_the_decision_budget(shape):
    m, sd, lin = _seeded_vgg_module()
    what = "lpips_vgg " + "x".join(map(str, shape))
    a, b = R.seeded_images(shape)
    bd = b.to(dev()).requires_grad_(True)
    v = m(a.to(dev()), bd)
    v.sum().backward()
    with torch.no_grad():
        acts = m.features(b.to(dev()), all_layers=True)
        taps = m.features(b.to(dev()))
    assert len(acts) == 13 and len(taps) == 5
    assert all(torch.equal(t, acts[j]) for t, j in zip(taps, R.TAPS))
    decisions = R.decisions_of_acts(acts)

    sd64, lin64 = R.cast(sd, lin, torch.float64)
    with torch.no_grad():
        v_free, rec = R.lpips_vgg(sd64, lin64, a.double(), b.double())
    differ, outside, total = R.decision_budget(rec, decisions)
    print(f"{what}: {differ} of {total} device decisions differ from float64's own, {outside} outside the 1e-4 window")
    assert differ <= R.BUDGET and outside == 0

    b64 = b.double().requires_grad_(True)
    v64, _ = R.lpips_vgg(sd64, lin64, a.double(), b64, decisions=decisions)
    v64.sum().backward()
    e_v, e_g = R.max_rel(v, v64), R.rel_l2(bd.grad, b64.grad)
    print(f"{what}: value max|d|/max|ref| {e_v:.3e} (gate {GATE:.0e}); image gradient rel L2 {e_g:.3e} (gate {GATE:.0e}); "
          f"value against the free float64 run {R.max_rel(v, v_free):.3e}")
    assert e_v <= GATE, f"{what}: value {e_v:.3e}"
    assert e_g <= GATE, f"{what}: gradient {e_g:.3e}"


def test_lpips_vgg_refuses_images_below_16_pixels():
    m, _, _ = _seeded_vgg_module()
    x = seeded_input("lpips_vgg.small", (1, 3, 15, 16)).to(dev())
    with pytest.raises(ValueError, match="16 x 16"):
        m(x, x)


@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_range_norm_is_the_scaling_of_the_inputs(net):
    """LPIPSLoss(range_norm=True) on [0, 1] images = LPIPSLoss(range_norm=False) on 2x - 1: value to 2e-6, gradient (after the chain rule's
    factor 2) to 2e-5"""
    from crdr_amd.losses.perceptual_loss import LPIPSLoss
    torch.manual_seed(5)
    plain = LPIPSLoss(loss_weight=1.0, net=net, allow_random_weights=True)
    fold = LPIPSLoss(loss_weight=1.0, net=net, range_norm=True, allow_random_weights=True)
    with torch.no_grad():
        for p, q in zip(fold.parameters(), plain.parameters()):
            p.copy_(q)
    plain, fold = plain.to(dev()), fold.to(dev())
    a, b = ((t + 1) / 2 for t in R.seeded_images((2, 3, 32, 32)))
    b01 = b.to(dev()).requires_grad_(True)
    v1 = fold(a.to(dev()), b01)
    v1.backward()
    b11 = (2 * b - 1).to(dev()).requires_grad_(True)
    v2 = plain((2 * a - 1).to(dev()), b11)
    v2.backward()
    e_v, e_g = R.max_rel(v1, v2.cpu()), R.rel_l2(b01.grad, 2 * b11.grad.cpu())
    print(f"lpips range_norm {net}: value {e_v:.3e} (gate 2e-06), gradient rel L2 {e_g:.3e} (gate 2e-05)")
    assert e_v <= 2e-6 and e_g <= 2e-5


def test_default_lpips_loss_is_lpips_alex_bit_for_bit():
    from crdr_amd.losses.perceptual_loss import LPIPSLoss, LpipsAlex
    torch.manual_seed(11)
    loss = LPIPSLoss(loss_weight=1).to(dev())
    torch.manual_seed(11)
    alex = LpipsAlex().to(dev())
    assert type(loss.lpips) is LpipsAlex
    for (k, p), (k2, q) in zip(loss.lpips.state_dict().items(), alex.state_dict().items()):
        assert k == k2 and torch.equal(p, q), k
    a, b = (t.to(dev()) for t in R.seeded_images((2, 3, 64, 64)))
    b1, b2 = b.clone().requires_grad_(True), b.clone().requires_grad_(True)
    v1, v2 = loss(a, b1), alex(a, b2).mean()
    v1.backward()
    v2.backward()
    assert torch.equal(v1, v2) and torch.equal(b1.grad, b2.grad)


def _stage1_trainer(net, graphs):
    from crdr_amd.trainer import build_trainer
    opt = _opt(1)
    opt["loss"]["perceptual_loss"]["net"] = net
    opt["hip_graphs"] = graphs
    tr = build_trainer(opt)
    _seed_params(tr.comp_model, "")
    _seed_params(tr.perceptual_loss.lpips, "lpips.")
    tr.loss_huge_threshold = float("inf")
    return tr


def test_stage1_step_with_lpips_vgg_replays_bit_for_bit():
    """tests/test_gpu_graph.py's stage-1 case with `net: vgg`: two eager warm-up iterations, then three through the captured graphs, against
    five eager ones"""
    from crdr_amd.losses.perceptual_loss import LpipsVgg
    x = seeded_input("image", (2, 3, 64, 64)).to(dev())
    noise = {"y": seeded_input("noise.y", (2, 320, 4, 4), 0.5).to(dev()), "z": seeded_input("noise.z", (2, 192, 1, 1), 0.5).to(dev())}
    logs, params = {}, {}
    for mode in (False, True):
        tr = _stage1_trainer("vgg", mode)
        assert isinstance(tr.perceptual_loss.lpips, LpipsVgg)
        logs[mode] = [tr.optimize_parameters(it, {"real_images": x, "noise": noise}) for it in range(1, 6)]
        if mode:
            assert len(tr.graphs) == 2, "segments were not captured"
        params[mode] = {k: p.detach().clone() for k, p in tr.comp_model.named_parameters()}
        del tr
    for a, b in zip(logs[False], logs[True]):
        assert a is not None and b is not None and a.keys() == b.keys()
        for k in a:
            assert a[k] == b[k], (k, a[k], b[k])
    for k in params[False]:
        assert torch.equal(params[False][k], params[True][k]), k
    alex = _stage1_trainer("alex", False).optimize_parameters(1, {"real_images": x, "noise": noise})
    print(f"stage 1, first step: perceptual {logs[False][0]['perceptual']} with net: vgg, {alex['perceptual']} with net: alex")
    assert alex["perceptual"] != logs[False][0]["perceptual"]
    assert alex["distortion"] == logs[False][0]["distortion"]
