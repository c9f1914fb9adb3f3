"""LPIPS-VGG without a GPU: the restatement in tests/lpips_vgg_ref.py against torch's own pool, the shapes and keys of LpipsVgg, the
options of LPIPSLoss, the weights file, the folded range_norm constants, and the decision budget that the GPU parity test
(tests/test_gpu_lpips_vgg.py) relies on, here between a float32 and a float64 run of the restatement."""
import pytest
import torch
import torch.nn.functional as F

from tests import lpips_vgg_ref as R
from tests.golden.seeded_weights import seeded_input

SHAPE = (2, 3, 35, 45)


# ---- the restated pool is torch's --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 4, 2, 2), (2, 8, 5, 7), (2, 8, 35, 45)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["post_relu", "doubled_max"])
def test_restated_pool_is_torch_max_pool2d(shape, kind):
    x = R.POOL_INPUTS[kind](shape).double()
    win = R.windows(x)
    if kind == "doubled_max":
        assert bool(((win == win.max(-1, keepdim=True).values).sum(-1) >= 2).all())
    elif x.numel() > 64:
        assert bool((win.sum(-1) == 0).any()), "no all-zero window: the tie at zero would go untested"
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = R.pool2(xa)[0], F.max_pool2d(xb, 2, 2)
    assert torch.equal(ya, yb)
    cot = R.pool_cotangent(tuple(ya.shape)).double()
    ya.backward(cot)
    yb.backward(cot)
    assert torch.equal(xa.grad, xb.grad)


# ---- the restated net ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def runs():
    """the float32 and the float64 run of the restatement on the 2 x 3 x 35 x 45 input, with and without the weight gain; shared,
    never modified"""
    out = {}
    a, b = R.seeded_images(SHAPE)
    for gain in (True, False):
        sd, lin = R.seeded_vgg(gain)
        for dt in (torch.float32, torch.float64):
            bb = b.to(dt).clone().requires_grad_(True)
            v, rec = R.lpips_vgg(*R.cast(sd, lin, dt), a.to(dt), bb)
            v.sum().backward()
            out[gain, dt] = (v.detach(), rec, bb.grad)
    return out


def test_restated_net_tap_shapes_and_scale(runs):
    _, rec, _ = runs[True, torch.float64]
    assert [tuple(t.shape[2:]) for t in rec["taps"]] == [(35, 45), (17, 22), (8, 11), (4, 5), (2, 2)]
    assert [t.shape[1] for t in rec["taps"]] == [64, 128, 256, 512, 512]
    assert sum(z.numel() for z in rec["z"]) == 803584 and sum(i.numel() for i in rec["argmax"]) == 84736
    for i, t in enumerate(rec["taps"]):
        rms = t.square().mean().sqrt().item()
        print(f"tap {i}: RMS {rms:.3f}")
        assert 0.1 <= rms <= 10


@pytest.mark.parametrize("gain", [True, False], ids=["gain_sqrt2", "no_gain"])
def test_decision_budget_float32_against_float64(runs, gain):
    """The budget the GPU parity test applies to the device, applied to torch's own float32: at most 8 of the 888 320 decisions differ from
    float64's, each where float64 is within 1e-4 of undecided, and with float32's decisions imposed the float64 gradient agrees with the
    float32 one to 2e-5 (relative L2)."""
    v32, rec32, g32 = runs[gain, torch.float32]
    v64, rec64, g64_free = runs[gain, torch.float64]
    dec = {"masks": rec32["masks"], "argmax": rec32["argmax"]}
    differ, outside, total = R.decision_budget(rec64, dec)
    print(f"gain {gain}: {differ} of {total} decisions differ, {outside} outside the window; free-run gradient rel L2 "
          f"{R.rel_l2(g32, g64_free):.3e}, value max rel {R.max_rel(v32, v64):.3e}")
    assert total == 803584 + 84736
    assert differ <= R.BUDGET and outside == 0
    a, b = R.seeded_images(SHAPE)
    sd, lin = R.cast(*R.seeded_vgg(gain), torch.float64)
    bb = b.double().requires_grad_(True)
    v, _ = R.lpips_vgg(sd, lin, a.double(), bb, decisions=dec)
    v.sum().backward()
    e_v, e_g = R.max_rel(v32, v), R.rel_l2(g32, bb.grad)
    print(f"gain {gain}: decisions imposed: value max rel {e_v:.3e}, gradient rel L2 {e_g:.3e}")
    assert e_g <= 2e-5 and e_v <= 2e-5


# ---- LpipsVgg / LPIPSLoss on the host -------------------------------------------------------------------------------------------------------

def test_lpips_loss_vgg_builds_with_the_vgg16_schema():
    from crdr_amd.losses.perceptual_loss import LPIPSLoss, LpipsVgg
    m = LPIPSLoss(loss_weight=1.0, net="vgg", allow_random_weights=True)
    assert isinstance(m.lpips, LpipsVgg) and m.pretrained is False
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    want = {"lpips.in_scale": (3,), "lpips.in_shift": (3,)}
    for j, (ci, co) in enumerate(R.CFG):
        want[f"lpips.net.{j}.weight"] = (co, ci, 3, 3)
        want[f"lpips.net.{j}.bias"] = (co,)
    for i, c in enumerate((64, 128, 256, 512, 512)):
        want[f"lpips.lin.{i}"] = (c,)
    assert shapes == want
    assert not any(p.requires_grad for p in m.parameters())
    with pytest.raises(ValueError, match="16"):
        m.lpips.features(torch.zeros(1, 3, 15, 32))


def test_lpips_loss_default_is_alex_and_other_nets_are_refused():
    from crdr_amd.losses.perceptual_loss import LPIPSLoss, LpipsAlex
    assert isinstance(LPIPSLoss(loss_weight=1.0, allow_random_weights=True).lpips, LpipsAlex)
    assert isinstance(LPIPSLoss(loss_weight=1.0, net="alex", allow_random_weights=True).lpips, LpipsAlex)
    with pytest.raises(NotImplementedError, match="net"):
        LPIPSLoss(loss_weight=1.0, net="squeeze", allow_random_weights=True)


def _files(tmp_path):
    from crdr_amd.losses.perceptual_loss import ALEX_CFG, _TV_IDX, VGG_TV_IDX
    out = {}
    for name, key, cfg, idx, taps in (("alex", "alexnet_features", [(ci, co, k) for ci, co, k, _, _ in ALEX_CFG], _TV_IDX, range(5)),
                                      ("vgg", "vgg16_features", [(ci, co, 3) for ci, co in R.CFG], VGG_TV_IDX, R.TAPS)):
        feats, lin = {}, {}
        for i, (ci, co, k) in enumerate(cfg):
            feats[f"{idx[i]}.weight"] = torch.full((co, ci, k, k), 0.01 * (i + 1))
            feats[f"{idx[i]}.bias"] = torch.full((co,), 0.1 * (i + 1))
        for i, j in enumerate(taps):
            lin[f"lin{i}.model.1.weight"] = torch.full((1, cfg[j][1], 1, 1), float(i + 2))
        out[name] = str(tmp_path / f"lpips_{name}.pth")
        torch.save({key: feats, "lpips_lin": lin}, out[name])
    return out


def test_weights_file_round_trip_and_wrong_net(tmp_path, monkeypatch):
    from crdr_amd.losses.perceptual_loss import LPIPSLoss
    monkeypatch.delenv("CRDR_ALLOW_RANDOM_LPIPS", raising=False)
    monkeypatch.delenv("CRDR_LPIPS_WEIGHTS", raising=False)
    f = _files(tmp_path)
    with pytest.raises(RuntimeError, match="pretrained"):
        LPIPSLoss(loss_weight=1.0, net="vgg")
    m = LPIPSLoss(loss_weight=1.0, net="vgg", weights=f["vgg"])
    assert m.pretrained
    assert float(m.lpips.net[12].bias[0]) == pytest.approx(1.3) and float(m.lpips.net[7].weight[5, 5, 1, 1]) == pytest.approx(0.08)
    assert float(m.lpips.lin[4][511]) == 6.0 and float(m.lpips.lin[0][63]) == 2.0
    with pytest.raises(ValueError, match="vgg16_features"):
        LPIPSLoss(loss_weight=1.0, net="vgg", weights=f["alex"])
    with pytest.raises(ValueError, match="alexnet_features"):
        LPIPSLoss(loss_weight=1.0, net="alex", weights=f["vgg"])
    monkeypatch.setenv("CRDR_LPIPS_WEIGHTS", f["vgg"])
    assert LPIPSLoss(loss_weight=1.0, net="vgg").pretrained


@pytest.mark.parametrize("net", ["alex", "vgg"])
def test_folded_range_norm_constants(net):
    """scale' x + shift' with the folded constants is the scaling layer applied to (x - 0.5) * 2"""
    from crdr_amd.losses.perceptual_loss import LPIPS_SCALE, LPIPS_SHIFT, LPIPSLoss
    plain = LPIPSLoss(loss_weight=1.0, net=net, allow_random_weights=True).lpips
    fold = LPIPSLoss(loss_weight=1.0, net=net, range_norm=True, allow_random_weights=True).lpips
    sh, sc = torch.tensor(LPIPS_SHIFT, dtype=torch.float64), torch.tensor(LPIPS_SCALE, dtype=torch.float64)
    assert torch.equal(plain.in_scale, 1.0 / torch.tensor(LPIPS_SCALE))
    assert torch.equal(plain.in_shift, -torch.tensor(LPIPS_SHIFT) / torch.tensor(LPIPS_SCALE))
    x = torch.linspace(0, 1, 11, dtype=torch.float64).view(-1, 1)
    two_step = ((x - 0.5) * 2 - sh) / sc
    one_step = x * fold.in_scale.double() + fold.in_shift.double()
    err = ((one_step - two_step).abs().max() / two_step.abs().max()).item()
    print(f"{net}: folded range_norm constants against the two-step formula: {err:.2e}")
    assert err <= 1e-7
    assert (fold.in_scale.double() - 2 / sc).abs().max() <= 1e-7 * (2 / sc).max()
