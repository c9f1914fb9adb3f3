"""MS-SSIM and L1 on the HIP kernels against the test-side restatement of pytorch_msssim 1.0.0 (tests/msssim_ref.py,
PARITY UNPINNED: the library is not installed here).  Every value / gradient gate is max(floor, 3 x |fp32 restatement -
float64 restatement|): the fp32 restatement is what the reference computes, so the gate never sits below the reference's
own rounding noise."""
import os

import numpy as np
import pytest
import torch

from tests import msssim_ref as R
from tests.golden.seeded_weights import seeded_input
from tests.test_gpu_model import dev, rel
from tests.test_gpu_step import N_GENERATOR_RELUS, _MaskSink, _opt, _seed_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g) * 2 - 1
    y = (x + 0.3 * (torch.rand(shape, generator=g) * 2 - 1)).clamp(-1, 1)
    return x, y


def _ref(x, y, dtype, data_range=1.0):
    xr, yr = x.clone().to(dtype).requires_grad_(True), y.clone().to(dtype).requires_grad_(True)
    v = R.ms_ssim(xr, yr, data_range, dtype)
    v.backward()
    return v.detach().double(), xr.grad.double(), yr.grad.double()


def _relerr(a, b):
    return ((a.double() - b).norm() / b.norm()).item()


@pytest.mark.parametrize("shape,layout", [((2, 3, 256, 256), "nchw"), ((1, 3, 197, 263), "nchw"), ((2, 3, 193, 170), "nhwc_ld4")])
def test_ms_ssim_value_and_gradients(shape, layout):
    from crdr_amd.hip import msssim as MS, ops
    x, y = _pair(shape, 7)
    v64, gx64, gy64 = _ref(x, y, torch.float64)
    v32, gx32, gy32 = _ref(x, y, torch.float32)
    xd, yd = x.to(dev()), y.to(dev())
    if layout == "nhwc_ld4":
        xd, ld = ops.nhwc(xd)
        yd, _ = ops.nhwc(yd)
        assert ld == 4 and not xd.is_contiguous()
    xd.requires_grad_(True)
    yd.requires_grad_(True)
    v = MS.ms_ssim(xd, yd, 1.0)
    v.backward()
    tol_v = max(1e-5, 3 * abs(v32.item() - v64.item()))
    tol_gx, tol_gy = max(1e-4, 3 * _relerr(gx32, gx64)), max(1e-4, 3 * _relerr(gy32, gy64))
    e_v, e_gx, e_gy = abs(v.item() - v64.item()), _relerr(xd.grad.cpu(), gx64), _relerr(yd.grad.cpu(), gy64)
    print(f"\n{shape} {layout}: value {e_v:.2e} (gate {tol_v:.2e}), dX {e_gx:.2e} (gate {tol_gx:.2e}), dY {e_gy:.2e} (gate {tol_gy:.2e})")
    assert e_v <= tol_v and e_gx <= tol_gx and e_gy <= tol_gy, (e_v, tol_v, e_gx, tol_gx, e_gy, tol_gy)


def test_ms_ssim_is_deterministic():
    from crdr_amd.hip import msssim as MS
    x, y = _pair((2, 3, 200, 230), 3)
    outs = []
    for _ in range(2):
        yd = y.to(dev()).requires_grad_(True)
        v = MS.ms_ssim(x.to(dev()), yd, 1.0)
        v.backward()
        outs.append((v.detach().clone(), yd.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_ms_ssim_size_check_launches_nothing(monkeypatch):
    from crdr_amd.hip import msssim as MS

    def no_library():
        raise RuntimeError("the library was reached")
    monkeypatch.setattr(MS.L, "load", no_library)
    x = torch.zeros(1, 3, 160, 300, device=dev())
    with pytest.raises(AssertionError):
        MS.ms_ssim(x, x, 1.0)
    with pytest.raises(AssertionError):
        MS.ms_ssim(x.transpose(2, 3), x.transpose(2, 3), 1.0)


def test_calc_ms_ssim_on_kodim23():
    from PIL import Image
    from crdr_amd.utils.img_utils import calc_ms_ssim
    img = np.asarray(Image.open(os.path.join(ROOT, "demo_images", "kodim23.png")).convert("RGB"), dtype=np.float32)
    real = torch.from_numpy(img).permute(2, 0, 1)[None] / 255.0 * 2 - 1        # [-1, 1], 512 x 768
    assert real.shape[2:] == (512, 768)
    noise = torch.randn(real.shape, generator=torch.Generator().manual_seed(23)) * 0.05
    fake = (real + noise).clamp(-1, 1)
    q64 = R.ms_ssim(*R.quantize(real, fake), 255, torch.float64).item()
    q32 = R.ms_ssim(*R.quantize(real, fake), 255, torch.float32).item()
    got = calc_ms_ssim(real.to(dev()), fake.to(dev()))
    tol = max(5e-5, 3 * abs(q32 - q64))
    print(f"\nkodim23: |gpu - f64| {abs(got - q64):.2e}, |f32 - f64| {abs(q32 - q64):.2e}, gate {tol:.2e}")
    assert abs(got - q64) <= tol, (got, q64, tol)
    # 0..255 input: no conversion, truncation only
    r255, f255 = (real + 1) / 2 * 255 + 0.25, (fake + 1) / 2 * 255 + 0.25
    want = R.ms_ssim(r255.int().float(), f255.int().float(), 255, torch.float64).item()
    got = calc_ms_ssim(r255.to(dev()), f255.to(dev()))
    assert abs(got - want) <= tol, (got, want)
    assert calc_ms_ssim(real[..., :128, :128].to(dev()), fake[..., :128, :128].to(dev())) == -1.0


def test_l1_loss_against_torch():
    from crdr_amd.losses import build_loss
    loss = build_loss({"type": "L1Loss", "loss_weight": 2.5})
    a, b = _pair((2, 3, 40, 36), 5)
    b[:, :, ::3] = a[:, :, ::3]                     # tied elements: sign(0) = 0
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    want = 2.5 * torch.nn.L1Loss()(ar, br)
    want.backward()
    ad, bd = a.to(dev()).requires_grad_(True), b.to(dev()).requires_grad_(True)
    got = loss(ad, bd)
    got.backward()
    assert abs(got.item() - want.item()) <= 1e-5 * abs(want.item())
    for g, r in ((ad.grad.cpu(), ar.grad), (bd.grad.cpu(), br.grad)):
        assert torch.equal(torch.sign(g), torch.sign(r)) and torch.allclose(g, r, rtol=1e-6, atol=0)
    assert (ad.grad.cpu()[:, :, ::3] == 0).all()


def _msssim_opt(bs, size, graphs=None):
    opt = _opt(1, bs, size)
    opt["loss"]["distortion_loss"] = {"type": "MSSSIMLoss", "loss_weight": 1.0}
    if graphs is not None:
        opt["hip_graphs"] = graphs
    return opt


def test_stage1_step_with_msssim_loss():
    """one stage-1 step with distortion_loss MSSSIMLoss at bs 2 x 192^2 against the oracle's step whose distortion term is the
    float64-restated MS-SSIM loss of the oracle's own reconstruction (ReLU masks imposed, as _stage1_step(impose_masks=True))"""
    from oracle import crdr_oracle as O
    from crdr_amd.trainer import build_trainer
    from tests.test_gpu_model import grad_sd
    bs, size = 2, 192
    tr = build_trainer(_msssim_opt(bs, size))
    sd_g = _seed_params(tr.comp_model, "")
    sd_l = _seed_params(tr.perceptual_loss.lpips, "lpips.")
    x = seeded_input("image", (bs, 3, size, size))
    ny = seeded_input("noise.y", (bs, 320, size // 16, size // 16), 0.5)
    nz = seeded_input("noise.z", (bs, 192, size // 64, size // 64), 0.5)
    tr.loss_huge_threshold = float("inf")
    tr.comp_model.context_model.record_symbols = []
    z_hats, captured = [], {}
    run_model, g_step = tr.comp_model.run_model, tr.g_optimizer.step

    def spy(*a, **k):
        o = run_model(*a, **k)
        z_hats.append(o["z_hat"].detach().cpu())
        return o

    def wrapped(*a, **k):
        captured.update({n: (p.grad.clone() if p.grad is not None else None) for n, p in tr.comp_model.named_parameters()})
        return g_step(*a, **k)
    tr.comp_model.run_model, tr.g_optimizer.step = spy, wrapped
    with _MaskSink(tr.comp_model) as sink:
        log = tr.optimize_parameters(1, {"real_images": x.to(dev()), "noise": {"y": ny.to(dev()), "z": nz.to(dev())}})
    assert len(sink.masks) == N_GENERATOR_RELUS
    impose = {"masks": sink.masks, "report": {}}
    med = sd_g["entropy_model_z.quantiles"][:, 0, 1].reshape(1, -1, 1, 1)
    forced = {"y": [t.cpu() for t in tr.comp_model.context_model.record_symbols], "z": torch.round(z_hats[0] - med)}
    g_ref, rep = grad_sd(sd_g), {}
    losses, out = O.stage1_losses(g_ref, sd_l, x, ny, nz, forced=forced, report=rep, impose=impose)
    O.check_forced(rep, rep.get("symbols", 0))
    O.check_imposed(impose["report"])
    losses["distortion"] = 1.0 * (1 - R.ms_ssim(x, out["fake_images"], 1.0, torch.float64))
    (losses["distortion"] + losses["rate"] + losses["perceptual"]).backward()
    for k in ("distortion", "rate", "perceptual"):   # the stage-1 step test's loss gate (upstream differences dominate)
        assert abs(log[k] - losses[k].item()) <= 3e-4 * abs(losses[k].item()), (k, log[k], losses[k].item())
    bad = []
    for n, g in captured.items():
        r = g_ref[n].grad
        if n.endswith(".quantiles") or r is None or r.abs().max() == 0:
            continue
        e = rel(g, r)
        if e > 5e-3:
            bad.append((n, e))
    assert not bad, bad[:8]


def test_stage1_msssim_graph_replay_equals_eager():
    from crdr_amd.trainer import build_trainer
    x = seeded_input("image", (2, 3, 192, 192)).to(dev())
    noise = {"y": seeded_input("noise.y", (2, 320, 12, 12), 0.5).to(dev()), "z": seeded_input("noise.z", (2, 192, 3, 3), 0.5).to(dev())}
    logs, params = {}, {}
    for mode in (False, True):
        tr = build_trainer(_msssim_opt(2, 192, graphs=mode))
        _seed_params(tr.comp_model, "")
        _seed_params(tr.perceptual_loss.lpips, "lpips.")
        tr.loss_huge_threshold = float("inf")
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


def test_validation_writes_ms_ssim_columns():
    from crdr_amd.models import build_comp_model
    from crdr_amd.utils.img_utils import calc_ms_ssim
    from crdr_amd.utils.options import BaseConfig, ConfigDict
    cfg, _, _ = BaseConfig._file2dict_yaml(os.path.join(ROOT, "config", "_base_", "model", "interp_ca_elic_charm.yaml"))
    cfg["device"] = "cuda:0"
    model = build_comp_model(ConfigDict(cfg))
    _seed_params(model, "")
    model.to(dev()).eval()
    x = seeded_input("image", (1, 3, 192, 192)).to(dev())
    df = model.validation([{"real_images": x}], max_sample_size=1)
    q = model.rate_level
    want = ["idx"] + [f"{m}_{i + 1}" for i in range(q) for m in ("bpp", "psnr", "ms_ssim")]
    assert list(df.columns) == want, list(df.columns)
    for i in range(q):
        with torch.no_grad():
            out = model.run_model(real_images=x, rate_ind=float(i), is_train=False)
        v = df[f"ms_ssim_{i + 1}"].iloc[0]
        assert v != -1.0 and v == calc_ms_ssim(out["real_images"], out["fake_images"]), (i, v)
