"""GPU tests of the hyperprior-only models and of sub-pixel up-sampling: the pixel-shuffle kernel bit for bit against torch, the
Cheng20 hyper-transforms and the three decoders with `pixel_shuffle=True` against the float64 restatement
(tests/hyperprior_only_ref.py, itself held to the reference's recorded vectors by tests/test_hyperprior_only_host.py), the three
models' training / eval forward and gradients against the restatement with the device's rounding decisions handed over, the codec
round trip with the y string pinned against the torch formulas, and the two entry-point scripts.

The parity tests print their measured ratios under -s."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import hyperprior_only_ref as R
from tests.golden.seeded_weights import seeded_input
from tests.test_gpu_model import check_grads, close, dev, grad_sd, seed_module

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {"plain": ("elic_hyperprior.yaml", {}), "interp": ("interp_ca_elic_hyperprior.yaml", {"rate_ind": 2.0}),
          "beta": ("beta_cond_interp_ca_elic_hyperprior.yaml", {"rate_ind": 2.0, "beta": 3.84})}


def _report(tag):
    """the ratios the helpers of tests/test_gpu_model.py measured in this test so far (shown under -s)"""
    from tests import parity_margins as PM
    for group, m in sorted(PM._measured.get(PM._test_id(), {}).items()):
        if isinstance(m, dict) and "max" in m:
            print(f"{tag} {group}: {m['max']:.3e} (worst: {m['worst']}, n = {m['n']})")


def _f64(sd):
    return {k: v.double().requires_grad_(True) for k, v in sd.items()}


def _nhwc(t):
    return t.to(dev()).contiguous(memory_format=torch.channels_last)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nhw", [(2, 5, 7), (1, 1, 1)])
@pytest.mark.parametrize("C", [3, 4, 8, 96, 256])
def test_pixel_shuffle_is_bit_exact(C, nhw):
    from crdr_amd.hip import functional as HF
    from crdr_amd.hip import ops
    n, h, w = nhw
    x = seeded_input(f"ps.x{C}", (n, 4 * C, h, w)).to(dev())
    cot = seeded_input(f"ps.cot{C}", (n, C, 2 * h, 2 * w)).to(dev())
    xd = _nhwc(x).requires_grad_(True)
    y = HF.pixel_shuffle(xd)
    assert torch.equal(y, F.pixel_shuffle(x, 2))
    y.backward(cot)
    assert torch.equal(xd.grad, F.pixel_unshuffle(cot, 2))
    if C == 3:   # the image layout: pixel stride 4, the fourth lane exactly zero
        yy, ld = ops.nhwc(y)
        assert ld == 4 and yy.data_ptr() == y.data_ptr()
        lanes = torch.as_strided(y.detach(), (n, 2 * h, 2 * w, 4), (4 * h * w * 4, 2 * w * 4, 4, 1))
        assert torch.equal(lanes[..., :3], F.pixel_shuffle(x, 2).permute(0, 2, 3, 1)) and float(lanes[..., 3].abs().max()) == 0.0


def _raw(fn, src, lds, n, h, w, C, dst, ldd):
    from crdr_amd.hip import lib as L
    from crdr_amd.hip import ops
    L.check(getattr(L.load(), fn)(src.data_ptr(), lds, n, h, w, C, dst.data_ptr(), ldd, ops._stream()), fn)


def test_pixel_shuffle_on_channel_slices_leaves_the_rest_alone():
    n, h, w, C = 2, 3, 5, 8
    ldx, ldy, lddy = 4 * C + 8, C + 4, C + 8
    x = seeded_input("ps.slice.x", (n, h, w, ldx)).to(dev())
    y = torch.full((n, 2 * h, 2 * w, ldy), 7.0, device=dev())
    _raw("crdr_pixel_shuffle_fwd", x[..., 4:], ldx, n, h, w, C, y[..., 4:], ldy)    # slices start 16 bytes into the rows
    want = F.pixel_shuffle(x[..., 4:4 + 4 * C].permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert torch.equal(y[..., 4:], want) and bool((y[..., :4] == 7.0).all())
    dy = seeded_input("ps.slice.dy", (n, 2 * h, 2 * w, lddy)).to(dev())
    dx = torch.full((n, h, w, ldx), -3.0, device=dev())
    _raw("crdr_pixel_shuffle_bwd", dy[..., 8:], lddy, n, h, w, C, dx[..., 4:], ldx)
    want = F.pixel_unshuffle(dy[..., 8:].permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert torch.equal(dx[..., 4:4 + 4 * C], want)
    assert bool((dx[..., :4] == -3.0).all()) and bool((dx[..., 4 + 4 * C:] == -3.0).all())


def test_pixel_shuffle_grid_stride_tail():
    """more threads than the capped grid holds (2048 workgroups x 256), by a ragged amount: C = 4 is one thread per input pixel"""
    from crdr_amd.hip import functional as HF
    h, w = 725, 724
    assert h * w > 2048 * 256 and (h * w - 2048 * 256) % 256 != 0
    x = torch.arange(4 * 4 * h * w, dtype=torch.float32, device=dev()).reshape(1, 16, h, w)   # every element distinct (< 2^24)
    xd = _nhwc(x).requires_grad_(True)
    y = HF.pixel_shuffle(xd)
    assert torch.equal(y, F.pixel_shuffle(x, 2))
    y.backward(y.detach())
    assert torch.equal(xd.grad, x)


def test_pixel_shuffle_refusals():
    from crdr_amd.hip.lib import CrdrHipError
    buf = torch.zeros(1 << 12, device=dev())
    with pytest.raises(CrdrHipError):
        _raw("crdr_pixel_shuffle_fwd", buf, 24, 1, 2, 2, 6, buf, 8)          # C = 6
    with pytest.raises(CrdrHipError):
        _raw("crdr_pixel_shuffle_fwd", buf, 34, 1, 2, 2, 8, buf, 8)          # a stride that is no multiple of 4
    with pytest.raises(CrdrHipError):
        _raw("crdr_pixel_shuffle_bwd", buf, 8, 1, 2, 2, 8, buf, 28)          # a stride below the row width
    with pytest.raises(CrdrHipError):
        _raw("crdr_pixel_shuffle_fwd", buf[1:], 32, 1, 2, 2, 8, buf, 8)      # a pointer off the 16-byte grid


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. hyper-transforms, 3. decoders
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["he", "hd"])
def test_hyper_transforms_fwd_bwd(tag):
    from crdr_amd.models.subnet.hyperprior.cheng20_hyperprior import Cheng20HyperDecoder, Cheng20HyperEncoder
    m, shape, fn = ((Cheng20HyperEncoder(**R.HE_KW), (2, 320, 8, 4), R.hyper_encoder) if tag == "he" else
                    (Cheng20HyperDecoder(**R.HD_KW), (2, 192, 2, 1), R.hyper_decoder))
    p = f"ho.{tag}"
    sdg = _f64(seed_module(m, p + "."))
    m.to(dev())
    x = seeded_input(f"{p}.x", shape, 2.0)
    xg = x.double().requires_grad_(True)
    ref = fn(sdg, xg, p)
    cot = seeded_input(f"{p}.cot", tuple(ref.shape))
    ref.backward(cot.double())
    xd = _nhwc(x).requires_grad_(True)
    out = m(xd)
    close(out, ref, f"{tag} out")
    out.backward(cot.to(dev()))
    close(xd.grad, xg.grad, f"{tag} dx")
    check_grads(m, p + ".", sdg, tag)
    _report(f"hyper-transform {tag}")
    if tag == "hd":
        with torch.no_grad():
            assert torch.equal(m.hd_mu(xd), m(xd)[:, :320])


@pytest.mark.parametrize("tag", sorted(R.DEC_CASES))
def test_pixel_shuffle_decoders_fwd_bwd(tag):
    import crdr_amd.models  # noqa: F401
    from crdr_amd.utils.registry import DECODER_REGISTRY
    cls, kw, q, beta = R.DEC_CASES[tag]
    m = DECODER_REGISTRY.get(cls)(**kw)
    p = f"ho.dec.{tag}"
    sdg = _f64(seed_module(m, p + "."))
    m.to(dev())
    args = () if q is None else ((q,) if beta is None else (q, beta))
    x = seeded_input("ho.dec.x", (2, 16, 3, 2), 3.0)
    xg = x.double().requires_grad_(True)
    ref = R.decoder_ps(sdg, xg, q, beta, p=p)
    assert tuple(ref.shape) == (2, 3, 48, 32)
    cot = seeded_input("ho.dec.cot", tuple(ref.shape))
    ref.backward(cot.double())
    xd = _nhwc(x).requires_grad_(True)
    out = m(xd, *args)
    close(out, ref, f"dec {tag} out")
    out.backward(cot.to(dev()))
    close(xd.grad, xg.grad, f"dec {tag} dx")
    check_grads(m, p + ".", sdg, f"dec {tag}")
    _report(f"pixel-shuffle decoder {tag}")
    with torch.no_grad():
        assert torch.equal(m(xd, *args), out)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. models, 5. codec
# ---------------------------------------------------------------------------------------------------------------------------------
def _model(tag):
    from crdr_amd.models import build_comp_model
    from crdr_amd.utils.options import BaseConfig, ConfigDict
    cfg, _, _ = BaseConfig._file2dict_yaml(os.path.join(ROOT, "config", "_base_", "model", MODELS[tag][0]))
    cfg["device"] = "cuda:0"
    model = build_comp_model(ConfigDict(cfg))
    sd = seed_module(model, "")
    return model.to(dev()), sd, MODELS[tag][1]


def _forced(model, out, sd):
    assert len(model.context_model.record_symbols) == 1
    return {"y": model.context_model.record_symbols[0].cpu(),
            "z": torch.round(out["z_hat"].detach().cpu() - sd["entropy_model_z.quantiles"][:, 0, 1].reshape(1, -1, 1, 1))}


@pytest.mark.parametrize("tag", sorted(MODELS))
def test_models_forward_backward(tag):
    from oracle import crdr_oracle as O
    model, sd, kw = _model(tag)
    q, beta = kw.get("rate_ind"), kw.get("beta")
    x = seeded_input("image", (2, 3, 128, 64))
    ny = seeded_input("noise.y", (2, 320, 8, 4), 0.5)
    nz = seeded_input("noise.z", (2, 192, 2, 1), 0.5)
    model.context_model.record_symbols = []
    out = model.run_model(x, is_train=True, noise={"y": ny.to(dev()), "z": nz.to(dev())}, **kw)
    forced = _forced(model, out, sd)
    model.context_model.record_symbols = None
    sdg = grad_sd(sd)
    rep = {}
    ref = R.model_forward(sdg, x, q, beta, ny, nz, forced=forced, report=rep)
    print(f"model {tag} forced decisions: {rep}")
    O.check_forced(rep, rep.get("symbols", 0))
    close(out["y_hat"], ref["y_hat"], "y_hat", 3e-4)
    close(out["z_hat"], ref["z_hat"], "z_hat", 1e-6)
    close(out["fake_images"], ref["fake_images"], "fake_images", 5e-4)
    close(out["bpp"], ref["bpp"], "bpp", 1e-4)
    close(out["qbpp"], ref["qbpp"], "qbpp", 1e-4)
    (ref["fake_images"].square().mean() + ref["bpp"].mean()).backward()
    (out["fake_images"].square().mean() + out["bpp"].mean()).backward()
    check_grads(model, "", sdg, f"model {tag}", tol=5e-3)
    # the no-grad reconstruction is the training forward's
    rec = model.reconstruct(x, **kw)
    assert torch.equal(rec["y_hat"], out["y_hat"]) and torch.equal(rec["z_hat"], out["z_hat"])
    assert torch.equal(rec["fake_images"], out["fake_images"])
    # eval mode
    model.eval()
    model.context_model.record_symbols = []
    with torch.no_grad():
        ev = model.run_model(x, is_train=False, **kw)
        forced = _forced(model, ev, sd)
        model.context_model.record_symbols = None
        rep = {}
        ref = R.model_forward(sd, x, q, beta, is_train=False, forced=forced, report=rep)
    O.check_forced(rep, rep.get("symbols", 0))
    close(ev["bpp"], ref["bpp"], "eval bpp", 1e-4)
    close(ev["fake_images"], ref["fake_images"], "eval fake_images", 5e-4)
    _report(f"model {tag}")


@pytest.mark.parametrize("tag", sorted(MODELS))
def test_codec_roundtrip(tag):
    from oracle import crdr_oracle as O
    from crdr_amd.codec import rans
    model, _, kw = _model(tag)
    ckw = {k: v for k, v in kw.items() if k == "rate_ind"}
    dkw = {k: v for k, v in kw.items() if k == "beta"}
    model.eval()
    model.codec_setup()
    x = seeded_input("ho.codec", (1, 3, 72, 100))
    out = model.compress(x, **ckw)
    strings = out["string_list"]
    assert len(strings) == 3
    assert tuple(out["y_hat"].shape) == (1, 320, 8, 8) and tuple(out["z_hat"].shape) == (1, 192, 2, 2)   # padded to 128 x 128
    fake, z_hat, y_hat = model.decompress(strings, **dkw)
    assert torch.equal(y_hat, out["y_hat"]) and torch.equal(z_hat, out["z_hat"])
    with torch.no_grad():
        ev = model.run_model(x, is_train=False, **kw)
    assert tuple(fake.shape) == (1, 3, 72, 100) and torch.equal(fake, ev["fake_images"])
    assert strings[0] == O.header_bytes((72, 100), out["y_hat"].cpu(), ckw.get("rate_ind"))
    # the y string: the kernel's symbols, indexes and stream order against the torch formulas on the device's own y and hyper_out
    with torch.no_grad():
        xi = model.data_preprocess(x, is_train=False)
        y = model._encode(xi, **ckw)
        z_q = model.entropy_model_z(model.hyperencoder(y), is_train=False)[0]
        mu, sigma = torch.chunk(model.hyperdecoder(z_q), 2, dim=1)
        em = model.entropy_model_y
        sym = em.quantize(y, "symbols", mu).contiguous().cpu().numpy().reshape(-1)
        idx = em.build_indexes(sigma).contiguous().cpu().numpy().reshape(-1)
    assert strings[2] == rans.encode_with_indexes(sym, idx, *em.host_tables())
    # the pipelined sweeps through the inherited code
    imgs = [x, seeded_input("ho.codec2", (1, 3, 64, 130))]
    serial = [model.compress(im, **ckw) for im in imgs]
    piped = list(model.compress_many(imgs, **ckw))
    assert [a["string_list"] for a in serial] == [b["string_list"] for b in piped]
    one = [model.decompress(a["string_list"], **dkw) for a in serial]
    many = list(model.decompress_many([a["string_list"] for a in serial], **dkw))
    for (f0, z0, y0), (f1, z1, y1) in zip(one, many):
        assert torch.equal(f0, f1) and torch.equal(z0, z1) and torch.equal(y0, y1)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. scripts
# ---------------------------------------------------------------------------------------------------------------------------------
def _run(args, cwd, timeout=300):
    import subprocess
    import sys
    env = dict(os.environ, CRDR_AUTOTUNE="0", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-4000:]
    return r.stdout


def _dataset_yaml(tmp_path, eval_dir):
    return f"""pretrained_weight_path: null
ckpt_root: {tmp_path}/checkpoint
hip_graphs: true
dataset:
  batch_size: 2
  train_dataset:
    root_dir: {tmp_path}/train
    name: openimage
    type: ImageDataset
    image_size: 64
    subset_list: [0]
  eval_dataset:
    root_dir: {eval_dir}
    name: Kodak
    type: ImageDataset
"""


def test_example_1_trains_and_compresses(tmp_path):
    """config/examples/example_1.yaml (the "w/o Charm Model" recipe) through scripts/train.py with HIP graphs, then
    scripts/compress.py --decompress on its checkpoint"""
    import json
    from PIL import Image
    from tests.test_gpu_scripts import _png_dir
    train_dir, eval_dir = str(tmp_path / "train" / "0"), str(tmp_path / "kodak")
    _png_dir(train_dir, 4, 80, 96, 7)
    _png_dir(eval_dir, 1, 64, 96, 8)
    os.makedirs(tmp_path / "checkpoint")
    cfg = tmp_path / "tiny_example_1.yaml"
    cfg.write_text(f"_base_: [{os.path.relpath(os.path.join(ROOT, 'config', 'examples', 'example_1.yaml'), str(tmp_path))}]\n"
                   + _dataset_yaml(tmp_path, eval_dir))
    _run([os.path.join(ROOT, "scripts", "train.py"), str(cfg), "-d", "cuda:0", "-b", "2", "-ti", "4", "-s", "4", "-l", "2", "-e", "4", "-nw", "0"],
         cwd=str(tmp_path))
    ckpt = tmp_path / "checkpoint" / "tiny_example_1" / "model" / "comp_model_iter4.pth.tar"
    assert os.path.exists(ckpt), os.listdir(os.path.dirname(ckpt))
    assert not [k for k in torch.load(ckpt, map_location="cpu")["comp_model"] if "context_model" in k]
    out_dir = tmp_path / "out"
    _run([os.path.join(ROOT, "scripts", "compress.py"), "--config_path", str(cfg), "--model_path", str(ckpt), "--img_dir", eval_dir,
          "--save_dir", str(out_dir), "-q", "1.5", "--decompress", "-d", "cuda:0"], cwd=ROOT)
    files = sorted(os.listdir(out_dir))
    assert "im00.bin" in files and "im00.png" in files and "_avg_bitrate.json" in files, files
    assert 0 < list(json.load(open(out_dir / "_avg_bitrate.json")).values())[0] < 24
    assert Image.open(out_dir / "im00.png").size == (96, 64)


def test_stage3_hyperprior_only_with_pixel_shuffle(tmp_path):
    """the GAN trainer (its no-grad high-rate `reconstruct` pass included) and HIP graphs on the beta-conditioned hyperprior-only model
    with sub-pixel up-sampling in the decoder"""
    import yaml
    from tests.test_gpu_scripts import _png_dir
    train_dir, eval_dir = str(tmp_path / "train" / "0"), str(tmp_path / "kodak")
    _png_dir(train_dir, 4, 80, 96, 9)
    _png_dir(eval_dir, 1, 64, 64, 10)
    os.makedirs(tmp_path / "checkpoint")
    stage3 = yaml.safe_load(open(os.path.join(ROOT, "config", "crdr_stage_3.yaml")))   # trainer, discriminator, losses, optimisers
    for k in ("_base_", "pretrained_weight_path"):
        stage3.pop(k)
    base = os.path.relpath(os.path.join(ROOT, "config", "_base_"), str(tmp_path))
    cfg = tmp_path / "tiny_stage3_hyperprior.yaml"
    cfg.write_text(f"_base_: [{base}/default.yaml, {base}/training/default.yaml, {base}/dataset/openimage_kodak.yaml, "
                   f"{base}/model/beta_cond_interp_ca_elic_hyperprior.yaml]\n" + _dataset_yaml(tmp_path, eval_dir)
                   + "subnet:\n  decoder:\n    pixel_shuffle: true\n" + yaml.safe_dump(stage3))
    _run([os.path.join(ROOT, "scripts", "train.py"), str(cfg), "-d", "cuda:0", "-b", "2", "-ti", "4", "-s", "4", "-l", "2", "-e", "4", "-nw", "0"],
         cwd=str(tmp_path))
    ckpt = tmp_path / "checkpoint" / "tiny_stage3_hyperprior" / "model" / "comp_model_iter4.pth.tar"
    assert os.path.exists(ckpt), os.listdir(os.path.dirname(ckpt))
    sd = torch.load(ckpt, map_location="cpu")["comp_model"]
    assert tuple(sd["decoder.conv1.0.weight"].shape) == (1024, 320, 5, 5) and "hyperdecoder.c4.0.weight" in sd
