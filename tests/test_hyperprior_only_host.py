"""Host-side checks of the hyperprior-only models and the sub-pixel decoders: the shipped configs build, the registries hold the new
names, the state-dict schemas are the reference's, the float64 restatement (tests/hyperprior_only_ref.py) equals vectors recorded from
the reference's own modules, and the index rule of the pixel-shuffle kernel is F.pixel_shuffle's.  Construction only: the arithmetic
runs on the GPU (tests/test_gpu_hyperprior_only.py)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import hyperprior_only_ref as R
from tests.golden.seeded_weights import fill_state_dict, seeded_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_DIR = os.path.join(ROOT, "config", "_base_", "model")
PAIRS = {"elic_hyperprior.yaml": "elic_charm.yaml", "interp_ca_elic_hyperprior.yaml": "interp_ca_elic_charm.yaml",
         "beta_cond_interp_ca_elic_hyperprior.yaml": "beta_cond_interp_ca_elic_charm.yaml"}
NAMES = {"elic_hyperprior.yaml": "HyperpriorModel", "interp_ca_elic_hyperprior.yaml": "InterpCaHyperpriorModel",
         "beta_cond_interp_ca_elic_hyperprior.yaml": "BetaCondInterpCaHyperpriorModel"}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_hyperprior_only.npz"))


def build(path, **override):
    from crdr_amd.models import build_comp_model
    from crdr_amd.utils.options import BaseConfig, ConfigDict
    cfg, _, _ = BaseConfig._file2dict_yaml(path)
    cfg["device"] = "cpu"
    for k, v in override.items():
        cfg["subnet"]["decoder"][k] = v
    return build_comp_model(ConfigDict(cfg))


def keys_of(gold, name):
    return [str(k) for k in gold[name]]


@pytest.mark.parametrize("yaml", sorted(PAIRS))
def test_model_configs_build_with_the_charm_siblings_keys(gold, yaml):
    m = build(os.path.join(MODEL_DIR, yaml))
    assert type(m).__name__ == NAMES[yaml]
    assert not [k for k in m.state_dict() if k.startswith("context_model.")]
    assert "context_model" not in dict(m.named_children())          # the adapter is no sub-module ...
    for call in ("forward", "reconstruct_latent", "forward_compress_device", "forward_decompress", "seed_noise", "noise_state", "load_noise_state"):
        assert callable(getattr(m.context_model, call))              # ... and answers the calls the base class and the trainers make
    sib = build(os.path.join(MODEL_DIR, PAIRS[yaml]))
    hyper = ("hyperencoder.", "hyperdecoder.")
    want = [k for k in sib.state_dict() if not k.startswith(("context_model.",) + hyper)]
    want += ["hyperencoder." + k for k in keys_of(gold, "he.keys")] + ["hyperdecoder." + k for k in keys_of(gold, "hd.keys")]
    assert sorted(m.state_dict()) == sorted(want)
    assert m.hyperencoder.num_downscale == 2 and m.hyperencoder.latent_ch == 192


def test_example_1_builds_through_its_base_chain():
    m = build(os.path.join(ROOT, "config", "examples", "example_1.yaml"))
    assert type(m).__name__ == "InterpCaHyperpriorModel" and m.rate_level == 3
    assert m.decoder.conv1.weight.shape[1] == 192                   # the example's narrower decoder


def test_registries_hold_the_new_names():
    import crdr_amd.models  # noqa: F401
    from crdr_amd.utils import registry as Rg
    assert set(NAMES.values()) <= set(Rg.MODEL_REGISTRY.keys())
    assert "Cheng20HyperEncoder" in Rg.HYPERENCODER_REGISTRY.keys() and "Cheng20HyperDecoder" in Rg.HYPERDECODER_REGISTRY.keys()


def _decoder(tag, **kw):
    from crdr_amd.utils.registry import DECODER_REGISTRY
    import crdr_amd.models  # noqa: F401
    cls, ckw, _, _ = R.DEC_CASES[tag]
    return DECODER_REGISTRY.get(cls)(**{**ckw, **kw})


@pytest.mark.parametrize("tag", sorted(R.DEC_CASES))
def test_decoder_keys_are_the_references_in_both_forms(gold, tag):
    from crdr_amd.models.layer.elic_layers import SubPixelConv
    from crdr_amd.models.layer.hip_layers import HipConvTranspose2d
    m = _decoder(tag)
    assert sorted(m.state_dict()) == keys_of(gold, f"dec.{tag}.keys")
    assert tuple(m.conv1[0].weight.shape) == (4 * 24, 16, 5, 5) and tuple(m.conv4[0].weight.shape) == (12, 24, 5, 5)
    assert all(isinstance(getattr(m, f"conv{i}"), SubPixelConv) for i in (1, 2, 3, 4))
    t = _decoder(tag, pixel_shuffle=False)
    assert sorted(t.state_dict()) == keys_of(gold, f"dec.{tag}.keys_convt")
    assert all(type(getattr(t, f"conv{i}")) is HipConvTranspose2d for i in (1, 2, 3, 4))
    assert tuple(t.conv1.weight.shape) == (16, 24, 5, 5)


def test_hyper_transform_keys_are_the_references(gold):
    from crdr_amd.models.subnet.hyperprior.cheng20_hyperprior import Cheng20HyperDecoder, Cheng20HyperEncoder
    assert sorted(Cheng20HyperEncoder(**R.HE_KW).state_dict()) == keys_of(gold, "he.keys")
    assert sorted(Cheng20HyperDecoder(**R.HD_KW).state_dict()) == keys_of(gold, "hd.keys")
    e, d = Cheng20HyperEncoder(), Cheng20HyperDecoder()             # the reference's defaults
    assert tuple(e.c1[0].weight.shape) == (192, 192, 3, 3) and tuple(d.c5.weight.shape) == (384, 192, 3, 3)
    assert tuple(d.c2[0].weight.shape) == (192, 192, 4, 4) and d.c2[0].stride == (2, 2) and d.c2[0].padding == (1, 1)
    assert e.c3[0].stride == (2, 2) and e.c5.stride == (2, 2) and e.c2[0].stride == (1, 1)


def _f64_sd(module, prefix):
    sd = fill_state_dict({prefix + k: v.shape for k, v in module.state_dict().items() if torch.is_floating_point(v) and v.numel()})
    return {k: v.double().requires_grad_(True) for k, v in sd.items()}


def _gate(got, want, name):
    want = torch.from_numpy(np.asarray(want))
    assert tuple(got.shape) == tuple(want.shape), (name, got.shape, want.shape)
    err = float((got.detach() - want).abs().max() / want.abs().max())
    assert err < 1e-12, (name, err)


@pytest.mark.parametrize("tag", ["he", "hd"])
def test_hyper_transform_restatement_equals_the_recorded_reference(gold, tag):
    from crdr_amd.models.subnet.hyperprior.cheng20_hyperprior import Cheng20HyperDecoder, Cheng20HyperEncoder
    m, shape, fn, grads = ((Cheng20HyperEncoder(**R.HE_KW), (2, 320, 8, 4), R.hyper_encoder, R.HE_GRADS) if tag == "he" else
                           (Cheng20HyperDecoder(**R.HD_KW), (2, 192, 2, 1), R.hyper_decoder, R.HD_GRADS))
    p = f"ho.{tag}"
    sd = _f64_sd(m, p + ".")
    x = seeded_input(f"{p}.x", shape, 2.0).double().requires_grad_(True)
    y = fn(sd, x, p)
    y.backward(seeded_input(f"{p}.cot", tuple(y.shape)).double())
    _gate(y, gold[f"{tag}.out"], f"{tag}.out")
    _gate(x.grad, gold[f"{tag}.dx"], f"{tag}.dx")
    for k in grads:
        _gate(R.cut(sd[f"{p}.{k}"].grad), gold[f"{tag}.grad.{k}"], f"{tag}.grad.{k}")


@pytest.mark.parametrize("tag", sorted(R.DEC_CASES))
def test_decoder_restatement_equals_the_recorded_reference(gold, tag):
    _, _, q, beta = R.DEC_CASES[tag]
    p = f"ho.dec.{tag}"
    sd = _f64_sd(_decoder(tag), p + ".")
    x = seeded_input("ho.dec.x", (2, 16, 3, 2), 3.0).double().requires_grad_(True)
    y = R.decoder_ps(sd, x, q, beta, p=p)
    y.backward(seeded_input("ho.dec.cot", tuple(y.shape)).double())
    _gate(y, gold[f"dec.{tag}.out"], "out")
    _gate(x.grad, gold[f"dec.{tag}.dx"], "dx")
    seen = 0
    for k in R.DEC_GRADS:
        if f"dec.{tag}.grad.{k}" in gold.files:
            _gate(R.cut(sd[f"{p}.{k}"].grad), gold[f"dec.{tag}.grad.{k}"], k)
            seen += 1
    assert seen == (2 if tag == "plain" else 3)


@pytest.mark.parametrize("C", [3, 4, 8])
def test_kernel_index_rule_is_pixel_shuffle(C):
    """include/crdr_hip.h: y[n][2h+i][2w+j][c] = x[n][h][w][4c+2i+j], and the backward's rule inverts it"""
    N, H, W = 2, 2, 3
    x = torch.arange(N * 4 * C * H * W, dtype=torch.float32).reshape(N, 4 * C, H, W)
    y = torch.zeros(N, C, 2 * H, 2 * W)
    for n in range(N):
        for h in range(H):
            for w in range(W):
                for c in range(C):
                    for i in range(2):
                        for j in range(2):
                            y[n, c, 2 * h + i, 2 * w + j] = x[n, 4 * c + 2 * i + j, h, w]
    assert torch.equal(y, F.pixel_shuffle(x, 2))
    dx = torch.zeros_like(x)
    for n in range(N):
        for h in range(H):
            for w in range(W):
                for c in range(C):
                    for i in range(2):
                        for j in range(2):
                            dx[n, 4 * c + 2 * i + j, h, w] = y[n, c, 2 * h + i, 2 * w + j]
    assert torch.equal(dx, x) and torch.equal(dx, F.pixel_unshuffle(y, 2))


def test_arithmetic_still_refuses_the_cpu():
    from crdr_amd.hip.lib import CrdrHipError
    m = build(os.path.join(MODEL_DIR, "elic_hyperprior.yaml"))
    with pytest.raises(CrdrHipError):
        m.hyperencoder(torch.zeros(1, 320, 4, 4))
