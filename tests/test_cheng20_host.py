"""Host-side checks of the Cheng20 transforms: the float64 restatement (tests/cheng20_ref.py) equals vectors recorded from the
reference's own modules, the HIP modules carry the reference's state-dict keys, the registries hold the four names, what the port
refuses it refuses by name, the fixture's decoder cases do not saturate their tanh, and the two new YAML files merge and name only
registered types.  Construction only: the arithmetic runs on the GPU (tests/test_gpu_cheng20.py)."""
import os

import numpy as np
import pytest
import torch

from tests import cheng20_ref as R
from tests.golden.seeded_weights import fill_state_dict, seeded_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"Cheng20Encoder": "ENCODER_REGISTRY", "Cheng20InterpCaEncoder": "ENCODER_REGISTRY",
         "Cheng20Decoder": "DECODER_REGISTRY", "Cheng20InterpCaDecoder": "DECODER_REGISTRY"}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_cheng20.npz"))


def keys_of(gold, name):
    return [str(k) for k in gold[name]]


def hip_block(tag):
    from crdr_amd.models.layer import cheng_resblock
    cls, args, kw, _ = R.BLOCK_CASES[tag]
    return getattr(cheng_resblock, cls)(*args, **kw)


def hip_transform(tag):
    import crdr_amd.models  # noqa: F401
    from crdr_amd.utils import registry as Rg
    cls, kw = R.XFORM_CASES[tag][:2]
    return getattr(Rg, NAMES[cls]).get(cls)(**kw)


def f64_sd(module, prefix):
    """seeded float64 leaves under the module's own keys, GDN parameters by seed_gdn_"""
    sd = fill_state_dict({prefix + k: v.shape for k, v in module.state_dict().items() if torch.is_floating_point(v) and v.numel()})
    sd = R.seed_gdn_(sd)
    return {k: v.double().requires_grad_(True) for k, v in sd.items()}


def _gate(got, want, name):
    want = torch.from_numpy(np.asarray(want))
    assert tuple(got.shape) == tuple(want.shape), (name, got.shape, want.shape)
    err = float((got.detach() - want).abs().max() / want.abs().max())
    assert err < 1e-9, (name, err)


def _gate_grads(gold, tag, sd, prefix, params):
    ks = R.grad_keys(params)
    assert ks and all(f"{tag}.grad.{k}" in gold.files for k in ks), [k for k in ks if f"{tag}.grad.{k}" not in gold.files]
    for k in ks:
        _gate(R.cut(sd[prefix + k].grad), gold[f"{tag}.grad.{k}"], f"{tag}.grad.{k}")


@pytest.mark.parametrize("tag", sorted(R.BLOCK_CASES))
def test_block_restatement_equals_the_recorded_reference(gold, tag):
    m = hip_block(tag)
    p = f"c20.{tag}."
    sd = f64_sd(m, p)
    x = seeded_input(f"c20.{tag}.x", R.BLOCK_CASES[tag][3]).double().requires_grad_(True)
    y = R.block(sd, p[:-1], x, tag)
    y.backward(seeded_input(p + "cot", tuple(y.shape)).double())
    _gate(y, gold[f"block.{tag}.out"], "out")
    _gate(x.grad, gold[f"block.{tag}.dx"], "dx")
    _gate_grads(gold, f"block.{tag}", sd, p, [k for k, _ in m.named_parameters()])


@pytest.mark.parametrize("tag", sorted(R.XFORM_CASES))
def test_transform_restatement_equals_the_recorded_reference(gold, tag):
    _, _, shape, scale, q, more_q = R.XFORM_CASES[tag]
    m = hip_transform(tag)
    p = f"c20.{tag}."
    sd = f64_sd(m, p)
    x = seeded_input(f"c20.{tag}.x", shape, scale).double().requires_grad_(True)
    y = R.transform(sd, x, tag, q)
    y.backward(seeded_input(p + "cot", tuple(y.shape)).double())
    _gate(y, gold[f"{tag}.out"], "out")
    _gate(x.grad, gold[f"{tag}.dx"], "dx")
    _gate_grads(gold, tag, sd, p, [k for k, _ in m.named_parameters()])
    for qq in more_q:
        with torch.no_grad():
            _gate(R.transform(sd, x, tag, qq), gold[f"{tag}.out.q{qq:g}"], f"out q={qq}")


@pytest.mark.parametrize("tag", sorted(R.BLOCK_CASES))
def test_block_keys_are_the_references(gold, tag):
    assert sorted(hip_block(tag).state_dict()) == keys_of(gold, f"block.{tag}.keys")


@pytest.mark.parametrize("tag", sorted(R.XFORM_CASES))
def test_transform_keys_are_the_references(gold, tag):
    assert sorted(hip_transform(tag).state_dict()) == keys_of(gold, f"{tag}.keys")


def test_default_arguments_are_the_references():
    from crdr_amd.models.subnet.autoencoder.cheng20_autoencoder import Cheng20Decoder, Cheng20Encoder
    e, d = Cheng20Encoder(), Cheng20Decoder()
    assert tuple(e.block1.conv1.weight.shape) == (192, 3, 3, 3) and e.block1.conv1.stride == (2, 2)
    assert tuple(e.block1.shortcut.weight.shape) == (192, 3, 1, 1) and e.block1.shortcut.stride == (2, 2) and e.block1.shortcut.padding == (0, 0)
    assert e.block2.shortcut is None and e.latent_ch == 192 and e.num_downscale == 4
    assert tuple(e.conv7.weight.shape) == (192, 192, 3, 3) and e.conv7.stride == (2, 2)
    assert d.use_tanh is True and tuple(getattr(d.up3, "0").weight.shape) == (12, 192, 3, 3)
    assert tuple(getattr(d.up0.shortcut, "0").weight.shape) == (768, 192, 1, 1) and getattr(d.up0.c1, "4").inverse
    assert Cheng20Encoder(unknown_argument=1) is not None   # **kwargs is accepted and ignored, as in the reference


def test_registries_hold_the_four_names():
    import crdr_amd.models  # noqa: F401
    from crdr_amd.utils import registry as Rg
    for name, reg in NAMES.items():
        assert name in getattr(Rg, reg).keys(), name


@pytest.mark.parametrize("make, word", [
    (lambda B: B.ResBlock(8, 8, bn=True), "bn"),
    (lambda B: B.UpResBlock(8, 8, up_type="interpolate"), "up_type"),
    (lambda B: B.ResBlock(8, 8, padding_mode="reflect"), "padding_mode"),
    (lambda B: B.UpResBlock(8, 8, padding_mode="replicate"), "padding_mode"),
])
def test_refusals_name_the_argument(make, word):
    from crdr_amd.models.layer import cheng_resblock as B
    with pytest.raises(NotImplementedError, match=word):
        make(B)


def test_transforms_pass_the_padding_mode_refusal_on():
    from crdr_amd.models.subnet.autoencoder.cheng20_autoencoder import Cheng20Decoder, Cheng20Encoder
    for cls in (Cheng20Encoder, Cheng20Decoder):
        with pytest.raises(NotImplementedError, match="padding_mode"):
            cls(main_ch=8, padding_mode="reflect")


def test_interpca_encoder_needs_out_ch_equal_main_ch():
    from crdr_amd.models.subnet.autoencoder.cheng20_interpca_autoencoder import Cheng20InterpCaEncoder
    with pytest.raises(AssertionError, match="out_ch .* must equal main_ch"):
        Cheng20InterpCaEncoder(rate_level=5, out_ch=16, main_ch=24, ca_kwargs=R.CA)


@pytest.mark.parametrize("tag", ["dec", "idec"])
def test_fixture_decoders_do_not_saturate_their_tanh(gold, tag):
    """at most a quarter of the reference's recorded pre-tanh values lie beyond |3| (tanh(3) = 0.995: past it the output is +-1 and its
    gradient nothing); the recorded quantiles say the same"""
    frac = float(gold[f"{tag}.pre_tanh.frac_beyond_3"])
    q, v = gold[f"{tag}.pre_tanh.abs_quantiles"]
    print(f"{tag}: {100 * frac:.1f} % of the pre-tanh values beyond |3|; median |x| {v[list(q).index(0.5)]:.2f}")
    assert frac <= 0.25
    assert v[list(q).index(0.75)] <= 3.0


def test_yaml_files_merge_and_name_registered_types():
    import crdr_amd.models  # noqa: F401
    import crdr_amd.trainer  # noqa: F401
    from crdr_amd.utils import registry as Rg
    from crdr_amd.utils.options import BaseConfig
    base, _, _ = BaseConfig._file2dict_yaml(os.path.join(ROOT, "config", "_base_", "model", "interp_ca_cheng20_hyperprior.yaml"))
    full, _, _ = BaseConfig._file2dict_yaml(os.path.join(ROOT, "config", "examples", "cheng20_interp_ca.yaml"))
    where = {"encoder": Rg.ENCODER_REGISTRY, "decoder": Rg.DECODER_REGISTRY, "hyperencoder": Rg.HYPERENCODER_REGISTRY,
             "hyperdecoder": Rg.HYPERDECODER_REGISTRY}
    for cfg in (base, full):
        assert cfg["model_type"] == "InterpCaHyperpriorModel" and cfg["model_type"] in Rg.MODEL_REGISTRY.keys()
        for part, reg in where.items():
            assert cfg["subnet"][part]["type"] in reg.keys(), (part, cfg["subnet"][part]["type"])
        assert cfg["subnet"]["encoder"]["type"] == "Cheng20InterpCaEncoder" and cfg["subnet"]["decoder"]["type"] == "Cheng20InterpCaDecoder"
        assert cfg["subnet"]["encoder"]["out_ch"] == cfg["subnet"]["encoder"]["main_ch"] == cfg["subnet"]["decoder"]["in_ch"] == 192
        assert cfg["subnet"]["decoder"]["use_tanh"] is True and cfg["subnet"]["hyperdecoder"]["out_ch"] == 384
    assert full["trainer"]["type"] == "RateDistortionTrainer" and full["trainer"]["type"] in Rg.TRAINER_REGISTRY.keys()


def test_model_yaml_builds():
    from crdr_amd.models import build_comp_model
    from crdr_amd.utils.options import BaseConfig, ConfigDict
    cfg, _, _ = BaseConfig._file2dict_yaml(os.path.join(ROOT, "config", "_base_", "model", "interp_ca_cheng20_hyperprior.yaml"))
    cfg["device"] = "cpu"
    m = build_comp_model(ConfigDict(cfg))
    assert type(m).__name__ == "InterpCaHyperpriorModel" and m.rate_level == 5
    assert type(m.encoder).__name__ == "Cheng20InterpCaEncoder" and len(m.encoder.interp_ca_list) == 9 and len(m.decoder.interp_ca_list) == 10
