"""CPU-side checks (no GPU) of CLIC21GVAELatentConditionalDiscriminator and the x16 up-sample + concat op behind it: the registry name,
state-dict keys and shapes against the recorded reference (tests/golden/reference_latent_cond.npz), the constructor's refusals, the
example config, the exported symbols, and the argument checks of the C entry points, which return before any HIP call."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.golden.gen_golden_latent_cond import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "reference_latent_cond.npz")
NAME = "CLIC21GVAELatentConditionalDiscriminator"
CASES = cases()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def lib():
    from crdr_amd.hip import lib as L
    if not os.path.exists(L.LIB_PATH):
        L.build()
    return L.load()


def build(**kw):
    from crdr_amd.utils.registry import DISCRIMINATOR_REGISTRY
    import crdr_amd.models.discriminator  # noqa: F401  (fills the registry)
    return DISCRIMINATOR_REGISTRY.get(NAME)(**kw)


# ---- 1. registry, keys, refusals ------------------------------------------------------------------------------------------------------

def test_the_name_resolves_in_the_registry_and_under_the_alias():
    from crdr_amd.models.discriminator import build_discriminator
    D = build_discriminator({"type": NAME, "y_ch": 24, "latent_nc": 4, "main_ch": 8, "norm_type": "none"})
    assert type(D).__name__ == NAME
    from src.models import build_discriminator as alias_build   # the reference's import path, like its siblings
    from src.utils.registry import DISCRIMINATOR_REGISTRY as alias_registry
    assert alias_registry.get(NAME) is type(D)
    assert type(alias_build({"type": NAME, "y_ch": 24, "latent_nc": 4, "main_ch": 8, "norm_type": "CN"})) is type(D)


@pytest.mark.parametrize("tag,kw,grads", CASES, ids=[c[0] for c in CASES])
def test_state_dict_keys_and_shapes_equal_the_recorded_ones(gold, tag, kw, grads):
    D = build(**kw)
    sd = D.state_dict()
    assert sorted(sd.keys()) == [str(k) for k in gold[f"{tag}.keys"]]
    assert [",".join(str(int(d)) for d in sd[k].shape) for k in sorted(sd.keys())] == [str(s) for s in gold[f"{tag}.shapes"]]
    params = dict(D.named_parameters())
    for g in grads:
        assert tuple(params[g].shape) == gold[f"{tag}.grad.{g}"].shape, g
    assert tuple(params["model.0.weight"].shape) == (16, 7, 3, 3), "the trunk's first conv reads 3 + latent_nc channels"


@pytest.mark.parametrize("kw", [dict(norm_type="BN"), dict(norm_type="IN"), dict()], ids=["BN", "IN", "default"])
def test_batch_and_instance_norm_are_refused(kw):
    with pytest.raises(NotImplementedError) as e:
        build(y_ch=24, latent_nc=4, main_ch=8, **kw)
    assert "'none'" in str(e.value) and "'CN'" in str(e.value)


def test_bad_arguments_are_refused_by_name():
    with pytest.raises(AssertionError):
        build(y_ch=24, latent_nc=4, main_ch=8, norm_type="none", latent_interp_mode="area")
    with pytest.raises(NotImplementedError) as e:
        build(y_ch=24, latent_nc=6, main_ch=8, norm_type="none")
    assert "latent_nc" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        build(in_ch=1, y_ch=24, latent_nc=4, main_ch=8, norm_type="none")
    assert "in_ch" in str(e.value)


def test_the_class_declares_its_per_sample_input():
    assert build(y_ch=24, latent_nc=4, main_ch=8, norm_type="none").BATCH_INPUTS == ("y_hat",)


def test_example_config_loads_and_builds_the_discriminator():
    import crdr_amd.trainer  # noqa: F401
    from crdr_amd.models.discriminator import build_discriminator
    from crdr_amd.utils import registry as Rg
    from crdr_amd.utils.options import BaseConfig
    full, _, _ = BaseConfig._file2dict_yaml(os.path.join(ROOT, "config", "examples", "latent_cond_discriminator.yaml"))
    stage3, _, _ = BaseConfig._file2dict_yaml(os.path.join(ROOT, "config", "crdr_stage_3.yaml"))
    d = full["discriminator"]
    assert d["type"] == "ModuleListDiscriminator" and d["_subd_type"] == NAME and d["_num_subd"] == 5
    assert (d["y_ch"], d["latent_nc"], d["norm_type"], d["latent_interp_mode"]) == (320, 12, "none", "bilinear")
    assert full["trainer"]["type"] == stage3["trainer"]["type"] and full["trainer"]["type"] in Rg.TRAINER_REGISTRY.keys()
    for k in ("loss", "optim", "subnet", "model_type", "total_iter"):
        assert full[k] == stage3[k], f"{k}: the recipe is stage 3's"
    D = build_discriminator(d)
    assert len(D.subD_list) == 5 and all(type(s).__name__ == NAME for s in D.subD_list)
    assert tuple(D.subD_list[0].latent_conv[0].weight.shape)[:2] == (12, 320)
    assert tuple(D.subD_list[4].model.state_dict()["0.weight"].shape) == (64, 15, 3, 3)


# ---- 2. the C entry points ------------------------------------------------------------------------------------------------------------

def test_library_exports_the_upsample_symbols(lib):
    from crdr_amd.hip import functional as HF
    from crdr_amd.hip import lib as L
    raw = C.CDLL(L.LIB_PATH)
    for name in ("crdr_upsample16_cat_workspace", "crdr_upsample16_cat_fwd", "crdr_upsample16_cat_bwd"):
        assert hasattr(raw, name) and name in L.SIGNATURES, name
    assert callable(HF.upsample16_cat) and HF.UPSAMPLE16_MODES == {"nearest": 0, "bilinear": 1, "bicubic": 2}
    assert C.sizeof(L.Upsample16Desc) == 32


P = 0x10000   # a 16-byte aligned address that is never dereferenced: every call below must return before a launch


def _desc(**kw):
    from crdr_amd.hip import lib as L
    base = dict(N=2, h=2, w=3, Cc=12, ldi=4, ldc=12, ldo=16, mode=1)
    base.update(kw)
    return L.Upsample16Desc(**base)


def _fwd(lib, d, img=P, cond=P, out=P):
    return lib.crdr_upsample16_cat_fwd(C.byref(d), img, cond, out, None)


def _bwd(lib, d, dout=P, dimg=P, dcond=P, ws=P, n=1 << 30):
    return lib.crdr_upsample16_cat_bwd(C.byref(d), dout, dimg, dcond, ws, n, None)


@pytest.mark.parametrize("what,kw,word", [("Cc = 6", dict(Cc=6, ldc=8, ldo=12), "multiple of 4"), ("Cc = 68", dict(Cc=68, ldc=68, ldo=72), "64"),
                                          ("Cc = 0", dict(Cc=0), "multiple of 4"), ("mode = 3", dict(mode=3), "mode"),
                                          ("mode = -1", dict(mode=-1), "mode"), ("ldi = 3", dict(ldi=3), "image"),
                                          ("ldc < Cc", dict(ldc=8), "condition"), ("ldc no multiple of 4", dict(ldc=14), "condition"),
                                          ("ldo < Cc + 4", dict(ldo=12), "output"), ("ldo no multiple of 4", dict(ldo=18), "output"),
                                          ("h = 0", dict(h=0), "latent grid"), ("N above 2^20", dict(N=(1 << 20) + 1), "latent grid")])
def test_bad_descriptors_are_refused(lib, what, kw, word):
    d = _desc(**kw)
    assert _fwd(lib, d) == -1, what
    assert word in lib.crdr_last_error().decode(), (what, lib.crdr_last_error())
    assert _bwd(lib, d) == -1, what
    assert lib.crdr_upsample16_cat_workspace(C.byref(d)) == 0, what


def test_bad_pointers_are_refused_and_the_workspace_follows_the_tiling(lib):
    d = _desc()
    # bilinear: (h + 1) bands x 2 staged rows x column tiles x 9 staged column slots x (Cc + 4) lanes; 48 output columns are one tile
    assert lib.crdr_upsample16_cat_workspace(C.byref(d)) == 2 * 3 * 2 * 1 * 9 * 16 * 4
    assert lib.crdr_upsample16_cat_workspace(C.byref(_desc(mode=2))) == 2 * 3 * 4 * 1 * 11 * 16 * 4
    assert lib.crdr_upsample16_cat_workspace(C.byref(_desc(w=9))) == 2 * 3 * 2 * 2 * 9 * 16 * 4   # 144 columns: two tiles of 128
    assert _fwd(lib, d, img=None) == -1 and b"null" in lib.crdr_last_error()
    assert _fwd(lib, d, cond=None) == -1 and _fwd(lib, d, out=None) == -1
    assert _bwd(lib, d, dout=None) == -1 and b"null" in lib.crdr_last_error()
    assert _fwd(lib, d, img=P + 4) == -1 and b"aligned" in lib.crdr_last_error()
    assert _fwd(lib, d, cond=P + 8) == -1 and _fwd(lib, d, out=P + 4) == -1
    assert _bwd(lib, d, dout=P + 4) == -1 and b"aligned" in lib.crdr_last_error()
    assert _bwd(lib, d, dimg=P + 4) == -1 and _bwd(lib, d, dcond=P + 8) == -1 and _bwd(lib, d, ws=P + 4) == -1
    assert _bwd(lib, d, ws=None) == -1 and b"workspace" in lib.crdr_last_error()
    assert _bwd(lib, d, n=16) == -1 and b"workspace" in lib.crdr_last_error()
    assert lib.crdr_upsample16_cat_fwd(None, P, P, P, None) == -1
    assert _fwd(lib, _desc(N=0)) == 0 and _bwd(lib, _desc(N=0)) == 0   # an empty batch is no error, and nothing is launched
    assert _bwd(lib, d, dimg=None, dcond=None) == 0                     # nothing asked for: nothing launched
