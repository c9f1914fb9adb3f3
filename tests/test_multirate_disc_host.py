"""CPU-side checks (no GPU) of the InstanceNorm op and the four rate-aware discriminators: registry names and state-dict keys against
the recorded reference (tests/golden/reference_multirate_disc.npz), the optimiser partitions, the float64 restatement
(tests/instance_norm_ref.py) against torch's own instance_norm, and the argument checks of the C entry points, which return before any
HIP call."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import instance_norm_ref as R
from tests.golden.gen_golden_multirate_disc import cases
from tests.golden.seeded_weights import seeded_input

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_multirate_disc.npz")
NAMES = ("SharedBackboneClic21GvaeDiscriminator", "SharedHeadClic21GvaeDiscriminator", "MultirateSeparateClic21GvaeDiscriminator",
         "MultirateSharedRateCondClic21GvaeDiscriminator")
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


def build(cls, kw):
    from crdr_amd.utils.registry import DISCRIMINATOR_REGISTRY
    import crdr_amd.models.discriminator  # noqa: F401  (fills the registry)
    return DISCRIMINATOR_REGISTRY.get(cls)(**kw)


# ---- 1. registry, keys, refusals ------------------------------------------------------------------------------------------------------

def test_the_four_names_resolve():
    from crdr_amd.models.discriminator import build_discriminator
    for name in NAMES:   # default depths (2 + 2, or 4) at the smallest image size whose channel table reaches them
        first = {"SharedBackboneClic21GvaeDiscriminator": "num_head", "SharedHeadClic21GvaeDiscriminator": "num_backbone"}.get(name, "rate_level")
        D = build_discriminator({"type": name, first: 2, "img_size": 64, "main_ch": 8})
        assert type(D).__name__ == name


@pytest.mark.parametrize("tag,cls,kw,grads", CASES, ids=[c[0] for c in CASES])
def test_state_dict_keys_equal_the_recorded_ones(gold, tag, cls, kw, grads):
    D = build(cls, kw)
    assert sorted(D.state_dict().keys()) == [str(k) for k in gold[f"{tag}.keys"]]
    params = dict(D.named_parameters())
    for q in (0, 2):
        for g in grads:
            name = g.format(q=q)
            assert tuple(params[name].shape) == gold[f"{tag}.q{q}.grad.{name}"].shape, name


def test_in_without_affine_adds_no_keys():
    by_tag = {c[0]: c for c in CASES}
    for a, b in (("sb.none.c1", "sb.IN.c1"), ("sh.none.c0", "sh.IN.c0"), ("sep.none", "sep.IN"), ("src.none", "src.IN")):
        assert sorted(build(*by_tag[a][1:3]).state_dict()) == sorted(build(*by_tag[b][1:3]).state_dict())


@pytest.mark.parametrize("name", NAMES)
def test_batch_norm_is_refused(name):
    first = {"SharedBackboneClic21GvaeDiscriminator": "num_head", "SharedHeadClic21GvaeDiscriminator": "num_backbone"}.get(name, "rate_level")
    with pytest.raises(NotImplementedError) as e:
        build(name, {first: 3, "img_size": 64, "main_ch": 8, "norm_type": "BN"})
    assert "'none'" in str(e.value) and "'IN'" in str(e.value)


def test_channel_dict_and_as_list():
    from crdr_amd.models.discriminator.multirate_clic21_gvae_discriminator import as_list, build_channel_dict
    assert build_channel_dict(256, 3, 64, 512) == {256: 3, 128: 64, 64: 128, 32: 256, 16: 512, 8: 512, 4: 512}
    assert build_channel_dict(32, 6, 8, 64) == {32: 6, 16: 8, 8: 16, 4: 32}
    with pytest.raises(AssertionError):
        build_channel_dict(48, 3, 8, 64)
    assert as_list(4, 3) == [4, 4, 4] and as_list([1, 2, 3], 3) == [1, 2, 3]
    with pytest.raises(AssertionError):
        as_list([1, 2], 3)
    with pytest.raises(TypeError):
        as_list(1.5, 3)


# ---- 2. partitions ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,cls,kw,grads", CASES, ids=[c[0] for c in CASES])
def test_partition_modules_cover_the_parameters_in_order(tag, cls, kw, grads):
    D = build(cls, kw)
    mods = D.partition_modules()
    flat = [id(p) for m in mods for p in m.parameters()]
    assert flat == [id(p) for p in D.parameters()], "partitions are not contiguous, in registration order and complete"
    assert all(len(list(m.parameters())) > 0 for m in mods)
    n = len(mods)
    for q in (0, 1, 2, torch.tensor([2.0])):
        parts = D.partitions_for(q)
        assert parts == sorted(set(parts)) and all(0 <= i < n for i in parts)


def test_partitions_per_class():
    by_tag = {c[0]: c for c in CASES}
    sb = build(*by_tag["sb.IN.c0"][1:3])
    assert sb.partition_modules() == [sb.backbone, sb.head_list[0], sb.head_list[1], sb.head_list[2]]
    assert [sb.partitions_for(q) for q in range(3)] == [[0, 1], [0, 2], [0, 3]]
    sh = build(*by_tag["sh.none.c1"][1:3])
    assert sh.partition_modules() == [sh.backbone_list[0], sh.backbone_list[1], sh.backbone_list[2], sh.head]
    assert [sh.partitions_for(q) for q in range(3)] == [[0, 3], [1, 3], [2, 3]]
    sep = build(*by_tag["sep.IN"][1:3])
    assert sep.partition_modules() == list(sep.discriminator_list)
    assert [sep.partitions_for(q) for q in range(3)] == [[0], [1], [2]]
    src = build(*by_tag["src.none"][1:3])
    assert src.partition_modules() == [src.net]
    assert [src.partitions_for(q) for q in range(3)] == [[0], [0], [0]]


# ---- 3. the float64 restatement against torch ---------------------------------------------------------------------------------------------

def scale_err(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("shape", [(2, 4, 1, 2), (3, 8, 9, 7), (2, 12, 70, 75)])
def test_restatement_equals_torch_instance_norm(shape, affine):
    c = shape[1]
    x = seeded_input(f"in.host.x{shape}", shape, R.input_scale(shape)).double()
    w = (1 + 0.3 * seeded_input(f"in.host.w{c}", (c,))).double() if affine else None
    b = (0.2 * seeded_input(f"in.host.b{c}", (c,))).double() if affine else None
    cot = seeded_input(f"in.host.cot{shape}", shape).double()
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b) if t is not None]
    want = F.instance_norm(leaves[0], weight=leaves[1] if affine else None, bias=leaves[2] if affine else None, eps=1e-5)
    want.backward(cot)
    mine = [t.clone().requires_grad_(True) for t in (x, w, b) if t is not None]
    y, z = R.instance_norm(mine[0], mine[1] if affine else None, mine[2] if affine else None)
    y.backward(cot)
    assert torch.equal(y, z)
    assert scale_err(y, want) <= 1e-12
    for a, r in zip(mine, leaves):
        assert scale_err(a.grad, r.grad) <= 1e-12
    dx, dw, db = R.instance_norm_backward(x, w, b, cot)
    assert scale_err(dx, leaves[0].grad) <= 1e-12
    if affine:
        assert scale_err(dw, leaves[1].grad) <= 1e-12 and scale_err(db, leaves[2].grad) <= 1e-12


@pytest.mark.parametrize("act", ["relu", "lrelu"])
def test_restatement_activation_and_written_out_backward_agree(act):
    shape, c = (2, 8, 9, 7), 8
    x = seeded_input("in.host.act.x", shape, 3.0).double().requires_grad_(True)
    w = (1 + 0.3 * seeded_input("in.host.act.w", (c,))).double().requires_grad_(True)
    b = (0.2 * seeded_input("in.host.act.b", (c,))).double().requires_grad_(True)
    cot = seeded_input("in.host.act.cot", shape).double()
    y, z = R.instance_norm(x, w, b, act=act, slope=0.2)
    want = F.instance_norm(x.detach(), weight=w.detach(), bias=b.detach(), eps=1e-5)
    want = F.relu(want) if act == "relu" else F.leaky_relu(want, 0.2)
    assert scale_err(y.detach(), want) <= 1e-12
    y.backward(cot)
    dx, dw, db = R.instance_norm_backward(x.detach(), w.detach(), b.detach(), cot, act=act, slope=0.2)
    assert scale_err(dx, x.grad) <= 1e-12 and scale_err(dw, w.grad) <= 1e-12 and scale_err(db, b.grad) <= 1e-12


# ---- 4. the C entry points refuse bad arguments before any HIP call -------------------------------------------------------------------

def test_library_exports_the_instance_norm_symbols(lib):
    from crdr_amd.hip import lib as L
    raw = C.CDLL(L.LIB_PATH)
    for name in ("crdr_instance_norm_workspace", "crdr_instance_norm_fwd", "crdr_instance_norm_bwd"):
        assert hasattr(raw, name) and name in L.SIGNATURES, name


P = 0x10000   # a 16-byte aligned address that is never dereferenced: every call below must return before a launch


def _desc(**kw):
    from crdr_amd.hip import lib as L
    base = dict(HW=63, N=2, C=64, ldx=64, ldy=64, act=2, slope=0.2, eps=1e-5)
    base.update(kw)
    return L.InstanceNormDesc(**base)


def _fwd(lib, d, x=P, y=P, stats=P, ws=P, gamma=None):
    return lib.crdr_instance_norm_fwd(C.byref(d), x, gamma, None, y, stats, ws, 1 << 30, None)


def _bwd(lib, d, x=P, dy=P, dx=P, stats=P, ws=P, lddy=64, lddx=64):
    return lib.crdr_instance_norm_bwd(C.byref(d), x, None, None, stats, dy, lddy, dx, lddx, None, None, ws, 1 << 30, None)


@pytest.mark.parametrize("what,kw,word", [("C = 6", dict(C=6, ldx=8, ldy=8), "multiple of 4"), ("C = 1028", dict(C=1028, ldx=1028, ldy=1028), "1024"),
                                          ("HW = 1", dict(HW=1), "more than one value"), ("ldx < C", dict(ldx=60), "ldx"),
                                          ("ldx no multiple of 4", dict(ldx=66), "ldx"), ("act = 3", dict(act=3), "act")])
def test_bad_descriptors_are_refused(lib, what, kw, word):
    d = _desc(**kw)
    assert _fwd(lib, d) == -1, what
    assert word in lib.crdr_last_error().decode(), (what, lib.crdr_last_error())
    assert _bwd(lib, d) == -1, what
    assert lib.crdr_instance_norm_workspace(C.byref(d)) == 0, what


def test_bad_pointers_are_refused(lib):
    d = _desc()
    assert lib.crdr_instance_norm_workspace(C.byref(d)) == (2 * 1 * 2 * 64 + 2 * 2 * 64) * 4   # one slab per image, then the sums
    assert _fwd(lib, d, x=None) == -1 and b"null" in lib.crdr_last_error()
    assert _bwd(lib, d, x=None) == -1 and b"null" in lib.crdr_last_error()
    assert _bwd(lib, d, dy=None) == -1
    assert _fwd(lib, d, x=P + 4) == -1 and b"aligned" in lib.crdr_last_error()
    assert _fwd(lib, d, y=P + 8) == -1 and _fwd(lib, d, gamma=P + 4) == -1 and _fwd(lib, d, ws=P + 4) == -1
    assert _bwd(lib, d, dx=P + 4) == -1 and b"aligned" in lib.crdr_last_error()
    assert _fwd(lib, d, ws=None) == -1 and b"workspace" in lib.crdr_last_error()
    assert lib.crdr_instance_norm_fwd(C.byref(d), P, None, None, P, P, P, 16, None) == -1 and b"workspace" in lib.crdr_last_error()
    assert _fwd(lib, _desc(ldy=60)) == -1 and _bwd(lib, d, lddy=60) == -1 and _bwd(lib, d, lddx=62) == -1
    assert lib.crdr_instance_norm_fwd(None, P, None, None, P, P, P, 1 << 30, None) == -1
    assert _fwd(lib, _desc(N=0)) == 0   # an empty batch is no error, and nothing is launched
    slabs = _desc(HW=70 * 75)           # 11 slabs of 512 pixels, the last one ragged
    assert lib.crdr_instance_norm_workspace(C.byref(slabs)) == (2 * 11 * 2 * 64 + 2 * 2 * 64) * 4
