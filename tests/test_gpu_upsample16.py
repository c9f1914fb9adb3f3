"""GPU parity of the x16 up-sample + concat op (csrc/upsample.hip through crdr_amd/hip/functional.py upsample16_cat) against torch on the CPU
in float64: torch.cat((img, F.interpolate(cond, scale_factor=16, mode=..., align_corners=False)), dim=1) and its autograd.

Gates: nearest is pure data movement -- the output equals the ATen composition exactly and dimg is dout's image lanes bit for bit;
bilinear / bicubic forward and dcond within 2e-5 of the scale of the reference tensor (the project's gate for conv and norm ops; torch's own
fp32 result sits 1e-7 .. 2e-7 from float64 on these grids, a wrong phase, tap or clamp is an O(1) error).  Every comparison prints its
figure before it asserts (`-s` yields the margins, profiles/upsample16_test_margins.txt).

Latent grids (h, w): (1, 1) every tap clamps to one element; (1, 2); (2, 3) bicubic clamps at both edges at once; (5, 3) interior phases;
(2, 9) is 144 output columns, more than one workgroup's tile of 128 (UP_TILE_W, csrc/upsample.hip), so partial sums of two column tiles
meet in dcond.  Cc 4, 12, 16 give output pixel strides 8, 16, 20: the condition's 3-float offset meets every quad alignment; Cc 64, the
widest the entry points take, runs once per mode on (2, 3)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.golden.seeded_weights import seeded_input
from tests.test_gpu_instance_norm import gate
from tests.test_gpu_model import dev

pytestmark = pytest.mark.gpu

N = 2
GRIDS = [(1, 1), (1, 2), (2, 3), (5, 3), (2, 9)]
WIDTHS = [4, 12, 16]
MODES = ["nearest", "bilinear", "bicubic"]
TILE_W = 128   # UP_TILE_W of csrc/upsample.hip
assert 16 * GRIDS[-1][1] > TILE_W and all(16 * w <= TILE_W for _, w in GRIDS[:-1])

_REF = {}


def reference(hw, cc, mode):
    """-> (img, cond, cot, out, dimg, dcond): seeded float32 inputs and torch's float64 results on the CPU, computed once per case"""
    key = (hw, cc, mode)
    if key not in _REF:
        h, w = hw
        img = seeded_input(f"up16.img{hw}", (N, 3, 16 * h, 16 * w))
        cond = seeded_input(f"up16.cond{hw}.{cc}", (N, cc, h, w))
        cot = seeded_input(f"up16.cot{hw}.{cc}", (N, 3 + cc, 16 * h, 16 * w))
        i64, c64 = img.double().requires_grad_(True), cond.double().requires_grad_(True)
        kw = {} if mode == "nearest" else {"align_corners": False}
        out = torch.cat((i64, F.interpolate(c64, scale_factor=16, mode=mode, **kw)), dim=1)
        out.backward(cot.double())
        _REF[key] = (img, cond, cot, out.detach(), i64.grad, c64.grad)
    return _REF[key]


def device_inputs(img, cond):
    from crdr_amd.hip import ops
    from crdr_amd.models.layer.hip_layers import to_image_nhwc
    x = to_image_nhwc(img.to(dev())).detach().requires_grad_(True)
    c = ops.dense_nhwc(cond.to(dev())).detach().requires_grad_(True)
    return x, c


def run(img, cond, mode, cot_d, need_img=True, need_cond=True):
    """-> (out, dimg, dcond): the gradients as the op's backward hands them out (torch.autograd.grad; a .grad slot would be a re-laid copy),
    None for an input that asks for none -- its pointer reaches the kernel as null"""
    from crdr_amd.hip import functional as HF
    x, c = device_inputs(img, cond)
    x.requires_grad_(need_img)
    c.requires_grad_(need_cond)
    out = HF.upsample16_cat(x, c, mode)
    wanted = [t for t, need in ((x, need_img), (c, need_cond)) if need]
    got = list(torch.autograd.grad(out, wanted, cot_d))
    return out.detach(), (got.pop(0) if need_img else None), (got.pop(0) if need_cond else None)


def whole_pixels(t):
    """the dense NHWC buffer behind an NCHW view [:, :c] of pixel stride ld, as [N, H, W, ld]"""
    n, c, h, w = t.shape
    ld = t.stride(3)
    return torch.as_strided(t.detach(), (n, h, w, ld), (h * w * ld, w * ld, ld, 1), t.storage_offset())


# the widest condition the entry points take: 17 quads per pixel, so a thread walks several (column, quad) items, and the backward's
# dynamic LDS is 68 KiB (nearest, bilinear) and 136 KiB (bicubic), above the 64 KiB a kernel gets without asking
WIDEST = [((2, 3), 64, m) for m in MODES]


@pytest.mark.parametrize("hw,cc,mode", [(hw, cc, m) for m in MODES for cc in WIDTHS for hw in GRIDS] + WIDEST,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_upsample16_cat_matches_float64(hw, cc, mode):
    img, cond, cot, out_ref, dimg_ref, dcond_ref = reference(hw, cc, mode)
    cot_d = cot.to(dev())
    out, dimg, dcond = run(img, cond, mode, cot_d)
    h, w = hw
    assert tuple(out.shape) == (N, 3 + cc, 16 * h, 16 * w) and out.stride(1) == 1 and out.stride(3) == cc + 4, "dense NHWC, pixel stride Cc + 4"
    tag = f"{hw} Cc {cc} {mode}"
    full = whole_pixels(out)
    assert bool((full[..., 3 + cc:] == 0).all()), "pad lanes must be exact zeros"
    assert torch.equal(out[:, :3].detach(), img.to(dev())), "image lanes are copied bit for bit"
    assert torch.equal(dimg, cot_d[:, :3]), "dimg is dout's image lanes bit for bit"
    gfull = whole_pixels(dimg)
    assert gfull.shape[-1] == 4 and bool((gfull[..., 3] == 0).all()), "lane 3 of dimg must be an exact zero"
    if mode == "nearest":
        aten = torch.cat((img, F.interpolate(cond, scale_factor=16, mode="nearest")), dim=1)
        assert torch.equal(out.detach().cpu(), aten), "nearest is pure data movement"
    gate(f"{tag} out", out, out_ref, 2e-5)
    gate(f"{tag} dcond", dcond, dcond_ref, 2e-5)
    assert torch.equal(dimg.cpu().double(), dimg_ref)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("hw,cc", [((2, 3), 4), ((5, 3), 12), ((2, 9), 16)], ids=["2x3.4", "5x3.12", "2x9.16"])
def test_backward_is_deterministic_and_null_outputs_skip_work(hw, cc, mode):
    """Two backward calls agree bit for bit; asking for dimg alone (generator phase) or dcond alone (discriminator phase) leaves the
    result asked for unchanged bit for bit."""
    img, cond, cot, *_ = reference(hw, cc, mode)
    cot_d = cot.to(dev())

    def grads(need_img, need_cond):
        return run(img, cond, mode, cot_d, need_img, need_cond)[1:]
    a_img, a_cond = grads(True, True)
    b_img, b_cond = grads(True, True)
    assert torch.equal(a_img, b_img) and torch.equal(a_cond, b_cond), "two backward calls must agree bit for bit"
    only_img, none_cond = grads(True, False)
    none_img, only_cond = grads(False, True)
    assert none_cond is None and none_img is None
    assert torch.equal(only_img, a_img) and torch.equal(only_cond, a_cond)
    assert bool((whole_pixels(only_img)[..., 3] == 0).all())


@pytest.mark.parametrize("mode", MODES)
def test_operands_straight_from_the_layers(mode):
    """cond as a HipConv2d output (LeakyReLU in its epilogue), img from to_image_nhwc, the result into a HipConv2d: the module's own path"""
    from crdr_amd.hip import functional as HF
    from crdr_amd.models.layer.hip_layers import HipConv2d, to_image_nhwc
    h, w, cc = 2, 3, 12
    conv = HipConv2d(24, cc, 1).to(dev())
    first = HipConv2d(3 + cc, 8, 3, stride=1, padding=1).to(dev())
    y = seeded_input("up16.layers.y", (N, 24, h, w)).to(dev())
    img = seeded_input("up16.layers.img", (N, 3, 16 * h, 16 * w)).to(dev()).requires_grad_(True)
    cond = conv(y, act="lrelu")
    x = HF.upsample16_cat(to_image_nhwc(img), cond, mode)
    out = first(x, act="lrelu")
    cot = seeded_input("up16.layers.cot", tuple(out.shape)).to(dev())
    out.backward(cot)
    # the same graph on the CPU in float64
    c64 = torch.nn.Conv2d(24, cc, 1).double()
    f64 = torch.nn.Conv2d(3 + cc, 8, 3, padding=1).double()
    with torch.no_grad():
        c64.weight.copy_(conv.weight.detach().cpu().double().view_as(c64.weight)); c64.bias.copy_(conv.bias.detach().cpu().double())
        f64.weight.copy_(first.weight.detach().cpu().double()); f64.bias.copy_(first.bias.detach().cpu().double())
    i64 = img.detach().cpu().double().requires_grad_(True)
    kw = {} if mode == "nearest" else {"align_corners": False}
    up = F.interpolate(F.leaky_relu(c64(y.cpu().double()), 0.2), scale_factor=16, mode=mode, **kw)
    ref = F.leaky_relu(f64(torch.cat((i64, up), dim=1)), 0.2)
    ref.backward(cot.cpu().double())
    gate(f"layers {mode} out", out, ref, 2e-5)
    gate(f"layers {mode} dimg", img.grad, i64.grad, 2e-5)
    gate(f"layers {mode} dW latent conv", conv.weight.grad.view_as(c64.weight), c64.weight.grad, 2e-5)
    gate(f"layers {mode} db latent conv", conv.bias.grad, c64.bias.grad, 2e-5)


def test_refusals():
    from crdr_amd.hip import functional as HF
    from crdr_amd.hip import lib as L
    img = seeded_input("up16.refuse.img", (N, 3, 32, 48)).to(dev())
    with pytest.raises(L.CrdrHipError):
        HF.upsample16_cat(img, seeded_input("up16.refuse.c6", (N, 6, 2, 3)).to(dev()), "bilinear")
    cond = seeded_input("up16.refuse.c8", (N, 8, 2, 3)).to(dev())
    with pytest.raises(L.CrdrHipError):
        HF.upsample16_cat(img, cond, "area")
    with pytest.raises(L.CrdrHipError):
        HF.upsample16_cat(img, cond, 3)
    with pytest.raises(L.CrdrHipError):
        HF.upsample16_cat(img[:, :, :16], cond, "bilinear")   # an image that is not 16 h x 16 w
    # a misaligned pointer, straight at the entry point: refused before any launch
    lib = L.load()
    from crdr_amd.hip import ops
    x, _ = ops.nhwc(img)
    c = ops.dense_nhwc(cond)
    out = torch.empty((N, 32, 48, 12), device=dev())
    d = L.Upsample16Desc(N=N, h=2, w=3, Cc=8, ldi=4, ldc=8, ldo=12, mode=1)
    with pytest.raises(L.CrdrHipError):
        L.check(lib.crdr_upsample16_cat_fwd(C.byref(d), x.data_ptr(), c.data_ptr() + 4, out.data_ptr(), ops._stream()), "upsample16_cat_fwd")
    L.check(lib.crdr_upsample16_cat_fwd(C.byref(d), x.data_ptr(), c.data_ptr(), out.data_ptr(), ops._stream()), "upsample16_cat_fwd")
    torch.cuda.synchronize()
