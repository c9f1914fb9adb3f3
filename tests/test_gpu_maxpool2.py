"""HF.maxpool2s2 (crdr_maxpool2s2_fwd / _bwd) against torch's CPU F.max_pool2d(x, 2, 2) and its autograd in float32: bit for bit, ties
included.  A pool moves values and routes gradients; nothing is rounded, so nothing but equality is the gate.

Widths: one quad, a block of 16 x 16, a block of 24 x 10 (240 threads), 128 quads by 2 pixels.  Sizes: a single window, odd in both
directions (the dropped row and column must come back as zeros), more pixels per row than a block covers (45 -> 22 windows + 1 partial;
131 -> 65 + 1), more than one image."""
import pytest
import torch
import torch.nn.functional as F

from tests import lpips_vgg_ref as R
from tests.test_gpu_model import dev

pytestmark = pytest.mark.gpu

WIDTHS = [4, 64, 96, 512]
SIZES = [(1, 2, 2), (2, 5, 7), (2, 35, 45), (1, 2, 131)]


def HF():
    from crdr_amd.hip import functional
    return functional


def cl(t):
    return t.to(dev()).contiguous(memory_format=torch.channels_last)


def _torch_pool(x, cot):
    xr = x.clone().requires_grad_(True)
    y = F.max_pool2d(xr, 2, 2)
    y.backward(cot)
    return y.detach(), xr.grad


@pytest.mark.parametrize("kind", list(R.POOL_INPUTS))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("c", WIDTHS)
def test_maxpool2s2_is_torch_bit_for_bit(c, size, kind):
    n, h, w = size
    x = R.POOL_INPUTS[kind]((n, c, h, w))
    cot = R.pool_cotangent((n, c, h // 2, w // 2))
    y_ref, dx_ref = _torch_pool(x, cot)
    xd = cl(x).requires_grad_(True)
    y = HF().maxpool2s2(xd)
    assert y.shape == y_ref.shape and torch.equal(y.cpu(), y_ref)
    y.backward(cl(cot))
    assert torch.equal(xd.grad.cpu(), dx_ref)
    assert int((dx_ref != 0).sum()) == y_ref.numel()   # one pixel per window took the gradient


@pytest.mark.parametrize("kind", list(R.POOL_INPUTS))
def test_maxpool2s2_channel_slice_equals_dense_copy(kind):
    """x = wide[:, 4:68] of a 96-wide NHWC tensor goes in without a copy and gives the dense copy's result; the wide tensor is left as
    it was"""
    from crdr_amd.hip import ops
    n, h, w = 2, 35, 45
    x = R.POOL_INPUTS[kind]((n, 64, h, w))
    cot = R.pool_cotangent((n, 64, h // 2, w // 2))
    wide_host = R.negative_input((n, 96, h, w)) - 7.0
    wide_host[:, 4:68] = x
    wide = cl(wide_host)
    xs = wide[:, 4:68].detach().requires_grad_(True)
    t, ld = ops.nhwc(xs)
    assert ld == 96 and t.data_ptr() == xs.data_ptr(), "the slice was copied"
    y = HF().maxpool2s2(xs)
    y.backward(cl(cot))
    xd = cl(x).requires_grad_(True)
    y0 = HF().maxpool2s2(xd)
    y0.backward(cl(cot))
    y_ref, dx_ref = _torch_pool(x, cot)
    assert torch.equal(y, y0) and torch.equal(xs.grad, xd.grad)
    assert torch.equal(y.cpu(), y_ref) and torch.equal(xs.grad.cpu(), dx_ref)
    assert torch.equal(wide.cpu(), wide_host)


def test_maxpool2s2_writes_only_its_slice_of_wider_outputs():
    """the C ABI with every stride wider than C: y and dx are channel slices of 96- and 80-wide buffers whose other lanes hold a sentinel"""
    from crdr_amd.hip import lib as L
    from crdr_amd.hip import ops
    lib = L.load()
    n, c, h, w = 2, 64, 5, 7
    x = R.POOL_INPUTS["post_relu"]((n, c, h, w))
    cot = R.pool_cotangent((n, c, h // 2, w // 2))
    y_ref, dx_ref = _torch_pool(x, cot)
    d = dev()
    xw = torch.full((n, h, w, 72), -3.0, device=d)
    xw[..., 8:72] = x.permute(0, 2, 3, 1).to(d)
    gw = torch.full((n, h // 2, w // 2, 68), -5.0, device=d)
    gw[..., 4:68] = cot.permute(0, 2, 3, 1).to(d)
    yw = torch.full((n, h // 2, w // 2, 96), 9.0, device=d)
    dxw = torch.full((n, h, w, 80), 9.0, device=d)
    L.check(lib.crdr_maxpool2s2_fwd(xw.data_ptr() + 32, 72, n, h, w, c, yw.data_ptr() + 64, 96, ops._stream()), "fwd")
    L.check(lib.crdr_maxpool2s2_bwd(xw.data_ptr() + 32, 72, gw.data_ptr() + 16, 68, n, h, w, c, dxw.data_ptr() + 16, 80, ops._stream()), "bwd")
    assert torch.equal(yw[..., 16:80].cpu(), y_ref.permute(0, 2, 3, 1))
    assert torch.equal(dxw[..., 4:68].cpu(), dx_ref.permute(0, 2, 3, 1))
    assert bool((yw[..., :16] == 9).all()) and bool((yw[..., 80:] == 9).all())
    assert bool((dxw[..., :4] == 9).all()) and bool((dxw[..., 68:] == 9).all())


def test_maxpool2s2_refusals():
    from crdr_amd.hip import lib as L
    from crdr_amd.hip import ops
    lib = L.load()
    with pytest.raises(L.CrdrHipError, match="H >= 2"):
        HF().maxpool2s2(cl(torch.zeros(1, 4, 1, 8)))
    with pytest.raises(L.CrdrHipError, match="W >= 2"):
        HF().maxpool2s2(cl(torch.zeros(1, 4, 8, 1)))
    with pytest.raises(L.CrdrHipError, match="multiple of 4"):
        HF().maxpool2s2(cl(torch.zeros(1, 8, 4, 4))[:, 0:6])
    with pytest.raises(L.CrdrHipError, match="CPU tensor"):
        HF().maxpool2s2(torch.zeros(1, 4, 4, 4))
    x, y = torch.zeros(1, 4, 4, 8, device=dev()), torch.zeros(1, 2, 2, 8, device=dev())
    bad = [(x.data_ptr(), 6, 8, y.data_ptr(), 8),        # stride no multiple of 4
           (x.data_ptr(), 4, 8, y.data_ptr(), 8),        # stride below C
           (x.data_ptr(), 8, 8, y.data_ptr(), 4),        # output stride below C
           (x.data_ptr(), 8, 6, y.data_ptr(), 8),        # C no multiple of 4
           (x.data_ptr() + 4, 8, 4, y.data_ptr(), 8)]    # misaligned pointer
    for xp, ldx, c, yp, ldy in bad:
        assert lib.crdr_maxpool2s2_fwd(xp, ldx, 1, 4, 4, c, yp, ldy, ops._stream()) < 0
        assert lib.crdr_maxpool2s2_bwd(xp, ldx, yp, ldy, 1, 4, 4, c, x.data_ptr(), 8, ops._stream()) < 0
    assert lib.crdr_maxpool2s2_bwd(x.data_ptr(), 8, y.data_ptr(), 8, 1, 4, 4, 8, x.data_ptr(), 6, ops._stream()) < 0
