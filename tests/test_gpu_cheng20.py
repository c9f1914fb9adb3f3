"""GPU tests of the Cheng20 transforms and of the device work they add: GDN / IGDN with the shortcut fused into its epilogue
(crdr_gdn_res_fwd) and the tanh op (crdr_tanh_fwd / _bwd) against float64, the 1x1 stride-2 conv of the down-sampling shortcut against
float64 F.conv2d, the blocks and the four transforms against the float64 restatement (tests/cheng20_ref.py, itself held to the
reference's recorded vectors by tests/test_cheng20_host.py), the full-width transforms, the model of the new YAML and the two scripts.

Gates: 2e-5 of the reference tensor's largest magnitude for forward values and input gradients of single ops, 5e-5 for GDN parameter
gradients, close / grad_close / check_grads of tests/test_gpu_model.py with their defaults for whole transforms.  Every comparison
prints its figure (shown under -s)."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

from tests import cheng20_ref as R
from tests.golden.seeded_weights import seeded_input
from tests.test_gpu_gdn import _gdn_f64
from tests.test_gpu_model import check_grads, close, dev, grad_close, rel, seed_module

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nhwc(t):
    return t.to(dev()).contiguous(memory_format=torch.channels_last)


def _maxrel(got, ref, what, tol):
    """max |got - ref| / max |ref|, printed, then gated"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    e = float((got - ref).abs().max() / (ref.abs().max() + 1e-300))
    print(f"{what}: {e:.3e} of the largest magnitude (gate {tol:.0e})")
    assert e <= tol, (what, e)
    return e


def _report(tag):
    from tests import parity_margins as PM
    for group, m in sorted(PM._measured.get(PM._test_id(), {}).items()):
        if isinstance(m, dict) and "max" in m:
            print(f"{tag} {group}: {m['max']:.3e} (worst: {m['worst']}, n = {m['n']})")


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. GDN with the fused shortcut, 2. GDN without it
# ---------------------------------------------------------------------------------------------------------------------------------
def _gdn(c, inverse, seed):
    from crdr_amd.models.layer.gdn import GDN
    m = GDN(c, inverse=inverse)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.gamma.copy_(torch.sqrt(torch.rand(c, c, generator=g) * 0.02 + 2.0 ** -36))
        m.beta.copy_(torch.sqrt(torch.rand(c, generator=g) + 0.5))
    return m.to(dev()), g


def _gdn_desc(m, x, ldx, ldy):
    from crdr_amd.hip import lib as L
    n, c, h, w = x.shape
    d = L.GdnDesc(M=n * h * w, C=c, ldx=ldx, ldy=ldy, inverse=int(m.inverse), beta_min=m.beta_min, reparam_offset=m.reparam_offset)
    nb = L.load().crdr_gdn_workspace(C.byref(d), 0)
    ws = torch.empty(nb + 256, dtype=torch.uint8, device=x.device)
    return d, ws, (ws.data_ptr() + 255) // 256 * 256, nb


def _raw_res_fwd(m, x, res_ptr, ldres, y, x_ptr=None, y_ptr=None):
    """crdr_gdn_res_fwd on dense NHWC x / y with the shortcut handed over as (pointer, stride); -> return code"""
    from crdr_amd.hip import lib as L
    from crdr_amd.hip import ops
    c = x.shape[1]
    d, ws, p, nb = _gdn_desc(m, x, c, c)
    rc = L.load().crdr_gdn_res_fwd(C.byref(d), x.data_ptr() if x_ptr is None else x_ptr, m.beta.data_ptr(), m.gamma.data_ptr(), res_ptr, ldres,
                                   y.data_ptr() if y_ptr is None else y_ptr, p, nb, ops._stream())
    torch.cuda.synchronize()
    return rc


GDN_RES_SHAPES = [(192, 2, 9, 7),        # two tiles, ragged
                  (64, 1, 16, 16),       # NS = 4
                  (128, 3, 10, 7),       # NS = 8, ragged
                  (36, 3, 5, 5),         # channels that do not fill the padded blocks
                  (192, 2, 100, 100),    # 313 tiles of 64 pixels > 256 persistent workgroups: deferred stores and shortcut loads of a second tile
                  (64, 4, 75, 75),       # 352 tiles
                  (224, 2, 9, 7)]        # the route beyond 192 channels


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("c,n,h,w", GDN_RES_SHAPES)
def test_gdn_res_fwd_bwd_vs_float64(inverse, c, n, h, w):
    m, g = _gdn(c, inverse, 23 + c + int(inverse))
    x = _nhwc(torch.randn(n, c, h, w, generator=g) * 2.0)
    res = _nhwc(torch.randn(n, c, h, w, generator=g) * 1.5)
    cot = _nhwc(torch.randn(n, c, h, w, generator=g))
    y64, dx64, db64, dg64 = _gdn_f64(m, x, cot, inverse)
    y64 = y64 + res.double()

    def run():
        m.zero_grad(set_to_none=True)
        xd, rd = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
        y = m(xd, rd)
        (y * cot).sum().backward()
        torch.cuda.synchronize()
        return y.detach().clone(), xd.grad.clone(), rd.grad.clone(), m.beta.grad.clone(), m.gamma.grad.clone()
    y, dx, dres, db, dg = run()
    with torch.no_grad():
        unfused = m(x) + res     # the pair this launch replaces
    tag = f"gdn_res c={c} {'igdn' if inverse else 'gdn'} {n}x{h}x{w}"
    e = _maxrel(y, y64, tag + " forward", 2e-5)
    e_u = float((unfused.double() - y64).abs().max() / y64.abs().max())
    print(f"{tag}: fused {e:.3e}, GDN then add {e_u:.3e}")
    assert e <= 3 * e_u + 2e-6, (e, e_u)
    _maxrel(dx, dx64, tag + " dx", 2e-5)
    for name, a, r in (("dbeta", db, db64), ("dgamma", dg, dg64)):
        ee = rel(a.double(), r)
        print(f"{tag} {name}: relative L2 {ee:.3e} (gate 5e-5)")
        assert ee < 5e-5, (name, ee)
    assert torch.equal(dres, cot), "the shortcut's gradient is not dy bit for bit"
    again = run()
    assert all(torch.equal(a, b) for a, b in zip((y, dx, dres, db, dg), again)), "two runs differ"


@pytest.mark.parametrize("c", [192, 36, 224])
def test_gdn_res_from_a_channel_slice_equals_the_dense_shortcut(c):
    from crdr_amd.hip import ops
    n, h, w = 2, 9, 7
    m, g = _gdn(c, False, 5 + c)
    x = _nhwc(torch.randn(n, c, h, w, generator=g) * 2.0)
    wide = torch.randn(n, h, w, c + 8, generator=g).to(dev())
    res = wide[..., 4:4 + c].permute(0, 3, 1, 2)     # starts 16 bytes into the row, pixel stride C + 8
    r2, ld = ops.nhwc(res)
    assert ld == c + 8 and r2.data_ptr() == res.data_ptr() == wide.data_ptr() + 16
    with torch.no_grad():
        y_slice = m(x, res)
        y_dense = m(x, res.contiguous(memory_format=torch.channels_last))
    assert torch.equal(y_slice, y_dense)
    assert float((y_slice.double() - (_gdn_f64(m, x, torch.zeros_like(x), False)[0] + res.double())).abs().max()) < 2e-5 * float(y_dense.abs().max())


def test_gdn_res_refusals():
    c, n, h, w = 64, 1, 4, 4
    m, g = _gdn(c, False, 3)
    x = _nhwc(torch.randn(n, c, h, w, generator=g))
    buf = torch.zeros(n * h * w * (c + 8) + 8, device=dev())
    y = torch.empty_like(x)
    assert _raw_res_fwd(m, x, buf.data_ptr(), c, y) == 0                       # the accepted form
    assert _raw_res_fwd(m, x, None, c, y) < 0                                  # res NULL
    assert _raw_res_fwd(m, x, buf.data_ptr(), c + 2, y) < 0                    # ldres not a multiple of 4
    assert _raw_res_fwd(m, x, buf.data_ptr(), c - 4, y) < 0                    # ldres below C
    assert _raw_res_fwd(m, x, buf.data_ptr() + 4, c, y) < 0                    # res off the 16-byte grid
    assert _raw_res_fwd(m, x, buf.data_ptr(), c, y, x_ptr=x.data_ptr() + 4) < 0
    assert _raw_res_fwd(m, x, buf.data_ptr(), c, y, y_ptr=buf.data_ptr() + 16) < 0   # res overlaps y
    assert _raw_res_fwd(m, x, y.data_ptr(), c, y) < 0


@pytest.mark.parametrize("inverse", [False, True])
def test_gdn_without_shortcut_is_still_crdr_gdn_fwd(inverse):
    from crdr_amd.hip import lib as L
    from crdr_amd.hip import ops
    c, n, h, w = 192, 2, 100, 100
    m, g = _gdn(c, inverse, 41 + int(inverse))
    x = _nhwc(torch.randn(n, c, h, w, generator=g) * 2.0)
    with torch.no_grad():
        y_mod = m(x)
    y_raw = torch.empty(n, h, w, c, device=dev()).permute(0, 3, 1, 2)
    d, ws, p, nb = _gdn_desc(m, x, c, c)
    L.check(L.load().crdr_gdn_fwd(C.byref(d), x.data_ptr(), m.beta.data_ptr(), m.gamma.data_ptr(), y_raw.data_ptr(), p, nb, ops._stream()), "gdn_fwd")
    torch.cuda.synchronize()
    assert torch.equal(y_mod, y_raw)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. tanh
# ---------------------------------------------------------------------------------------------------------------------------------
def _tanh_raw(fn, *args):
    from crdr_amd.hip import lib as L
    from crdr_amd.hip import ops
    ptr = lambda a: a.data_ptr() if torch.is_tensor(a) else a
    rc = getattr(L.load(), fn)(*[ptr(a) for a in args], ops._stream())
    torch.cuda.synchronize()
    return rc


def _planted(tag, shape):
    x = seeded_input(tag, shape, 20.0)
    flat = x.reshape(-1)
    flat[0], flat[1], flat[2] = 20.0, -20.0, 0.0
    return x


@pytest.mark.parametrize("shape", [(2, 32, 5, 3), (2, 3, 5, 3)])
def test_tanh_vs_float64(shape):
    from crdr_amd.hip import functional as HF
    from crdr_amd.hip import ops
    x = _planted(f"tanh.x{shape[1]}", shape)
    cot = seeded_input(f"tanh.cot{shape[1]}", shape)
    xr = x.double().requires_grad_(True)
    ref = torch.tanh(xr)
    ref.backward(cot.double())
    xd = ops.nhwc(x.to(dev()))[0].detach().requires_grad_(True)
    y = HF.tanh(xd)
    _maxrel(y, ref, f"tanh forward C={shape[1]}", 2e-5)
    y.backward(cot.to(dev()))
    _maxrel(xd.grad, xr.grad, f"tanh backward C={shape[1]}", 2e-5)
    if shape[1] == 3:   # the image layout: pixel stride 4 and the library's own zero fourth lane
        yy, ld = ops.nhwc(y)
        assert ld == 4 and yy.data_ptr() == y.data_ptr()


def test_tanh_image_layout_writes_the_fourth_lane_as_zero():
    n, h, w = 2, 5, 3
    x = _planted("tanh.img.x", (n, h, w, 4)).to(dev())            # lane 3 holds garbage in every operand
    dy = seeded_input("tanh.img.dy", (n, h, w, 4)).to(dev())
    assert float(x[..., 3].abs().min()) > 0 and float(dy[..., 3].abs().min()) > 0
    y = torch.full((n, h, w, 4), 7.0, device=dev())
    dx = torch.full((n, h, w, 4), 7.0, device=dev())
    assert _tanh_raw("crdr_tanh_fwd", x, 4, n * h * w, 3, y, 4) == 0
    assert _tanh_raw("crdr_tanh_bwd", y, 4, dy, 4, n * h * w, 3, dx, 4) == 0
    assert float(y[..., 3].abs().max()) == 0.0 and float(dx[..., 3].abs().max()) == 0.0
    ref = torch.tanh(x[..., :3].double())
    _maxrel(y[..., :3], ref, "tanh image forward", 2e-5)
    _maxrel(dx[..., :3], dy[..., :3].double() * (1 - ref * ref), "tanh image backward", 2e-5)


def test_tanh_on_channel_slices_leaves_the_rest_alone_and_in_place_is_the_same():
    n, h, w, c = 2, 3, 5, 8
    M, ld = n * h * w, c + 8
    x = _planted("tanh.slice.x", (n, h, w, ld)).to(dev())
    y = torch.full((n, h, w, ld), 7.0, device=dev())
    assert _tanh_raw("crdr_tanh_fwd", x[..., 4:], ld, M, c, y[..., 4:], ld) == 0      # slices start 16 bytes into the rows
    _maxrel(y[..., 4:4 + c], torch.tanh(x[..., 4:4 + c].double()), "tanh slice forward", 2e-5)
    assert bool((y[..., :4] == 7.0).all()) and bool((y[..., 4 + c:] == 7.0).all())
    dy = seeded_input("tanh.slice.dy", (n, h, w, ld)).to(dev())
    dx = torch.full((n, h, w, ld), -3.0, device=dev())
    assert _tanh_raw("crdr_tanh_bwd", y[..., 4:], ld, dy[..., 4:], ld, M, c, dx[..., 4:], ld) == 0
    t = torch.tanh(x[..., 4:4 + c].double())
    _maxrel(dx[..., 4:4 + c], dy[..., 4:4 + c].double() * (1 - t * t), "tanh slice backward", 2e-5)
    assert bool((dx[..., :4] == -3.0).all()) and bool((dx[..., 4 + c:] == -3.0).all())
    # in place: x aliasing y, dy aliasing dx
    xi, dyi = x.clone(), dy.clone()
    assert _tanh_raw("crdr_tanh_fwd", xi[..., 4:], ld, M, c, xi[..., 4:], ld) == 0
    assert torch.equal(xi[..., 4:4 + c], y[..., 4:4 + c]) and torch.equal(xi[..., :4], x[..., :4]) and torch.equal(xi[..., 4 + c:], x[..., 4 + c:])
    assert _tanh_raw("crdr_tanh_bwd", y[..., 4:], ld, dyi[..., 4:], ld, M, c, dyi[..., 4:], ld) == 0
    assert torch.equal(dyi[..., 4:4 + c], dx[..., 4:4 + c]) and torch.equal(dyi[..., :4], dy[..., :4])


def test_tanh_grid_stride_tail():
    """more quads than the capped grid holds (8192 workgroups x 256 threads, one quad each), by a ragged amount: C = 3 is one quad per pixel"""
    from crdr_amd.hip import functional as HF
    h, w = 1449, 1448
    assert h * w > 8192 * 256 and (h * w - 8192 * 256) % 256 != 0
    x = (torch.arange(h * w * 3, dtype=torch.float32, device=dev()).reshape(1, h, w, 3) % 4001.0 - 2000.0) / 500.0
    xd = x.permute(0, 3, 1, 2).requires_grad_(True)
    y = HF.tanh(xd)
    ref = torch.tanh(x.double()).permute(0, 3, 1, 2)
    _maxrel(y, ref, "tanh tail forward", 2e-5)
    y.backward(torch.ones_like(y))
    _maxrel(xd.grad, 1 - ref * ref, "tanh tail backward", 2e-5)


def test_tanh_refusals():
    buf = torch.zeros(1 << 12, device=dev())
    p = buf.data_ptr()
    assert _tanh_raw("crdr_tanh_fwd", p, 8, 4, 8, p + 4096, 8) == 0
    assert _tanh_raw("crdr_tanh_fwd", p, 10, 4, 8, p + 4096, 8) < 0            # a stride that is no multiple of 4
    assert _tanh_raw("crdr_tanh_fwd", p, 8, 4, 8, p + 4096, 4) < 0             # a stride below the row width
    assert _tanh_raw("crdr_tanh_fwd", p, 4, 4, 6, p + 4096, 8) < 0             # ... below the ROUNDED row width
    assert _tanh_raw("crdr_tanh_fwd", p + 4, 8, 4, 8, p + 4096, 8) < 0         # a pointer off the 16-byte grid
    assert _tanh_raw("crdr_tanh_fwd", None, 8, 4, 8, p + 4096, 8) < 0
    assert _tanh_raw("crdr_tanh_fwd", p, 8, 4, 8, p, 16) < 0                   # in place with two strides
    assert _tanh_raw("crdr_tanh_fwd", p, 8, 4, 0, p + 4096, 8) < 0             # no channels
    assert _tanh_raw("crdr_tanh_bwd", p, 8, p + 4096, 8, 4, 8, p + 8192, 8) == 0
    assert _tanh_raw("crdr_tanh_bwd", p, 8, p + 4096, 6, 4, 8, p + 8192, 8) < 0
    assert _tanh_raw("crdr_tanh_bwd", p, 8, p + 4096, 8, 4, 8, p + 8192 + 8, 8) < 0
    assert _tanh_raw("crdr_tanh_bwd", p, 4, p + 4096, 8, 4, 8, p + 8192, 8) < 0


@pytest.mark.parametrize("with_affine", [False, True])
def test_add_affine_vs_float64(with_affine):
    """the sum that ends a block whose second activation is conv2's epilogue (crdr_add_affine), one addend a channel slice of a wider
    tensor; values and all gradients at 2e-5, the affine's own gradients by the conv tests' 1e-3 of test_epilogue_bwd"""
    from crdr_amd.hip import functional as HF
    n, c, h, w = 2, 24, 5, 3
    a = seeded_input("addaff.a", (n, c, h, w), 2.0)
    wide = seeded_input("addaff.r", (n, h, w, c + 8), 2.0)
    cot = seeded_input("addaff.cot", (n, c, h, w))
    s, t = seeded_input("addaff.s", (c,)) + 1.5, seeded_input("addaff.t", (c,))
    a64, r64 = a.double().requires_grad_(True), wide[..., 4:4 + c].permute(0, 3, 1, 2).double().requires_grad_(True)
    s64, t64 = s.double().requires_grad_(True), t.double().requires_grad_(True)
    ref = a64 + r64
    if with_affine:
        ref = ref * s64.view(1, -1, 1, 1) + t64.view(1, -1, 1, 1)
    ref.backward(cot.double())
    ad = _nhwc(a).requires_grad_(True)
    wd = wide.to(dev()).requires_grad_(True)
    sd, td = s.to(dev()).requires_grad_(True), t.to(dev()).requires_grad_(True)
    out = HF.add_affine(ad, wd[..., 4:4 + c].permute(0, 3, 1, 2), (sd, td) if with_affine else None)
    _maxrel(out, ref, "add_affine forward", 2e-5)
    out.backward(cot.to(dev()))
    _maxrel(ad.grad, a64.grad, "add_affine da", 2e-5)
    _maxrel(wd.grad[..., 4:4 + c].permute(0, 3, 1, 2), r64.grad, "add_affine dr", 2e-5)
    assert float(wd.grad[..., :4].abs().max()) == 0.0 and float(wd.grad[..., 4 + c:].abs().max()) == 0.0
    if with_affine:
        _maxrel(sd.grad, s64.grad, "add_affine dscale", 1e-3)
        _maxrel(td.grad, t64.grad, "add_affine dshift", 1e-3)


def test_add_affine_refusals():
    from crdr_amd.hip import lib as L
    from crdr_amd.hip import ops
    buf = torch.zeros(1 << 12, device=dev())
    p = buf.data_ptr()
    call = lambda *a: L.load().crdr_add_affine(*a, ops._stream())
    assert call(p, 8, p + 4096, 8, None, None, p + 8192, 8, 4, 8) == 0
    assert call(p, 8, p + 4096, 8, p + 12288, None, p + 8192, 8, 4, 8) < 0      # scale without shift
    assert call(p, 8, p + 4096, 6, None, None, p + 8192, 8, 4, 8) < 0           # a stride that is no multiple of 4
    assert call(p, 8, p + 4096, 8, None, None, p + 8192, 4, 4, 8) < 0           # a stride below C
    assert call(p, 8, p + 4096, 8, None, None, p + 8192, 8, 4, 6) < 0           # C no multiple of 4
    assert call(p + 4, 8, p + 4096, 8, None, None, p + 8192, 8, 4, 8) < 0       # a pointer off the 16-byte grid
    assert call(None, 8, p + 4096, 8, None, None, p + 8192, 8, 4, 8) < 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the 1x1 stride-2 conv of the down-sampling shortcut
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ci,h,w,co", [(2, 24, 9, 7, 24), (2, 192, 10, 6, 192), (2, 3, 9, 7, 24)])
def test_conv_1x1_stride_2(n, ci, h, w, co):
    from crdr_amd.models.layer.hip_layers import HipConv2d
    from tests.test_gpu_conv import _close, _rand
    m = HipConv2d(ci, co, 1, stride=2)
    with torch.no_grad():
        m.weight.copy_(_rand(co, ci, 1, 1, seed=2, scale=ci ** -0.5))
        m.bias.copy_(_rand(co, seed=3))
    x = _rand(n, ci, h, w, seed=1)
    xr, wr, br = x.double().requires_grad_(True), m.weight.detach().double().requires_grad_(True), m.bias.detach().double().requires_grad_(True)
    ref = F.conv2d(xr, wr, br, stride=2)
    assert tuple(ref.shape[2:]) == ((h + 1) // 2, (w + 1) // 2)
    dy = _rand(*ref.shape, seed=4)
    ref.backward(dy.double())
    m.to(dev())
    xd = x.to(dev()).requires_grad_(True)
    out = m(xd)
    assert out.shape == ref.shape
    _close(out, ref, "1x1 s2 fwd")
    out.backward(dy.to(dev()))
    torch.cuda.synchronize()
    _close(xd.grad, xr.grad, "1x1 s2 dgrad")
    _close(m.weight.grad, wr.grad, "1x1 s2 wgrad")
    _close(m.bias.grad, br.grad, "1x1 s2 dbias")
    for name, a, b in (("fwd", out, ref), ("dgrad", xd.grad, xr.grad), ("wgrad", m.weight.grad, wr.grad), ("dbias", m.bias.grad, br.grad)):
        print(f"1x1 s2 {ci}->{co} {name}: {float((a.detach().cpu().double() - b.detach()).abs().max() / b.detach().abs().max()):.3e}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. blocks and transforms against the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def _seeded(m, prefix):
    """HIP module on the device with seeded weights (GDN parameters by seed_gdn_) and the float64 leaves of the same values"""
    sd = seed_module(m, prefix)
    R.seed_gdn_(m, prefix)
    sd = R.seed_gdn_(sd)
    sdg = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    return m.to(dev()), sdg


@pytest.mark.parametrize("tag", sorted(R.BLOCK_CASES))
def test_blocks_fwd_bwd(tag):
    from tests.test_cheng20_host import hip_block
    m, sdg = _seeded(hip_block(tag), f"c20.{tag}.")
    x = seeded_input(f"c20.{tag}.x", R.BLOCK_CASES[tag][3])
    xg = x.double().requires_grad_(True)
    ref = R.block(sdg, f"c20.{tag}", xg, tag)
    cot = seeded_input(f"c20.{tag}.cot", tuple(ref.shape))
    ref.backward(cot.double())
    xd = x.to(dev()).requires_grad_(True)
    out = m(xd)
    close(out, ref, f"block {tag} out")
    out.backward(cot.to(dev()))
    close(xd.grad, xg.grad, f"block {tag} dx")
    check_grads(m, f"c20.{tag}.", sdg, f"block {tag}")
    _report(f"block {tag}")


@pytest.mark.parametrize("tag", sorted(R.XFORM_CASES))
def test_transforms_fwd_bwd(tag):
    from tests.test_cheng20_host import hip_transform
    _, _, shape, scale, q, more_q = R.XFORM_CASES[tag]
    p = f"c20.{tag}."
    m, sdg = _seeded(hip_transform(tag), p)
    args = () if q is None else (q,)
    x = seeded_input(f"c20.{tag}.x", shape, scale)
    xg = x.double().requires_grad_(True)
    ref = R.transform(sdg, xg, tag, q)
    cot = seeded_input(p + "cot", tuple(ref.shape))
    ref.backward(cot.double())
    xd = x.to(dev()).requires_grad_(True)
    out = m(xd, *args)
    close(out, ref, f"{tag} out")
    out.backward(cot.to(dev()))
    grad_close(xd.grad, xg.grad, f"{tag} dx")
    check_grads(m, p, sdg, tag)
    with torch.no_grad():
        for qq in more_q:
            close(m(x.to(dev()), qq), R.transform(sdg, x.double(), tag, qq), f"{tag} out q={qq}")
    _report(f"transform {tag}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. full width
# ---------------------------------------------------------------------------------------------------------------------------------
def test_full_width_transforms_build_and_run():
    import crdr_amd.models  # noqa: F401
    from crdr_amd.utils.registry import DECODER_REGISTRY, ENCODER_REGISTRY
    torch.manual_seed(0)
    enc = ENCODER_REGISTRY.get("Cheng20Encoder")(in_ch=3, out_ch=192, main_ch=192).to(dev())
    dec = DECODER_REGISTRY.get("Cheng20Decoder")(in_ch=192, out_ch=3, main_ch=192).to(dev())
    x = seeded_input("image", (2, 3, 64, 64)).to(dev())
    y = enc(x)
    xh = dec(y)
    assert y.shape == (2, 192, 4, 4) and xh.shape == (2, 3, 64, 64)
    assert float(xh.abs().max()) <= 1.0
    (xh - x).square().mean().backward()
    for k, p in list(enc.named_parameters()) + list(dec.named_parameters()):
        assert p.grad is not None and torch.isfinite(p.grad).all(), k


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. model, 8. scripts
# ---------------------------------------------------------------------------------------------------------------------------------
def _model():
    from crdr_amd.models import build_comp_model
    from crdr_amd.utils.options import BaseConfig, ConfigDict
    cfg, _, _ = BaseConfig._file2dict_yaml(os.path.join(ROOT, "config", "_base_", "model", "interp_ca_cheng20_hyperprior.yaml"))
    cfg["device"] = "cuda:0"
    model = build_comp_model(ConfigDict(cfg))
    seed_module(model, "")
    R.seed_gdn_(model, "")
    return model.to(dev())


def test_model_trains_reconstructs_and_codes():
    model = _model()
    x = seeded_input("image", (2, 3, 64, 64))
    ny = seeded_input("noise.y", (2, 192, 4, 4), 0.5)
    nz = seeded_input("noise.z", (2, 192, 1, 1), 0.5)
    out = model.run_model(x, rate_ind=2.0, is_train=True, noise={"y": ny.to(dev()), "z": nz.to(dev())})
    assert tuple(out["fake_images"].shape) == (2, 3, 64, 64) and tuple(out["y_hat"].shape) == (2, 192, 4, 4)
    ((out["fake_images"] - out["real_images"]).square().mean() + out["bpp"].mean()).backward()
    missing = [k for k, p in model.named_parameters() if p.requires_grad and (p.grad is None or not torch.isfinite(p.grad).all())
               and not k.endswith("quantiles")]
    assert not missing, missing
    rec = model.reconstruct(x, rate_ind=2.0)
    assert torch.equal(rec["y_hat"], out["y_hat"]) and torch.equal(rec["z_hat"], out["z_hat"])
    assert torch.equal(rec["fake_images"], out["fake_images"])
    model.eval()
    model.codec_setup()
    img = seeded_input("c20.codec", (1, 3, 72, 100))
    comp = model.compress(img, rate_ind=2.0)
    assert tuple(comp["y_hat"].shape) == (1, 192, 8, 8) and tuple(comp["z_hat"].shape) == (1, 192, 2, 2)   # padded to 128 x 128
    fake, z_hat, y_hat = model.decompress(comp["string_list"])
    assert torch.equal(y_hat, comp["y_hat"]) and torch.equal(z_hat, comp["z_hat"])
    with torch.no_grad():
        ev = model.run_model(img, is_train=False, rate_ind=2.0)
    assert tuple(fake.shape) == (1, 3, 72, 100) and torch.equal(fake, ev["fake_images"])


def test_example_config_trains_and_compresses(tmp_path):
    """config/examples/cheng20_interp_ca.yaml through scripts/train.py (hip_graphs left at its default, off), then scripts/compress.py
    --decompress on its checkpoint, in the form of test_example_1_trains_and_compresses"""
    import json
    from PIL import Image
    from tests.test_gpu_hyperprior_only import _dataset_yaml, _run
    from tests.test_gpu_scripts import _png_dir
    train_dir, eval_dir = str(tmp_path / "train" / "0"), str(tmp_path / "kodak")
    _png_dir(train_dir, 4, 80, 96, 7)
    _png_dir(eval_dir, 1, 64, 96, 8)
    os.makedirs(tmp_path / "checkpoint")
    cfg = tmp_path / "tiny_cheng20.yaml"
    cfg.write_text(f"_base_: [{os.path.relpath(os.path.join(ROOT, 'config', 'examples', 'cheng20_interp_ca.yaml'), str(tmp_path))}]\n"
                   + _dataset_yaml(tmp_path, eval_dir).replace("hip_graphs: true\n", ""))
    _run([os.path.join(ROOT, "scripts", "train.py"), str(cfg), "-d", "cuda:0", "-b", "2", "-ti", "4", "-s", "4", "-l", "2", "-e", "4", "-nw", "0"],
         cwd=str(tmp_path))
    ckpt = tmp_path / "checkpoint" / "tiny_cheng20" / "model" / "comp_model_iter4.pth.tar"
    assert os.path.exists(ckpt), os.listdir(os.path.dirname(ckpt))
    sd = torch.load(ckpt, map_location="cpu")["comp_model"]
    assert "encoder.block1.actv2.gamma" in sd and "decoder.up3.0.weight" in sd and "decoder.interp_ca_list.9.weight" in sd
    out_dir = tmp_path / "out"
    _run([os.path.join(ROOT, "scripts", "compress.py"), "--config_path", str(cfg), "--model_path", str(ckpt), "--img_dir", eval_dir,
          "--save_dir", str(out_dir), "-q", "1.5", "--decompress", "-d", "cuda:0"], cwd=ROOT)
    files = sorted(os.listdir(out_dir))
    assert "im00.bin" in files and "im00.png" in files and "_avg_bitrate.json" in files, files
    assert 0 < list(json.load(open(out_dir / "_avg_bitrate.json")).values())[0] < 24
    assert Image.open(out_dir / "im00.png").size == (96, 64)
