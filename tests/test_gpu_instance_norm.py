"""GPU parity of the InstanceNorm op (csrc/instnorm.hip through crdr_amd/models/layer/instance_norm.py) against the float64 restatement
(tests/instance_norm_ref.py, pinned to torch's own instance_norm by tests/test_multirate_disc_host.py).

Gates are the project's gates for norm ops (tests/test_gpu_hific.py): y and dx within 2e-5 of the scale of the reference tensor, parameter
gradients within 5e-5.  Every comparison prints its figure before it asserts (`-s` yields the margins, profiles/instance_norm_test_margins.txt).

Shapes (N, H, W): (2, 1, 2) is the smallest legal plane (two values per channel; its input scale is tests/instance_norm_ref.py's
TWO_VALUE_PLANE_SCALE, see the reasoning there); (3, 9, 7) is ragged inside one slab; (2, 70, 75) = 5250 pixels per image crosses the kernel's
slab size of 512 pixels (IN_SLAB, csrc/instnorm.hip): ten full slabs and a ragged one of 130, merged by Chan's formula."""
import pytest
import torch
import torch.nn.functional as F

from tests import instance_norm_ref as R
from tests.golden.seeded_weights import seeded_input
from tests.test_gpu_model import dev

pytestmark = pytest.mark.gpu

WIDTHS = [4, 8, 64, 96, 512, 1024]
ACTS = [None, "relu", "lrelu"]
SHAPES = [(2, 1, 2), (3, 9, 7), (2, 70, 75)]
SLAB = 512   # IN_SLAB of csrc/instnorm.hip
assert SHAPES[2][1] * SHAPES[2][2] > 2 * SLAB and (SHAPES[2][1] * SHAPES[2][2]) % SLAB != 0 and SHAPES[1][1] * SHAPES[1][2] < SLAB


def nhwc(t):
    return t.to(dev()).contiguous(memory_format=torch.channels_last)


def err(got, ref):
    """max |got - ref| / max |ref|"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-300)).item()


def gate(what, got, ref, tol):
    e = err(got, ref)
    print(f"{what}: {e:.3e} (gate {tol:.0e})")
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    assert e <= tol, (what, e)
    return e


def op_inputs(c, nhw=(2, 9, 7), offset=None, tag=""):
    shape = (nhw[0], c, nhw[1], nhw[2])
    key = f"{tag}{c}.{nhw}"
    x = seeded_input(f"in.x{key}", shape, R.input_scale(shape)) if offset is None else offset + 0.1 * seeded_input(f"in.off.x{key}", shape)
    weight = 1 + 0.3 * seeded_input(f"in.w{c}", (c,))
    bias = 0.2 * seeded_input(f"in.b{c}", (c,))
    cot = seeded_input(f"in.cot{key}", shape)
    return x, weight, bias, cot


def make_norm(c, weight=None, bias=None):
    from crdr_amd.models.layer.instance_norm import InstanceNorm2D
    m = InstanceNorm2D(c, affine=weight is not None)
    if weight is not None:
        with torch.no_grad():
            m.weight.copy_(weight)
            m.bias.copy_(bias)
    return m.to(dev())


def run(m, x, cot, **kw):
    """-> (y, dx) of one forward + backward of the module on the device"""
    xd = nhwc(x).requires_grad_(True)
    y = m(xd, **kw)
    y.backward(nhwc(cot))
    return y.detach(), xd.grad


# ---- 1. op parity -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("nhw", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("c", WIDTHS)
def test_instance_norm_matches_float64(c, nhw, act, affine):
    x, weight, bias, cot = op_inputs(c, nhw)
    w, b = (weight, bias) if affine else (None, None)
    m = make_norm(c, w, b)
    y, dx = run(m, x, cot, act=act, slope=0.2)
    what = f"instance_norm {c} {nhw} {act} {'affine' if affine else 'plain'}"
    y64, z64 = R.instance_norm(x, w, b, act=act, slope=0.2)
    gate(f"{what} y", y, y64, 2e-5)
    mask = None
    if act is not None:
        mask = y.cpu() > 0
        differ = mask != (z64 > 0)
        n_diff = int(differ.sum())
        print(f"{what}: {n_diff} mask elements differ from float64; smallest |z64| {z64.abs().min().item():.2e}")
        assert n_diff <= 2 and bool((z64[differ].abs() < 1e-5).all()), (n_diff, z64[differ])
    dx64, dw64, db64 = R.instance_norm_backward(x, w, b, cot, act=act, slope=0.2, mask=mask)
    gate(f"{what} dx", dx, dx64, 2e-5)
    if affine:
        gate(f"{what} dweight", m.weight.grad, dw64, 5e-5)
        gate(f"{what} dbias", m.bias.grad, db64, 5e-5)


def test_instance_norm_matches_torch_module_keys_and_eval():
    """`weight` / `bias` of shape [C] (torch's keys), no buffers; eval equals train (no running statistics)"""
    c = 8
    x, weight, bias, cot = op_inputs(c)
    m = make_norm(c, weight, bias)
    assert sorted(m.state_dict()) == sorted(torch.nn.InstanceNorm2d(c, affine=True).state_dict()) == ["bias", "weight"]
    assert make_norm(c).state_dict() == {}
    y, _ = run(m, x, cot)
    y_eval, _ = run(m.eval(), x, cot)
    assert torch.equal(y, y_eval)
    gate("instance_norm against F.instance_norm (float64)", y, F.instance_norm(x.double(), weight=weight.double(), bias=bias.double()), 2e-5)


def test_instance_norm_refuses_what_the_kernel_cannot_take():
    from crdr_amd.hip import lib as L
    from crdr_amd.models.layer import instance_norm as IN
    with pytest.raises(L.CrdrHipError):   # one value per channel
        IN.instance_norm_fwd(nhwc(torch.zeros(2, 8, 1, 1)))
    with pytest.raises(L.CrdrHipError):   # 16-byte rows: a channel count that is no multiple of 4 is refused, not rounded
        IN.instance_norm_fwd(nhwc(torch.zeros(2, 8, 3, 3))[:, :6])
    with pytest.raises(ValueError):
        IN.instance_norm_fwd(nhwc(torch.zeros(2, 8, 3, 3)), act="gelu")


# ---- 2. channel slices ----------------------------------------------------------------------------------------------------------------

def test_instance_norm_on_channel_slices_is_bit_equal_to_the_dense_call():
    from crdr_amd.models.layer import instance_norm as IN
    n, h, w = 2, 30, 30   # 900 pixels: two slabs
    wide_x = seeded_input("in.wide.x", (n, 96, h, w), 3.0)
    cot = seeded_input("in.wide.cot", (n, 64, h, w))
    _, weight, bias, _ = op_inputs(64)
    m = make_norm(64, weight, bias)
    xs = nhwc(wide_x)[:, 8:72]
    assert xs.stride(3) == 96 and xs.data_ptr() % 16 == 0
    buf = torch.full((n, h, w, 96), 777.0, device=dev())
    out = buf.permute(0, 3, 1, 2)[:, 8:72]
    y, _, _, ldx = IN.instance_norm_fwd(xs, m.weight, m.bias, eps=m.eps, act="lrelu", slope=0.2, out=out)
    assert ldx == 96 and y.data_ptr() == out.data_ptr()
    assert bool((buf[..., :8] == 777.0).all()) and bool((buf[..., 72:] == 777.0).all()), "channels outside the slice were written"
    y_dense, dx_dense = run(m, wide_x[:, 8:72], cot, act="lrelu", slope=0.2)
    gw, gb = m.weight.grad.clone(), m.bias.grad.clone()
    assert torch.equal(out, y_dense)
    m.weight.grad, m.bias.grad = None, None
    xs.requires_grad_(True)
    y2 = m(xs, act="lrelu", slope=0.2)
    wide_cot = torch.zeros(n, 96, h, w)
    wide_cot[:, 8:72] = cot
    y2.backward(nhwc(wide_cot)[:, 8:72])   # the cotangent is a slice too
    assert torch.equal(y2.detach(), y_dense) and torch.equal(xs.grad, dx_dense)
    assert torch.equal(m.weight.grad, gw) and torch.equal(m.bias.grad, gb)


# ---- 3. common offset -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [64, 512])
def test_instance_norm_with_a_common_offset(c):
    """x = 50 + 0.1 u: the variance must come from centred values.  Yardstick: 4 x the error of torch's own float32 instance_norm on the
    CPU against float64, measured here."""
    x, _, _, cot = op_inputs(c, offset=50.0)
    y64, _ = R.instance_norm(x)
    dx64, _, _ = R.instance_norm_backward(x, None, None, cot)
    x32 = x.clone().requires_grad_(True)
    y32 = F.instance_norm(x32, eps=1e-5)
    y32.backward(cot)
    ey32, edx32 = err(y32, y64), err(x32.grad, dx64)
    y, dx = run(make_norm(c), x, cot)
    ey, edx = err(y, y64), err(dx, dx64)
    print(f"common offset {c}: y device {ey:.3e} torch float32 {ey32:.3e}; dx device {edx:.3e} torch float32 {edx32:.3e}")
    assert ey <= 4 * ey32, (ey, ey32)
    assert edx <= 4 * edx32, (edx, edx32)


# ---- 4. determinism and graphs --------------------------------------------------------------------------------------------------------------

def test_instance_norm_is_bit_reproducible():
    c, nhw = 96, SHAPES[2]
    x, weight, bias, cot = op_inputs(c, nhw)
    outs = []
    for _ in range(2):
        m = make_norm(c, weight, bias)
        y, dx = run(m, x, cot, act="lrelu", slope=0.2)
        outs.append((y, dx, m.weight.grad.clone(), m.bias.grad.clone()))
    for name, a, b in zip(("y", "dx", "dweight", "dbias"), *outs):
        assert torch.equal(a, b), name


def test_instance_norm_graph_replay_equals_eager():
    c, nhw = 64, (2, 30, 30)
    shape = (nhw[0], c, nhw[1], nhw[2])
    _, weight, bias, _ = op_inputs(c)
    m = make_norm(c, weight, bias)
    cd = nhwc(seeded_input("in.graph.cot", shape))
    xs = nhwc(torch.zeros(shape)).requires_grad_(True)
    inputs = [nhwc(seeded_input(f"in.graph.x{i}", shape, 3.0)) for i in range(3)]

    def step():
        m.weight.grad.zero_()
        m.bias.grad.zero_()
        y = m(xs, act="lrelu", slope=0.2)
        dx, = torch.autograd.grad(y, xs, cd)
        return y, dx

    def eager(x):
        with torch.no_grad():
            xs.copy_(x)
        y, dx = step()
        return [t.clone() for t in (y.detach(), dx, m.weight.grad, m.bias.grad)]
    m.weight.grad, m.bias.grad = torch.zeros_like(m.weight), torch.zeros_like(m.bias)
    want = [eager(x) for x in inputs]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.no_grad():
        xs.copy_(inputs[0])
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        y, dx = step()
    for i in (1, 2):
        with torch.no_grad():
            xs.copy_(inputs[i])
        g.replay()
        torch.cuda.synchronize()
        for name, got, ref in zip(("y", "dx", "dweight", "dbias"), (y.detach(), dx, m.weight.grad, m.bias.grad), want[i]):
            assert torch.equal(got, ref), (i, name)


# ---- 5. accumulation ------------------------------------------------------------------------------------------------------------------------

def test_parameter_gradients_accumulate_into_their_slots():
    c, nhw = 64, (3, 9, 7)
    x, weight, bias, cot = op_inputs(c, nhw)
    m = make_norm(c, weight, bias)
    run(m, x, cot, act="relu")
    gw, gb = m.weight.grad.clone(), m.bias.grad.clone()
    assert float(gw.abs().max()) > 0 and float(gb.abs().max()) > 0
    pre_w, pre_b = seeded_input("in.pre.w", (c,), 5.0).to(dev()), seeded_input("in.pre.b", (c,), 5.0).to(dev())
    m.weight.grad, m.bias.grad = pre_w.clone(), pre_b.clone()
    run(m, x, cot, act="relu")
    assert torch.equal(m.weight.grad, pre_w + gw) and torch.equal(m.bias.grad, pre_b + gb)
    # only one of the two slots wanted
    m.weight.grad, m.bias.grad = None, None
    m.bias.requires_grad_(False)
    run(m, x, cot, act="relu")
    assert torch.equal(m.weight.grad, gw) and m.bias.grad is None
