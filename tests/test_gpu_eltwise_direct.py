"""Direct GPU parity of the loss, LPIPS and spectral-norm ops of csrc/eltwise.hip, each through its crdr_amd.hip.functional wrapper (or
the module that owns its buffers), against the float64 restatements of tests/eltwise_ref.py and the oracle's spectral norm /
interpolated channel-attention vectors: lrp, maxpool3s2, lpips_layer, sqdiff_sum, l1_sum, bce_diff_sum (values and gradients),
spectral_norm_weight and interp_ca_vectors; ops.dense_nhwc, which hands the kernels without a stride argument their operands.

Gates: elementwise outputs and input gradients within 2e-5 of the reference tensor's largest magnitude, parameter gradients within 5e-5
(the gates tests/test_gpu_hific.py holds GDN and ChannelNorm to); max-pool values, gradient positions on integer data and every
"exactly zero" / "bit-equal" / "unchanged" statement at tolerance 0; scalar reductions at (k + t) 2^-24 relative to the float64 sum
(`reduce_gate` derives k and t).  Every comparison prints its figure before it asserts (profiles/eltwise_direct_test_margins.txt)."""
import math

import pytest
import torch

from tests import eltwise_ref as R
from tests.golden.seeded_weights import seeded_input, seeded_tensor
from tests.test_gpu_model import close, dev, rel

pytestmark = pytest.mark.gpu

U = 2.0 ** -24   # unit roundoff of fp32


def HF():
    from crdr_amd.hip import functional
    return functional


def cl(t):
    """dense channels-last memory on the device"""
    return t.to(dev()).contiguous(memory_format=torch.channels_last)


def padded(t):
    """the library's own layout: NHWC memory, pixel stride = channels rounded up to 4, zero padding lanes"""
    from crdr_amd.models.layer.hip_layers import to_image_nhwc
    return to_image_nhwc(t.to(dev()))


def err(got, ref):
    """max |got - ref| / max |ref|"""
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-300)).item()


def gate(what, got, ref, tol):
    assert got is not None, what
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    e = err(got, ref)
    print(f"{what}: {e:.3e} (gate {tol:.0e})")
    assert e <= tol, (what, e)
    return e


def exact(what, got, ref):
    got, ref = torch.as_tensor(got).detach().cpu(), torch.as_tensor(ref).detach().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    n = int((got.double() != ref.double()).sum())
    print(f"{what}: {n} of {ref.numel()} elements differ (gate 0)")
    assert n == 0, (what, n)


# ---- ops.dense_nhwc ----------------------------------------------------------------------------------------------------------------------

def _wide_of(t, ctot, c0):
    """a ctot-wide dense NHWC device tensor that holds `t` (CPU, NCHW) in its channels [c0, c0 + C) and 77 in the others"""
    n, c, h, w = t.shape
    wide = torch.full((n, h, w, ctot), 77.0, device=dev()).permute(0, 3, 1, 2)
    wide[:, c0:c0 + c] = t.to(dev())
    return wide.detach()


def _slice_of(t, ctot, c0):
    return _wide_of(t, ctot, c0)[:, c0:c0 + t.shape[1]]


DENSE_CASES = {"slice_w5": ((2, 8, 1, 5), lambda t: _slice_of(t, 16, 4), True),
               "nchw_w1": ((1, 6, 3, 1), lambda t: t.to(dev()).contiguous(), True),
               "pixels_of_8": ((3, 4, 1, 1), lambda t: _slice_of(t, 8, 4), True),
               "one_pixel_of_16": ((1, 8, 1, 1), lambda t: _slice_of(t, 16, 4), False)}


@pytest.mark.parametrize("name", list(DENSE_CASES))
def test_dense_nhwc_is_the_input_in_dense_nhwc_memory(name):
    """ops.dense_nhwc on the shapes where x.contiguous(memory_format=torch.channels_last), which some wrappers used instead, leaves strides
    of one-entry dimensions to torch: the result equals the input, its memory read in N, H, W, C order at pixel stride C reproduces it, and
    it is a copy exactly where ops.nhwc reports a pixel stride other than C.  A single pixel has no pixel stride: it is dense as it is.
    The result itself is dense: where ops.nhwc takes it in place (C % 4 == 0; it pads any other C to four-lane pixels first) a second call
    hands it back."""
    from crdr_amd.hip import ops
    shape, put, copies = DENSE_CASES[name]
    n, c, h, w = shape
    x = put(seeded_input(f"elt.dense.{name}", shape))
    assert (ops.nhwc(x)[1] != c) == copies, name
    r = ops.dense_nhwc(x)
    exact(f"dense_nhwc {name} values", r, x)
    rows = torch.as_strided(r, (n, h, w, c), (h * w * c, w * c, c, 1), r.storage_offset())
    exact(f"dense_nhwc {name} memory in N,H,W,C order at stride C", rows, x.permute(0, 2, 3, 1))
    assert (r.data_ptr() != x.data_ptr()) == copies, name
    again = ops.dense_nhwc(r)
    exact(f"dense_nhwc {name} applied twice", again, x)
    assert c % 4 != 0 or again.data_ptr() == r.data_ptr(), name + ": a dense tensor was copied"


def test_dense_nhwc_returns_a_dense_tensor_itself():
    from crdr_amd.hip import ops
    x = cl(seeded_input("elt.dense.cl", (2, 8, 3, 5)))
    r = ops.dense_nhwc(x)
    assert r.data_ptr() == x.data_ptr() and r.stride() == x.stride()


@pytest.mark.parametrize("h,w", [(7, 7), (3, 3)])
def test_maxpool_channel_slice_equals_dense_copy(h, w):
    """Input and cotangent as channels [4, 12) of 16-wide NHWC buffers against the same call on dense clones: bit-equal forward and
    gradient.  The kernel refuses W < 3 (a W = 1 input has no window), so 3x3, the smallest size it accepts, stands for the narrow case."""
    oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    x = R.pool_input(8, h, w)
    cot = seeded_input(f"elt.pool.slice.cot{h}x{w}", (2, 8, oh, ow))
    wide = _wide_of(x, 16, 4).requires_grad_(True)
    dense = cl(x).requires_grad_(True)
    y = HF().maxpool3s2(wide[:, 4:12])
    y.backward(_slice_of(cot, 16, 4))
    y0 = HF().maxpool3s2(dense)
    y0.backward(cl(cot))
    assert torch.equal(y, y0), "forward"
    assert torch.equal(wide.grad[:, 4:12], dense.grad), "gradient"
    assert not bool(wide.grad[:, :4].any()) and not bool(wide.grad[:, 12:].any()), "gradient outside the slice"
    exact(f"maxpool slice {h}x{w} y against float64", y, R.maxpool3s2(x.double()))


@pytest.mark.parametrize("h,w", [(7, 7), (7, 1)])
def test_lpips_layer_channel_slices_equal_dense_copies(h, w):
    """both feature maps as channels [4, 12) of 16-wide NHWC buffers against the same call on dense clones: bit-equal value and gradient"""
    f0, f1, lin, g = R.lpips_inputs(2, 8, h, w)
    wide = _wide_of(f1, 16, 4).requires_grad_(True)
    dense = cl(f1).requires_grad_(True)
    lind, gd = lin.to(dev()), g.to(dev())
    v = HF().lpips_layer(_slice_of(f0, 16, 4), wide[:, 4:12], lind)
    v.backward(gd)
    v0 = HF().lpips_layer(cl(f0), dense, lind)
    v0.backward(gd)
    assert torch.equal(v, v0), "value"
    assert torch.equal(wide.grad[:, 4:12], dense.grad), "gradient"
    assert not bool(wide.grad[:, :4].any()) and not bool(wide.grad[:, 12:].any()), "gradient outside the slice"
    gate(f"lpips slice {h}x{w} value against float64", v, R.lpips_layer(f0.double(), f1.double(), lin.double()), 2e-5)


# ---- lrp ---------------------------------------------------------------------------------------------------------------------------------

def _lrp_operands(kind, shape):
    """-> (a, z, leaves, read): device operands, the leaves that collect gradients and how to read (da, dz) off them"""
    n, c, h, w = shape
    a = seeded_input(f"elt.lrp.a.{kind}{c}.{h}", shape, 2.0)
    z = seeded_input(f"elt.lrp.z.{kind}{c}.{h}", shape, 20.0)   # |z| up to 20: tanh saturates
    z[0, 0, 0, :3] = torch.tensor([20.0, -20.0, 0.0])
    if kind == "slices":
        wide = torch.zeros(n, 3 * c, h, w)
        wide[:, :c], wide[:, c:2 * c], wide[:, 2 * c:] = a, z, 77.0
        wide = cl(wide).requires_grad_(True)
        return a, z, wide[:, :c], wide[:, c:2 * c], lambda: (wide.grad[:, :c], wide.grad[:, c:2 * c], wide.grad[:, 2 * c:])
    put = {"cl": cl, "nchw": lambda t: t.to(dev()).contiguous(), "padded": padded}[kind]
    ad, zd = put(a).requires_grad_(True), put(z).requires_grad_(True)
    return a, z, ad, zd, lambda: (ad.grad, zd.grad, None)


@pytest.mark.parametrize("kind,shape", [("cl", (2, 32, 5, 3)), ("nchw", (2, 6, 5, 3)), ("padded", (2, 3, 5, 3)), ("slices", (2, 8, 5, 3)),
                                        ("cl", (2, 1, 5, 3)), ("cl", (2, 8, 384, 384))])
def test_lrp_matches_float64(kind, shape):
    """(2, 8, 384, 384) is 2359296 elements > 8192 blocks x 256: the grid-stride loop runs a second, partial pass"""
    a, z, ad, zd, grads = _lrp_operands(kind, shape)
    cot = seeded_input(f"elt.lrp.cot{shape[1]}.{shape[2]}", shape)
    what = f"lrp {kind} C={shape[1]} {shape[2]}x{shape[3]}"
    y = HF().lrp(ad, zd)
    cd = cot.to(dev())
    y.backward(cd)
    a64, z64 = a.double().requires_grad_(True), z.double().requires_grad_(True)
    y64 = R.lrp(a64, z64)
    y64.backward(cot.double())
    close(y, y64, what + " forward", 2e-5)
    gate(what + " y", y, y64, 2e-5)
    da, dz, rest = grads()
    exact(what + " da is dy", da, cot)
    gate(what + " dz", dz, z64.grad, 2e-5)
    if rest is not None:
        exact(what + " gradient of the channels outside both slices", rest, torch.zeros(rest.shape))


# ---- maxpool3s2 --------------------------------------------------------------------------------------------------------------------------

def _pool_run(x, cot, put):
    xd = put(x).requires_grad_(True)
    y = HF().maxpool3s2(xd)
    y.backward(cot.to(dev()))
    x64 = x.double().requires_grad_(True)
    y64 = R.maxpool3s2(x64)
    y64.backward(cot.double())
    return y, xd.grad, y64.detach(), x64.grad


@pytest.mark.parametrize("c", R.POOL_CHANNELS)
@pytest.mark.parametrize("h,w", R.POOL_SIZES)
def test_maxpool_matches_float64(h, w, c):
    oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    what = f"maxpool {h}x{w} C={c}"
    x = R.pool_input(c, h, w)
    cot = seeded_input(f"elt.pool.cot{c}.{h}x{w}", (2, c, oh, ow))
    y, dx, y64, dx64 = _pool_run(x, cot, cl)
    exact(what + " y", y, y64)
    gate(what + " dx", dx, dx64, 2e-5)   # up to four fp32 additions per pixel
    exact(what + " dx support", dx != 0, dx64 != 0)
    if h % 2 == 0:   # the last row and column of an even size sit in no window
        exact(what + " dx of the last row", dx[:, :, -1], torch.zeros(2, c, w))
    if w % 2 == 0:
        exact(what + " dx of the last column", dx[:, :, :, -1], torch.zeros(2, c, h))
    # ties: values in {0, 1, 2} and integer cotangents, so the position and the value of every gradient element are exact
    xt = R.tie_input(c, h, w)
    cot_t = R.int_cotangent(f"elt.pool.tiecot{c}.{h}x{w}", (2, c, oh, ow))
    print(f"{what} ties: {R.window_ties(xt):.2f} of the windows hold their maximum more than once")
    for name, put in (("channels-last", cl), ("NCHW", lambda t: t.to(dev()).contiguous())):
        y, dx, y64, dx64 = _pool_run(xt, cot_t, put)
        exact(f"{what} ties {name} y", y, y64)
        exact(f"{what} ties {name} dx", dx, dx64)


@pytest.mark.parametrize("c", [6, 64])
def test_maxpool_overlapping_windows_sum(c):
    """5x5 input, 2x2 windows: pixel (2,2) lies in all four, pixel (2,1) in the two of the first window column"""
    x = torch.zeros(2, c, 5, 5)
    x[0, :, 2, 2] = 5.0
    x[1, :, 2, 1] = 5.0
    cot = R.int_cotangent(f"elt.pool.overlap{c}", (2, c, 2, 2))
    y, dx, y64, dx64 = _pool_run(x, cot, cl)
    exact(f"maxpool overlap C={c} y", y, y64)
    exact(f"maxpool overlap C={c} dx", dx, dx64)
    exact(f"maxpool overlap C={c} argmax of four windows", dx[0, :, 2, 2], cot[0].sum((1, 2)))
    exact(f"maxpool overlap C={c} argmax of two windows", dx[1, :, 2, 1], cot[1, :, :, 0].sum(1))


# ---- lpips_layer -------------------------------------------------------------------------------------------------------------------------

def _lpips_run(f0, f1, lin, g, put=cl):
    f0d, f1d = put(f0).requires_grad_(True), put(f1).requires_grad_(True)
    lind = lin.to(dev()).requires_grad_(True)
    v = HF().lpips_layer(f0d, f1d, lind)
    v.backward(g.to(dev()))
    return v, f0d, f1d, lind


@pytest.mark.parametrize("shape", R.LPIPS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_lpips_layer_matches_float64(shape):
    f0, f1, lin, g = R.lpips_inputs(*shape)
    what = "lpips " + "x".join(map(str, shape))
    v, f0d, f1d, lind = _lpips_run(f0, f1, lin, g)
    f64 = f1.double().requires_grad_(True)
    v64 = R.lpips_layer(f0.double(), f64, lin.double())
    v64.backward(g.double())
    gate(what + " value", v, v64, 2e-5)
    gate(what + " df1", f1d.grad, f64.grad, 2e-5)
    assert f0d.grad is None and lind.grad is None, what + ": a gradient reached f0 or lin"


def test_lpips_layer_nchw_operands():
    shape = (3, 6, 15, 15)
    f0, f1, lin, g = R.lpips_inputs(*shape)
    v, _, f1d, _ = _lpips_run(f0, f1, lin, g, put=lambda t: t.to(dev()).contiguous())
    f64 = f1.double().requires_grad_(True)
    v64 = R.lpips_layer(f0.double(), f64, lin.double())
    v64.backward(g.double())
    gate("lpips NCHW 3x6x15x15 value", v, v64, 2e-5)
    gate("lpips NCHW 3x6x15x15 df1", f1d.grad, f64.grad, 2e-5)


def test_lpips_layer_all_zero_f0_pixel():
    for shape in ((3, 64, 3, 3), (1, 6, 1, 3)):
        f0, f1, lin, g = R.lpips_inputs(*shape)
        f0[0, :, 0, 1] = 0
        what = "lpips zero f0 pixel " + "x".join(map(str, shape))
        v, _, f1d, _ = _lpips_run(f0, f1, lin, g)
        f64 = f1.double().requires_grad_(True)
        v64 = R.lpips_layer(f0.double(), f64, lin.double())
        v64.backward(g.double())
        assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(f1d.grad).all()), what
        gate(what + " value", v, v64, 2e-5)
        gate(what + " df1", f1d.grad, f64.grad, 2e-5)


def test_lpips_layer_all_zero_f1_pixel_stays_finite():
    """No parity here: the reference's gradient at an all-zero f1 pixel is NaN (d sqrt(s) / ds is infinite at s = 0 and meets a zero factor,
    tests/test_eltwise_ref_host.py checks that), so there is nothing to compare with.  The kernel must not produce a NaN or an infinity:
    a NaN in one pixel's gradient would reach every weight of the generator."""
    f0, f1, lin, g = R.lpips_inputs(3, 64, 3, 3)
    f1[1, :, 2, 0] = 0
    v, _, f1d, _ = _lpips_run(f0, f1, lin, g)
    fin_v, fin_g = bool(torch.isfinite(v).all()), bool(torch.isfinite(f1d.grad).all())
    print(f"lpips zero f1 pixel: value finite {fin_v}, gradient finite {fin_g}, largest |df1| {f1d.grad.abs().max().item():.3e}")
    assert fin_v and fin_g


# ---- scalar reductions -------------------------------------------------------------------------------------------------------------------

def reduce_chain(n):
    """k, the longest chain of fp32 additions between a term and the result, from the structure of reduce_kernel / reduce_final:
    min(max(ceil(n / 1024), 1), 1024) blocks of 256 threads; a thread adds its ceil(n / (256 blocks)) terms one after the other, the 64
    lanes of a wave combine in a tree of 6 steps, the 4 wave sums in 3 additions; the final block does the same with the block sums
    (ceil(blocks / 256) serial additions per thread, 6, 3)."""
    nb = min(max(-(-n // 1024), 1), 1024)
    return -(-n // (256 * nb)) + 6 + 3 + -(-nb // 256) + 6 + 3


def reduce_gate(what, got, ref64, n, t):
    """Every term is non-negative, so each addition of the chain costs at most 2^-24 of the running sum, and a term that reaches the chain
    with a relative error of t 2^-24 keeps it: |got - ref| <= (k + t) 2^-24 ref to first order in 2^-24."""
    k = reduce_chain(n)
    tol = (k + t) * U
    got, ref = got.detach().cpu().double().reshape(()), ref64.detach().double().reshape(())
    e = ((got - ref).abs() / ref).item() if ref.item() != 0 else (got - ref).abs().item()
    print(f"{what}: {e:.3e} (gate (k={k} + t={t:.2f}) 2^-24 = {tol:.3e})")
    assert e <= tol, (what, e, tol)


def bce_term_roundings(x64, target):
    """t for the BCE sum, in units of 2^-24 of the float64 sum.  The kernel forms x = p - q (one rounding, which moves the term by
    |x| |sigmoid(x) - t|), x t (one rounding, of size |x| t; the fp32 value of t is another |x| t; both vanish for t = 0 and t = 1, which
    are exact), max(x, 0) - x t (one rounding of that difference), expf and log1pf (each within 1 ulp = 2 x 2^-24 of log(1 + e^-|x|), the second argument error not amplified) and adds the
    two parts (one rounding of the term).  Summed over the data and divided by the float64 sum."""
    x = x64
    f = R.bce_terms(x, target)
    soft = torch.log1p(torch.exp(-x.abs()))
    prod = 0.0 if target in (0.0, 1.0) else 2 * target
    bound = x.abs() * (torch.sigmoid(x) - target).abs() + prod * x.abs() + (x.clamp(min=0) - x * target).abs() + 4 * soft + f
    return (bound.sum() / f.sum()).item()


def _reduce_case(name, n):
    """-> (hip op, float64 op, operands, t).  sqdiff: d = a - b carries one rounding, doubled by the square, plus the rounding of d d: t = 3.
    l1: the rounding of a - b: t = 1."""
    if name == "sqdiff":
        return HF().sqdiff_sum, R.sqdiff_sum, R.reduce_pair(n), 3.0
    if name == "l1":
        return HF().l1_sum, R.l1_sum, R.reduce_pair(n), 1.0
    target = float(name[3:])
    p, q = R.bce_pair(n)
    hip = lambda a, b: HF().bce_diff_sum(a, b, target)   # noqa: E731
    return hip, (lambda a, b: R.bce_diff_sum(a, b, target)), (p, q), bce_term_roundings(p.double() - q.double(), target)


@pytest.mark.parametrize("shape4", [False, True], ids=["flat", "n111"])
@pytest.mark.parametrize("n", R.REDUCE_SIZES)
@pytest.mark.parametrize("name", ["sqdiff", "l1"] + [f"bce{t}" for t in R.BCE_TARGETS])
def test_reduction_matches_float64(name, n, shape4):
    """n = 2^20 + 3 is past the 1024-block cap: every thread runs its loop a fifth time for the last three elements"""
    hip, ref, (a, b), t = _reduce_case(name, n)
    shape = (n, 1, 1, 1) if shape4 else (n,)
    a, b = a.reshape(shape), b.reshape(shape)
    what = f"{name} n={n} {'[n,1,1,1]' if shape4 else 'flat'}"
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    v64 = ref(a64, b64)
    (v64 * 0.37).backward()
    ga64, gb64 = a64.grad, b64.grad
    # gradient to neither operand, and two calls on the same inputs
    ad, bd = a.to(dev()), b.to(dev())
    v0 = hip(ad, bd)
    assert not v0.requires_grad
    reduce_gate(what + " value", v0, v64, n, t)
    exact(what + " second call", hip(ad, bd), v0)
    for wa, wb in ((True, False), (False, True), (True, True)):
        ad, bd = a.to(dev()).requires_grad_(wa), b.to(dev()).requires_grad_(wb)
        v = hip(ad, bd)
        exact(f"{what} value with gradients to ({wa}, {wb})", v, v0)
        (v * 0.37).backward()   # an upstream gradient other than 1
        for g, g64, want, side in ((ad.grad, ga64, wa, "da"), (bd.grad, gb64, wb, "db")):
            if not want:
                assert g is None, (what, side)
                continue
            gate(f"{what} {side} ({wa}, {wb})", g, g64, 2e-5)
            if name in ("sqdiff", "l1"):   # a == b exactly in one element of eight: the gradient there is exactly 0
                exact(f"{what} {side} where a == b", g.reshape(-1)[::8], torch.zeros((n + 7) // 8))
            if name == "l1":   # sign(a - b) g elsewhere: one value, with either sign
                mags = g.reshape(-1).abs().cpu()
                nz = mags[mags != 0]
                exact(f"{what} {side} magnitudes", nz, torch.full_like(nz, float(torch.tensor(0.37))))


@pytest.mark.parametrize("grad_to", [0, 1])
@pytest.mark.parametrize("name", ["sqdiff", "l1", "bce0.9"])
def test_reduction_allocates_only_the_gradient_that_is_needed(name, grad_to):
    """requires_grad on one operand of n = 4096: the other side's gradient is None and no buffer is made for it -- the backward leaves
    exactly one 16 KiB gradient behind, and at its peak holds less than two (the gradient, the one-element upstream gradient)"""
    n = 4096
    hip, _, (a, b), _ = _reduce_case(name, n)
    opsd = [a.to(dev()), b.to(dev())]
    opsd[grad_to].requires_grad_(True)
    v = hip(*opsd)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    m0 = torch.cuda.memory_allocated()
    v.backward()
    torch.cuda.synchronize()
    kept, peak = torch.cuda.memory_allocated() - m0, torch.cuda.max_memory_allocated() - m0
    print(f"{name} n={n} grad to {'ab'[grad_to]}: backward keeps {kept} bytes, peak {peak} (one gradient: {4 * n})")
    assert opsd[grad_to].grad is not None and opsd[1 - grad_to].grad is None
    assert kept == 4 * n and peak < 8 * n, (kept, peak)


# ---- layouts of the loss operands -------------------------------------------------------------------------------------------------------

LAYOUTS = ["nchw", "channels_last", "padded", "slice0", "slice_off"]


def _in_layout(t, kind):
    """`t` (CPU, NCHW) on the device in one of the five layouts; a slice is cut from a 16-channel NHWC buffer whose other channels hold
    large values (offset 4 for C = 4, 5 -- not 16-byte aligned -- for C = 3)"""
    c = t.shape[1]
    if kind == "nchw":
        return t.to(dev()).contiguous()
    if kind == "channels_last":
        return cl(t)
    if kind == "padded":
        return padded(t)
    off = 0 if kind == "slice0" else (4 if c % 4 == 0 else 5)
    wide = 100 + seeded_input(f"elt.layout.wide.{kind}{c}", (t.shape[0], 16, t.shape[2], t.shape[3]), 50.0)
    wide[:, off:off + c] = t
    return cl(wide)[:, off:off + c]


@pytest.mark.parametrize("grad_to", [0, 1])
@pytest.mark.parametrize("lb", LAYOUTS)
@pytest.mark.parametrize("la", LAYOUTS)
@pytest.mark.parametrize("c", [4, 3])
@pytest.mark.parametrize("name", ["sqdiff", "l1"])
def test_loss_layout_pairings(name, c, la, lb, grad_to):
    """sqdiff_sum / l1_sum take two operands of one shape in any two of the five layouts: the value and the gradient equal the float64
    reference.  (The wrappers may refuse a pairing with CrdrHipError before any launch; they refuse none of these, and a refusal here
    fails the case like a wrong number or any other exception, so that a wrapper which refuses everything cannot pass.)"""
    hip, ref = (HF().sqdiff_sum, R.sqdiff_sum) if name == "sqdiff" else (HF().l1_sum, R.l1_sum)
    a, b = R.layout_pair(c)
    what = f"{name} C={c} {la} / {lb} grad to {'ab'[grad_to]}"
    ops64 = [a.double(), b.double()]
    ops64[grad_to].requires_grad_(True)
    v64 = ref(*ops64)
    (v64 * 0.37).backward()
    opsd = [_in_layout(a, la), _in_layout(b, lb)]
    opsd[grad_to].requires_grad_(True)
    v = hip(*opsd)
    (v * 0.37).backward()
    n = a.numel() // c * ((c + 3) // 4 * 4)   # what the kernel sums over when the operands keep their padding lanes
    reduce_gate(what + " value", v, v64, n, 3.0 if name == "sqdiff" else 1.0)
    gate(what + " gradient", opsd[grad_to].grad, ops64[grad_to].grad, 2e-5)
    assert opsd[1 - grad_to].grad is None


@pytest.mark.parametrize("name", ["sqdiff", "l1"])
def test_loss_three_of_four_channel_views_keep_the_stated_contract(name):
    """A [:, 0:3] view of a tensor that is exactly 4 channels wide has the library's own strides and is summed in place, 4th lane included
    (DESIGN 3): the caller keeps that lane equal in both operands.  Pinned here: with equal, non-zero 4th lanes the value and the gradient
    equal the float64 reference of the three channels, and the 4th lane of the owning tensor receives exactly 0."""
    hip, ref = (HF().sqdiff_sum, R.sqdiff_sum) if name == "sqdiff" else (HF().l1_sum, R.l1_sum)
    a, b = R.layout_pair(3)
    lane = 7 + seeded_input("elt.layout.lane4", (2, 1, 5, 3))
    wa, wb = cl(torch.cat((a, lane), 1)).requires_grad_(True), cl(torch.cat((b, lane), 1))
    a64 = a.double().requires_grad_(True)
    v64 = ref(a64, b.double())
    (v64 * 0.37).backward()
    v = hip(wa[:, :3], wb[:, :3])
    (v * 0.37).backward()
    reduce_gate(f"{name} 3-of-4 views value", v, v64, 2 * 5 * 3 * 4, 3.0 if name == "sqdiff" else 1.0)
    gate(f"{name} 3-of-4 views gradient", wa.grad[:, :3], a64.grad, 2e-5)
    exact(f"{name} 3-of-4 views gradient of the 4th lane", wa.grad[:, 3:], torch.zeros(2, 1, 5, 3))


# ---- spectral norm -----------------------------------------------------------------------------------------------------------------------

SN_SHAPES = [(1, 7), (5, 3), (64, 48), (130, 1030)]   # O < 4, O % 4 != 0, K < 64; K > 1024: the one-block normalise strides


def _sn_state(o, k):
    w = seeded_tensor(f"elt.sn.w{o}x{k}", (o, k, 1, 1)) * 0.3
    u = torch.nn.functional.normalize(seeded_input(f"elt.sn.u{o}", (o,)), dim=0)
    v = torch.nn.functional.normalize(seeded_input(f"elt.sn.v{k}", (k,)), dim=0)
    cot = seeded_input(f"elt.sn.cot{o}x{k}", (o, k, 1, 1))
    return w, u, v, cot


class _Sn:
    """the device side: a parameter, the u / v buffers and the persistent output buffer, as HipSpectralNormConv2d owns them"""

    def __init__(self, w, u, v):
        self.w = torch.nn.Parameter(w.to(dev()))
        self.u, self.v = u.to(dev()).clone(), v.to(dev()).clone()
        self.out = torch.zeros_like(self.w)

    def __call__(self, training):
        """-> (live output: an alias of the persistent buffer, a copy of its values, the sigma the output was divided by: w / (w / sigma)
        at the largest |w|, two fp32 roundings away from the kernel's own)"""
        y = HF().spectral_norm_weight(self.w, self.u, self.v, training, self.out)
        w64, y64 = self.w.detach().cpu().double().reshape(-1), y.detach().cpu().double().reshape(-1)
        i = int(w64.abs().argmax())
        return y, y.detach().clone(), w64[i] / y64[i]


@pytest.mark.parametrize("o,k", SN_SHAPES)
def test_spectral_norm_forward_matches_float64(o, k):
    w, u, v, _ = _sn_state(o, k)
    m = _Sn(w, u, v)
    w64, u64, v64 = w.double(), u.double(), v.double()
    for it in (1, 2):   # the second training call continues from the first one's u, v: two reference iterations
        _, y, sigma = m(True)
        y64, s64, u64, v64 = R.spectral_norm(w64, u64, v64, True)
        what = f"spectral norm {o}x{k} training call {it}"
        gate(what + " w / sigma", y, y64, 2e-5)
        gate(what + " sigma", sigma.reshape(()), s64, 2e-5)
        gate(what + " u", m.u, u64, 2e-5)
        gate(what + " v", m.v, v64, 2e-5)
    u_before, v_before = m.u.clone(), m.v.clone()
    _, y, sigma = m(False)
    y64, s64, _, _ = R.spectral_norm(w64, u64, v64, False)
    gate(f"spectral norm {o}x{k} eval w / sigma", y, y64, 2e-5)
    gate(f"spectral norm {o}x{k} eval sigma", sigma.reshape(()), s64, 2e-5)
    exact(f"spectral norm {o}x{k} eval u", m.u, u_before)
    exact(f"spectral norm {o}x{k} eval v", m.v, v_before)


def test_spectral_norm_through_the_module():
    """HipSpectralNormConv2d hands its own buffers to the same op: 3 -> 64 channels, 4x4 taps is the 64 x 48 matrix"""
    from crdr_amd.models.layer.hip_layers import HipSpectralNormConv2d
    w, u, v, _ = _sn_state(64, 48)
    m = HipSpectralNormConv2d(3, 64, 4, stride=2, padding=2)
    with torch.no_grad():
        m.weight_orig.copy_(w.reshape(64, 3, 4, 4))
        m.weight_u.copy_(u)
        m.weight_v.copy_(v)
    m.to(dev()).train()
    m(padded(seeded_input("elt.sn.image", (1, 3, 8, 8))))
    y64, _, u64, v64 = R.spectral_norm(w.double(), u.double(), v.double(), True)
    gate("spectral norm module w / sigma", m._w_sn.reshape(64, 48, 1, 1), y64, 2e-5)
    gate("spectral norm module u", m.weight_u, u64, 2e-5)
    gate("spectral norm module v", m.weight_v, v64, 2e-5)


def _sn_ref_grad(w, u, v, cot):
    """-> (d/dw of sum(cot w / sigma) after one training iteration from (u, v), u', v')"""
    w64 = w.double().requires_grad_(True)
    y64, _, u2, v2 = R.spectral_norm(w64, u.double(), v.double(), True)
    (y64 * cot.double()).sum().backward()
    return w64.grad, u2, v2


@pytest.mark.parametrize("o,k", SN_SHAPES)
def test_spectral_norm_backward_matches_float64(o, k):
    w, u, v, cot = _sn_state(o, k)
    g64, u2, v2 = _sn_ref_grad(w, u, v, cot)
    what = f"spectral norm {o}x{k}"
    m = _Sn(w, u, v)
    y, _, _ = m(True)
    loss = (y * cot.to(dev())).sum()
    loss.backward(retain_graph=True)
    gate(what + " weight_orig.grad", m.w.grad, g64, 5e-5)
    once = m.w.grad.clone()
    loss.backward()
    exact(what + " weight_orig.grad after a second backward is twice the first", m.w.grad, 2 * once)
    # forward A, forward B, backward A: the gradient belongs to A's u, v, sigma although B has moved the buffers on
    m = _Sn(w, u, v)
    ya, _, _ = m(True)
    loss_a = (ya * cot.to(dev())).sum()
    m(True)
    gate(what + " u after forward B (two iterations)", m.u, R.spectral_norm(w.double(), u2, v2, True)[2], 2e-5)
    loss_a.backward()
    gate(what + " weight_orig.grad of A after forward B", m.w.grad, g64, 5e-5)
    exact(what + " weight_orig.grad of A after forward B, against A alone", m.w.grad, once)


# ---- interpolated channel-attention vectors ----------------------------------------------------------------------------------------------

QS = [0.0, 0.25, 2.0, 3.5, 4.0]   # 4 = L - 1: the l == r branch


def _ca_module(ch, use_bias):
    from crdr_amd.models.layer.interp_channel_attention import InterpChAtt
    m = InterpChAtt(ch, rate_level=5, actv="softplus", use_interp=True, use_bias=use_bias)
    W = seeded_tensor(f"elt.ica.w{ch}", (5, 1, ch, 1, 1)) * 2
    W[4] = 21 + 4 * seeded_input(f"elt.ica.hi{ch}", (1, ch, 1, 1)).abs()   # above 20: softplus is the identity
    W[0] = -20 + 0.5 * seeded_input(f"elt.ica.lo{ch}", (1, ch, 1, 1))      # near -20: softplus ~ e^w
    B = seeded_tensor(f"elt.ica.b{ch}", (5, 1, ch, 1, 1))
    with torch.no_grad():
        m.weight.copy_(W)
        if use_bias:
            m.bias.copy_(B)
    return m.to(dev()), W, (B if use_bias else torch.zeros_like(B))


@pytest.mark.parametrize("use_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("ch", [1, 63, 64, 65, 192])
def test_interp_ca_vectors_match_float64(ch, use_bias):
    from oracle import crdr_oracle as O
    m, W, B = _ca_module(ch, use_bias)
    cs, ct = seeded_input(f"elt.ica.cs{ch}", (ch,)), seeded_input(f"elt.ica.ct{ch}", (ch,))
    for q in QS:
        what = f"interp_ca ch={ch} {'bias' if use_bias else 'no bias'} q={q}"
        l = math.floor(q)
        r = min(l + 1, 4)
        others = [i for i in range(5) if i not in (l, r)]
        W64, B64 = W.double().requires_grad_(True), B.double().requires_grad_(True)
        s64, t64 = O.interp_ca_vectors(W64, B64, q)
        ((s64.reshape(-1) * cs.double()).sum() + (t64.reshape(-1) * ct.double()).sum()).backward()

        def run(weight, bias):
            s, t = HF().interp_ca_vectors(weight, bias, q)
            ((s * cs.to(dev())).sum() + (t * ct.to(dev())).sum()).backward()
            return s, t
        m.weight.grad = None
        if use_bias:
            m.bias.grad = None
        s, t = m.vectors(q)
        ((s * cs.to(dev())).sum() + (t * ct.to(dev())).sum()).backward()
        gate(what + " scale", s, s64.reshape(-1), 2e-5)
        if use_bias:
            gate(what + " shift", t, t64.reshape(-1), 2e-5)
        else:
            exact(what + " shift", t, torch.zeros(ch))
        gate(what + " weight.grad", m.weight.grad, W64.grad, 5e-5)
        exact(what + " weight.grad rows other than l, r", m.weight.grad[others], torch.zeros(len(others), 1, ch, 1, 1))
        if use_bias:
            gate(what + " bias.grad", m.bias.grad, B64.grad, 5e-5)
            exact(what + " bias.grad rows other than l, r", m.bias.grad[others], torch.zeros(len(others), 1, ch, 1, 1))
        once_w = m.weight.grad.clone()
        once_b = m.bias.grad.clone() if use_bias else None
        # a second backward accumulates into .grad
        run(m.weight, m.bias)
        exact(what + " weight.grad after a second backward is twice the first", m.weight.grad, 2 * once_w)
        if use_bias:
            exact(what + " bias.grad after a second backward is twice the first", m.bias.grad, 2 * once_b)
        # the non-leaf path returns the same gradient through autograd
        m.weight.grad = None
        if use_bias:
            m.bias.grad = None
        run(m.weight * 1.0, m.bias * 1.0 if use_bias else None)
        exact(what + " weight.grad through a non-leaf weight", m.weight.grad, once_w)
        if use_bias:
            exact(what + " bias.grad through a non-leaf bias", m.bias.grad, once_b)
    print(f"interp_ca ch={ch}: relative L2 of the last weight.grad {rel(m.weight.grad, W64.grad):.3e}")
