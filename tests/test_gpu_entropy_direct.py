"""Direct GPU parity of the entropy-model kernels of csrc/entropy.hip against the float64 restatements of tests/entropy_ref.py:
gauss_cond through crdr_amd.hip.functional.gauss_cond (values, both bit sums, dy / dmu / dsigma with and without a y_hat cotangent, every
layout, both dispatches, one block per image to the grid-stride second passes) and through the raw ABI (every stride of crdr_gc_desc2,
untouched memory, bit-sum accumulation, the no-workspace path), the in-kernel Philox noise against its numpy restatement, a NaN latent,
the factorised prior through SteEntropyBottleneck (every named parameter gradient), eb_aux_loss and crdr_gauss_symbols.

Gates (none taken from the code under test): likelihoods at the bounds tests/test_gpu_model.py::test_gauss_cond_likelihood_against_float64
holds the vector path to (3e-6 relative + 3e-7 absolute above 1e-5, 3e-7 absolute below, the floor exact); EB likelihoods 2e-5 of the
tensor's largest magnitude; input gradients max(2e-5, 4 s), parameter gradients and dquantiles max(5e-5, 4 s) of the reference tensor's
largest magnitude, s the error of the same restatement evaluated in fp32 on the same operands (computed here, printed); gauss_cond bit
sums 1e-5, EB bits and the aux loss 2e-5 of the float64 sum; everything worded exactly / bit-equal / unchanged at tolerance 0.  The inputs
are built so that the float64 reference alone decides every discrete choice (tests/test_entropy_ref_host.py): no comparison leaves an
element out.  Every comparison prints its figure before it asserts (profiles/entropy_direct_test_margins.txt)."""
import ctypes as C
import functools

import pytest
import torch

from tests import entropy_ref as R
from tests.test_gpu_eltwise_direct import HF, cl, err, exact, gate, padded
from tests.test_gpu_model import dev

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32


def hip():
    from crdr_amd.hip import lib as L
    from crdr_amd.hip import ops
    return L, L.load(), ops


# ---- gates -----------------------------------------------------------------------------------------------------------------------------

def lik_gate(what, got, ref):
    """Gaussian likelihoods: |got - ref| <= 3e-6 ref + 3e-7 above 1e-5, 3e-7 below; at the floor exactly where the reference is"""
    got, ref = got.detach().cpu().double(), ref.detach().double()
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    bound = torch.where(ref > 1e-5, 3e-6 * ref + 3e-7, torch.full_like(ref, 3e-7))
    ratio = ((got - ref).abs() / bound).max().item()
    off = int(((got == R.LIK_BOUND) != (ref == R.LIK_BOUND)).sum())
    print(f"{what}: {ratio:.3f} of its bound at worst, {off} of {int((ref == R.LIK_BOUND).sum())} floor elements differ (gate 1, 0)")
    assert ratio <= 1 and off == 0 and bool((got >= R.LIK_BOUND).all()), (what, ratio, off)


def sum_gate(what, got, ref, tol):
    """per-image sums: max |got - ref| / |ref|"""
    got, ref = torch.as_tensor(got).detach().cpu().double().reshape(-1), torch.as_tensor(ref).detach().double().reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    e = ((got - ref).abs() / ref.abs()).max().item()
    print(f"{what}: {e:.3e} (gate {tol:.0e})")
    assert e <= tol, (what, e)


def grad_gate(what, got, r64, r32, floor):
    s = err(r32, r64)
    print(f"{what}: fp32 restatement s = {s:.3e}")
    return gate(what, got, r64, max(floor, 4 * s))


# ---- gauss_cond through HF.gauss_cond ------------------------------------------------------------------------------------------------------

def put(kind, t):
    """the [N, C, H, W] CPU tensor on the device in layout `kind` (tests/entropy_ref.py GC_KINDS)"""
    from crdr_amd.hip import ops
    if kind == "cl":
        return cl(t)
    if kind == "nchw":
        return t.to(dev()).contiguous()
    if kind == "padded":
        return padded(t)
    n, c, h, w = t.shape
    off = {"slice4": 4, "slice3": 3}[kind]
    wide = torch.full((n, h, w, ops.ld_for(c) + 8), 77.0, device=dev()).permute(0, 3, 1, 2)
    wide[:, off:off + c] = t.to(dev())
    return wide[:, off:off + c]


def gc_reference(d):
    """-> {"r64", "r32"}: the restatement in float64 and in fp32 on the case's operands: y_hat, both likelihoods and bit sums, the gradients
    of sum_n gbits[n] bits_noisy[n] (+ sum y_hat gyh) without and with the y_hat cotangent; "under": float64 noisy likelihood under the
    floor; "sblocked": where the scale LowerBound's rule blocks dsigma"""
    out = {}
    for name, dt in (("r64", F64), ("r32", F32)):
        y, mu, sg = (d[k].to(dt).clone().requires_grad_(True) for k in ("y", "mu", "sigma"))
        nz, gb, gyh = d["noise"].to(dt), d["gbits"].to(dt), d["gyh"].to(dt)
        yh, lik = R.gaussian_conditional(y, mu, sg, nz)
        bits = R.bits_per_image(lik)
        g0 = torch.autograd.grad((bits * gb).sum(), (y, mu, sg), retain_graph=True)
        g1 = torch.autograd.grad((bits * gb).sum() + (yh * gyh).sum(), (y, mu, sg))
        with torch.no_grad():
            _, qlik = R.gaussian_conditional(y, mu, sg, None)
            out[name] = {"yh": yh.detach(), "lik": lik.detach(), "qlik": qlik, "bits": bits.detach(), "qbits": R.bits_per_image(qlik),
                         False: g0, True: g1}
    out["under"] = R.gc_raw_likelihoods(d)[0] < R.LIK_BOUND
    out["sblocked"] = (d["sigma"].double() < R.SCALE_BOUND) & (R.gc_scale_grad(d) >= 0)
    return out


@functools.lru_cache(maxsize=None)
def gc_shared(size, c):
    d = R.gc_case(f"gcd.{size}.{c}", *R.gc_shape(size, c))
    return d, gc_reference(d)


def run_gc(kind, d, cot, noise=True):
    leaves = [put(kind, d[k]).detach().requires_grad_(True) for k in ("y", "mu", "sigma")]
    out = HF().gauss_cond(*leaves, put(kind, d["noise"]) if noise else None, 0.11, 1e-9, True)
    if noise:
        loss = (out[1] * d["gbits"].to(dev())).sum()
        if cot:
            loss = loss + (out[0] * d["gyh"].to(dev())).sum()
        loss.backward()
    return out, [t.grad for t in leaves]


def padding_lane(what, t):
    """a C = 3 output of the library lives in four-lane pixels whose fourth lane stays 0"""
    n, c, h, w = t.shape
    assert c == 3 and t.stride() == (h * w * 4, 1, w * 4, 4), (what, t.stride())
    lane = torch.as_strided(t.detach(), (n, h, w), (h * w * 4, w * 4, 4), t.storage_offset() + 3)
    exact(what + " padding lane", lane, torch.zeros(n, h, w))


def check_gc(what, kind, d, ref):
    r64, r32 = ref["r64"], ref["r32"]
    c = d["y"].shape[1]
    neg = int(torch.argmin(d["gbits"]))
    under = ref["under"][neg]
    assert bool(under.any()) and not bool(under.all())
    for cot in (True, False):
        (yh, bn, bq, ln, lq), grads = run_gc(kind, d, cot)
        if cot:
            gate(what + " y_hat", yh, r64["yh"], 6e-8)      # round(y - mu) is the reference's integer; one fp32 rounding of the sum with mu
            lik_gate(what + " lik_noisy", ln, r64["lik"])
            lik_gate(what + " lik_quant", lq, r64["qlik"])
            sum_gate(what + " bits_noisy", bn, r64["bits"], 1e-5)
            sum_gate(what + " bits_quant", bq, r64["qbits"], 1e-5)
            if c == 3:
                for nm, t in (("y_hat", yh), ("lik_noisy", ln), ("lik_quant", lq)):
                    padding_lane(f"{what} {nm}", t)
        tag = f"{what} cotangent {'present' if cot else 'absent'}"
        for i, nm in enumerate(("dy", "dmu", "dsigma")):
            grad_gate(f"{tag} {nm}", grads[i], r64[cot][i], r32[cot][i], 2e-5)
        dy, dmu, dsg = (g.cpu() for g in grads)
        exact(f"{tag} dsigma where the scale bound blocks it ({int(ref['sblocked'].sum())} elements)", dsg[ref["sblocked"]],
              torch.zeros(int(ref["sblocked"].sum())))
        k = int(under.sum())
        exact(f"{tag} dmu under the floor, negative weight ({k} elements)", dmu[neg][under], torch.zeros(k))
        exact(f"{tag} dsigma under the floor, negative weight", dsg[neg][under], torch.zeros(k))
        exact(f"{tag} dy under the floor, negative weight", dy[neg][under], d["gyh"][neg][under] if cot else torch.zeros(k))


@pytest.mark.parametrize("kind,c", R.GC_SMALL)
def test_gauss_cond_one_block_per_image(kind, c):
    """3 x C x 5 x 5: per_img <= 900, one block per image.  Dispatch: the four-channel kernels for C = 32, 36, the scalar ones for
    C = 1, 3, 6 (GC_KINDS: whatever the layout, strides and pointers reach the kernel as multiples of four floats)"""
    d, ref = gc_shared("small", c)
    check_gc(f"gauss_cond small {kind} C={c}", kind, d, ref)


@pytest.mark.parametrize("kind,c", R.GC_MEDIUM)
def test_gauss_cond_several_blocks_per_image(kind, c):
    """per_img = 3337 .. 4576, no multiple of 1024 nor of 256: 4 or 5 blocks per image, per-block partials and the finishing kernel"""
    d, ref = gc_shared("medium", c)
    check_gc(f"gauss_cond medium {kind} C={c}", kind, d, ref)


@pytest.mark.parametrize("shape", R.GC_BIG, ids=["vector", "scalar"])
def test_gauss_cond_grid_stride_second_pass(shape):
    """2 x 8 x 513 x 513 (vector): per_img = 2 105 352 > 2048 x 1024, the forward strides and the finishing kernel sums 2048 > 256
    partials per image; total / 4 = 1 052 676 > 4096 x 256, the backward strides.  2 x 3 x 419 x 419 (scalar): total = 1 053 366 >
    4096 x 256.  The smallest square sizes that reach those loops."""
    n, c, h, w = shape
    d = R.gc_case(f"gcd.big.{c}", n, c, h, w)
    check_gc(f"gauss_cond big C={c} {h}x{w}", "cl", d, gc_reference(d))


@pytest.mark.parametrize("c", [6, 32])
def test_gauss_cond_exact_grid_rounds_half_to_even(c):
    """y, mu on the 2^-4 grid: y - mu and round(y - mu) + mu are exact in fp32, ties of both parities included"""
    g = R.gc_grid_case(f"gcd.grid.{c}", 3, c, 5, 5)
    ref = torch.round(g["y"].double() - g["mu"].double()) + g["mu"].double()
    for noise in (None, cl(g["noise"])):
        yh = HF().gauss_cond(cl(g["y"]), cl(g["mu"]), cl(g["sigma"]), noise, 0.11, 1e-9, False)[0]
        exact(f"gauss_cond grid C={c} y_hat ({'eval' if noise is None else 'training'})", yh, ref)


@pytest.mark.parametrize("c", [6, 32])
def test_gauss_cond_nan_latent(c):
    """one NaN in y of image 1: that element of y_hat and of both likelihoods, that image's two bit sums and that element of the three
    gradients are NaN -- as in the reference -- and nothing else changes"""
    d, _ = gc_shared("small", c)
    at = (1, c // 2, 2, 3)
    dn = dict(d, y=d["y"].clone())
    dn["y"][at] = float("nan")
    y, mu, sg = (dn[k].double().requires_grad_(True) for k in ("y", "mu", "sigma"))
    yh64, l64 = R.gaussian_conditional(y, mu, sg, dn["noise"].double())
    b64 = R.bits_per_image(l64)
    ((b64 * dn["gbits"].double()).sum() + (yh64 * dn["gyh"].double()).sum()).backward()
    q64 = R.gaussian_conditional(y.detach(), mu.detach(), sg.detach(), None)[1]
    spot = torch.zeros(d["y"].shape, dtype=torch.bool)
    spot[at] = True
    for nm, t in (("y_hat", yh64), ("lik_noisy", l64), ("lik_quant", q64), ("dy", y.grad), ("dmu", mu.grad), ("dsigma", sg.grad)):
        assert torch.equal(torch.isnan(t), spot), "reference " + nm
    assert torch.isnan(b64).tolist() == [False, True, False] and torch.isnan(R.bits_per_image(q64)).tolist() == [False, True, False]
    (yh0, bn0, bq0, ln0, lq0), g0 = run_gc("cl", d, True)
    (yh1, bn1, bq1, ln1, lq1), g1 = run_gc("cl", dn, True)
    pairs = [("y_hat", yh0, yh1), ("lik_noisy", ln0, ln1), ("lik_quant", lq0, lq1), ("dy", g0[0], g1[0]), ("dmu", g0[1], g1[1]),
             ("dsigma", g0[2], g1[2])]
    for nm, a, b in pairs:
        a, b = a.detach().cpu().clone(), b.detach().cpu().clone()
        nan = torch.isnan(b)
        print(f"gauss_cond NaN C={c} {nm}: {int(nan.sum())} NaN, at the element: {bool(nan[at])}")
        assert torch.equal(nan, spot), nm
        a[at], b[at] = 0, 0
        exact(f"gauss_cond NaN C={c} {nm} elsewhere", b, a)
    for nm, a, b in (("bits_noisy", bn0, bn1), ("bits_quant", bq0, bq1)):
        a, b = a.cpu(), b.cpu()
        print(f"gauss_cond NaN C={c} {nm}: {b.tolist()}")
        assert torch.isnan(b).tolist() == [False, True, False], nm
        exact(f"gauss_cond NaN C={c} {nm} of images 0 and 2", b[[0, 2]], a[[0, 2]])


# ---- gauss_cond through the raw ABI -------------------------------------------------------------------------------------------------------

class Strided:
    """[N HW, ld] device rows prefilled with `fill`; channels [off, off + C) hold `t` ([N, C, H, W]) when given"""

    def __init__(self, shape, ld, off, t=None, fill=77.0):
        self.n, self.c, self.h, self.w = shape
        self.ld, self.off, self.fill = ld, off, fill
        self.buf = torch.full((self.n * self.h * self.w, ld), fill, dtype=F32, device=dev())
        if t is not None:
            self.buf[:, off:off + self.c] = t.permute(0, 2, 3, 1).reshape(-1, self.c).to(dev())

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.off

    def read(self):
        return self.buf[:, self.off:self.off + self.c].reshape(self.n, self.h, self.w, self.c).permute(0, 3, 1, 2).cpu()

    def untouched(self, what):
        rest = torch.cat([self.buf[:, :self.off], self.buf[:, self.off + self.c:]], 1)
        exact(what + " memory outside the written channels", rest, torch.full(tuple(rest.shape), self.fill))


# name -> C, then (ld, first channel) of y, mu, sigma, noise, yhat, yhat2, lik_noisy, lik_quant, dyhat, dy, dmu, dsigma.  Both
# likelihoods share ldlik and the three gradients ldgrad.  "vector": every stride and offset a multiple of 4; "misaligned": the same
# but y starts at channel 3, so its pointer is not 16-byte aligned; "odd": C = 5 and strides that are no multiples of 4.
RAW = {"vector": (8, [(12, 4), (16, 8), (8, 0), (20, 4), (24, 8), (12, 0), (16, 4), (16, 8), (12, 4), (28, 12), (28, 0), (28, 20)]),
       "misaligned": (8, [(12, 3), (16, 8), (8, 0), (20, 4), (24, 8), (12, 0), (16, 4), (16, 8), (12, 4), (28, 12), (28, 0), (28, 20)]),
       "odd": (5, [(7, 1), (9, 3), (5, 0), (6, 1), (11, 5), (10, 2), (13, 7), (13, 0), (9, 4), (17, 11), (17, 0), (17, 6)])}


@functools.lru_cache(maxsize=None)
def raw_shared(c):
    d = R.gc_case(f"gcd.raw.{c}", 3, c, 10, 15)
    return d, gc_reference(d)


@pytest.mark.parametrize("name", list(RAW))
def test_gauss_cond_raw_abi_strides(name):
    """crdr_gauss_cond_fwd2 / bwd2 on 3 x C x 10 x 15 (per_img = 1200 or 750) with distinct non-default ldlik, ldgrad, ldyhat, ldyhat2,
    ldnoise, lddyhat: values against float64, yhat2 bit-equal to yhat, memory between the written channels untouched, bit sums added into
    what the caller left there, the no-workspace path (one block per image) at the same gates, two runs bit-equal"""
    L, lib, ops = hip()
    c, lay = RAW[name]
    d, ref = raw_shared(c)
    r64, r32 = ref["r64"], ref["r32"]
    shape = tuple(d["y"].shape)
    n, _, h, w = shape
    lds, offs = [v[0] for v in lay], [v[1] for v in lay]
    assert R.gc_vector(c, lds, offs) == (name == "vector")
    y, mu, sg, nz = (Strided(shape, *lay[i], t=d[k]) for i, k in enumerate(("y", "mu", "sigma", "noise")))
    gyh = Strided(shape, *lay[8], t=d["gyh"])
    gb = d["gbits"].to(dev())
    what = f"gauss_cond raw {name} C={c}"

    def desc():
        return L.GcDesc2(N=n, HW=h * w, C=c, ldy=lds[0], ldmu=lds[1], ldsigma=lds[2], ldnoise=lds[3], ldyhat=lds[4], ldyhat2=lds[5],
                         ldlik=lds[6], lddyhat=lds[8], ldgrad=lds[9], scale_bound=0.11, likelihood_bound=1e-9)

    def forward(workspace, prefill):
        o = [Strided(shape, *lay[i]) for i in (4, 5, 6, 7)]
        bn, bq = (torch.full((n,), prefill, dtype=F32, device=dev()) for _ in range(2))
        io = L.GcIO(y=y.ptr, mu=mu.ptr, sigma=sg.ptr, noise=nz.ptr, yhat=o[0].ptr, yhat2=o[1].ptr, lik_noisy=o[2].ptr, lik_quant=o[3].ptr,
                    bits_noisy=bn.data_ptr(), bits_quant=bq.data_ptr())
        if workspace:
            HF().gauss_cond_fwd2(desc(), io, dev())
        else:
            L.check(lib.crdr_gauss_cond_fwd2(C.byref(desc()), C.byref(io), ops._stream()), "gauss_cond_fwd2")
        return o, bn.cpu(), bq.cpu()

    for workspace in (True, False):
        tag = what + (" workspace" if workspace else " no workspace")
        o, bn, bq = forward(workspace, 3.5)
        gate(tag + " yhat", o[0].read(), r64["yh"], 6e-8)
        exact(tag + " yhat2 against yhat", o[1].read(), o[0].read())
        lik_gate(tag + " lik_noisy", o[2].read(), r64["lik"])
        lik_gate(tag + " lik_quant", o[3].read(), r64["qlik"])
        for nm, t in zip(("yhat", "yhat2", "lik_noisy", "lik_quant"), o):
            t.untouched(f"{tag} {nm}")
        sum_gate(tag + " 3.5 + bits_noisy", bn, 3.5 + r64["bits"], 1e-5)
        sum_gate(tag + " 3.5 + bits_quant", bq, 3.5 + r64["qbits"], 1e-5)
        _, bn2, bq2 = forward(workspace, 3.5)
        exact(tag + " bit sums of a second run", torch.stack([bn2, bq2]), torch.stack([bn, bq]))
    for cot in (True, False):
        tag = f"{what} cotangent {'present' if cot else 'absent'}"
        g = [Strided(shape, *lay[i]) for i in (9, 10, 11)]
        io = L.GcIO(y=y.ptr, mu=mu.ptr, sigma=sg.ptr, noise=nz.ptr, gbits=gb.data_ptr(), dyhat=gyh.ptr if cot else None, dy=g[0].ptr,
                    dmu=g[1].ptr, dsigma=g[2].ptr)
        L.check(lib.crdr_gauss_cond_bwd2(C.byref(desc()), C.byref(io), ops._stream()), "gauss_cond_bwd2")
        for i, nm in enumerate(("dy", "dmu", "dsigma")):
            grad_gate(f"{tag} {nm}", g[i].read(), r64[cot][i], r32[cot][i], 2e-5)
            g[i].untouched(f"{tag} {nm}")


# ---- Philox ----------------------------------------------------------------------------------------------------------------------------

def philox_state():
    return torch.tensor([R.PHILOX_SEED, R.PHILOX_OFFSET], dtype=torch.int64, device=dev())


def test_philox_uniform_equals_its_restatement():
    """crdr_philox_uniform against the numpy Philox4x32-10 at tolerance 0: a full 2 x 12 x 35 tensor and the (c0, Ctot) = (3, 12) slice of
    5 channels at pixel stride 7; both key words in use, the counter carries into its second word inside the tensor"""
    L, lib, ops = hip()
    st = philox_state()
    n, hw, ctot = 2, 35, 12
    full = Strided((n, ctot, 5, 7), ctot, 0)
    L.check(lib.crdr_philox_uniform(st.data_ptr(), n, hw, ctot, ctot, 0, full.ptr, ctot, ops._stream()), "philox_uniform")
    exact("philox_uniform full tensor", full.read().reshape(n, ctot, hw), R.philox_uniform(R.PHILOX_SEED, R.PHILOX_OFFSET, n, hw, ctot))
    part = Strided((n, 5, 5, 7), 7, 1)
    L.check(lib.crdr_philox_uniform(st.data_ptr(), n, hw, 5, ctot, 3, part.ptr, 7, ops._stream()), "philox_uniform")
    exact("philox_uniform slice c0=3 C=5 of 12", part.read().reshape(n, 5, hw), R.philox_uniform(R.PHILOX_SEED, R.PHILOX_OFFSET, n, hw, 5, ctot, 3))
    part.untouched("philox_uniform slice")
    assert st.tolist() == [R.PHILOX_SEED, R.PHILOX_OFFSET]


@pytest.mark.parametrize("c,c0,ctot", [(8, 8, 24), (5, 3, 24)], ids=["vector", "scalar"])
def test_gauss_cond_philox_noise_equals_given_noise(c, c0, ctot):
    """fwd2 / bwd2 drawing their noise in the kernel (io.philox, channels [c0, c0 + C) of a Ctot-wide latent) give outputs bit-equal to the
    same calls with io.noise holding the restated samples"""
    L, lib, ops = hip()
    d, ref = raw_shared(c)
    shape = tuple(d["y"].shape)
    n, _, h, w = shape
    assert R.gc_vector(c, ctot=ctot, c0=c0) == (c == 8)
    nz = R.philox_uniform(R.PHILOX_SEED, R.PHILOX_OFFSET, n, h * w, c, ctot, c0).reshape(n, c, h, w)
    y, mu, sg, gyh, noise = (Strided(shape, c, 0, t=t) for t in (d["y"], d["mu"], d["sigma"], d["gyh"], nz))
    st, gb = philox_state(), d["gbits"].to(dev())
    outs = []
    for given in (True, False):
        src = {"noise": noise.ptr} if given else {"philox": st.data_ptr()}
        o = [Strided(shape, c, 0) for _ in range(6)]
        bn, bq = (torch.zeros(n, dtype=F32, device=dev()) for _ in range(2))
        desc = L.GcDesc2(N=n, HW=h * w, C=c, ldy=c, ldmu=c, ldsigma=c, ldyhat=c, lddyhat=c, Ctot=ctot, c0=c0, scale_bound=0.11,
                         likelihood_bound=1e-9)
        io = L.GcIO(y=y.ptr, mu=mu.ptr, sigma=sg.ptr, yhat=o[0].ptr, lik_noisy=o[1].ptr, lik_quant=o[2].ptr, bits_noisy=bn.data_ptr(),
                    bits_quant=bq.data_ptr(), **src)
        HF().gauss_cond_fwd2(desc, io, dev())
        io = L.GcIO(y=y.ptr, mu=mu.ptr, sigma=sg.ptr, gbits=gb.data_ptr(), dyhat=gyh.ptr, dy=o[3].ptr, dmu=o[4].ptr, dsigma=o[5].ptr, **src)
        L.check(lib.crdr_gauss_cond_bwd2(C.byref(desc), C.byref(io), ops._stream()), "gauss_cond_bwd2")
        outs.append([t.read() for t in o] + [bn.cpu(), bq.cpu()])
    for nm, a, b in zip(("yhat", "lik_noisy", "lik_quant", "dy", "dmu", "dsigma", "bits_noisy", "bits_quant"), *outs):
        exact(f"gauss_cond philox C={c} c0={c0} {nm}: in-kernel noise against given noise", b, a)
    lik_gate(f"gauss_cond philox C={c} lik_noisy", outs[1][1], R.gaussian_likelihood(d["y"].double() + nz.double(), d["mu"].double(), d["sigma"].double()))


@pytest.mark.parametrize("shape", [(2, 6, 4, 4), (1, 8, 3, 5)], ids=["scalar", "vector"])
def test_gauss_cond_wrapper_philox_equals_given_noise(shape):
    """HF.gauss_cond drawing its noise in the kernel (philox_state) against the same call given crdr_philox_uniform's samples for the pair
    the call forks (the state as it stands before the call): every output and all three gradients bit-equal; the state moves on by the
    fork's increment, numel / 4 rounded up, plus one."""
    L, lib, ops = hip()
    n, c, h, w = shape
    d = R.gc_case("gcd.dispatch.%d" % c, n, c, h, w)
    st = philox_state()
    nz = torch.empty(n, h, w, c, dtype=F32, device=dev())
    L.check(lib.crdr_philox_uniform(st.data_ptr(), n, h * w, c, c, 0, nz.data_ptr(), c, ops._stream()), "philox_uniform")
    gb, gyh = d["gbits"].to(dev()), cl(d["gyh"])
    res = []
    for src in ({"philox_state": st}, {"noise": nz.permute(0, 3, 1, 2)}):
        leaves = [cl(d[k]).requires_grad_(True) for k in ("y", "mu", "sigma")]
        out = HF().gauss_cond(*leaves, src.get("noise"), 0.11, 1e-9, True, philox_state=src.get("philox_state"))
        ((out[1] * gb).sum() + (out[0] * gyh).sum()).backward()
        res.append(list(out) + [t.grad for t in leaves])
    assert st.tolist() == [R.PHILOX_SEED, R.PHILOX_OFFSET + (n * c * h * w + 3) // 4 + 1]
    for nm, a, b in zip(("y_hat", "bits_noisy", "bits_quant", "lik_noisy", "lik_quant", "dy", "dmu", "dsigma"), *res):
        assert a is not None and b is not None, nm
        exact(f"gauss_cond wrapper {n}x{c}x{h}x{w} {nm}: in-kernel noise against given noise", a, b)


# ---- entropy bottleneck ----------------------------------------------------------------------------------------------------------------

def eb_module(sd, c):
    from crdr_amd.models.subnet.entropy_model.entropy_bottleneck import SteEntropyBottleneck
    m = SteEntropyBottleneck(channels=c)
    with torch.no_grad():
        for k, v in m.named_parameters():
            v.copy_(sd[f"{R.EB}.{k}"])
    return m.to(dev())


def eb_reference(sd, d):
    out = {}
    for name, dt in (("r64", F64), ("r32", F32)):
        sdg = R.as_dtype(sd, dt, grad=True)
        z = d["z"].to(dt).clone().requires_grad_(True)
        nz, gb, gzh = d["noise"].to(dt), d["gbits"].to(dt), d["gzh"].to(dt)
        zh, lik = R.entropy_bottleneck(sdg, z, nz)
        bits = R.bits_per_image(lik)
        keys = sorted(sdg)
        g0 = torch.autograd.grad((bits * gb).sum(), [z] + [sdg[k] for k in keys], retain_graph=True, allow_unused=True)
        g1 = torch.autograd.grad((bits * gb).sum() + (zh * gzh).sum(), [z] + [sdg[k] for k in keys], allow_unused=True)
        with torch.no_grad():
            zq, qlik = R.entropy_bottleneck(sdg, z, None)
        out[name] = {"zh": zh.detach(), "lik": lik.detach(), "bits": bits.detach(), "zq": zq, "qlik": qlik, "qbits": R.bits_per_image(qlik),
                     False: (g0[0], dict(zip(keys, g0[1:]))), True: (g1[0], dict(zip(keys, g1[1:])))}
    sd64 = R.as_dtype(sd, F64)
    out["under"] = R.eb_likelihood(sd64, d["z"].double() + d["noise"].double(), raw=True) < R.LIK_BOUND
    return out


@pytest.mark.parametrize("nhw", R.EB_SIZES)
@pytest.mark.parametrize("c", R.EB_CHANNELS)
def test_entropy_bottleneck_matches_float64(c, nhw):
    """SteEntropyBottleneck on seeded parameters: training path with and without a z_hat cotangent under the mixed-sign bit weights (every
    named parameter gradient against the oracle's float64 one), eval path, bit sums.  N HW = 1 .. 1021: one thread of the channel's block
    up to four strided passes with a partial last one, one to four waves in the reduction of the 58 sums"""
    sd, d = R.eb_case(c, nhw)
    ref = eb_reference(sd, d)
    r64, r32 = ref["r64"], ref["r32"]
    what = f"eb C={c} NHW={nhw}"
    n = d["z"].shape[0]
    neg = int(torch.argmin(d["gbits"]))
    for cot in (True, False):
        m = eb_module(sd, c)
        zd = cl(d["z"]).requires_grad_(True)
        zh, lik, bits = m(zd, is_train=True, noise=cl(d["noise"]), want_bits=True)
        loss = (bits * d["gbits"].to(dev())).sum()
        if cot:
            loss = loss + (zh * d["gzh"].to(dev())).sum()
        loss.backward()
        tag = f"{what} cotangent {'present' if cot else 'absent'}"
        if cot:
            gate(what + " z_hat", zh, r64["zh"], 6e-8)
            gate(what + " lik", lik, r64["lik"], 2e-5)
            sum_gate(what + " bits", bits, r64["bits"], 2e-5)
        grad_gate(tag + " dz", zd.grad, r64[cot][0], r32[cot][0], 2e-5)
        for k, p in m.named_parameters():
            g64, g32 = r64[cot][1][f"{R.EB}.{k}"], r32[cot][1][f"{R.EB}.{k}"]
            if p.grad is None:   # the medians under straight-through rounding: the float64 gradient is exactly 0 or absent
                assert k == "quantiles" and (g64 is None or g64.abs().max().item() == 0), k
                continue
            grad_gate(f"{tag} d{k}", p.grad, g64, g32, 5e-5)
        if d["gbits"][neg] < 0 and bool(ref["under"][neg].any()):
            under = ref["under"][neg]
            k = int(under.sum())
            exact(f"{tag} dz under the floor, negative weight ({k} elements)", zd.grad.cpu()[neg][under],
                  d["gzh"][neg][under] if cot else torch.zeros(k))
    m = eb_module(sd, c)
    zq, qlik, qbits = m(cl(d["z"]), is_train=False, want_bits=True)
    gate(what + " eval z_hat", zq, r64["zq"], 6e-8)
    gate(what + " eval lik", qlik, r64["qlik"], 2e-5)
    sum_gate(what + " eval bits", qbits, r64["qbits"], 2e-5)


@pytest.mark.parametrize("c", R.EB_CHANNELS)
def test_entropy_bottleneck_exact_grid(c):
    """z on the 2^-4 grid, medians off it: z_hat equals the float64 round(z - median) + median, rounded once to fp32, on both paths"""
    sd, d = R.eb_case(c, 255, grid=True)
    med = sd[R.EB + ".quantiles"][:, 0, 1].double().reshape(1, -1, 1, 1)
    ref = (torch.round(d["z"].double() - med) + med).float()
    m = eb_module(sd, c)
    exact(f"eb grid C={c} z_hat (training)", m(cl(d["z"]), is_train=True, noise=cl(d["noise"]))[0], ref)
    exact(f"eb grid C={c} z_hat (eval)", m(cl(d["z"]), is_train=False)[0], ref)


def test_entropy_bottleneck_bits_accumulate():
    """crdr_entropy_bottleneck_fwd adds the bit sums into what the caller left there"""
    L, lib, ops = hip()
    c = 6
    sd, d = R.eb_case(c, 48)
    ref = eb_reference(sd, d)["r64"]
    m = eb_module(sd, c)
    shape = tuple(d["z"].shape)
    n, _, h, w = shape
    z, nz, zh, lik = Strided(shape, c, 0, t=d["z"]), Strided(shape, c, 0, t=d["noise"]), Strided(shape, c, 0), Strided(shape, c, 0)
    bits = torch.full((n,), 5.0, dtype=F32, device=dev())
    params, med = m.packed_params().detach().contiguous(), m.quantiles.detach()[:, 0, 1].contiguous()
    L.check(lib.crdr_entropy_bottleneck_fwd(z.ptr, nz.ptr, params.data_ptr(), med.data_ptr(), n, h * w, c, 1e-9, zh.ptr, lik.ptr,
                                            bits.data_ptr(), ops._stream()), "entropy_bottleneck_fwd")
    gate("eb raw lik", lik.read(), ref["lik"], 2e-5)
    sum_gate("eb raw 5 + bits", bits, 5.0 + ref["bits"], 2e-5)


@pytest.mark.parametrize("c", R.AUX_CHANNELS)
def test_eb_aux_loss_matches_float64(c):
    """sum |logits(quantiles) - target| and its gradient with respect to the quantiles; 3 C = 258 > 256 at C = 86: a second pass"""
    sd = R.eb_state(c)
    m = eb_module(sd, c)
    loss = m.loss()
    loss.backward()
    refs = {}
    for name, dt in (("r64", F64), ("r32", F32)):
        sdg = R.as_dtype(sd, dt, grad=True)
        aux = R.eb_aux_loss(sdg)
        aux.backward()
        refs[name] = (aux.detach(), sdg[R.EB + ".quantiles"].grad)
    sum_gate(f"eb aux C={c} loss", loss, refs["r64"][0], 2e-5)
    grad_gate(f"eb aux C={c} dquantiles", m.quantiles.grad, refs["r64"][1], refs["r32"][1], 5e-5)
    for k, p in m.named_parameters():
        assert k == "quantiles" or p.grad is None, k      # the density network is detached


# ---- crdr_gauss_symbols ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("levels", R.SYMBOL_LEVELS)
def test_gauss_symbols_exact(levels):
    """int32 symbols round(y - mu) (exact ties, half to even) and scale-table indexes (sigma exactly on table entries, at the bound and
    below it) in (n, c, pixel) order, from dense rows and from strided channel slices, both outputs, symbols only and indexes only"""
    L, lib, ops = hip()
    y, mu, sg, table = R.symbol_case(levels)
    shape = tuple(y.shape)
    n, c, h, w = shape
    ref_sym, ref_idx = R.symbols(y.double(), mu.double()), R.build_indexes(sg.double(), table.double())
    tab = table.to(dev())
    for name, lay in (("dense", [(c, 0)] * 3), ("strided", [(9, 2), (8, 1), (11, 3)])):
        ys, ms, ss = (Strided(shape, *lay[i], t=t) for i, t in enumerate((y, mu, sg)))
        for want_sym, want_idx in ((True, True), (True, False), (False, True)):
            sym, idx = (torch.full(shape, -7, dtype=torch.int32, device=dev()) for _ in range(2))
            L.check(lib.crdr_gauss_symbols(ys.ptr if want_sym else None, ys.ld, ms.ptr if want_sym else None, ms.ld,
                                           ss.ptr if want_idx else None, ss.ld, tab.data_ptr() if want_idx else None, levels, 0.11, n, h * w, c,
                                           sym.data_ptr() if want_sym else None, idx.data_ptr() if want_idx else None, ops._stream()),
                    "gauss_symbols")
            what = f"gauss_symbols levels={levels} {name} ({'symbols' if want_sym else ''}{'+' if want_sym and want_idx else ''}{'indexes' if want_idx else ''})"
            exact(what + " symbols", sym, ref_sym if want_sym else torch.full(shape, -7, dtype=torch.int32))
            exact(what + " indexes", idx, ref_idx if want_idx else torch.full(shape, -7, dtype=torch.int32))
