"""Direct GPU parity of crdr_gan_loss_fwd / crdr_gan_loss_bwd (csrc/ganloss.hip) through crdr_amd.hip.functional.gan_loss_sum against the
float64 restatement tests/gan_loss_ref.py: every kind x {no q, paired, centred with nq = 1 and 300} x {mask, no mask} x n in {1, 63, 256,
257, 4099, 2^20 + 4099} (the last is past the 1024-block cap: every thread runs its loop a fifth time), value, dp and dq.

Gates are rounding counts in units of 2^-24, evaluated in float64 on each input, to first order in 2^-24 like
tests/test_gpu_eltwise_direct.py::reduce_gate, whose helpers (`reduce_chain`, `bce_term_roundings`) are used as they are:
  value   |got - ref| <= 2^-24 (k sum_i |m_i l_i| + sum_i m_i b_i + sum_i |m_i l_i| + dr sum_i m_i |l'_i|)
          k = reduce_chain(n): the kernel keeps reduce_kernel / reduce_final's structure (same grid rule, same thread loop, shuffle tree, four
          wave sums); the terms may have either sign (kind 2), so a step of the chain costs 2^-24 of the sum of MAGNITUDES;
          b_i = the roundings inside one term: kind 0: bce_term_roundings' count (x = p - r, x t, the difference, expf, log1pf, the final
          add), evaluated per mask value; kind 1: the subtraction p - r moves an active term by |x| and 1 - sgn x is rounded once:
          |x_i| + |l_i| on the active set, 0 off it; kind 2: |x_i| (the subtraction alone: the negation is exact);
          |m_i l_i| again for the product with the mask;
          dr (centred form) = what mean(q) carries: (k_q sum_j |q_j| / nq + |mean|) 2^-24 for its own chain and the division; it moves every
          term by |l'_i| dr (|l'| <= 1 for all kinds).
  dp      per element: kind 0: |g m_i| (|x_i| / 4 + 3.5 + 3 |s_i - t| + t) 2^-24 + |g m_i| dr / 4 (s = sigmoid: the rounding of x through
          s' <= 1/4, expf's 2 x 2^-24 through s (1 - s) <= 1/4, the addition 1 + e and the division through s <= 1, the difference s - t, t's
          own fp32 value, the products g m and (g m)(s - t));  kinds 1, 2: the value is g m_i or 0: 2 |g m_i| 2^-24 -- and the ACTIVE SET is
          exact: no seeded logit lies within 1e-3 of a hinge kink (counted on the float64 side, asserted 0).
  dq      paired: exactly -dp;  centred: one value everywhere, within (k sum_i |dp_i| 2^-24 + sum_i bound(dp_i)) / nq + 2 |dq| 2^-24 of
          -(sum_i dp_i) / nq.
Every comparison prints its figure before it asserts (profiles/gan_loss_test_margins.txt)."""
import ast
import ctypes

import pytest
import torch

from tests import eltwise_ref as ER
from tests import gan_loss_ref as R
from tests.test_gpu_eltwise_direct import HF, U, bce_term_roundings, exact, reduce_chain
from tests.test_gpu_model import dev

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 256, 257, 4099, 2 ** 20 + 4099]
FORMS = {"noq": ("none", None), "paired": ("paired", None), "centred1": ("centred", 1), "centred300": ("centred", 300)}
KINDS = {"bce1": (R.BCE, 1.0, 1.0), "bce0.1": (R.BCE, 0.1, 1.0), "hingeD+": (R.HINGE_D, 0.0, 1.0), "hingeD-": (R.HINGE_D, 0.0, -1.0),
         "hingeG": (R.HINGE_G, 0.0, 1.0)}
G_UP = float(torch.tensor(0.37))   # the upstream gradient, as fp32 holds it


def mean_error(q64):
    """dr in units of 2^-24: the chain of the sum over q and the rounding of the division (float(nq) is exact below 2^24)"""
    return reduce_chain(q64.numel()) * q64.abs().sum().item() / q64.numel() + abs(q64.mean().item())


def term_roundings(x64, m64, kind, target, sgn):
    """sum_i m_i b_i + sum_i |m_i l_i| in units of 2^-24 (module docstring)"""
    l = R.terms(x64, kind, target, sgn)
    mask_product = 0.0 if m64 is None else (m64 * l).abs().sum().item()
    w = torch.ones_like(x64) if m64 is None else m64
    if kind == R.BCE:
        inner = 0.0
        for v in torch.unique(w).tolist():
            if v == 0.0:
                continue
            xs = x64[w == v]
            inner += v * bce_term_roundings(xs, target) * ER.bce_terms(xs, target).sum().item()
    elif kind == R.HINGE_D:
        inner = (w * (l > 0) * (x64.abs() + l)).sum().item()
    else:
        inner = (w * x64.abs()).sum().item()
    return inner + mask_product


def slope_roundings(x64, kind, target, sgn, dr):
    """per-element bound of l'(x) before the factor |g m_i|, in units of 2^-24"""
    if kind != R.BCE:
        return torch.full_like(x64, 2.0)
    s = torch.sigmoid(x64)
    return x64.abs() / 4 + 3.5 + 3 * (s - target).abs() + target + dr / 4


def value_tolerance(x64, m64, kind, target, sgn, dr=0.0):
    """the gate of the summed value (module docstring), absolute"""
    w64 = torch.ones_like(x64) if m64 is None else m64
    l64 = R.terms(x64, kind, target, sgn) * w64
    return U * (reduce_chain(x64.numel()) * l64.abs().sum().item() + term_roundings(x64, m64, kind, target, sgn)
                + dr * (w64 * R.slope(x64, kind, target, sgn).abs()).sum().item())


def run_hip(p, q, mask, kind, target, sgn, center, grads=True):
    pd = p.to(dev()).requires_grad_(grads)
    qd = None if q is None else q.to(dev()).requires_grad_(grads)
    md = None if mask is None else mask.to(dev())
    v = HF().gan_loss_sum(pd, qd, kind=kind, target=target, sgn=sgn, center=center, mask=md)
    if grads:
        (v * 0.37).backward()
    return v.detach(), pd.grad, None if qd is None else qd.grad


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kname", list(KINDS))
def test_gan_loss_matches_float64(kname, n, form, masked):
    kind, target, sgn = KINDS[kname]
    fname, nq = FORMS[form]
    center = fname == "centred"
    p, q, mask = R.case(n, fname, nq, masked)
    what = f"{kname} n={n} {form} {'mask' if masked else 'nomask'}"
    p64, q64, m64 = p.double(), None if q is None else q.double(), None if mask is None else mask.double()
    x64 = R.argument(p64, q64, center)
    kinks = R.kink_count(x64)
    print(f"{what}: {kinks} logits within {R.KINK_WINDOW} of a hinge kink (gate 0)")
    assert kinks == 0
    kw = dict(kind=kind, target=target, sgn=sgn, center=center, mask=m64)
    v64 = R.gan_loss_sum(p64, q64, **kw)
    dp64, dq64 = R.gan_loss_grads(p64, q64, g=G_UP, **kw)
    w64 = torch.ones_like(x64) if m64 is None else m64
    l64 = R.terms(x64, kind, target, sgn) * w64
    dr = mean_error(q64) if center else 0.0

    v, dp, dq = run_hip(p, q, mask, kind, target, sgn, center)
    # value
    k = reduce_chain(n)
    tol = value_tolerance(x64, m64, kind, target, sgn, dr)
    e = abs(v.cpu().double().item() - v64.item())
    print(f"{what} value: |err| {e:.3e} of {v64.item():.6e} (gate {tol:.3e}: chain k={k})")
    assert e <= tol, (what, e, tol)
    # dp
    bound = U * G_UP * w64 * slope_roundings(x64, kind, target, sgn, dr)
    err = (dp.cpu().double() - dp64).abs()
    worst = (err / bound.clamp(min=1e-300)).max().item() if n else 0.0
    print(f"{what} dp: max |err| {err.max().item():.3e}, {worst:.3f} of its bound (gate 1)")
    assert bool((err <= bound).all()), (what, worst)
    if kind == R.HINGE_D:
        exact(f"{what} active set", dp != 0, dp64 != 0)
    # dq
    if fname == "none":
        assert dq is None
    elif fname == "paired":
        exact(f"{what} dq == -dp", dq, -dp)
    else:
        assert dq.shape == (nq,)
        exact(f"{what} dq is one value", dq, dq[:1].expand(nq))
        tol_q = (U * k * dp64.abs().sum().item() + bound.sum().item()) / nq + 2 * U * abs(dq64[0].item())
        e = abs(dq[0].cpu().double().item() - dq64[0].item())
        print(f"{what} dq: |err| {e:.3e} of {dq64[0].item():.6e} (gate {tol_q:.3e})")
        assert e <= tol_q, (what, e, tol_q)
    # a second call: the same bits; without gradients: the same value
    v2, dp2, dq2 = run_hip(p, q, mask, kind, target, sgn, center)
    exact(f"{what} second call value", v2, v)
    exact(f"{what} second call dp", dp2, dp)
    if dq is not None:
        exact(f"{what} second call dq", dq2, dq)
    v3, _, _ = run_hip(p, q, mask, kind, target, sgn, center, grads=False)
    exact(f"{what} value without gradients", v3, v)


@pytest.mark.parametrize("grad_to", ["p", "q"])
@pytest.mark.parametrize("form", ["paired", "centred300"])
def test_gan_loss_gradient_to_one_operand(form, grad_to):
    """dp or dq NULL: the other comes out with the bits of the two-gradient call"""
    fname, nq = FORMS[form]
    p, q, _ = R.case(4099, fname, nq)
    _, dp, dq = run_hip(p, q, None, R.BCE, 1.0, 1.0, fname == "centred")
    pd, qd = p.to(dev()).requires_grad_(grad_to == "p"), q.to(dev()).requires_grad_(grad_to == "q")
    (HF().gan_loss_sum(pd, qd, kind=R.BCE, target=1.0, center=fname == "centred") * 0.37).backward()
    if grad_to == "p":
        assert qd.grad is None
        exact(f"{form} dp alone", pd.grad, dp)
    else:
        assert pd.grad is None
        exact(f"{form} dq alone", qd.grad, dq)


@pytest.mark.parametrize("n", [257, 2 ** 20 + 4099])
@pytest.mark.parametrize("target", [1.0, 0.0, 0.9])
def test_paired_bce_is_bce_diff_sum(n, target):
    """kind 0, paired, no mask: the bits of crdr_bce_diff_sum / crdr_bce_diff_bwd, which the stage-3 trainer keeps using"""
    p, q, _ = R.case(n, "paired")
    v, dp, dq = run_hip(p, q, None, R.BCE, target, 1.0, False)
    pd, qd = p.to(dev()).requires_grad_(True), q.to(dev()).requires_grad_(True)
    v0 = HF().bce_diff_sum(pd, qd, target)
    (v0 * 0.37).backward()
    exact(f"bce_diff_sum n={n} t={target} value", v, v0.detach())
    exact(f"bce_diff_sum n={n} t={target} dp", dp, pd.grad)
    exact(f"bce_diff_sum n={n} t={target} dq", dq, qd.grad)


@pytest.mark.parametrize("kname,form", [("bce1", "centred300"), ("hingeD+", "centred300"), ("bce0.1", "paired"), ("hingeG", "noq")])
def test_captured_graph_replays_to_the_eager_bits(kname, form):
    """forward + backward captured once on one set of logits, replayed on two others: value, dp, dq equal the eager call's bits -- the
    mean of the centred form is read from device memory by the replay, not baked in at capture"""
    from crdr_amd.hip import ops
    kind, target, sgn = KINDS[kname]
    fname, nq = FORMS[form]
    center, n = fname == "centred", 4099
    data = []
    for i in range(3):
        p, q, m = R.case(n, fname, nq, True)
        data.append((torch.roll(p, 17 * i) + 0.25 * i, None if q is None else torch.roll(q, 5 * i) - 0.5 * i, m))
    want = [run_hip(p, q, m, kind, target, sgn, center) for p, q, m in data]
    ps = data[0][0].to(dev()).requires_grad_(True)
    qs = None if data[0][1] is None else data[0][1].to(dev()).requires_grad_(True)
    ms = data[0][2].to(dev())

    def step():
        v = HF().gan_loss_sum(ps, qs, kind=kind, target=target, sgn=sgn, center=center, mask=ms)
        gs = torch.autograd.grad(v * 0.37, [ps] + ([qs] if qs is not None else []))
        return v.detach(), gs[0], (gs[1] if qs is not None else None)
    step()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    ops.reserve_workspace(dev(), side)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        v, dp, dq = step()
    for i in (1, 2, 0):
        with torch.no_grad():
            ps.copy_(data[i][0])
            if qs is not None:
                qs.copy_(data[i][1])
        g.replay()
        torch.cuda.synchronize()
        exact(f"{kname} {form} replay {i} value", v, want[i][0])
        exact(f"{kname} {form} replay {i} dp", dp, want[i][1])
        if qs is not None:
            exact(f"{kname} {form} replay {i} dq", dq, want[i][2])


CLASS_SIDES = {"d_real": (True, True), "d_fake": (False, True), "g_real": (True, False), "g_fake": (False, False)}


@pytest.mark.parametrize("name", ["VanillaGANLoss", "MaskedVanillaGANLoss", "MultiscaleVanillaGANLoss", "HingeGANLoss", "MultiscaleHingeGANLoss"])
def test_loss_classes_match_the_recorded_reference(name):
    """the five registered classes on the inputs of tests/golden/reference_gan_loss.npz (fp32 copies), against the float64 restatement on
    those copies: a class value is (weight / n) x the kernel's sum per scale, so its gate is that factor times the sum's gate plus two
    roundings (the division, the weight) of each scale's value and one per addition of scales; dx against the recorded gradient within
    the per-element bound of dp.  The recorded reference value itself is met to fp32 input rounding (printed, not gated here: the host test
    holds the restatement to it at 1e-12)."""
    import os
    import numpy as np
    from crdr_amd.losses import build_loss
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_gan_loss.npz"))
    kwargs = ast.literal_eval(str(gold["meta.ctor_kwargs"]))[name]
    m = build_loss({"type": name, **kwargs})
    multi, hinge = name.startswith("Multiscale"), "Hinge" in name
    w = kwargs["loss_weight"]
    for side, (is_real, is_disc) in CLASS_SIDES.items():
        key = f"loss.{name}.{side}"
        if key + ".value" not in gold.files:
            continue
        xs = [torch.from_numpy(gold[f"{key}.x{i}"]).float() for i in range(2)] if multi else [torch.from_numpy(gold[key + ".x"]).float()]
        mask = torch.from_numpy(gold[key + ".mask"]).float() if name == "MaskedVanillaGANLoss" else None
        kind = (R.HINGE_D if is_disc else R.HINGE_G) if hinge else R.BCE
        target = 0.0 if hinge else (kwargs.get("real_label", 1.0) if is_real else kwargs.get("fake_label", 0.0))
        sgn = 1.0 if is_real else -1.0
        xd = [x.to(dev()).requires_grad_(True) for x in xs]
        extra = {} if mask is None else {"mask": mask.to(dev())}
        v = m(xd if multi else xd[0], is_real=is_real, is_disc=is_disc, **extra)
        (v * 0.37).backward()
        x64 = [x.double() for x in xs]
        m64 = None if mask is None else mask.double()
        v64 = R.LOSSES[name](x64 if multi else x64[0], is_real, is_disc, **kwargs, **({} if m64 is None else {"mask": m64}))
        f = (1.0 if is_disc else abs(w)) / (len(xs) if (multi and not hinge) else 1)
        tol = sum(f / x.numel() * value_tolerance(x.reshape(-1), None if m64 is None else m64.reshape(-1), kind, target, sgn) for x in x64)
        tol += U * (2 + len(xs)) * sum(f / x.numel() * abs(R.gan_loss_sum(x, kind=kind, target=target, sgn=sgn, mask=m64).item()) for x in x64)
        e = abs(v.item() - v64.item())
        print(f"{name} {side} value: |err| {e:.3e} of {v64.item():.6e} (gate {tol:.3e}); recorded reference {float(gold[key + '.value']):.6e}")
        assert e <= tol, (name, side, e, tol)
        for i, (x, xg) in enumerate(zip(x64, xd)):
            g = G_UP * f / x.numel()
            w64 = torch.ones_like(x) if m64 is None else m64
            dx64, _ = R.gan_loss_grads(x, kind=kind, target=target, sgn=sgn, mask=m64, g=g)
            bound = U * g * w64 * (slope_roundings(x, kind, target, sgn, 0.0) + 3)   # (+ 3: the factors weight, 1 / n, 1 / scales in g)
            err = (xg.grad.cpu().double() - dx64).abs()
            print(f"{name} {side} dx{i}: max |err| {err.max().item():.3e}, {(err / bound.clamp(min=1e-300)).max().item():.3f} of its bound (gate 1)")
            assert bool((err <= bound).all()), (name, side, i)
    if hinge:   # the forms the relativistic trainers would hand a hinge loss: exactly the kernel's sums, scaled
        p, q, _ = R.case(257, "paired")
        pd, qd = p.to(dev()), q.to(dev())
        exact("hinge forward_diff D", m.forward_diff(pd, qd, True, True), HF().gan_loss_sum(pd, qd, kind=R.HINGE_D, sgn=1.0).reshape(()) / 257)
        exact("hinge forward_centered D fake", m.forward_centered(pd, qd[:100], False, True),
              HF().gan_loss_sum(pd, qd[:100], kind=R.HINGE_D, sgn=-1.0, center=True).reshape(()) / 257)
        exact("hinge forward_diff G", m.forward_diff(pd, qd, True, False), w * (HF().gan_loss_sum(pd, qd, kind=R.HINGE_G).reshape(()) / 257))


def test_bad_arguments_are_refused():
    """every refusal is an error return of the C entry (or a ValueError of the wrapper) before any launch"""
    from crdr_amd.hip import lib as L, ops
    lib = L.load()
    n = 300
    p, q, out, stats = (torch.zeros(k, device=dev()) for k in (n + 1, n + 1, 1, 2))
    dp = torch.zeros(n + 1, device=dev())
    g = torch.ones(1, device=dev())
    ws, wsn = ops.workspace(lib.crdr_gan_loss_workspace(n, n), dev())
    st = ops._stream()

    def fwd(d, pp=p.data_ptr(), qq=q.data_ptr(), mm=None, oo=out.data_ptr(), ss=stats.data_ptr(), w=ws, wn=wsn):
        return lib.crdr_gan_loss_fwd(ctypes.byref(d) if d is not None else None, pp, qq, mm, oo, ss, w, wn, st)

    def bwd(d, pp=p.data_ptr(), qq=q.data_ptr(), gg=g.data_ptr(), dpp=dp.data_ptr(), dqq=None, ss=stats.data_ptr(), wn=wsn):
        return lib.crdr_gan_loss_bwd(ctypes.byref(d), pp, qq, None, ss, gg, 1.0, dpp, dqq, ws, wn, st)

    def desc(**kw):
        return L.GanLossDesc(**{**dict(n=n, nq=n, kind=0, center=0, target=1.0, sgn=1.0), **kw})
    assert fwd(desc()) == 0 and bwd(desc()) == 0   # the well-formed call
    bad = {"null desc": fwd(None), "null p": fwd(desc(), pp=None), "null out": fwd(desc(), oo=None), "null stats": fwd(desc(), ss=None),
           "null workspace": fwd(desc(), w=None), "small workspace": fwd(desc(), wn=4), "n = 0": fwd(desc(n=0, nq=0)),
           "kind 3": fwd(desc(kind=3)), "kind -1": fwd(desc(kind=-1)), "hinge sgn 0.5": fwd(desc(kind=1, sgn=0.5)),
           "paired nq != n": fwd(desc(nq=n - 1)), "centred without q": fwd(desc(center=1), qq=None), "centred nq 0": fwd(desc(center=1, nq=0)),
           "center 2": fwd(desc(center=2)), "misaligned p": fwd(desc(), pp=p.data_ptr() + 2), "misaligned q": fwd(desc(), qq=q.data_ptr() + 1),
           "misaligned mask": fwd(desc(), mm=p.data_ptr() + 2), "misaligned out": fwd(desc(), oo=out.data_ptr() + 2),
           "bwd null g": bwd(desc(), gg=None), "bwd null stats": bwd(desc(), ss=None), "bwd misaligned dp": bwd(desc(), dpp=dp.data_ptr() + 2),
           "bwd dq without q": bwd(desc(nq=0), qq=None, dqq=dp.data_ptr()), "bwd small workspace": bwd(desc(), wn=4)}
    torch.cuda.synchronize()
    print({k: v for k, v in bad.items()})
    assert all(rc == -1 for rc in bad.values()), bad
    assert b"gan_loss" in lib.crdr_last_error()
    with pytest.raises(L.CrdrHipError):
        L.check(fwd(desc(kind=3)), "gan_loss_fwd")
    x = torch.zeros(8, device=dev())
    with pytest.raises(ValueError):
        HF().gan_loss_sum(x, x[:5], kind=R.BCE)                 # paired operands of different sizes
    with pytest.raises(ValueError):
        HF().gan_loss_sum(x, None, kind=R.BCE, center=True)     # nothing to centre on
    with pytest.raises(ValueError):
        HF().gan_loss_sum(x, x.double(), kind=R.BCE)            # not float32
    with pytest.raises(L.CrdrHipError):
        HF().gan_loss_sum(x, kind=7)
