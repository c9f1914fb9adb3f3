"""The float64 restatements of tests/eltwise_ref.py against torch's own modules (1e-12, on the shapes the GPU tests use), and the
properties of the seeded inputs that tests/test_gpu_eltwise_direct.py relies on.  Runs without a GPU."""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import eltwise_ref as R
from tests.golden.seeded_weights import seeded_input, seeded_tensor

TOL = 1e-12


def rel_err(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-300)).item()


@pytest.mark.parametrize("n", R.REDUCE_SIZES)
def test_sums_match_torch_losses(n):
    a, b = (t.double() for t in R.reduce_pair(n))
    assert rel_err(R.l1_sum(a, b), nn.L1Loss(reduction="sum")(a, b)) <= TOL
    assert rel_err(R.sqdiff_sum(a, b), nn.MSELoss(reduction="sum")(a, b)) <= TOL
    # what the GPU tests rely on: one element in eight has a - b == 0 exactly, the rest do not
    zero = (a - b) == 0
    assert bool(zero[::8].all()) and int(zero.sum()) == (n + 7) // 8


@pytest.mark.parametrize("target", R.BCE_TARGETS)
@pytest.mark.parametrize("n", R.REDUCE_SIZES)
def test_bce_matches_torch(n, target):
    p, q = (t.double() for t in R.bce_pair(n))
    pg = p.clone().requires_grad_(True)
    ref_p = p.clone().requires_grad_(True)
    got = R.bce_diff_sum(pg, q, target)
    ref = nn.BCEWithLogitsLoss(reduction="sum")(ref_p - q, torch.full_like(p, target))
    assert rel_err(got, ref) <= TOL
    got.backward()
    ref.backward()
    # sigmoid(x) - t lies in [-1, 1] and torch forms it by that subtraction (exactly 0 at x = 46.6, t = 1, where the restatement
    # keeps -e^-x = -1e-36): absolute, on the scale 1 of the quantity
    assert (pg.grad - ref_p.grad).abs().max().item() <= TOL
    x = (p - q).float()
    if n < 255:   # no cancellation in sigmoid(x) - t for t = 0, 0.9, 1
        assert x.max().item() <= -0.5 and x.min().item() >= -6.5
    else:
        assert x.max().item() >= 100 and x.min().item() <= -100 and bool((x == 0).any())


def test_lrp_and_maxpool_are_the_stated_formulas():
    a, z = seeded_input("elt.host.a", (2, 6, 5, 3)).double(), seeded_input("elt.host.z", (2, 6, 5, 3), 20.0).double()
    # a + tanh(z) / 2 through the exponential form of tanh, and its derivative (1 - tanh^2) / 2 by autograd
    zg = z.clone().requires_grad_(True)
    y = R.lrp(a, zg)
    t = (torch.exp(2 * z) - 1) / (torch.exp(2 * z) + 1)
    assert rel_err(y, a + t / 2) <= TOL
    y.sum().backward()
    assert (zg.grad - (1 - t * t) / 2).abs().max().item() <= TOL
    assert z.abs().max().item() > 19   # tanh saturates in fp32 from |z| ~ 9
    for h, w in R.POOL_SIZES:
        x = R.pool_input(6, h, w).double()
        y = R.maxpool3s2(x)
        assert y.shape[2:] == ((h - 3) // 2 + 1, (w - 3) // 2 + 1)
        assert torch.equal(y, F.unfold(x.reshape(-1, 1, h, w), 3, stride=2).max(1).values.reshape(y.shape))


def test_maxpool_gradient_goes_to_the_first_maximum():
    """the rule the kernel states (first maximum in row-major scan order) is the rule of float64 max_pool2d on the CPU"""
    x = torch.zeros(1, 1, 5, 5, dtype=torch.float64)
    x[0, 0, 1, 1] = x[0, 0, 1, 2] = x[0, 0, 2, 0] = x[0, 0, 4, 4] = x[0, 0, 3, 3] = 7.0
    x.requires_grad_(True)
    cot = torch.tensor([[1.0, 2.0], [4.0, 8.0]], dtype=torch.float64).reshape(1, 1, 2, 2)
    R.maxpool3s2(x).backward(cot)
    want = torch.zeros(5, 5, dtype=torch.float64)
    want[1, 1] = 1.0      # window (0, 0): maxima at (1,1), (1,2), (2,0) -> the first
    want[1, 2] = 2.0      # window (0, 1) covers columns 2..4: maxima at (1,2), (3,3)
    want[2, 0] = 4.0      # window (1, 0) covers rows 2..4: only (2,0)
    want[3, 3] = 8.0      # window (1, 1): maxima at (3,3), (4,4)
    assert torch.equal(x.grad[0, 0], want)


@pytest.mark.parametrize("c", R.POOL_CHANNELS)
def test_tie_inputs_contain_ties(c):
    for h, w in R.POOL_SIZES:
        x = R.tie_input(c, h, w)
        assert set(x.unique().tolist()) <= {0.0, 1.0, 2.0}
        frac = R.window_ties(x)
        assert frac > 0.5, (c, h, w, frac)
        cot = R.int_cotangent("host.cot", (2, c, (h - 3) // 2 + 1, (w - 3) // 2 + 1))
        assert cot.min().item() >= 1 and cot.max().item() <= 4 and torch.equal(cot, cot.round())


@pytest.mark.parametrize("shape", R.LPIPS_SHAPES)
def test_lpips_restatement_and_inputs(shape):
    f0, f1, lin, g = R.lpips_inputs(*shape)
    f0, f1, lin = f0.double(), f1.double(), lin.double()
    # the published form: normalize_tensor (eps 1e-10 added to the norm), squared difference, 1x1 `lin` conv, spatial average
    n0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + 1e-10)
    ref = F.conv2d((n0 - n1) ** 2, lin.reshape(1, -1, 1, 1)).mean((2, 3)).reshape(-1)
    assert rel_err(R.lpips_layer(f0, f1, lin), ref) <= TOL
    # no all-zero pixel in either operand, positive weights and cotangents
    assert f0.abs().sum(1).min().item() > 0 and f1.abs().sum(1).min().item() > 0
    assert lin.min().item() > 0 and g.min().item() > 0


def test_lpips_gradient_is_nan_at_an_all_zero_f1_pixel():
    """why the parity cases avoid it: d sqrt(s) / ds is infinite at s = 0 and is multiplied by 0"""
    f0, f1, lin, _ = (t.double() for t in R.lpips_inputs(1, 6, 1, 3))
    f1[0, :, 0, 1] = 0
    f1.requires_grad_(True)
    v = R.lpips_layer(f0, f1, lin)
    assert bool(torch.isfinite(v).all())
    v.sum().backward()
    assert bool(torch.isnan(f1.grad[0, :, 0, 1]).all()) and bool(torch.isfinite(f1.grad[0, :, 0, 0]).all())
    # an all-zero f0 pixel is harmless: f0 takes no gradient and 0 / (0 + 1e-10) = 0
    f0[0, :, 0, 2] = 0
    assert bool(torch.isfinite(R.lpips_layer(f0, f1.detach(), lin)).all())


SN_SHAPES = [(1, 7, 1), (5, 3, 1), (64, 3, 4), (130, 1030, 1)]   # (out, in, kernel): weight matrices 1x7, 5x3, 64x48, 130x1030


@pytest.mark.parametrize("o,i,k", SN_SHAPES)
def test_spectral_norm_matches_torch(o, i, k):
    conv = nn.Conv2d(i, o, k).double()
    with torch.no_grad():
        conv.weight.copy_(seeded_tensor(f"elt.sn.w{o}x{i * k * k}", conv.weight.shape).double())
    m = torch.nn.utils.spectral_norm(conv)
    w = m.weight_orig.detach().clone()
    u, v = m.weight_u.detach().clone(), m.weight_v.detach().clone()
    x = seeded_input("elt.sn.x", (1, i, k, k)).double()
    m.train()
    for _ in range(2):   # two training calls: u, v carry over
        m(x)
        w_sn, sigma, u, v = R.spectral_norm(w, u, v, True)
        assert rel_err(w_sn, m.weight) <= TOL and rel_err(u, m.weight_u) <= TOL and rel_err(v, m.weight_v) <= TOL
        assert rel_err(sigma * w_sn, w) <= TOL
    m.eval()
    m(x)
    w_sn, sigma, u2, v2 = R.spectral_norm(w, u, v, False)
    assert rel_err(w_sn, m.weight) <= TOL
    assert torch.equal(u2, u) and torch.equal(v2, v) and torch.equal(m.weight_u, u) and torch.equal(m.weight_v, v)
    # gradient: u, v are constants
    m.train()
    cot = seeded_input("elt.sn.cot", w.shape).double()
    m(x)   # the third power iteration
    (m.weight * cot).sum().backward()
    wr = w.clone().requires_grad_(True)
    (R.spectral_norm(wr, u, v, True)[0] * cot).sum().backward()
    assert rel_err(wr.grad, m.weight_orig.grad) <= TOL


@pytest.mark.parametrize("q", [0.0, 0.25, 2.0, 3.5, 4.0])
def test_interp_vectors_oracle_takes_float64(q):
    from oracle import crdr_oracle as O
    W = seeded_tensor("elt.ica.w", (5, 1, 9, 1, 1)).double() * 8
    B = seeded_tensor("elt.ica.b", (5, 1, 9, 1, 1)).double()
    s, t = O.interp_ca_vectors(W, B, q)
    assert s.dtype == torch.float64 and t.dtype == torch.float64
    l = math.floor(q)
    r = min(l + 1, 4)
    w = W[l] * (r - q) + W[r] * (1 - (r - q))
    assert rel_err(s.reshape(-1), torch.log1p(torch.exp(w)).reshape(-1)) <= 1e-8   # softplus is the identity above 20: e^-20 = 2e-9
    assert rel_err(t.reshape(-1), (B[l] * (r - q) + B[r] * (1 - (r - q))).reshape(-1)) <= TOL
