"""Float64 restatements of the loss, LPIPS and spectral-norm ops of csrc/eltwise.hip, and the seeded inputs the direct tests feed them.

Plain torch on the CPU, differentiable by autograd; nothing here is shaped like a kernel.  tests/test_eltwise_ref_host.py ties each
restatement to torch's own module at 1e-12 and checks the properties of the inputs that tests/test_gpu_eltwise_direct.py relies on
(ties, exact zeros, no all-zero pixel).  Spectral norm and the interpolated channel-attention vectors are restated by the oracle
(oracle.crdr_oracle.spectral_norm_weight / interp_ca_vectors, generic in the dtype); `spectral_norm` below only wraps the former."""
import torch
import torch.nn.functional as F

from tests.golden.seeded_weights import seeded_input

# ---- restatements ------------------------------------------------------------------------------------------------------------------


def lrp(a, z):
    return a + 0.5 * torch.tanh(z)


def sqdiff_sum(a, b):
    return (a - b).square().sum()


def l1_sum(a, b):
    return (a - b).abs().sum()


def bce_terms(x, target: float):
    """BCEWithLogits(x, t) = t softplus(-x) + (1 - t) softplus(x), elementwise: no cancellation for t in [0, 1], derivative
    sigmoid(x) - t everywhere (softplus as logaddexp(0, .), accurate for large |x|)"""
    zero = torch.zeros_like(x)
    return target * torch.logaddexp(zero, -x) + (1 - target) * torch.logaddexp(zero, x)


def bce_diff_sum(p, q, target: float):
    return bce_terms(p - q, target).sum()


def maxpool3s2(x):
    """3x3 windows, stride 2, no padding; autograd sends a window's gradient to its first maximum in row-major scan order"""
    return F.max_pool2d(x, 3, 2)


def lpips_layer(f0, f1, lin):
    """per image: spatial mean of sum_c lin_c (f0_c / (|f0| + 1e-10) - f1_c / (|f1| + 1e-10))^2, |.| the norm over channels"""
    n0 = f0 / (f0.square().sum(1, keepdim=True).sqrt() + 1e-10)
    n1 = f1 / (f1.square().sum(1, keepdim=True).sqrt() + 1e-10)
    return (lin.reshape(1, -1, 1, 1) * (n0 - n1).square()).sum(1).mean((1, 2))


def spectral_norm(w, u, v, training: bool, eps: float = 1e-12):
    """-> (w / sigma, sigma, u', v') of torch.nn.utils.spectral_norm's one power iteration (none in eval); u', v' are constants"""
    from oracle import crdr_oracle as O
    w_sn, u2, v2 = O.spectral_norm_weight({"m.weight_orig": w, "m.weight_u": u, "m.weight_v": v}, "m", training, eps)
    sigma = torch.dot(u2, torch.mv(w.detach().reshape(w.shape[0], -1), v2))
    return w_sn, sigma, u2, v2


# ---- seeded inputs (float32, CPU, NCHW) ---------------------------------------------------------------------------------------------

POOL_SIZES = [(3, 3), (4, 4), (8, 6), (15, 15), (7, 9)]
POOL_CHANNELS = [64, 192, 6, 3]
# (N, C, H, W): HW = 1, 3, 9, 225, 300 (> 4 x 64: the forward's pixel loop strides), 1056 (> 4 x 256: the backward's does)
LPIPS_SHAPES = [(1, 20, 1, 1), (3, 64, 1, 1), (1, 6, 1, 3), (3, 100, 1, 3), (3, 20, 3, 3), (1, 192, 3, 3), (3, 64, 15, 15), (1, 100, 15, 15),
                (1, 192, 15, 15), (3, 6, 15, 15), (3, 6, 15, 20), (1, 64, 15, 20), (3, 20, 20, 15), (1, 8, 32, 33), (3, 8, 33, 32)]
REDUCE_SIZES = [1, 255, 256, 257, 1023, 1025, 2 ** 20 + 3]
BCE_TARGETS = [0.0, 1.0, 0.9]


def pool_input(c, h, w, n=2):
    return seeded_input(f"elt.pool.x{c}.{h}x{w}", (n, c, h, w), 3.0)


def tie_input(c, h, w, n=2):
    """values in {0, 1, 2} (post-ReLU style): most 3x3 windows hold their maximum more than once"""
    return torch.floor((seeded_input(f"elt.pool.tie{c}.{h}x{w}", (n, c, h, w)) + 1) * 1.5).clamp_(0, 2)


def int_cotangent(tag, shape):
    """integers 1..4: sums of up to four of them are exact in fp32"""
    return torch.floor((seeded_input(tag, shape) + 1) * 2).clamp_(0, 3) + 1


def window_ties(x):
    """fraction of the 3x3 stride-2 windows of x whose maximum occurs more than once"""
    p = F.unfold(x.double().reshape(-1, 1, x.shape[2], x.shape[3]), 3, stride=2)   # [N C, 9, windows]
    return ((p == p.max(1, keepdim=True).values).sum(1) > 1).double().mean().item()


def lpips_inputs(n, c, h, w):
    f0 = seeded_input(f"elt.lpips.f0.{n}x{c}x{h}x{w}", (n, c, h, w), 2.0)
    f1 = seeded_input(f"elt.lpips.f1.{n}x{c}x{h}x{w}", (n, c, h, w), 2.0)
    lin = seeded_input(f"elt.lpips.lin{c}", (c,)).abs() + 0.01   # the trained LPIPS weights are non-negative
    g = seeded_input(f"elt.lpips.g{n}", (n,)) + 1.5
    return f0, f1, lin, g


def reduce_pair(n):
    """a, b for sqdiff_sum / l1_sum: every eighth element has a == b exactly"""
    a = seeded_input(f"elt.red.a{n}", (n,), 2.0)
    b = seeded_input(f"elt.red.b{n}", (n,), 2.0)
    b[::8] = a[::8]
    return a, b


def bce_pair(n):
    """logits whose difference x spans +-100.  The few elements of the sizes below 255 (n = 1) cannot span anything, and their gradient
    sigmoid(x) - t is measured against its own magnitude alone: they get x in [-6.5, -0.5], where that difference does not cancel for any
    of the targets (sigmoid(x) in [0.0015, 0.38] against t = 0, 0.9 or 1; for t = 0 it is 1 / (1 + e^-x) itself), so that the case
    measures the kernel and not the 2^-24 absolute resolution of a difference of O(1) numbers.  Saturation and cancellation are
    exercised from n = 255 up, where the tensor holds elements of magnitude ~1 to be measured against."""
    if n < 255:
        p = -0.5 - 3.0 * seeded_input(f"elt.bce.p{n}", (n,)).abs()
        q = 3.0 * seeded_input(f"elt.bce.q{n}", (n,)).abs()
        return p, q
    p = seeded_input(f"elt.bce.p{n}", (n,), 50.0)
    q = seeded_input(f"elt.bce.q{n}", (n,), 50.0)
    p[:4] = torch.tensor([50.0, -50.0, 0.25, 0.0])
    q[:4] = torch.tensor([-50.0, 50.0, 0.25, 0.0])
    return p, q


def layout_pair(c):
    a = seeded_input(f"elt.layout.a{c}", (2, c, 5, 3), 2.0)
    b = seeded_input(f"elt.layout.b{c}", (2, c, 5, 3), 2.0)
    return a, b
