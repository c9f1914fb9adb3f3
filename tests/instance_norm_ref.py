"""float64 torch restatement of the InstanceNorm op (moments per (image, channel) over H x W with the BIASED variance, optional affine,
the fused activation), for the tests to call at any shape, plus its backward written out.  `instance_norm` goes through plain autograd;
`instance_norm_backward` is the closed form the kernel implements, so the two pin each other (tests/test_multirate_disc_host.py)."""
import torch

# Input scale for a plane of TWO values (H W = 2, the smallest legal one).  There xhat = (s, -s) with s^2 = var / (var + eps), and the input
# gradient is (dz_1 - dz_2) / 2 * rstd * (1 - s^2) * (1, -1): nothing but the residue eps / (var + eps) of a cancellation.  With inputs of
# order 1 (var >> eps = 1e-5) that residue is ~1e-5 of the terms it is left over from, so float32 -- the rounding of x - mu alone, before any
# kernel runs -- resolves it to a few digits at most (torch's own float32 instance_norm on the CPU: 1e-3 of the gradient's scale), and even
# float64 only to ~1e-11.  Inputs of order sqrt(eps) make eps / (var + eps) of order one: the plane is then a well-posed check of how eps
# enters, at the gates every other shape has.
TWO_VALUE_PLANE_SCALE = 1e-2


def input_scale(shape, default=3.0):
    return TWO_VALUE_PLANE_SCALE if shape[2] * shape[3] == 2 else default


def _act(z, act, slope, mask):
    if act is None:
        return z
    neg = {"relu": 0.0, "lrelu": slope}[act]
    m = (z > 0) if mask is None else mask
    return torch.where(m, z, neg * z)


def instance_norm(x, weight=None, bias=None, eps=1e-5, act=None, slope=0.2, mask=None, dtype=torch.float64):
    """x [N,C,H,W], weight / bias [C] (or None).  `mask` (bool, z > 0 as some other implementation saw it) replaces this function's
    own activation mask, so that a gradient can be compared on the same side of every kink.  Returns (y, z)."""
    x = x.to(dtype)
    mu = x.mean(dim=(2, 3), keepdim=True)
    d = x - mu
    var = (d * d).mean(dim=(2, 3), keepdim=True)
    z = d * torch.rsqrt(var + eps)
    if weight is not None:
        z = weight.to(dtype).view(1, -1, 1, 1) * z
    if bias is not None:
        z = z + bias.to(dtype).view(1, -1, 1, 1)
    return _act(z, act, slope, mask), z


def instance_norm_backward(x, weight, bias, dy, eps=1e-5, act=None, slope=0.2, mask=None, dtype=torch.float64):
    """(dx, dweight, dbias) written out:  dz = act'(z) dy, gh = weight dz,
    dx = rstd (gh - mean_hw gh - xhat mean_hw(gh xhat)),  dweight = sum_n sum_hw dz xhat,  dbias = sum_n sum_hw dz"""
    x, dy = x.to(dtype), dy.to(dtype)
    mu = x.mean(dim=(2, 3), keepdim=True)
    d = x - mu
    rstd = torch.rsqrt((d * d).mean(dim=(2, 3), keepdim=True) + eps)
    xhat = d * rstd
    g = torch.ones(x.shape[1], dtype=dtype) if weight is None else weight.to(dtype)
    b = torch.zeros(x.shape[1], dtype=dtype) if bias is None else bias.to(dtype)
    z = g.view(1, -1, 1, 1) * xhat + b.view(1, -1, 1, 1)
    if act is None:
        dz = dy
    else:
        neg = {"relu": 0.0, "lrelu": slope}[act]
        m = (z > 0) if mask is None else mask
        dz = torch.where(m, dy, neg * dy)
    gh = g.view(1, -1, 1, 1) * dz
    dx = rstd * (gh - gh.mean(dim=(2, 3), keepdim=True) - xhat * (gh * xhat).mean(dim=(2, 3), keepdim=True))
    return dx, (dz * xhat).sum(dim=(0, 2, 3)), dz.sum(dim=(0, 2, 3))
