"""Golden vectors of the reference's Cheng20 residual blocks and of its four Cheng20 transforms, same rules as
gen_golden_hyperprior_only.py: the reference's own modules (src/models/layer/cheng_resblock.py:20-107,
src/models/subnet/autoencoder/cheng20_autoencoder.py:12-106, cheng20_interpca_autoencoder.py:16-74) are run on seeded weights, in
float64; only inputs -> outputs are stored (the inputs are regenerated from their seeds).  Stored per case: the output, dx, the
parameter gradients tests.cheng20_ref.grad_keys names (large ones as slices, tests.cheng20_ref.cut), the sorted state-dict keys, and
for the decoders the quantiles of the tensor in front of the tanh (the host test's conditioning check).

compressai is not installed and the stubs of gen_golden.install_stubs make its GDN inert, so the reference's blocks get the stand-in
below in its place: the published definition (Balle et al. 2016; y = x / sqrt(beta + gamma x^2), or times for the inverse) under
compressai's parameter and buffer names -- the ones crdr_amd/models/layer/gdn.py registers -- with the parametrizer's constants as
constants (fill_module_ overwrites the buffers).  Parity against the compressai package itself stays unpinned, as it is for oracle.gdn.

    python tests/golden/gen_golden_cheng20.py      # needs /root/reference; writes tests/golden/reference_cheng20.npz
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from seeded_weights import fill_module_, seeded_input  # noqa: E402

from tests import cheng20_ref as R  # noqa: E402

QUANTILES = (0.0, 0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 1.0)


class _Bound(torch.autograd.Function):
    """max(x, bound) whose gradient passes where x >= bound or where it would raise x (the LowerBound rule)"""

    @staticmethod
    def forward(ctx, x, bound):
        ctx.save_for_backward(x)
        ctx.bound = bound
        return x.clamp(min=bound)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return torch.where((x >= ctx.bound) | (g < 0), g, torch.zeros_like(g)), None


def _reparam_buffers(bound: float, ped: float) -> nn.Module:
    m = nn.Module()
    m.register_buffer("pedestal", torch.tensor([ped]))
    m.add_module("lower_bound", nn.Module())
    m.lower_bound.register_buffer("bound", torch.tensor([bound]))
    return m


class StandInGDN(nn.Module):
    BETA_MIN, OFFSET = 1e-6, 2.0 ** -18

    def __init__(self, in_channels, inverse=False, beta_min=1e-6, gamma_init=0.1):
        super().__init__()
        assert beta_min == self.BETA_MIN
        ped = self.OFFSET ** 2
        self.inverse = bool(inverse)
        self.beta_reparam = _reparam_buffers((self.BETA_MIN + ped) ** 0.5, ped)
        self.gamma_reparam = _reparam_buffers(self.OFFSET, ped)
        self.beta = nn.Parameter(torch.sqrt(torch.ones(in_channels) + ped))
        self.gamma = nn.Parameter(torch.sqrt(gamma_init * torch.eye(in_channels) + ped))

    def forward(self, x):
        ped = self.OFFSET ** 2
        beta = _Bound.apply(self.beta, (self.BETA_MIN + ped) ** 0.5) ** 2 - ped
        gamma = _Bound.apply(self.gamma, self.OFFSET) ** 2 - ped
        c = x.shape[1]
        norm = F.conv2d(x ** 2, gamma.reshape(c, c, 1, 1), beta)
        return x * torch.sqrt(norm) if self.inverse else x / torch.sqrt(norm)


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def record(out, tag, m, prefix, x, run):
    """fill, run, back-propagate a seeded cotangent; store output, dx, the chosen gradients and the keys"""
    fill_module_(m, prefix)
    R.seed_gdn_(m, prefix)
    m.double()
    x = x.double().requires_grad_(True)
    y = run(m, x)
    y.backward(seeded_input(prefix + "cot", tuple(y.shape)).double())
    out[f"{tag}.out"], out[f"{tag}.dx"] = f64(y), f64(x.grad)
    params = dict(m.named_parameters())
    keys = sorted(m.state_dict().keys())
    for k in R.grad_keys([k for k in keys if k in params]):
        out[f"{tag}.grad.{k}"] = f64(R.cut(params[k].grad))
    out[f"{tag}.keys"] = np.array(keys)
    return y


def main():
    from gen_golden import REF, install_stubs
    install_stubs()
    sys.modules["compressai.layers"].GDN = StandInGDN
    sys.path.insert(0, REF)
    import logging
    logging.disable(logging.CRITICAL)
    from src.models.layer import cheng_resblock
    from src.models.subnet.autoencoder import cheng20_autoencoder, cheng20_interpca_autoencoder
    assert cheng_resblock.GDN is StandInGDN
    out = {}

    for tag, (cls, args, kw, shape) in R.BLOCK_CASES.items():
        m = getattr(cheng_resblock, cls)(*args, **kw)
        y = record(out, f"block.{tag}", m, f"c20.{tag}.", seeded_input(f"c20.{tag}.x", shape), lambda m, x: m(x))
        if tag.startswith("res"):
            assert tuple(y.shape[2:]) == (5, 4)   # 3x3 s2 p1 and 1x1 s2 p0 agree on odd sides

    classes = {**vars(cheng20_autoencoder), **vars(cheng20_interpca_autoencoder)}
    for tag, (cls, kw, shape, scale, q, more_q) in R.XFORM_CASES.items():
        m = classes[cls](**kw)
        args = () if q is None else (q,)
        pre = []
        if tag in ("dec", "idec"):   # the tensor in front of the tanh: what up3 returns
            m.up3.register_forward_hook(lambda _m, _i, o: pre.append(o.detach()))
        record(out, tag, m, f"c20.{tag}.", seeded_input(f"c20.{tag}.x", shape, scale), lambda m, x: m(x, *args))
        x = seeded_input(f"c20.{tag}.x", shape, scale).double()
        for qq in more_q:
            with torch.no_grad():
                out[f"{tag}.out.q{qq:g}"] = f64(m(x, qq))
        if pre:
            t = pre[0].abs().flatten()
            out[f"{tag}.pre_tanh.abs_quantiles"] = np.stack([np.array(QUANTILES), f64(torch.quantile(t, torch.tensor(QUANTILES, dtype=t.dtype)))])
            out[f"{tag}.pre_tanh.frac_beyond_3"] = np.array(float((t > 3).double().mean()))

    path = os.path.join(HERE, "reference_cheng20.npz")
    np.savez_compressed(path, **out)
    print({k: v.shape for k, v in out.items() if not k.endswith("keys")})
    for tag in ("dec", "idec"):
        print(tag, "pre-tanh beyond |3|:", float(out[f"{tag}.pre_tanh.frac_beyond_3"]), "|x| quantiles:", out[f"{tag}.pre_tanh.abs_quantiles"][1])
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
