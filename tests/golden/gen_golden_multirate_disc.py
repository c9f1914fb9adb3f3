"""Golden vectors of the reference's four rate-aware discriminators (src/models/discriminator/multirate_clic21_gvae_discriminator.py:
122-283), same rules as gen_golden_channel_norm.py: the reference's own classes are run on seeded weights, in float64; only inputs ->
outputs are stored.  Every class with norm_type none and IN, img_size 32 and main_ch 8 (backbone + head depth 3, the limit of
build_channel_dict at 32), three rates, `use_rate_ind_cond` both ways where the class has it, one 2 x 3 x 32 x 48 input, rate_ind 0 and 2.
Per run: `out`, `dx`, three named parameter gradients (small tensors, from both ends of the net); per case the sorted state-dict keys.
The input gradients are the bulk of the file -- 24 runs x 9216 values -- and are stored, like the parameter gradients, rounded to
float32 (6e-8 of their scale, against gates of 2e-5 and 5e-5), which is what keeps the file under the size limit for a committed file
(the 24 input gradients alone are 0.88 MB in float32); the outputs are float64.

    python tests/golden/gen_golden_multirate_disc.py      # needs the reference checkout (gen_golden.REF); writes tests/golden/reference_multirate_disc.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from seeded_weights import fill_module_, seeded_input  # noqa: E402

COMMON = dict(img_size=32, main_ch=8)
RATES = (0, 2)
NORMS = ("none", "IN")
X_SHAPE = (2, 3, 32, 48)


def cases():
    """(tag, class name, constructor arguments, the three gradient names with {q} for the rate index)"""
    out = []
    for norm in NORMS:
        for cond in (False, True):
            out.append((f"sb.{norm}.c{int(cond)}", "SharedBackboneClic21GvaeDiscriminator",
                        dict(num_head=3, norm_type=norm, backbone_depth=2, head_depth=1, use_rate_ind_cond=cond, **COMMON),
                        ("backbone.b32.0.0.weight", "head_list.{q}.last_conv.weight", "head_list.{q}.last_conv.bias")))
            out.append((f"sh.{norm}.c{int(cond)}", "SharedHeadClic21GvaeDiscriminator",
                        dict(num_backbone=3, norm_type=norm, backbone_depth=1, head_depth=2, use_rate_ind_cond=cond, **COMMON),
                        ("backbone_list.{q}.b32.1.0.weight", "head.block.b16.0.0.weight", "head.last_conv.weight")))
        out.append((f"sep.{norm}", "MultirateSeparateClic21GvaeDiscriminator", dict(rate_level=3, norm_type=norm, depth=3, **COMMON),
                    ("discriminator_list.{q}.block.b32.0.0.weight", "discriminator_list.{q}.block.b32.1.0.weight",
                     "discriminator_list.{q}.last_conv.weight")))
        out.append((f"src.{norm}", "MultirateSharedRateCondClic21GvaeDiscriminator", dict(rate_level=3, norm_type=norm, depth=3, **COMMON),
                    ("net.block.b32.0.0.weight", "net.block.b32.1.0.weight", "net.last_conv.bias")))
    return out


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def f32(t):
    return t.detach().cpu().numpy().astype(np.float32)


def main():
    from gen_golden import REF, install_stubs
    install_stubs()
    sys.path.insert(0, REF)
    import logging
    logging.disable(logging.CRITICAL)
    from src.models.discriminator import multirate_clic21_gvae_discriminator as M
    out = {}
    x0 = seeded_input("mrd.x", X_SHAPE)
    out["x"] = f32(x0)   # exact: the seeded input is float32
    for tag, cls, kw, grads in cases():
        D = getattr(M, cls)(**kw)
        fill_module_(D, f"mrd.{tag}.")
        D.double()
        out[f"{tag}.keys"] = np.array(sorted(D.state_dict().keys()))
        for q in RATES:
            D.zero_grad(set_to_none=True)
            x = x0.double().requires_grad_(True)
            o = D(x, rate_ind=torch.tensor([float(q)]))
            if "cot" not in out:
                out["cot"] = f64(seeded_input("mrd.cot", tuple(o.shape)))
            assert tuple(o.shape) == out["cot"].shape, (tag, o.shape)
            o.backward(torch.from_numpy(out["cot"]))
            out[f"{tag}.q{q}.out"] = f64(o)
            out[f"{tag}.q{q}.dx"] = f32(x.grad)
            params = dict(D.named_parameters())
            for g in grads:
                name = g.format(q=q)
                out[f"{tag}.q{q}.grad.{name}"] = f32(params[name].grad)

    path = os.path.join(HERE, "reference_multirate_disc.npz")
    np.savez_compressed(path, **out)
    print({k: v.shape for k, v in out.items() if not k.endswith("keys")})
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
