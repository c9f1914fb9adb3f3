"""Golden vectors of the reference's CLIC21GVAELatentConditionalDiscriminator (src/models/discriminator/clic21_gvae_discriminator.py:
53-68), same rules as gen_golden_hific.py: the reference's own class is run on seeded weights, in float64; only inputs -> outputs are
stored.  One 2 x 3 x 32 x 48 image and one 2 x 24 x 2 x 3 latent, main_ch 16, latent_nc 4; norm_type none with the three up-sampling
modes and CN with bilinear.  Per case: `out`, `dx`, the gradients of latent_conv.0.{weight,bias}, model.0.weight and the head's bias, and
the sorted state-dict keys.

    python tests/golden/gen_golden_latent_cond.py      # needs the reference checkout (gen_golden.REF); writes tests/golden/reference_latent_cond.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from seeded_weights import fill_module_, seeded_input  # noqa: E402

COMMON = dict(in_ch=3, out_ch=1, y_ch=24, latent_nc=4, main_ch=16)
X_SHAPE, Y_SHAPE = (2, 3, 32, 48), (2, 24, 2, 3)
HEAD = {"none": "model.16", "CN": "model.23"}   # the last conv as nn.Sequential numbers it


def cases():
    """(tag, constructor arguments, the recorded gradient names)"""
    out = []
    for norm, mode in (("none", "bilinear"), ("none", "bicubic"), ("none", "nearest"), ("CN", "bilinear")):
        out.append((f"{norm}.{mode}", dict(norm_type=norm, latent_interp_mode=mode, **COMMON),
                    ("latent_conv.0.weight", "latent_conv.0.bias", "model.0.weight", HEAD[norm] + ".bias")))
    return out


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def main():
    from gen_golden import REF, install_stubs
    install_stubs()
    sys.path.insert(0, REF)
    import logging
    logging.disable(logging.CRITICAL)
    from src.models.discriminator.clic21_gvae_discriminator import CLIC21GVAELatentConditionalDiscriminator
    out = {}
    x0, y0 = seeded_input("lcd.x", X_SHAPE), seeded_input("lcd.y", Y_SHAPE)
    out["x"], out["y"] = x0.numpy().astype(np.float32), y0.numpy().astype(np.float32)   # exact: the seeded inputs are float32
    for tag, kw, grads in cases():
        D = CLIC21GVAELatentConditionalDiscriminator(**kw)
        fill_module_(D, f"lcd.{tag}.")
        D.double()
        sd = D.state_dict()
        out[f"{tag}.keys"] = np.array(sorted(sd.keys()))
        out[f"{tag}.shapes"] = np.array([",".join(str(int(d)) for d in sd[k].shape) for k in sorted(sd.keys())])
        x = x0.double().requires_grad_(True)
        o = D(x, y_hat=y0.double())
        if "cot" not in out:
            out["cot"] = f64(seeded_input("lcd.cot", tuple(o.shape)))
        o.backward(torch.from_numpy(out["cot"]))
        out[f"{tag}.out"] = f64(o)
        out[f"{tag}.dx"] = f64(x.grad)
        params = dict(D.named_parameters())
        for g in grads:
            out[f"{tag}.grad.{g}"] = f64(params[g].grad)
    path = os.path.join(HERE, "reference_latent_cond.npz")
    np.savez_compressed(path, **out)
    print({k: v.shape for k, v in out.items() if not k.endswith("keys") and not k.endswith("shapes")})
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
