"""Golden vectors of the reference's Cheng20 hyper-transforms and of its three ELIC decoders with `pixel_shuffle=True`, same rules as
gen_golden_hific.py: the reference's own modules (src/models/subnet/hyperprior/cheng20_hyperprior.py:22-59,
src/models/layer/elic_layers.py:14-21, src/models/subnet/autoencoder/elic_autoencoder.py:76-119, elic_interpca_autoencoder.py:60-97,
elic_interpca_beta_cond_autoencoder.py:88-162) are run on seeded weights, in float64; only inputs -> outputs are stored (the inputs
themselves are regenerated from their seeds).  Large gradients are stored as slices (tests.hyperprior_only_ref.cut).

The reference's three hyperprior-only model classes need compressai, which the stubs only imitate: their key schema is pinned through
these parts and the Charm models' fixtures.

    python tests/golden/gen_golden_hyperprior_only.py      # needs /root/reference; writes tests/golden/reference_hyperprior_only.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from seeded_weights import fill_module_, seeded_input  # noqa: E402

from tests import hyperprior_only_ref as R  # noqa: E402


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def main():
    from gen_golden import REF, install_stubs
    install_stubs()
    sys.path.insert(0, REF)
    import logging
    logging.disable(logging.CRITICAL)
    from src.models.subnet.autoencoder import elic_autoencoder, elic_interpca_autoencoder, elic_interpca_beta_cond_autoencoder
    from src.models.subnet.hyperprior.cheng20_hyperprior import Cheng20HyperDecoder, Cheng20HyperEncoder
    out = {}

    # (1) hyper-transforms
    for tag, m, shape, grads in (("he", Cheng20HyperEncoder(**R.HE_KW), (2, 320, 8, 4), R.HE_GRADS),
                                 ("hd", Cheng20HyperDecoder(**R.HD_KW), (2, 192, 2, 1), R.HD_GRADS)):
        fill_module_(m, f"ho.{tag}.")
        m.double()
        x = seeded_input(f"ho.{tag}.x", shape, 2.0).double().requires_grad_(True)
        y = m(x)
        y.backward(seeded_input(f"ho.{tag}.cot", tuple(y.shape)).double())
        out[f"{tag}.out"], out[f"{tag}.dx"] = f64(y), f64(x.grad)
        params = dict(m.named_parameters())
        for k in grads:
            out[f"{tag}.grad.{k}"] = f64(R.cut(params[k].grad))
        out[f"{tag}.keys"] = np.array(sorted(m.state_dict().keys()))

    # (2) decoders with sub-pixel up-sampling
    classes = {"ElicDecoder": elic_autoencoder.ElicDecoder, "ElicInterpCaDecoder": elic_interpca_autoencoder.ElicInterpCaDecoder,
               "ElicInterpCaBetaCondDecoder": elic_interpca_beta_cond_autoencoder.ElicInterpCaBetaCondDecoder}
    for tag, (cls, kw, q, beta) in R.DEC_CASES.items():
        m = classes[cls](**kw)
        fill_module_(m, f"ho.dec.{tag}.")
        m.double()
        if beta is not None:   # the Fourier features are float32 by construction: hand them to the float64 MLP as they are
            embed = m.embed.embed
            m.embed.embed = lambda b: embed(b).double()
        x = seeded_input("ho.dec.x", (2, 16, 3, 2), 3.0).double().requires_grad_(True)
        args = () if q is None else ((q,) if beta is None else (q, beta))
        y = m(x, *args)
        assert tuple(y.shape) == (2, 3, 48, 32)
        y.backward(seeded_input("ho.dec.cot", tuple(y.shape)).double())
        out[f"dec.{tag}.out"], out[f"dec.{tag}.dx"] = f64(y), f64(x.grad)
        params = dict(m.named_parameters())
        for k in R.DEC_GRADS:
            if k in params:
                out[f"dec.{tag}.grad.{k}"] = f64(R.cut(params[k].grad))
        out[f"dec.{tag}.keys"] = np.array(sorted(m.state_dict().keys()))
        # ... and the transposed-conv form of the same decoder, which the sub-pixel form must leave alone
        out[f"dec.{tag}.keys_convt"] = np.array(sorted(classes[cls](**{**kw, "pixel_shuffle": False}).state_dict().keys()))

    path = os.path.join(HERE, "reference_hyperprior_only.npz")
    np.savez_compressed(path, **out)
    print({k: v.shape for k, v in out.items() if not k.endswith("keys")})
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
