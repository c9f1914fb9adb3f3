"""Test-side restatement of what the hyperprior-only models add to the oracle: the Cheng20 hyper-transforms, the three ELIC decoders
with sub-pixel up-sampling, and the three models' forward.  A composition of oracle.crdr_oracle functions (imported, not edited) with
torch ops; tests/test_hyperprior_only_host.py holds it, in float64, to vectors recorded from the reference's own modules
(tests/golden/reference_hyperprior_only.npz), and the GPU tests compare the HIP modules against it."""
import torch
import torch.nn.functional as F

from oracle import crdr_oracle as O

CA = dict(actv="softplus", use_interp=True, use_bias=True)
# the fixture's decoder (tests/golden/gen_golden_hyperprior_only.py); use_pi / L / max_beta / ca_kwargs are the shipped configs' values
DEC_KW = dict(in_ch=16, out_ch=3, main_ch=24, block_mid_ch=12, pixel_shuffle=True, use_tanh=False)
COND_KW = dict(rate_level=5, ca_kwargs=CA)
BETA_KW = dict(L=10, max_beta=5.12, cond_ch=32, use_pi=False, weight_init=False)
DEC_CASES = {   # name -> (class name, constructor kwargs, q, beta)
    "plain": ("ElicDecoder", DEC_KW, None, None),
    "interp": ("ElicInterpCaDecoder", {**DEC_KW, **COND_KW}, 1.5, None),
    "beta": ("ElicInterpCaBetaCondDecoder", {**DEC_KW, **COND_KW, **BETA_KW}, 1.5, 3.84),
}
HE_KW = dict(in_ch=320, out_ch=192, main_ch=192)
HD_KW = dict(in_ch=192, out_ch=640, main_ch=192)
HE_GRADS = ("c1.0.weight", "c3.0.weight", "c5.bias")
HD_GRADS = ("c2.0.weight", "c5.weight")
DEC_GRADS = ("conv1.0.weight", "conv4.0.bias", "interp_ca_list.3.weight")


def cut(g):
    """the slice of a large gradient the fixture keeps: first 8 input channels, then first 32 output channels"""
    if g.numel() > 4096 and g.ndim == 4:
        g = g[:, :8]
        if g.numel() > 4096:
            g = g[:32]
    return g


def _lrelu(x):
    return F.leaky_relu(x, 0.2)


def hyper_encoder(sd, y, p="hyperencoder"):
    """Cheng20HyperEncoder.forward (cheng20_hyperprior.py:22-40)"""
    x = y
    for name, s in (("c1", 1), ("c2", 1), ("c3", 2), ("c4", 1)):
        x = _lrelu(O.conv(sd, f"{p}.{name}.0", x, stride=s, pad=1))
    return O.conv(sd, p + ".c5", x, stride=2, pad=1)


def hyper_decoder(sd, z_hat, p="hyperdecoder"):
    """Cheng20HyperDecoder.forward (cheng20_hyperprior.py:43-59)"""
    x = _lrelu(O.conv(sd, p + ".c1.0", z_hat, pad=1))
    x = _lrelu(O.convT(sd, p + ".c2.0", x, stride=2, pad=1, out_pad=0))
    x = _lrelu(O.conv(sd, p + ".c3.0", x, pad=1))
    x = _lrelu(O.convT(sd, p + ".c4.0", x, stride=2, pad=1, out_pad=0))
    return O.conv(sd, p + ".c5", x, pad=1)


def decoder_ps(sd, y_hat, q=None, beta=None, p="decoder", max_beta=5.12, L=10):
    """O.decoder with up_conv(pixel_shuffle=True): Conv2d(in, 4 out, 5, padding=2) under key `.0`, then PixelShuffle(2) (elic_layers.py:16-20)"""
    cond = None
    if beta is not None:
        e = O.fourier_embed(beta, L=L, max_beta=max_beta).to(y_hat.dtype)
        h = F.relu(F.linear(e, sd[p + ".mlp.0.weight"], sd[p + ".mlp.0.bias"]))
        cond = F.linear(h, sd[p + ".mlp.2.weight"], sd[p + ".mlp.2.bias"]).reshape(1, -1, 1, 1)
    x = y_hat
    for i, name in enumerate(O.DEC_LAYERS):
        if q is not None:
            x = O.interp_ca(sd, f"{p}.interp_ca_list.{i}", x, q)
        if name.startswith("conv"):
            x = F.pixel_shuffle(O.conv(sd, f"{p}.{name}.0", x, pad=2), 2)
        elif name.startswith("block"):
            x = O.res_blocks(sd, f"{p}.{name}", x, cond)
        else:
            x = O.nlam(sd, f"{p}.{name}", x)
    return x


def model_forward(sd, x, q=None, beta=None, noise_y=None, noise_z=None, is_train=True, forced=None, report=None, pixel_shuffle=False):
    """{Hyperprior, InterpCaHyperprior, BetaCondInterpCaHyperprior}Model.forward + get_rate_summary_dict (hyperprior_model.py:60-118):
    O._generator_forward with the Cheng20 hyper-transforms and the Gaussian conditional on the hyper-decoder's (mean | scale) in the
    Charm's place.  forced = {"z": symbols, "y": symbols} of another implementation (O.forced_round)."""
    _, _, H, W = x.shape
    y = O.encoder(sd, x, q)
    z = hyper_encoder(sd, y)
    fz = None if forced is None else forced["z"]
    fy = None if forced is None else forced["y"]
    z_hat, z_lik = O.entropy_bottleneck(sd, "entropy_model_z", z, noise_z if is_train else None, forced=fz, report=report)
    hyper = hyper_decoder(sd, z_hat)
    mu, sigma = torch.chunk(hyper, 2, 1)
    y_hat, y_lik = O.gaussian_conditional(y, mu, sigma, noise_y if is_train else None, forced=fy, report=report)
    fake = (decoder_ps if pixel_shuffle else O.decoder)(sd, y_hat, q, beta)
    if not is_train:
        fake = fake.clamp(-1, 1)
    with torch.no_grad():
        y_qlik = O.gaussian_conditional(y, mu, sigma, None, forced=fy)[1]
        z_qlik = O.entropy_bottleneck(sd, "entropy_model_z", z, None, forced=fz)[1]
    bpp = (O.bits_per_image(y_lik) + O.bits_per_image(z_lik)) / (H * W)
    qbpp = (O.bits_per_image(y_qlik) + O.bits_per_image(z_qlik)) / (H * W)
    return dict(fake_images=fake, y=y, z=z, y_hat=y_hat, z_hat=z_hat, bpp=bpp, qbpp=qbpp, hyper_out=hyper)
