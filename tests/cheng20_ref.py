"""Test-side float64 restatement of the Cheng20 residual blocks (src/models/layer/cheng_resblock.py:20-107) and of the four Cheng20
transforms (cheng20_autoencoder.py:12-106, cheng20_interpca_autoencoder.py:16-74): a composition of oracle.crdr_oracle functions
(conv, nlam, interp_ca, gdn -- imported, not edited) with torch ops.  tests/test_cheng20_host.py holds it to vectors recorded from the
reference's own modules (tests/golden/reference_cheng20.npz); the GPU tests compare the HIP modules against it.

GDN parameters are not filled by seeded_tensor -- its generic values give half the stored beta a negative sign, far below the
parametrizer's bound -- but by seed_gdn_: gamma = sqrt(0.02 U + 2^-36), beta = sqrt(U + 0.5) from a generator seeded with
crc32(prefix + name), with gamma[0, :3] = 0 and beta[1] = 0 stored BELOW their bounds so that the LowerBound rule is exercised."""
import zlib

import torch
import torch.nn.functional as F

from oracle import crdr_oracle as O

CA = dict(actv="softplus", use_interp=True, use_bias=True)
COND_KW = dict(rate_level=5, ca_kwargs=CA)
ENC_LAYERS = ("block1", "block2", "block3", "nlam1", "block4", "block5", "block6", "conv7", "nlam2")
DEC_LAYERS = ("nlam0", "block0", "up0", "block1", "up1", "nlam2", "block2", "up2", "block3", "up3")
DOWN = ("block1", "block3", "block5")    # the encoder's ResBlocks with downscale=True, actv2='gdn'

# block cases of the fixture: tag -> (class name, positional arguments, keyword arguments, input shape)
BLOCK_CASES = {
    "res24": ("ResBlock", (24, 24), dict(actv="lrelu", actv2="gdn", downscale=True), (2, 24, 9, 7)),
    "res3": ("ResBlock", (3, 24), dict(actv="lrelu", actv2="gdn", downscale=True), (2, 3, 9, 7)),
    "up24": ("UpResBlock", (24, 24), dict(actv="lrelu", actv2="igdn"), (2, 24, 5, 3)),
}
# transform cases: tag -> (class name, keyword arguments, input shape, input scale, rate index of the gradients, further forward-only q)
# Decoder inputs have scale 0.3: the IGDN stack amplifies, and at the scale 3.0 of the other decoder fixtures the reference's output
# was +-1 almost everywhere (86 - 89 % of the pre-tanh values beyond |3|)
XFORM_CASES = {
    "enc": ("Cheng20Encoder", dict(in_ch=3, out_ch=16, main_ch=24), (2, 3, 48, 32), 1.0, None, ()),
    "dec": ("Cheng20Decoder", dict(in_ch=16, out_ch=3, main_ch=24, use_tanh=True), (2, 16, 3, 2), 0.3, None, ()),
    "ienc": ("Cheng20InterpCaEncoder", dict(in_ch=3, out_ch=24, main_ch=24, **COND_KW), (2, 3, 48, 32), 1.0, 1.5, (0.0, 4.0)),
    "idec": ("Cheng20InterpCaDecoder", dict(in_ch=24, out_ch=3, main_ch=24, use_tanh=True, **COND_KW), (2, 24, 3, 2), 0.3, 1.5, (0.0, 4.0)),
}


def cut(g):
    """the slice of a large gradient the fixture keeps: first 8 input channels, then first 32 output channels"""
    if g.numel() > 4096 and g.ndim == 4:
        g = g[:, :8]
        if g.numel() > 4096:
            g = g[:32]
    return g


def gdn_values(key: str, shape) -> torch.Tensor:
    """the stored value of one GDN parameter (`key` ends in .beta or .gamma), float32"""
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()) % (2 ** 31))
    u = torch.rand(tuple(shape), generator=g)
    if key.endswith(".gamma"):
        v = torch.sqrt(0.02 * u + 2.0 ** -36)
        v[0, :3] = 0.0
    else:
        v = torch.sqrt(u + 0.5)
        v[1] = 0.0
    return v


def seed_gdn_(module_or_sd, prefix: str = ""):
    """Overwrite the beta / gamma of every GDN in a module (children with `beta_reparam` and `gamma`; names are prefixed with `prefix`) or
    in a state dict (every `X.beta` / `X.gamma` pair; the keys carry their prefix already).  Values depend on the full name and the shape
    only.  Returns what it was given."""
    if isinstance(module_or_sd, dict):
        stems = {k.rsplit(".", 1)[0] for k in module_or_sd if k.endswith(".gamma")}
        for k in [s + leaf for s in sorted(stems) if s + ".beta" in module_or_sd for leaf in (".beta", ".gamma")]:
            t = module_or_sd[k]
            v = gdn_values(k, t.shape).to(t.dtype)
            module_or_sd[k] = v.requires_grad_(True) if t.requires_grad else v
        return module_or_sd
    with torch.no_grad():
        for name, m in module_or_sd.named_modules():
            if hasattr(m, "beta_reparam") and hasattr(m, "gamma"):
                for leaf in ("beta", "gamma"):
                    p = getattr(m, leaf)
                    p.copy_(gdn_values(f"{prefix}{name}.{leaf}" if name else prefix + leaf, p.shape).to(p.dtype))
    return module_or_sd


def _lrelu(x):
    return F.leaky_relu(x, 0.2)


def res_block(sd, p, x, actv2="lrelu", downscale=False):
    """ResBlock.forward with actv='lrelu' (cheng_resblock.py:49-64); the 1x1 shortcut exists iff its key does"""
    s = 2 if downscale else 1
    shortcut = O.conv(sd, p + ".shortcut", x, stride=s) if p + ".shortcut.weight" in sd else x
    y = _lrelu(O.conv(sd, p + ".conv1", x, stride=s, pad=1))
    y = O.conv(sd, p + ".conv2", y, pad=1)
    if actv2 == "lrelu":
        y = _lrelu(y)
    elif actv2 in ("gdn", "igdn"):
        y = O.gdn(sd, p + ".actv2", y, inverse=(actv2 == "igdn"))
    return y + shortcut


def up_res_block(sd, p, x, actv2="igdn"):
    """UpResBlock.forward with actv='lrelu', up_type='pixelshuffle' (cheng_resblock.py:82-107)"""
    shortcut = F.pixel_shuffle(O.conv(sd, p + ".shortcut.0", x), 2)
    y = _lrelu(F.pixel_shuffle(O.conv(sd, p + ".c1.0", x, pad=1), 2))
    y = O.conv(sd, p + ".c1.3", y, pad=1)
    if actv2 in ("gdn", "igdn"):
        y = O.gdn(sd, p + ".c1.4", y, inverse=(actv2 == "igdn"))
    return y + shortcut


def block(sd, p, x, tag):
    cls, _, kw, _ = BLOCK_CASES[tag]
    if cls == "ResBlock":
        return res_block(sd, p, x, actv2=kw["actv2"], downscale=kw["downscale"])
    return up_res_block(sd, p, x, actv2=kw["actv2"])


def _enc_layer(sd, p, name, x):
    if name.startswith("block"):
        return res_block(sd, f"{p}.{name}", x, *(("gdn", True) if name in DOWN else ("lrelu", False)))
    if name.startswith("nlam"):
        return O.nlam(sd, f"{p}.{name}", x)
    return O.conv(sd, f"{p}.{name}", x, stride=2, pad=1)   # conv7


def encoder(sd, x, q=None, p="encoder"):
    """Cheng20Encoder.forward; with q, InterpChAtt AFTER each of the nine stages (cheng20_interpca_autoencoder.py:36-41)"""
    for i, name in enumerate(ENC_LAYERS):
        x = _enc_layer(sd, p, name, x)
        if q is not None:
            x = O.interp_ca(sd, f"{p}.interp_ca_list.{i}", x, q)
    return x


def decoder(sd, y_hat, q=None, p="decoder", use_tanh=True, pre_tanh=None):
    """Cheng20Decoder.forward; with q, InterpChAtt BEFORE each of the ten stages (cheng20_interpca_autoencoder.py:67-74).  `pre_tanh`: a
    list that receives the tensor in front of the tanh."""
    x = y_hat
    for i, name in enumerate(DEC_LAYERS):
        if q is not None:
            x = O.interp_ca(sd, f"{p}.interp_ca_list.{i}", x, q)
        if name.startswith("block"):
            x = res_block(sd, f"{p}.{name}", x)
        elif name.startswith("nlam"):
            x = O.nlam(sd, f"{p}.{name}", x)
        elif name == "up3":
            x = F.pixel_shuffle(O.conv(sd, f"{p}.up3.0", x, pad=1), 2)
        else:
            x = up_res_block(sd, f"{p}.{name}", x)
    if pre_tanh is not None:
        pre_tanh.append(x.detach())
    return torch.tanh(x) if use_tanh else x


def transform(sd, x, tag, q=None, p=None, pre_tanh=None):
    p = p or f"c20.{tag}"
    if tag in ("enc", "ienc"):
        return encoder(sd, x, q, p)
    return decoder(sd, x, q, p, use_tanh=XFORM_CASES[tag][1]["use_tanh"], pre_tanh=pre_tanh)


def grad_keys(keys):
    """the parameter gradients the fixture keeps of a module with state-dict keys `keys`: every GDN parameter, every shortcut, every
    InterpChAtt tensor, and the first and last conv weight"""
    keys = sorted(keys)
    ks = [k for k in keys if k.endswith((".beta", ".gamma")) or "shortcut" in k or "interp_ca_list" in k]
    convs = [k for k in keys if k.endswith(".weight") and "interp_ca_list" not in k and "shortcut" not in k]
    return sorted(set(ks + convs[:1] + convs[-1:]))
