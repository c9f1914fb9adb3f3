"""Float64 restatements of the entropy-model kernels of csrc/entropy.hip and the seeded inputs the direct tests feed them.

Plain torch / numpy on the CPU, differentiable by autograd; nothing here is shaped like a kernel.  The restatements are thin wrappers
around oracle.crdr_oracle (generic in the dtype): the direct tests call them on `.double()` copies of the fp32 operands, and once more on
the fp32 operands themselves to measure what fp32 arithmetic alone costs (the `s` of the gradient gates).  The two bounds are the values
the kernels receive -- `float` -- so that sigma = float32(0.11) sits on the same side of the bound in both implementations.

The input builders make operands for which the float64 reference alone decides every discrete choice (which side of the likelihood
floor, which way y - mu rounds, which side of the scale bound), so the GPU tests compare every element and exclude none;
tests/test_entropy_ref_host.py asserts those properties of the reference alone."""

import numpy as np
import torch

from oracle import crdr_oracle as O
from tests.golden.seeded_weights import seeded_input, seeded_tensor

SCALE_BOUND = float(np.float32(0.11))
LIK_BOUND = float(np.float32(1e-9))
GBITS = (0.7, -1.3, 0.2)            # per-image bit weights: image 1 runs the blocking branch of the likelihood LowerBound
WINDOW = (0.5e-9, 2e-9)             # no raw float64 likelihood of a built input lies inside (an fp32 kernel may land on either side)
ROUND_MARGIN = 2.0 ** -10           # |frac(y - mu) - 1/2| of every continuous input
EB = "entropy_model_z"

# ---- restatements ------------------------------------------------------------------------------------------------------------------


def gaussian_likelihood(values, mu, sigma, raw=False):
    """O.gaussian_likelihood with the fp32-rounded bounds; raw: before the likelihood floor"""
    s = O.lower_bound(sigma, SCALE_BOUND)
    v = torch.abs(values - mu)
    lik = O._phi((0.5 - v) / s) - O._phi((-0.5 - v) / s)
    return lik if raw else O.lower_bound(lik, LIK_BOUND)


def gaussian_conditional(y, mu, sigma, noise=None):
    """O.gaussian_conditional with the fp32-rounded bounds -> (y_hat, likelihood); noise None: the quantised (eval) pair"""
    v = y - mu
    q = O.forced_round(v)
    if noise is not None:
        return (q - v).detach() + v + mu, gaussian_likelihood(y + noise, mu, sigma)
    return q + mu, gaussian_likelihood(q + mu, mu, sigma)


def eb_likelihood(sd, v, raw=False):
    """O.eb_likelihood with the fp32-rounded floor; v [N, C, H, W]"""
    n, c = v.shape[:2]
    flat = v.transpose(0, 1).reshape(c, 1, -1)
    lo, up = O.eb_logits(sd, EB, flat - 0.5), O.eb_logits(sd, EB, flat + 0.5)
    sign = -torch.sign(lo + up).detach()
    lik = torch.abs(torch.sigmoid(sign * up) - torch.sigmoid(sign * lo))
    if not raw:
        lik = O.lower_bound(lik, LIK_BOUND)
    return lik.reshape(c, n, *v.shape[2:]).transpose(0, 1)


def entropy_bottleneck(sd, z, noise=None):
    """O.entropy_bottleneck with the fp32-rounded floor -> (z_hat, likelihood)"""
    med = sd[EB + ".quantiles"][:, 0, 1].reshape(1, -1, 1, 1)
    if noise is not None:
        v = z - med
        return (O.forced_round(v) - v).detach() + v + med, eb_likelihood(sd, z + noise)
    q = O.forced_round(z - med.detach()) + med.detach()
    return q, eb_likelihood(sd, q)


def eb_aux_loss(sd):
    return O.eb_aux_loss(sd, EB)


def bits_per_image(lik):
    return O.bits_per_image(lik)


def build_indexes(sigma, scale_table):
    return O.build_indexes(sigma, scale_table, SCALE_BOUND)


def symbols(y, mu):
    return torch.round(y - mu).to(torch.int32)


def as_dtype(sd, dtype, grad=False):
    return {k: v.detach().to(dtype).clone().requires_grad_(grad) for k, v in sd.items()}


# ---- Philox4x32-10 and the sample rule of include/crdr_hip.h (integers only) ------------------------------------------------------------

_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key: int):
    """counter: uint64 array (the low two of the four counter words; the high two are 0) -> four uint32 arrays"""
    ctr = np.asarray(counter, dtype=np.uint64)
    c = [ctr & _M32, ctr >> np.uint64(32), np.zeros_like(ctr), np.zeros_like(ctr)]
    k0, k1 = key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]   # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _M32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def philox_counter_lane(n_img, hw, c, ctot=None, c0=0):
    """-> (idx // 4, idx % 4) of element (n, ch, px) of an [N, C, HW] slice, idx = (n HW + px) Ctot + c0 + ch"""
    ctot = c if ctot is None else ctot
    pix = np.arange(n_img * hw, dtype=np.uint64).reshape(n_img, 1, hw)
    idx = pix * np.uint64(ctot) + np.uint64(c0) + np.arange(c, dtype=np.uint64).reshape(1, c, 1)
    return idx >> np.uint64(2), (idx & np.uint64(3)).astype(np.int64)


def philox_uniform(seed: int, offset: int, n_img, hw, c, ctot=None, c0=0):
    """the U[-1/2, 1/2) samples of crdr_philox_uniform / io.philox as a float32 [N, C, HW] tensor: (word >> 8) 2^-24 - 1/2, exact"""
    grp, lane = philox_counter_lane(n_img, hw, c, ctot, c0)
    with np.errstate(over="ignore"):
        words = philox4x32_10(grp + np.uint64(offset), seed)      # (counter = philox[1] + idx / 4 wraps at 2^64 like the kernel's)
    r = np.choose(lane, words)
    return torch.from_numpy(((r >> np.uint64(8)).astype(np.float64) * 2.0 ** -24 - 0.5).astype(np.float32))


# ---- dispatch arithmetic of crdr_gauss_cond_{fwd,bwd}2 ------------------------------------------------------------------------------------

def gc_blocks(hw, c):
    """blocks per image of the forward: one 16-byte group per thread, at most 2048"""
    return max(1, min(-(-hw * c // 1024), 2048))


def gc_vector(c, lds=(), offsets=(), ctot=None, c0=0):
    """the four-channel kernels run iff C, every pixel stride, every channel offset (pointer alignment), Ctot and c0 are multiples of 4"""
    return all(v % 4 == 0 for v in (c, *lds, *offsets, c if ctot is None else ctot, c0))


def fwd_passes(hw, c, vec):
    """grid-stride passes of the forward over one image"""
    return -(-(hw * c // 4 if vec else hw * c) // (gc_blocks(hw, c) * 256))


def bwd_passes(n, hw, c, vec):
    work = n * hw * c // 4 if vec else n * hw * c
    return -(-work // (min(-(-work // 256), 4096) * 256))


# ---- seeded inputs (float32, CPU, NCHW) ---------------------------------------------------------------------------------------------

def sigma_specials():
    """exactly the fp32 bound, one ulp above, one ulp below, below the bound, negative"""
    b = np.float32(0.11)
    return torch.tensor([b, np.nextafter(b, np.float32(1)), np.nextafter(b, np.float32(0)), np.float32(0.05), np.float32(-1.0)])


def round_margin(v):
    """min |frac(v) - 1/2| in float64"""
    v = v.double()
    return ((v - torch.floor(v)) - 0.5).abs().min().item()


def in_window(raw):
    return (raw > WINDOW[0]) & (raw < WINDOW[1])


def gc_raw_likelihoods(d):
    """float64 raw (unfloored) likelihoods of a case: (noisy, quantised)"""
    y, mu, sg, nz = (d[k].double() for k in ("y", "mu", "sigma", "noise"))
    return gaussian_likelihood(y + nz, mu, sg, raw=True), gaussian_likelihood(torch.round(y - mu) + mu, mu, sg, raw=True)


SIGMA_GRAD_MARGIN = 1e-3


def gc_scale_grad(d):
    """float64 gradient of sum_n gbits[n] bits[n] with respect to the BOUNDED scale max(sigma, bound): what reaches the scale
    LowerBound's rule, which blocks it where sigma < bound unless it is negative"""
    y, mu, nz = (d[k].double() for k in ("y", "mu", "noise"))
    s = torch.clamp(d["sigma"].detach().double(), min=SCALE_BOUND).requires_grad_(True)
    bits = bits_per_image(gaussian_likelihood(y + nz, mu, s))
    (bits * d["gbits"].double()).sum().backward()
    return s.grad


def gc_case(tag, n, c, h, w):
    """-> dict of y, mu, sigma, noise, gyh (the y_hat cotangent), gbits.  Scales 6 / 4 / 2: about a third of the elements sit at the
    likelihood floor, sigma goes below the bound and negative.  Elements whose float64 likelihood (noisy or quantised) falls in WINDOW
    are moved to y = mu + 1/4, and so are elements above the floor and below the scale bound whose scale gradient is within
    SIGMA_GRAD_MARGIN of a change of sign (d lik / d sigma changes sign near |v| = 1/2; the terms of the difference are O(10), their fp32 error
    O(1e-5): the sign, which decides whether the rule blocks, is then the reference's alone); elements within ROUND_MARGIN of a rounding
    boundary are moved by 2^-8."""
    assert n * c * h * w >= 8 and w >= 2
    shape = (n, c, h, w)
    d = {"y": seeded_input(tag + ".y", shape, 6.0), "mu": seeded_input(tag + ".mu", shape, 4.0), "sigma": seeded_input(tag + ".sg", shape, 2.0),
         "noise": seeded_input(tag + ".noise", shape, 0.5), "gyh": seeded_input(tag + ".gyh", shape),
         "gbits": torch.tensor(GBITS[:n]) if n > 1 else torch.tensor([GBITS[1]])}
    sp = sigma_specials()
    d["sigma"].view(-1)[:sp.numel()] = sp
    neg = 1 if n > 1 else 0            # the image with the negative weight: one element far under the floor, one well above it
    d["y"][neg, 0, 0, 0], d["sigma"][neg, 0, 0, 0] = d["mu"][neg, 0, 0, 0] + 9.3, 0.5
    d["y"][neg, 0, 0, 1], d["sigma"][neg, 0, 0, 1] = d["mu"][neg, 0, 0, 1] + 0.3, 1.0
    for _ in range(8):
        ln, lq = gc_raw_likelihoods(d)
        gs = gc_scale_grad(d)
        bad = in_window(ln) | in_window(lq) | ((d["sigma"].double() < SCALE_BOUND) & (ln > WINDOW[1]) & (gs.abs() < SIGMA_GRAD_MARGIN))
        d["y"][bad] = d["mu"][bad] + 0.25
        d["noise"][bad] *= 0.5
        v = d["y"].double() - d["mu"].double()
        near = ((v - torch.floor(v)) - 0.5).abs() < 2 * ROUND_MARGIN
        d["y"][near] += 2.0 ** -8
        if not bool(bad.any()) and not bool(near.any()):
            return d
    raise AssertionError(tag)


def gc_grid_case(tag, n, c, h, w):
    """y, mu on the grid of multiples of 2^-4 with |.| < 64: y - mu and round(y - mu) + mu are exact in fp32.  The first elements hold
    exact ties of both parities (x.5 with x even and odd, both signs)."""
    shape = (n, c, h, w)
    y = torch.round(seeded_input(tag + ".y", shape, 60.0) * 16) / 16
    mu = torch.round(seeded_input(tag + ".mu", shape, 60.0) * 16) / 16
    ties = torch.tensor([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, -3.5])
    y.view(-1)[:ties.numel()] = mu.view(-1)[:ties.numel()] + ties
    y[..., -1] = mu[..., -1] + 6.5   # one tie per row as well, wherever the row lands in a vector of four
    assert y.abs().max() < 128
    return {"y": y, "mu": mu, "sigma": seeded_input(tag + ".sg", shape, 2.0), "noise": seeded_input(tag + ".noise", shape, 0.5)}


def eb_state(c):
    """seeded parameters of an EntropyBottleneck(channels=c), keyed like the oracle's state dict (fp32)"""
    f = (1, 3, 3, 3, 3, 1)
    sd = {}
    for i in range(5):
        sd[f"{EB}._matrix{i}"] = seeded_tensor(f"{EB}._matrix{i}", (c, f[i + 1], f[i]))
        sd[f"{EB}._bias{i}"] = seeded_tensor(f"{EB}._bias{i}", (c, f[i + 1], 1))
        if i < 4:
            sd[f"{EB}._factor{i}"] = seeded_tensor(f"{EB}._factor{i}", (c, f[i + 1], 1))
    sd[f"{EB}.quantiles"] = seeded_tensor(f"{EB}.quantiles", (c, 1, 3))
    return sd


EB_Z_SCALE, EB_Z_TAIL = 8.0, 12.0


def eb_shape(c, nhw):
    n = 3 if nhw % 3 == 0 else 1
    return (n, c, 1, nhw // n)


def eb_case(c, nhw, grid=False):
    """-> (state dict, dict of z, noise, gzh, gbits).  z = u |u| * EB_Z_SCALE (u uniform in [-1, 1)): dense around the medians and out
    to the saturated tails, where the likelihood is at the floor.  Elements in WINDOW are moved to the median + 1/4 and their noise shrunk; elements near a
    rounding boundary by 2^-8.  grid: z on multiples of 2^-4 (the medians are not)."""
    sd = eb_state(c)
    shape = eb_shape(c, nhw)
    n = shape[0]
    tag = f"ebd.{c}.{nhw}" + (".grid" if grid else "")
    u = seeded_input(tag + ".z", shape)
    z = u * u.abs() * EB_Z_SCALE
    if grid:
        z = torch.round(z * 16) / 16
    d = {"z": z, "noise": seeded_input(tag + ".noise", shape, 0.5), "gzh": seeded_input(tag + ".gzh", shape),
         "gbits": torch.tensor(GBITS[:n]) if n > 1 else torch.tensor([GBITS[1] if nhw % 2 else GBITS[0]])}
    med = sd[EB + ".quantiles"][:, 0, 1].reshape(1, -1, 1, 1)
    if nhw >= 48:
        neg = 1 if n > 1 else 0        # the middle image (weight -1.3 wherever n = 3): one element in the tail, one at the centre
        d["z"][neg, :, 0, 0] = EB_Z_TAIL
        d["z"][neg, :, 0, 1] = (med[0, :, 0, 0] + 0.25) if not grid else 0.25
    sd64 = as_dtype(sd, torch.float64)
    for _ in range(8):
        zz = d["z"].double()
        bad = in_window(eb_likelihood(sd64, zz + d["noise"].double(), raw=True)) | in_window(eb_likelihood(sd64, entropy_bottleneck(sd64, zz)[0], raw=True))
        if grid:
            d["z"][bad] = torch.round(med.expand(shape)[bad])
        else:
            d["z"][bad] = (med.expand(shape) + 0.25)[bad]
        d["noise"][bad] *= 0.25          # (a narrow channel can hold the window within half a step of its median)
        v = d["z"].double() - med.double()
        near = ((v - torch.floor(v)) - 0.5).abs() < 2 * ROUND_MARGIN
        d["z"][near] += 2.0 ** -4 if grid else 2.0 ** -8
        if not bool(bad.any()) and not bool(near.any()):
            return sd, d
    raise AssertionError(tag)


def symbol_case(levels, n=2, c=6, h=5, w=7):
    """-> (y, mu, sigma, table): y, mu on the 2^-4 grid with exact ties; sigma log-uniform over the table's range with entries exactly on
    table values, at the bound and below it"""
    g = gc_grid_case(f"sym.{levels}", n, c, h, w)
    table = O.get_scale_table(0.11, 256.0, levels).float()
    sg = torch.exp(seeded_input(f"sym.{levels}.sg", (n, c, h, w)) * 4.5 + 1.5)     # e^-3 .. e^6: both ends of the table are passed
    flat = sg.view(-1)
    k = min(levels, 40)
    flat[:k] = table[:: max(1, levels // k)][:k]
    flat[k:k + 5] = sigma_specials()
    flat[k + 5] = table[-1]
    return g["y"], g["mu"], sg, table


# ---- the cases of tests/test_gpu_entropy_direct.py (their size and dispatch claims are asserted by tests/test_entropy_ref_host.py) -------

GC_KINDS = ("cl", "nchw", "padded", "slice4", "slice3")
# kind: dense channels-last | NCHW memory | NHWC memory with the channels padded to four lanes | channels [4, 4 + C) of a wider NHWC
# buffer (pixel stride a multiple of 4, pointer 16-byte aligned: taken as it is) | channels [3, 3 + C) of one (pointer not aligned: the
# wrapper copies it).  Whatever the layout, what reaches the kernel has strides and pointers that are multiples of four floats, so
# the dispatch is decided by C alone: the four-channel kernels for C % 4 == 0, the scalar ones otherwise.
GC_SMALL = [("cl", 1), ("cl", 3), ("cl", 6), ("cl", 32), ("cl", 36), ("nchw", 6), ("nchw", 32), ("padded", 3), ("slice4", 6), ("slice4", 32),
            ("slice3", 6), ("slice3", 36)]                      # 3 x C x 5 x 5: per_img <= 900, one block per image
GC_MEDIUM_HW = {1: (47, 71), 3: (31, 37), 6: (23, 29), 32: (11, 13), 36: (9, 13)}   # per_img 3337 .. 4576: 4 or 5 blocks per image
GC_MEDIUM = [("cl", 1), ("cl", 3), ("cl", 6), ("cl", 32), ("cl", 36), ("nchw", 36), ("slice4", 32), ("padded", 3)]
GC_BIG = [(2, 8, 513, 513), (2, 3, 419, 419)]                   # the smallest sizes at which the grid-stride loops run a second pass
EB_CHANNELS = (1, 6, 24)
EB_SIZES = (1, 48, 255, 256, 257, 1021)                         # N HW: one thread .. four passes of the 256-thread block, a partial last
AUX_CHANNELS = (1, 24, 86, 192)                                 # 3 C = 258 > 256 at C = 86: a second pass of the single block
SYMBOL_LEVELS = (1, 64, 256)
PHILOX_SEED, PHILOX_OFFSET = 0x1234567887654321, (1 << 32) - 3  # both key words in use; the counter carries into its second word


def gc_shape(size, c):
    return (3, c, 5, 5) if size == "small" else (3, c, *GC_MEDIUM_HW[c])
