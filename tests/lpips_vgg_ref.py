"""A restatement of LPIPS-VGG (lpips 0.1.4 `LPIPS(net="vgg")` over torchvision `vgg16.features`) in plain torch CPU ops, generic in the
dtype: F.conv2d, a first-maximum 2x2 pool written out explicitly, and the LPIPS formula.  Nothing here is shaped like a kernel.

The network makes discrete decisions -- which pre-activations a ReLU lets through, which of a window's four values a pool forwards --
and the gradient with respect to the image is discontinuous in them: one pre-activation of 1e-7 that rounds to the other side of zero
changes the gradient by a part in a thousand.  Two correct evaluations in different arithmetic can therefore not be compared on the
gradient unless they take the same decisions.  `lpips_vgg(..., decisions=...)` imposes a given set on the pass of the second argument
(the one gradients flow to); `decision_budget` says how many of them differ from the restatement's own and whether each difference sits
where the restatement itself is undecided (a pre-activation, or the gap between two window values, within 1e-4 of its layer's largest
value).  The value is continuous in the decisions, so the first argument's pass keeps its own."""
import math

import torch
import torch.nn.functional as F

from tests.golden.seeded_weights import seeded_input, seeded_tensor

CFG = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512), (512, 512),
       (512, 512), (512, 512))
POOL_BEFORE = (2, 4, 7, 10)      # convs that read a pooled map
TAPS = (1, 3, 6, 9, 12)          # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
WINDOW = 1e-4                    # a decision may differ only where the float64 run is this close (relative to the layer) to undecided
BUDGET = 8                       # and at most this many may (1e-5 of the 888 320 decisions of the 2 x 3 x 35 x 45 input)


# ---- seeded weights and inputs (float32 values, CPU) ---------------------------------------------------------------------------------

def seeded_vgg(gain: bool = True):
    """-> (sd, lin): {"net.{j}.weight" / ".bias"} and the five lin vectors, float32.  The conv weights carry a gain of sqrt(2) (He
    scaling: without it the activations shrink layer by layer until the biases take over) and the lin weights are non-negative, as
    the trained ones are."""
    sd = {}
    for j, (ci, co) in enumerate(CFG):
        w = seeded_tensor(f"lpips_vgg.net.{j}.weight", (co, ci, 3, 3))
        sd[f"net.{j}.weight"] = w * math.sqrt(2.0) if gain else w
        sd[f"net.{j}.bias"] = seeded_tensor(f"lpips_vgg.net.{j}.bias", (co,))
    lin = [seeded_tensor(f"lpips_vgg.lin.{i}", (CFG[j][1],)).abs() for i, j in enumerate(TAPS)]
    return sd, lin


def seeded_images(shape):
    tag = "x".join(map(str, shape))
    return seeded_input(f"lpips_vgg.a.{tag}", shape), seeded_input(f"lpips_vgg.b.{tag}", shape)


def cast(sd, lin, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}, [v.to(dtype) for v in lin]


def _tag(shape):
    return "x".join(map(str, shape))


def post_relu_input(shape):
    """about half exact zeros: all-zero windows are ties at zero"""
    return torch.relu(seeded_input("lpips_vgg.pool." + _tag(shape), shape, 2.0))


def negative_input(shape):
    return -0.25 - seeded_input("lpips_vgg.neg." + _tag(shape), shape).abs()


def doubled_max_input(shape):
    """every whole window holds its maximum twice: values from {1, 2, 3}, the window's largest written to a seeded pair of positions"""
    n, c, h, w = shape
    x = torch.floor((seeded_input("lpips_vgg.tie." + _tag(shape), shape) + 1) * 1.5).clamp_(0, 2) + 1
    oh, ow = h // 2, w // 2
    top = windows(x).max(-1).values
    pair = torch.floor((seeded_input("lpips_vgg.tiepos." + _tag(shape), (n, c, oh, ow)) + 1) * 2).clamp_(0, 3).long()
    for k, cells in enumerate([((0, 0), (1, 1)), ((0, 1), (1, 0)), ((0, 0), (0, 1)), ((1, 0), (1, 1))]):
        for i, j in cells:
            v = x[:, :, i:2 * oh:2, j:2 * ow:2]   # a view: the assignment writes into x
            v[pair == k] = top[pair == k]
    return x


POOL_INPUTS = {"post_relu": post_relu_input, "doubled_max": doubled_max_input, "negative": negative_input}


def pool_cotangent(shape):
    return seeded_input("lpips_vgg.poolcot." + _tag(shape), shape) + 1.5


# ---- the pool ---------------------------------------------------------------------------------------------------------------------------

def windows(x):
    """[N, C, H, W] -> [N, C, H/2, W/2, 4]: the values of every whole 2x2 window in scan order (0,0), (0,1), (1,0), (1,1); an odd last
    row / column belongs to no window"""
    oh, ow = x.shape[2] // 2, x.shape[3] // 2
    x = x[:, :, :2 * oh, :2 * ow]
    return torch.stack([x[..., 0::2, 0::2], x[..., 0::2, 1::2], x[..., 1::2, 0::2], x[..., 1::2, 1::2]], -1)


def first_max(win):
    """index of the first maximum along the last axis: a later value replaces the running best only when it is strictly greater"""
    best = win[..., 0]
    at = torch.zeros(best.shape, dtype=torch.long)
    for k in range(1, 4):
        take = win[..., k] > best
        best = torch.where(take, win[..., k], best)
        at = torch.where(take, torch.full_like(at, k), at)
    return at


def pool2(x, at=None):
    """MaxPool2d(2, 2): -> (y, index taken in each window, window values).  `at` imposes the indices.  Autograd sends a window's gradient
    to the taken position and zero to the other three and to the pixels of a dropped odd row / column."""
    win = windows(x)
    if at is None:
        at = first_max(win.detach())
    return win.gather(-1, at.unsqueeze(-1)).squeeze(-1), at, win


# ---- the network and the distance -------------------------------------------------------------------------------------------------------

def _taps(sd, x, decisions=None, record=None):
    dt = x.dtype
    x = (x - torch.tensor(SHIFT, dtype=dt).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=dt).view(1, 3, 1, 1)
    taps, p = [], 0
    for j in range(len(CFG)):
        if j in POOL_BEFORE:
            x, at, win = pool2(x, None if decisions is None else decisions["argmax"][p])
            p += 1
            if record is not None:
                record["win"].append(win.detach())
                record["argmax"].append(at)
        z = F.conv2d(x, sd[f"net.{j}.weight"], sd[f"net.{j}.bias"], padding=1)
        mask = (z > 0) if decisions is None else decisions["masks"][j]
        if record is not None:
            record["z"].append(z.detach())
            record["masks"].append(mask)
        x = torch.where(mask, z, torch.zeros_like(z))
        if j in TAPS:
            taps.append(x)
    return taps


def lpips_layer(f0, f1, lin):
    """per image: spatial mean of sum_c lin_c (f0_c / (|f0| + 1e-10) - f1_c / (|f1| + 1e-10))^2, |.| the norm over channels"""
    n0 = f0 / (f0.square().sum(1, keepdim=True).sqrt() + 1e-10)
    n1 = f1 / (f1.square().sum(1, keepdim=True).sqrt() + 1e-10)
    return (lin.reshape(1, -1, 1, 1) * (n0 - n1).square()).sum(1).mean((1, 2))


def lpips_vgg(sd, lin, a, b, decisions=None):
    """lpips.LPIPS(net="vgg")(a, b) on [-1, 1] images -> (value [N], record).  record = {"z": 13 pre-activations, "masks": 13 ReLU masks,
    "win": 4 pools' window values, "argmax": 4 pools' indices, "taps": 5 maps} of b's pass; `decisions` = {"masks", "argmax"} replaces
    that pass's own.  Differentiable with respect to b."""
    record = {"z": [], "masks": [], "win": [], "argmax": []}
    with torch.no_grad():
        fa = _taps(sd, a)
    fb = _taps(sd, b, decisions, record)
    record["taps"] = [t.detach() for t in fb]
    return sum(lpips_layer(x, y, w) for x, y, w in zip(fa, fb, lin)), record


def decisions_of_acts(acts):
    """the decisions an implementation took, read off its thirteen post-ReLU maps: masks = act > 0, pool indices = the first maximum of
    its own values"""
    acts = [t.detach().cpu() for t in acts]
    return {"masks": [t > 0 for t in acts], "argmax": [first_max(windows(acts[j - 1])) for j in POOL_BEFORE]}


def decision_budget(record, decisions):
    """Compare `decisions` with the ones `record` (a free run of the restatement, ideally float64) took.
    -> (number that differ, number of those outside the window, total decisions).  A ReLU difference is inside the window when the
    record's |z| there is at most WINDOW x the layer's largest |z|; a pool difference when the record's two candidate values differ by at
    most WINDOW x the layer's largest value."""
    differ = outside = total = 0
    for z, own, got in zip(record["z"], record["masks"], decisions["masks"]):
        total += z.numel()
        d = own != got
        differ += int(d.sum())
        outside += int((z.abs()[d] > WINDOW * z.abs().max()).sum())
    for win, own, got in zip(record["win"], record["argmax"], decisions["argmax"]):
        total += own.numel()
        d = own != got
        differ += int(d.sum())
        gap = (win.gather(-1, own.unsqueeze(-1)) - win.gather(-1, got.unsqueeze(-1))).squeeze(-1).abs()
        outside += int((gap[d] > WINDOW * win.abs().max()).sum())
    return differ, outside, total


# ---- error measures -----------------------------------------------------------------------------------------------------------------------

def max_rel(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().double()
    return ((got - ref).abs().max() / ref.abs().max()).item()


def rel_l2(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().double()
    return ((got - ref).norm() / ref.norm()).item()
