"""Device time of the perceptual loss for both backbones and of the 2x2 max-pool kernels (csrc/maxpool2.hip) at their four LPIPS-VGG
shapes:  python tools/bench_lpips.py [--out profiles/lpips_vgg_bench.json]

Size: 16 x 3 x 256 x 256, the batch of the stage-3 step.  `loss.<net>`: one forward + backward of LPIPSLoss (both images through the
frozen net, the gradient with respect to the reconstruction).  `pool.fwd.<C>x<H>` / `pool.bwd.<C>x<H>`: crdr_maxpool2s2_fwd / _bwd
alone, through the C ABI, on the map each VGG pool reads, [16, C, H, H].  Each figure is the time of a window of calls between two
device events after WARMUP_S seconds of the same calls; ROUNDS windows per variant, the variants taking turns.  Every run of the command
appends its record to --out; the summary over all recorded runs holds min / median / max per variant.

Algorithmic bytes of the pool (fp32, U = 4 N (H/2) (W/2) C): the forward reads x once (4 U) and writes y (U); the backward reads x and dy
(5 U) and writes dx (4 U).  The achieved rate is those bytes over the median time, stated as a share of the 8 TB/s HBM peak and of the
6.3 TB/s a streaming kernel reaches on an MI355X.  Only the first shape (268 MB of input) is larger than the 256 MiB Infinity Cache: the
other three can be served from it in a loop like this one, so their rate is not an HBM rate."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from crdr_amd.hip import lib as L  # noqa: E402
from crdr_amd.hip import ops  # noqa: E402

N, SIZE = 16, 256
POOL_SHAPES = [(64, 256), (128, 128), (256, 64), (512, 32)]   # (C, H = W) of the map each pool reads
ROUNDS, WARMUP_S = 5, 3.0
ITERS = {"loss": 10, "pool": 100}
HBM_PEAK, HBM_STREAM = 8.0e12, 6.3e12   # B/s


def pool_bytes(c, h, direction):
    unit = 4 * N * (h // 2) * (h // 2) * c
    return {"fwd": 5 * unit, "bwd": 9 * unit}[direction]


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def measure():
    from crdr_amd.losses.perceptual_loss import LPIPSLoss
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    real = ops.nhwc((torch.rand(N, 3, SIZE, SIZE, generator=g) * 2 - 1).to(dev))[0]
    fake = ops.nhwc((torch.rand(N, 3, SIZE, SIZE, generator=g) * 2 - 1).to(dev))[0].detach().requires_grad_(True)
    variants, keep = {}, []
    for net in ("alex", "vgg"):
        torch.manual_seed(0)
        loss = LPIPSLoss(loss_weight=1.0, net=net, allow_random_weights=True).to(dev)   # the time does not depend on the weights

        def step(loss=loss):
            torch.autograd.grad(loss(real, fake), (fake,))
        variants[f"loss.{net}"] = step
    lib, st = L.load(), ops._stream()
    for c, h in POOL_SHAPES:   # the kernels through the C ABI on preallocated tensors: no allocation, no autograd between two launches
        x = torch.relu(torch.randn(N, h, h, c, generator=g)).to(dev)
        cot = torch.randn(N, h // 2, h // 2, c, generator=g).to(dev)
        y, dx = torch.empty_like(cot), torch.empty_like(x)
        keep.append((x, cot, y, dx))
        variants[f"pool.fwd.{c}x{h}"] = lambda x=x, y=y, c=c, h=h: L.check(
            lib.crdr_maxpool2s2_fwd(x.data_ptr(), c, N, h, h, c, y.data_ptr(), c, st), "maxpool2s2_fwd")
        variants[f"pool.bwd.{c}x{h}"] = lambda x=x, cot=cot, dx=dx, c=c, h=h: L.check(
            lib.crdr_maxpool2s2_bwd(x.data_ptr(), c, cot.data_ptr(), c, N, h, h, c, dx.data_ptr(), c, st), "maxpool2s2_bwd")
    t0 = time.time()
    while time.time() - t0 < WARMUP_S:
        for k, fn in variants.items():
            for _ in range(2 if k.startswith("loss") else 20):
                fn()
        torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():   # the variants take turns
            times[k].append(window(fn, ITERS[k.split(".")[0]]))
    return {"shape": {"N": N, "size": SIZE}, "iters_per_window": ITERS, "window_s": times}


def summarise(runs):
    out = {}
    for k in runs[0]["window_s"]:
        ts = [t for r in runs for t in r["window_s"][k]]
        med = statistics.median(ts)
        out[k] = {"min_us": min(ts) * 1e6, "median_us": med * 1e6, "max_us": max(ts) * 1e6, "windows": len(ts)}
        if k.startswith("pool"):
            _, direction, shape = k.split(".")
            c, h = map(int, shape.split("x"))
            nbytes = pool_bytes(c, h, direction)
            out[k].update({"algorithmic_MB": nbytes / 1e6, "TBps_at_median": nbytes / med / 1e12, "share_of_hbm_peak": nbytes / med / HBM_PEAK,
                           "share_of_streaming_rate": nbytes / med / HBM_STREAM})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips: no GPU -- a time is measured on the device or not at all")
    record = {"runs": []}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            record = json.load(f)
    record["runs"].append(measure())
    record["summary"] = summarise(record["runs"])
    print(json.dumps(record["summary"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
