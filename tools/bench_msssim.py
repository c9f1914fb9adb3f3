"""Device time of the MS-SSIM kernels (msssim.hip) and, for comparison only, of the composed torch restatement
(tests/msssim_ref.py) on the same GPU:  python tools/bench_msssim.py [--step]

Rows: forward + backward of ms_ssim (gradient to y, as MSSSIMLoss needs) at the benchmark batch 16 x 3 x 256^2 and at
1 x 3 x 512 x 768, the forward alone, and the validation metric (calc_ms_ssim).  Kernel times are the best of 5 replays
of a HIP graph holding 10 calls, HIP events around the replay.  Bytes are the algorithmic HBM traffic of the kernels
(images, pyramid, per-pixel maps, gradients; LDS-resident halos counted once).  --step: three stage-1 iterations at
bs 16 x 256^2 with distortion_loss MSSSIMLoss (the run to put under rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from crdr_amd.hip import msssim as MS  # noqa: E402
from crdr_amd.hip import ops  # noqa: E402


def timed_graph(fn, reps=10):
    side = torch.cuda.Stream()
    fn()
    torch.cuda.synchronize()
    ops.reserve_workspace(torch.device("cuda:0"), side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(reps):
            fn()
    return _best(g.replay, reps)


def timed_eager(fn, reps=10):
    fn()
    torch.cuda.synchronize()

    def run():
        for _ in range(reps):
            fn()
    return _best(run, reps)


def _best(run, reps):
    best = 1e9
    for _ in range(5):
        run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps * 1e-3)
    return best


def hbm_bytes(n, h, w, backward):
    """fp32 NHWC ld-4 pixels: 16 B each; maps 64 B per output pixel"""
    total, hl, wl = 0.0, h, w
    for level in range(5):
        pix, opix = n * hl * wl, n * (hl - 10) * (wl - 10)
        nh, nw = (hl + 1) // 2, (wl + 1) // 2
        fwd = 2 * 16 * pix + (2 * 16 * n * nh * nw if level < 4 else 0) + (64 * opix if backward else 0)
        bwd = 64 * opix + 2 * 16 * pix + 16 * pix + (16 * n * nh * nw if level < 4 else 0) if backward else 0
        total += fwd + bwd
        hl, wl = nh, nw
    return total


def kernels(dev):
    from crdr_amd.utils.img_utils import calc_ms_ssim
    from tests import msssim_ref as R
    rows = []
    for n, h, w in ((16, 256, 256), (1, 512, 768)):
        g = torch.Generator(device="cpu").manual_seed(0)
        x = (torch.rand(n, 3, h, w, generator=g) * 2 - 1).to(dev)
        y0 = (x.cpu() + 0.2 * torch.randn(n, 3, h, w, generator=g)).clamp(-1, 1).to(dev)
        xs, _ = ops.nhwc(x)
        ys, _ = ops.nhwc(y0)     # the decoder's layout: NHWC, pixel stride 4
        ys.requires_grad_(True)

        def fwd_bwd():
            ys.grad = None
            MS.ms_ssim(xs, ys, 1.0).backward()

        def fwd():
            with torch.no_grad():
                MS.ms_ssim(xs, ys, 1.0)
        t_fb, t_f = timed_graph(fwd_bwd), timed_graph(fwd)
        xr, yr = x.clone(), y0.clone().requires_grad_(True)

        def torch_fb():
            yr.grad = None
            R.ms_ssim(xr, yr, 1.0).backward()
        t_torch = timed_eager(torch_fb, reps=3)
        nb_fb, nb_f = hbm_bytes(n, h, w, True), hbm_bytes(n, h, w, False)
        rows.append({"shape": [n, 3, h, w], "fwd_bwd_ms": t_fb * 1e3, "fwd_ms": t_f * 1e3, "fwd_bwd_hbm_MB": nb_fb / 1e6,
                     "fwd_hbm_MB": nb_f / 1e6, "fwd_bwd_GBps": nb_fb / t_fb / 1e9, "torch_restatement_fwd_bwd_ms": t_torch * 1e3})
        print(json.dumps(rows[-1]), flush=True)
    real = (torch.rand(1, 3, 512, 768, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
    fake = (real + 0.05 * torch.randn(real.shape, device=dev)).clamp(-1, 1)
    calc_ms_ssim(real, fake)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        calc_ms_ssim(real, fake)
    e1.record()
    torch.cuda.synchronize()
    rows.append({"metric": "calc_ms_ssim 1x3x512x768 (host round trip included)", "ms": e0.elapsed_time(e1) / 10})
    print(json.dumps(rows[-1]), flush=True)
    return rows


def step(dev):
    import bench
    tr = bench.build_trainer(1, 16, 256, str(dev), graphs=True)
    from crdr_amd.losses import build_loss
    tr.distortion_loss = build_loss({"type": "MSSSIMLoss", "loss_weight": 1.0}, loss_name="distortion_loss")
    x = (torch.rand(16, 3, 256, 256, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
    for it in range(1, 4):
        log = tr.optimize_parameters(it, {"real_images": x})
    torch.cuda.synchronize()
    print(json.dumps({"stage1_msssim_step": {k: float(v) for k, v in (log or {}).items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.step:
        step(dev)
        return
    rows = kernels(dev)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
