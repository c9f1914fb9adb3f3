"""Device time of the x16 up-sample + concat op (csrc/upsample.hip, hip/functional.py upsample16_cat) and of the ATen composition it replaces,
in one process, alternating:  python tools/bench_upsample16.py [--out profiles/upsample16_bench.json] [--mode bilinear]

Size: N = 32, latent 16 x 16, Cc = 12 -- the [x_hat; x] pass of a bs-16 256 x 256 step with latent_nc 12.  The ATen composition is
F.interpolate + torch.cat + the conversion to dense NHWC memory of pixel stride 16 (zero-filled buffer, channels copied in: the form
HipConv2d takes a 15-channel input in), forward and its autograd backward.  Each figure is the time of ITERS calls between two device
events after a warm-up of four seconds of load; ROUNDS such windows per variant, the variants taking turns, so that both see the same machine.  Every run of the
command appends its record to --out; the summary over all recorded runs holds min / median / max per variant (the spread) and the
verdict: the op counts as faster only where its slowest window is faster than the composition's fastest.

Algorithmic bytes (fp32): forward writes the output once (4 ld B per pixel, ld = Cc + 4) and reads the image once (16 B per pixel at pixel
stride 4) and the condition once; backward reads dout once, writes dimg once and dcond once.  The achieved rate is those bytes over the
median time, stated as a share of the 6.29 TB/s a float4 copy reaches on an MI355X."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from crdr_amd.hip import functional as HF  # noqa: E402
from crdr_amd.hip import ops  # noqa: E402

N, H_LAT, W_LAT, CC = 32, 16, 16, 12
ITERS, ROUNDS, WARMUP_S = 200, 5, 4.0   # warm-up: the variants in turn until this many seconds of load have passed
COPY_RATE = 6.29e12   # B/s, float4 copy


def algorithmic_bytes(n, h, w, cc, direction):
    pixels, ld = n * 16 * h * 16 * w, cc + 4
    cond = 4 * n * h * w * cc
    return {"fwd": pixels * (4 * ld + 16) + cond, "bwd": pixels * (4 * ld + 16) + cond, "bwd_dcond": pixels * 4 * ld + cond}[direction]


def aten_composition(img, cond, mode):
    kw = {} if mode == "nearest" else {"align_corners": False}
    x = torch.cat((img, F.interpolate(cond, scale_factor=16, mode=mode, **kw)), dim=1)
    n, c, h, w = x.shape
    buf = torch.zeros((n, h, w, ops.ld_for(c)), dtype=x.dtype, device=x.device)
    buf[..., :c] = x.permute(0, 2, 3, 1)
    return buf.permute(0, 3, 1, 2)[:, :c]


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS * 1e-3


def measure(mode):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    img = ops.nhwc((torch.rand(N, 3, 16 * H_LAT, 16 * W_LAT, generator=g) * 2 - 1).to(dev))[0].detach().requires_grad_(True)
    cond = ops.dense_nhwc(torch.randn(N, CC, H_LAT, W_LAT, generator=g).to(dev)).detach().requires_grad_(True)
    cot = ops.nhwc(torch.randn(N, 3 + CC, 16 * H_LAT, 16 * W_LAT, generator=g).to(dev))[0]
    forwards = {"hip": lambda i=img: HF.upsample16_cat(i, cond, mode), "aten": lambda i=img: aten_composition(i, cond, mode)}
    outs = {k: f() for k, f in forwards.items()}
    outs_d = {k: f(img.detach()) for k, f in forwards.items()}   # the discriminator phase: the image is detached, only dcond is wanted
    err = float((outs["hip"].detach() - outs["aten"].detach()).abs().max())
    variants = {}
    for k in ("hip", "aten"):
        def fwd(k=k):
            with torch.no_grad():
                forwards[k]()
        variants[f"{k}.fwd"] = fwd
        variants[f"{k}.bwd"] = lambda k=k: torch.autograd.grad(outs[k], (img, cond), cot, retain_graph=True)
        variants[f"{k}.bwd_dcond"] = lambda k=k: torch.autograd.grad(outs_d[k], (cond,), cot, retain_graph=True)
    t0 = time.time()
    while time.time() - t0 < WARMUP_S:   # (the backward's first second or so under load runs at half speed: DESIGN 16)
        for fn in variants.values():
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():   # the variants take turns
            times[k].append(window(fn))
    return {"mode": mode, "shape": {"N": N, "latent": [H_LAT, W_LAT], "Cc": CC}, "iters_per_window": ITERS, "max_abs_diff_hip_vs_aten": err,
            "window_s": times}


def summarise(runs):
    out = {}
    for k in runs[0]["window_s"]:
        ts = [t for r in runs for t in r["window_s"][k]]
        direction = k.split(".", 1)[1]
        nbytes = algorithmic_bytes(N, H_LAT, W_LAT, CC, direction)
        med = statistics.median(ts)
        out[k] = {"min_us": min(ts) * 1e6, "median_us": med * 1e6, "max_us": max(ts) * 1e6, "windows": len(ts), "algorithmic_MB": nbytes / 1e6,
                  "TBps_at_median": nbytes / med / 1e12, "share_of_float4_copy_rate": nbytes / med / COPY_RATE}
    verdict = {d: bool(out[f"hip.{d}"]["max_us"] < out[f"aten.{d}"]["min_us"]) for d in ("fwd", "bwd", "bwd_dcond")}
    speedup = {d: out[f"aten.{d}"]["median_us"] / out[f"hip.{d}"]["median_us"] for d in ("fwd", "bwd", "bwd_dcond")}
    return {"per_variant": out, "hip_slowest_window_beats_aten_fastest": verdict, "median_speedup_over_aten": speedup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--mode", default="bilinear", choices=sorted(HF.UPSAMPLE16_MODES))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_upsample16: no GPU -- a time is measured on the device or not at all")
    run = measure(a.mode)
    record = {"runs": []}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            record = json.load(f)
    record["runs"] = [r for r in record["runs"] if r["mode"] == a.mode] + [run]
    record["summary"] = summarise(record["runs"])
    print(json.dumps(record["summary"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
