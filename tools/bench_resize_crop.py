"""Time of the device crop loader with and without resize_range (csrc/resize_crop.hip, dataset/device_pipeline.py), in one process, the
variants taking turns:  python tools/bench_resize_crop.py [--out profiles/resize_crop_bench.json]

Size: bs 16, crop 256, a pool of 32 synthetic 512 x 768 images -- the input stage of a bs-16 256 x 256 training step.  Variants:
  plain.kernel        crdr_crop_flip_normalize, the launch alone (items already on the device)
  scale1.kernel       crdr_resize_crop_flip_normalize at scale 1.0 (both passes skipped: 1 tap), the launch alone
  bicubic.kernel      the same with draws of resize_range [0.5, 1.0], bicubic (up to 9 taps), the launch alone
  bilinear.kernel     ... bilinear (up to 5 taps)
  plain.cut / scale1.cut / bicubic.cut / bilinear.cut     DeviceCropLoader.cut() as the trainer calls it: host tables, upload, launch
  bicubic.host_tables / bilinear.host_tables              the numpy table build alone (no device work)
  bicubic.upload                                          the one host-to-device copy of a batch's items + tables alone
Kernel variants: ITERS launches between two device events.  cut / upload variants: a host clock around ITERS calls that end in a device
synchronise (the host part is what they are about).  host_tables: a host clock.  Every variant rotates through 8 different batches of
draws.  A warm-up of two seconds of all variants comes first; then ROUNDS windows per variant.  Every run of the command appends its
record to --out; the summary over all recorded runs holds min / median / max per variant and each median as a share of the 71.5 ms
stage-3 step the README records (the yardstick: an input stage should stay under 1 % of it)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from crdr_amd.dataset.device_pipeline import DeviceCropLoader, DeviceImagePool, draw_crops, draw_resized_crops  # noqa: E402
from crdr_amd.hip import lib as L  # noqa: E402
from crdr_amd.hip import ops  # noqa: E402

BS, SIZE, POOL, SHAPE = 16, 256, 32, (512, 768)
ITERS, HOST_ITERS, ROUNDS, WARMUP_S, BATCHES = 200, 20, 5, 2.0, 8
STEP_S = 71.5e-3   # README: the stage-3 step at bs 16


def device_window(fn, iters=ITERS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(iters):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def host_window(fn, iters=HOST_ITERS, sync=True):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(iters):
        fn(k)
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def measure():
    dev = torch.device("cuda:0")
    lib = L.load()
    rng = np.random.default_rng(0)
    pool = DeviceImagePool([rng.integers(0, 256, size=SHAPE + (3,), dtype=np.uint8) for _ in range(POOL)], dev)
    out = ops.empty_nhwc(BS, 3, SIZE, SIZE, dev)
    idx = [rng.integers(0, POOL, size=BS) for _ in range(BATCHES)]
    plain = DeviceCropLoader(pool, BS, SIZE)
    plain_draws = [draw_crops(pool.shapes, i, SIZE, rng) for i in idx]
    plain_items = [torch.from_numpy(np.concatenate([pool.offsets[i][:, None], d], axis=1).astype(np.int64)).to(dev) for i, d in zip(idx, plain_draws)]
    variants, windows, info = {}, {}, {}

    def plain_kernel(k):
        L.check(lib.crdr_crop_flip_normalize(pool.pool.data_ptr(), plain_items[k % BATCHES].data_ptr(), BS, SIZE, SIZE, out.data_ptr(), 4, ops._stream()))
    variants["plain.kernel"], windows["plain.kernel"] = plain_kernel, device_window
    variants["plain.cut"], windows["plain.cut"] = (lambda k: plain.cut(idx[k % BATCHES], plain_draws[k % BATCHES], out=out)), host_window

    def add(name, interpolation, draws):
        loader = DeviceCropLoader(pool, BS, SIZE, resize_range=(0.5, 1.0), interpolation=interpolation)
        host = [loader.host_tables(i, d) for i, d in zip(idx, draws)]
        bufs = [torch.from_numpy(h).to(dev) for h, _ in host]
        info[name] = {"taps": [t for _, t in host], "upload_bytes": [int(h.nbytes) for h, _ in host]}

        def kernel(k):
            b, taps = bufs[k % BATCHES], host[k % BATCHES][1]
            L.check(lib.crdr_resize_crop_flip_normalize(pool.pool.data_ptr(), b.data_ptr(), b.data_ptr() + 16 * BS, BS, taps, SIZE, SIZE,
                                                        out.data_ptr(), 4, ops._stream()))
        variants[f"{name}.kernel"], windows[f"{name}.kernel"] = kernel, device_window
        variants[f"{name}.cut"], windows[f"{name}.cut"] = (lambda k: loader.cut(idx[k % BATCHES], draws[k % BATCHES], out=out)), host_window
        if name != "scale1":
            variants[f"{name}.host_tables"] = lambda k: loader.host_tables(idx[k % BATCHES], draws[k % BATCHES])
            windows[f"{name}.host_tables"] = lambda fn: host_window(fn, sync=False)
        if name == "bicubic":
            stage = torch.empty(max(h.size for h, _ in host), dtype=torch.int32, device=dev)
            variants["bicubic.upload"] = lambda k: stage[:host[k % BATCHES][0].size].copy_(torch.from_numpy(host[k % BATCHES][0]))
            windows["bicubic.upload"] = host_window

    add("scale1", "bicubic", [np.concatenate([np.ones((BS, 1)), d], axis=1).astype(np.float64) for d in plain_draws])
    for interpolation in ("bicubic", "bilinear"):
        add(interpolation, interpolation, [draw_resized_crops(pool.shapes, i, SIZE, rng, (0.5, 1.0)) for i in idx])

    scale1 = DeviceCropLoader(pool, BS, SIZE, resize_range=(0.5, 1.0))
    same = bool(torch.equal(scale1.cut(idx[0], np.concatenate([np.ones((BS, 1)), plain_draws[0]], axis=1)), plain.cut(idx[0], plain_draws[0])))
    t0 = time.time()
    while time.time() - t0 < WARMUP_S:
        for fn in variants.values():
            for k in range(8):
                fn(k)
        torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():   # the variants take turns
            times[k].append(windows[k](fn))
    return {"shape": {"bs": BS, "size": SIZE, "pool": POOL, "image": list(SHAPE)}, "scale1_equals_plain_cut": same, "info": info, "window_s": times}


def summarise(runs):
    out = {}
    for k in runs[0]["window_s"]:
        ts = [t for r in runs for t in r["window_s"][k]]
        med = statistics.median(ts)
        out[k] = {"min_us": min(ts) * 1e6, "median_us": med * 1e6, "max_us": max(ts) * 1e6, "windows": len(ts),
                  "median_share_of_71.5ms_step": med / STEP_S}
    ratios = {f"{n}.{w}_over_plain.{w}": out[f"{n}.{w}"]["median_us"] / out[f"plain.{w}"]["median_us"]
              for n in ("scale1", "bicubic", "bilinear") for w in ("kernel", "cut")}
    return {"per_variant": out, "median_ratio": ratios,
            "augmented_cut_under_1_percent_of_step": {n: bool(out[f"{n}.cut"]["max_us"] * 1e-6 < 0.01 * STEP_S) for n in ("bicubic", "bilinear")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize_crop: no GPU -- a time is measured on the device or not at all")
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
