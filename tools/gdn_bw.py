"""Achieved HBM bandwidth of the GDN / IGDN op (crdr_gdn_fwd / crdr_gdn_bwd) at the Balle18 analysis sizes (bs 16, 192 channels):
algorithmic bytes = forward: read x, write y (8 B / element; x^2 and the norm are internal scratch); backward: read x, dy, write dx
(12 B / element).  Usage: python tools/gdn_bw.py

    python tools/gdn_bw.py --shortcut [--lib other/libcrdr_hip.so]
the fused shortcut (crdr_gdn_res_fwd: read x and res, write y, 12 B / element) against the pair it replaces (crdr_gdn_fwd, then an ATen
add of the shortcut: 8 + 12 B / element), and plain crdr_gdn_fwd through the raw C ABI in several trials (their spread is the yardstick
for "unchanged"); with --lib the plain forward is also timed in another build of the library (the parent's), interleaved trial by trial."""
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crdr_amd.models.layer.gdn import GDN  # noqa: E402


def timed(fn, reps=10):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def shortcut_mode(other_lib=None, trials=7):
    from crdr_amd.hip import lib as L
    from crdr_amd.hip import ops
    dev = torch.device("cuda:0")
    n, c, hw = 16, 192, 128
    libs = {"this": L.load()}
    if other_lib:
        libs["other"] = C.CDLL(other_lib)
        for name in ("crdr_gdn_workspace", "crdr_gdn_fwd"):
            getattr(libs["other"], name).restype, getattr(libs["other"], name).argtypes = L.SIGNATURES[name]
    out = {}
    for inverse in (False, True):
        m = GDN(c, inverse=inverse).to(dev)
        x = torch.randn(n, c, hw, hw, device=dev).contiguous(memory_format=torch.channels_last)
        res = torch.randn_like(x)
        y = torch.empty_like(x)
        d = L.GdnDesc(M=n * hw * hw, C=c, ldx=c, ldy=c, inverse=int(inverse), beta_min=m.beta_min, reparam_offset=m.reparam_offset)
        nb = libs["this"].crdr_gdn_workspace(C.byref(d), 0)
        ws = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
        p = (ws.data_ptr() + 255) // 256 * 256
        args = (C.byref(d), x.data_ptr(), m.beta.data_ptr(), m.gamma.data_ptr())

        def plain(lib):
            return lambda: lib.crdr_gdn_fwd(*args, y.data_ptr(), p, nb, ops._stream())

        def fused():
            libs["this"].crdr_gdn_res_fwd(*args, res.data_ptr(), c, y.data_ptr(), p, nb, ops._stream())

        def pair():
            libs["this"].crdr_gdn_fwd(*args, y.data_ptr(), p, nb, ops._stream())
            torch.add(y, res, out=y)
        runs = {"fused": fused, "pair": pair, **{f"plain_{k}": plain(v) for k, v in libs.items()}}
        t = {k: [] for k in runs}
        for _ in range(trials):      # interleaved: every trial times every variant once
            for k, fn in runs.items():
                t[k].append(timed(fn, reps=20) * 1e6)
        el = x.numel()
        rec = {k: {"us_min": round(min(v), 1), "us_median": round(sorted(v)[len(v) // 2], 1), "us_max": round(max(v), 1)} for k, v in t.items()}
        rec["fused"]["GBps_at_12B_per_element"] = round(12.0 * el / (min(t["fused"]) * 1e-6) / 1e9, 1)
        rec["pair"]["GBps_at_20B_per_element"] = round(20.0 * el / (min(t["pair"]) * 1e-6) / 1e9, 1)
        rec["plain_this"]["GBps_at_8B_per_element"] = round(8.0 * el / (min(t["plain_this"]) * 1e-6) / 1e9, 1)
        out[f"{'igdn' if inverse else 'gdn'} {n}x{c}x{hw}x{hw}"] = rec
    print(json.dumps(out, indent=1))


def main():
    if "--shortcut" in sys.argv:
        return shortcut_mode(sys.argv[sys.argv.index("--lib") + 1] if "--lib" in sys.argv else None)
    dev = torch.device("cuda:0")
    out = {}
    for inverse in (False, True):
        m = GDN(192, inverse=inverse).to(dev)
        for hw in (128, 64, 32):
            x = torch.randn(16, 192, hw, hw, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            tf = timed(lambda: m(x.detach()))
            y = m(x)
            g = torch.randn_like(y)
            tb = timed(lambda: torch.autograd.grad(y, x, g, retain_graph=True))
            n = x.numel()
            flop = 2.0 * 16 * hw * hw * 192 * 192
            out[f"{'igdn' if inverse else 'gdn'} 16x192x{hw}x{hw}"] = {
                "fwd_us": round(tf * 1e6, 1), "fwd_GBps_algorithmic": round(8.0 * n / tf / 1e9, 1), "fwd_mix_TFLOPs": round(flop / tf / 1e12, 1),
                "bwd_us": round(tb * 1e6, 1), "bwd_GBps_algorithmic": round(12.0 * n / tb / 1e9, 1)}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
