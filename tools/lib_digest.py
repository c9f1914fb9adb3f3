"""Digest of a build of libcrdr_hip.so, for proving a host-only change: python tools/lib_digest.py crdr_amd/_lib [--json FILE]

(a) Device code: per object file and embedded gfx950 code object, the SHA-256 of .text and of .rodata and every kernel's resource record
    (whole code objects differ between two compiles of one file: a per-compile id sits in their string tables).
(b) Plans: a sweep over the host planners through the C ABI alone (no device is opened).  Descriptors: every 'c' and 'w' key of the shipped
    tune database (a 'c' key omits the weight pack's size: the packers' round32(OC) x round32(C), tap-major round32(4 taps) columns) and the
    shapes of tests/test_cabi_and_host.py's Winograd planning test, at G = 1, 3, 16; conv flags as shipped and with COLSUM, each also with
    NOSPLIT / BF16X3 / BF16X6; wgrad modes 0 / BF16X3 / BF16X6 / SQUARE_Q; algorithm id 0 and every base id up to two past the last one,
    each with all sixteen values of bits 8..11; crdr_gdn_workspace (forward and backward) over M = 1 .. 262144, C = 4 .. 320 and
    a dense or padded ldx.  Printed per requested family: records, records that planned, and one SHA-256 over all.
Two builds compute the same plans and run the same device code when the two outputs are equal."""
import argparse
import ast
import ctypes as C
import glob
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import kernel_resources  # noqa: E402
from crdr_amd.hip import lib as L  # noqa: E402

OBJCOPY = "/opt/rocm/lib/llvm/bin/llvm-objcopy"


def device_code(lib_dir):
    out = {}
    for path in sorted(glob.glob(os.path.join(lib_dir, "*.o"))):
        cos = []
        for co in kernel_resources.code_objects(path):
            rec = {}
            with tempfile.TemporaryDirectory() as tmp:
                elf = os.path.join(tmp, "co.elf")
                open(elf, "wb").write(co)
                for sec in (".text", ".rodata"):
                    raw = os.path.join(tmp, "sec.bin")
                    subprocess.run([OBJCOPY, "-O", "binary", f"--only-section={sec}", elf, raw], check=True)
                    rec[sec] = hashlib.sha256(open(raw, "rb").read()).hexdigest()
            cos.append(rec)
        out[os.path.basename(path)] = {"code_objects": cos, "kernels": sorted(kernel_resources.kernels(path), key=lambda k: k["name"])}
    return out


def load(lib_dir):
    lib = C.CDLL(os.path.join(lib_dir, "libcrdr_hip.so"))
    for name, (res, args) in L.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def round32(v):
    return (v + 31) // 32 * 32


def conv_desc(n, h, w, c, oh, ow, oc, k, stride, pad, transposed, ldx, ldy, flags, ldres, ldg, wlayout):
    return L.ConvDesc(N=n, H=h, W=w, C=c, OH=oh, OW=ow, OC=oc, kh=k[0], kw=k[1], stride=stride, pad=pad, transposed=transposed, ldx=ldx, ldy=ldy,
                      wrows=round32(oc), wcols=round32(4 * k[0] * k[1] if wlayout else c), flags=flags, ldres=ldres, ldg=ldg, wlayout=wlayout,
                      reserved=0, ldpre=0, ldmask=0)


def test_conv_descs():
    """the descriptors of test_winograd_ids_are_planned_only_for_the_shapes_they_take (they reach the pair-tile variant; no shipped shape does)"""
    def desc(c, oc, h, k, stride=1, pad=None, transposed=0, n=2, oh=None):
        pad = k // 2 if pad is None else pad
        oh = oh or ((h - 1) * stride - 2 * pad + k if transposed else (h + 2 * pad - k) // stride + 1)
        return L.ConvDesc(N=n, H=h, W=h, C=c, OH=oh, OW=oh, OC=oc, kh=k, kw=k, stride=stride, pad=pad, transposed=transposed, ldx=c, ldy=oc,
                          wrows=oc, wcols=round32(c), flags=0, ldres=0, ldg=0, wlayout=0, reserved=0, ldpre=0, ldmask=0)
    return [desc(96, 96, 32, 3), desc(128, 128, 32, 3), desc(96, 104, 32, 3), desc(96, 96, 16, 3, n=1), desc(96, 96, 32, 3, transposed=1),
            desc(320, 224, 16, 5), desc(96, 96, 32, 3, stride=2), desc(96, 96, 32, 1), desc(96, 96, 32, 7), desc(100, 96, 32, 3),
            desc(32, 64, 16, 5), desc(96, 96, 64, 3), desc(96, 96, 64, 3, transposed=1), desc(96, 96, 16, 3), desc(96, 96, 8, 3),
            desc(96, 96, 64, 3, stride=2), desc(320, 224, 64, 5), desc(8, 224, 64, 5), desc(192, 192, 128, 5, stride=2),
            desc(192, 192, 64, 5, stride=2), desc(192, 192, 32, 5, stride=2), desc(256, 256, 64, 5, stride=2, transposed=1, oh=128),
            desc(96, 98, 64, 3), desc(4256, 320, 16, 5, transposed=1, n=16), desc(12, 64, 64, 3), desc(24, 64, 16, 5), desc(100, 96, 64, 3)]


def fields(s):
    return tuple(getattr(s, f) for f, _ in s._fields_)


def sweep(lib):
    db = json.load(open(os.path.join(ROOT, "crdr_amd", "hip", "tune_gfx950.json")))["algos"]
    keys = sorted((ast.literal_eval(k) for k in db), key=repr)
    convs, wgrads, bad = [], [], []
    for k in keys:
        try:
            if k[0] == "c":
                convs.append(conv_desc(*k[1:]))
            elif k[0] == "w":
                wgrads.append(L.WgradDesc(*k[1:10], k[10][0], k[10][1], *k[11:15], 0, 0))
        except (TypeError, IndexError):
            bad.append(k)
    convs += test_conv_descs()
    wgrads += [L.WgradDesc(N=2, PH=32, PW=32, PC=96, ldp=96, QH=32, QW=32, QC=64, ldq=64, kh=k, kw=k, stride=s, pad=k // 2, gI=96, gJ=64,
                           accumulate=0, algo=0) for k, s in ((3, 1), (3, 2), (5, 1), (5, 2))]
    err = lambda: lib.crdr_last_error()
    nt, ns, nw = lib.crdr_conv2d_num_configs(), lib.crdr_conv2d_num_stream_configs(), lib.crdr_conv2d_num_wino_configs()
    wino_names = ["F(2x2)", "F(2x2) pair tiles", "F(4x4)"]
    conv_family = lambda b: ("built-in" if b == 0 else "tiled" if b <= nt else "streaming" if b <= nt + ns else
                             wino_names[b - nt - ns - 1] if b <= nt + ns + min(nw, 3) else "beyond")
    nd = lib.crdr_conv2d_wgrad_num_configs() - 1   # (num_configs counts the F(2x2) slab kernel, num_wino_configs counts it again)
    wgrad_family = lambda b: "built-in" if b == 0 else "direct" if b <= nd else "F(2x2) slab" if b == nd + 1 else "F(4x4) slab" if b == nd + 2 else "beyond"
    stats, sha = {}, hashlib.sha256()

    def record(side, family, ok, rec):
        s = stats.setdefault((side, family), [0, 0])
        s[0] += 1
        s[1] += bool(ok)
        sha.update(repr(rec).encode())

    rows, ld, item = C.c_int(), C.c_int(), L.W4FilterItem()
    extra = [0, L.CONV_NOSPLIT, L.CONV_BF16X3, L.CONV_BF16X6]
    for i, d in enumerate(convs):
        own, p = d.flags, C.byref(d)
        for flags in [own | cs | e for cs in (0, L.EPI_COLSUM) for e in extra]:
            d.flags = flags
            for G in (1, 3, 16):
                for base in range(nt + ns + nw + 3):
                    for hi in range(16):
                        d.reserved = base | (hi << 8)
                        algo = lib.crdr_conv2d_choose_algo(p, G)
                        rec = [i, flags, G, d.reserved, algo, algo or err(), lib.crdr_conv2d_grouped_workspace(p, G)]
                        rc = lib.crdr_conv2d_colsum_layout(p, G, C.byref(rows), C.byref(ld))
                        rec += [rc, (rows.value, ld.value) if rc == 0 else err(), lib.crdr_conv2d_filter_cache_bytes(p, G)]
                        rc = lib.crdr_conv2d_filter_item(p, G, C.byref(item))
                        rec += [rc, bytes(item) if rc == 0 else err()]
                        record("conv", conv_family(base), algo, rec)
        d.flags, d.reserved = own, 0
    for i, d in enumerate(wgrads):
        p = C.byref(d)
        for mode in (0, L.WGRAD_BF16X3, L.WGRAD_BF16X6, L.WGRAD_SQUARE_Q):
            for G in (1, 3, 16):
                for base in range(nd + 5):
                    for hi in range(16):
                        d.algo = base | (hi << 8) | mode
                        # a successful plan that needs no workspace does not occur (a slab is never empty); a refusal leaves its text
                        ws = lib.crdr_conv2d_wgrad_grouped_workspace(p, G)
                        record("wgrad", wgrad_family(base), ws, [i, mode, G, d.algo, ws, ws or err()])
    for m in (1, 63, 64, 65, 126, 4096, 32768, 262144):
        for c in range(4, 321, 4):
            for ldx in (c, c + 4):
                d = L.GdnDesc(M=m, C=c, ldx=ldx, ldy=c, inverse=0, beta_min=1e-6, reparam_offset=2.0 ** -18)
                ws = [lib.crdr_gdn_workspace(C.byref(d), backward) for backward in (0, 1)]
                record("gdn", "workspace", all(ws), [m, c, ldx] + ws)
    return {"descriptors": {"conv": [fields(d) for d in convs], "wgrad": [fields(d)[:-1] for d in wgrads]},
            "families": {f"{side} {fam}": {"records": n, "planned": ok} for (side, fam), (n, ok) in sorted(stats.items())},
            "sha256": sha.hexdigest(), "skipped_keys": [repr(k) for k in bad]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("lib_dir")
    ap.add_argument("--json")
    a = ap.parse_args()
    res = {"device_code": device_code(a.lib_dir), "plans": sweep(load(a.lib_dir))}
    dev = hashlib.sha256(json.dumps(res["device_code"], sort_keys=True).encode()).hexdigest()
    nk = sum(len(o["kernels"]) for o in res["device_code"].values())
    print(f"device code: {len(res['device_code'])} objects, {nk} kernels, sha256 over all section digests and kernel records {dev}")
    for fam, s in res["plans"]["families"].items():
        print(f"plans: {fam:26s} {s['planned']:9d} / {s['records']:9d} planned")
    print(f"plans: sha256 over all records {res['plans']['sha256']}")
    for k in res["plans"]["skipped_keys"]:
        print("SKIPPED (no descriptor from this key):", k)
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1, default=lambda b: b.hex())
    sys.exit(1 if res["plans"]["skipped_keys"] else 0)
