"""Torch-facing wrappers over the C ABI: device memory, streams and autograd plumbing only.

Tensors are logical NCHW with channels_last strides (memory NHWC); a channel slice of such a tensor is passed
to the kernels in place through its pixel stride (`ld`).  All arithmetic happens in libcrdr_hip.so.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import Optional, Tuple

import torch

from . import lib as L
from . import packs, tune
from .batched import BumpArena, JobTable, SiteTables, _capturing, _require_gpu, _stream  # noqa: F401  (the capture rules of the batched launches live there)

_ws_cache = {}
_ws_keep = []   # superseded buffers stay alive: captured graphs may still reference them
_ws_max = 0     # largest request seen so far (eager warm-up), so a buffer created under graph capture never has to grow

# Algorithm selection per problem shape, the analogue of the reference's `cudnn.benchmark = True`
# (base_trainer.py:20): with AUTOTUNE on, the first call of a shape times every tile configuration x split depth
# of the library on the real operands and caches the fastest; off, the library's built-in cost model decides.
AUTOTUNE = False
# Nonzero: every forward / input-gradient convolution without an explicit algorithm takes this forced id (tile configuration
# + split, see crdr_conv_desc.reserved) instead of the tuner's or the cost model's choice.  The choice normally depends on the
# problem size, and with it the fp32 summation order; tests that compare runs at different batch sizes bit for bit pin it.
FORCED_CONV_ALGO = 0
# Opt-in reduced-cost matrix mode ("bf16x3", include/crdr_hip.h CRDR_CONV_BF16X3): conv / weight-gradient products run as
# split-bf16 triples on the bf16 MFMA path (per-product relative error <= 3 * 2^-16), everything else unchanged.  Set by the
# trainers from the YAML key `precision: bf16x3` for the duration of a training step; the codec and every parity claim use
# the exact fp32 default.
MATRIX_BF16X3 = False
# Opt-in fp32-EQUIVALENT matrix mode ("bf16x6", CRDR_CONV_BF16X6): every operand is split exactly into three bf16 pieces and a product is the
# six piece products of weight >= 2^-16 with fp32 accumulation (dropped terms <= 2^-23 of the product: one fp32 rounding) at 3/8 of the exact
# fp32 MFMA time.  Direct kernels only (tiled, streaming 1x1, direct weight gradients); the Winograd kernels stay on the exact fp32
# instruction and remain tuner candidates beside them.  YAML key `precision: bf16x6`; held to the fp32 parity gates (tests/test_gpu_bf16x6.py).
MATRIX_BF16X6 = False


def _matrix_mode() -> int:   # 0 exact fp32, 1 bf16x3, 2 bf16x6
    return 2 if MATRIX_BF16X6 else (1 if MATRIX_BF16X3 else 0)


def _cf() -> int:
    return (0, L.CONV_BF16X3, L.CONV_BF16X6)[_matrix_mode()]


def _wa(algo: int) -> int:
    return int(algo) | (0, L.WGRAD_BF16X3, L.WGRAD_BF16X6)[_matrix_mode()]


def _mk() -> tuple:   # suffix of the weight-gradient tuner keys (the conv keys carry the mode in their flags)
    return ((), (1,), (2,))[_matrix_mode()]


# The tuner lives in tune.py.  bench.py reads these names as attributes of ops, so they stay bound here, to the SAME objects (tune only
# mutates its containers); everything else says tune.<name>.
_algo_cache, TUNE_LOG, TUNE_REJECTED = tune.algo_cache, tune.LOG, tune.REJECTED
load_tune_cache, save_tune_cache, DEFAULT_TUNE_DB = tune.load, tune.save, tune.DEFAULT_DB

WINOGRAD = os.environ.get("CRDR_WINOGRAD", "1") != "0"   # 0: the tuner never offers the Winograd kernel
WINO4 = os.environ.get("CRDR_WINO4", "1") != "0"         # 0: ... never the F(4x4, 3x3) / F(3x3, 4x4) kernels (F(2x2) stays)

# Tests: every convolution a Winograd kernel accepts takes it (without the tuner, whose choice is per shape and speed): the
# model-level parity tests run once more through it.  True: the F(2x2, 3x3) kernel (variants 0 / 1); 4: the F(4x4, 3x3) kernel
# (variant 2) where it applies, F(2x2, 3x3) elsewhere.
PREFER_WINOGRAD = False


def _prefer_wino(d, G: int = 1) -> int:
    """-> the Winograd algorithm id if PREFER_WINOGRAD is set and the library accepts it for this launch, else 0."""
    if not PREFER_WINOGRAD or (d.kh, d.kw, d.stride) not in (((3, 3, 1), (5, 5, 1), (5, 5, 2)) if PREFER_WINOGRAD == 4 else ((3, 3, 1), (5, 5, 1))):
        return 0
    q = L.ConvDesc.from_buffer_copy(d)
    for wid in reversed(tune.ids().wino if PREFER_WINOGRAD == 4 else tune.ids().wino[:2]):   # (F(4x4) / the pair-tile variant where they apply)
        q.reserved = wid
        if L.load().crdr_conv2d_choose_algo(C.byref(q), G) == wid:
            return wid
    return 0


WINO4_SPLITS = (1, 2, 3, 5, 7, 11, 15)


def _wgrad_wino4_ids():
    """Forced ids of the F(3x3, 4x4) weight-gradient slab kernel (wino4_wgrad.hip: the id behind the last wgrad configuration) with its strip
    splits 1 .. 256; the library refuses them for the shapes it does not take."""
    w4 = tune.ids().wgrad_wino4
    return [tune.tile_id(w4 - 1, ls) for ls in range(9)] if WINOGRAD and WINO4 and w4 >= 0 else []


# Test hook: callable(weight, saved activation as an NCHW view, offset vector or None) called in grad mode by every fused conv / chain layer /
# Charm transform with a ReLU epilogue -- the activations the product's backward derives its ReLU masks from (CRDR_EPI_RELUMASK: act > 0;
# with CRDR_EPI_MASKOFF, where a beta vector was added after the ReLU: act - offset > 0).  tests/test_gpu_step.py hands the generator's masks
# to the oracle (oracle.relu / generator_forward(impose=...)).  None in production.
RELU_MASK_SINK = None


def _is_wino4(algo: int) -> bool:   # the F(4x4, 3x3) kernel, whatever K split the id carries in bits 8..11
    return (algo & 0xFF) == tune.ids().wino4


WINO4_DEMOTED = [0]   # launches whose tuned / preferred F(4x4) plan was dropped because an epilogue operand was not 16-byte aligned


def _demote_if_misaligned(d, ios, G: int, explicit: bool) -> None:
    """The F(4x4) kernel's epilogue works with 16-byte accesses.  A plan id out of the perf database (or ops.PREFER_WINOGRAD) is keyed by shape
    and strides, not by pointer alignment: for an output / residual / mask view at a channel offset that is not a multiple of 4 floats the
    launch would be refused by the library (it hard-fails an id it cannot honour, which is right for an EXPLICITLY forced one).  Such a
    launch takes the built-in plan instead."""
    if not explicit and _is_wino4(d.reserved) and any(p_ and int(p_) % 16 for g in range(G) for p_ in (ios[g].y, ios[g].res, ios[g].mask)):
        d.reserved = 0
        WINO4_DEMOTED[0] += 1


def _launch_conv(lib, d, ios, G: int, ws, ws_n, device):
    """crdr_conv2d_grouped, through the persistent filter cache (packs) where the launch runs the F(4x4) kernel on registered weight packs."""
    cached = packs.filter_cache_for(d, ios, G, device) if _is_wino4(d.reserved) else None
    if cached is None:
        return lib.crdr_conv2d_grouped(C.byref(d), ios, G, ws, ws_n, _stream())
    ent, valid = cached
    return lib.crdr_conv2d_grouped_ex(C.byref(d), ios, G, ws, ws_n, ent.u.data_ptr(), ent.nbytes, int(valid), _stream())


# Tuner trials of the F(4x4) kernel: in the step its transformed filters are rebuilt once per optimiser update by the batched launch, not in
# front of the convolution, so a candidate is timed with its filters in place (a scratch cache filled by the first trial launch) and charged
# the share of the batched rebuild it causes: the cache's bytes at the rate that launch runs at (~4.8 GB per ms).
_tune_filters = {}


def _conv_workspace(lib, d, G: int, device):
    nb = lib.crdr_conv2d_grouped_workspace(C.byref(d), G)
    return workspace(nb, device, conv=True) if nb else (None, 0)


def _tune_conv_launch(lib, d, ios, G: int, device) -> Tuple[bool, float]:   # -> (the library took it, ms of batched filter rebuild it is charged)
    w_, wn_ = _conv_workspace(lib, d, G, device)
    nb = int(lib.crdr_conv2d_filter_cache_bytes(C.byref(d), G)) if _is_wino4(d.reserved) else 0
    if not nb or not packs.cacheable(ios, G) or _capturing():
        # (no transformed filters, or) the real launch will not find a cache (sub-block / temporary packs, or a launch first seen under
        # capture): it transforms on every call, and that is what the candidate is timed with
        return lib.crdr_conv2d_grouped(C.byref(d), ios, G, w_, wn_, _stream()) == 0, 0.0
    key = (packs.filter_key(d, ios, G), tuple(packs.version(int(ios[g].w)) for g in range(G)))
    ent = _tune_filters.get(key)
    valid = int(ent is not None and ent.numel() * 4 >= nb)
    if not valid:
        _tune_filters.clear()   # (one shape is tuned at a time: the previous shape's scratch is garbage)
        ent = _tune_filters[key] = torch.empty(nb // 4, dtype=torch.float32, device=device)
    return lib.crdr_conv2d_grouped_ex(C.byref(d), ios, G, w_, wn_, ent.data_ptr(), nb, valid, _stream()) == 0, nb / 4.8e9


def _stream_ids():
    """Forced-algorithm ids of the streaming 1x1 variants and of the Winograd 3x3 kernel (the library rejects them for other shapes)."""
    ids = list(tune.ids().stream) + (list(tune.ids().wino if WINO4 else tune.ids().wino[:2]) if WINOGRAD else [])
    if WINOGRAD and WINO4 and tune.ids().wino4 >= 0:   # the F(4x4) kernel with 2, 3, 4, 6, 8, 12 or 16 K splits per tile (bits 8..11 = splits - 1): launches with fewer tiles than CUs
        ids += [tune.ids().wino4 | (v << 8) for v in WINO4_SPLITS]
    return ids


def _conv_trial(lib, d, ios, G: int, device, colsum: bool, trial_out):
    """-> (run, result, reset, penalty) of tune.autotune for the conv launch d / ios.  Trials run in `trial_out` (conv2d_raw's output, which
    the launch writes afterwards), else on scratch outputs with the same strides: timing runs would accumulate into live data, and the tuner
    compares every candidate's result with the baseline plan's on a tensor it owns (tune.scratch: its pattern is from torch's generator)."""
    if trial_out is not None:
        tio, res_t, reset = ios, trial_out, None
    else:
        span = (d.N * d.OH * d.OW - 1) * d.ldy + d.OC
        res_t, reset = tune.scratch(G * span + 64, device)
        tio = (L.ConvIO * G)()
        C.memmove(tio, ios, C.sizeof(tio))
        for g in range(G):
            tio[g].y = res_t.data_ptr() + 4 * g * span
            if ios[g].pre == ios[g].y:
                tio[g].pre = tio[g].y
            if ios[g].res == ios[g].y:
                tio[g].res = tio[g].y
    keep, cost = [], 0.0

    def run(a):
        nonlocal cost
        d.reserved = a
        if colsum:   # (the layout of the partial rows depends on the plan)
            try:
                _, _, nf = _colsum_layout(lib, d, G)
            except L.CrdrHipError:
                return False
            keep[:] = [torch.empty(G * nf, dtype=torch.float32, device=device)]
            for g in range(G):
                tio[g].cs = keep[0].data_ptr() + 4 * g * nf
        ok, cost = _tune_conv_launch(lib, d, tio, G, device)
        return ok
    return run, (lambda: res_t), reset, (lambda: cost)


def _wgrad_trial(lib, d, G: int, pa, qa, device, whole: bool):
    """-> (run, result, reset, penalty) of tune.autotune for the weight gradients d / pa / qa, written to a tensor of the trial's own: the complete
    gradient with accumulate = 0 (`whole`; on a copy of d, the caller's keeps its accumulate), or the slab launch and the batched reduce of a deferred one."""
    gsize = d.gI * d.gJ * d.kh * d.kw
    tmp = torch.zeros(G * gsize + 64, dtype=torch.float32, device=device)
    ta = (C.c_void_p * G)(*[tmp.data_ptr() + 4 * g * gsize for g in range(G)])
    jobs_t = (L.WgradJob * G)()
    d, slab = L.WgradDesc.from_buffer_copy(d), 0
    d.accumulate = 0 if whole else d.accumulate

    def run(a):
        nonlocal slab
        d.algo = _wa(a)
        nb = lib.crdr_conv2d_wgrad_grouped_workspace(C.byref(d), G)
        if nb == 0 or nb > (2 << 30):
            return False
        slab = nb
        w_, wn_ = workspace(nb, device)
        if whole:
            return lib.crdr_conv2d_wgrad(C.byref(d), pa[0], qa[0], ta[0], w_, wn_, _stream()) == 0
        return lib.crdr_conv2d_wgrad_partial_grouped(C.byref(d), pa, qa, ta, G, w_, wn_, jobs_t, _stream()) == 0
    if whole:
        return run, (lambda: tmp), None, None

    def result():   # the trial's slabs reduced into tmp (the jobs accumulate: tmp is zeroed by reset())
        reduce_jobs_now(jobs_t, device)
        return tmp
    # + the batched reduce's read of these slabs at its measured 3.8 TB/s (profiles/r2_h_hbm_families.json)
    return run, result, tmp.zero_, (lambda: slab / 3.8e9)


# Optional per-launch timing (bench.py): {"igemm": [(flops, ev0, ev1), ...], "wgrad": [...]} or None.
# Events are recorded on the stream the kernels are launched on (torch's current stream).
PROFILE = None


def _prof_begin():
    if PROFILE is None:
        return None
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _prof_end(kind: str, flops: float, e0, label: str = "", nbytes: float = 0.0) -> None:
    """nbytes: ALGORITHMIC HBM bytes of the launch (each operand / result element once: activations in and out, the
    weight pack, residual / pre-activation / mask operands) -- what bench.py prices `roofline.traffic` against."""
    if e0 is None:
        return
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record()
    PROFILE.setdefault(kind, []).append((flops, e0, e1, label, nbytes))


_WS_HEAD = 4 * 16384  # bytes at the head of every scratch buffer: the split-K tickets of the conv kernels (CRDR_CONV_TICKETS int32)


def _ws_fit(key, device, need: Optional[int]) -> torch.Tensor:
    """-> the scratch buffer of `key` with at least `need` bytes (None, reserve_workspace: as many as a new buffer gets).  A new buffer is zeroed
    and sized for the largest request seen so far plus headroom, the one it supersedes stays alive; a launch's request may not grow under capture."""
    size = max(int(_ws_max * 1.25), 1 << 20)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < (size if need is None else need):
        if need is not None and torch.cuda.is_current_stream_capturing():
            # a buffer born inside a capture would belong to that graph's private pool and die with it
            raise L.CrdrHipError("workspace must be reserved before graph capture (ops.reserve_workspace); "
                                 f"need {need} bytes, have {0 if buf is None else buf.numel()}")
        if buf is not None:
            _ws_keep.append(buf)
        buf = _ws_cache[key] = torch.zeros(size, dtype=torch.uint8, device=device)
    return buf


def workspace(nbytes: int, device, conv: bool = False) -> Tuple[int, int]:
    """Grow-only per-device scratch (kernels on one stream serialise, so one buffer is enough).  The buffer is born zeroed and
    its first _WS_HEAD bytes belong to the conv kernels' split-K tickets, which every launch leaves at zero (include/crdr_hip.h,
    CRDR_CONV_TICKETS): conv launches (`conv=True`) get the buffer from its start, everything else the part behind the head."""
    global _ws_max
    nbytes = int(nbytes) + (0 if conv else _WS_HEAD)
    _ws_max = max(_ws_max, nbytes)
    buf = _ws_fit((device.index if device.index is not None else torch.cuda.current_device(), _stream()), device, nbytes)
    if conv:
        return buf.data_ptr(), buf.numel()
    return buf.data_ptr() + _WS_HEAD, buf.numel() - _WS_HEAD


def reserve_workspace(device, stream: "torch.cuda.Stream") -> None:
    """Give `stream` its scratch buffer from the ordinary allocator, sized for the largest request seen so far
    (eager warm-up).  Call before capturing a graph on that stream."""
    dev = torch.device(device)
    _ws_fit((dev.index if dev.index is not None else torch.cuda.current_device(), stream.cuda_stream), dev, None)


def _pixel_stride(t: torch.Tensor) -> int:
    """Distance in elements between two pixels of a [N,C,H,W] tensor in NHWC memory, read off the first dimension that has more than one
    entry; a single pixel has no neighbour and counts as dense (C)."""
    n, c, h, w = t.shape
    return t.stride(3) if w > 1 else (t.stride(2) if h > 1 else (t.stride(0) if n > 1 else c))


def nhwc(t: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """Return (tensor, pixel stride) for a [N,C,H,W] tensor whose memory is NHWC (possibly a channel slice);
    copies into channels_last if the layout is anything else."""
    _require_gpu(t)
    n, c, h, w = t.shape
    ld = _pixel_stride(t)
    ok = (c == 1 or t.stride(1) == 1) and ld >= c
    ok = ok and (w == 1 or t.stride(3) == ld) and (h == 1 or t.stride(2) == w * ld) and (n == 1 or t.stride(0) == h * w * ld)
    if not ok or ld % 4 != 0 or (t.data_ptr() % 16) != 0:
        if c % 4 == 0:
            t = t.contiguous(memory_format=torch.channels_last)
            if t.stride(1) != 1 or (w > 1 and t.stride(3) != c):  # degenerate sizes: force real NHWC memory
                t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            ld = c
        else:  # pad channels to a multiple of 4 (image tensors)
            cp = (c + 3) // 4 * 4
            buf = torch.zeros((n, h, w, cp), dtype=t.dtype, device=t.device)
            buf[..., :c] = t.permute(0, 2, 3, 1)
            t = buf.permute(0, 3, 1, 2)[:, :c]
            ld = cp
    return t, ld


def dense_nhwc(t: torch.Tensor) -> torch.Tensor:
    """A [N,C,H,W] tensor in NHWC memory whose pixel stride is C itself: the operand of a kernel that takes no stride.  Copies only when
    nhwc() gives another stride (a channel slice of a wider buffer, padded image lanes), through permute / contiguous / permute, which
    yields real NHWC memory at every size.  x.contiguous(memory_format=torch.channels_last) under the same condition, which some call
    sites used to spell out, gives the same elements in the same order and copies in the same cases: torch skips the copy only where
    every dimension with more than one entry already has its dense NHWC stride, and then nhwc() reports C.  The one tensor whose strides
    torch does not look at at all is a single pixel (N = H = W = 1); nhwc() takes its stride as C, so neither form copies it.  (nhwc() pads
    C % 4 != 0 to four-lane pixels whatever comes in, so such a tensor is copied even when it is dense already.)"""
    t, ld = nhwc(t)
    if ld != t.shape[1]:
        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return t


def ld_for(c: int) -> int:
    """Pixel stride the library's own allocations use: channels rounded up to a multiple of 4 (16-byte rows)."""
    return (c + 3) // 4 * 4


def empty_nhwc(n, c, h, w, device, ld: Optional[int] = None, zero: bool = False) -> torch.Tensor:
    ld = ld_for(c) if ld is None else ld
    mk = torch.zeros if (zero or ld != c) else torch.empty
    buf = mk((n, h, w, ld), dtype=torch.float32, device=device)
    return buf.permute(0, 3, 1, 2)[:, :c]


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def round32(v: int) -> int:
    return (v + 31) // 32 * 32


def pack_weight_tapmajor(w: torch.Tensor) -> torch.Tensor:
    """Conv2d weight [O][C<=4][kh][kw] -> [1][round32(O)][round32(4*kh*kw)] (crdr_conv_desc.wlayout = 1)."""
    _require_gpu(w)
    w = w.contiguous()
    I, J = w.shape[0], w.shape[1]
    T = w.shape[2] * w.shape[3]
    rows, cols = round32(I), round32(4 * T)
    dst = torch.empty((1, rows, cols), dtype=torch.float32, device=w.device)
    lib = L.load()
    L.check(lib.crdr_pack_weight(w.data_ptr(), dst.data_ptr(), I, J, T, rows, cols, 2, _stream()), "pack_weight")
    return dst


def pack_weight(w: torch.Tensor, transpose: bool) -> torch.Tensor:
    """[I][J][kh][kw] parameter -> [T][rows][cols] pack (rows/cols padded to 32)."""
    _require_gpu(w)
    w = w.contiguous()
    I, J = w.shape[0], w.shape[1]
    T = w.shape[2] * w.shape[3]
    rows, cols = (round32(J), round32(I)) if transpose else (round32(I), round32(J))
    dst = torch.empty((T, rows, cols), dtype=torch.float32, device=w.device)
    lib = L.load()
    L.check(lib.crdr_pack_weight(w.data_ptr(), dst.data_ptr(), I, J, T, rows, cols, int(transpose), _stream()), "pack_weight")
    return dst


_SPAN_LIMIT = (1 << 31) - (1 << 20)  # operand byte span the conv kernels address with one buffer descriptor


def _colsum_layout(lib, d, G: int):
    """-> (rows, ld, floats) of every problem's CRDR_EPI_COLSUM partial rows under the plan in d"""
    rows, ld = C.c_int(), C.c_int()
    L.check(lib.crdr_conv2d_colsum_layout(C.byref(d), G, C.byref(rows), C.byref(ld)), "conv2d_colsum_layout")
    return rows.value, ld.value, max(1, rows.value * 2 * ld.value)


def _conv(lib, d, ios, G: int, key, device, *, flops: float, label: str, nbytes: float, algo: int = 0, plan_as: int = 0,
          colsum: bool = False, trial_out: Optional[torch.Tensor] = None):
    """Plan and launch the G convolutions that d and ios (a ctypes array of G lib.ConvIO) describe, and record their profile entry.
    The plan: an explicit id (`algo`, else FORCED_CONV_ALGO), else the Winograd kernel PREFER_WINOGRAD asks for, else the tuned plan of
    `key` (AUTOTUNE; None: this launch is never tuned), else the plan the library would give a launch of `plan_as` problems, else the
    built-in plan.  colsum: the launch carries CRDR_EPI_COLSUM; -> [(partial-row address, rows, ld)] per problem, in colsum_queue(device)'s
    arena (None without colsum).  trial_out: conv2d_raw's output, which its tuner trials run in (_conv_trial)."""
    forced = algo or FORCED_CONV_ALGO
    wino = 0 if forced else _prefer_wino(d, G)
    GP = plan_as or G
    if forced or wino:
        d.reserved = forced or wino
    elif AUTOTUNE and key is not None and (GP == G or key in tune.algo_cache):
        algo = tune.algo_cache.get(key)
        if algo is None:
            run, result, reset, penalty = _conv_trial(lib, d, ios, G, device, colsum, trial_out)
            algo = tune.autotune(key, lib.crdr_conv2d_num_configs(), 4, run, extra=_stream_ids(), result=result, reset=reset,
                                 agree=tune.AGREE["conv"], penalty=penalty)
        d.reserved = algo
    elif GP != G:
        d.reserved = lib.crdr_conv2d_choose_algo(C.byref(d), GP)
    _demote_if_misaligned(d, ios, G, bool(forced))
    cs = None
    if colsum:
        rows, ld, nf = _colsum_layout(lib, d, G)
        q = colsum_queue(device)
        cs = [(q.alloc(nf), rows, ld) for _ in range(G)]
        for g in range(G):
            ios[g].cs = cs[g][0]
    ws, ws_n = _conv_workspace(lib, d, G, device)
    e0 = _prof_begin()
    L.check(_launch_conv(lib, d, ios, G, ws, ws_n, device), "conv2d_grouped")
    _prof_end("igemm", flops, e0, label, nbytes)
    return cs


def _wgrad(lib, d, G: int, ps, qs, gs, key, device, *, flops: float, label: str, whole: bool = False, algo: int = 0,
           defer: bool = True) -> list:
    """Plan and launch the G weight gradients that d describes (operand / gradient addresses ps, qs, gs), and record their profile entry.
    The plan: the explicit `algo`, else the tuned plan of `key` (AUTOTUNE), else the built-in plan.  whole: a tuner trial runs the complete
    weight gradient, not the slab launch (_wgrad_trial).  The slabs' reduction is deferred onto WGRAD_DEFER (defer=False: reduced inside the
    same call); -> the jobs queued there, for the caller to adjust."""
    pa, qa, ga = ((C.c_void_p * G)(*v) for v in (ps, qs, gs))
    if algo:
        d.algo = _wa(algo)
    elif AUTOTUNE:
        algo = tune.algo_cache.get(key)
        if algo is None:
            run, result, reset, penalty = _wgrad_trial(lib, d, G, pa, qa, device, whole)
            algo = tune.autotune(key, lib.crdr_conv2d_wgrad_num_configs(), 8, run, extra=_wgrad_wino4_ids(), penalty=penalty, result=result,
                                 reset=reset, agree=tune.AGREE["wgrad"])
        d.algo = _wa(algo)
    nbytes = lib.crdr_conv2d_wgrad_grouped_workspace(C.byref(d), G)
    e0 = _prof_begin()
    queued = []
    if defer:
        assert WGRAD_DEFER is not None, "this launch needs deferred weight-gradient reductions (ops.WGRAD_DEFER)"
        jobs = (L.WgradJob * G)()
        L.check(lib.crdr_conv2d_wgrad_partial_grouped(C.byref(d), pa, qa, ga, G, WGRAD_DEFER.alloc(nbytes), nbytes, jobs, _stream()),
                "conv2d_wgrad_partial_grouped")
        queued = [L.WgradJob.from_buffer_copy(jb) for jb in jobs]
        WGRAD_DEFER.jobs += queued
    else:
        ws, ws_n = workspace(nbytes, device)
        L.check(lib.crdr_conv2d_wgrad(C.byref(d), pa[0], qa[0], ga[0], ws, ws_n, _stream()), "conv2d_wgrad")
    _prof_end("wgrad", flops, e0, label)
    return queued


def conv_out_size(h, k, stride, pad, transposed, out_pad=0):
    if transposed:
        return (h - 1) * stride - 2 * pad + k + out_pad
    return (h + 2 * pad - k) // stride + 1


def conv2d_raw(x: torch.Tensor, wpack: torch.Tensor, oc: int, k: Tuple[int, int], stride: int, pad: int,
               transposed: bool, out_hw: Tuple[int, int], *, bias=None, flags: int = 0, vec2=None, res=None,
               scale=None, shift=None, gate_x=None, gate_t=None, sig_out=None, out: Optional[torch.Tensor] = None,
               algo: int = 0, wlayout: int = 0):
    """One fused implicit-GEMM launch. `out` may be a channel slice of a wider NHWC tensor (written in place).
    The input may be of any size (the kernel re-bases its buffer descriptor per workgroup)."""
    lib = L.load()
    flags |= _cf()
    x, ldx = nhwc(x)
    n, c, h, w = x.shape
    oh, ow = out_hw
    if out is None:
        out = empty_nhwc(n, oc, oh, ow, x.device)
    out_t, ldy = out, _pixel_stride(out)
    d = L.ConvDesc(N=n, H=h, W=w, C=(c + 3) // 4 * 4 if ldx >= (c + 3) // 4 * 4 else c, OH=oh, OW=ow, OC=oc, kh=k[0], kw=k[1],
                   stride=stride, pad=pad, transposed=int(transposed), ldx=ldx, ldy=ldy, wrows=wpack.shape[1],
                   wcols=wpack.shape[2], flags=flags, ldres=0, ldg=0, wlayout=wlayout, reserved=0)
    io = L.ConvIO(x=x.data_ptr(), w=wpack.data_ptr(), y=out_t.data_ptr(), bias=_p(bias), vec2=_p(vec2))
    if res is not None:
        res, d.ldres = nhwc(res)
        io.res = res.data_ptr()
    if scale is not None:
        io.scale, io.shift = scale.data_ptr(), shift.data_ptr()
    if gate_x is not None:
        gate_x, ldg = nhwc(gate_x)
        gate_t, ldg2 = nhwc(gate_t)
        if ldg != ldg2 or ldg != oc:
            gate_x, gate_t = dense_nhwc(gate_x), dense_nhwc(gate_t)
            ldg = oc
        d.ldg = ldg
        io.gx, io.gt, io.sig = gate_x.data_ptr(), gate_t.data_ptr(), sig_out.data_ptr()
    key = None if flags & L.EPI_ACCUM else ("c", n, h, w, d.C, oh, ow, oc, k, stride, pad, int(transposed), ldx, ldy, flags, d.ldres,
                                            d.ldg, wlayout)
    _conv(lib, d, (L.ConvIO * 1)(io), 1, key, x.device, algo=algo, trial_out=out_t,
          flops=2.0 * n * (h * w if transposed else oh * ow) * c * oc * k[0] * k[1],
          label=f"{'T' if transposed else 'C'} {c}->{oc} k{k[0]}s{stride} in{h}x{w} f{flags}",
          nbytes=4.0 * (n * h * w * c + n * oh * ow * oc * (1 + (res is not None) + 3 * (gate_x is not None)) + k[0] * k[1] * c * oc))
    return out


def conv2d_wgrad_raw(p: torch.Tensor, q: torch.Tensor, g: torch.Tensor, k, stride, pad, accumulate: bool, algo: int = 0,
                      defer: bool = True):
    """g[I][J][kh][kw] (+)= sum P[., i] * Q[gathered, j]; P is the dense operand (see crdr_hip.h).
    Operands that reach the 2 GiB span of the kernel's 32-bit buffer offsets are processed in batch halves."""
    lib = L.load()
    p, ldp = nhwc(p)
    q, ldq = nhwc(q)
    n, pc, ph, pw = p.shape
    _, qc, qh, qw = q.shape
    if n * ph * pw == 0:  # empty batch: the gradient contribution is zero
        if not accumulate:
            g.zero_()
        return g
    if n > 1 and max(n * ph * pw * ldp, n * qh * qw * ldq) * 4 >= _SPAN_LIMIT:
        n1 = n // 2
        conv2d_wgrad_raw(p[:n1], q[:n1], g, k, stride, pad, accumulate, algo=algo, defer=False)
        conv2d_wgrad_raw(p[n1:], q[n1:], g, k, stride, pad, True, algo=algo, defer=False)
        return g
    pc4 = min((pc + 3) // 4 * 4, ldp)
    qc4 = min((qc + 3) // 4 * 4, ldq)
    assert g.is_contiguous() and g.shape[0] <= pc4 and g.shape[1] <= qc4
    d = L.WgradDesc(N=n, PH=ph, PW=pw, PC=pc4, ldp=ldp, QH=qh, QW=qw, QC=qc4, ldq=ldq, kh=k[0], kw=k[1],
                    stride=stride, pad=pad, gI=g.shape[0], gJ=g.shape[1], accumulate=int(accumulate), algo=_wa(0))
    key = ("w", n, ph, pw, pc4, ldp, qh, qw, qc4, ldq, k, stride, pad, g.shape[0], g.shape[1]) + _mk()
    _wgrad(lib, d, 1, [p.data_ptr()], [q.data_ptr()], [g.data_ptr()], key, p.device, whole=True, algo=algo,
           defer=defer and WGRAD_DEFER is not None and WGRAD_DEFER.device == p.device,
           flops=2.0 * n * ph * pw * g.shape[0] * g.shape[1] * k[0] * k[1], label=f"W {g.shape[0]}x{g.shape[1]} k{k[0]}s{stride} p{ph}x{pw}")
    return g


class DeferredWgrad:
    """Weight-gradient reductions of a whole backward pass finished by ONE launch (crdr_wgrad_reduce_batched) instead of one small launch
    per layer.  Slabs come from a batched.BumpArena recycled at every flush, the job tables are batched.SiteTables, one pair per flush site
    and round: a site captured in a HIP graph (same layers, same buffers every iteration) replays without host work (rules: see batched)."""
    CAP = 4096

    def __init__(self, device, arena_bytes: int = 2 << 30):
        self.device = torch.device(device)
        self._arena = BumpArena(self.device, arena_bytes, "DeferredWgrad: arena")
        self.alloc = self._arena.alloc
        self.jobs = []
        self.tables = SiteTables(self.device, L.WgradJob, self.CAP, name="DeferredWgrad")

    def pending(self) -> int:
        return len(self.jobs)

    def drop(self) -> None:   # forget the pending jobs (an exception left them behind) and hand their slabs out again
        self.jobs = []
        self._arena.rewind()

    def flush(self, key=None) -> None:
        """Reduce everything pending; `key` names the flush site."""
        if not self.jobs:
            return
        rounds = []  # no two jobs of one launch may write the same gradient (a weight used twice in one backward)
        for jb in self.jobs:
            for r in rounds:
                if jb.g not in r[1]:
                    r[0].append(jb); r[1].add(jb.g)
                    break
            else:
                rounds.append(([jb], {jb.g}))
        for ri, (js, _) in enumerate(rounds):
            tb = self.tables.upload((key, ri), js, _wgrad_job_tiles)
            L.check(L.load().crdr_wgrad_reduce_batched(*tb.operands, _stream()), "wgrad_reduce_batched")
        self.jobs = []
        self._arena.reset()


def _wgrad_job_tiles(j) -> int:
    """tiles of crdr_wgrad_reduce_batched for one job: one output row x 64 input channels x all taps (RGB / many-tap jobs: 256 outputs)"""
    return (j.gI * j.gJ * j.T + 255) // 256 if (j.smallj or j.T > 32) else j.gI * ((j.gJ + 63) // 64)


def reduce_jobs_now(jobs, device) -> None:
    """One crdr_wgrad_reduce_batched launch over `jobs` (a ctypes array / list of WgradJob) with a throw-away device table: the
    tuner finishes a trial's partial slabs with it so that the candidate's weight gradient can be compared with the baseline's."""
    tb = JobTable(device, L.WgradJob, len(jobs), name="reduce_jobs_now").upload(jobs, _wgrad_job_tiles)
    L.check(L.load().crdr_wgrad_reduce_batched(*tb.operands, _stream()), "wgrad_reduce_batched")
    torch.cuda.current_stream().synchronize()   # (the table dies with this frame)


WGRAD_DEFER: Optional[DeferredWgrad] = None  # set by a trainer; every backward must then be followed by flush_wgrads()


_local_defers = {}


@contextlib.contextmanager
def local_wgrad_defer(device, site):
    """Around a hand-written backward whose slab launches defer their reductions.  A trainer already defers on this device: nothing to do,
    the trainer flushes.  Otherwise the device's private DeferredWgrad stands in: flushed at `site` on the way out, its pending jobs
    dropped when the backward raises (the next one must not reduce stale slabs); the previous value is restored either way."""
    global WGRAD_DEFER
    prev = WGRAD_DEFER
    if prev is not None and prev.device == device:
        yield
        return
    d = _local_defers.get(device)
    if d is None:
        d = _local_defers[device] = DeferredWgrad(device, arena_bytes=256 << 20)
    WGRAD_DEFER = d
    try:
        yield
        d.flush(site)
    except BaseException:
        d.drop()
        raise
    finally:
        WGRAD_DEFER = prev


def flush_wgrads(key=None) -> None:
    if WGRAD_DEFER is not None:
        WGRAD_DEFER.flush(key)


def pending_wgrads() -> int:
    return WGRAD_DEFER.pending() if WGRAD_DEFER is not None else 0


def colsum(x: torch.Tensor, out: torch.Tensor, accumulate: bool):
    lib = L.load()
    x, ld = nhwc(x)
    n, c, h, w = x.shape
    m = n * h * w
    nbytes = lib.crdr_colsum_workspace(m, c)
    ws, ws_n = workspace(nbytes, x.device)
    L.check(lib.crdr_colsum(x.data_ptr(), ld, m, c, out.data_ptr(), int(accumulate), ws, ws_n, _stream()), "colsum")
    return out


def epilogue_bwd(dout, out, flags, *, vec2=None, scale=None, shift=None, gate_t=None, sig=None, need_dz=True,
                 dbias_accum: Optional[torch.Tensor] = None):
    """Returns (dz, gres, dgt, colsums[4][C]); `dbias_accum` [C] additionally receives += sum dz inside the same launch."""
    lib = L.load()
    dout, lddout = nhwc(dout)
    n, c, h, w = dout.shape
    m = n * h * w
    d = L.EbwdDesc(M=m, C=c, flags=flags, lddout=lddout, ldout=0, lddz=ld_for(c), ldgres=ld_for(c), ldg=c)
    io = L.EbwdIO(dout=dout.data_ptr(), vec2=_p(vec2), scale=_p(scale), shift=_p(shift))
    if out is not None:
        out, d.ldout = nhwc(out)
        io.out = out.data_ptr()
    dz = gres = dgt = None
    if need_dz:
        dz = empty_nhwc(n, c, h, w, dout.device)
        io.dz = dz.data_ptr()
    if flags & L.EPI_GATE:
        gate_t, ldg = nhwc(gate_t)
        sig, ldg2 = nhwc(sig)
        assert ldg == c and ldg2 == c
        io.gt, io.sig = gate_t.data_ptr(), sig.data_ptr()
        gres = empty_nhwc(n, c, h, w, dout.device)
        dgt = empty_nhwc(n, c, h, w, dout.device)
        io.gres, io.dgt = gres.data_ptr(), dgt.data_ptr()
    elif (flags & L.EPI_AFFINE) and (flags & L.EPI_RES):
        gres = empty_nhwc(n, c, h, w, dout.device)
        io.gres = gres.data_ptr()
    colsums = torch.empty((4, c), dtype=torch.float32, device=dout.device)
    io.colsums = colsums.data_ptr()
    if dbias_accum is not None:
        assert dbias_accum.is_contiguous() and dbias_accum.numel() == c
        io.dbias_accum = dbias_accum.data_ptr()
    nbytes = lib.crdr_epilogue_bwd_workspace(C.byref(d))
    ws, ws_n = workspace(nbytes, dout.device)
    L.check(lib.crdr_epilogue_bwd(C.byref(d), C.byref(io), ws, ws_n, _stream()), "epilogue_bwd")
    return dz, gres, dgt, colsums


# ---------------------------------------------------------------------------------------------------------
# pointer-level launchers (used by the fused Charm engine, crdr_amd/hip/charm.py): operands are (address, pixel stride)
# pairs into wide NHWC buffers owned by the caller -- no layout checks, no allocation, no autograd.
# ---------------------------------------------------------------------------------------------------------
class V:
    """A channel range of a wide NHWC buffer: address of channel 0 of pixel 0, pixel stride, channel count."""
    __slots__ = ("ptr", "ld", "c")

    def __init__(self, ptr: int, ld: int, c: int):
        self.ptr, self.ld, self.c = ptr, ld, c


def view(buf: torch.Tensor, c0: int, c: int) -> V:
    """Channels [c0, c0 + c) of a dense [pixels..., ld] buffer (last dim = pixel stride)."""
    return V(buf.data_ptr() + 4 * c0, buf.shape[-1], c)


def _conv_ios(xs, wpacks, ys, biases=None, pres=None, masks=None, ress=None, vec2=None, scale=None, shift=None):
    """ConvIO array of a grouped launch: xs / ys / pres / masks / ress lists of V, wpacks / biases lists of addresses, vec2 / scale /
    shift addresses shared by the group"""
    ios = (L.ConvIO * len(xs))()
    for g, io in enumerate(ios):
        io.x, io.w, io.y, io.vec2 = xs[g].ptr, wpacks[g], ys[g].ptr, vec2
        if biases is not None:
            io.bias = biases[g]
        if pres is not None:
            io.pre = pres[g].ptr
        if masks is not None:
            io.mask = masks[g].ptr
        if ress is not None:
            io.res = ress[g].ptr
        if scale is not None:
            io.scale, io.shift = scale, shift
    return ios


def conv_group(n: int, h: int, w: int, xs, wpacks, ys, oc: int, k: Tuple[int, int], pad: int, transposed: bool, *,
               wrows: int, wcols: int, biases=None, pres=None, masks=None, flags: int = 0, device=None, label: str = "",
               plan_as: Optional[int] = None):
    """G stride-1 'same' convolutions of one geometry in one launch (crdr_conv2d_grouped; G = 1: crdr_conv2d).
    xs / ys / pres / masks: lists of V (equal ld and c within each list); wpacks / biases: lists of addresses.
    plan_as: run with the tile configuration / split depth a launch of `plan_as` problems would get (same fp32 summation order
    as that launch: the Charm's mean-only pass reproduces the mean transforms of the full pass bit for bit)."""
    lib = L.load()
    G = len(xs)
    x0, y0 = xs[0], ys[0]
    if biases is not None:
        flags |= L.EPI_BIAS
    if pres is not None:
        flags |= L.EPI_PREADD
    if masks is not None:
        flags |= L.EPI_RELUMASK
    # a pure accumulation y += conv(x) is the residual epilogue with the output as its own residual operand (the same single
    # add, bit for bit): that form takes the straight-line buffer-op epilogue, CRDR_EPI_ACCUM the general one
    self_res = flags == L.EPI_ACCUM
    if self_res:
        flags = L.EPI_RES
    flags |= _cf()
    d = L.ConvDesc(N=n, H=h, W=w, C=x0.c, OH=h, OW=w, OC=oc, kh=k[0], kw=k[1], stride=1, pad=pad, transposed=int(transposed),
                   ldx=x0.ld, ldy=y0.ld, wrows=wrows, wcols=wcols, flags=flags, ldres=y0.ld if self_res else 0, ldg=0, wlayout=0, reserved=0,
                   ldpre=pres[0].ld if pres is not None else 0, ldmask=masks[0].ld if masks is not None else 0)
    ios = _conv_ios(xs, wpacks, ys, biases, pres, masks, ys if self_res else None)
    GP = plan_as or G
    key = ("g", GP, n, h, w, d.C, oc, k, pad, int(transposed), d.ldx, d.ldy, flags, d.ldpre, d.ldmask, wrows, wcols)
    _conv(lib, d, ios, G, key, device, plan_as=GP,
          flops=2.0 * G * n * h * w * x0.c * oc * k[0] * k[1],
          label=f"{'T' if transposed else 'C'} {G}x {x0.c}->{oc} k{k[0]} in{h}x{w} f{flags} {label}",
          nbytes=4.0 * G * (n * h * w * x0.c + n * h * w * oc * (1 + (pres is not None) + (masks is not None) + bool(flags & L.EPI_ACCUM))
                            + k[0] * k[1] * x0.c * oc))


def wgrad_group(n: int, h: int, w: int, ps, qs, gs, gi: int, gj: int, k: Tuple[int, int], pad: int, *, device, accumulate=True,
                label: str = ""):
    """G stride-1 weight gradients of one geometry in one slab launch, reductions deferred (WGRAD_DEFER must be active).
    ps / qs: lists of V (dense operand = output gradient, gathered operand = layer input); gs: list of
    (address of g[0][j0][0], gJtot) -- the job writes g[i][j0 + j][t], i < gi, j < gj, of a parameter whose second dim is
    gJtot.  Returns nothing; the jobs are queued on WGRAD_DEFER."""
    lib = L.load()
    G = len(ps)
    p0, q0 = ps[0], qs[0]
    d = L.WgradDesc(N=n, PH=h, PW=w, PC=p0.c, ldp=p0.ld, QH=h, QW=w, QC=q0.c, ldq=q0.ld, kh=k[0], kw=k[1], stride=1, pad=pad,
                    gI=gi, gJ=gj, accumulate=int(accumulate), algo=_wa(0))
    key = ("wg", G, n, h, w, p0.c, p0.ld, q0.c, q0.ld, k, pad, gi, gj) + _mk()
    jobs = _wgrad(lib, d, G, [v.ptr for v in ps], [v.ptr for v in qs], [g[0] for g in gs], key, device,
                  flops=2.0 * G * n * h * w * gi * gj * k[0] * k[1], label=f"W {G}x {gi}x{gj} k{k[0]} p{h}x{w} {label}")
    for jb, g in zip(jobs, gs):
        jb.gJtot = g[1]


def wgrad_split(n: int, h: int, w: int, p: V, q: V, parts, k: Tuple[int, int], pad: int, *, device, label: str = ""):
    """ONE slab launch whose rows feed several parameters: P = a wide output-gradient range (p.c channels = the
    concatenated outputs of several convs that read the same input q), parts = [(row0, rows, address of g[0][j0][0],
    gJtot)]: rows [row0, row0 + rows) of the slab reduce into g[i][j0 + j][t], j < q.c."""
    lib = L.load()
    d = L.WgradDesc(N=n, PH=h, PW=w, PC=p.c, ldp=p.ld, QH=h, QW=w, QC=q.c, ldq=q.ld, kh=k[0], kw=k[1], stride=1, pad=pad,
                    gI=p.c, gJ=q.c, accumulate=1, algo=_wa(0))
    key = ("ws", n, h, w, p.c, p.ld, q.c, q.ld, k, pad) + _mk()
    job, = _wgrad(lib, d, 1, [p.ptr], [q.ptr], [parts[0][2]], key, device, whole=True,
                  flops=2.0 * n * h * w * p.c * q.c * k[0] * k[1], label=f"W {p.c}x{q.c} k{k[0]} p{h}x{w} {label}")
    split = []
    for row0, rows, gptr, gjtot in parts:
        jb = L.WgradJob.from_buffer_copy(job)
        jb.slab = job.slab + 4 * row0 * q.c
        jb.g, jb.gI, jb.gJtot = gptr, rows, gjtot
        split.append(jb)
    WGRAD_DEFER.jobs[-1:] = split   # (the slab's one job becomes one job per part)


def colsum_scatter(x: V, m: int, block: int, outs_table: torch.Tensor, device, accumulate: bool = True):
    """outs_table: device int64 tensor of ceil(x.c / block) addresses (0 = skip)."""
    lib = L.load()
    nbytes = lib.crdr_colsum_workspace(m, x.c)
    ws, ws_n = workspace(nbytes, device)
    L.check(lib.crdr_colsum_scatter(x.ptr, x.ld, m, x.c, block, outs_table.data_ptr(), int(accumulate), ws, ws_n, _stream()),
            "colsum_scatter")


# ---------------------------------------------------------------------------------------------------------
# general pointer-level conv launch (any stride / transposed / group size / epilogue) + in-epilogue column sums
# ---------------------------------------------------------------------------------------------------------
class ColsumQueue:
    """Pending CRDR_EPI_COLSUM reductions of one device, finished by ONE crdr_colsum_finish_batched launch per flush.  Same scheme as
    DeferredWgrad (rules: see batched): partial rows from a BumpArena recycled at every flush, SiteTables per flush site; the pass-A scratch
    is offset-addressed and its address is the tables' trailer (a captured finish launch carries it as a kernel argument)."""
    CAP = 512

    def __init__(self, device, arena_bytes: int = 128 << 20):
        self.device = torch.device(device)
        self._arena = BumpArena(self.device, arena_bytes, "ColsumQueue: arena")
        self._scratch = BumpArena(self.device, 16 << 20, "ColsumQueue: scratch")
        self.scratch_off = 0   # floats of pass-A scratch handed out since the last flush
        self.jobs = []
        self.tables = SiteTables(self.device, L.ColsumJob, self.CAP, rows=2, name="ColsumQueue")

    arena = property(lambda self: self._arena.tensor)   # the uint8 tensor that the partial rows handed out since the last growth live in

    def alloc(self, nfloats: int) -> int:
        return self._arena.alloc(4 * nfloats)

    def add(self, cs_ptr: int, rows: int, ld: int, c: int, out_pre: Optional[int], out_post: Optional[int], accumulate: bool):
        slab = L.load().crdr_colsum_slab_rows()
        nslab, cpad = (rows + slab - 1) // slab, (c + 63) // 64 * 64
        off = self.scratch_off
        self.scratch_off += nslab * 2 * cpad
        self.jobs.append(L.ColsumJob(cs=cs_ptr, out_pre=out_pre, out_post=out_post, rows=rows, ld=ld, C=c, accumulate=int(accumulate),
                                     nslab=nslab, cpad=cpad, scratch_off=off))

    def drop(self) -> None:   # forget the pending jobs and hand their partial rows out again
        self.jobs, self.scratch_off = [], 0
        self._arena.rewind()

    def flush(self, key) -> None:
        if self.jobs:
            scratch = self._scratch.reserve(4 * self.scratch_off)
            tb = self.tables.upload(key, self.jobs, lambda j: ((j.cpad // 64) * j.nslab, j.cpad // 64),   # pass-A tiles, pass-B tiles
                                    trailer=scratch.to_bytes(8, "little"))
            L.check(L.load().crdr_colsum_finish_batched(*tb.operands, scratch, _stream()), "colsum_finish_batched")
        self.jobs, self.scratch_off = [], 0
        self._arena.reset()
        self._scratch.reset()


_colsum_queues = {}


def colsum_queue(device) -> ColsumQueue:
    dev = torch.device(device)
    dev = torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev
    q = _colsum_queues.get(dev)
    if q is None:
        q = _colsum_queues[dev] = ColsumQueue(dev)
    return q


def conv_multi(n: int, h: int, w: int, oh: int, ow: int, xs, wpacks, ys, oc: int, k: Tuple[int, int], stride: int, pad: int,
               transposed: bool, *, wrows: int, wcols: int, biases=None, pres=None, masks=None, ress=None, vec2=None, scale=None,
               shift=None, flags: int = 0, colsum: bool = False, wlayout: int = 0, device=None, label: str = ""):
    """G convolutions of one geometry in one launch, any stride / direction / epilogue (see crdr_conv2d_grouped for what a
    grouped launch may carry).  xs / ys / pres / masks / ress: lists of V; wpacks / biases: addresses; vec2 / scale / shift:
    addresses shared by the group (G = 1 only).  colsum=True adds CRDR_EPI_COLSUM and returns [(cs address, rows, ld)] per
    problem for colsum_queue(device).add (the partial rows live in that queue's arena until its next flush)."""
    lib = L.load()
    G = len(xs)
    x0, y0 = xs[0], ys[0]
    if biases is not None:
        flags |= L.EPI_BIAS
    if pres is not None:
        flags |= L.EPI_PREADD
    if ress is not None:
        flags |= L.EPI_RES
    if scale is not None:
        flags |= L.EPI_AFFINE
    if colsum:
        flags |= L.EPI_COLSUM
    flags |= _cf()
    cin = min((x0.c + 3) // 4 * 4, x0.ld)  # RGB / single-channel operands: the zeroed padding lanes ride along
    d = L.ConvDesc(N=n, H=h, W=w, C=cin, OH=oh, OW=ow, OC=oc, kh=k[0], kw=k[1], stride=stride, pad=pad, transposed=int(transposed),
                   ldx=x0.ld, ldy=y0.ld, wrows=wrows, wcols=wcols, flags=flags, ldres=ress[0].ld if ress is not None else 0, ldg=0,
                   wlayout=wlayout, reserved=0, ldpre=pres[0].ld if pres is not None else 0,
                   ldmask=masks[0].ld if masks is not None else 0)
    ios = _conv_ios(xs, wpacks, ys, biases, pres, masks, ress, vec2, scale, shift)
    key = ("m", G, n, h, w, oh, ow, d.C, oc, k, stride, pad, int(transposed), d.ldx, d.ldy, flags, d.ldres, d.ldpre, d.ldmask,
           wrows, wcols, wlayout)
    return _conv(lib, d, ios, G, key, device, colsum=colsum,
                 flops=2.0 * G * n * (h * w if transposed else oh * ow) * x0.c * oc * k[0] * k[1],
                 label=f"{'T' if transposed else 'C'} {G}x {x0.c}->{oc} k{k[0]}s{stride} in{h}x{w} f{flags} {label}",
                 nbytes=4.0 * G * (n * h * w * x0.c + n * oh * ow * oc * (1 + (pres is not None) + (masks is not None) + (ress is not None)
                                                                          + bool(flags & L.EPI_ACCUM)) + k[0] * k[1] * x0.c * oc))


def wgrad_multi(n: int, ph: int, pw: int, qh: int, qw: int, ps, qs, gs, gi: int, gj: int, k: Tuple[int, int], stride: int, pad: int, *,
                device, label: str = ""):
    """G weight gradients of one geometry (any stride), reductions deferred: ps = dense operands (V), qs = gathered operands
    (V), gs = gradient addresses (full parameters [gi][gj][kh][kw], accumulated)."""
    lib = L.load()
    G = len(ps)
    p0, q0 = ps[0], qs[0]
    pc, qc = min((p0.c + 3) // 4 * 4, p0.ld), min((q0.c + 3) // 4 * 4, q0.ld)
    d = L.WgradDesc(N=n, PH=ph, PW=pw, PC=pc, ldp=p0.ld, QH=qh, QW=qw, QC=qc, ldq=q0.ld, kh=k[0], kw=k[1], stride=stride, pad=pad,
                    gI=gi, gJ=gj, accumulate=1, algo=_wa(0))
    key = ("wm", G, n, ph, pw, pc, p0.ld, qh, qw, qc, q0.ld, k, stride, pad, gi, gj) + _mk()
    _wgrad(lib, d, G, [v.ptr for v in ps], [v.ptr for v in qs], gs, key, device,
           flops=2.0 * G * n * ph * pw * gi * gj * k[0] * k[1], label=f"W {G}x {gi}x{gj} k{k[0]}s{stride} p{ph}x{pw} {label}")
