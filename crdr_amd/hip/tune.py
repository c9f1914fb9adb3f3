"""The per-shape autotuner, the analogue of the reference's `cudnn.benchmark = True` (base_trainer.py:20): the ids it enumerates, its timer, the
agreement gate, and the perf database its choices persist in.  What is tuned -- keys, trial operands, the switches -- is decided in ops."""
import ast
import functools
import json
import os
import types

import torch

from . import lib as L
from .batched import _capturing

# The containers below are only ever mutated, never rebound: ops (and through it bench.py) holds aliases of them.
algo_cache = {}   # {shape key: forced algorithm id}
DEFAULT_DB = os.path.join(os.path.dirname(__file__), "tune_gfx950.json")   # the perf database that ships in-tree (save / load below)
LOG = []          # (key, chosen id, ms of the built-in plan, ms of the chosen one) of every key tuned on the spot
ROUNDS = int(os.environ.get("CRDR_TUNE_ROUNDS", "1"))  # >1: best of several timings (perf-database builds)
# CRDR_TUNE_COLD=1: evict L2 / Infinity Cache (a 512 MB read-modify-write) before every timed launch.  Inside a training step
# a conv finds its weights and activations cold -- the producer ran on other XCDs, 100+ MB of other tensors ago -- while
# back-to-back timing of one launch measures the cache-warm case, which favours configurations with more, smaller loads.
COLD = os.environ.get("CRDR_TUNE_COLD", "0") == "1"
_evict = None


def time_call(fn, reps: int = 2) -> float:
    """ms per launch of fn() after one untimed call, best of ROUNDS.  Warm: one event pair around `reps` back-to-back launches.  COLD: an
    event pair per launch, each after an eviction, mean over `reps`."""
    global _evict
    if COLD and _evict is None:
        _evict = torch.zeros(128 << 20, dtype=torch.float32, device="cuda")
    fn()
    best = float("inf")
    for _ in range(max(1, ROUNDS)):
        tot = 0.0
        for _ in range(reps if COLD else 1):
            if COLD:
                _evict.add_(1.0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(1 if COLD else reps):
                fn()
            e1.record()
            e1.synchronize()
            tot += e0.elapsed_time(e1)
        best = min(best, tot / reps)
    return best


@functools.lru_cache(maxsize=None)
def ids():
    """Where the kernel families sit among the forced-algorithm ids (layout: csrc/algo_id.hpp), read from the library once.  Library constants
    only: what the switches ops.WINOGRAD / ops.WINO4 leave of them is decided where a list is asked for.  -1: the library has no such kernel.
    (crdr_conv2d_wgrad_num_configs() counts the F(2x2) slab kernel: the F(4x4) one is the id behind it.)"""
    lib = L.load()
    n, ns, nw = lib.crdr_conv2d_num_configs(), lib.crdr_conv2d_num_stream_configs(), lib.crdr_conv2d_num_wino_configs()
    return types.SimpleNamespace(stream=tuple(range(n + 1, n + 1 + ns)), wino=tuple(range(n + 1 + ns, n + 1 + ns + nw)), wino4=n + ns + 3 if nw > 2 else -1,
                                 wgrad_wino4=lib.crdr_conv2d_wgrad_num_configs() + 1 if lib.crdr_conv2d_wgrad_num_wino_configs() >= 2 else -1)


def tile_id(cfg: int, log2_split: int = 0) -> int:   # forced id of tile configuration `cfg` (conv or weight gradient) split 2^log2_split ways
    return (cfg + 1) | (log2_split << 8)


# A candidate may only win if its result agrees with the baseline plan's (algo 0, the built-in plan the parity tests run) on the
# very operands it is timed on: max |candidate - baseline| <= AGREE[kind] x max |baseline|.  Two correct plans differ by fp32
# summation order only (measured over every entry of the shipped database: profiles/r4_plan_replay.json); a mis-tiled edge, a
# wrong split reduce or a stale workspace is orders of magnitude above that and must not ship because it is fast.
AGREE = {"conv": 2e-5, "wgrad": 2e-4, "wino4": 2e-5}   # wino4: the F(4x4, 3x3) Winograd kernel (round 5 points 0, +-3/4, +-5/4: 0.4e-6 .. 5e-6 of
#                                                         the output scale against float64, tests/test_gpu_wino.py; 6e-5 with round 4's 0, +-1, +-2)
REJECTED = []   # (key, algo, measured disagreement) of every candidate refused
SKIPPED = []    # keys whose tuning was put off because the call's result was all zero (no scale to compare candidates against)
ZERO_RETRIES = 3   # ... at most this often per key; then the built-in plan is cached for it
_zero_seen = {}


def autotune(key, ncfg: int, max_log2_split: int, run, extra=(), penalty=None, result=None, reset=None, agree: float = 2e-5) -> int:
    """run(algo) -> bool (False if the library rejects the combination). Returns the fastest algo id.  penalty() -> ms added to
    the candidate just timed: cost the launch causes elsewhere (the batched reduce reads every partial slab a weight-gradient
    launch writes, so a deeper pixel split that is 1 % faster in isolation can cost more than it gains).
    result() -> the tensor the launch just wrote (for weight-gradient slab launches: after their reduce); reset() restores the
    operands a launch reads AND writes (accumulating epilogues) before a run whose result is compared."""
    def fresh(a):
        if reset is not None:
            reset()
        return run(a)
    if _capturing():
        return 0   # timing needs host syncs: a key first seen under capture runs the built-in plan (and is tuned by a later eager call)
    fresh(0)
    ref = result().detach().clone() if result is not None else None
    ref_scale = float(ref.abs().max()) if ref is not None else 0.0
    if ref is not None and not ref_scale > 1e-30:
        # the operands of this call happen to give an all-zero (or denormal) result -- a zero gradient at warm-up, a masked branch: nothing
        # can be compared against it, and caching the baseline plan for the key would silently de-tune it.  Keep the built-in plan for THIS
        # call only; the next call with the same key tunes on its own operands.
        SKIPPED.append(key)
        _zero_seen[key] = _zero_seen.get(key, 0) + 1
        if _zero_seen[key] >= ZERO_RETRIES:   # persistently zero (a masked branch, a zero-initialised layer): stop paying a launch, a clone and
            algo_cache[key] = 0               # a host sync per call -- the built-in plan is cached and reported
            LOG.append((key, 0, 0.0, 0.0))
        return 0
    best, best_t = 0, time_call(lambda: run(0)) + (penalty() if penalty else 0.0)
    base_t = best_t
    for algo in [tile_id(c, ls) for c in range(ncfg) for ls in range(max_log2_split + 1)] + list(extra):
        try:
            if not fresh(algo):
                continue
            if ref is not None:
                dis = float((result() - ref).abs().max())
                tol = AGREE["wino4"] if ((algo & 0xff) == ids().wino4 and key[0] in ("c", "g", "m")) else agree
                if not dis <= tol * ref_scale:   # (NaN fails too)
                    REJECTED.append((key, algo, dis / (ref_scale + 1e-30)))
                    continue
            t = time_call(lambda: run(algo)) + (penalty() if penalty else 0.0)
        except L.CrdrHipError:
            continue
        if t < best_t:
            best, best_t = algo, t
    algo_cache[key] = best
    LOG.append((key, best, base_t, best_t))
    return best


def scratch(nfloats: int, device):
    """-> (scratch output tensor for tuner trials, reset() that restores its fixed pseudo-random content: accumulating epilogues
    read what they write, and a result is only comparable between plans if both started from the same content)"""
    buf = torch.empty(nfloats, dtype=torch.float32, device=device)
    pattern = torch.rand(nfloats, dtype=torch.float32, device=device) - 0.5
    return buf, (lambda: buf.copy_(pattern))


def signature() -> str:
    lib = L.load()
    return (f"v{lib.crdr_version()}-c{lib.crdr_conv2d_num_configs()}-s{lib.crdr_conv2d_num_stream_configs()}"
            f"-w{lib.crdr_conv2d_wgrad_num_configs()}+{lib.crdr_conv2d_wgrad_num_wino_configs() - 1}-n{lib.crdr_conv2d_num_wino_configs()}")


def save(path: str) -> None:
    """Persist the autotuner's choices (a perf database in the MIOpen sense): {repr(shape key): algo id}."""
    with open(path, "w") as f:
        json.dump({"signature": signature(), "algos": {repr(k): v for k, v in algo_cache.items()}}, f, indent=0)


def load(path: str, only_kinds=None, ignore_signature: bool = False, skip=None) -> int:
    """Load choices written by save(); ignored (returns 0) if the library's configuration list has changed.
    only_kinds / ignore_signature: seed a rebuild of the database with the entries of kernel families that did not change
    (key[0]: "c" / "g" / "m" conv launches, "w" / "wm" weight gradients)."""
    if not os.path.exists(path):
        return 0
    with open(path) as f:
        db = json.load(f)
    if db.get("signature") != signature() and not ignore_signature:
        return 0
    n = 0
    for k, v in db["algos"].items():
        key = ast.literal_eval(k)
        if (only_kinds is not None and key[0] not in only_kinds) or (skip is not None and skip(key)):
            continue   # (skip: entries the caller wants timed again, e.g. shapes a new kernel applies to)
        algo_cache.setdefault(key, int(v))
        n += 1
    return n
