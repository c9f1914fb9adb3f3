from typing import Dict

import torch
import torch.nn as nn
from torch import Tensor


class ContextRuntime:
    """What every object a model uses as its `context_model` carries besides its arithmetic: the state of the in-kernel noise
    generator (the trainers seed it per rank and checkpoint it) and the codec's wall-time ticks and pinned staging buffers."""

    # ---- noise: Philox state (seed, offset) on the device; the fused kernels draw U(-1/2, 1/2) from it and the backward
    # regenerates the same samples (crdr_gauss_cond_fwd2).  Seeded per rank by the trainer (seed_noise).
    def _philox(self, device) -> Tensor:
        st = getattr(self, "_philox_state", None)
        if st is None or st.device != device:
            seed = getattr(self, "_noise_seed", None)
            if seed is None:   # never seeded by a trainer: still one stream per rank
                from crdr_amd.trainer import dist as _D
                seed = (torch.initial_seed() + 7919 * (_D.rank() + 1)) & 0x7FFFFFFFFFFFFFFF
            st = torch.tensor([int(seed), int(getattr(self, "_noise_offset", 0))], dtype=torch.int64, device=device)
            self._philox_state = st
        return st

    def seed_noise(self, seed: int, offset: int = 0) -> None:
        self._noise_seed = int(seed) & 0x7FFFFFFFFFFFFFFF
        self._noise_offset = int(offset)
        self._philox_state = None

    def noise_state(self) -> Dict:
        """(seed, offset) of the in-kernel noise generator, for the trainer's checkpoint: a resumed run continues the
        sequence instead of replaying it from offset 0.  Synchronises."""
        st = getattr(self, "_philox_state", None)
        if st is None:
            return {"seed": getattr(self, "_noise_seed", None), "offset": int(getattr(self, "_noise_offset", 0))}
        seed, off = st.tolist()
        return {"seed": int(seed), "offset": int(off)}

    def load_noise_state(self, state: Dict) -> None:
        if state and state.get("seed") is not None:
            self.seed_noise(state["seed"], state.get("offset", 0))

    # ---- codec paths (GPU transforms, host rANS)
    codec_profile = None  # shared with the model's compress / decompress (wall-time split {charm, rans})

    def _tick(self, key, t0=None):
        import time
        if self.codec_profile is None:
            return 0.0
        torch.cuda.synchronize()
        t = time.perf_counter()
        if key is not None:
            self.codec_profile[key] = self.codec_profile.get(key, 0.0) + (t - t0)
        return t

    def _pinned_pair(self, shape):
        """Two pinned int32 host buffers of (at least) `shape` elements, kept per thread (decompress_many decodes several images
        concurrently, one thread and one stream each)."""
        import threading
        cache = self.__dict__.setdefault("_pin_cache", {})
        key = threading.get_ident()
        need = 1
        for d in shape:
            need *= int(d)
        pair = cache.get(key)
        if pair is None or pair[0].numel() < need:
            pair = cache[key] = (torch.empty(need, dtype=torch.int32, pin_memory=True), torch.empty(need, dtype=torch.int32, pin_memory=True))
        return pair


class BaseContextModel(ContextRuntime, nn.Module):
    def __init__(self, **kwargs):
        super().__init__()
