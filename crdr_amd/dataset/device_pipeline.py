"""Device-side training input pipeline (reference: data_transform.py:19-73 + base_trainer.py:74-80).

The reference decodes a JPEG, pads / crops / flips it with torchvision and normalises it, per sample, in 8 DataLoader
workers.  On an MI355X the decoded images of a training set fit in HBM (288 GB: ~370 k RGB images of 512x512), so the
pool is decoded ONCE into a flat uint8 buffer on the device and every batch is cut by one launch
(`crdr_crop_flip_normalize`) straight into NHWC fp32 -- no host pixels move per step; without `resize_range` only the 6
integers per sample that describe the random draw do.  The draws follow torchvision's semantics: `RandomCrop(size,
pad_if_needed=True, padding_mode='reflect')` pads BOTH sides by (size - dim) when a side is too short, the crop origin is
uniform over the padded image, and the flip has probability 0.5.

With `resize_range=(f_min, f_max)` the reference's `PilRandomResize` (data_transform.py:54-73) runs first: a scale is drawn
from U(low, high), low = max(size / min(h, w), f_min), high = max(low, f_max), and the WHOLE image is resized by PIL to
(int(w * scale), int(h * scale)) before the crop.  Here only the crop window of the resized image is computed, by
`crdr_resize_crop_flip_normalize`, in the integer arithmetic of PIL's 8-bit resampler and therefore bit-equal to it.  The
host's share is `resize_tables`: PIL's coefficient tables (Resample.c precompute_coeffs + normalize_coeffs_8bpc, float64)
for the `size` crop rows and `size` crop columns of each sample, with the reflect padding of the resized image and the
flip resolved into the order of the entries.  Per batch one int32 buffer goes up in one copy: 4 integers per sample (pool
offset, H, W) and 2 * size * (2 + taps) table integers per sample, taps = the widest entry of the batch (<= KMAX).  At
bs 16, size 256 that is 360,704 bytes for a [0.5, 1.0] bicubic batch (9 taps), 98,560 bytes at scale 1.0 (1 tap) and
622,848 bytes at the KMAX = 17 taps of a 4x bicubic down-scale."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from crdr_amd.hip import lib as L
from crdr_amd.hip import ops

KMAX = 17                  # taps per table entry the kernel takes (csrc/resize_crop.hip RC_KMAX): a 4x bicubic / 8x bilinear down-scale
PRECISION_BITS = 22        # PIL's 8-bit resampler: 32 - 8 - 2
FILTER_SUPPORT = {"bicubic": 2.0, "bilinear": 1.0}   # the reference's choices (data_transform.py:60-63)


def draw_crops(shapes: Sequence[Sequence[int]], idx: np.ndarray, size: int, rng: np.random.Generator) -> np.ndarray:
    """-> int64 [len(idx)][5] = (H, W, sy0, sx0, flip) for the images `idx` (crop origin in un-padded coordinates)."""
    out = np.zeros((len(idx), 5), dtype=np.int64)
    for k, i in enumerate(idx):
        h, w = shapes[i]
        ph, pw = max(0, size - h), max(0, size - w)            # padding added on BOTH sides (torchvision F.pad [p, p])
        assert ph < h and pw < w, "reflect padding needs pad < image side"
        y0 = int(rng.integers(0, h + 2 * ph - size + 1))
        x0 = int(rng.integers(0, w + 2 * pw - size + 1))
        out[k] = (h, w, y0 - ph, x0 - pw, int(rng.random() < 0.5))
    return out


def scale_bounds(h: int, w: int, size: int, resize_range: Tuple[float, float]) -> Tuple[float, float]:
    """PilRandomResize's (scale_low, scale_high) for an h x w image (data_transform.py:65-70)."""
    low = max(float(size) / float(min(h, w)), resize_range[0])
    return low, max(low, resize_range[1])


def draw_resized_crops(shapes: Sequence[Sequence[int]], idx: np.ndarray, size: int, rng: np.random.Generator,
                       resize_range: Tuple[float, float]) -> np.ndarray:
    """-> float64 [len(idx)][6] = (scale, RH, RW, sy0, sx0, flip): the scale, the size of the resized image (the float truncation
    of the reference: RH can come out one below `size` at the minimum scale) and `draw_crops`' rule on (RH, RW)."""
    out = np.zeros((len(idx), 6), dtype=np.float64)
    for k, i in enumerate(idx):
        h, w = shapes[i]
        low, high = scale_bounds(h, w, size, resize_range)
        scale = float(rng.uniform(low, high))
        rh, rw = int(h * scale), int(w * scale)
        ph, pw = max(0, size - rh), max(0, size - rw)
        assert ph < rh and pw < rw, "reflect padding needs pad < image side"
        y0 = int(rng.integers(0, rh + 2 * ph - size + 1))
        x0 = int(rng.integers(0, rw + 2 * pw - size + 1))
        out[k] = (scale, rh, rw, y0 - ph, x0 - pw, int(rng.random() < 0.5))
    return out


def max_taps(in_size: int, out_size: int, interpolation: str) -> int:
    """Upper bound of the taps of one output sample: xmax - xmin <= floor(2 * support) + 1."""
    if in_size == out_size:
        return 1
    return int(2.0 * FILTER_SUPPORT[interpolation] * max(in_size / out_size, 1.0)) + 1


def _filter(t: np.ndarray, interpolation: str) -> np.ndarray:
    """Resample.c bilinear_filter / bicubic_filter (a = -0.5), the operations in their order; multiplying by a comparison's 0 / 1 is exact"""
    x = np.abs(t, out=t)
    if interpolation == "bilinear":
        return (1.0 - x) * (x < 1.0)
    a = -0.5
    near = x < 1.0
    inner = (((a + 2.0) * x - (a + 3.0)) * x * x + 1) * near
    outer = (((x - 5) * x + 8) * x - 4) * a * ((x < 2.0) & ~near)
    return inner + outer                                                   # one of the two is a zero: the sum is the other, exactly


def axis_tables(in_size: np.ndarray, out_size: np.ndarray, xx: np.ndarray, interpolation: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """PIL's coefficients for the output samples `xx` (any order, repeats allowed) of axes resized from `in_size` to `out_size`
    samples -- three arrays of one length, one entry per output sample, so a whole batch is one call.
    -> lo [E], cnt [E], k [taps][E] int32: sample e is clip8((2^21 + sum_{i < cnt} k[i][e] * in[lo[e] + i]) >> 22); k is 0 past cnt.
    An axis PIL does not resample (in_size == out_size) is cnt = 1, k = 2^22: the byte itself."""
    support_of = FILTER_SUPPORT[interpolation]
    in_size, out_size, xx = (np.asarray(v, dtype=np.int64) for v in (in_size, out_size, xx))
    scale = in_size.astype(np.float64) / out_size
    fs = np.maximum(scale, 1.0)
    support = support_of * fs
    center = (xx + 0.5) * scale
    lo = np.maximum((center - support + 0.5).astype(np.int64), 0)          # (int) truncates towards zero, as astype does
    cnt = np.minimum((center + support + 0.5).astype(np.int64), in_size) - lo
    same = in_size == out_size
    lo, cnt = np.where(same, xx, lo), np.where(same, 1, cnt)
    taps = int(cnt.max())
    x = np.arange(taps, dtype=np.int64)[:, None]                           # taps lead: a tap's row is contiguous, as the kernel's table is
    t = x.astype(np.float64) + lo.astype(np.float64)                       # small integers: the float sum is the integer sum
    t -= center
    t += 0.5
    t *= 1.0 / fs
    w = _filter(t, interpolation)
    w *= x < cnt
    ww = np.zeros(w.shape[1], dtype=np.float64)
    for i in range(taps):                                                  # PIL sums in tap order; np.sum would pair the additions
        ww += w[i]
    w /= np.where(ww != 0.0, ww, 1.0)                                      # PIL divides only where the sum is not zero
    half = np.copysign(0.5, w)                                             # (int)(w * 2^22 + 0.5), or - 0.5 for w < 0 (a -0.0 rounds to 0 either way)
    w *= float(1 << PRECISION_BITS)
    w += half
    k = w.astype(np.int32)
    k[:, same] = 0
    k[0, same] = 1 << PRECISION_BITS
    return lo.astype(np.int32), cnt.astype(np.int32), k


def _reflect(p: np.ndarray, n: np.ndarray) -> np.ndarray:
    p = np.abs(p)
    return np.minimum(p, 2 * (n - 1) - p)    # p < n: 2 (n - 1) - p >= n - 1 >= p;  p >= n: the mirror image is the smaller one


def resize_tables(shapes: np.ndarray, draws: np.ndarray, size: int, interpolation: str) -> Tuple[np.ndarray, int]:
    """The kernel's tables for source images `shapes` [N][2] = (h, w) and `draws` [N][6] of draw_resized_crops.
    -> (int32 [N][2][2 + taps][size], taps): axis 0 the crop columns (horizontal pass, flip resolved), axis 1 the crop rows; the rows
    of an axis table are lo, cnt, k[0 .. taps).  Crop position j is sample reflect(origin + j) of the resized axis."""
    n = len(draws)
    shapes = np.asarray(shapes, dtype=np.int64).reshape(n, 2)
    d = np.asarray(draws, dtype=np.float64)
    rh, rw, sy0, sx0, flip = (d[:, c].astype(np.int64) for c in range(1, 6))
    j = np.arange(size, dtype=np.int64)[None, :]
    cols = _reflect(sx0[:, None] + np.where(flip[:, None] != 0, size - 1 - j, j), rw[:, None])
    rows = _reflect(sy0[:, None] + j, rh[:, None])
    in_size = np.repeat(np.stack([shapes[:, 1], shapes[:, 0]], axis=1).reshape(-1), size)      # [N][2][size] flattened
    out_size = np.repeat(np.stack([rw, rh], axis=1).reshape(-1), size)
    lo, cnt, k = axis_tables(in_size, out_size, np.stack([cols, rows], axis=1).reshape(-1), interpolation)
    taps = k.shape[0]
    tabs = np.empty((n, 2, 2 + taps, size), dtype=np.int32)
    tabs[:, :, 0] = lo.reshape(n, 2, size)
    tabs[:, :, 1] = cnt.reshape(n, 2, size)
    tabs[:, :, 2:] = k.reshape(taps, n, 2, size).transpose(1, 2, 0, 3)
    return tabs, taps


class DeviceImagePool:
    """Decoded uint8 RGB images, back to back in one device buffer."""

    def __init__(self, images: List[np.ndarray], device):
        assert len(images) > 0
        self.shapes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
        sizes = [h * w * 3 for h, w in self.shapes]
        self.offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        flat = np.concatenate([np.ascontiguousarray(im, dtype=np.uint8).reshape(-1) for im in images])
        self.pool = torch.from_numpy(flat).to(device)
        self.device = self.pool.device

    @classmethod
    def from_paths(cls, paths: Sequence[str], device) -> "DeviceImagePool":
        from PIL import Image
        return cls([np.asarray(Image.open(p).convert("RGB"), dtype=np.uint8) for p in paths], device)

    def __len__(self):
        return len(self.shapes)


class DeviceCropLoader:
    """Endless iterator of training batches cut on the device: {"real_images": [N, 3, size, size] (NHWC memory)}.

    Every rank of a data-parallel job passes its own `seed` (or the same one plus rank-strided `idx` draws via `rank` /
    `world_size`) so that ranks see different crops.

    `resize_range=(f_min, f_max)` puts the reference's PilRandomResize in front of the crop (`interpolation`: 'bicubic' or
    'bilinear', anything else is a KeyError as in the reference).  A range under which some pool image would need more than KMAX
    filter taps is refused here, not clamped.  With `resize_range=None` the loader draws and launches exactly what it did
    without the argument."""

    def __init__(self, pool: DeviceImagePool, batch_size: int, size: int = 256, seed: int = 0, rank: int = 0, world_size: int = 1,
                 resize_range: Optional[Sequence[float]] = None, interpolation: str = "bicubic"):
        self.pool, self.bs, self.size = pool, batch_size, size
        self.rng = np.random.default_rng([seed, rank])
        self.perm, self.cursor = None, 0
        self.items = torch.zeros((batch_size, 6), dtype=torch.int64, device=pool.device)
        self.interpolation = interpolation
        self.resize_range = None if resize_range is None else (float(resize_range[0]), float(resize_range[1]))
        self.tables = None     # the device buffer of cut()'s resize path: items + tables of one batch, made on first use
        if self.resize_range is not None:
            FILTER_SUPPORT[interpolation]   # an unknown name is a KeyError, as the reference's dict lookup (made only with a range)
            self._refuse_wide_filters()
        self._shapes = np.asarray(pool.shapes, dtype=np.int64)

    def _refuse_wide_filters(self):
        for h, w in self.pool.shapes:   # the lowest scale an image can draw is the widest filter it can need
            low, _ = scale_bounds(h, w, self.size, self.resize_range)
            taps = max(max_taps(h, int(h * low), self.interpolation), max_taps(w, int(w * low), self.interpolation))
            if taps > KMAX:
                raise ValueError(f"resize_range {self.resize_range} with f_min = {self.resize_range[0]} shrinks a {h} x {w} image by "
                                 f"{1.0 / low:.3g}, which needs {taps} {self.interpolation} taps; the device resampler takes {KMAX} "
                                 f"(a {KMAX // 4}x bicubic or {KMAX // 2}x bilinear down-scale)")

    def _next_indices(self) -> np.ndarray:
        out = []
        while len(out) < self.bs:  # shuffle=True, drop_last=True (base_trainer.py:74-80)
            if self.perm is None or self.cursor >= len(self.perm):
                self.perm, self.cursor = self.rng.permutation(len(self.pool)), 0
            out.append(int(self.perm[self.cursor]))
            self.cursor += 1
        return np.asarray(out)

    def draw(self, idx: np.ndarray) -> np.ndarray:
        """The random draws of one batch: draw_crops' [N][5] without a resize_range, draw_resized_crops' [N][6] with one."""
        if self.resize_range is None:
            return draw_crops(self.pool.shapes, idx, self.size, self.rng)
        return draw_resized_crops(self.pool.shapes, idx, self.size, self.rng, self.resize_range)

    def host_tables(self, idx: np.ndarray, draws: np.ndarray) -> Tuple[np.ndarray, int]:
        """-> (the int32 buffer of one resized batch as it is uploaded: [N][4] items, then the tables; taps)."""
        idx = np.asarray(idx)
        tabs, taps = resize_tables(self._shapes[idx], draws, self.size, self.interpolation)
        if taps > KMAX:
            raise ValueError(f"resize_range: a draw needs {taps} {self.interpolation} taps (images {self._shapes[idx].tolist()}, scales "
                             f"{np.asarray(draws)[:, 0].tolist()}); the device resampler takes {KMAX}")
        items = np.empty((len(idx), 2), dtype=np.int64)
        items[:, 0] = self.pool.offsets[idx]
        items[:, 1] = self._shapes[idx, 0] | (self._shapes[idx, 1] << 32)      # little-endian int32 pairs: (offset lo, hi), (H, W)
        return np.concatenate([items.view(np.int32).reshape(-1), tabs.reshape(-1)]), taps

    def cut(self, idx: np.ndarray, draws: np.ndarray, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One launch: images `idx` with draws [N][5] = (H, W, sy0, sx0, flip), or [N][6] = (scale, RH, RW, sy0, sx0, flip) for a
        crop of the image resized to RH x RW (the scale itself is not used: the sizes are) -> [N, 3, size, size]."""
        lib = L.load()
        n = len(idx)
        draws = np.asarray(draws)
        if out is None:
            out = ops.empty_nhwc(n, 3, self.size, self.size, self.pool.device)
        if draws.shape[1] == 6:
            host, taps = self.host_tables(idx, draws)
            if self.tables is None or self.tables.numel() < host.size:
                self.tables = torch.empty(max(host.size, self.bs * (4 + 2 * self.size * (2 + KMAX))), dtype=torch.int32, device=self.pool.device)
            dev = self.tables[:host.size]
            dev.copy_(torch.from_numpy(host))
            L.check(lib.crdr_resize_crop_flip_normalize(self.pool.pool.data_ptr(), dev.data_ptr(), dev.data_ptr() + 16 * n, n, taps, self.size,
                                                        self.size, out.data_ptr(), ops.ld_for(3), ops._stream()), "resize_crop_flip_normalize")
            return out
        table = np.concatenate([self.pool.offsets[idx][:, None], draws], axis=1).astype(np.int64)
        items = self.items[:n]
        items.copy_(torch.from_numpy(table))
        L.check(lib.crdr_crop_flip_normalize(self.pool.pool.data_ptr(), items.data_ptr(), n, self.size, self.size, out.data_ptr(),
                                             ops.ld_for(3), ops._stream()), "crop_flip_normalize")
        return out

    def __iter__(self):
        return self

    def __next__(self) -> Dict[str, torch.Tensor]:
        idx = self._next_indices()
        return {"real_images": self.cut(idx, self.draw(idx))}

    def __len__(self):
        return 1 << 30
