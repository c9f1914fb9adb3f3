"""Numpy restatement of PIL's 8-bit resize (Pillow, src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc,
ImagingResampleHorizontal_8bpc, ImagingResampleVertical_8bpc) and of the reference's training transform built on it
(data_transform.py:19-73), written one output sample at a time -- the slow, literal form the product's batched table
builder (crdr_amd/dataset/device_pipeline.py) and its kernel are checked against.  test_random_resize_host.py pins this
file to `Image.resize` itself, byte for byte."""
import numpy as np

PRECISION_BITS = 22
SUPPORT = {"bicubic": 2.0, "bilinear": 1.0}


def bicubic_filter(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def bilinear_filter(x: float) -> float:
    if x < 0.0:
        x = -x
    if x < 1.0:
        return 1.0 - x
    return 0.0


FILTERS = {"bicubic": bicubic_filter, "bilinear": bilinear_filter}


def coeffs(in_size: int, out_size: int, interpolation: str):
    """-> per output sample (xmin, [int coefficient of in[xmin + x] for x < xmax])"""
    filt, scale = FILTERS[interpolation], float(in_size) / out_size
    fs = max(scale, 1.0)
    support = SUPPORT[interpolation] * fs
    ss = 1.0 / fs
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [filt((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        out.append((xmin, [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]))
    return out


def clip8(acc: np.ndarray) -> np.ndarray:
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)   # >> on a signed array is arithmetic


def resample_axis0(img: np.ndarray, out_size: int, interpolation: str) -> np.ndarray:
    """one pass along axis 0 of a uint8 array; a pass whose output length equals its input length is skipped, as PIL does"""
    if out_size == img.shape[0]:
        return img
    out = np.empty((out_size,) + img.shape[1:], dtype=np.uint8)
    for xx, (xmin, k) in enumerate(coeffs(img.shape[0], out_size, interpolation)):
        acc = np.full(img.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for x, kv in enumerate(k):
            acc += kv * img[xmin + x].astype(np.int64)
        assert np.abs(acc).max() < 2 ** 31, "PIL's accumulator is 32 bits wide"
        out[xx] = clip8(acc)
    return out


def pil_resize(img: np.ndarray, rh: int, rw: int, interpolation: str) -> np.ndarray:
    """img [h][w][3] uint8 -> [rh][rw][3]: the horizontal pass, uint8 in between, then the vertical pass"""
    mid = resample_axis0(img.transpose(1, 0, 2), rw, interpolation).transpose(1, 0, 2)
    return resample_axis0(mid, rh, interpolation)


def reflect_crop_flip(img: np.ndarray, size: int, sy0: int, sx0: int, flip: int) -> np.ndarray:
    """RandomCrop(size, pad_if_needed, reflect) at origin (sy0, sx0) of the UNPADDED image, then the flip -> uint8 [size][size][3]"""
    h, w, _ = img.shape
    ph, pw = max(0, size - h), max(0, size - w)
    pad = np.pad(img, ((ph, ph), (pw, pw), (0, 0)), mode="reflect")
    c = pad[sy0 + ph:sy0 + ph + size, sx0 + pw:sx0 + pw + size]
    return c[:, ::-1] if flip else c


def apply_tables(img: np.ndarray, tabs: np.ndarray) -> np.ndarray:
    """The kernel's arithmetic on one sample: tabs int32 [2][2 + taps][size] (columns, rows; rows of a table: lo, cnt, k...)
    -> uint8 [size][size][3], computing nothing but the crop window."""
    (xlo, xcnt, kh), (ylo, ycnt, kv) = ((t[0], t[1], t[2:]) for t in tabs.astype(np.int64))
    size = tabs.shape[2]
    out = np.empty((size, size, 3), dtype=np.uint8)
    src = img.astype(np.int64)
    for r in range(size):
        rows = src[ylo[r]:ylo[r] + ycnt[r]]
        assert len(rows) == ycnt[r]
        for c in range(size):
            win = rows[:, xlo[c]:xlo[c] + xcnt[c]]
            assert win.shape[1] == xcnt[c]
            mid = clip8((1 << (PRECISION_BITS - 1)) + np.einsum("i,jic->jc", kh[:xcnt[c], c], win)).astype(np.int64)
            out[r, c] = clip8((1 << (PRECISION_BITS - 1)) + np.einsum("j,jc->c", kv[:ycnt[r], r], mid))
    return out


def normalise(crop_u8: np.ndarray) -> np.ndarray:
    """ToTensor + Normalize(0.5, 0.5): uint8 [S][S][3] -> float32 [3][S][S]"""
    t = crop_u8.astype(np.float32) / np.float32(255.0)
    return ((t - np.float32(0.5)) / np.float32(0.5)).transpose(2, 0, 1)


def checkerboard(h: int, w: int, cell: int = 1) -> np.ndarray:
    """0 / 255 squares, the three channels out of phase: where the intermediate clip8 and the negative lobes matter"""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(((y // cell + x // cell + p) % 2) * 255).astype(np.uint8) for p in (0, 1, 0)], axis=2)
