"""resize_range on the host (no GPU): the numpy restatement of PIL's 8-bit resampler equals Image.resize byte for byte; the
product's coefficient tables, applied to the crop window alone, equal "PIL resizes the whole image, reflect-pad, crop,
flip"; the draw rules of PilRandomResize (data_transform.py:54-73); the folder dataset's PIL path; the refusals."""
import numpy as np
import pytest
from PIL import Image

from tests import pil_resize_ref as R

PIL_FILTER = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}


def _pil(img, rh, rw, interpolation):
    return np.asarray(Image.fromarray(img).resize((rw, rh), PIL_FILTER[interpolation]), dtype=np.uint8)


def _cases():
    rng = np.random.default_rng(2024)
    out = []
    for k in range(40):
        h, w = (int(v) for v in rng.integers(20, 91, size=2))
        s = float(rng.uniform(0.25, 2.2))
        rh, rw = max(1, int(h * s)), max(1, int(w * s))
        if k % 5 == 4:
            rh = h                      # one pass skipped
        kind = ("random", "checker1", "checker3", "saturated")[k % 4]
        out.append((h, w, rh, rw, ("bicubic", "bilinear")[(k // 4) % 2], kind, k))
    return out


def _image(h, w, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    if kind == "saturated":
        return (rng.integers(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)
    return R.checkerboard(h, w, 1 if kind == "checker1" else 3)


@pytest.mark.parametrize("h,w,rh,rw,interpolation,kind,seed", _cases())
def test_restatement_equals_pil_resize(h, w, rh, rw, interpolation, kind, seed):
    img = _image(h, w, kind, seed)
    assert np.array_equal(R.pil_resize(img, rh, rw, interpolation), _pil(img, rh, rw, interpolation))


def test_restatement_equals_pil_at_the_scale_bounds():
    """0.25 and 2.2 themselves, both filters, on the 1-pixel checkerboard"""
    for interpolation in ("bicubic", "bilinear"):
        for s in (0.25, 2.2):
            img = R.checkerboard(88, 61)
            rh, rw = int(88 * s), int(61 * s)
            assert np.array_equal(R.pil_resize(img, rh, rw, interpolation), _pil(img, rh, rw, interpolation))


# (h, w, size, scale or None = the minimum scale size / min(h, w), sy0, sx0) -- origins in un-padded coordinates of the resized image
WINDOWS = [
    (70, 90, 32, 1.7, 40, 100), (70, 90, 32, 0.4, -2, 1), (49, 60, 32, None, -1, 3), (60, 49, 32, None, 5, 0), (40, 50, 32, 0.5, -10, -5),
    (64, 64, 32, 1.0, 17, 30), (40, 300, 32, 1.004, 8, 269), (90, 90, 32, 32 / 90, 0, 0), (90, 77, 80, 1.3, 30, 20),
]


@pytest.mark.parametrize("interpolation", ["bicubic", "bilinear"])
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("h,w,size,scale,sy0,sx0", WINDOWS)
def test_host_tables_on_the_crop_window_equal_pil_on_the_whole_image(h, w, size, scale, sy0, sx0, flip, interpolation):
    from crdr_amd.dataset.device_pipeline import KMAX, resize_tables
    scale = float(size) / min(h, w) if scale is None else scale
    rh, rw = int(h * scale), int(w * scale)
    if (h, w) == (49, 60):
        assert rh == 31, "the float truncation of the reference: one below the crop size"
    img = _image(h, w, "checker1" if (h + sy0) % 2 else "random", h * w)
    tabs, taps = resize_tables([(h, w)], np.asarray([[scale, rh, rw, sy0, sx0, flip]]), size, interpolation)
    assert tabs.shape == (1, 2, 2 + taps, size) and tabs.dtype == np.int32 and 1 <= taps <= KMAX
    assert int(tabs[0, :, 1].max()) == taps
    ref = R.reflect_crop_flip(_pil(img, rh, rw, interpolation), size, sy0, sx0, flip)
    assert np.array_equal(R.apply_tables(img, tabs[0]), ref)
    if rh == h and rw == w:
        assert taps == 1 and (tabs[0, :, 2] == 1 << 22).all()


def test_batched_tables_equal_the_restatements_coefficients():
    """a mixed batch in one call: every entry is the restatement's (xmin, coefficients) of its own axis"""
    from crdr_amd.dataset.device_pipeline import resize_tables
    shapes = [(70, 90), (49, 60), (64, 64), (90, 40)]
    draws = np.asarray([[1.7, 119, 153, 3, 5, 0], [32 / 49, 31, 39, -1, 2, 1], [1.0, 64, 64, 9, 9, 1], [0.3, 27, 12, -5, -20, 0]])
    for interpolation in ("bicubic", "bilinear"):
        tabs, taps = resize_tables(shapes, draws, 32, interpolation)
        for n, ((h, w), d) in enumerate(zip(shapes, draws)):
            rh, rw, sy0, sx0, flip = (int(v) for v in d[1:])
            for axis, (src, dst, origin) in enumerate(((w, rw, sx0), (h, rh, sy0))):
                co = R.coeffs(src, dst, interpolation) if src != dst else [(x, [1 << 22]) for x in range(src)]
                for j in range(32):
                    p = origin + (31 - j if (flip and axis == 0) else j)
                    p = -p if p < 0 else p
                    p = 2 * (dst - 1) - p if p >= dst else p
                    lo, k = co[p]
                    t = tabs[n, axis, :, j]
                    assert t[0] == lo and t[1] == len(k) and list(t[2:2 + len(k)]) == k and not t[2 + len(k):].any()


def test_draw_rules():
    from crdr_amd.dataset.device_pipeline import draw_resized_crops, scale_bounds
    size = 32
    shapes = [(49, 60), (40, 300), (90, 90), (33, 200), (500, 70)]
    low, high = scale_bounds(40, 300, size, (0.25, 0.5))
    assert low == high == 32.0 / 40.0, "size / min(h, w) > f_max: low = high"
    assert scale_bounds(90, 90, size, (0.5, 1.0)) == (0.5, 1.0)
    assert scale_bounds(90, 90, size, (0.1, 1.0)) == (32.0 / 90.0, 1.0)
    idx = np.arange(2000) % len(shapes)
    for rr in ((0.25, 0.5), (0.5, 1.0), (1.5, 1.5)):
        d = draw_resized_crops(shapes, idx, size, np.random.default_rng(5), rr)
        assert d.shape == (2000, 6) and d.dtype == np.float64
        for (scale, rh, rw, sy0, sx0, flip), i in zip(d, idx):
            h, w = shapes[i]
            lo, hi = scale_bounds(h, w, size, rr)
            assert lo <= scale <= hi
            assert (rh, rw) == (int(h * scale), int(w * scale))
            ph, pw = max(0, size - int(rh)), max(0, size - int(rw))
            assert -ph <= sy0 <= rh + ph - size and -pw <= sx0 <= rw + pw - size and flip in (0.0, 1.0)
        assert 0.4 < d[:, 5].mean() < 0.6
    d = draw_resized_crops([(49, 60)], np.zeros(50, dtype=np.int64), size, np.random.default_rng(1), (0.1, 0.1))
    assert (d[:, 1] == 31).all() and set(d[:, 3]) == {-1.0, 0.0}, "31 rows padded by one on both sides are 33: two origins"


class _CountingRng:
    def __init__(self, seed):
        self.rng, self.calls = np.random.default_rng(seed), []

    def __getattr__(self, name):
        fn = getattr(self.rng, name)

        def call(*a, **k):
            self.calls.append(name)
            return fn(*a, **k)
        return call


class _HostPool:
    """DeviceImagePool's host-side fields"""

    def __init__(self, shapes):
        import torch
        self.shapes = list(shapes)
        self.offsets = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in shapes])[:-1]]).astype(np.int64)
        self.device = torch.device("cpu")

    def __len__(self):
        return len(self.shapes)


def test_no_resize_range_draws_exactly_what_draw_crops_draws():
    from crdr_amd.dataset.device_pipeline import DeviceCropLoader, draw_crops
    pool = _HostPool([(300, 400), (256, 256), (200, 310), (257, 180)])
    loader = DeviceCropLoader(pool, batch_size=3, size=256, seed=9)
    assert loader.resize_range is None
    loader.rng = _CountingRng([9, 0])      # the loader's own seeding rule, with every call on it recorded
    mirror = np.random.default_rng([9, 0])
    perm, cursor = None, 0
    for _ in range(3):                     # crosses a reshuffle of the 4-image pool
        want = []                          # the parent's __next__ by hand: permutations as needed, then draw_crops, nothing else
        while len(want) < 3:
            if perm is None or cursor >= len(perm):
                perm, cursor = mirror.permutation(4), 0
            want.append(int(perm[cursor]))
            cursor += 1
        idx = loader._next_indices()
        assert list(idx) == want
        assert np.array_equal(loader.draw(idx), draw_crops(pool.shapes, np.asarray(want), 256, mirror))
    calls = loader.rng.calls
    assert calls.count("permutation") == 3 and calls.count("integers") == 18 and calls.count("random") == 9 and len(calls) == 30


def test_folder_dataset_resizes_with_pil_before_the_crop(tmp_path):
    """resize_range (2, 2) on a 40 x 40 PNG: the crop comes out of PIL's 80 x 80 bicubic up-scale, not out of the original"""
    from crdr_amd.dataset import build_dataset
    img = np.random.default_rng(0).integers(0, 256, size=(40, 40, 3), dtype=np.uint8)
    Image.fromarray(img).save(tmp_path / "a.png")
    opt = dict(name="openimage", type="ImageDataset", root_dir=str(tmp_path), image_size=32, resize_range=[2.0, 2.0], interpolation="bicubic")
    ds = build_dataset(opt, True)
    np.random.seed(123)
    got = ds[0]["real_images"].numpy()
    np.random.seed(123)
    assert np.random.uniform(2.0, 2.0) == 2.0
    big = _pil(img, 80, 80, "bicubic")
    y0, x0 = np.random.randint(0, 80 - 32 + 1), np.random.randint(0, 80 - 32 + 1)
    crop = big[y0:y0 + 32, x0:x0 + 32]
    if np.random.rand() < 0.5:
        crop = crop[:, ::-1]
    assert got.shape == (3, 32, 32) and np.array_equal(got, R.normalise(crop))
    # evaluation ignores both keys, as PilEvalTransform does
    ev = build_dataset(dict(opt, interpolation="no such filter"), False)
    assert ev[0]["real_images"].shape == (3, 40, 40)
    with pytest.raises(KeyError):
        build_dataset(dict(opt, interpolation="lanczos"), True)


def test_refusals():
    from crdr_amd.dataset.device_pipeline import KMAX, DeviceCropLoader, max_taps
    assert KMAX >= 17 and max_taps(400, 100, "bicubic") == 17 and max_taps(400, 50, "bilinear") == 17 and max_taps(64, 64, "bicubic") == 1
    pool = _HostPool([(300, 400), (3000, 2000)])
    DeviceCropLoader(pool, 2, size=256, resize_range=(0.25, 1.0), interpolation="bicubic")       # 4x: 17 taps, admitted
    DeviceCropLoader(pool, 2, size=256, resize_range=(0.125, 1.0), interpolation="bilinear")     # 2000 / 256 = 7.8x bilinear: 16 taps
    with pytest.raises(ValueError, match=r"resize_range.*3000 x 2000"):
        DeviceCropLoader(pool, 2, size=256, resize_range=(0.2, 1.0), interpolation="bicubic")    # 5x bicubic: 21 taps
    DeviceCropLoader(_HostPool([(300, 400)]), 2, size=256, resize_range=(0.2, 1.0))              # 300 / 256: the crop size bounds the shrink
    with pytest.raises(KeyError):
        DeviceCropLoader(pool, 2, size=256, resize_range=(0.5, 1.0), interpolation="lanczos")
    # explicit draws that need more than KMAX taps are refused when the tables are built, not clamped
    loader = DeviceCropLoader(_HostPool([(400, 400)]), 1, size=32, resize_range=(0.25, 1.0))
    with pytest.raises(ValueError, match="resize_range"):
        loader.host_tables(np.asarray([0]), np.asarray([[0.1, 40, 40, 0, 0, 0]]))
