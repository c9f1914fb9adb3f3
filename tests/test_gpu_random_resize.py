"""resize_range on the device: crdr_resize_crop_flip_normalize (csrc/resize_crop.hip) through DeviceCropLoader.cut() against PIL itself --
Image.resize of the WHOLE image, then the oracle's RandomCrop(pad_if_needed, reflect) -> HFlip -> ToTensor -> Normalize.  Every comparison is
torch.equal: the kernel's arithmetic is PIL's integer arithmetic, so there is no tolerance to state.

Sizes: crops of 32 (one tile of the kernel) and, in one case, 80 (3 x 3 tiles, ragged in both directions); images of at most 90 pixels
a side, except where the case itself needs a longer axis: 40 x 300 (the one-axis case), and 136 x 40 / 272 x 40 for the strongest
down-scales KMAX = 17 taps admit.  A resized side must stay above the reflect padding (pad < side, so >= 17 of 32), and an exact 4x
ratio meets only 16 taps (88 x 88 -> 22 x 22, both axes reflected, is kept for the reflection), so the 17-tap entries come from
136 -> 33 rows (4.12x bicubic) and 272 -> 33 rows (8.24x bilinear); the latter's 32 crop rows need 268 source rows at once, the longest
LDS span these tests meet (the kernel's array holds 288).  Those same 272 -> 33 rows would be 33 bicubic taps: the refusal case."""
import functools

import numpy as np
import pytest
import torch
from PIL import Image

from tests import pil_resize_ref as R
from tests.test_gpu_model import dev

pytestmark = pytest.mark.gpu

PIL_FILTER = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}
FILTERS = ("bicubic", "bilinear")
SHAPES = [(70, 90), (90, 90), (88, 88), (64, 64), (40, 300), (49, 60), (40, 50), (136, 40), (272, 40), (90, 77)]
CHECKER = 3   # index of the 64 x 64 image: a 0 / 255 checkerboard of 1-pixel cells


@functools.lru_cache(maxsize=None)
def _images():
    rng = np.random.default_rng(77)
    imgs = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in SHAPES]
    imgs[CHECKER] = R.checkerboard(64, 64)
    return imgs


@functools.lru_cache(maxsize=None)
def _pool():
    from crdr_amd.dataset.device_pipeline import DeviceImagePool
    return DeviceImagePool(_images(), dev())


@functools.lru_cache(maxsize=None)
def _loader(size, interpolation):
    from crdr_amd.dataset.device_pipeline import DeviceCropLoader
    return DeviceCropLoader(_pool(), batch_size=16, size=size, seed=1, resize_range=(0.25, 2.0), interpolation=interpolation)


@functools.lru_cache(maxsize=None)
def _resized(image, rh, rw, interpolation):
    return np.asarray(Image.fromarray(_images()[image]).resize((rw, rh), PIL_FILTER[interpolation]), dtype=np.uint8)


def _reference(image, draw, size, interpolation):
    from oracle.crdr_oracle import train_transform_sample
    _, rh, rw, sy0, sx0, flip = (int(v) for v in draw)
    return torch.from_numpy(np.ascontiguousarray(train_transform_sample(_resized(image, rh, rw, interpolation), size, sy0, sx0, flip)))


# name -> (image, RH, RW, sy0, sx0): origins in the un-padded coordinates of the resized image, as DeviceCropLoader.cut() takes them
CASES = {
    "up 1.7": (0, 119, 153, 60, 121),
    "down 0.4": (1, 36, 36, 3, 4),
    "4x, both axes reflected": (2, 22, 22, -7, -3),
    "4.12x rows, 17 bicubic taps": (7, 33, 40, 1, 5),
    "8.24x rows, 17 bilinear taps": (8, 33, 40, 0, 8),
    "scale 1.0": (3, 64, 64, 31, 17),
    "one axis": (4, 40, 301, 8, 269),
    "49 x 60 at the minimum scale": (5, 31, 39, -1, 6),
    "smaller than the crop": (6, 20, 25, -9, -2),
    "checkerboard down": (3, 41, 47, 5, 11),
    "checkerboard up": (3, 100, 83, 60, 40),
}


def _admitted(name, interpolation):
    """the 8.24x case is 33 bicubic taps: there the loader's refusal is the expected outcome (test_wide_draws_are_refused)"""
    return not (name.startswith("8.24x") and interpolation == "bicubic")


def _draw(name, flip):
    image, rh, rw, sy0, sx0 = CASES[name]
    return image, [rh / SHAPES[image][0], rh, rw, sy0, sx0, flip]


@pytest.mark.parametrize("name,flip,interpolation", [(n, f, i) for i in FILTERS for f in (0, 1) for n in CASES if _admitted(n, i)])
def test_crop_of_the_resized_image_equals_pil(name, flip, interpolation):
    image, draw = _draw(name, flip)
    out = _loader(32, interpolation).cut(np.asarray([image]), np.asarray([draw]))
    assert out.shape == (1, 3, 32, 32)
    assert torch.equal(out[0].cpu(), _reference(image, draw, 32, interpolation))


def test_49_by_60_at_the_minimum_scale_is_31_rows():
    assert int(49 * (32.0 / 49)) == 31 and CASES["49 x 60 at the minimum scale"][1:3] == (31, int(60 * (32.0 / 49)))


@pytest.mark.parametrize("interpolation", FILTERS)
@pytest.mark.parametrize("flip", [0, 1])
def test_ragged_tiles(flip, interpolation):
    """a crop of 80: 3 x 3 tiles of the kernel, the last ones 16 wide / high; 90 x 77 at 1.3 and, reflected on one axis, at 0.95"""
    idx = np.asarray([9, 9])
    draws = np.asarray([[1.3, 117, 100, 30, 19, flip], [0.95, 85, 73, 2, -5, flip]])
    out = _loader(80, interpolation).cut(idx, draws)
    for k in range(2):
        assert torch.equal(out[k].cpu(), _reference(9, draws[k], 80, interpolation)), k


@pytest.mark.parametrize("interpolation", FILTERS)
def test_mixed_batch_sentinel_fourth_lane_and_determinism(interpolation):
    """every case in ONE launch, flips alternating; written into the middle of a sentinel-filled buffer"""
    names = [n for n in CASES if _admitted(n, interpolation)]
    picks = [_draw(n, k % 2) for k, n in enumerate(names)] + [_draw(n, (k + 1) % 2) for k, n in enumerate(names[:16 - len(names)])]
    idx, draws = np.asarray([p[0] for p in picks]), np.asarray([p[1] for p in picks])
    n, s, guard, sentinel = len(idx), 32, 4096, -77.0
    assert n > len(CASES) - 2
    buf = torch.full((guard + n * s * s * 4 + guard,), sentinel, dtype=torch.float32, device=dev())
    nhwc = buf[guard:guard + n * s * s * 4].view(n, s, s, 4)
    out = _loader(s, interpolation).cut(idx, draws, out=nhwc.permute(0, 3, 1, 2)[:, :3])
    assert out.data_ptr() == nhwc.data_ptr()
    for k in range(n):
        assert torch.equal(out[k].cpu(), _reference(int(idx[k]), draws[k], s, interpolation)), (k, picks[k])
    assert bool((nhwc[..., 3] == 0).all()), "the fourth lane is written as zero"
    assert bool((buf[:guard] == sentinel).all()) and bool((buf[-guard:] == sentinel).all()), "a write outside [N, S, S, ldo]"
    again = _loader(s, interpolation).cut(idx, draws)
    assert torch.equal(again, out), "two launches differ"
    # fewer samples than the buffer holds: the rest keeps the sentinel
    buf.fill_(sentinel)
    _loader(s, interpolation).cut(idx[:3], draws[:3], out=nhwc[:3].permute(0, 3, 1, 2)[:, :3])
    assert torch.equal(nhwc[:3, ..., :3].cpu(), out[:3].permute(0, 2, 3, 1).cpu()) and bool((nhwc[3:] == sentinel).all())


def test_wide_draws_are_refused():
    image, draw = _draw("8.24x rows, 17 bilinear taps", 0)
    with pytest.raises(ValueError, match="resize_range"):
        _loader(32, "bicubic").cut(np.asarray([image]), np.asarray([draw]))


def test_without_a_range_the_loader_is_the_plain_cut():
    from crdr_amd.dataset.device_pipeline import DeviceCropLoader, draw_crops
    from crdr_amd.hip import lib as L
    from crdr_amd.hip import ops
    pool = _pool()
    a = DeviceCropLoader(pool, batch_size=8, size=32, seed=5, resize_range=None)
    b = DeviceCropLoader(pool, batch_size=8, size=32, seed=5)
    batch = next(a)["real_images"]
    idx = b._next_indices()
    draws = draw_crops(pool.shapes, idx, 32, b.rng)
    items = torch.from_numpy(np.concatenate([pool.offsets[idx][:, None], draws], axis=1).astype(np.int64)).to(dev())
    out = ops.empty_nhwc(8, 3, 32, 32, dev())
    L.check(L.load().crdr_crop_flip_normalize(pool.pool.data_ptr(), items.data_ptr(), 8, 32, 32, out.data_ptr(), 4, ops._stream()), "plain cut")
    assert torch.equal(batch, out)
    assert a.tables is None, "no table buffer without a range"
    # and at scale 1.0 the new kernel computes what the plain one does
    six = np.concatenate([np.ones((8, 1)), draws], axis=1).astype(np.float64)
    assert torch.equal(_loader(32, "bicubic").cut(idx, six), out)


def test_build_loaders_with_a_range(tmp_path):
    """a training config with device_pool and resize_range: [N, 3, S, S] in [-1, 1], equal to cut() of the draws it made and to PIL"""
    from crdr_amd.dataset import build_loaders
    from crdr_amd.dataset.device_pipeline import DeviceCropLoader
    from oracle.crdr_oracle import train_transform_sample
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, size=hw + (3,), dtype=np.uint8) for hw in ((60, 81), (75, 49), (90, 90))]
    for k, im in enumerate(imgs):
        Image.fromarray(im).save(tmp_path / f"{k}.png")
    tr = dict(name="openimage", type="ImageDataset", root_dir=str(tmp_path), image_size=32, device_pool=True, resize_range=[0.5, 1.0],
              interpolation="bilinear")
    train, _ = build_loaders({"dataset": {"batch_size": 5, "train_dataset": tr}, "data_seed": 4}, dev())
    assert isinstance(train, DeviceCropLoader) and train.resize_range == (0.5, 1.0) and train.interpolation == "bilinear"
    twin = DeviceCropLoader(train.pool, 5, 32, seed=4, resize_range=(0.5, 1.0), interpolation="bilinear")
    for _ in range(2):
        batch = next(train)["real_images"]
        assert batch.shape == (5, 3, 32, 32) and float(batch.min()) >= -1.0 and float(batch.max()) <= 1.0
        idx = twin._next_indices()
        draws = twin.draw(idx)
        assert draws.shape == (5, 6) and (draws[:, 0] >= 0.5).all() and (draws[:, 0] <= 1.0).all()
        assert torch.equal(batch, twin.cut(idx, draws))
        for k, i in enumerate(idx):
            _, rh, rw, sy0, sx0, flip = (int(v) for v in draws[k])
            big = np.asarray(Image.fromarray(imgs[i]).resize((rw, rh), Image.BILINEAR), dtype=np.uint8)
            assert np.array_equal(batch[k].cpu().numpy(), train_transform_sample(big, 32, sy0, sx0, flip)), (k, i, draws[k])


def test_cabi_refusals():
    from crdr_amd.dataset.device_pipeline import KMAX
    from crdr_amd.hip import lib as L
    from crdr_amd.hip import ops
    lib = L.load()
    pool = _pool().pool
    tabs = torch.zeros(4 + 2 * 3 * 32, dtype=torch.int32, device=dev())
    out = torch.zeros(32 * 32 * 8 + 4, dtype=torch.float32, device=dev())
    p, t, o = pool.data_ptr(), tabs.data_ptr(), out.data_ptr()

    def call(pool=p, items=t, tab=t + 16, n=1, ktaps=1, out=o, ldo=4):
        return L.check(lib.crdr_resize_crop_flip_normalize(pool, items, tab, n, ktaps, 32, 32, out, ldo, ops._stream()), "resize_crop")
    for bad in (dict(pool=None), dict(items=None), dict(tab=None), dict(out=None)):
        with pytest.raises(L.CrdrHipError, match="null pointer"):
            call(**bad)
    with pytest.raises(L.CrdrHipError, match="16-byte aligned"):
        call(out=o + 4)
    for ldo in (6, 2, 0):
        with pytest.raises(L.CrdrHipError, match="16-byte aligned"):
            call(ldo=ldo)
    for ktaps in (KMAX + 1, 0, -1):
        with pytest.raises(L.CrdrHipError, match="KMAX"):
            call(ktaps=ktaps)
    assert call(n=0) == 0
    assert call(ldo=8) == 0   # all-zero tables (cnt = 0) are a valid call: every byte is clip8(2^21 >> 22) = 0, i.e. -1.0
    torch.cuda.synchronize()
    assert bool((out[:32 * 32 * 8].view(32, 32, 8)[..., :3] == -1.0).all()) and float(out[-4:].abs().max()) == 0.0
