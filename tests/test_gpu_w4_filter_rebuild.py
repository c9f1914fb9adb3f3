"""The F(4x4, 3x3) filter transform (csrc/wino4.hip: wino4_filter_block behind crdr_w4_filters_batched and behind a conv launch whose cache
is not valid) against U = G g G^T evaluated in numpy float64 from the pack contents, in the documented block layout
[N tile of 64][variant][chunk of 4 channels][position 36][channel 4][oh 2][tx 16][ob 2], output channel = 64 tile + 32 oh + 16 ob + tx.

Cases: every form the kernel takes (3x3 stride 1 and its transposed twin, 5x5 stride-2 conv, 5x5 stride-2 transposed, 5x5 stride 1), Cout
below / above / not a multiple of 64, Cin not a multiple of 32 (a last run shorter than eight chunks), exactly five runs (Cin = 160), a
group of two, batch 2.  The transformed filters do not depend on the image size; the images are the smallest the F(4x4) kernel accepts
for each form (9 x 9 for the stride-1 forms, 24 output-phase columns for the stride-2 ones): crdr_conv2d_filter_item refuses anything
smaller, so there is no cache to test below that.

Tolerance: the kernel's double arithmetic may contract to FMA and sums in another order than numpy, so a double can fall on the other side of
a float32 rounding tie: every element within 1 float32 ulp, at most 1e-5 of the elements unequal at all, padding entries exactly 0.0.

The weights (_weights): 24-bit mantissas that are multiples of neither 3 nor 5, random sign, times 2^k with k uniform in -16 .. 16.  A mismatch
needs the exact U within ~1e-16 relative of a tie, ~1e-8 per element for a generic real number -- but U is a short rational.  The rows of G
are (256/225, 0, 0), (16, +-12, 9) / 18, (16, +-20, 25) / 50 and (0, 0, 1): wherever the numerator of a sum is divisible by what is left of
9, 25, 81, 225, 625 the exact value is dyadic, and with float32 weights of ONE magnitude it has only ~7 bits below the float32 result, so it
sits EXACTLY on a tie with probability ~2^-7.  Two correct float64 evaluations (sequential sums with and without FMA, against einsum) then
disagree on 1e-4 of normal-deviate weights, ten times the cap, whatever the kernel does.  Modulo 3 and modulo 5 every numerator reduces to
ONE weight times a unit, except where one factor is a +-a row and the other a +-b row: with every weight coprime to 15 an exact tie is impossible
at 28 of the 36 positions and needs divisibility by 225 at the other 8, and the spread of magnitudes puts ~20 more bits below the result
there.  The same numpy experiment with these weights: 3e-8 per element (2e6 samples of 36), the generic figure.  """
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 1024   # NaN floats on either side of every cache

# name, Cin, Cout, H = W, k, stride, transposed, G
CASES = [
    ("c3_36_100", 36, 100, 9, 3, 1, 0, 1),
    ("t3_36_100", 36, 100, 9, 3, 1, 1, 1),
    ("c3_160_64", 160, 64, 9, 3, 1, 0, 1),
    ("t3_160_64", 160, 64, 9, 3, 1, 1, 1),
    ("c5s2_36_100", 36, 100, 48, 5, 2, 0, 1),
    ("t5s2_100_36", 100, 36, 24, 5, 2, 1, 1),
    ("c5_12_72", 12, 72, 9, 5, 1, 0, 1),
    ("c5_100_36", 100, 36, 9, 5, 1, 0, 1),
    ("c3_36_100_g2", 36, 100, 9, 3, 1, 0, 2),
]
IDS = [c[0] for c in CASES]
SMALLEST = "c3_36_100"


def _w4_id(lib):
    return lib.crdr_conv2d_num_configs() + lib.crdr_conv2d_num_stream_configs() + 3


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _desc(lib, case):
    from crdr_amd.hip import lib as L
    _, ci, co, hw, k, s, tr, _ = case
    out = hw if s == 1 else (2 * hw if tr else hw // 2)
    return L.ConvDesc(N=2, H=hw, W=hw, C=ci, OH=out, OW=out, OC=co, kh=k, kw=k, stride=s, pad=k // 2, transposed=tr, ldx=ci, ldy=co,
                      wrows=(co + 31) // 32 * 32, wcols=(ci + 31) // 32 * 32, flags=0, reserved=_w4_id(lib))


def _item(lib, d, G, packs_, u):
    from crdr_amd.hip import lib as L
    it = L.W4FilterItem()
    L.check(lib.crdr_conv2d_filter_item(C.byref(d), G, C.byref(it)), "conv2d_filter_item")
    for g in range(G):
        it.w[g] = packs_[g].data_ptr()
    it.u = u.data_ptr()
    return it


def _guarded(nfloats, dev):
    """-> (whole NaN tensor, the cache inside it)"""
    whole = torch.full((nfloats + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
    return whole, whole[GUARD:GUARD + nfloats]


def _rebuild(lib, items, dev):
    from crdr_amd.hip import lib as L
    from crdr_amd.hip.batched import JobTable
    table = JobTable(dev, L.W4FilterItem, 16, name="test").upload(items, lambda it: int(it.units))
    L.check(lib.crdr_w4_filters_batched(*table.operands, _stream()), "w4_filters_batched")
    torch.cuda.synchronize()
    return table


def _expected(pack, widx, nvar, Cin, Cout):
    """U = G g G^T in float64 from the pack [T][rows][cols], rounded to float32, in the cache's layout; and the mask of its padding entries."""
    a, b = 0.75, 1.25
    Na, Nb, N0 = 2.0 * a * a * (a * a - b * b), 2.0 * b * b * (b * b - a * a), a * a * b * b
    Gm = np.array([[1.0 / N0, 0.0, 0.0], [1.0 / Na, a / Na, a * a / Na], [1.0 / Na, -a / Na, a * a / Na],
                   [1.0 / Nb, b / Nb, b * b / Nb], [1.0 / Nb, -b / Nb, b * b / Nb], [0.0, 0.0, 1.0]], dtype=np.float64)
    ntile, kch = (Cout + 63) // 64, (Cin + 3) // 4
    out = np.zeros((ntile, nvar, kch, 36, 4, 2, 16, 2), dtype=np.float32)
    live = np.zeros(out.shape, dtype=bool)
    p64 = pack.double().cpu().numpy()
    for v in range(nvar):
        g = np.zeros((3, 3, ntile * 64, kch * 4), dtype=np.float64)
        for t in range(9):
            if widx[v][t] >= 0:
                g[t // 3, t % 3, :Cout, :Cin] = p64[widx[v][t], :Cout, :Cin]
        u = np.einsum("ia,aboc,jb->ijoc", Gm, g, Gm).astype(np.float32).reshape(36, ntile, 2, 2, 16, kch, 4)   # [pos][tile][oh][ob][tx][chunk][c4]
        out[:, v] = u.transpose(1, 5, 0, 6, 2, 4, 3)
        lv = np.zeros((ntile * 64, kch * 4), dtype=bool)
        lv[:Cout, :Cin] = True
        live[:, v] = np.broadcast_to(lv.reshape(1, ntile, 2, 2, 16, kch, 4), (36, ntile, 2, 2, 16, kch, 4)).transpose(1, 5, 0, 6, 2, 4, 3)
    return out.reshape(-1), live.reshape(-1)


def _weights(shape, gen):
    """seeded: mantissa in [2^23, 2^24) coprime to 15, random sign, times 2^k, k uniform in -16 .. 16 (why: the module docstring)"""
    m = torch.randint(1 << 23, (1 << 24) - 15, shape, generator=gen)
    m = m - m % 15 + torch.tensor([1, 2, 4, 7, 8, 11, 13, 14])[torch.randint(0, 8, shape, generator=gen)]
    sign = 2 * torch.randint(0, 2, shape, generator=gen) - 1
    w = (m * sign).double() * torch.exp2((torch.randint(-16, 17, shape, generator=gen) - 23).double())
    assert torch.equal(w.float().double(), w)
    return w.float()


class _Built:
    pass


@pytest.fixture(scope="module")
def built():
    """Every case's packs, item and the cache a launch holding only that item builds (inside NaN guards); computed once, never modified."""
    from crdr_amd.hip import lib as L, ops
    lib = L.load()
    dev = torch.device("cuda:0")
    res = {}
    for i, case in enumerate(CASES):
        name, ci, co, hw, k, s, tr, G = case
        gen = torch.Generator().manual_seed(100 + i)
        shape = (ci, co, k, k) if tr else (co, ci, k, k)
        b = _Built()
        b.case, b.d = case, _desc(lib, case)
        b.packs = [ops.pack_weight(_weights(shape, gen).to(dev), transpose=bool(tr)) for _ in range(G)]
        assert b.packs[0].shape[1:] == (b.d.wrows, b.d.wcols)
        b.nbytes = int(lib.crdr_conv2d_filter_cache_bytes(C.byref(b.d), G))
        assert b.nbytes > 0 and b.nbytes % 16 == 0
        b.whole, b.u = _guarded(b.nbytes // 4, dev)
        b.item = _item(lib, b.d, G, b.packs, b.u)
        _rebuild(lib, [b.item], dev)
        res[name] = b
    return res


@pytest.mark.parametrize("name", IDS)
def test_cache_matches_float64(built, name):
    b = built[name]
    _, ci, co, _, k, _, _, G = b.case
    it = b.item
    nvar = it.nvar
    widx = [list(r) for r in it.widx]
    # the tap tables: every tap of the pack exactly once across the variants; the 5x5 forms leave 11 of their 36 entries at -1
    named = sorted(t for v in range(nvar) for t in widx[v] if t >= 0)
    assert named == list(range(k * k)), widx
    assert sum(t < 0 for v in range(nvar) for t in widx[v]) == 9 * nvar - k * k and nvar == (1 if k == 3 else 4)
    assert (it.kchunks, it.ntile, it.units) == ((ci + 3) // 4, (co + 63) // 64, G * it.ntile * nvar * ((it.kchunks + 7) // 8))
    got = b.u.cpu().numpy().reshape(G, -1)
    for g in range(G):
        exp, live = _expected(b.packs[g], widx, nvar, ci, co)
        assert got[g].shape == exp.shape
        assert np.all(got[g][~live] == 0.0), "padding entries must be exactly 0.0"
        assert not np.isnan(got[g]).any()
        diff = np.abs(got[g].astype(np.float64) - exp.astype(np.float64))
        ulp = np.spacing(np.maximum(np.abs(got[g]), np.abs(exp)))
        nneq = int((got[g] != exp).sum())
        print(f"{name}[{g}]: {got[g].size} elements, {nneq} unequal, max diff / ulp {float((diff / ulp).max()):.2f}")
        assert np.all(diff <= ulp), f"{name}: an element is more than 1 float32 ulp off"
        assert nneq <= 1e-5 * got[g].size, f"{name}: {nneq} of {got[g].size} elements unequal"


@pytest.mark.parametrize("name", IDS)
def test_nothing_left_nothing_outside(built, name):
    b = built[name]
    n = b.nbytes // 4
    whole = b.whole.cpu()
    assert not torch.isnan(whole[GUARD:GUARD + n]).any(), "a float of the cache was not written"
    assert torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[GUARD + n:]).all(), "a write outside the cache"


def test_one_launch_many_items(built):
    """All items in one launch, the smallest first and (a second cache of it) last: each equals the single-item launch's, byte for byte."""
    from crdr_amd.hip import lib as L
    lib = L.load()
    dev = torch.device("cuda:0")
    assert min(built.values(), key=lambda b: b.nbytes).case[0] == SMALLEST
    order = [SMALLEST] + [n for n in IDS if n != SMALLEST] + [SMALLEST]
    bufs, items = [], []
    for n in order:
        b = built[n]
        whole, u = _guarded(b.nbytes // 4, dev)
        bufs.append((whole, u))
        items.append(_item(lib, b.d, b.case[7], b.packs, u))
    _rebuild(lib, items, dev)
    for n, (whole, u) in zip(order, bufs):
        assert torch.equal(u.view(torch.int32), built[n].u.view(torch.int32)), n
        assert torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[GUARD + u.numel():]).all(), n


@pytest.mark.parametrize("name", IDS)
def test_in_launch_transform_agrees(built, name):
    """The cache a forced-F(4x4) conv launch leaves with filter_cache_valid = 0 == the batched rebuild's, byte for byte."""
    from crdr_amd.hip import lib as L, ops
    lib = L.load()
    dev = torch.device("cuda:0")
    b = built[name]
    d, G = b.d, b.case[7]
    gen = torch.Generator().manual_seed(7)
    xs = [torch.randn((d.N, d.H, d.W, d.C), generator=gen).to(dev) for _ in range(G)]
    ys = [torch.empty((d.N, d.OH, d.OW, d.OC), dtype=torch.float32, device=dev) for _ in range(G)]
    ios = (L.ConvIO * G)(*[L.ConvIO(x=xs[g].data_ptr(), w=b.packs[g].data_ptr(), y=ys[g].data_ptr()) for g in range(G)])
    nws = int(lib.crdr_conv2d_grouped_workspace(C.byref(d), G))
    ws, ws_n = ops.workspace(nws, dev, conv=True) if nws else (None, 0)
    whole, u = _guarded(b.nbytes // 4, dev)
    L.check(lib.crdr_conv2d_grouped_ex(C.byref(d), ios, G, ws, ws_n, u.data_ptr(), b.nbytes, 0, _stream()), "conv2d_grouped_ex")
    torch.cuda.synchronize()
    assert torch.equal(u.view(torch.int32), b.u.view(torch.int32))
    assert torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[GUARD + u.numel():]).all()
    assert all(bool(torch.isfinite(y).all()) for y in ys)
